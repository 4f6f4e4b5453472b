"""The in-node switch: K6 over W workers' planes, its exponent half, the word
and segment copies of its all-gather / multicast, the uint8 widen / narrow of
the CollNet plugin's buckets, and the writer's release to peer GPUs."""
from __future__ import annotations

import ctypes

from .abi import FLOAT32, INT32, MAX_SWITCH_WORKERS, call
from .glue import _dev, _float_type, _opt, _ptr_table, _stream, _torch
from .planes import num_blocks


def _worker_count(planes) -> int:
    W = len(planes)
    if W == 0 or W > MAX_SWITCH_WORKERS:
        raise ValueError(f"1 <= workers <= {MAX_SWITCH_WORKERS}, got {W}")
    return W


def switch_aggregate(payloads, exps=None, numel: int | None = None, packet_numel: int = 256,
                     payload_out=None, exps_out=None, out=None, flags: int = 0, stream=None, out_dtype=None):
    """K6: the switch's per-slot aggregation over W worker planes, fused with
    the dequantize (p4/processor.p4:48-54 wrapping bit<32> sum,
    p4/exponents.p4:48-54 signed int8 max, then PostprocessSingle with
    scale(W, e_max), ppp.cc:197-251).  `payloads`: W int32 planes of B*P
    words (BE unless FLAG_PAYLOAD_LE); `exps`: W int8 planes of B bytes.
    Writes whichever of payload_out / exps_out / out is given; with none
    given, returns a new bucket `out` of `numel` elements of `out_dtype`
    (default fp32; fp16 / bf16, or a typed `out`: narrowed inside the kernel)."""
    torch = _torch()
    W = _worker_count(payloads)
    n_words = payloads[0].numel()
    if any(p.numel() != n_words for p in payloads):
        raise ValueError("payload planes differ in size")
    if numel is None:
        numel = n_words
    B = num_blocks(numel, packet_numel)
    if B * packet_numel != n_words:
        raise ValueError(f"payload planes hold {n_words} words, B*P = {B * packet_numel}")
    if exps is not None:
        if len(exps) != W or any(e.numel() != B for e in exps):
            raise ValueError("need one exponent plane of B bytes per payload plane")
    if out is None and (out_dtype is not None or (payload_out is None and exps_out is None)):
        out = torch.empty(numel, dtype=out_dtype or torch.float32, device=payloads[0].device)
    elif out is not None and out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype {out_dtype}")
    dt = FLOAT32 if out is None else _float_type(out.dtype, "out")
    # planes are int32 tensors, or (peer-to-peer switch) mapped peer planes
    # exposing data_ptr()/numel() only
    pp = _ptr_table(payloads, torch.int32, "payloads[w]", raw=True)
    ep = None if exps is None else _ptr_table(exps, torch.int8, "exps[w]")
    call("sml_switch_aggregate_typed", pp, ep, W, numel, packet_numel,
         _opt(payload_out, torch.int32, "payload_out"), _opt(exps_out, torch.int8, "exps_out"),
         None if out is None else _dev(out, out.dtype, "out"), dt, flags, _stream(stream, payloads[0]))
    return out


def switch_exps(exps, out=None, flags: int = 0, stream=None):
    """sml_switch_exps: the switch's exponent half alone, out[k] = the signed
    int8 max over the W planes `exps` (int8, equal length) of byte k
    (p4/exponents.p4:48-54).  The planes and `out` may sit at any byte
    alignment.  flags = FLAG_PEER_PLANES when planes were written by other
    GPUs.  Returns `out`."""
    torch = _torch()
    W = _worker_count(exps)
    B = exps[0].numel()
    if any(e.numel() != B for e in exps):
        raise ValueError("exponent planes differ in size")
    if out is None:
        out = torch.empty(B, dtype=torch.int8, device=exps[0].device)
    elif out.numel() != B:
        raise ValueError(f"out must hold B = {B} bytes")
    call("sml_switch_exps", _ptr_table(exps, torch.int8, "exps[w]"), W, B, _dev(out, torch.int8, "out"), flags,
         _stream(stream, exps[0]))
    return out


def copy_words(src, dst, stream=None):
    """sml_copy_words: `src` copied into `dst`, 32-bit tensors of equal numel
    (any 32-bit dtypes, any 4-byte alignment; CUDA or pinned host).  Returns
    `dst`."""
    if src.numel() != dst.numel() or src.element_size() != 4 or dst.element_size() != 4:
        raise ValueError("src and dst are 32-bit tensors of equal numel")
    call("sml_copy_words", _dev(src, src.dtype, "src"), _dev(dst, dst.dtype, "dst"), src.numel(),
         _stream(stream, src))
    return dst


def _resize(x, out, out_dtype, entry: str, in_dtype, stream):
    """widen / narrow: one element of `out` (a new tensor of out_dtype unless
    given) per element of `x`."""
    torch = _torch()
    if out is None:
        out = torch.empty(x.numel(), dtype=out_dtype, device=x.device)
    elif out.numel() != x.numel():
        raise ValueError("x and out differ in numel")
    call(entry, _dev(x, in_dtype, "x"), _dev(out, out_dtype, "out"), x.numel(), _stream(stream, x))
    return out


def widen_u8_i32(x, out=None, stream=None):
    """sml_widen_u8_i32: each uint8 of `x` zero-extended into an int32 (the
    CollNet plugin's ncclUint8 buckets on their way into the INT32
    all-reduce).  `x` may start at any byte.  Returns `out`."""
    torch = _torch()
    return _resize(x, out, torch.int32, "sml_widen_u8_i32", torch.uint8, stream)


def narrow_i32_u8(x, out=None, stream=None):
    """sml_narrow_i32_u8: the low byte of each int32 of `x` (the sum mod 256),
    back into a uint8 bucket at any byte.  Returns `out`."""
    torch = _torch()
    return _resize(x, out, torch.uint8, "sml_narrow_i32_u8", torch.int32, stream)


def _segment_tables(pairs, dtype=None):
    """The three tables of a segment copy — sources, destinations, element
    counts — from (src, dst) tensor pairs of equal numel, all of `dtype`
    (None: any 32-bit dtypes, each tensor its own)."""
    k = len(pairs)
    srcs = (ctypes.c_void_p * max(1, k))()
    dsts = (ctypes.c_void_p * max(1, k))()
    numel = (ctypes.c_uint64 * max(1, k))()
    for i, (s, d) in enumerate(pairs):
        if s.numel() != d.numel() or (dtype is None and (s.element_size() != 4 or d.element_size() != 4)):
            raise ValueError("segments are pairs of equal-size " + ("32-bit tensors" if dtype is None else "tensors"))
        srcs[i] = _dev(s, dtype or s.dtype, "src").value
        dsts[i] = _dev(d, dtype or d.dtype, "dst").value
        numel[i] = s.numel()
    return srcs, dsts, numel


def copy_segments(pairs, flags: int = 0, stream=None):
    """sml_copy_segments: every (src, dst) pair of 32-bit tensors (same
    numel; CUDA or pinned host) copied in ONE launch, the tiles dealt
    round-robin over the pairs (the in-node switch's multicast).
    flags = FLAG_PEER_PLANES when sources were written by other GPUs."""
    if len(pairs) > MAX_SWITCH_WORKERS:
        raise ValueError(f"at most {MAX_SWITCH_WORKERS} segments")
    call("sml_copy_segments", *_segment_tables(pairs), len(pairs), flags,
         _stream(stream, pairs[0][0] if pairs else None))


def copy_segments_typed(pairs, flags: int = 0, stream=None):
    """sml_copy_segments_typed: every (src, dst) pair of tensors of one dtype
    (same numel; CUDA or pinned host) copied in ONE launch.  float16 /
    bfloat16 pairs may start at any element (views at odd offsets) and hold
    an odd number of elements; float32 / int32 pairs go to sml_copy_segments'
    kernel.  The in-node switch's multicast of a job of that type."""
    torch = _torch()
    if len(pairs) > MAX_SWITCH_WORKERS:
        raise ValueError(f"at most {MAX_SWITCH_WORKERS} segments")
    dtypes = {t.dtype for pair in pairs for t in pair}
    if len(dtypes) > 1:
        raise TypeError(f"segments are tensors of one dtype, got {sorted(map(str, dtypes))}")
    dtype = dtypes.pop() if dtypes else torch.float32
    dt = INT32 if dtype == torch.int32 else _float_type(dtype, "segments")
    call("sml_copy_segments_typed", *_segment_tables(pairs, dtype), len(pairs), dt, flags,
         _stream(stream, pairs[0][0] if pairs else None))


def release_to_peers(stream=None, device=None):
    """sml_release_to_peers: system-scope release on every XCD after the work
    on `stream` (the writer's half of a hand-off to other GPUs)."""
    if stream is None:
        stream = _torch().cuda.current_stream(device)
    call("sml_release_to_peers", _stream(stream))
