"""The plane kernels: K2 exponents, K1 / K3 quantize + pack, K4 dequantize, the
INT32 byte swap, the loopback switch K5 and the fused round trip, single and
batched; the scale table and the FIFO slice rule beside them."""
from __future__ import annotations

from .abi import SML_OK, SwitchMLError, TypedSlice, call, lib
from .glue import _dev, _float_type, _opt, _stream, _torch


def num_blocks(numel: int, packet_numel: int = 256) -> int:
    return int(lib().sml_num_blocks(numel, packet_numel))


def fifo_slice(numel: int, num_slices: int, t: int) -> tuple[int, int]:
    """(offset, numel) of slice t of a job split num_slices ways — the FIFO
    scheduler's rule (client_lib/src/schedulers/fifo_scheduler.cc:93-109):
    the first numel % num_slices slices get one extra element.  Used for the
    multi-GPU sharding mode (slice g -> GPU g, as worker thread g would get it)."""
    if num_slices <= 0 or not 0 <= t < num_slices:
        raise ValueError("need 0 <= t < num_slices")
    n, rem = divmod(numel, num_slices)
    return (t * (n + 1), n + 1) if t < rem else (t * n + rem, n)


def shard_quantize_pack(job, rank: int, world: int, packet_numel: int = 256, num_workers: int = 1,
                        flags: int = 0, stream=None):
    """Sharding mode: K1 over this rank's FIFO slice of `job` (a 1-D fp32
    device tensor holding the whole job).  Returns (offset, payload, exps);
    blocks restart at the slice start, exactly as for worker thread `rank`
    of `world` (ppp.cc:54-62 per slice)."""
    off, n = fifo_slice(job.numel(), world, rank)
    payload, exps = quantize_pack(job[off:off + n], packet_numel, num_workers, flags=flags, stream=stream)
    return off, payload, exps


def scale_lut(num_workers: int):
    import numpy as np
    out = np.empty(256, dtype=np.float32)
    call("sml_scale_lut", num_workers, out.ctypes.data)
    return out


def scale_lut_device(num_workers: int, device="cuda", stream=None):
    torch = _torch()
    out = torch.empty(256, dtype=torch.float32, device=device)
    call("sml_scale_lut_device", num_workers, _dev(out, torch.float32, "lut"), _stream(stream, out))
    return out


def exponents(x, packet_numel: int = 256, out=None, stream=None):
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    if out is None:
        out = torch.empty(B, dtype=torch.int8, device=x.device)
    dt = _float_type(x.dtype, "x")
    call("sml_exponents_typed", _dev(x, x.dtype, "x"), dt, x.numel(), packet_numel, _dev(out, torch.int8, "exps"),
         _stream(stream, x))
    return out


def quantize_pack(x, packet_numel: int = 256, num_workers: int = 1, global_exps=None,
                  payload=None, exps_out=None, want_exps: bool = True, flags: int = 0, stream=None):
    """Returns (payload int32[B*P] (BE words unless FLAG_PAYLOAD_LE), exps int8[B] or None).
    `x` is fp32, or fp16 / bf16 (widened inside the kernel: the planes are
    those of x.float())."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    if payload is None:
        payload = torch.empty(B * packet_numel, dtype=torch.int32, device=x.device)
    if global_exps is None and want_exps and exps_out is None:
        exps_out = torch.empty(B, dtype=torch.int8, device=x.device)
    g = _opt(global_exps, torch.int8, "global_exps")
    e = _opt(exps_out, torch.int8, "exps_out")
    dt = _float_type(x.dtype, "x")
    call("sml_quantize_pack_typed", _dev(x, x.dtype, "x"), dt, x.numel(), packet_numel, num_workers, g,
         _dev(payload, torch.int32, "payload"), e, flags, _stream(stream, x))
    return payload, (global_exps if global_exps is not None else exps_out)


def quantize_pack_launcher(x, packet_numel: int, num_workers: int, payload, exps_out=None, global_exps=None,
                           flags: int = 0, stream=None):
    """A zero-argument callable that launches sml_quantize_pack_typed on these
    tensors: every argument checked and converted once, so a loop over the
    same bucket (a training step's gradient bucket, the bench's steps) pays
    one C call per launch instead of the wrapper's tensor checks.  The
    tensors must stay alive while the callable is used."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    if payload.numel() != B * packet_numel:
        raise ValueError(f"payload must hold B*P = {B * packet_numel} words")
    if exps_out is not None and exps_out.numel() != B:
        raise ValueError(f"exps_out must hold B = {B} bytes")
    dt = _float_type(x.dtype, "x")
    args = (x.numel(), packet_numel, num_workers, _opt(global_exps, torch.int8, "global_exps"),
            _dev(payload, torch.int32, "payload"), _opt(exps_out, torch.int8, "exps_out"), flags, _stream(stream, x))
    fn, args = lib().sml_quantize_pack_typed, (_dev(x, x.dtype, "x"), dt) + args

    def launch():
        s = fn(*args)
        if s != SML_OK:
            raise SwitchMLError("sml_quantize_pack_typed", s)
    return launch


def dequantize(payload, exps, numel: int, packet_numel: int = 256, num_workers: int = 1,
               out=None, flags: int = 0, stream=None, out_dtype=None):
    """K4 into `out`, or into a new bucket of `out_dtype` (default fp32; fp16 /
    bf16: the fp32 result narrowed inside the kernel, round to nearest even)."""
    torch = _torch()
    if out is None:
        out = torch.empty(numel, dtype=out_dtype or torch.float32, device=payload.device)
    elif out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype {out_dtype}")
    dt = _float_type(out.dtype, "out")
    call("sml_dequantize_typed", _dev(payload, torch.int32, "payload"), _dev(exps, torch.int8, "exps"), numel,
         packet_numel, num_workers, _dev(out, out.dtype, "out"), dt, flags, _stream(stream, payload))
    return out


def bswap_i32(x, out=None, stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(x)
    call("sml_bswap_i32", _dev(x, torch.int32, "x"), _dev(out, torch.int32, "out"), x.numel(), _stream(stream, x))
    return out


def loopback_aggregate(payload, num_workers: int, flags: int = 0, stream=None):
    torch = _torch()
    call("sml_loopback_aggregate", _dev(payload, torch.int32, "payload"), payload.numel(), num_workers, flags,
         _stream(stream, payload))
    return payload


def roundtrip_loopback(x, packet_numel: int = 256, num_workers: int = 1, out=None,
                       payload=None, exps_out=None, flags: int = 0, stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(x)
    p = _opt(payload, torch.int32, "payload")
    e = _opt(exps_out, torch.int8, "exps_out")
    dt = _float_type(x.dtype, "x")   # the same type in and out
    call("sml_roundtrip_loopback_typed", _dev(x, x.dtype, "x"), _dev(out, x.dtype, "out"), dt, x.numel(),
         packet_numel, num_workers, p, e, flags, _stream(stream, x))
    return out


def roundtrip_loopback_batch(slices, packet_numel: int = 256, num_workers: int = 1, flags: int = 0, stream=None):
    """The fused round trip over several slices in one call: `slices` is a
    list of (x, out) device (or pinned host) tensor pairs, fp32, fp16 or bf16
    (a pair's two dtypes equal, the pairs' dtypes free); slice i gets exactly
    roundtrip_loopback(x_i, out=out_i) — its blocks start at its own first
    element.  The list goes whole through sml_roundtrip_loopback_batch_typed:
    one launch per dtype present (an all-fp32 list: the one launch of
    sml_roundtrip_loopback_batch)."""
    for x, o in slices:
        if x.numel() != o.numel():
            raise ValueError("slice in/out sizes differ")
        if getattr(x, "dtype", None) != getattr(o, "dtype", None):
            raise TypeError(f"slice in/out dtypes differ: {x.dtype}, {o.dtype}")
    st = _stream(stream, slices[0][0]) if slices else None
    arr = (TypedSlice * max(1, len(slices)))()
    for i, (x, o) in enumerate(slices):
        dt = _float_type(getattr(x, "dtype", None), "x")
        arr[i] = TypedSlice(_dev(x, x.dtype, "x").value, _dev(o, x.dtype, "out").value, x.numel(), dt, 0)
    call("sml_roundtrip_loopback_batch_typed", arr, len(slices), packet_numel, num_workers, flags, st)
