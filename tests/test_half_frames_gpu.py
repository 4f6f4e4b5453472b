"""FLOAT16 / BFLOAT16 job slices over DPDK frames on the GPU
(sml_quantize_pack_frames_typed, sml_dequantize_frames_typed; the kernels of
sml_frames_half.hip) against the CPU oracle on the widened slice.

Recipe of test_half_gpu.py (the oracle does not know the 16-bit types):
x32 = x.float() on the CPU (exact); the expected frames are
O.build_frames(x32, ...), the expected outputs narrow(O.dequantize_frames(...).out, T).
Every comparison is bit-exact; a 16-bit output goes through assert_half_equal
(an expected NaN accepts any NaN, at least 99 % of the positions compared by
bits — the cases below have no NaN in their expected outputs at all).
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from switchml_amd import frame_wire as FW
from test_frames import rdma_imm_reference
from test_frames_rx import rx_stream, switch_return
from test_half_gpu import assert_half_equal, bits_of, from_bits, make, narrow, tdtype, x32_of

pytestmark = pytest.mark.gpu

TYPES = ("fp16", "bf16")
KINDS = ("normal", "special")
# (P, numel, W, batch_max)
CASES = [(64, 1, 1, 64),          # one element, one block
         (64, 777, 2, 8),
         (128, 4099, 8, 16),
         (256, 1027, 3, 2),       # partial last block of 3 elements, b < B, division path
         (256, 5000, 1, 4),
         (256, 4113, 8, 64),      # b = B: every tile takes the extra-batch branch
         (512, 3000, 3, 3),
         (1024, 9000, 3, 2),      # one packet per tile
         (1024, 2049, 1, 64)]     # ragged last block
JOB = 0x3C
SENT16 = 0x3C5A                   # a finite number in both types
SENT8 = 0xAB
CODE = {"fp16": 2, "bf16": 3}


def sw():
    import switchml_amd
    return switchml_amd


def params(job_id=JOB):
    return sw().frame_params(job_id=job_id, pool_index_start=16, pool_index_shift=3, max_outstanding_pkts=8)


@functools.lru_cache(maxsize=None)
def slice_of(kind, T, P, n):
    """(x of type T on the CPU, x32): one slice per case, shared by the tests."""
    x = make(kind, T, n, seed=P)
    x32 = x32_of(x)
    x32.setflags(write=False)
    return x, x32


@functools.lru_cache(maxsize=None)
def expected_frames(kind, T, P, n, W, bm, glob):
    """The oracle's frames of the widened slice, [B + b, frame bytes]; glob: global
    exponents one above the slice's own, returned with them."""
    _, x32 = slice_of(kind, T, P, n)
    ge = None
    if glob:
        ge = np.clip(O.exponents(x32, P).astype(np.int32) + 1, -128, 127).astype(np.int8)
    fr = O.build_frames(x32, params(), P=P, num_workers=W, batch_max=bm, global_exps=ge).reshape(-1, FW.frame_bytes(P))
    fr.setflags(write=False)
    return fr, ge


def in_buffer(x, off, cuda):
    """x as a slice at element offset `off` of a larger device buffer."""
    import torch
    buf = torch.zeros(x.numel() + off + 5, dtype=x.dtype, device=cuda)
    buf[off:off + x.numel()] = x.to(cuda)
    return buf[off:off + x.numel()]


def run_tx(cuda, kind, T, P, n, W, bm, glob, off, pad, where):
    import torch
    x, _ = slice_of(kind, T, P, n)
    exp, ge = expected_frames(kind, T, P, n, W, bm, glob)
    F, fb = exp.shape
    stride = fb + pad
    frames = torch.full((F * stride,), SENT8, dtype=torch.uint8)
    frames = frames.to(cuda) if where == "device" else frames.pin_memory()
    xd = in_buffer(x, off, cuda)
    assert xd.data_ptr() % 4 == (2 * off) % 4
    sw().quantize_pack_frames(xd, params(), P, W, batch_max=bm, frames=frames, stride=stride,
                              global_exps=None if ge is None else torch.from_numpy(ge).to(cuda))
    torch.cuda.synchronize()
    got = frames.cpu().numpy().reshape(F, stride)
    bad = np.argwhere(got[:, :fb] != exp)
    assert bad.size == 0, (len(bad), [tuple(int(v) for v in r) for r in bad[:8]])
    assert np.all(got[:, fb:] == SENT8)


# ----------------------------------------------------------------- tx --

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("P,n,W,bm", CASES)
def test_tx_frames_equal_the_oracles_frames_of_the_widened_slice(cuda, P, n, W, bm, T, kind):
    """Every byte of every frame, with and without global exponents; the slice
    at element offsets 0, 1 and 3 of a larger buffer; a padded stride whose pad
    bytes keep their sentinel; device and pinned host frames."""
    for glob in (False, True):
        for off, pad, where in ((0, 0, "device"), (1, 12, "device"), (3, 0, "device"), (1, 0, "pinned"),
                                (0, 60, "pinned")):
            run_tx(cuda, kind, T, P, n, W, bm, glob, off, pad, where)


# ----------------------------------------------------------------- rx --

@functools.lru_cache(maxsize=None)
def stream_of(kind, T, P, n, W, bm):
    """The frames a switch returns for the slice, in rx order with the
    anomalies of rx_stream."""
    _, x32 = slice_of(kind, T, P, n)
    frames, _ = rx_stream(x32, P, W, bm, job_id=JOB, seed=n + P)
    frames.setflags(write=False)
    return frames


def oracle_rx(frames, T, P, n, W, bm, cuts):
    ref = O.RxState(n, P, bm)
    for a, c in zip(cuts[:-1], cuts[1:]):
        O.dequantize_frames(frames[a:c], int(c - a), frames.shape[1], ref, W, job_id=JOB)
    return narrow(ref.out, T), ref.exps, ref.counts


def run_rx(cuda, frames, T, P, n, W, bm, off, calls, where="device"):
    """(output [n], the whole buffer's bits, exps, counts): the output lives at
    element offset `off` of a sentinel-filled 16-bit buffer."""
    import torch
    S = sw()
    F, stride = frames.shape
    t = torch.from_numpy(frames.reshape(-1).copy())
    t = t.to(cuda) if where == "device" else t.pin_memory()
    buf = from_bits(np.full(n + off + 7, SENT16, dtype=np.uint16), T).to(cuda)
    out = buf[off:off + n]
    rx = S.RxSlice(n, P, bm, device=cuda, out=out)
    assert rx.out.dtype == tdtype(T) and rx.out.data_ptr() == buf.data_ptr() + 2 * off
    cuts = np.linspace(0, F, calls + 1).astype(int)
    for a, c in zip(cuts[:-1], cuts[1:]):
        S.dequantize_frames(t[a * stride:c * stride], int(c - a), rx, num_workers=W, job_id=JOB, stride=stride)
    torch.cuda.synchronize()
    return out.cpu(), bits_of(buf), rx.exps.cpu().numpy(), [int(v) for v in rx.counts.cpu()], cuts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("P,n,W,bm", CASES)
def test_rx_equals_the_narrowed_oracle_output(cuda, P, n, W, bm, T, kind):
    """Shuffled windows, garbage duplicates, another job's frames, an
    out-of-range pkt_id: out, exps and counts; the output at element offsets
    0, 1 and 3 of a sentinel-filled buffer, whose other elements keep the
    sentinel; at offset 1 the stream is split over three calls."""
    frames = stream_of(kind, T, P, n, W, bm)
    for off, calls, where in ((0, 1, "device"), (1, 3, "device"), (3, 1, "pinned")):
        out, whole, exps, cnt, cuts = run_rx(cuda, frames, T, P, n, W, bm, off, min(calls, frames.shape[0]), where)
        want, want_exps, want_cnt = oracle_rx(frames, T, P, n, W, bm, cuts)
        assert_half_equal(out, want)
        assert np.array_equal(exps, want_exps)
        assert cnt == want_cnt
        assert np.all(whole[:off] == SENT16) and np.all(whole[off + n:] == SENT16)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("P,n,W,bm", [c for c in CASES if O.num_blocks(c[1], c[0]) >= 3])
def test_rx_blocks_without_a_payload_frame_keep_their_bytes(cuda, P, n, W, bm, T):
    """The payload frames of two blocks never arrive: those blocks keep the
    sentinel, everything else is exact."""
    kind = "special"
    frames = stream_of(kind, T, P, n, W, bm)
    B = O.num_blocks(n, P)
    b = min(B, bm)
    lost = (0, B - 1)                                        # the first block and the (partial) last one
    pid = FW.get(frames, FW.PKT_ID)
    mine = FW.get(frames, FW.JOB) == JOB
    keep = ~(mine & np.isin(pid, [k + b for k in lost]))
    frames = np.ascontiguousarray(frames[keep])
    out, whole, exps, cnt, cuts = run_rx(cuda, frames, T, P, n, W, bm, 1, 1)
    want, want_exps, want_cnt = oracle_rx(frames, T, P, n, W, bm, cuts)
    got_bits = bits_of(out)
    held = np.zeros(n, dtype=bool)
    for k in lost:
        held[k * P:min((k + 1) * P, n)] = True
    assert np.all(got_bits[held] == SENT16)
    assert_half_equal(out[~held], want[~held])
    assert np.array_equal(exps, want_exps)                   # the exponent frames did arrive
    assert cnt == want_cnt
    assert np.all(whole[:1] == SENT16) and np.all(whole[1 + n:] == SENT16)


# ------------------------------------- store policies, grid-stride path --

@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("thr", [0, 2 ** 64 - 1])
def test_both_store_policies_on_a_one_workgroup_grid(cuda, T, thr):
    """Non-temporal stores always (threshold 0) and never (UINT64_MAX), each
    on one workgroup, so that every wave strides over several tiles: the same
    bytes as the oracle's, hence as each other's."""
    S = sw()
    P, n, W, bm = 256, 5000, 1, 4
    thr0 = S.set_payload_nt_threshold(thr)
    grid0 = S.set_grid_limit(1)
    try:
        run_tx(cuda, "special", T, P, n, W, bm, False, 1, 12, "device")
        frames = stream_of("special", T, P, n, W, bm)
        out, whole, exps, cnt, cuts = run_rx(cuda, frames, T, P, n, W, bm, 3, 1)
        want, want_exps, want_cnt = oracle_rx(frames, T, P, n, W, bm, cuts)
        assert_half_equal(out, want)
        assert np.array_equal(exps, want_exps) and cnt == want_cnt
        assert np.all(whole[:3] == SENT16) and np.all(whole[3 + n:] == SENT16)
    finally:
        S.set_grid_limit(grid0)
        S.set_payload_nt_threshold(thr0)


# -------------------------------------------------------- cross-checks --

def test_typed_entry_points_with_float32_are_the_untyped_ones(cuda):
    import torch
    S = sw()
    L = S.lib()
    P, n, W, bm = 256, 4113, 3, 8
    x32 = O.splitmix_normal(3, n)
    xd = torch.from_numpy(x32).to(cuda)
    prm = params()
    B = O.num_blocks(n, P)
    F, stride = B + min(B, bm), FW.frame_bytes(P)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    fr = [torch.full((F * stride,), SENT8, dtype=torch.uint8, device=cuda) for _ in range(2)]
    assert L.sml_quantize_pack_frames(xd.data_ptr(), n, P, W, None, bm, ctypes.byref(prm), fr[0].data_ptr(), stride,
                                      st) == 0
    assert L.sml_quantize_pack_frames_typed(xd.data_ptr(), S.FLOAT32, n, P, W, None, bm, ctypes.byref(prm),
                                            fr[1].data_ptr(), stride, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(fr[0], fr[1])
    assert np.array_equal(fr[1].cpu().numpy(), O.build_frames(x32, prm, P=P, num_workers=W, batch_max=bm))
    frames, _ = rx_stream(x32, P, W, bm, job_id=JOB, seed=5)
    t = torch.from_numpy(frames.reshape(-1).copy()).to(cuda)
    rxs = [S.RxSlice(n, P, bm, device=cuda) for _ in range(2)]
    a = rxs[0]
    assert L.sml_dequantize_frames(t.data_ptr(), frames.shape[0], stride, n, P, W, bm, JOB, a.exps.data_ptr(),
                                   a.state.data_ptr(), a.out.data_ptr(), a.counts.data_ptr(), st) == 0
    a = rxs[1]
    assert L.sml_dequantize_frames_typed(t.data_ptr(), frames.shape[0], stride, n, P, W, bm, JOB, a.exps.data_ptr(),
                                         a.state.data_ptr(), a.out.data_ptr(), S.FLOAT32, a.counts.data_ptr(),
                                         st) == 0
    torch.cuda.synchronize()
    assert torch.equal(rxs[0].out.view(torch.int32), rxs[1].out.view(torch.int32))
    assert torch.equal(rxs[0].exps, rxs[1].exps) and torch.equal(rxs[0].counts, rxs[1].counts)
    assert torch.equal(rxs[0].state, rxs[1].state)
    ref = O.dequantize_frames(frames, frames.shape[0], stride, O.RxState(n, P, bm), W, job_id=JOB)
    assert np.array_equal(rxs[1].out.cpu().numpy().view(np.uint32), ref.out.view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TYPES)
def test_tx_switch_rx_equals_the_fused_16_bit_round_trip(cuda, T, kind):
    """Quantize into frames -> the switch (x W on the wire words, on the host)
    -> dequantize from frames == sml_roundtrip_loopback_typed on the slice."""
    import torch
    S = sw()
    P, n, W, bm = 256, 4113, 8, 64
    x, _ = slice_of(kind, T, P, n)
    xd = x.to(cuda)
    stride = S.frame_bytes(P)
    fr = S.quantize_pack_frames(xd, params(job_id=4), packet_numel=P, num_workers=W, batch_max=bm)
    torch.cuda.synchronize()
    ret = switch_return(fr.cpu().numpy(), stride, P, W)
    F = ret.shape[0]
    rx = S.RxSlice(n, P, bm, device=cuda, dtype=tdtype(T))
    S.dequantize_frames(torch.from_numpy(ret.reshape(-1).copy()).to(cuda), F, rx, num_workers=W, job_id=4)
    ref = S.roundtrip_loopback(xd, P, W)
    torch.cuda.synchronize()
    assert ref.dtype == tdtype(T)
    assert_half_equal(rx.out, ref.cpu())
    assert rx.counts.tolist() == [F, 0]


# ---------------------------------------------------------------- RDMA --

@pytest.mark.parametrize("T", TYPES)
def test_rdma_messages_of_a_16_bit_slice(cuda, T):
    """A 16-bit slice's RDMA messages need no code of their own: the P = 1024
    planes of sml_quantize_pack_typed are the message payloads and sml_rdma_imm
    on its exponent plane gives the immediates — those of the widened slice."""
    P, n, W, bm = 1024, 5003, 2, 3
    x, x32 = slice_of("special", T, P, n)
    payload, exps = sw().quantize_pack(x.to(cuda), P, W)
    assert np.array_equal(payload.cpu().numpy().view(np.uint32), O.quantize(x32, P, W))
    assert np.array_equal(exps.cpu().numpy(), O.exponents(x32, P))
    imm = sw().rdma_imm(exps, bm).cpu().numpy().view(np.uint32)
    assert np.array_equal(imm, rdma_imm_reference(O.exponents(x32, P), bm))
