"""Long RDMA messages on the GPU (sml_messages.hip): every comparison is
bit-exact against the CPU oracle at P = msg_numel (O.quantize_vcl / vcl=True
under FLAG_ROUND_RNE).  16-bit types by test_half_gpu.py's recipe: the oracle on
the widened input, torch's CPU narrow, its NaN rule.  Every typed buffer is a
view one element into its allocation, so every typed access is unaligned, and
the elements on both sides of an output must keep their sentinel."""
import numpy as np
import pytest

from oracle import oracle as O
from test_half_gpu import assert_half_equal, narrow, sw, words_equal

pytestmark = pytest.mark.gpu

# sub-slice, below a tile, tile-straddling, 2 waves, 3 (a workgroup below 256 threads), 4, 5 and 16 waves
MS = (192, 768, 1280, 2048, 2304, 4096, 4160, 16384)
NS = (lambda M: 1, lambda M: M - 1, lambda M: M, lambda M: M + 1, lambda M: 2 * M + 3, lambda M: 5 * M + M // 2 + 1)
SHAPES = [(M, f(M)) for M in MS for f in NS]
RNE, LE = 2, 1
# (type, W, flags): the pairs that differ in code path — division / exact reciprocal, rounding, byte order, element
PATHS = [("fp32", 1, 0), ("fp32", 3, RNE), ("fp32", 3, LE), ("fp16", 3, 0), ("bf16", 1, RNE)]


def dtype(T):
    import torch
    return {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[T]


def data(T, n, seed, sigma=1.0):
    """CPU tensor of type T and its exact fp32 widening."""
    import torch
    x = torch.from_numpy(O.splitmix_normal(seed, n, sigma)).to(dtype(T))
    return x, x.float().numpy()


def offset1(x, cuda, fill=None):
    """x (CPU) on the device as a view one element into a guarded allocation."""
    import torch
    buf = torch.full((x.numel() + 2,), 77.0, dtype=x.dtype, device=cuda)
    if fill is None:
        buf[1:-1].copy_(x)
    return buf, buf[1:-1]


def assert_out(buf, y32, T):
    """The view's elements equal y32 narrowed to T; the guards kept their value."""
    assert float(buf[0]) == 77.0 and float(buf[-1]) == 77.0, "a byte outside the slice was written"
    got = buf[1:-1].cpu()
    if T == "fp32":
        assert words_equal(got.numpy(), y32)
    else:
        assert_half_equal(got, narrow(y32, T))


def planes(x32, M, W, flags, global_exps=None):
    if flags & RNE and global_exps is None:
        pay, ex = O.quantize_vcl(x32, M, W)
    else:                       # under given exponents (O.quantize_vcl takes none) the RNE body is O.quantize's mode
        rounding = O.RNE_VCL if flags & RNE else O.HALF_AWAY
        pay, ex = O.quantize(x32, M, W, global_exps=global_exps, rounding=rounding), O.exponents(x32, M)
    return (pay.byteswap() if flags & LE else pay), ex


@pytest.mark.parametrize("T,W,flags", PATHS)
@pytest.mark.parametrize("M,n", SHAPES)
def test_k1_k2_k4(cuda, M, n, T, W, flags):
    import torch
    x, x32 = data(T, n, M + n)
    _, xd = offset1(x, cuda)
    pay, ex = planes(x32, M, W, flags)
    assert np.array_equal(sw().msg_exponents(xd, M).cpu().numpy(), ex)
    got_pay, got_ex = sw().msg_quantize_pack(xd, M, W, flags=flags)
    assert np.array_equal(got_ex.cpu().numpy(), ex) and words_equal(got_pay.cpu().numpy(), pay)
    # K4 on the switch's answer to W such workers (the payload x W, wrapping), exponents off 4-byte alignment
    agg = O.loopback_aggregate(pay.byteswap() if flags & LE else pay, W)
    y32 = O.dequantize(agg, ex, n, M, W)
    agg_d = torch.from_numpy((agg.byteswap() if flags & LE else agg).view(np.int32)).to(cuda)
    ex_d = torch.from_numpy(np.concatenate([[0], ex]).astype(np.int8)).to(cuda)[1:]
    buf, out = offset1(x, cuda, fill=False)
    sw().msg_dequantize(agg_d, ex_d, n, M, W, out=out, flags=flags & LE)
    assert_out(buf, y32, T)


@pytest.mark.parametrize("T,flags", [("fp32", 0), ("bf16", LE), ("fp32", RNE)])
@pytest.mark.parametrize("M,n", SHAPES)
def test_k3_global_exponents(cuda, M, n, T, flags):
    import torch
    xs = [data(T, n, 3 * M + n + w, sigma=4.0 ** w) for w in range(3)]
    ge = O.switch_exps([O.exponents(x32, M) for _, x32 in xs])
    pay, _ = planes(xs[0][1], M, 3, flags, global_exps=ge)
    got, _ = sw().msg_quantize_pack(offset1(xs[0][0], cuda)[1], M, 3, global_exps=torch.from_numpy(ge).to(cuda),
                                    flags=flags)
    assert words_equal(got.cpu().numpy(), pay)


@pytest.mark.parametrize("T,W,flags,inplace,want_planes", [
    ("fp32", 1, 0, True, True), ("fp32", 3, RNE, False, False), ("fp32", 4, LE, False, True),
    ("fp16", 3, 0, True, False), ("bf16", 2, RNE, False, True)])
@pytest.mark.parametrize("M,n", SHAPES)
def test_fused_round_trip(cuda, M, n, T, W, flags, inplace, want_planes):
    import torch
    x, x32 = data(T, n, 5 * M + n)
    y32 = O.dummy_allreduce(x32, P=M, num_worker_threads=1, num_workers=W, vcl=bool(flags & RNE))
    buf, xd = offset1(x, cuda)
    obuf, out = (buf, xd) if inplace else offset1(x, cuda, fill=False)
    B = -(-n // M)
    pl = torch.empty(B * M, dtype=torch.int32, device=cuda) if want_planes else None
    ex = torch.empty(B, dtype=torch.int8, device=cuda) if want_planes else None
    sw().msg_roundtrip_loopback(xd, M, W, out=out, payload=pl, exps_out=ex, flags=flags)
    assert_out(obuf, y32, T)
    if want_planes:
        pay, e = planes(x32, M, W, flags)
        assert np.array_equal(ex.cpu().numpy(), e) and words_equal(pl.cpu().numpy(), pay)


@pytest.mark.parametrize("pos", [0, 255, 256, 1023, 1024, -65, -1])
@pytest.mark.parametrize("M", [1280, 2304, 4096, 4160, 16384])
def test_cross_wave_maximum(cuda, M, pos):
    """One spike of 2^7 in message 1 of 3, wherever it lies in the message: its
    exponent must see it from every wave, and the neighbours' must not."""
    _, x32 = data("fp32", 3 * M, M, sigma=1e-3)
    x32[M + pos % M] = 128.0
    import torch
    pay, ex = planes(x32, M, 1, 0)
    assert ex[1] == 8 and ex[0] < 0 and ex[2] < 0
    got_pay, got_ex = sw().msg_quantize_pack(offset1(torch.from_numpy(x32), cuda)[1], M)
    assert got_ex.cpu().tolist() == ex.tolist() and words_equal(got_pay.cpu().numpy(), pay)


@pytest.mark.parametrize("T", ["fp32", "bf16"])
@pytest.mark.parametrize("M", [768, 2304, 4160, 16384])
def test_grid_stride_and_nontemporal_stores(cuda, M, T):
    """Two workgroups walk all the message groups (the prefetched loads, the LDS
    words alternating by loop trip) and every store takes the non-temporal form."""
    n, W = 9 * M + 5, 3
    x, x32 = data(T, n, M)
    pay, ex = planes(x32, M, W, 0)
    old = sw().set_grid_limit(2), sw().set_payload_nt_threshold(0)
    try:
        got_pay, got_ex = sw().msg_quantize_pack(offset1(x, cuda)[1], M, W)
        rbuf, rout = offset1(x, cuda, fill=False)
        sw().msg_roundtrip_loopback(offset1(x, cuda)[1], M, W, out=rout)
        kbuf, kout = offset1(x, cuda, fill=False)
        sw().msg_dequantize(got_pay, got_ex, n, M, W, out=kout)
    finally:
        sw().set_grid_limit(old[0])
        sw().set_payload_nt_threshold(old[1])
    assert np.array_equal(got_ex.cpu().numpy(), ex) and words_equal(got_pay.cpu().numpy(), pay)
    assert_out(rbuf, O.dummy_allreduce(x32, P=M, num_worker_threads=1, num_workers=W), T)
    assert_out(kbuf, O.dequantize(pay, ex, n, M, W), T)


def special_message(kind, M):
    x = O.splitmix_normal(9, M)
    if kind == "zeros":
        return np.zeros(M, np.float32)                                   # e = -126, payload 0
    if kind == "nan_inf":
        x[[3, 1500]] = np.nan, -np.inf
        return x
    if kind == "denormals":
        return (np.arange(M, dtype=np.uint32) * 4099 % (1 << 23) | (np.arange(M, dtype=np.uint32) & 1) << 31
                ).view(np.float32)
    return x * np.float32(2.0 ** -100)                                   # e <= -97: an infinite scale


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("kind", ["zeros", "nan_inf", "denormals", "tiny"])
def test_special_messages(cuda, kind, W):
    import torch
    M = 2048
    x32 = np.concatenate([O.splitmix_normal(1, M), special_message(kind, M), O.splitmix_normal(2, 700)])
    pay, ex = planes(x32, M, W, 0)
    if kind != "nan_inf":
        assert ex[1] == O.exponents(special_message(kind, M), M)[0] <= (-97 if kind == "tiny" else -126)
    got_pay, got_ex = sw().msg_quantize_pack(offset1(torch.from_numpy(x32), cuda)[1], M, W)
    assert np.array_equal(got_ex.cpu().numpy(), ex) and words_equal(got_pay.cpu().numpy(), pay)
    out = sw().msg_roundtrip_loopback(offset1(torch.from_numpy(x32), cuda)[1], M, W)
    assert words_equal(out.cpu().numpy(), O.dummy_allreduce(x32, P=M, num_worker_threads=1, num_workers=W))


@pytest.mark.parametrize("T", ["fp32", "bf16"])
@pytest.mark.parametrize("M", [256, 1024])
def test_equals_the_packet_kernels_at_packet_sizes(cuda, M, T):
    import torch
    xd = offset1(data(T, 5 * M + 77, M)[0], cuda)[1]
    for flags in (0, RNE):
        a, b = sw().quantize_pack(xd, M, 3, flags=flags), sw().msg_quantize_pack(xd, M, 3, flags=flags)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ya = sw().dequantize(a[0], a[1], xd.numel(), M, 3)
        assert torch.equal(ya.view(torch.int32), sw().msg_dequantize(b[0], b[1], xd.numel(), M, 3).view(torch.int32))
        assert torch.equal(sw().roundtrip_loopback(xd, M, 3, flags=flags).view(torch.int16),
                           sw().msg_roundtrip_loopback(xd, M, 3, flags=flags).view(torch.int16))


def test_composed_switch_step(cuda):
    """exponents -> switch_exps -> quantize with the global exponents -> the
    payload sum (block-size free) -> dequantize, W = 3 workers, M = 2304."""
    import torch
    M, W, n = 2304, 3, 2 * 2304 + 100
    xs = [O.splitmix_normal(40 + w, n, sigma=3.0 ** w) for w in range(W)]
    xd = [offset1(torch.from_numpy(x), cuda)[1] for x in xs]
    ge = sw().switch_exps([sw().msg_exponents(x, M) for x in xd])
    pls = [sw().msg_quantize_pack(x, M, W, global_exps=ge)[0] for x in xd]
    total = torch.empty_like(pls[0])
    sw().switch_aggregate(pls, packet_numel=64, payload_out=total)
    out = sw().msg_dequantize(total, ge, n, M, W)
    e, p = O.np_switch([O.exponents(x, M) for x in xs],
                       [O.quantize(x, M, W, global_exps=O.switch_exps([O.exponents(y, M) for y in xs])) for x in xs])
    assert np.array_equal(ge.cpu().numpy(), e) and words_equal(total.cpu().numpy(), p)
    assert words_equal(out.cpu().numpy(), O.dequantize(p, e, n, M, W))
