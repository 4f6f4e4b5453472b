"""FLOAT16 / BFLOAT16 job slices on the GPU: the kernels that read and write
16-bit elements themselves (sml_half.hip, the typed K6) against the CPU oracle
on the widened input.

Recipe (the oracle does not know the 16-bit types): x32 = x.float() computed
by torch on the CPU (exact); the expected planes are O.exponents(x32, P) and
O.quantize(x32, P, W[, global_exps]) (O.quantize_vcl under FLAG_ROUND_RNE);
the expected outputs are torch.from_numpy(y32).to(T) on the CPU (round to
nearest even), y32 from O.dequantize / O.dummy_allreduce / O.np_switch +
O.dequantize.

Every comparison is bit-exact on the raw 16-bit or 32-bit words.  The one
exception is the project's NaN rule (test_gpu_parity.py): where the expected
16-bit value is NaN the result must be a NaN, any payload.  Each comparison of
a 16-bit output asserts that at least 99 % of its positions were compared by
their bits.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

PS = (64, 128, 256, 512, 1024)
WS = (1, 3, 8)          # 3: the division path; 1, 8: the exact-reciprocal path
NS = (1, 3, 63, 64, 65, 255, 257, 1023, 1024, 1025, 2049, 4113, 100_003)
TYPES = ("fp16", "bf16")

# raw 16-bit patterns: (largest finite, +inf, NaN, most denormal bits, exponent
# of a block whose roundf ties are representable, mantissa bits incl. the implicit one)
SPEC = {"fp16": dict(max=0x7BFF, inf=0x7C00, nan=0x7E00, den=0x03FF, tie_e=8, mant=11),
        "bf16": dict(max=0x7F7F, inf=0x7F80, nan=0x7FC0, den=0x007F, tie_e=1, mant=8)}


def sw():
    import switchml_amd
    return switchml_amd


def tdtype(T):
    import torch
    return torch.float16 if T == "fp16" else torch.bfloat16


def from_bits(bits, T):
    """CPU tensor of type T from raw uint16 patterns."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(tdtype(T))


def bits_of(t):
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def narrow(y32, T):
    """The expected 16-bit output: torch's CPU narrow (round to nearest even)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(y32, dtype=np.float32)).to(tdtype(T))


def assert_half_equal(got, exp):
    """Bit-exact, except that an expected NaN accepts any NaN; at least 99 %
    of the positions are compared by bits."""
    import torch
    got = got.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape
    nan_e = torch.isnan(exp).numpy()
    nan_g = torch.isnan(got).numpy()
    assert nan_g[nan_e].all(), "expected NaN, got a number"
    by_bits = ~nan_e
    if by_bits.size:
        assert by_bits.mean() >= 0.99, f"only {by_bits.mean():.4f} of the positions compared by bits"
    g, e = bits_of(got)[by_bits], bits_of(exp)[by_bits]
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[0]}: got {g[bad[0]]:#06x}, expected {e[bad[0]]:#06x}"


def words_equal(got, exp):
    return np.array_equal(np.asarray(got).view(np.uint32), np.asarray(exp).view(np.uint32))


def host(t):
    return t.detach().cpu().numpy()


def normal(T, n, seed=0):
    """Normal data at the type's scale (N(0, 1) rounded to T)."""
    import torch
    return torch.from_numpy(O.splitmix_normal(seed + 7, n)).to(tdtype(T))


def special(T, n, seed=0):
    """Built in the 16-bit type: whole blocks of zeros, +-0, the type's
    denormals, its largest finite value, +-inf, NaN, and a run whose products
    are exact ties under roundf for power-of-two W: every 64th element is
    1.5 * 2^(e-1) (block exponent e), the rest odd multiples of 2^(e-32), so
    x * 2^(31-e) = m + 0.5."""
    s = SPEC[T]
    rng = np.random.default_rng(seed + 1)
    bits = bits_of(normal(T, n, seed + 100)).copy()
    k = max(n // 16, 1)
    sign = lambda m: (rng.integers(0, 2, size=m).astype(np.uint16) << 15)
    bits[0:k] = 0                                                     # blocks of zeros
    seg = bits[k:2 * k]
    seg[:] = sign(seg.size)                                           # +-0
    seg = bits[2 * k:3 * k]
    seg[:] = rng.integers(1, s["den"] + 1, size=seg.size).astype(np.uint16) | sign(seg.size)   # denormals
    seg = bits[3 * k:4 * k]
    seg[:] = np.uint16(s["max"]) | sign(seg.size)                     # largest finite
    tie = np.arange(bits[4 * k:5 * k].size)
    e = s["tie_e"]
    odd = 2 * (tie % (1 << (s["mant"] - 2))) + 1                      # fits the mantissa
    vals = np.where(tie % 64 == 0, 1.5 * 2.0 ** (e - 1), odd * 2.0 ** (e - 32) * np.where(tie % 2, -1.0, 1.0))
    tb = bits_of(narrow(vals.astype(np.float32), T))
    assert np.array_equal(from_bits(tb, T).float().numpy().astype(np.float64), vals)   # exactly representable
    bits[4 * k:5 * k] = tb
    if n > 8:
        bits[5 * k + 1] = s["nan"]
        bits[6 * k + 2] = s["inf"]
        bits[6 * k + 3] = s["inf"] | 0x8000
        bits[7 * k + 1] = 0x0001                                       # smallest denormal
        bits[7 * k + 2] = 0x8000 | s["den"]                            # largest denormal, negative
    return from_bits(bits, T)


def make(kind, T, n, seed=0):
    return normal(T, n, seed) if kind == "normal" else special(T, n, seed)


def x32_of(x):
    return x.float().numpy()


# ------------------------------------------------------------ K1h / K2h / K3h

@pytest.mark.parametrize("kind", ["normal", "special"])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("T", TYPES)
def test_k1h_k2h_planes_equal_oracle(cuda, T, P, W, kind):
    for n in NS:
        x = make(kind, T, n, seed=n)
        x32 = x32_of(x)
        xd = x.to(cuda)
        payload, exps = sw().quantize_pack(xd, P, W)
        assert np.array_equal(host(exps), O.exponents(x32, P)), (n, "K1h exponents")
        assert words_equal(host(payload), O.quantize(x32, P, W)), (n, "K1h payload")
        assert np.array_equal(host(sw().exponents(xd, P)), O.exponents(x32, P)), (n, "K2h")


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("T", TYPES)
def test_k3h_global_exponents_above_own(cuda, T, P, W):
    import torch
    for n in NS:
        x = make("special" if n % 2 else "normal", T, n, seed=n)
        x32 = x32_of(x)
        own = O.exponents(x32, P)
        ge = np.minimum(own.astype(np.int32) + 1 + np.arange(own.size) % 3, 127).astype(np.int8)
        payload, e = sw().quantize_pack(x.to(cuda), P, W, global_exps=torch.from_numpy(ge).to(cuda))
        assert words_equal(host(payload), O.quantize(x32, P, W, ge)), n
        assert np.array_equal(host(e), ge)


@pytest.mark.parametrize("kind", ["normal", "special"])
@pytest.mark.parametrize("T", TYPES)
def test_k1h_flags_le_and_rne(cuda, T, kind):
    P = 256
    for W in WS:
        for n in NS:
            x = make(kind, T, n, seed=n)
            x32 = x32_of(x)
            xd = x.to(cuda)
            le, _ = sw().quantize_pack(xd, P, W, flags=sw().FLAG_PAYLOAD_LE)
            assert words_equal(host(le), O.bswap32(O.quantize(x32, P, W))), (W, n, "LE")
            rne, e = sw().quantize_pack(xd, P, W, flags=sw().FLAG_ROUND_RNE)
            vp_, ve = O.quantize_vcl(x32, P, W)
            assert words_equal(host(rne), vp_) and np.array_equal(host(e), ve), (W, n, "RNE")


@pytest.mark.parametrize("T", TYPES)
def test_quantize_pack_launcher_takes_16_bit_inputs(cuda, T):
    import torch
    P, W, n = 256, 3, 4113
    x = make("special", T, n)
    xd = x.to(cuda)
    B = O.num_blocks(n, P)
    payload = torch.zeros(B * P, dtype=torch.int32, device=cuda)
    exps = torch.zeros(B, dtype=torch.int8, device=cuda)
    sw().quantize_pack_launcher(xd, P, W, payload, exps_out=exps)()
    assert words_equal(host(payload), O.quantize(x32_of(x), P, W)) and np.array_equal(host(exps), O.exponents(x32_of(x), P))


# ------------------------------------------------------------------- K4h

@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("T", TYPES)
def test_k4h_equals_oracle_on_its_payload(cuda, T, P, W):
    import torch
    for n in NS:
        x32 = x32_of(make("special" if n % 2 else "normal", T, n, seed=n))
        exps = O.exponents(x32, P)
        payload = O.loopback_aggregate(O.quantize(x32, P, W), W)
        exp = narrow(O.dequantize(payload, exps, n, P, W), T)
        got = sw().dequantize(torch.from_numpy(payload.view(np.int32)).to(cuda), torch.from_numpy(exps).to(cuda),
                              n, P, W, out_dtype=tdtype(T))
        assert_half_equal(got, exp)
        le = sw().dequantize(torch.from_numpy(O.bswap32(payload).view(np.int32)).to(cuda),
                             torch.from_numpy(exps).to(cuda), n, P, W, out_dtype=tdtype(T),
                             flags=sw().FLAG_PAYLOAD_LE)
        assert_half_equal(le, exp)


def k4h_case(cuda, T, q, e, P, W):
    """K4h on explicit host-order words q and one exponent for every block."""
    import torch
    n = q.size
    B = O.num_blocks(n, P)
    words = np.zeros(B * P, dtype=np.int32)
    words[:n] = q
    payload = O.bswap32(words)
    exps = np.full(B, e, dtype=np.int8)
    y32 = O.dequantize(payload, exps, n, P, W)
    got = sw().dequantize(torch.from_numpy(payload.view(np.int32)).to(cuda), torch.from_numpy(exps).to(cuda), n, P, W,
                          out_dtype=tdtype(T))
    assert_half_equal(got, narrow(y32, T))
    return y32, got.cpu()


@pytest.mark.parametrize("P", PS)
def test_k4h_fp16_overflows_to_inf(cuda, P):
    import torch
    rng = np.random.default_rng(5)
    q = rng.integers(-2 ** 31, 2 ** 31, size=4113, dtype=np.int64).astype(np.int32)
    y32, got = k4h_case(cuda, "fp16", q, 20, P, 1)      # |y| up to 2^20, fp16 ends at 65504
    assert np.isfinite(y32).all() and torch.isinf(got).float().mean() > 0.5 and torch.isfinite(got).any()


@pytest.mark.parametrize("P", PS)
def test_k4h_fp16_lands_in_denormal_range(cuda, P):
    rng = np.random.default_rng(6)
    q = rng.integers(-2 ** 31, 2 ** 31, size=4113, dtype=np.int64).astype(np.int32)
    y32, got = k4h_case(cuda, "fp16", q, -16, P, 1)     # |y| < 2^-16, fp16 normals start at 2^-14
    b = bits_of(got)
    assert ((b & 0x7C00) == 0).all() and ((b & 0x03FF) != 0).mean() > 0.9   # denormals, not flushed to zero


@pytest.mark.parametrize("W", (1, 2, 3))
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("T", TYPES)
def test_k4h_keeps_the_sign_of_zero(cuda, T, P, W):
    """Exponent -128: the scale is +inf, so every output is a zero with the
    sign of its word (q / inf), through the division (W = 3) and through the
    exact reciprocal (W = 1, 2: q * 0), whose fp32 multiply must not be fused
    into the fp16 conversion (an fma with a +0 addend gives +0 for -0)."""
    rng = np.random.default_rng(8)
    q = rng.integers(-2 ** 31, 2 ** 31, size=4113, dtype=np.int64).astype(np.int32)
    q[:8] = (-1, 1, 0, -2 ** 31, -1, -1, -1, -1)
    y32, got = k4h_case(cuda, T, q, -128, P, W)
    assert (y32 == 0).all() and np.array_equal(np.signbit(y32), q < 0)
    assert np.array_equal(bits_of(got), np.where(q < 0, 0x8000, 0).astype(np.uint16))


@pytest.mark.parametrize("P", PS)
def test_k4h_bf16_exact_rne_ties(cuda, P):
    i = np.arange(4113)
    q = (((128 + i % 128) << 16) | 0x8000).astype(np.int32) * np.where(i % 3 == 0, -1, 1).astype(np.int32)
    y32, got = k4h_case(cuda, "bf16", q, 0, P, 1)       # y = q * 2^-31: the dropped 16 bits are 0x8000
    assert ((y32.view(np.uint32) & 0xFFFF) == 0x8000).all()
    assert (bits_of(got) & 1 == 0).all()                # ties went to the even neighbour


# ------------------------------------------------------------- round trip

@pytest.mark.parametrize("kind", ["normal", "special"])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("T", TYPES)
def test_roundtrip_h_equals_oracle_loop_and_k1h_k5_k4h(cuda, T, P, W, kind):
    import torch
    for n in NS:
        x = make(kind, T, n, seed=n)
        x32 = x32_of(x)
        xd = x.to(cuda)
        B = O.num_blocks(n, P)
        # one FIFO slice: the packet loop of one worker thread over the whole job
        exp = narrow(O.dummy_allreduce(x32, P=P, max_outstanding_packets=64, num_worker_threads=1, num_workers=W), T)
        plane = torch.empty(B * P, dtype=torch.int32, device=cuda)
        eplane = torch.empty(B, dtype=torch.int8, device=cuda)
        got = sw().roundtrip_loopback(xd, P, W, payload=plane, exps_out=eplane)
        assert_half_equal(got, exp)
        assert_half_equal(sw().roundtrip_loopback(xd, P, W), exp)          # without the planes
        # the planes as sent, and the three-kernel pipeline bit for bit
        payload, exps = sw().quantize_pack(xd, P, W)
        assert torch.equal(plane, payload) and torch.equal(eplane, exps), n
        sw().loopback_aggregate(payload, W)
        three = sw().dequantize(payload, exps, n, P, W, out_dtype=tdtype(T))
        assert np.array_equal(bits_of(got), bits_of(three)), n
        # in == out
        y = xd.clone()
        assert sw().roundtrip_loopback(y, P, W, out=y) is y
        assert np.array_equal(bits_of(y), bits_of(got)), n


@pytest.mark.parametrize("T", TYPES)
def test_roundtrip_h_rne(cuda, T):
    for n in NS:
        x = make("special", T, n, seed=n)
        exp = narrow(O.dummy_allreduce(x32_of(x), P=256, max_outstanding_packets=64, num_worker_threads=1,
                                       num_workers=3, vcl=True), T)
        assert_half_equal(sw().roundtrip_loopback(x.to(cuda), 256, 3, flags=sw().FLAG_ROUND_RNE), exp)


# --------------------------------------------------------------- alignment

SENTINEL = 0x5A5A


@pytest.mark.parametrize("exact_end", [False, True])
@pytest.mark.parametrize("off", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("T", TYPES)
def test_misaligned_slices(cuda, T, off, exact_end):
    """Slices at element offsets that are not 8-byte aligned, for input and
    output; exact_end: the slice ends where its tensor (allocated at that
    size) ends.  Nothing outside the output slice changes."""
    import torch
    P, W = 256, 3
    n = 50_000 + off
    pad = 0 if exact_end else 9
    x = make("special", T, n, seed=off)
    x32 = x32_of(x)
    big_in = from_bits(np.full(off + n + pad, SENTINEL, np.uint16), T).to(cuda)
    big_in[off:off + n] = x.to(cuda)
    xin = big_in[off:off + n]
    assert xin.data_ptr() % 8 == (2 * off) % 8

    def fresh_out():
        return from_bits(np.full(off + n + pad, SENTINEL, np.uint16), T).to(cuda)

    def sentinels_kept(big):
        b = bits_of(big)
        return (b[:off] == SENTINEL).all() and (b[off + n:] == SENTINEL).all()

    payload, exps = sw().quantize_pack(xin, P, W)
    assert np.array_equal(host(exps), O.exponents(x32, P))
    assert words_equal(host(payload), O.quantize(x32, P, W))
    assert np.array_equal(host(sw().exponents(xin, P)), O.exponents(x32, P))

    sw().loopback_aggregate(payload, W)
    exp = narrow(O.dummy_allreduce(x32, P=P, max_outstanding_packets=64, num_worker_threads=1, num_workers=W), T)
    big = fresh_out()
    sw().dequantize(payload, exps, n, P, W, out=big[off:off + n])
    assert_half_equal(big[off:off + n], exp)
    assert sentinels_kept(big)

    big = fresh_out()
    sw().roundtrip_loopback(xin, P, W, out=big[off:off + n])
    assert_half_equal(big[off:off + n], exp)
    assert sentinels_kept(big)

    sw().roundtrip_loopback(xin, P, W, out=xin)          # in place, misaligned
    assert_half_equal(xin, exp)
    assert sentinels_kept(big_in)

    planes = [payload, payload]
    big = fresh_out()
    sw().switch_aggregate(planes, [exps, exps], n, P, out=big[off:off + n])
    e, p = O.np_switch([host(exps)] * 2, [host(payload).view(np.uint32)] * 2)
    assert_half_equal(big[off:off + n], narrow(O.dequantize(p, e, n, P, 2), T))
    assert sentinels_kept(big)


# ------------------------------------------------------------ store policy

@pytest.mark.parametrize("threshold", [0, None])
@pytest.mark.parametrize("T", TYPES)
def test_both_store_policies(cuda, T, threshold):
    """set_payload_nt_threshold(0): every payload plane and 16-bit output is
    written with non-temporal stores; None: the default (these sizes: default
    policy).  Same bits."""
    import torch
    prev = sw().set_payload_nt_threshold(threshold) if threshold is not None else None
    try:
        for P in PS:
            for n in (1, 255, 1025, 4113, 100_003):
                x = make("special", T, n, seed=n)
                x32 = x32_of(x)
                xd = x.to(cuda)
                payload, exps = sw().quantize_pack(xd, P, 3)
                assert words_equal(host(payload), O.quantize(x32, P, 3)), (P, n)
                exp = narrow(O.dummy_allreduce(x32, P=P, max_outstanding_packets=64, num_worker_threads=1,
                                               num_workers=3), T)
                assert_half_equal(sw().roundtrip_loopback(xd, P, 3), exp)
                sw().loopback_aggregate(payload, 3)
                assert_half_equal(sw().dequantize(payload, exps, n, P, 3, out_dtype=tdtype(T)), exp)
    finally:
        if prev is not None:
            sw().set_payload_nt_threshold(prev)


# -------------------------------------------------------------- K6 typed

@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("T", TYPES)
def test_k6_typed_output(cuda, T, P, W):
    import torch
    for n in NS:
        xs = [make("special" if w == 0 else "normal", T, n, seed=n + 31 * w) for w in range(W)]
        planes = [sw().quantize_pack(x.to(cuda), P, W) for x in xs]
        pl, ex = [p for p, _ in planes], [e for _, e in planes]
        e, p = O.np_switch([host(t) for t in ex], [host(t).view(np.uint32) for t in pl])
        exp = narrow(O.dequantize(p, e, n, P, W), T)
        got = sw().switch_aggregate(pl, ex, n, P, out_dtype=tdtype(T))
        assert got.dtype == tdtype(T)
        assert_half_equal(got, exp)
        # with the aggregated planes written as well, and little-endian words
        pout = torch.empty_like(pl[0])
        eout = torch.empty_like(ex[0])
        got = sw().switch_aggregate(pl, ex, n, P, payload_out=pout, exps_out=eout, out_dtype=tdtype(T))
        assert_half_equal(got, exp)
        assert words_equal(host(pout), p) and np.array_equal(host(eout), e)
        le = [torch.from_numpy(O.bswap32(host(t)).view(np.int32)).to(cuda) for t in pl]
        got = sw().switch_aggregate(le, ex, n, P, payload_out=pout, out_dtype=tdtype(T), flags=sw().FLAG_PAYLOAD_LE)
        assert_half_equal(got, exp)
        assert words_equal(host(pout), O.bswap32(p))


# ------------------------------------------- typed entry points with fp32

def test_typed_entry_points_with_fp32_equal_untyped(cuda):
    import torch
    L = sw().lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for P, W, n in ((64, 3, 100_003), (256, 8, 4113), (1024, 1, 1025)):
        x = torch.from_numpy(O.splitmix_normal(n, n)).to(cuda)
        B = O.num_blocks(n, P)
        payload, exps = sw().quantize_pack(x, P, W)
        tp = torch.zeros_like(payload)
        te = torch.zeros_like(exps)
        assert L.sml_quantize_pack_typed(vp(x), 0, n, P, W, None, vp(tp), vp(te), 0, st) == 0
        assert torch.equal(tp, payload) and torch.equal(te, exps)
        te.zero_()
        assert L.sml_exponents_typed(vp(x), 0, n, P, vp(te), st) == 0
        assert torch.equal(te, exps)
        out = sw().dequantize(payload, exps, n, P, W)
        to = torch.zeros_like(out)
        assert L.sml_dequantize_typed(vp(payload), vp(exps), n, P, W, vp(to), 0, 0, st) == 0
        assert torch.equal(to.view(torch.int32), out.view(torch.int32))
        rt = sw().roundtrip_loopback(x, P, W)
        to.zero_()
        assert L.sml_roundtrip_loopback_typed(vp(x), vp(to), 0, n, P, W, None, None, 0, st) == 0
        assert torch.equal(to.view(torch.int32), rt.view(torch.int32))
        agg = sw().switch_aggregate([payload, payload], [exps, exps], n, P)
        to.zero_()
        pp = (ctypes.c_void_p * 2)(payload.data_ptr(), payload.data_ptr())
        ep = (ctypes.c_void_p * 2)(exps.data_ptr(), exps.data_ptr())
        assert L.sml_switch_aggregate_typed(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ep, ctypes.c_void_p), 2, n,
                                            P, None, None, vp(to), 0, 0, st) == 0
        assert torch.equal(to.view(torch.int32), agg.view(torch.int32))
        assert B == exps.numel()
        # INT32 is not a typed float bucket
        assert L.sml_quantize_pack_typed(vp(x), 1, n, P, W, None, vp(tp), vp(te), 0, st) == sw().SML_ERR_UNSUPPORTED


def test_burst_with_a_16_bit_type_is_unsupported(cuda):
    """The burst entry points know FLOAT32 and INT32 only: data_type 2 / 3 is
    refused, never run as INT32."""
    import torch
    P = 256
    x = torch.ones(4 * P, dtype=torch.float16, device=cuda)
    ring = torch.zeros(P, dtype=torch.int32, device=cuda)
    extra = torch.zeros(2, dtype=torch.uint8, device=cuda)
    recv = torch.zeros(4, dtype=torch.int8, device=cuda)
    before = x.clone()
    for dt in (2, 3):
        b = sw().packet_burst(x, x, P, 1, 1, recv, [0], [ring.data_ptr()], [extra.data_ptr()])
        b.data_type = dt
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for fn in (sw().lib().sml_preprocess_burst, sw().lib().sml_postprocess_burst, sw().lib().sml_exchange_burst):
            assert fn(ctypes.byref(b), st) == sw().SML_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(x, before) and not ring.any()
