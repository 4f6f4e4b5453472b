"""GPU: the in-node switch's kernels (csrc/sml_switch.hip) called directly, on
arbitrary planes and at the offsets the switch backend gives them, against
the oracle bit for bit.

The other switch tests feed K6 planes that O.quantize made (the sum of W
words fits, the tail past numel is zero) and exponent planes whose maximum is
plane 0 and positive.  Here the payload planes are uniformly random 32-bit
words, tail included, so every sum wraps; the exponent maximum is any int8,
held by any worker (a kernel that returned plane 0, or compared the bytes
unsigned, differs in a large share of the blocks); and some sums are exactly
0, so 0 / 0 occurs.  sml_switch_exps, sml_copy_words, sml_widen_u8_i32 and
sml_narrow_i32_u8 are called on their own, on both of their paths.

Expectations come from O.switch_exps / O.switch_payload / O.dequantize (or the
source bytes of a copy).  Every comparison is bit-exact; the one exception is
the project's NaN rule (test_gpu_parity.py): where the oracle's fp32 output
is NaN, any NaN is accepted.  Every output buffer has GUARD sentinel elements
on both sides of the span the call may write, checked after each call.

The standard shape is test_dispatch_axes_gpu.py's n = 4 * 1024 + P + 3: four
full tiles of 1024 elements, a partial packet and a ragged tail.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from test_gpu_parity import float_bits_equal_nan_ok  # noqa: E402
from test_half_gpu import assert_half_equal, narrow, tdtype  # noqa: E402
from test_launch_geometry import GEOMETRIES  # noqa: E402

PACKETS = (64, 128, 256, 512, 1024)
GUARD = 64                        # elements; a multiple of 16 bytes for every element size
SENT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}
FORCED_TOPS = (-128, 127, -1, 0)  # the maxima of blocks 0..3
GROUP = 16 * 1024                 # elements of a copy_segments group (kSegGroup tiles of 1024)


def size(P):
    return 4 * 1024 + P + 3


@pytest.fixture
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    yield switchml_amd
    switchml_amd.set_grid_limit(0)
    switchml_amd.set_xcd_chunk(64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------- the input builder --

@functools.lru_cache(maxsize=None)
def arbitrary_exps(W, B, seed):
    """W exponent planes of B bytes.  Per block the maximum `top` is uniform
    in [-128, 127] (blocks 0..3: -128, 127, -1, 0) and belongs to a worker
    drawn uniformly; every other worker's byte is min(top, a fresh draw)."""
    rng = np.random.default_rng([seed, W, B])
    top = rng.integers(-128, 128, size=B).astype(np.int16)
    k = min(B, len(FORCED_TOPS))
    top[:k] = FORCED_TOPS[:k]
    winner = rng.integers(0, W, size=B)
    planes = []
    for w in range(W):
        e = np.minimum(top, rng.integers(-128, 128, size=B).astype(np.int16))
        planes.append(np.where(winner == w, top, e).astype(np.int8))
    return frozen(*planes)


@functools.lru_cache(maxsize=None)
def arbitrary_planes(W, n, P, seed):
    """(payload planes, exponent planes) of a slice of n elements in B =
    ceil(n / P) blocks.  Payload: W planes of B * P uniformly random 32-bit
    words (wire order, BE), the tail past n included; for W > 1 every 97th
    word of the last plane makes the W words' sum, in host order after ntohl,
    wrap to exactly 0.  Exponents: arbitrary_exps."""
    B = O.num_blocks(n, P)
    rng = np.random.default_rng([seed, W, n, P])
    host = [rng.integers(0, 2 ** 32, size=B * P, dtype=np.uint64).astype(np.uint32) for _ in range(W)]
    if W > 1:
        rest = np.zeros(B * P, dtype=np.uint32)
        for h in host[:-1]:
            rest = rest + h                                   # uint32: wraps
        host[-1][::97] = (np.uint32(0) - rest)[::97]
        total = np.zeros(B * P, dtype=np.uint32)
        for h in host:
            total = total + h
        assert not total[::97].any()
    return frozen(*[h.byteswap() for h in host]), arbitrary_exps(W, B, seed)


@functools.lru_cache(maxsize=None)
def oracle_case(W, n, P, seed):
    """(planes, exps, aggregated BE plane, max exponents, fp32 output) of
    arbitrary_planes(W, n, P, seed): computed once, shared read-only.  The
    builder's conditions are asserted here, on the oracle's output."""
    pls, exps = arbitrary_planes(W, n, P, seed)
    agg = O.switch_payload(list(pls))
    e = O.switch_exps(list(exps))
    out = O.dequantize(agg, e, n, P, W)
    nan = np.isnan(out)
    assert nan.mean() < 0.01, (W, n, P, nan.mean())
    # block 1 has e = 127 (scale 0 for W >= 2) and, once whole, holds a zero
    # sum: every P >= 64 consecutive words from P on include a multiple of 97
    if W > 1 and n >= 2 * P:
        assert nan.any(), (W, n, P)
    if W > 1 and e.size >= 64:
        # the winner is not guessable: neither plane 0 nor an unsigned max
        unsigned = np.max([x.view(np.uint8) for x in exps], axis=0).view(np.int8)
        assert (unsigned != e).mean() > 0.1 and (exps[0] != e).mean() > 0.05
    return pls, exps, *frozen(agg, e, out)


# ---------------------------------------------------------- device buffers --

def guarded(torch, dev, n, dtype, off=0):
    """(buffer, view): `view` is n elements of `dtype`, `off` elements past a
    16-byte boundary, with GUARD sentinel elements (and the offset's slack) on
    both sides inside `buffer`."""
    size_ = torch.empty(0, dtype=dtype).element_size()
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[size_]
    raw = torch.full((GUARD + off + n + GUARD,), SENT[size_], dtype=idt, device=dev)
    assert raw.data_ptr() % 16 == 0
    buf = raw.view(dtype)
    return buf, buf[GUARD + off:GUARD + off + n]


def fetch(torch, buf, view, written=True):
    """(the view's elements on the host as raw unsigned integers, whether every
    element of `buf` outside the view still holds the sentinel), from one copy
    of `buf`.  written=False: the view must hold the sentinel too."""
    size_ = buf.element_size()
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[size_]
    raw = buf.view(idt).cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[size_])
    n = view.numel()
    if not written or n == 0:
        return raw[:0], bool((raw == SENT[size_]).all())
    lo = (view.data_ptr() - buf.data_ptr()) // size_
    return raw[lo:lo + n], bool((raw[:lo] == SENT[size_]).all() and (raw[lo + n:] == SENT[size_]).all())


def guards_intact(torch, buf, view, written=True):
    return fetch(torch, buf, view, written)[1]


def put(torch, dev, arr, off=0):
    """A copy of `arr` on the device, `off` elements past a 16-byte boundary."""
    src = torch.from_numpy(np.array(arr))
    buf = torch.empty(arr.size + 16, dtype=src.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + arr.size]
    t.copy_(src)
    return t


def words(t):
    return t.cpu().numpy().view(np.uint32)


def i32(a):
    return np.asarray(a).view(np.int32)


# -------------------------------------------------------- sml_switch_exps --

EXPS_BLOCKS = (1, 2, 3, 4, 5, 7, 8, 1023, 1025, 4099)


@pytest.mark.parametrize("placement", ("aligned", "planes-offset", "out-offset"))
@pytest.mark.parametrize("W", (1, 2, 3, 5, 16))
def test_switch_exps_matches_oracle(sw, cuda, W, placement):
    """sml_switch_exps against O.switch_exps: the dword path (planes and
    output 4-byte aligned), the byte path (plane w at byte offset w % 4; for
    W = 1 at offset 1), the byte path for an output at byte offset 1; every
    block count with its num_blocks % 4 tail; with and without
    SML_FLAG_PEER_PLANES; 4099 blocks also on one workgroup (grid-stride:
    1024 blocks per pass)."""
    import torch
    full = arbitrary_exps(W, max(EXPS_BLOCKS), 11)
    offs = [(w % 4 if W > 1 else 1) if placement == "planes-offset" else 0 for w in range(W)]
    d_full = [put(torch, cuda, e, off) for e, off in zip(full, offs)]
    assert all(d.data_ptr() % 4 == off for d, off in zip(d_full, offs))
    for nb in EXPS_BLOCKS:
        want = O.switch_exps([e[:nb] for e in full])
        if W > 1 and nb >= 4:
            assert tuple(want[:4]) == FORCED_TOPS
        for cap in (0, 1) if nb == max(EXPS_BLOCKS) else (0,):
            sw.set_grid_limit(cap)
            for flags in (0, sw.FLAG_PEER_PLANES):
                buf, out = guarded(torch, cuda, nb, torch.int8, off=1 if placement == "out-offset" else 0)
                assert sw.switch_exps([d[:nb] for d in d_full], out=out, flags=flags) is out
                got, intact = fetch(torch, buf, out)
                assert np.array_equal(got.view(np.int8), want) and intact, (nb, cap, flags)
        sw.set_grid_limit(0)


def test_switch_exps_allocates_its_output(sw, cuda):
    import torch
    exps = arbitrary_exps(3, 1025, 12)
    got = sw.switch_exps([put(torch, cuda, e) for e in exps])
    assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), O.switch_exps(list(exps)))
    with pytest.raises(ValueError):
        sw.switch_exps([])
    with pytest.raises(ValueError):
        sw.switch_exps([got, got[:5]])


# --------------------------------------------------------------------- K6 --

SUBSETS = [s for s in range(1, 8)]            # bit 0: payload_out, bit 1: exps_out, bit 2: out


def run_k6(sw, torch, dev, d_pl, d_ex, n, P, subset, flags, want, tag, e_off=0, o_off=0):
    """One K6 call writing the outputs `subset` names into guarded buffers;
    each is compared with `want` = (agg words as stored, exponents, fp32 out)."""
    B = O.num_blocks(n, P)
    pb, p_out = guarded(torch, dev, B * P, torch.int32)
    eb, e_out = guarded(torch, dev, B, torch.int8, off=e_off)
    ob, o_out = guarded(torch, dev, n, torch.float32, off=o_off)
    need_exps = subset & 6
    sw.switch_aggregate(d_pl, d_ex if need_exps else None, n, P,
                        payload_out=p_out if subset & 1 else None, exps_out=e_out if subset & 2 else None,
                        out=o_out if subset & 4 else None, flags=flags)
    # an output that was not asked for is untouched too: its view still holds the sentinel
    got = [fetch(torch, buf, view, written=bool(subset & bit))
           for bit, buf, view in ((1, pb, p_out), (2, eb, e_out), (4, ob, o_out))]
    assert all(intact for _, intact in got), (tag, [intact for _, intact in got])
    agg, e, out = want
    if subset & 1:
        assert np.array_equal(got[0][0], agg), tag
    if subset & 2:
        assert np.array_equal(got[1][0].view(np.int8), e), tag
    if subset & 4:
        assert float_bits_equal_nan_ok(got[2][0].view(np.float32), out), tag


def device_planes(torch, dev, pls, le):
    return [put(torch, dev, i32(O.bswap32(p) if le else p)) for p in pls]


@pytest.mark.parametrize("W", (1, 3, 2, 16))
@pytest.mark.parametrize("P", PACKETS)
def test_k6_every_output_subset(sw, cuda, P, W):
    """K6 on arbitrary planes: each of the seven non-empty subsets of
    {payload_out, exps_out, out}, BE and LE words, W = 1, 3 (division) and
    2, 16 (reciprocal).  payload_out over all B * P words (the tail is the
    planes' non-zero tail summed), exps_out over B bytes, out over n."""
    import torch
    n = size(P)
    pls, exps, agg, e, out = oracle_case(W, n, P, 21)
    d_ex = [put(torch, cuda, x) for x in exps]
    for le in (False, True):
        d_pl = device_planes(torch, cuda, pls, le)
        want = (O.bswap32(agg) if le else agg, e, out)
        for subset in SUBSETS:
            run_k6(sw, torch, cuda, d_pl, d_ex, n, P, subset, sw.FLAG_PAYLOAD_LE if le else 0, want, (le, subset))


@pytest.mark.parametrize("W", (3, 16))
@pytest.mark.parametrize("P", PACKETS)
def test_k6_exponent_placement(sw, cuda, P, W):
    """Exponent plane w at byte offset w % 4 (the per-lane byte loads),
    exps_out at byte offsets 0..3 past a 16-byte boundary (one store per tile
    where the address allows it, per-packet byte stores elsewhere), the fp32
    bucket at a 4-byte offset; all three outputs."""
    import torch
    n = size(P)
    pls, exps, agg, e, out = oracle_case(W, n, P, 22)
    d_pl = device_planes(torch, cuda, pls, False)
    d_ex = [put(torch, cuda, x, w % 4) for w, x in enumerate(exps)]
    assert [d.data_ptr() % 4 for d in d_ex] == [w % 4 for w in range(W)]
    for e_off in range(4):
        run_k6(sw, torch, cuda, d_pl, d_ex, n, P, 7, 0, (agg, e, out), e_off, e_off=e_off, o_off=1)
    # the per-packet byte stores behind the scalar slice load (aligned planes) once
    d_al = [put(torch, cuda, x) for x in exps]
    run_k6(sw, torch, cuda, d_pl, d_al, n, P, 7, 0, (agg, e, out), "aligned", e_off=1, o_off=1)


@pytest.mark.parametrize("P", PACKETS)
def test_k6_edge_sizes(sw, cuda, P):
    """One element, one packet less / exactly / plus one element, and the
    tile boundary: W = 3, all three outputs, both byte orders."""
    import torch
    W = 3
    for n in (1, P - 1, P, P + 1, 1023, 1024, 1025, 2048):
        pls, exps, agg, e, out = oracle_case(W, n, P, 23)
        d_ex = [put(torch, cuda, x) for x in exps]
        for le in (False, True):
            d_pl = device_planes(torch, cuda, pls, le)
            want = (O.bswap32(agg) if le else agg, e, out)
            run_k6(sw, torch, cuda, d_pl, d_ex, n, P, 7, sw.FLAG_PAYLOAD_LE if le else 0, want, (n, le))


@pytest.mark.parametrize("W", (3, 16))
@pytest.mark.parametrize("P", PACKETS)
def test_k6_in_place_into_last_plane(sw, cuda, P, W):
    """Payload only, aggregated in place into plane W - 1 (2 of 3, 15 of 16),
    BE and LE: the other planes are unchanged."""
    import torch
    n = size(P)
    pls, _, agg, _, _ = oracle_case(W, n, P, 24)
    for le in (False, True):
        d_pl = device_planes(torch, cuda, pls, le)
        sw.switch_aggregate(d_pl, None, n, P, payload_out=d_pl[W - 1], flags=sw.FLAG_PAYLOAD_LE if le else 0)
        assert np.array_equal(words(d_pl[W - 1]), O.bswap32(agg) if le else agg), le
        for w in range(W - 1):
            assert np.array_equal(words(d_pl[w]), O.bswap32(pls[w]) if le else pls[w]), (le, w)


# --------------------------------------------------------- the shard form --

# (n, P, W).  The first three are the issue's; S = ceil(B / W) is odd in the
# first only (49; the others give 6 and 2, shard starts at even blocks), so
# two more with an odd S follow: (17 blocks, W 4: S 5, a ragged last shard)
# and (11 blocks, W 5: S 3, a short fourth shard and an empty fifth).
SHARD_CASES = [(9 * 1024 + 7, 64, 3), (5 * 1024 + 1, 256, 4), (7 * 1024 + 5, 1024, 5),
               (4 * 1024 + 1, 256, 4), (10 * 1024 + 5, 1024, 5)]


@pytest.mark.parametrize("typ", ("fp32", "fp16", "bf16"))
@pytest.mark.parametrize("n,P,W", SHARD_CASES)
def test_k6_shard_form_float(sw, cuda, n, P, W, typ):
    """K6 as the switch backend's Aggregate calls it, rank by rank: the
    planes from block b0 on, all W exponent pointers the one view gexp[b0:]
    (any byte alignment), `out` only, into out[b0 * P:] (a 16-bit bucket
    starts at an odd element), SML_FLAG_PEER_PLANES.  After all ranks the
    whole bucket is the oracle's and the guards are intact."""
    import torch
    from switchml_amd.p2pswitch import shard_blocks
    pls, _, _, gexp, out = oracle_case(W, n, P, 25)
    B = O.num_blocks(n, P)
    dtype = torch.float32 if typ == "fp32" else tdtype(typ)
    d_pl = device_planes(torch, cuda, pls, False)
    d_gexp = put(torch, cuda, gexp)
    buf, bucket = guarded(torch, cuda, n, dtype, off=0 if typ == "fp32" else 1)
    shards = [shard_blocks(B, W, r) for r in range(W)]
    assert sum(nb for _, nb in shards) == B and shards[-1][1] < shards[0][1]
    for b0, nb in shards:
        numel = max(0, min(nb * P, n - b0 * P))
        ex = d_gexp[b0:b0 + nb]
        sw.switch_aggregate([p[b0 * P:(b0 + nb) * P] for p in d_pl], [ex] * W, numel, P,
                            out=bucket[b0 * P:b0 * P + numel], flags=sw.FLAG_PEER_PLANES)
    # `out` is O.dequantize(O.switch_payload(planes), gexp, n, P, W): the max of W copies of gexp is gexp
    got, intact = fetch(torch, buf, bucket)
    if typ == "fp32":
        assert float_bits_equal_nan_ok(got.view(np.float32), out)
    else:
        assert_half_equal(torch.from_numpy(got.view(np.int16).copy()).view(dtype), narrow(out, typ))
    assert intact


@pytest.mark.parametrize("n,P,W", SHARD_CASES)
def test_k6_shard_form_int32(sw, cuda, n, P, W):
    """K6 as IntChunk calls it: host-order words, payload only over the
    shard's whole blocks, SML_FLAG_PAYLOAD_LE | SML_FLAG_PEER_PLANES, into
    outplane[b0 * P:].  Full-range int32 planes: the wrapping sum."""
    import torch
    from switchml_amd.p2pswitch import shard_blocks
    B = O.num_blocks(n, P)
    rng = np.random.default_rng([26, n, P, W])
    pls = [rng.integers(-2 ** 31, 2 ** 31, size=B * P, dtype=np.int64).astype(np.int32) for _ in range(W)]
    want = np.zeros(B * P, dtype=np.uint32)
    for p in pls:
        want = want + p.view(np.uint32)                        # uint32: wraps
    assert np.array_equal(want, O.bswap32(O.switch_payload([O.bswap32(p) for p in pls])))
    d_pl = [put(torch, cuda, p) for p in pls]
    buf, outplane = guarded(torch, cuda, B * P, torch.int32)
    for r in range(W):
        b0, nb = shard_blocks(B, W, r)
        sw.switch_aggregate([p[b0 * P:(b0 + nb) * P] for p in d_pl], None, nb * P, P,
                            payload_out=outplane[b0 * P:(b0 + nb) * P],
                            flags=sw.FLAG_PAYLOAD_LE | sw.FLAG_PEER_PLANES)
    got, intact = fetch(torch, buf, outplane)
    assert np.array_equal(got, want) and intact


# -------------------------------------------------------- launch geometry --

@pytest.mark.parametrize("P", (64, 1024))
def test_switch_kernels_geometry_invariant(sw, cuda, P):
    """K6, sml_switch_exps, sml_copy_words and both segment copies under
    every (grid cap, XCD chunk) pair of test_launch_geometry.py, each against
    the oracle or the source bytes.  42 tiles are 11 workgroups: chunk 1
    permutes a head of 8 and keeps a tail of 3, caps 8 and 13 stride."""
    import torch
    W = 3
    n = 41 * 1024 + P + 3
    pls, exps, agg, e, out = oracle_case(W, n, P, 27)
    d_pl = device_planes(torch, cuda, pls, False)
    d_ex = [put(torch, cuda, x) for x in exps]
    # the exponent max alone: the issue's 656 blocks (one workgroup), and 41 * 1024 (41 workgroups: caps stride)
    ex_sets = [arbitrary_exps(W, nb, 28) for nb in (41 * 1024 // 64, 41 * 1024)]
    d_sets = [[put(torch, cuda, x) for x in s] for s in ex_sets]
    ex_want = [O.switch_exps(list(s)) for s in ex_sets]
    g = torch.Generator(device="cuda")
    g.manual_seed(P)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 3,), dtype=torch.int32, device=cuda, generator=g)
    counts = (GROUP * 5 // 2, GROUP, GROUP * 3 // 10)         # 2.5, 1 and 0.3 groups
    seg32 = [torch.randint(-2 ** 31, 2 ** 31 - 1, (c + 1,), dtype=torch.int32, device=cuda, generator=g)
             for c in counts]
    seg16 = [torch.randint(-2 ** 15, 2 ** 15 - 1, (c + 1,), dtype=torch.int16, device=cuda, generator=g)
             for c in counts]
    h_src = words(src)
    h_seg = {torch.int32: [words(s) for s in seg32],
             torch.bfloat16: [s.cpu().numpy().view(np.uint16) for s in seg16]}
    for cap, chunk in GEOMETRIES:
        sw.set_grid_limit(cap)
        sw.set_xcd_chunk(chunk)
        tag = (cap, chunk)
        run_k6(sw, torch, cuda, d_pl, d_ex, n, P, 7, 0, (agg, e, out), tag)
        for d_set, want in zip(d_sets, ex_want):
            buf, o = guarded(torch, cuda, want.size, torch.int8)
            sw.switch_exps(d_set, out=o)
            got, intact = fetch(torch, buf, o)
            assert np.array_equal(got.view(np.int8), want) and intact, tag
        buf, dst = guarded(torch, cuda, n, torch.int32, off=1)
        sw.copy_words(src[3:], dst)
        got, intact = fetch(torch, buf, dst)
        assert np.array_equal(got, h_src[3:]) and intact, tag
        for segs, dtype in ((seg32, torch.int32), (seg16, torch.bfloat16)):
            outs = [guarded(torch, cuda, c, dtype, off=i) for i, c in enumerate(counts)]
            pairs = [(s[1:].view(dtype), o) for s, (_, o) in zip(segs, outs)]
            (sw.copy_segments if dtype == torch.int32 else sw.copy_segments_typed)(pairs)
            for h, (buf, o) in zip(h_seg[dtype], outs):
                got, intact = fetch(torch, buf, o)
                assert np.array_equal(got, h[1:]) and intact, (tag, dtype)


# --------------------------------------------------------- sml_copy_words --

@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 1024, 1025, 5 * 1024 + 7))
def test_copy_words(sw, cuda, n):
    """Random words, source and destination each 0..3 words past a 16-byte
    boundary: the destination is the source, its guards and the source are
    untouched."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 4,), dtype=torch.int32, device=cuda, generator=g)
    assert raw.data_ptr() % 16 == 0
    h_raw = words(raw)
    for so in range(4):
        src = raw[so:so + n]
        for do in range(4):
            # float32 on one side: the words are copied, whatever the 32-bit dtype
            buf, dst = guarded(torch, cuda, n, torch.float32 if do == 3 else torch.int32, off=do)
            assert sw.copy_words(src, dst) is dst
            got, intact = fetch(torch, buf, dst)
            assert np.array_equal(got, h_raw[so:so + n]) and intact, (so, do)
    assert np.array_equal(words(raw), h_raw)
    with pytest.raises(ValueError):
        sw.copy_words(raw[:2], raw[2:])


# ------------------------------------------ sml_widen_u8_i32 / narrow_i32_u8 --

U8_SIZES = (1, 3, 4, 5, 255, 256, 257, 5 * 1024 + 7)


@pytest.mark.parametrize("n", U8_SIZES)
def test_widen_u8_i32(sw, cuda, n):
    """Bytes zero-extended: element 0 is 128 and from 256 elements on every
    byte value occurs, so a sign extension shows at every size."""
    import torch
    x = ((np.arange(n) * 89 + 128) % 256).astype(np.uint8)
    assert x[0] == 128 and (n < 256 or np.unique(x).size == 256)
    for off in range(4):
        d_x = put(torch, cuda, x, off)
        assert d_x.data_ptr() % 4 == off
        buf, out = guarded(torch, cuda, n, torch.int32)
        assert sw.widen_u8_i32(d_x, out=out) is out
        got, intact = fetch(torch, buf, out)
        assert np.array_equal(got.view(np.int32), x.astype(np.int32)) and intact, off
    assert np.array_equal(sw.widen_u8_i32(d_x).cpu().numpy(), x.astype(np.int32))


@pytest.mark.parametrize("n", U8_SIZES)
def test_narrow_i32_u8(sw, cuda, n):
    """Full-range int32 words, negatives included, to their low bytes, into a
    uint8 bucket at byte offsets 0..3 with guard bytes on both sides."""
    import torch
    rng = np.random.default_rng(n)
    x = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    x[0] = -1
    x[-1] = np.int32(-2 ** 31 + 0x80)
    want = (x & 0xFF).astype(np.uint8)
    d_x = put(torch, cuda, x)
    for off in range(4):
        buf, out = guarded(torch, cuda, n, torch.uint8, off=off)
        assert out.data_ptr() % 4 == off
        assert sw.narrow_i32_u8(d_x, out=out) is out
        got, intact = fetch(torch, buf, out)
        assert np.array_equal(got, want) and intact, off
    assert np.array_equal(sw.narrow_i32_u8(d_x).cpu().numpy(), want)


def test_u8_allreduce_chain(sw, cuda):
    """The plugin's ncclUint8 path: widen W = 3 byte buckets into planes, K6
    payload only over host-order words, narrow: the byte sums mod 256."""
    import torch
    W, P, n = 3, 256, 5 * 1024 + 7
    B = O.num_blocks(n, P)
    rng = np.random.default_rng(31)
    xs = [rng.integers(0, 256, size=n, dtype=np.int64).astype(np.uint8) for _ in range(W)]
    xs[0][:256] = np.arange(256)
    xs[1][:256] = 255
    want = (sum(x.astype(np.int64) for x in xs) % 256).astype(np.uint8)
    planes = [torch.zeros(B * P, dtype=torch.int32, device=cuda) for _ in range(W)]
    for w, x in enumerate(xs):
        sw.widen_u8_i32(put(torch, cuda, x, w + 1), out=planes[w][:n])
    pb, summed = guarded(torch, cuda, B * P, torch.int32)
    sw.switch_aggregate(planes, None, n, P, payload_out=summed, flags=sw.FLAG_PAYLOAD_LE)
    buf, out = guarded(torch, cuda, n, torch.uint8, off=3)
    sw.narrow_i32_u8(summed[:n], out=out)
    got, intact = fetch(torch, buf, out)
    assert np.array_equal(got, want) and intact and guards_intact(torch, pb, summed)
