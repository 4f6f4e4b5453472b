"""CPU tests: the oracle against the COMPILED reference.

oracle/ref/ builds the reference's client library, unmodified, into
oracle/_ref/ (a stand-in glog header is all it lacks): the
CpuExponentQuantizerPPP behind a C ABI under the reference's release flags and
under its debug flags (-O0: the float -> uint32_t conversion of ppp.cc:103 is
undefined for out-of-range values, so both code generations are held), and the
whole dummy-backend Context as a program.  Everything the GPU suite trusts
(oracle/sml_oracle.c and its numpy twin) is compared with them here, bit for
bit on the raw words, NaN payload bits included.

The one deliberate difference is asserted, not sliced away: bytes the
reference never writes (the words of a partial last block past numel, the
exponent byte of the packets p >= B) keep the sentinel the buffers were
prefilled with, and the oracle defines them as 0.

Skips only where neither oracle/_ref/ nor the reference checkout exists; with
the checkout present a missing oracle/_ref/ is a failure.
"""
import json

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import special_values
from test_oracle import dnn_example_layers, kat_arrays, load_kats

PS = (64, 128, 256, 512, 1024)
WS = (1, 2, 3, 8, 255, 65535)
NS = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4113)
BATCHES = (1, 2, 64, 1 << 20)          # the last is >= B for every n here
FAMILIES = ("special", "glibc", "bits", "normal", "pattern")
BUILDS = [pytest.param(False, id="release"), pytest.param(True, id="debug")]

COUNTS = {}                             # case counts, printed by the last test


@pytest.fixture(scope="module", autouse=True)
def _reference_built():
    if O.ref_available():
        return
    if O.reference_checkout_available():
        pytest.fail("the reference checkout exists but oracle/_ref/ is not built: run __graft_entry__.build()")
    pytest.skip("neither oracle/_ref/ nor the reference checkout exists here")


def family(kind, n, seed):
    if kind == "special":
        return special_values(n, np.random.default_rng(seed))
    if kind == "glibc":
        return O.c_ref_random_floats(seed + 1, n)
    if kind == "bits":
        return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    if kind == "normal":
        return O.splitmix_normal(seed + 42, n)
    if kind == "pattern":
        return O.ref_pattern_floats(n)
    raise ValueError(kind)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def count(key, k=1):
    COUNTS[key] = COUNTS.get(key, 0) + k


def check_stream(r, x, P, W, ge, ctx):
    """What the reference sent for one slice against the oracle's planes.
    Returns (own exponents, oracle payload)."""
    n, B, b = x.size, r["B"], r["b"]
    own = r["tx_extra"][:B, 0].view(np.int8)
    assert np.array_equal(own, O.exponents(x, P)), ("exponent plane", ctx)
    want = O.quantize(x, P, W, global_exps=ge)
    got = r["tx"][b:].reshape(-1)
    assert np.array_equal(got[:n], want[:n]), ("payload", ctx)
    # never written by the reference; 0 by the oracle's definition
    assert np.all(got[n:] == O.SENTINEL_WORD) and np.all(want[n:] == 0), ("stale tail", ctx)
    assert np.all(r["tx"][:b] == O.SENTINEL_WORD), ("extra batch payload", ctx)
    assert np.all(r["tx_extra"][B:, 0] == O.SENTINEL_BYTE), ("exponent byte of p >= B", ctx)
    assert np.all(r["tx_extra"][:, 1] == O.SENTINEL_BYTE), ("second extra-info byte", ctx)
    return own, want


def cases(P, with_kats=False):
    """(W, n, family, batch, x) over the whole W x n grid, every data family at
    every point, the batch value rotating so each meets every n and W."""
    i = 0
    for W in WS:
        for n in NS:
            for kind in FAMILIES:
                yield W, n, kind, BATCHES[i % len(BATCHES)], family(kind, n, seed=n * 7 + W)
                i += 1
    if with_kats:
        for c in load_kats():
            x, _, _, _ = kat_arrays(c)
            for batch in BATCHES:
                yield c["W"], x.size, "kat:" + c["name"], batch, x


# ------------------------------------------------------- per-packet PPP --

@pytest.mark.parametrize("debug", BUILDS)
@pytest.mark.parametrize("P", PS)
def test_ppp_own_exponents_round_trip(P, debug):
    """Exponent plane, payload with the slice's own exponents, and the
    dequantize of the dummy backend's x W, packet by packet."""
    for W, n, kind, batch, x in cases(P, with_kats=True):
        ctx = (P, W, n, kind, batch)
        r = O.ref_packet_stream(x, P, W, batch, debug=debug, aggregate=True)
        assert r["b"] == min(r["B"], batch) and r["total"] == r["B"] + r["b"]
        own, q = check_stream(r, x, P, W, None, ctx)
        want = O.dequantize(O.loopback_aggregate(q, W), own, n, P, W)
        assert np.array_equal(bits(r["out"]), bits(want)), ("round trip", ctx)
        count("ppp own exponents + round trip")


@pytest.mark.parametrize("debug", BUILDS)
@pytest.mark.parametrize("P", PS)
def test_ppp_global_exponents(P, debug):
    """Payload with global exponents above and 1..40 below the own ones
    (clipped to int8; below is the x86 wrap path of ppp.cc:103), and the
    dequantize of those words x W under the same exponents."""
    for W, n, kind, batch, x in cases(P, with_kats=True):
        ctx = (P, W, n, kind, batch)
        rng = np.random.default_rng(n * 31 + W)
        own = O.exponents(x, P).astype(np.int32)       # e = 128 arrives here as -128
        delta = np.where(rng.random(own.size) < 0.3, rng.integers(1, 6, own.size), -rng.integers(1, 41, own.size))
        ge = np.clip(own + delta, -128, 127).astype(np.int8)
        r = O.ref_packet_stream(x, P, W, batch, debug=debug, global_exps=ge, aggregate=True)
        _, q = check_stream(r, x, P, W, ge, ctx)
        want = O.dequantize(O.loopback_aggregate(q, W), ge, n, P, W)
        assert np.array_equal(bits(r["out"]), bits(want)), ("dequantize", ctx)
        count("ppp global exponents")


def arbitrary_words(rng, B, P):
    w = rng.integers(0, 1 << 32, B * P, dtype=np.uint64).astype(np.uint32)
    w[rng.random(B * P) < 0.1] = 0
    w[:: 7] = O.bswap32(rng.integers(-3, 4, w[::7].size).astype(np.int32))
    w[:P // 2] = 0                                      # a run of zero words in block 0
    return w


def arbitrary_exps(rng, B):
    e = rng.integers(-128, 128, B).astype(np.int8)
    fixed = np.array([127, -128, -97, -96, 0, 120, -126], dtype=np.int8)   # scale 0 (W > 1), +inf, boundary
    k = min(B, fixed.size)
    e[:k] = np.roll(fixed, int(rng.integers(0, fixed.size)))[:k]
    return e


@pytest.mark.parametrize("debug", BUILDS)
@pytest.mark.parametrize("P", PS)
def test_ppp_arbitrary_words_and_exponents(P, debug):
    """PostprocessSingle on arbitrary received words under arbitrary exponents
    in [-128, 127]: zero words under a scale of 0 (0/0) and of +inf included.
    The payload quantized under those exponents is compared on the way."""
    zero_by_zero = 0
    for W in WS:
        for i, n in enumerate(NS):
            rng = np.random.default_rng(P + W * 13 + n)
            x = family(FAMILIES[(i + W) % len(FAMILIES)], n, seed=n + W)
            B = O.num_blocks(n, P)
            batch = BATCHES[(i + W) % len(BATCHES)]
            ge, words = arbitrary_exps(rng, B), arbitrary_words(rng, B, P)
            ctx = (P, W, n, batch)
            r = O.ref_packet_stream(x, P, W, batch, debug=debug, global_exps=ge, rx_words=words)
            check_stream(r, x, P, W, ge, ctx)
            want = O.dequantize(words, ge, n, P, W)
            assert np.array_equal(bits(r["out"]), bits(want)), ("dequantize", ctx)
            s = np.repeat(O.scale_lut(W)[ge.view(np.uint8)], P)[:n]
            zero_by_zero += int(np.sum((s == 0) & (words[:n] == 0)))
            assert np.all(np.isnan(r["out"][(s == 0) & (words[:n] == 0)]))
            assert np.all(r["out"][np.isinf(s)] == 0)
            count("ppp arbitrary words and exponents")
    assert zero_by_zero > 0


@pytest.mark.parametrize("debug", BUILDS)
def test_zero_by_zero_nan_bits(debug):
    """0/0 in the dequantize (scale 0 from the float overflow of W * 2^e,
    times a zero word): x86 SSE gives the default NaN 0xffc00000, in the
    reference's two builds and in the oracle alike."""
    P, W, n = 64, 3, 130
    words = np.zeros(3 * P, dtype=np.uint32)
    ge = np.array([127, 127, 127], dtype=np.int8)
    assert O.scale_lut(W)[127] == 0
    r = O.ref_packet_stream(np.ones(n, np.float32), P, W, 2, debug=debug, global_exps=ge, rx_words=words)
    assert np.all(bits(r["out"]) == 0xFFC00000)
    assert np.all(bits(O.dequantize(words, ge, n, P, W)) == 0xFFC00000)
    count("ppp 0/0 NaN bits")


@pytest.mark.parametrize("debug", BUILDS)
def test_numpy_twin_against_reference(debug):
    """The independent numpy restatement on a subset of the grid."""
    for P in (64, 256, 1024):
        for W in (1, 3, 65535):
            for n in (65, 1025):
                for kind in FAMILIES:
                    x = family(kind, n, seed=n + W)
                    rng = np.random.default_rng(n + W)
                    own = O.np_exponents(x, P)
                    ge = np.clip(own.astype(np.int32) - rng.integers(0, 30, own.size), -128, 127).astype(np.int8)
                    r = O.ref_packet_stream(x, P, W, 64, debug=debug, global_exps=ge, aggregate=True)
                    B, b = r["B"], r["b"]
                    assert np.array_equal(r["tx_extra"][:B, 0].view(np.int8), own)
                    q = O.np_quantize(x, P, W, global_exps=ge)
                    assert np.array_equal(r["tx"][b:].reshape(-1)[:n], q[:n])
                    want = O.np_dequantize(O.loopback_aggregate(q, W), ge, n, P, W)
                    assert np.array_equal(bits(r["out"]), bits(want)), (P, W, n, kind)
                    count("numpy twin")


@pytest.mark.parametrize("debug", BUILDS)
@pytest.mark.parametrize("P", PS)
def test_int32_slices(P, debug):
    """INT32: PreprocessSingle / PostprocessSingle are the byte swap, there is
    no extra batch, and the tail of a partial last block is never written."""
    for n in NS:
        for W in (1, 3):
            x = np.random.default_rng(n + P).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
            r = O.ref_packet_stream(x, P, W, BATCHES[n % 4], debug=debug, aggregate=True)
            B = O.num_blocks(n, P)
            assert r["total"] == r["B"] == B                      # NeedsExtraBatch() is false
            sent = r["tx"].reshape(-1)
            assert np.array_equal(sent[:n], O.bswap32(x)), (P, n)
            assert np.all(sent[n:] == O.SENTINEL_WORD)
            assert np.all(r["tx_extra"] == O.SENTINEL_BYTE)       # no exponent byte at all
            want = O.bswap32(O.loopback_aggregate(O.bswap32(x), W)).view(np.int32)
            assert np.array_equal(r["out"], want), (P, n, W)
            assert np.array_equal(want, (x.astype(np.int64) * W).astype(np.int32))
            count("ppp INT32")


@pytest.mark.parametrize("debug", BUILDS)
@pytest.mark.parametrize("P,n,batch", [(64, 65, 1), (64, 4113, 64), (256, 257, 2), (256, 1, 64), (1024, 1025, 1 << 20)])
def test_stale_bytes_are_the_one_deliberate_difference(P, n, batch, debug):
    """The reference leaves the words of a partial last block past numel and
    the exponent byte of the packets p >= B as it found them; the oracle (and,
    on the GPU, the C ABI: tests/test_ref_vectors_gpu.py) writes 0 there."""
    x = O.splitmix_normal(n, n)
    r = O.ref_packet_stream(x, P, 2, batch, debug=debug, aggregate=True)
    B, b = r["B"], r["b"]
    tail = B * P - n
    assert tail > 0
    assert np.all(r["tx"][b:].reshape(-1)[n:] == O.SENTINEL_WORD)
    assert np.all(r["tx_extra"][B:, 0] == O.SENTINEL_BYTE) and r["tx_extra"][B:].size > 0
    assert np.all(O.quantize(x, P, 2)[n:] == 0)
    pe, pp, out, sb = O.dummy_packet_stream(x, P=P, batch_max=min(batch, 1 << 16), num_workers=2)
    assert sb == b
    assert np.all(pe[B:] == 0) and np.all(pp[:b] == 0) and np.all(pp[b:].reshape(-1)[n:] == 0)
    assert np.array_equal(pp[b:].reshape(-1)[:n], r["tx"][b:].reshape(-1)[:n])
    assert np.array_equal(bits(out), bits(r["out"]))
    count("stale bytes")


# -------------------------------------------------------------- Context --

def oracle_allreduce(x, P, W, T, mop, process_packets):
    """One job of the reference's Context by the oracle: the packet loop where
    the dummy backend multiplies by W, the planes slice by slice where it does
    not (process_packets off leaves the quantization round trip)."""
    if x.dtype == np.int32:
        return (x.astype(np.int64) * (W if process_packets else 1)).astype(np.int32)
    if x.size == 0:
        return x.copy()
    if process_packets:
        return O.dummy_allreduce(x, P=P, max_outstanding_packets=mop, num_worker_threads=T, num_workers=W)
    out = np.empty_like(x)
    for t in range(T):
        off, m = O.slice_geometry(x.size, T, t)
        sl = x[off:off + m]
        out[off:off + m] = O.dequantize(O.quantize(sl, P, W), O.exponents(sl, P), m, P, W)
    return out


def context_data(dtype, n, seed):
    if dtype == "i32":
        return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    x = family(FAMILIES[seed % len(FAMILIES)], n, seed)
    return x


@pytest.mark.parametrize("T", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("dtype", ["f32", "i32"])
def test_context_allreduce(T, dtype):
    """Context::Start / AllReduceAsync / WaitForAllJobs of the reference in a
    fresh process per case against the oracle's packet loop and FIFO split.
    Every (T, mop, n) with P, W, process_packets and in-place rotating."""
    i = 0
    for mop in (T, 64, 256):
        for n in (1, T - 1, 1000, 65_537, 100_003):
            for rep in range(2):
                P = (64, 256, 1024)[(i + rep) % 3]
                W = (1, 3, 8)[(i // 3 + rep) % 3]
                process = bool((i + rep) % 2)
                inplace = bool((i // 2 + rep) % 2)
                x = context_data(dtype, n, seed=i + T)
                x0 = x.copy()
                got = O.ref_allreduce(x, P=P, num_workers=W, num_worker_threads=T, max_outstanding_packets=mop,
                                      process_packets=process, inplace=inplace)
                want = oracle_allreduce(x0, P, W, T, mop, process)
                assert np.array_equal(bits(got), bits(want)), (T, mop, n, P, W, process, inplace, dtype)
                count("context")
            i += 1


def scaled_dnn_layers():
    """The example model's layers scaled down to <= 100 003 elements, each
    keeping its numel mod 16 (the ragged slice starts)."""
    return [(m // 168 // 16) * 16 + m % 16 for m in dnn_example_layers()]


def test_context_multi_job_dnn_flow():
    """dnn_benchmark's flow in ONE Context: slices of one buffer, in place,
    submitted in backward order, two iterations back to back."""
    layers = scaled_dnn_layers()
    assert max(layers) <= 100_003 and [m % 16 for m in layers] == [m % 16 for m in dnn_example_layers()]
    offs = np.concatenate([[0], np.cumsum(layers)])
    P, W, T, mop = 256, 2, 4, 256
    x = O.ref_pattern_floats(int(offs[-1]))
    order = [(int(offs[li]), layers[li]) for li in reversed(range(len(layers)))] * 2
    got = O.ref_allreduce(x, order, P=P, num_workers=W, num_worker_threads=T, max_outstanding_packets=mop,
                          inplace=True)
    want = x.copy()
    for off, m in order:
        v = want[off:off + m]
        O.dummy_allreduce(v, P=P, max_outstanding_packets=mop, num_worker_threads=T, num_workers=W, out=v)
    assert np.array_equal(bits(got), bits(want))
    count("context multi-job")


# ------------------------------- the reference's known-answer programs --

@pytest.mark.parametrize("num_workers", [1, 2, 3, 8])
def test_hello_world_kat_reference(num_workers):
    """tests/test_oracle.py::test_hello_world_kat through the compiled Context."""
    numel = 1 << 15
    for i in range(8):
        x = (i * numel + np.arange(numel, dtype=np.int64)).astype(np.float32)
        out = O.ref_allreduce(x, P=256, num_workers=num_workers, num_worker_threads=4, max_outstanding_packets=256)
        expected = x * np.float32(num_workers)
        err = (expected - out) / (expected + np.finfo(np.float32).eps) * 100
        assert not np.any(err > 1), (i, np.max(err))
        want = O.dummy_allreduce(x, P=256, max_outstanding_packets=256, num_worker_threads=4, num_workers=num_workers)
        assert np.array_equal(bits(out), bits(want))
        count("known-answer programs")


def test_allreduce_benchmark_verify_pattern_inplace_reference():
    """test_allreduce_benchmark_verify_pattern_inplace: 15 in-place jobs on one
    buffer, one Context."""
    n, W, jobs = 1 << 20, 2, 15
    x = O.ref_pattern_floats(n)
    got = O.ref_allreduce(x, [(0, n)] * jobs, P=256, num_workers=W, num_worker_threads=4,
                          max_outstanding_packets=256, inplace=True)
    expected = x * np.float32(W ** jobs)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = (expected - got) / expected * 100
    assert not np.any(err > 1)
    want = x.copy()
    for _ in range(jobs):
        O.dummy_allreduce(want, P=256, max_outstanding_packets=256, num_worker_threads=4, num_workers=W, out=want)
    assert np.array_equal(bits(got), bits(want))
    count("known-answer programs")


def test_allreduce_benchmark_verify_random_not_inplace_reference():
    n, W, P = 1 << 18, 2, 256
    x = O.c_ref_random_floats(1234, n)
    got = O.ref_allreduce(x, P=P, num_workers=W, num_worker_threads=1, max_outstanding_packets=256)
    want = O.dummy_allreduce(x, P=P, max_outstanding_packets=256, num_worker_threads=1, num_workers=W)
    assert np.array_equal(bits(got), bits(want))
    expected = x * np.float32(W)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = (expected - got) / expected * 100
    e = np.repeat(O.exponents(x, P).astype(np.int32), P)[:n]
    resolved = np.abs(x.astype(np.float64)) >= np.ldexp(1.0, e - 24)
    assert not np.any(err[resolved] > 1)
    count("known-answer programs")


def test_dnn_benchmark_verify_example_model_reference():
    """test_dnn_benchmark_verify_example_model at full size: the example
    model's layers as slices of one buffer, in place, backward order, two
    iterations, one Context."""
    layers = dnn_example_layers()
    W, iters = 2, 2
    offs = np.concatenate([[0], np.cumsum(layers)])
    x = O.ref_pattern_floats(sum(layers))
    order = [(int(offs[li]), layers[li]) for li in reversed(range(len(layers)))] * iters
    got = O.ref_allreduce(x, order, P=256, num_workers=W, num_worker_threads=4, max_outstanding_packets=256,
                          inplace=True, timeout=600)
    expected = x * np.float32(W ** iters)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = (expected - got) / expected * 100
    assert not np.any(err > 1)
    want = x.copy()
    for off, m in order:
        v = want[off:off + m]
        O.dummy_allreduce(v, P=256, max_outstanding_packets=256, num_worker_threads=4, num_workers=W,
                          threaded=True, out=v)
    assert np.array_equal(bits(got), bits(want))
    count("known-answer programs")


def test_zz_case_counts(capsys):
    """Reports how many reference comparisons the tests above made."""
    with capsys.disabled():
        print("\nreference comparisons: " + json.dumps(COUNTS, sort_keys=True) + f" total {sum(COUNTS.values())}")
