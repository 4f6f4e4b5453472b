"""GPU tests of FLOAT16 / BFLOAT16 slices in the batched round trip:
sml_roundtrip_loopback_batch_typed (one launch per element type) against one
sml_roundtrip_loopback_typed per slice, and the client's batch worker, which
now carries 16-bit jobs in its batch calls (client.batch_stats()).

Two references.  The per-slice kernel runs the same device arithmetic, so the
raw words must be equal everywhere, NaNs included.  The oracle recipe is
test_half_client_gpu's: x.float() -> the oracle's dummy-backend packet loop per
FIFO slice -> .to(T); an expected NaN accepts any NaN and at least 99 % of the
positions are compared by bits (its make() puts one NaN and one inf into
20 011 elements; counted on the CPU for every shape of this file, the
expectations hold no NaN at all — a NaN element leaves the quantizer as 0 —
so every position is compared by bits)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_batch_gpu import fifo_slices
from test_collnet_plugin import run_driver
from test_half_client_gpu import N, assert_half_equal, bits_of, expected, make, tdtype

pytestmark = pytest.mark.gpu


def make_n(T, n, seed):
    """make()'s mixture for any length: 20 011-element pieces, cut to n."""
    import torch
    if n == 0:
        return torch.empty(0, dtype=tdtype(T))
    return torch.cat([make(T, N, seed + 1000 * k) for k in range(-(-n // N))])[:n].clone()


def words(t):
    import torch
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_words(a, b):
    import torch
    return torch.equal(words(a), words(b))


@pytest.mark.parametrize("P", [64, 128, 256, 512, 1024])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("typ", ["fp16", "bf16"])
def test_typed_batch_equals_per_slice(cuda, typ, W, P):
    """The shapes of test_batch_kernel_equals_per_slice as 16-bit jobs: ragged
    slices, odd-element starts, a 1-element slice, empty slices, slices shorter
    than a packet, many tiles with a partial last one."""
    import torch
    import switchml_amd as sw
    sizes = [(100_003, 4), (1, 3), (257 * P + 5, 2), (5_000, 7), (0, 2)]
    hs = [make_n(typ, n, 11 * i + P + W) for i, (n, _) in enumerate(sizes)]
    xs = [h.cuda() for h in hs]
    outs = [torch.full_like(x, float("nan")) for x in xs]
    ref = [torch.full_like(x, float("nan")) for x in xs]
    batch = []
    for (n, T), x, o, r in zip(sizes, xs, outs, ref):
        for off, m in fifo_slices(n, T):
            batch.append((x[off:off + m], o[off:off + m]))
            if m:
                sw.roundtrip_loopback(x[off:off + m], P, W, out=r[off:off + m])
    assert len(batch) <= sw.MAX_BATCH_SLICES
    sw.roundtrip_loopback_batch(batch, P, W)
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        assert same_words(o, r)
    for (n, T), h, x, o in zip(sizes, hs, xs, outs):
        assert same_words(x.cpu(), h)                          # inputs untouched
        if n:
            assert_half_equal(o, expected(h, T, W, P))


def test_mixed_types_in_one_call_rne_in_place_pinned_and_max_slices(cuda):
    import torch
    import switchml_amd as sw
    P, W, flags = 256, 2, sw.FLAG_ROUND_RNE
    dts = [torch.float32, torch.float16, torch.bfloat16]
    n = 64 * 700 + 13
    # 64 slices, the three types interleaved; every other slice in place
    src = {torch.float32: torch.from_numpy(O.splitmix_normal(3, n)).cuda(),
           torch.float16: make_n("fp16", n, 4).cuda(), torch.bfloat16: make_n("bf16", n, 5).cuda()}
    work = {dt: x.clone() for dt, x in src.items()}
    out = {dt: torch.full_like(x, float("nan")) for dt, x in src.items()}
    ref = {dt: torch.full_like(x, float("nan")) for dt, x in src.items()}
    batch = []
    for i, (off, m) in enumerate(fifo_slices(n, sw.MAX_BATCH_SLICES)):
        dt = dts[i % 3]
        sw.roundtrip_loopback(src[dt][off:off + m], P, W, out=ref[dt][off:off + m], flags=flags)
        if i % 2:
            batch.append((work[dt][off:off + m], work[dt][off:off + m]))
        else:
            batch.append((src[dt][off:off + m], out[dt][off:off + m]))
    assert len(batch) == sw.MAX_BATCH_SLICES
    sw.roundtrip_loopback_batch(batch, P, W, flags=flags)
    torch.cuda.synchronize()
    for i, (off, m) in enumerate(fifo_slices(n, sw.MAX_BATCH_SLICES)):
        dt = dts[i % 3]
        got = (work if i % 2 else out)[dt][off:off + m]
        assert same_words(got, ref[dt][off:off + m]), (i, dt)
        # and nothing else was written: the other buffer keeps its content
        other, kept = (out, ref[dt].new_full((m,), float("nan"))) if i % 2 else (work, src[dt][off:off + m])
        assert same_words(other[dt][off:off + m], kept), (i, dt)
    x = src[torch.bfloat16]
    with pytest.raises(RuntimeError):
        sw.roundtrip_loopback_batch([(x[:10], out[torch.bfloat16][:10])] * (sw.MAX_BATCH_SLICES + 1), P, W)
    # pinned host 16-bit slices (zero-copy over PCIe) next to an fp32 device slice
    for typ in ("fp16", "bf16"):
        h = make(typ, N, seed=8)
        hx = h.clone().pin_memory()
        ho = torch.zeros_like(hx).pin_memory()
        f = src[torch.float32][:1000]
        fo = torch.empty_like(f)
        sw.roundtrip_loopback_batch([(hx[off:off + m], ho[off:off + m]) for off, m in fifo_slices(N, 3)] + [(f, fo)],
                                    P, W)
        torch.cuda.synchronize()
        assert_half_equal(ho, expected(h, 3, W, P))
        assert same_words(fo, sw.roundtrip_loopback(f, P, W))


def test_typed_batch_random_byte_pools(cuda):
    """Hypothesis (derandomized): 1-8 jobs of 0-40 000 elements, a type per
    job, T = 1-8 FIFO slices, gaps of 0-8 bytes in one byte pool (16-bit jobs
    at any 2-byte offset, fp32 jobs rounded up to 4), P, W, RNE.  The whole
    output pool, pre-filled with a sentinel, must equal byte for byte what the
    per-slice launches leave: the gaps and both ends included."""
    pytest.importorskip("hypothesis")
    from hypothesis import HealthCheck, given, settings
    from hypothesis import strategies as st
    import torch
    import switchml_amd as sw
    dts = [torch.float32, torch.float16, torch.bfloat16]
    # bf16 N(0, 1) words: ordinary values read as fp16, and as fp32 at any 4-byte offset
    pool = bits_of(torch.from_numpy(O.splitmix_normal(99, 700_000)).to(torch.bfloat16))
    pool = torch.from_numpy(pool.view(np.uint8).copy()).cuda()
    sentinel = torch.full_like(pool, 0xA5)

    @settings(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(jobs=st.lists(st.tuples(st.integers(0, 40_000), st.integers(1, 8), st.integers(0, 2), st.integers(0, 8)),
                         min_size=1, max_size=8),
           P=st.sampled_from([64, 128, 256, 512, 1024]), W=st.sampled_from([1, 2, 3, 8, 255]), rne=st.booleans())
    def check(jobs, P, W, rne):
        flags = sw.FLAG_ROUND_RNE if rne else 0
        out, ref = sentinel.clone(), sentinel.clone()
        batch, pos = [], 1 if len(jobs) % 2 else 0            # the first job, too, starts off the pool's alignment
        for n, T, k, gap in jobs:
            esz = dts[k].itemsize
            pos = -(-(pos + gap) // esz) * esz
            assert pos + n * esz <= pool.numel()
            for off, m in fifo_slices(n, T):
                if len(batch) == sw.MAX_BATCH_SLICES:
                    break
                a, b = pos + off * esz, pos + (off + m) * esz
                x, o, r = (p[a:b].view(dts[k]) for p in (pool, out, ref))
                batch.append((x, o))
                if m:
                    sw.roundtrip_loopback(x, P, W, out=r, flags=flags)
            pos += n * esz
        sw.roundtrip_loopback_batch(batch, P, W, flags=flags)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)

    check()


@pytest.fixture
def C(cuda):
    from switchml_amd import client
    yield client
    if client.state() == client.RUNNING:
        client.stop()


def _client_round(C, batch_jobs, vcl=False):
    """6 bf16, 2 fp16 and 2 fp32 device jobs, an in-place bf16 job issued
    twice on one buffer, one INT32 host job; returns the buffers to compare."""
    import torch
    T, W, P = 3, 2, 256
    C.start(C.make_config(num_workers=W, num_worker_threads=T, packet_numel=P, max_outstanding_packets=64 * T,
                          mode="fused", batch_jobs=batch_jobs, bandwidth=0, vcl=vcl))
    hx = [make("bf16", N, seed=70 + i) for i in range(6)] + [make("fp16", N, seed=80 + i) for i in range(2)]
    fx = [O.splitmix_normal(90 + i, N) for i in range(2)]
    hd = [a.cuda() for a in hx]
    fd = [torch.from_numpy(a).cuda() for a in fx]
    ho = [torch.zeros_like(a) for a in hd]
    fo = [torch.zeros_like(a) for a in fd]
    ipx = make("bf16", N, seed=95)
    ip = ipx.cuda()
    xi = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, N, dtype=np.int64).astype(np.int32)
    oi = np.empty_like(xi)
    jobs = []
    for i in range(6):                                        # bf16, with the others in between
        jobs.append(C.allreduce_async(hd[i], ho[i]))
        if i < 2:
            jobs.append(C.allreduce_async(fd[i], fo[i]))
            jobs.append(C.allreduce_async(hd[6 + i], ho[6 + i]))
        if i == 2:
            jobs.append(C.allreduce_async(ip))
        if i == 3:
            jobs.append(C.allreduce_async(xi, oi))
        if i == 4:
            jobs.append(C.allreduce_async(ip))
    C.wait_for_all_jobs()
    assert len(jobs) == 13 and all(j.status() == C.JOB_FINISHED for j in jobs)
    stats, bstats = C.stats(), C.batch_stats()
    C.stop()
    for x, o in zip(hx, ho):
        assert_half_equal(o, expected(x, T, W, P, vcl=vcl))
    for x, o in zip(fx, fo):
        want = O.dummy_allreduce(x, P=P, max_outstanding_packets=64 * T, num_worker_threads=T, num_workers=W, vcl=vcl)
        assert np.array_equal(o.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert_half_equal(ip, expected(expected(ipx, T, W, P, vcl=vcl), T, W, P, vcl=vcl))
    assert np.array_equal(oi, (xi.astype(np.int64) * W).astype(np.int32))
    blocks = [O.num_blocks(O.slice_geometry(N, T, t)[1], P) for t in range(T)]
    assert stats["packets"] == 12 * sum(B + min(B, 64) for B in blocks) + sum(blocks)
    return bstats, [bits_of(o) for o in ho] + [bits_of(ip)] + [o.cpu().numpy() for o in fo]


def test_client_batch_worker_carries_16_bit_jobs(C):
    T = 3
    bstats, bits = _client_round(C, batch_jobs=16)
    assert bstats["batched_slices"] == T * 12 and bstats["single_slices"] == T
    assert 1 <= bstats["launches"] <= bstats["batched_slices"]
    zeros, bits0 = _client_round(C, batch_jobs=0)              # the threaded path: same bits, no batch calls
    assert zeros == {"launches": 0, "batched_slices": 0, "single_slices": 0}
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(bits, bits0))
    _client_round(C, batch_jobs=16, vcl=True)


def test_client_batch_worker_fault_and_stop_with_bf16_jobs(C):
    """test_client_batch_mode_fault_and_stop with bf16 jobs: the injected
    failing worker thread's slice fails its job and its buffer is not
    touched; Stop with jobs queued ends every job and does not hang."""
    import torch
    T = 4
    C.start(C.make_config(num_workers=2, num_worker_threads=T, packet_numel=256, mode="fused", bandwidth=0,
                          batch_jobs=16, fail_worker_thread=2))
    x = make("bf16", N, seed=1).cuda()
    o = torch.full_like(x, 7.0)
    j = C.allreduce_async(x, o)
    with pytest.raises(C.ContextError):
        j.wait()
    assert j.status() == C.JOB_FAILED
    off, m = O.slice_geometry(N, T, 2)
    assert bool((o[off:off + m] == 7.0).all())
    assert same_words(x.cpu(), make("bf16", N, seed=1))
    C.stop()
    C.start(C.make_config(num_workers=2, num_worker_threads=T, packet_numel=256, mode="fused", bandwidth=0,
                          batch_jobs=16))
    big = torch.randn(16 * 2 ** 20, device="cuda").to(torch.bfloat16)
    jobs = [C.allreduce_async(big) for _ in range(20)]
    C.stop()
    assert all(j.status() in (C.JOB_FINISHED, C.JOB_FAILED) for j in jobs)


def test_plugin_allreduce_bf16_device_fused(cuda):
    """A device bf16 buffer (ncclBfloat16 = 9) through the CollNet table with
    mode = fused (batched dispatch): size == 2 * count, bits per the recipe."""
    body = '''
import torch
from oracle import oracle as O
from test_half_client_gpu import assert_half_equal, expected, make
T, W, P, n = 4, 2, 256, 20011
xb = make("bf16", n, seed=21)
xd = xb.cuda(); od = torch.zeros_like(xd)
out["dev_size"] = run(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(od.data_ptr()), n, 9)
assert_half_equal(od, expected(xb, T, W, P))
out["dev_ok"] = True
out["dev_send_untouched"] = bool(torch.equal(xd.cpu().view(torch.int16), xb.view(torch.int16)))
'''
    ini = ("[general]\nnum_workers = 2\nnum_worker_threads = 4\npacket_numel = 256\n"
           "max_outstanding_packets = 256\n[backend.dummy]\nbandwidth = 0\n[backend.hip]\nmode = fused\n")
    out = run_driver(body, ini, preload="import torch")
    assert out["init"] == 0
    assert out["dev_size"] == 2 * 20011 and out["dev_ok"] and out["dev_send_untouched"]
