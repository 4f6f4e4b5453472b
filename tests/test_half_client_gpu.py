"""GPU tests of FLOAT16 / BFLOAT16 jobs through the C++ client (loopback
backend, bulk and fused modes, batched dispatch) and the CollNet plugin.

Expectation, per FIFO slice (O.slice_geometry; blocks restart at the slice
start): x32 = x.float() on the CPU, y32 = the oracle's dummy-backend packet
loop on x32, expected = torch.from_numpy(y32).to(T) (round to nearest even).
Bit-exact on the raw 16-bit words; an expected NaN accepts any NaN, and at
least 99 % of the positions are compared by bits."""
import numpy as np
import pytest

from oracle import oracle as O
from test_collnet_plugin import run_driver

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 256), (3, 2, 64), (2, 8, 1024)]   # (T, W, P)
N = 20_011


@pytest.fixture
def C(cuda):
    from switchml_amd import client
    yield client
    if client.state() == client.RUNNING:
        client.stop()


def tdtype(T):
    import torch
    return torch.float16 if T == "fp16" else torch.bfloat16


def bits_of(t):
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def make(T, n, seed):
    """N(0, 1) in the type, with zeros, the largest finite value, denormals,
    an inf and a NaN mixed in."""
    import torch
    x = torch.from_numpy(O.splitmix_normal(seed, n)).to(tdtype(T))
    b = bits_of(x).copy()
    b[5:40] = 0
    b[100:110] = 0x7BFF if T == "fp16" else 0x7F7F
    b[300:330] = np.arange(1, 31, dtype=np.uint16)
    b[1000] = 0x7C00 if T == "fp16" else 0x7F80
    b[2000] = 0x7E00 if T == "fp16" else 0x7FC0
    return torch.from_numpy(b.view(np.int16)).view(tdtype(T))


def expected(x, threads, W, P, vcl=False):
    import torch
    x32 = x.float().numpy()
    y32 = np.empty_like(x32)
    for t in range(threads):
        off, n = O.slice_geometry(x32.size, threads, t)
        if n:
            y32[off:off + n] = O.dummy_allreduce(x32[off:off + n], P=P, max_outstanding_packets=64,
                                                 num_worker_threads=1, num_workers=W, vcl=vcl)
    return torch.from_numpy(y32).to(x.dtype)


def assert_half_equal(got, exp):
    import torch
    got = got.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape
    nan_e = torch.isnan(exp).numpy()
    assert torch.isnan(got).numpy()[nan_e].all(), "expected NaN, got a number"
    by_bits = ~nan_e
    assert by_bits.mean() >= 0.99
    g, e = bits_of(got)[by_bits], bits_of(exp)[by_bits]
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[0]}: got {g[bad[0]]:#06x}, expected {e[bad[0]]:#06x}"


def _mode(mode):
    return dict(mode="fused", batch_jobs=0) if mode == "fused-threads" else dict(mode=mode)


@pytest.mark.parametrize("mode", ["bulk", "fused", "fused-threads"])
@pytest.mark.parametrize("T,W,P", CASES)
@pytest.mark.parametrize("typ", ["fp16", "bf16"])
def test_allreduce_16_bit_tensors(C, typ, T, W, P, mode):
    """Device, pinned-host and pageable-host tensors, in place and not; T = 3
    gives ragged slices that start at odd elements."""
    import torch
    C.start(C.make_config(num_workers=W, num_worker_threads=T, packet_numel=P, max_outstanding_packets=64 * T,
                          bandwidth=0, **_mode(mode)))
    x = make(typ, N, seed=T * 10 + W)
    exp = expected(x, T, W, P)
    # device
    xd = x.cuda()
    od = torch.zeros_like(xd)
    C.allreduce(xd, od)
    assert_half_equal(od, exp)
    # a packet is P wire words whatever the element size, and the 16-bit
    # types are float types: every slice counts B + min(B, b) packets
    C.wait_for_all_jobs()
    blocks = [O.num_blocks(O.slice_geometry(N, T, t)[1], P) for t in range(T)]
    assert C.stats()["packets"] == sum(B + min(B, 64) for B in blocks)
    assert np.array_equal(bits_of(xd), bits_of(x))            # input untouched
    C.allreduce(xd)                                           # in place
    assert_half_equal(xd, exp)
    # pinned host (zero-copy)
    hx = x.clone().pin_memory()
    ho = torch.zeros_like(hx).pin_memory()
    C.allreduce(hx, ho)
    assert_half_equal(ho, exp)
    C.allreduce(hx)
    assert_half_equal(hx, exp)
    # pageable host (staged by numel * 2 bytes)
    px = x.clone()
    po = torch.zeros_like(px)
    C.allreduce(px, po)
    assert_half_equal(po, exp)
    C.allreduce(px)
    assert_half_equal(px, exp)
    if typ == "fp16":                                         # numpy.float16 arrays
        a = x.numpy().copy()
        C.allreduce(a)
        assert_half_equal(torch.from_numpy(a), exp)
    C.stop()


def test_bf16_jobs_interleaved_with_fp32_under_batched_dispatch(C):
    """batch_jobs on: fp32 jobs go into batched launches, a 16-bit job takes
    the slice-by-slice route between them, FIFO order on one stream."""
    import torch
    T, W, P = 3, 2, 256
    C.start(C.make_config(num_workers=W, num_worker_threads=T, packet_numel=P, max_outstanding_packets=64 * T,
                          mode="fused", batch_jobs=16, bandwidth=0))
    fx = [O.splitmix_normal(50 + i, N + i) for i in range(4)]
    hx = [make("bf16" if i % 2 else "fp16", N + 7 * i, seed=60 + i) for i in range(4)]
    fd = [torch.from_numpy(a).cuda() for a in fx]
    hd = [a.cuda() for a in hx]
    fo = [torch.zeros_like(a) for a in fd]
    ho = [torch.zeros_like(a) for a in hd]
    jobs = []
    for i in range(4):
        jobs.append(C.allreduce_async(fd[i], fo[i]))
        jobs.append(C.allreduce_async(hd[i], ho[i]))
    C.wait_for_all_jobs()
    assert all(j.status() == C.JOB_FINISHED for j in jobs)
    for i in range(4):
        ref = O.dummy_allreduce(fx[i], P=P, max_outstanding_packets=64 * T, num_worker_threads=T, num_workers=W)
        assert np.array_equal(fo[i].cpu().numpy().view(np.uint32), ref.view(np.uint32)), i
        assert_half_equal(ho[i], expected(hx[i], T, W, P))
    C.stop()


def test_packet_mode_refuses_a_bf16_job_and_goes_on(C, capfd):
    import torch
    T, W, P = 2, 2, 256
    C.start(C.make_config(num_workers=W, num_worker_threads=T, packet_numel=P, max_outstanding_packets=64 * T,
                          mode="packet", bandwidth=0))
    x = make("bf16", N, seed=3).cuda()
    before = bits_of(x)
    j = C.allreduce_async(x)
    with pytest.raises(C.ContextError):
        j.wait()
    assert j.status() == C.JOB_FAILED
    err = capfd.readouterr().err
    assert "BFLOAT16" in err and "mode = packet" in err, err
    assert np.array_equal(bits_of(x), before)                 # never run as another type
    f = O.splitmix_normal(9, N)
    out = np.empty_like(f)
    C.allreduce(f, out)                                       # the context is still usable
    ref = O.dummy_allreduce(f, P=P, max_outstanding_packets=64 * T, num_worker_threads=T, num_workers=W)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    C.stop()


def test_plugin_allreduce_bf16_device_and_fp16_host(cuda):
    """Through the CollNet table as RCCL's proxy calls it: a device bf16
    buffer (ncclBfloat16 = 9) and a host fp16 buffer (ncclFloat16 = 6);
    size == 2 * count, bits equal to the recipe."""
    body = '''
import torch
from oracle import oracle as O
T, W, P, n = 4, 2, 256, 20011
def expected(x):
    x32 = x.float().numpy(); y32 = np.empty_like(x32)
    for t in range(T):
        off, m = O.slice_geometry(n, T, t)
        y32[off:off + m] = O.dummy_allreduce(x32[off:off + m], P=P, max_outstanding_packets=64, num_worker_threads=1,
                                             num_workers=W)
    return torch.from_numpy(y32).to(x.dtype)
def same(got, exp):
    nan = torch.isnan(exp)
    ok = bool(torch.isnan(got)[nan].all()) and float((~nan).float().mean()) >= 0.99
    return ok and bool(torch.equal(got.view(torch.int16)[~nan], exp.view(torch.int16)[~nan]))
xb = torch.from_numpy(O.splitmix_normal(21, n)).to(torch.bfloat16)
xd = xb.cuda(); od = torch.zeros_like(xd)
out["dev_size"] = run(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(od.data_ptr()), n, 9)
out["dev_ok"] = same(od.cpu(), expected(xb))
out["dev_send_untouched"] = bool(torch.equal(xd.cpu().view(torch.int16), xb.view(torch.int16)))
xh = torch.from_numpy(O.splitmix_normal(22, n)).to(torch.float16)
h = xh.numpy().copy()
out["host_size"] = run(ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), n, 6)
out["host_ok"] = same(torch.from_numpy(h), expected(xh))
'''
    ini = ("[general]\nnum_workers = 2\nnum_worker_threads = 4\npacket_numel = 256\n"
           "max_outstanding_packets = 256\n[backend.dummy]\nbandwidth = 0\n[backend.hip]\nmode = bulk\n")
    out = run_driver(body, ini, preload="import torch")
    assert out["init"] == 0
    assert out["dev_size"] == 2 * 20011 and out["dev_ok"] and out["dev_send_untouched"]
    assert out["host_size"] == 2 * 20011 and out["host_ok"]


def _xgmi_worker(rank, W, init, session):
    """backend = xgmi: a bf16 job is refused on every worker before any
    barrier (FAILED), the plugin's reduceSupport is 0 for the 16-bit types
    under this configuration, and the session still reduces fp32 buckets."""
    import ctypes
    import torch
    from switchml_amd import client as C
    from switchml_amd.collnet import CollNetV6
    from test_collnet_plugin import PLUGIN
    from test_xgmi_switch import oracle_switch_allreduce, worker_bucket
    C.start(C.make_config(backend="xgmi", rank=rank, num_workers=W, num_worker_threads=2, packet_numel=256,
                          max_outstanding_packets=128, mode="bulk", bandwidth=0, device=0, session=session,
                          timeout_ms=20000))
    tbl = CollNetV6.in_dll(ctypes.CDLL(PLUGIN), "ncclCollNetPlugin_v6")
    sup = {}
    for dt in (6, 9, 7):
        s = ctypes.c_int(-1)
        tbl.reduceSupport(dt, 0, ctypes.byref(s))
        sup[dt] = s.value
    h = torch.from_numpy(worker_bucket(rank, N, 1)).to(torch.bfloat16).cuda()
    before = bits_of(h)
    job = C.allreduce_async(h)
    C.wait_for_all_jobs()
    half_status = job.status()
    untouched = bool(np.array_equal(bits_of(h), before))
    xs = [worker_bucket(r, N, 2) for r in range(W)]
    t = torch.from_numpy(xs[rank].copy()).cuda()
    job = C.allreduce_async(t)
    C.wait_for_all_jobs()
    ref = oracle_switch_allreduce(xs, 256, 2)
    fp32_ok = job.status() == C.JOB_FINISHED and bool(np.array_equal(t.cpu().numpy().view(np.uint32),
                                                                      ref.view(np.uint32)))
    C.stop()
    return {"support": sup, "half_status": half_status, "untouched": untouched, "fp32_ok": fp32_ok}


def test_xgmi_backend_refuses_a_bf16_job_and_the_session_goes_on(cuda):
    import uuid
    from mp_ranks import spawn
    from switchml_amd import client as C
    W = 2
    out = spawn(_xgmi_worker, W, ("half-" + uuid.uuid4().hex,), timeout=120, what="xgmi workers, bf16 refusal")
    for rank, res, err in out:
        assert res is not None, (rank, err)
        assert res["support"] == {6: 0, 9: 0, 7: 1}, res
        assert res["half_status"] == C.JOB_FAILED and res["untouched"], res
        assert res["fp32_ok"], res
