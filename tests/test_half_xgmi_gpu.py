"""FLOAT16 / BFLOAT16 jobs through the in-node switch (general.backend = xgmi
with backend.xgmi.half_types = true): W worker processes on cuda:0 exchange
16-bit buckets through each other's planes.

Expectation, per FIFO slice (O.slice_geometry; blocks restart at the slice
start, chunks of max_slice_numel do not move block boundaries):
    expected = narrow_T(oracle_switch_allreduce([widen(x_r) for r], P, T, rounding))
widen = x.float() on the CPU, narrow_T = torch.from_numpy(y32).to(T) (round
to nearest even); the value is narrowed once, at its shard's owner, so every
worker holds the same bits.  Compared with assert_half_equal: raw 16-bit
words, an expected NaN accepts any NaN, at least 99 % of the positions by
bits (the expected tensors here hold no NaN at all; each test asserts a NaN
share of at most 1 % before it compares)."""
import os
import uuid

import numpy as np
import pytest

from oracle import oracle as O
from mp_ranks import spawn

pytestmark = pytest.mark.gpu

XGMI_CASES = [(2, 1, 256, False), (3, 2, 64, False), (4, 4, 1024, False),
              (2, 1, 256, True), (3, 2, 64, True), (5, 2, 1024, True)]    # (W, T, P, push)


def make(typ, rank, n, seed):
    """worker_bucket in the type; buckets of more than 2000 elements get
    zeros, denormal bit patterns and large finite values (fp16: 0x7BFF, which
    sums past the fp16 range, so the narrowing gives +inf) on every rank, an
    inf and a NaN on rank 0."""
    import torch
    from test_half_client_gpu import bits_of, tdtype
    from test_xgmi_switch import worker_bucket
    x = torch.from_numpy(worker_bucket(rank, n, seed)).to(tdtype(typ))
    if n <= 2000:
        return x
    b = bits_of(x).copy()
    b[5:40] = 0
    b[100:110] = 0x7BFF if typ == "fp16" else 0x5F7F
    b[300:330] = np.arange(1, 31, dtype=np.uint16)
    if rank == 0:
        b[1000] = 0x7C00 if typ == "fp16" else 0x7F80
        b[2000] = 0x7E00 if typ == "fp16" else 0x7FC0
    return torch.from_numpy(b.view(np.int16)).view(tdtype(typ))


def expected(xs, P, T, rounding=O.HALF_AWAY):
    import torch
    from test_xgmi_switch import oracle_switch_allreduce
    y32 = oracle_switch_allreduce([x.float().numpy() for x in xs], P, T, rounding)
    exp = torch.from_numpy(y32).to(xs[0].dtype)
    assert exp.numel() == 0 or float(torch.isnan(exp).float().mean()) <= 0.01
    return exp


def check(got, exp):
    """assert_half_equal, but for an empty bucket (nothing to compare)."""
    from test_half_client_gpu import assert_half_equal
    if exp.numel() == 0:
        assert got.numel() == 0
        return
    assert_half_equal(got, exp)


def place(x, where):
    return x.cuda() if where == "device" else x.pin_memory() if where == "pinned" else x


def start(C, rank, W, T, P, session, **kw):
    C.start(C.make_config(backend="xgmi", rank=rank, num_workers=W, num_worker_threads=T, packet_numel=P,
                          max_outstanding_packets=64 * T, mode="bulk", bandwidth=0, device=0, session=session,
                          **kw))


def _allreduce_worker(rank, W, init, typ, T, P, session, cap, push):
    import torch
    from test_half_client_gpu import bits_of
    from switchml_amd import client as C
    start(C, rank, W, T, P, session, max_slice_numel=cap, push=push, half_types=True)
    sizes = [20_011, 1, 3 * cap + 517, 0, 4 * P * W + 5]
    for i, n in enumerate(sizes):
        xs = [make(typ, r, n, i) for r in range(W)]
        x = place(xs[rank].clone(), ("device", "pageable", "pinned")[i % 3])
        inplace = i % 2 == 0
        out = x if inplace else place(torch.zeros_like(xs[rank]), ("device", "pageable", "pinned")[i % 3])
        assert C.allreduce(x, out).status() == C.JOB_FINISHED, (i, n)
        check(out, expected(xs, P, T))
        if not inplace and n:
            assert np.array_equal(bits_of(x), bits_of(xs[rank])), (i, n)      # the input is unchanged
    C.stop()
    return True


@pytest.mark.parametrize("typ", ["fp16", "bf16"])
@pytest.mark.parametrize("W,T,P,push", XGMI_CASES)
def test_half_allreduce_matches_oracle_switch(cuda, W, T, P, push, typ):
    """Device, pageable and pinned tensors, in place and not; one element, an
    empty bucket, a ragged multiple of the shards, and a slice exchanged in
    several chunks of max_slice_numel; T = 2 with an odd numel puts the second
    slice (and its shards' destinations) on an odd element.  Pull and push."""
    cap = 8192 * (P // 64)
    session = "h16-" + uuid.uuid4().hex
    out = spawn(_allreduce_worker, W, (typ, T, P, session, cap, push), timeout=240,
                what=f"xgmi workers W={W}, {typ}")
    for rank, res, err in out:
        assert res is True, (rank, err)
    assert not os.path.exists(f"/dev/shm/switchml-{session}")


def _mixed_worker(rank, W, init, T, P, session, cap, push):
    """fp32, bf16, fp16 and INT32 jobs in flight on one session, the same
    order on every worker: every slice ends in the barrier that protects the
    planes, whatever the next slice's type makes of them."""
    import torch
    from test_xgmi_switch import oracle_switch_allreduce, worker_bucket
    from switchml_amd import client as C
    start(C, rank, W, T, P, session, max_slice_numel=cap, push=push, half_types=True)
    kinds = ["fp32", "bf16", "fp16", "int32", "fp16", "fp32", "int32", "bf16"]
    ins, exps = [], []
    for j, kind in enumerate(kinds):
        n = 20_011 + 7 * j                      # two chunks of `cap` per slice
        if kind == "fp32":
            xs = [worker_bucket(r, n, 40 + j) for r in range(W)]
            ins.append(torch.from_numpy(xs[rank].copy()).cuda())
            exps.append(oracle_switch_allreduce(xs, P, T).view(np.uint32))
        elif kind == "int32":
            xi = [np.random.default_rng(90 + 10 * j + r).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
                  for r in range(W)]
            ins.append(torch.from_numpy(xi[rank].copy()).cuda())
            exps.append(O.bswap32(O.switch_payload([O.bswap32(v) for v in xi])))
        else:
            xs = [make(kind, r, n, 40 + j) for r in range(W)]
            ins.append(xs[rank].clone().cuda())
            exps.append(expected(xs, P, T))
    jobs = [C.allreduce_async(t) for t in ins]
    C.wait_for_all_jobs()
    assert [j.status() for j in jobs] == [C.JOB_FINISHED] * len(jobs)
    for kind, t, exp in zip(kinds, ins, exps):
        if kind in ("fp32", "int32"):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), exp), kind
        else:
            check(t, exp)
    C.stop()
    return True


@pytest.mark.parametrize("push", [False, True], ids=["pull", "push"])
def test_mixed_type_jobs_in_flight(cuda, push):
    W, T, P = 3, 2, 64
    session = "mix-" + uuid.uuid4().hex
    for rank, res, err in spawn(_mixed_worker, W, (T, P, session, 8192, push), timeout=240,
                                what="xgmi workers, mixed types"):
        assert res is True, (rank, err)


def bf16_tie_bucket(n, P, W, seed):
    """A bf16 bucket whose quantized values are mostly exact .5 ties, and
    whose sums survive the narrowing.  test_client_gpu.tie_bucket rounded to
    bf16 keeps almost none: its ties (m + 0.5) W 2^-30 have m up to 2^20, 21
    significant bits against bf16's 8, and a one-unit difference in a sum of
    that size is far below a bf16 ulp.  So the ties are built in bf16
    directly: every block holds a 1.0 (exponent 1, scale 2^30 / W, exact for a
    power-of-two W); at the tie positions — the same on every worker —
    x = +-(m + 0.5) W 2^-30 with m < 64 (2 m + 1 < 128: exact in bf16), so
    x scale = +-(m + 0.5) exactly and the W workers' sum stays below 256
    units, which bf16 holds exactly; elsewhere N(0, 0.25) rounded to bf16."""
    import torch
    rng = np.random.default_rng(seed)
    x = np.clip(rng.standard_normal(n) * 0.25, -0.99, 0.99).astype(np.float32)
    m = rng.integers(0, 64, n)
    ties = ((m + 0.5) * W * 2.0 ** -30 * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    sel = np.random.default_rng(12345).random(n) < 0.6
    x[sel] = ties[sel]
    x[::P] = 1.0
    t = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy()[sel], x[sel])       # the ties are exact in bf16
    return t


def _vcl_worker(rank, W, init, T, P, session, push):
    import torch
    from test_half_client_gpu import bits_of
    from switchml_amd import client as C
    start(C, rank, W, T, P, session, push=push, half_types=True, vcl=True)
    for i, n in enumerate([20_011, 3 * P + 5]):
        xs = [bf16_tie_bucket(n, P, W, 1000 * i + r) for r in range(W)]
        t = xs[rank].clone().cuda()
        C.allreduce(t)
        ref = expected(xs, P, T, rounding=O.RNE_VCL)
        check(t, ref)
        if i == 0:   # the flag demonstrably reached the typed K3: half away gives other bits
            away = expected(xs, P, T)
            assert int((bits_of(ref) != bits_of(away)).sum()) > n // 100
    C.stop()
    return True


@pytest.mark.parametrize("push", [False, True], ids=["pull", "push"])
def test_vcl_rounding_reaches_the_typed_quantizer(cuda, push):
    """backend.hip.vcl = true: bit-exact against the oracle switch with the
    reference's VCL=1 rounding, on bf16 buckets built of ties (bf16_tie_bucket
    says why test_client_gpu.tie_bucket rounded to bf16 would not do)."""
    W, T, P = 2, 1, 256
    session = "hvcl-" + uuid.uuid4().hex
    for rank, res, err in spawn(_vcl_worker, W, (T, P, session, push), timeout=240, what="xgmi workers, vcl"):
        assert res is True, (rank, err)


def _plugin_worker(rank, W, init, session):
    import ctypes
    import torch
    ini = ("[general]\nbackend = xgmi\nrank = %d\nnum_workers = %d\nnum_worker_threads = 2\npacket_numel = 256\n"
           "max_outstanding_packets = 128\n[backend.dummy]\nbandwidth = 0\n[backend.hip]\nmode = bulk\n"
           "device = 0\n[backend.xgmi]\nsession = %s\nhalf_types = true\n" % (rank, W, session))
    os.environ["SWITCHML_CONFIG_INI"] = ini
    os.environ.pop("SWITCHML_COLLNET_LOOPBACK", None)
    from switchml_amd.collnet import CollNetComm, CollNetV6, NCCL_BFLOAT16, NCCL_FLOAT16
    from test_collnet_plugin import PLUGIN
    comm = CollNetComm(nranks=W, rank=rank)
    tbl = CollNetV6.in_dll(ctypes.CDLL(PLUGIN), "ncclCollNetPlugin_v6")
    sup = {}
    for dt in (6, 9, 7):
        s = ctypes.c_int(-1)
        tbl.reduceSupport(dt, 0, ctypes.byref(s))
        sup[dt] = s.value
    assert sup == {6: 1, 9: 1, 7: 1}, sup
    for typ, code, n in (("bf16", NCCL_BFLOAT16, 5_896_232), ("fp16", NCCL_FLOAT16, 1000)):
        xs = [make(typ, r, n, 7) for r in range(W)]
        send = xs[rank].clone().cuda()
        recv = torch.zeros_like(send)
        torch.cuda.synchronize()                # ready when posted, as RCCL's proxy sees them
        sizes = comm.allreduce_buckets([(send.data_ptr(), recv.data_ptr(), n)], code)
        assert sizes == [2 * n], sizes
        check(recv, expected(xs, 256, 2))
    comm.close()
    from switchml_amd import client as C
    C.stop()
    return True


def test_plugin_offers_and_runs_16_bit_buckets(cuda):
    """With half_types the CollNet plugin answers reduceSupport(ncclFloat16 /
    ncclBfloat16, sum) with 1 and posts such buckets as FLOAT16 / BFLOAT16
    jobs: a ResNet-50 DDP bucket's element count in bf16 and a small fp16 one."""
    session = "hplug-" + uuid.uuid4().hex
    for rank, res, err in spawn(_plugin_worker, 2, (session,), timeout=240, what="xgmi workers, plugin"):
        assert res is True, (rank, err)


def _disagreeing_worker(rank, W, init, session):
    import time
    from switchml_amd import client as C
    t0 = time.time()
    try:
        start(C, rank, W, 1, 256, session, timeout_ms=30000, half_types=rank != 1)
    except C.ContextError as e:
        return {"started": False, "error": str(e), "seconds": time.time() - t0}
    C.stop()
    return {"started": True, "error": "", "seconds": time.time() - t0}


def test_workers_disagreeing_on_half_types_fail_setup_together(cuda):
    """Worker 1 without half_types in a session whose worker 0 has it: a
    configuration error, reported by C.start on both workers with the key's
    name — neither starts, neither waits out a barrier."""
    session = "hdis-" + uuid.uuid4().hex
    out = {rank: res for rank, res, err in spawn(_disagreeing_worker, 2, (session,), timeout=120,
                                                 what="xgmi workers, half_types disagreement")}
    assert set(out) == {0, 1} and all(v is not None for v in out.values()), out
    for rank in (0, 1):
        assert out[rank]["started"] is False, out
        assert "workers disagree" in out[rank]["error"] and "half_types" in out[rank]["error"], out
        assert out[rank]["seconds"] < 20, out      # no 30 s barrier timeout waited out
    assert not os.path.exists(f"/dev/shm/switchml-{session}")
