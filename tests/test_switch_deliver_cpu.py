"""CPU tests of the frame switch's egress and ingress (no GPU needed): the
sequential model of tests/switch_deliver_model.py against SwitchModel's own
result frames, its ring order, overflow and closed loop, and the host-side
contract of sml_frame_switch_deliver / sml_frame_gather — every argument
check, which returns before any HIP call."""
import ctypes

import numpy as np
import pytest

import switch_deliver_model as D
import switch_frames_model as M
from switchml_amd import frame_wire as FW


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def int32_sets(seed, W, N, mop, P):
    """W workers' INT32 slices as tx frame sets built by the model's
    worker_frame: (xs, sets)."""
    rng = np.random.default_rng(seed)
    workers = M.default_workers(W)
    xs = [rng.integers(-2 ** 31, 2 ** 31, N * P, dtype=np.int64).astype(np.int32) for _ in range(W)]
    sets = [[M.worker_frame(P, workers[w], p, M.pool_index(p, mop),
                            xs[w][p * P:(p + 1) * P].astype(">i4").view(np.uint8), src_port=4000 + w)
             for p in range(N)] for w in range(W)]
    return xs, sets


@pytest.mark.parametrize("W", [1, 2, 5, 32])
def test_broadcast_copy_is_the_switch_models_result(W):
    P, S = 64, 4
    workers = M.default_workers(W)
    model = M.SwitchModel(workers, S, P)
    rng = np.random.default_rng(W)
    frames = [M.worker_frame(P, workers[w], 3, 0x8002, rng.integers(0, 256, 4 * P, dtype=np.uint8), (w, 1),
                             src_port=4000 + w) for w in range(W)]
    verdicts, results, _ = M.model_call(model, frames)
    assert verdicts.tolist() == [M.CONSUMED] * (W - 1) + [M.BROADCAST]
    last = W - 1
    appended, counts, fill = D.deliver(model, frames, verdicts, results, None, [0] * W, 4)
    assert counts == [W, 0, 0, 0] and fill == [1] * W
    for u in range(W):
        want = model.result(frames[last], u, 2, 1)
        assert np.array_equal(appended[u][0], want), u
        assert M.ipv4_checksum(appended[u][0][FW.IP_HEADER]) == 0
    assert np.array_equal(appended[last][0], results[last])           # the addressee's copy: byte for byte


def test_retransmit_reaches_only_its_asker():
    P, W = 64, 3
    workers = M.default_workers(W)
    model = M.SwitchModel(workers, 2, P)
    pay = np.arange(4 * P, dtype=np.uint8)
    frames = [M.worker_frame(P, workers[w], 0, 0, pay, src_port=4000 + w) for w in range(W)]
    frames.append(M.worker_frame(P, workers[1], 0, 0, pay, src_port=777))
    verdicts, results, _ = M.model_call(model, frames)
    assert verdicts.tolist() == [0, 0, 1, 2]
    appended, counts, fill = D.deliver(model, frames, verdicts, results, None, [0] * W, 8)
    assert fill == [1, 2, 1] and counts == [4, 0, 0, 0]
    assert appended[1][1] is results[3]                               # unchanged
    # an answer to nobody the table knows
    stray = results[3].copy()
    stray[FW.DST_IP] = [10, 9, 9, 9]
    appended, counts, fill = D.deliver(model, frames[3:], verdicts[3:], {0: stray}, None, [0] * W, 8)
    assert fill == [0, 0, 0] and counts == [0, 0, 0, 1]


def synthetic_call(rng, model, n):
    """n input positions with random verdicts over all five values; a result
    frame (pkt_id = its index) wherever the verdict has one."""
    P, W = model.P, model.W
    verdicts = rng.integers(0, 5, n).astype(np.uint8)
    frames, results = [None] * n, {}
    for i in range(n):
        if verdicts[i] in (M.BROADCAST, M.RETRANSMIT):
            w = int(rng.integers(0, W))
            f = M.worker_frame(P, (model.workers[w][0], "10.0.1.%d" % (w + 1)), i, 0,
                               rng.integers(0, 256, 4 * P, dtype=np.uint8))
            results[i] = model.result(f, w, 0, 0)
    return frames, verdicts, results


def test_ring_order():
    P, W, n = 64, 4, 200
    model = M.SwitchModel(M.default_workers(W), 4, P)
    rng = np.random.default_rng(21)
    frames, verdicts, results = synthetic_call(rng, model, n)
    drop = rng.integers(0, 1 << W, n) & rng.integers(0, 1 << W, n)     # about a quarter of the bits
    appended, counts, fill = D.deliver(model, frames, verdicts, results, drop, [0] * W, n)
    total = 0
    for u in range(W):
        want = [i for i in range(n) if not (drop[i] >> u) & 1 and
                (verdicts[i] == M.BROADCAST or (verdicts[i] == M.RETRANSMIT and D.asker(model, results[i]) == u))]
        assert [D.pkt_id(f) for f in appended[u]] == want
        assert all(FW.get(f, FW.DST_MAC) == model.workers[u][0] and FW.get(f, FW.DST_IP) == model.workers[u][1]
                   for f in appended[u])
        total += len(want)
    copies = sum(W if v == M.BROADCAST else 1 for v in verdicts if v in (M.BROADCAST, M.RETRANSMIT))
    assert counts == [total, copies - total, 0, 0] and fill == [len(a) for a in appended]


def test_overflow_drops_the_highest_indices():
    P, W, n = 64, 3, 60
    model = M.SwitchModel(M.default_workers(W), 4, P)
    rng = np.random.default_rng(22)
    frames, verdicts, results = synthetic_call(rng, model, n)
    full, _, fill_all = D.deliver(model, frames, verdicts, results, None, [0] * W, n)
    cap = max(fill_all)
    start = [0, cap - 3, 2]                                            # ring 1 overflows, ring 0 cannot
    room = [cap - s for s in start]
    assert fill_all[1] > 3
    appended, counts, fill = D.deliver(model, frames, verdicts, results, None, start, cap)
    for u in range(W):
        assert [D.pkt_id(f) for f in appended[u]] == [D.pkt_id(f) for f in full[u][:room[u]]]
    assert fill == [min(s + n_u, cap) for s, n_u in zip(start, fill_all)]
    kept = sum(len(a) for a in appended)
    assert counts == [kept, 0, sum(fill_all) - kept, 0] and counts[D.OVERFLOW] >= fill_all[1] - 3 > 0


def test_gather_model():
    sets = [[np.full(4, 10 * s + i, dtype=np.uint8) for i in range(3)] for s in range(2)]
    out, skipped = D.gather(sets, [1, 0, 2, 1, 1], [2, 0, 0, 3, 2])
    assert skipped == 2 and out[2] is None and out[3] is None
    assert [int(o[0]) for o in out if o is not None] == [12, 0, 12]


@pytest.mark.parametrize("seed", D.LOSSY_SEEDS)
def test_lossy_loop_finishes_on_the_model(seed):
    """The seeds of the GPU's closed loop: the model alone finishes inside the
    cap, without a ring overflowing, and every worker's ring holds every
    packet's wrapping sum."""
    c = D.LOSSY
    xs, sets = int32_sets(seed, c["W"], c["N"], c["mop"], c["P"])
    switch = D.ModelSwitch(sets, M.default_workers(c["W"]), c["mop"], c["P"], c["ring_frames"])
    ncalls = D.lossy_loop(seed, c["W"], c["N"], c["mop"], c["q"], switch)
    assert 0 < ncalls <= 100 * c["N"] * c["W"]
    assert switch.counts[D.OVERFLOW] == 0 and switch.counts[D.UNROUTABLE] == 0 and switch.counts[D.DROPPED] > 0
    assert switch.verdicts[M.BROADCAST] == c["N"] and switch.verdicts[M.RETRANSMIT] > 0
    assert switch.verdicts[M.DEFERRED] > 0                            # resubmission by index is on the path
    want = (xs[0].astype(np.int64) + xs[1] + xs[2]).astype(np.uint32)
    for u in range(c["W"]):
        got = {}
        for f in switch.rings[u]:
            got.setdefault(D.pkt_id(f), FW.payload_words(f, c["P"]))
        assert sorted(got) == list(range(c["N"]))
        assert all(np.array_equal(got[p], want[p * c["P"]:(p + 1) * c["P"]]) for p in got)


# ------------------------------------------------------------ the C entry points

def test_deliver_argument_checks_without_gpu(sw):
    L = sw.lib()
    vp = ctypes.c_void_p
    f = L.sml_frame_switch_deliver
    INV, UNS, ALN, OK = sw.SML_ERR_INVALID_ARG, sw.SML_ERR_UNSUPPORTED, sw.SML_ERR_ALIGNMENT, sw.SML_OK

    def params(W=2, P=64):
        sp = sw.frame_switch_params(M.default_workers(min(W, 32)), 4, P)
        sp.num_workers = W
        return ctypes.byref(sp)

    fb = FW.frame_bytes(64)
    out, vd, dr, rg, rc, cnt, sc = vp(4096), vp(8192), vp(12288), vp(16384), vp(32768), vp(65536), vp(131072)
    good = dict(prm=None, out=out, n=1, ostr=fb, vd=vd, dr=dr, rg=rg, rb=4 * fb, rf=4, rx=fb, rc=rc, cnt=cnt, sc=sc)

    def call(**kw):
        a = dict(good, **kw)
        prm = a["prm"] if a["prm"] is not None else params()
        return f(prm, a["out"], a["n"], a["ostr"], a["vd"], a["dr"], a["rg"], a["rb"], a["rf"], a["rx"], a["rc"],
                 a["cnt"], a["sc"], None)

    # null
    assert f(None, out, 1, fb, vd, dr, rg, 4 * fb, 4, fb, rc, cnt, sc, None) == INV
    assert call(prm=params(W=0)) == INV
    for name in ("out", "vd", "rg", "rc", "sc"):
        assert call(**{name: None}) == INV, name
    # unsupported: packet size, workers, an empty ring, too many frames — and null wins over them
    assert call(prm=params(P=100)) == UNS
    assert call(prm=params(W=33)) == UNS
    assert call(rf=0) == UNS
    assert call(n=2 ** 31) == UNS
    assert call(prm=params(P=100), out=None) == INV
    assert call(prm=params(P=100), rx=50, rg=vp(16386)) == UNS                # ... over alignment
    # nothing to do: no buffer is looked at, the parameters still are
    assert call(n=0, out=None, vd=None, dr=None, rg=None, rc=None, cnt=None, sc=None) == OK
    assert call(prm=params(P=100), n=0) == UNS
    assert call(n=0, rf=0) == UNS
    # alignment: frames, strides, rings, the ring's size, the device arrays
    assert call(out=vp(4098)) == ALN
    assert call(ostr=fb - 4) == ALN and call(ostr=fb + 2) == ALN
    assert call(rg=vp(16386)) == ALN
    assert call(rx=fb - 4) == ALN and call(rx=fb + 2, rb=8 * fb) == ALN
    assert call(rb=4 * fb - 4) == ALN and call(rb=4 * fb + 2) == ALN
    assert call(rx=fb + 4) == ALN                                             # 4 frames no longer fit ring_bytes
    assert call(rx=fb + 4, rb=4 * fb + 12) == ALN and call(rx=2 ** 62, rb=2 ** 63) == ALN
    assert call(dr=vp(12290)) == ALN
    assert call(rc=vp(32772)) == ALN and call(cnt=vp(65540)) == ALN and call(sc=vp(131080)) == ALN
    # d_drop and d_counts may be absent; the scratch size
    g = L.sml_frame_switch_deliver_scratch_bytes
    assert g(0, 0) == 0 and g(1, 33) == 0 and g(2 ** 31, 2) == 0
    for n, W in [(1, 1), (64, 2), (65, 2), (65537, 32)]:
        groups = (n + 63) // 64
        assert g(n, W) >= 4 * n + 4 * W * groups + 8 * 32 and g(n, W) <= 4 * n + 4 * W * (groups + 3) + 8 * 32 + 16
    assert L.sml_abi_version() == 2


def test_gather_argument_checks_without_gpu(sw):
    L = sw.lib()
    vp = ctypes.c_void_p
    f = L.sml_frame_gather
    INV, UNS, ALN, OK = sw.SML_ERR_INVALID_ARG, sw.SML_ERR_UNSUPPORTED, sw.SML_ERR_ALIGNMENT, sw.SML_OK
    fb = FW.frame_bytes(64)

    def sets(*ptrs):
        return (vp * len(ptrs))(*ptrs)

    two = sets(4096, 8192)
    si, fi, dst, sk = vp(16384), vp(32768), vp(65536), vp(131072)
    # null
    assert f(None, 2, 8, fb, si, fi, 1, 64, dst, fb, sk, None) == INV
    assert f(two, 0, 8, fb, si, fi, 1, 64, dst, fb, sk, None) == INV
    assert f(two, 2, 8, fb, None, fi, 1, 64, dst, fb, sk, None) == INV
    assert f(two, 2, 8, fb, si, None, 1, 64, dst, fb, sk, None) == INV
    assert f(two, 2, 8, fb, si, fi, 1, 64, None, fb, sk, None) == INV
    assert f(sets(4096, None), 2, 8, fb, si, fi, 1, 64, dst, fb, sk, None) == INV
    # unsupported
    assert f(two, 2, 8, fb, si, fi, 1, 100, dst, fb, sk, None) == UNS
    assert f(sets(*[4096] * 33), 33, 8, fb, si, fi, 1, 64, dst, fb, sk, None) == UNS
    assert f(two, 2, 8, fb, None, fi, 1, 100, dst, fb, sk, None) == INV       # null wins
    assert f(two, 2, 8, 50, si, fi, 1, 100, dst, fb, sk, None) == UNS         # ... over alignment
    # nothing to do
    assert f(two, 2, 8, fb, None, None, 0, 64, None, 0, None, None) == OK
    assert f(two, 2, 8, fb, None, None, 0, 100, None, 0, None, None) == UNS
    # alignment
    assert f(sets(4096, 8194), 2, 8, fb, si, fi, 1, 64, dst, fb, sk, None) == ALN
    assert f(two, 2, 8, fb - 4, si, fi, 1, 64, dst, fb, sk, None) == ALN
    assert f(two, 2, 8, fb + 2, si, fi, 1, 64, dst, fb, sk, None) == ALN
    assert f(two, 2, 8, fb, si, fi, 1, 64, vp(65538), fb, sk, None) == ALN
    assert f(two, 2, 8, fb, si, fi, 1, 64, dst, fb - 4, sk, None) == ALN
    assert f(two, 2, 8, fb, si, fi, 1, 64, dst, fb + 2, sk, None) == ALN
    assert f(two, 2, 8, fb, vp(16386), fi, 1, 64, dst, fb, sk, None) == ALN
    assert f(two, 2, 8, fb, si, vp(32772), 1, 64, dst, fb, sk, None) == ALN
    assert f(two, 2, 8, fb, si, fi, 1, 64, dst, fb, vp(131076), None) == ALN
