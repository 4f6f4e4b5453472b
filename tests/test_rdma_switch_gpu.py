"""GPU tests of the RDMA switch (sml_rdma_switch / switchml_amd.RdmaSwitch,
DESIGN §9 F4 "Switch side"): every call's verdicts, immediates, counts and
the workers' whole receive regions — sentinel-prefilled, like the verdict and
immediate buffers, so that a stray write shows — are compared bit for bit
with the sequential model of tests/rdma_switch_model.py."""
import numpy as np
import pytest

import rdma_switch_model as R
import switch_deliver_model as D
from oracle import oracle as O
from test_rdma_switch_cpu import LOSSY, LOSSY_SEEDS, lossy_inputs

pytestmark = pytest.mark.gpu

SENTINEL, SENTINEL32 = 0x5A, 0x5A5A5A5A
E0, E1 = (3, -5, 100, -128), (-7, 9, -100, 127)              # both signs, in each byte on its own


@pytest.fixture(scope="module")
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


class Pair:
    """The GPU switch and the model, side by side, over receive regions that persist across calls."""

    def __init__(self, sw, W, S, M, ppm, rx_bytes, pinned=False):
        import torch
        self.gpu, self.model = sw.RdmaSwitch(W, S, M, ppm), R.RdmaSwitchModel(W, S, M, ppm)
        self.place = (lambda t: t.pin_memory()) if pinned else (lambda t: t.cuda())
        self.rx = self.place(torch.full((W, rx_bytes), SENTINEL, dtype=torch.uint8))
        self.rx_model = np.full((W, rx_bytes), SENTINEL, dtype=np.uint8)
        self.counts = np.zeros(6, dtype=np.int64)

    def reset(self):
        self.gpu.reset()
        self.model.reset()
        self.counts[:] = 0

    def check(self, recs, landing, drop=None):
        """One call on both; everything compared.  Returns the verdicts."""
        import torch
        n = len(recs)
        verdicts, imms, counts = R.model_call(self.model, recs, landing, self.rx_model, drop)
        self.counts += counts
        d_verdict = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        d_imm = torch.full((n,), SENTINEL32, dtype=torch.int32, device="cuda")
        d_drop = None if drop is None else torch.from_numpy(drop.astype(np.uint32).view(np.int32)).cuda()
        got_v, got_imm = self.gpu.step(recs, self.place(torch.from_numpy(landing)), self.rx, d_drop,
                                       verdict=d_verdict, out_imm=d_imm)
        torch.cuda.synchronize()
        assert got_v.cpu().numpy().tolist() == verdicts.tolist()
        want = np.full(n, SENTINEL32, dtype=np.uint32)
        want[list(imms)] = list(imms.values())
        assert np.array_equal(got_imm.cpu().numpy().view(np.uint32), want)
        assert np.array_equal(self.rx.cpu().numpy(), self.rx_model)
        assert self.gpu.counts.tolist() == self.counts.tolist()
        return verdicts


def window(rng, W, mop, M, ppm, set_, stride=None):
    """A record per (worker, slot), shuffled; every payload byte random, the bytes past a message too."""
    landing = rng.integers(0, 256, (W * mop, stride or 4 * M), dtype=np.uint8)
    rows = [(w, R.rkey(s, set_, ppm), R.imm(s + 7, E0[(w + s) % 4], E1[(w // 2 + s) % 4]), w * mop + s, s * 4 * M)
            for w in range(W) for s in range(mop)]
    return R.arrivals([rows[i] for i in rng.permutation(len(rows))]), landing


def cuts_and_reuse(sw, M, W, ppm, **kw):
    rng = np.random.default_rng(M + W + ppm)
    mop, stride, dropped = 2, kw.pop("stride", None), 0
    pair = Pair(sw, W, mop, M, ppm, mop * 4 * M, **kw)
    recs, landing = window(rng, W, mop, M, ppm, 0, stride)
    sums = landing[:, :4 * M].view(">u4").astype(np.uint64).reshape(W, mop * M).sum(axis=0)
    assert W == 1 or sums.max() > 0xFFFFFFFF                              # the sums wrap
    for cut in range(1, len(recs) + 1):                                  # a slot part-filled by one call
        pair.reset()
        drop = rng.integers(0, 2 ** W, len(recs), dtype=np.uint64) & rng.integers(0, 2 ** W, len(recs), dtype=np.uint64)
        seen = pair.check(recs[:cut], landing, drop[:cut]).tolist()
        if cut < len(recs):
            seen += pair.check(recs[cut:], landing, drop[cut:]).tolist()
        assert seen.count(R.BROADCAST) == mop and seen.count(R.CONSUMED) == len(recs) - mop
        dropped += pair.counts[R.DROPPED]
    assert W == 1 or dropped > 0
    for set_ in (1, 0, 1):                                               # rkey ^= 1: the slots again, other set
        recs, landing = window(rng, W, mop, M, ppm, set_, stride)
        assert pair.check(recs, landing).tolist().count(R.BROADCAST) == mop


@pytest.mark.parametrize("ppm", [1, 4])
@pytest.mark.parametrize("W", [1, 2, 32])
@pytest.mark.parametrize("M", [64, 256, 1024])
def test_slots_filled_across_calls_at_every_cut_then_reused(sw, M, W, ppm):
    cuts_and_reuse(sw, M, W, ppm)


def test_pinned_host_memory_and_a_stride_past_the_message(sw):
    cuts_and_reuse(sw, 256, 3, 1, pinned=True, stride=4 * 256 + 48)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_record_counts_around_the_claim_workgroup(sw, n):
    W, mop, M, ppm = 4, 64, 64, 2
    pair = Pair(sw, W, mop, M, ppm, mop * 4 * M)
    recs, landing = window(np.random.default_rng(n), W, mop, M, ppm, 1)
    verdicts = pair.check(np.concatenate([recs, recs[:1]])[:n], landing)
    assert verdicts.tolist().count(R.BROADCAST) == (mop if n > 255 else mop - 1)


def test_duplicates_deferral_and_every_ignored_cause(sw):
    W, S, M, ppm = 2, 2, 64, 4
    pair = Pair(sw, W, S, M, ppm, 2 * 4 * M)
    landing = np.random.default_rng(3).integers(0, 256, (4, 4 * M), dtype=np.uint8)
    k0, k1 = R.rkey(0, 0, ppm), R.rkey(0, 1, ppm)
    rows = [(0, k0, R.imm(1, -3, 4), 0, 0), (0, k0, R.imm(2), 0, 0),           # a duplicate before completion
            (1, k0, R.imm(3, 5, -6), 1, 256), (1, k0, R.imm(4), 1, 0),       # ... and after: answered
            (0, k1, R.imm(5), 2, 0),                                         # the pair's other set
            (0, k0 + 2, 0, 0, 0), (0, R.rkey(2, 0, ppm), 0, 0, 0), (2, k0, 0, 0, 0), (0, k0, 0, 4, 0),
            (0, k0, 0, 0, 8), (0, k0, 0, 0, 4 * M + 16)]
    verdicts = pair.check(R.arrivals(rows), landing, np.array([0, 0, 2, 0] + [0] * 7, dtype=np.uint32))
    assert verdicts.tolist() == [R.CONSUMED, R.CONSUMED, R.BROADCAST, R.RETRANSMIT, R.DEFERRED] + [R.IGNORED] * 6
    assert pair.counts[R.DROPPED] == 1 and np.all(pair.rx_model[1, 256:] == SENTINEL)
    assert pair.check(R.arrivals(rows[4:5]), landing).tolist() == [R.CONSUMED]    # resubmitted: NULL d_drop


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "int32"])
def test_end_to_end_against_the_plane_oracle(sw, dtype):
    """W workers: sml_quantize_pack_typed at P = 1024 (INT32: the byte swap) and
    sml_rdma_imm -> RdmaSwitch.step -> sml_dequantize_typed of each worker's own
    receive region with the exponents from out_imm.  Floats take two phases:
    own exponents first, the maxed ones back in the immediates."""
    import torch
    W, M, ppm = 3, 1024, 4
    n = 3 * M + 7
    B = O.num_blocks(n, M)
    gpu = sw.RdmaSwitch(W, B, M, ppm)
    rx = torch.zeros((W, B * 4 * M), dtype=torch.uint8, device="cuda")

    def switch(planes, imms, set_):
        recs = R.arrivals([(w, R.rkey(m, set_, ppm), int(imms[w][m]) & 0xFFFFFFFF, w * B + m, m * 4 * M)
                           for m in range(B) for w in range(W)])
        verdict, out_imm = gpu.step(recs, torch.stack(planes).view(W * B, M), rx.view(torch.int32))
        assert verdict.tolist() == ([R.CONSUMED] * (W - 1) + [R.BROADCAST]) * B
        return out_imm[W - 1::W]

    if dtype == "int32":
        rng = np.random.default_rng(11)
        xs = [rng.integers(-2 ** 31, 2 ** 31, B * M, dtype=np.int64).astype(np.int32) for _ in range(W)]
        imms = [sw.rdma_imm(None, num_blocks_int32=B).cpu().numpy() for _ in range(W)]
        out_imm = switch([sw.bswap_i32(torch.from_numpy(x).cuda()) for x in xs], imms, 0)
        assert out_imm.tolist() == list(range(B))
        for u in range(W):
            assert np.array_equal(sw.bswap_i32(rx[u].view(torch.int32)).cpu().numpy(), xs[0] + xs[1] + xs[2])
        return
    tdt = getattr(torch, dtype)
    xd = [torch.from_numpy(O.splitmix_normal(40 + w, n) * np.float32(4.0 ** w)).cuda().to(tdt) for w in range(W)]
    xs = [x.float().cpu().numpy() for x in xd]                       # what the kernels widen to
    own = [sw.quantize_pack(x, M, W) for x in xd]
    out_imm = switch([p for p, _ in own], [sw.rdma_imm(e).cpu().numpy() for _, e in own], 0)
    gexp = ((out_imm >> 16) & 0xFF).to(torch.uint8).view(torch.int8)
    want_exps = O.switch_exps([O.exponents(x, M) for x in xs])
    assert np.array_equal(gexp.cpu().numpy(), want_exps) and len({tuple(e.tolist()) for _, e in own}) == W
    glob = [sw.quantize_pack(x, M, W, global_exps=gexp) for x in xd]
    switch([p for p, _ in glob], [sw.rdma_imm(gexp).cpu().numpy()] * W, 1)
    want = O.dequantize(O.switch_payload([O.quantize(x, M, W, global_exps=want_exps) for x in xs]), want_exps, n, M, W)
    want = torch.from_numpy(want).to(tdt)
    for u in range(W):
        got = sw.dequantize(rx[u].view(torch.int32), gexp, n, M, W, out_dtype=tdt)
        assert torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8)), u


@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_lossy_closed_loop(sw, seed):
    """INT32, W = 3, 40 messages, window 8, loss 0.1 each way and duplication 0.1
    inbound: workers in host Python that see only verdicts and out_imm."""
    import torch
    c, xs = LOSSY, lossy_inputs(seed)
    gpu = sw.RdmaSwitch(c["W"], c["mop"], c["M"], c["ppm"])
    rx = torch.zeros((c["W"], c["N"] * 4 * c["M"]), dtype=torch.uint8, device="cuda")

    def step(recs, drop):
        verdict, out_imm = gpu.step(recs, landing, rx, torch.from_numpy(drop.view(np.int32)).cuda())
        return verdict.cpu().numpy(), out_imm.cpu().numpy()

    loop = R.ClosedLoop(step, xs, c["mop"], c["M"], c["ppm"])
    landing = torch.from_numpy(loop.landing).cuda()
    D.lossy_loop(seed, c["W"], c["N"], c["mop"], c["q"], loop)
    assert loop.verdicts[R.RETRANSMIT] > 0 and loop.verdicts[R.DEFERRED] > 0
    assert gpu.counts[:5].tolist() == loop.verdicts and gpu.counts[5] > 0
    for r in rx.cpu().numpy():
        assert np.array_equal(r.view(">i4").astype(np.int32), xs[0] + xs[1] + xs[2])
