"""GPU tests of the RDMA switch for long messages (sml_msg_switch, reached
through switchml_amd.RdmaSwitch: DESIGN §9 F4 "Switch side", long messages),
with the harness of tests/test_rdma_switch_gpu.py: every call's verdicts,
immediates, counts and whole receive regions bit for bit against the sequential
model of tests/rdma_switch_model.py, which is general in M and pkts_per_msg."""
import numpy as np
import pytest

import rdma_switch_model as R
from oracle import oracle as O
from test_rdma_switch_gpu import SENTINEL, Pair, cuts_and_reuse, sw, window  # noqa: F401 (sw: the fixture)

pytestmark = pytest.mark.gpu

# (M, W, pkts_per_msg): the smallest shapes at which the item geometry can go wrong
GEOMETRY = [(192, 2, 3),         # one item, 48 lanes
            (1024, 3, 3),        # the long path at a size the old path serves too
            (1088, 3, 17),       # the second item is one 16-lane slice
            (1280, 2, 5),        # 5 slices over 2 items
            (1984, 2, 31),       # the last slice is 48 lanes
            (2304, 32, 9),       # every worker: 16 rounds of contributor loads
            (4160, 3, 65),       # 17 slices dealt over 5 items
            (16384, 3, 256)]     # the longest message


@pytest.mark.parametrize("M,W,ppm", GEOMETRY)
def test_slots_filled_across_calls_at_every_cut_then_reused(sw, M, W, ppm):
    cuts_and_reuse(sw, M, W, ppm)


def test_retransmit_from_the_state_deferral_and_every_ignored_cause(sw):
    W, S, M, ppm = 2, 2, 2304, 9
    pair = Pair(sw, W, S, M, ppm, 2 * 4 * M)
    landing = np.random.default_rng(9).integers(0, 256, (4, 4 * M), dtype=np.uint8)
    k0, k1 = R.rkey(0, 0, ppm), R.rkey(0, 1, ppm)
    rows = [(0, k0, R.imm(1, -3, 4), 0, 0), (1, k0, R.imm(2, 5, -6), 1, 0)]   # worker 0's copy of the result is lost
    assert pair.check(R.arrivals(rows), landing, np.array([0, 1], dtype=np.uint32)).tolist() == [R.CONSUMED, R.BROADCAST]
    assert pair.counts[R.DROPPED] == 1 and np.all(pair.rx_model[0] == SENTINEL)
    rows = [(0, k0, R.imm(3), 0, 4 * M),                                     # the resend: no contributor in this call
            (0, k1, R.imm(4), 2, 0),                                         # the pair's other set
            (0, k0 + 2, 0, 0, 0), (0, R.rkey(2, 0, ppm), 0, 0, 0), (0, k0, 0, 0, 4 * M + 16), (0, k0, 0, 0, 8),
            (0, k0, 0, 4, 0)]
    assert pair.check(R.arrivals(rows), landing).tolist() == [R.RETRANSMIT, R.DEFERRED] + [R.IGNORED] * 5
    assert np.array_equal(pair.rx_model[0, 4 * M:], pair.rx_model[1, :4 * M]) and np.all(pair.rx_model[0, :4 * M] == SENTINEL)


def test_grid_stride_over_items(sw):
    W, S, M, ppm = 2, 64, 1280, 5                                            # 128 items over 8 waves
    pair = Pair(sw, W, S, M, ppm, S * 4 * M)
    recs, landing = window(np.random.default_rng(1), W, S, M, ppm, 0)
    old = sw.set_grid_limit(2)
    try:
        verdicts = pair.check(recs, landing)
    finally:
        sw.set_grid_limit(old)
    assert verdicts.tolist().count(R.BROADCAST) == S


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_end_to_end_against_the_plane_oracle(sw, dtype):
    """W workers: msg_quantize_pack and rdma_imm -> RdmaSwitch.step -> msg_dequantize of each worker's own receive
    region, in two phases: own exponents first, the maxed ones back in the immediates."""
    import torch
    W, M, ppm = 3, 2304, 9
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

    tdt = getattr(torch, dtype)
    xd = [torch.from_numpy(O.splitmix_normal(40 + w, n) * np.float32(4.0 ** w)).cuda().to(tdt) for w in range(W)]
    xs = [x.float().cpu().numpy() for x in xd]                       # what the kernels widen to
    own = [sw.msg_quantize_pack(x, M, W) for x in xd]
    out_imm = switch([p for p, _ in own], [sw.rdma_imm(e).cpu().numpy() for _, e in own], 0)
    gexp = ((out_imm >> 16) & 0xFF).to(torch.uint8).view(torch.int8)
    want_exps = O.switch_exps([O.exponents(x, M) for x in xs])
    assert np.array_equal(gexp.cpu().numpy(), want_exps) and len({tuple(e.tolist()) for _, e in own}) == W
    glob = [sw.msg_quantize_pack(x, M, W, global_exps=gexp) for x in xd]
    switch([p for p, _ in glob], [sw.rdma_imm(gexp).cpu().numpy()] * W, 1)
    want = O.dequantize(O.switch_payload([O.quantize(x, M, W, global_exps=want_exps) for x in xs]), want_exps, n, M, W)
    want = torch.from_numpy(want).to(tdt)
    for u in range(W):
        got = sw.msg_dequantize(rx[u].view(torch.int32), gexp, n, M, W, out_dtype=tdt)
        assert torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8)), u
