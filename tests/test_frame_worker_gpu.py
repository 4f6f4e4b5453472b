"""GPU tests of the DPDK worker's receive loop (sml_frame_worker_* / FrameWorker, DESIGN §9 F3 "Worker side"):
W workers around one FrameSwitch as a chain of launches, outputs bit for bit against the plane oracle (INT32: the
wrapping sum), every emitted frame byte for byte against the oracle's bulk frames under the global exponents."""
import numpy as np
import pytest

import switch_frames_model as M
from oracle import oracle as O
from switchml_amd import frame_wire as FW
from test_frame_worker_cpu import LOSSY, LOSSY_SEEDS, lossy_loop

pytestmark = pytest.mark.gpu

SENTINEL, JOB = 0x5A, 7
WRONG, POSTED, FINISHED, IGNORED = range(4)
RETRANSMIT = 2


@pytest.fixture(scope="module")
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def inputs(dtype, W, P, n, seed):
    """(the workers' device tensors, the values the kernels widen them to, the oracle's all-reduce in the dtype)."""
    import torch
    if dtype == "int32":
        rng = np.random.default_rng(seed)
        xs = [rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) for _ in range(W)]
        return [torch.from_numpy(x).cuda() for x in xs], xs, torch.from_numpy(sum(xs[1:], xs[0]))
    tdt = getattr(torch, dtype)
    xd = [torch.from_numpy(O.splitmix_normal(seed + w, n) * np.float32(4.0 ** w)).cuda().to(tdt) for w in range(W)]
    xs = [x.float().cpu().numpy() for x in xd]
    exps = O.switch_exps([O.exponents(x, P) for x in xs])
    want = O.dequantize(O.switch_payload([O.quantize(x, P, W, global_exps=exps) for x in xs]), exps, n, P, W)
    return xd, xs, torch.from_numpy(want).to(tdt)


class Loop:
    """W workers around one switch: tx rings [W, Q, stride], receive rings [W, R, stride]."""

    def __init__(self, sw, dtype, W, P, Q, ring, pad=0):
        import torch
        self.sw, self.W, self.P, self.Q, self.R, self.tdt = sw, W, P, Q, ring, getattr(torch, dtype)
        self.fb, self.stride = M.frame_bytes(P), M.frame_bytes(P) + pad
        workers = M.default_workers(W)
        self.switch = sw.FrameSwitch(workers, Q, P, switch_mac=M.SWITCH_MAC, switch_ip=M.SWITCH_IP)
        self.workers = [sw.FrameWorker(sw.frame_params(
            dst_mac=M.SWITCH_MAC, src_mac=mac, src_ip=ip, dst_ip=M.SWITCH_IP, src_port=4000 + w, job_id=JOB,
            max_outstanding_pkts=Q), W, P, dtype=self.tdt) for w, (mac, ip) in enumerate(workers)]
        self.tx, self.rings = (torch.full((W, k, self.stride), SENTINEL, dtype=torch.uint8, device="cuda")
                               for k in (Q, ring))
        self.set_idx = {k: torch.arange(W, dtype=torch.int32, device="cuda").repeat_interleave(k) for k in (Q, ring)}

    def begin(self, xs, outs):
        return [wk.begin(x, o, self.tx[w].reshape(-1), self.stride) for w, (wk, x, o) in enumerate(zip(self.workers, xs, outs))]

    def step(self, set_idx, frame_idx, drop=None):
        """gather -> switch -> deliver -> every worker's poll: (verdicts, sends) per worker, all on the device."""
        n = frame_idx.numel()
        frames, _ = self.sw.gather_frames(list(self.tx), set_idx, frame_idx, self.P, set_frames=self.Q,
                                          set_stride=self.stride)
        out, verdict, _ = self.switch(frames, n)
        self.switch.reset_rings()
        self.switch.deliver(out, verdict, n, rings=self.rings, drop=drop)
        return [wk.poll(self.rings[w].reshape(-1), self.R, self.tx[w].reshape(-1), self.switch.ring_count[w:w + 1],
                        self.stride, self.stride) for w, wk in enumerate(self.workers)]

    def emitted(self, w, slots):
        """{pkt_id: frame} of worker w's tx slots `slots`, read now."""
        fr = self.tx[w].cpu().numpy()[np.asarray(slots, dtype=np.int64), :self.fb]
        return {int(FW.get(f, FW.PKT_ID)): f for f in fr}

    def want_frames(self, xs):
        """Every worker's B + b frames as the bulk tx builds them under the global exponents (after begin: the shift)."""
        if xs[0].dtype == np.int32:
            return [O.build_frames_i32(x, wk.params.frame, self.P).reshape(-1, self.fb) for x, wk in
                    zip(xs, self.workers)]
        exps = O.switch_exps([O.exponents(x, self.P) for x in xs])
        return [O.build_frames(x, wk.params.frame, self.P, self.W, batch_max=self.Q, global_exps=exps)
                .reshape(-1, self.fb) for x, wk in zip(xs, self.workers)]


def run_slice(loop, dtype, n, seed):
    """One slice on every worker to completion; the host only reads what it checks and counts."""
    import torch
    W, Q = loop.W, loop.Q
    xd, xs, want = inputs(dtype, W, loop.P, n, seed)
    outs = [torch.zeros_like(x) for x in xd]
    sends = loop.begin(xd, outs)
    frames = loop.want_frames(xs)
    total, b = len(frames[0]), min(Q, O.num_blocks(n, loop.P))
    seen = [loop.emitted(w, range(b)) for w in range(W)]
    set_idx = loop.set_idx[Q]
    for _ in range(2 * total):
        polled = loop.step(set_idx, torch.cat(sends))
        sends, set_idx, done = [s for _, s in polled], loop.set_idx[loop.R], 0
        for w, (v, s) in enumerate(polled):
            v, s = v.cpu().numpy(), s.cpu().numpy()
            assert np.all(v[b:] == IGNORED) and np.all(s[v != POSTED] == -1)
            new = loop.emitted(w, s[v == POSTED])
            assert not set(new) & set(seen[w])
            seen[w].update(new)
            done += int(loop.workers[w].counts[POSTED] + loop.workers[w].counts[FINISHED])
        if done == W * total:
            break
    assert done == W * total
    for w in range(W):
        assert sorted(seen[w]) == list(range(total))                      # every pkt_id emitted exactly once
        for p, f in seen[w].items():
            assert np.array_equal(f, frames[w][p]), (w, p)
        assert torch.equal(outs[w].cpu().view(torch.uint8), want.view(torch.uint8)), w
    for wk in loop.workers:
        wk.counts.zero_()


@pytest.mark.parametrize("P,Q,n,W", [(64, 4, 5 * 64 + 7, 3), (128, 3, 7 * 128, 2), (256, 8, 3 * 256, 2),
                                     (1024, 1, 2 * 1024 + 1, 2)])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16", "int32"])
def test_closed_loop_through_the_switch(sw, dtype, P, Q, n, W):
    """Two slices back to back: the shift moves on, the switch is not reset."""
    loop = Loop(sw, dtype, W, P, Q, ring=Q + 2)
    for seed in (40, 50):
        run_slice(loop, dtype, n, seed)
    assert loop.workers[0].params.frame.pool_index_shift == loop.workers[0].total % (2 * Q)


def result_frame(P, pkt_id, payload, exp=0, job=JOB):
    return FW.worker_frame(P, M.default_workers(1)[0], pkt_id, 0, payload, (exp, 0), job=job)


def test_verdict_rules_in_one_call(sw):
    import torch
    P, Q, blocks = 64, 2, 4                                               # b = 2, total = 6
    fb = M.frame_bytes(P)
    rng = np.random.default_rng(9)
    x = torch.from_numpy(O.splitmix_normal(9, blocks * P)).cuda()
    out = torch.full_like(x, float("nan"))
    tx = torch.zeros(Q * fb, dtype=torch.uint8, device="cuda")
    wk = sw.FrameWorker(sw.frame_params(job_id=JOB, max_outstanding_pkts=Q), 1, P)
    ring = lambda frames: torch.from_numpy(np.concatenate(frames)).cuda()       # noqa: E731
    poll = lambda frames, live=None: wk.poll(ring(frames), len(frames), tx, live)        # noqa: E731
    pay = [rng.integers(0, 256, 4 * P, dtype=np.uint8) for _ in range(3)]
    assert wk.begin(x, out, tx).tolist() == [0, 1]
    assert poll([result_frame(P, 0, pay[0], 3), result_frame(P, 1, pay[0], 3)])[0].tolist() == [POSTED, POSTED]
    tx.fill_(SENTINEL)
    frames = [result_frame(P, 2, pay[1], 5, job=JOB + 1), result_frame(P, 0, pay[1], 5), result_frame(P, 4, pay[1], 5),
              result_frame(P, 6, pay[1], 5), result_frame(P, 2, pay[1], 5), result_frame(P, 2, pay[2], 6),
              result_frame(P, 3, pay[2], 6), result_frame(P, 3, pay[2], 6)]
    verdict, sends = poll(frames, torch.tensor([6], device="cuda"))       # the last two lie past the live count
    assert verdict.tolist() == [WRONG] * 4 + [POSTED, WRONG, IGNORED, IGNORED]
    assert sends.tolist() == [-1] * 4 + [0] + [-1] * 3
    # packet 2 on slot 0: block 0 out of the first copy under the kept exponent 3, frame 4 = block 2 under the received 5
    got = out.cpu().numpy()
    want = O.dequantize(pay[1].view(np.uint32), np.array([3], np.int8), P, P, 1)
    assert np.array_equal(got[:P].view(np.uint32), want.view(np.uint32)) and np.isnan(got[P:]).all()
    bulk = O.build_frames(x.cpu().numpy(), wk.params.frame, P, 1, batch_max=Q,
                          global_exps=np.array([3, 3, 5, 0], np.int8)).reshape(-1, fb)
    after = tx.cpu().numpy().reshape(Q, fb)
    assert np.array_equal(after[0], bulk[4]) and np.all(after[1] == SENTINEL)
    assert wk.resend([1, 0, 5]).tolist() == [1, 0, -1]
    assert poll([result_frame(P, 3, pay[2], 6)])[0].tolist() == [POSTED]
    assert np.array_equal(tx.cpu().numpy().reshape(Q, fb)[1], O.build_frames(
        x.cpu().numpy(), wk.params.frame, P, 1, batch_max=Q, global_exps=np.array([3, 3, 5, 6], np.int8))
        .reshape(-1, fb)[5])
    assert poll([result_frame(P, 5, pay[0]), result_frame(P, 4, pay[0])])[0].tolist() == [FINISHED, FINISHED]
    assert wk.resend([0, 1]).tolist() == [-1, -1] and poll([result_frame(P, 4, pay[0])])[0].tolist() == [WRONG]
    assert wk.counts.tolist() == [6, 4, 2, 2]
    assert sw.FrameWorker(sw.frame_params(max_outstanding_pkts=Q), 1, P).poll(ring(frames), 8, tx)[0].tolist() == \
        [IGNORED] * 8                                                     # no slice under way


class GpuLoop:
    """lossy_loop's backend on the GPU: the gather list and the drop masks come from the host."""

    def __init__(self, loop, xd, outs):
        self.loop, self.begin = loop, lambda: loop.begin(xd, outs) and self.outstanding()

    def outstanding(self):
        every = list(range(self.loop.Q))
        return [(w, s) for w, wk in enumerate(self.loop.workers) for s in wk.resend(every).tolist() if s >= 0]

    def round(self, batch, drop):
        import torch
        if not batch:
            return [0] * self.loop.W, self.outstanding()
        cols = [torch.tensor(c, dtype=t).cuda() for c, t in zip((*zip(*batch), drop), (torch.int32, torch.int64, torch.int32))]
        return [int(((v == POSTED) | (v == FINISHED)).sum()) for v, _ in self.loop.step(*cols)], self.outstanding()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_closed_loop_under_loss_and_duplication(sw, seed, dtype):
    import torch
    c = LOSSY
    loop = Loop(sw, dtype, c["W"], c["P"], c["Q"], ring=c["ring"], pad=12)
    xd, _, want = inputs(dtype, c["W"], c["P"], c["blocks"] * c["P"], seed)
    outs = [torch.zeros_like(x) for x in xd]
    lossy_loop(np.random.default_rng(seed), c["W"], c["blocks"] + (dtype != "int32") * c["Q"], GpuLoop(loop, xd, outs))
    for out in outs:
        assert torch.equal(out.cpu().view(torch.uint8), want.view(torch.uint8))
    assert sum(int(wk.counts[WRONG]) for wk in loop.workers) > 0 and int(loop.switch.counts[RETRANSMIT]) > 0
    assert int(loop.switch.deliver_counts[2]) == 0                         # no ring overflowed


@pytest.mark.parametrize("n,pad,offset,pinned", [(255, 12, 4, False), (256, 64, 0, True), (257, 0, 0, False)])
def test_layout_and_frame_counts_around_the_judge_workgroup(sw, n, pad, offset, pinned):
    """INT32, B = 2 Q: n - 1 slots accept their first frame and post their second, one frame is a second copy.
    Strides past the frame, bases at 4 mod 16, pinned host rings."""
    import torch
    P, Q = 64, 257
    fb = M.frame_bytes(P)
    stride = fb + pad
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, 2 * Q * P, dtype=np.int64).astype(np.int32)).cuda()
    out = torch.full_like(x, 0x5A5A5A5A)
    place = (lambda t: t.pin_memory()) if pinned else (lambda t: t.cuda())
    tx = place(torch.full((offset + Q * stride,), SENTINEL, dtype=torch.uint8))[offset:]
    pay = rng.integers(0, 256, (n, 4 * P), dtype=np.uint8)
    host = np.full((n, stride), SENTINEL, dtype=np.uint8)
    for i in range(n):
        host[i, :fb] = result_frame(P, i if i < n - 1 else 0, pay[i])
    rx = place(torch.cat([torch.zeros(offset, dtype=torch.uint8), torch.from_numpy(host.reshape(-1))]))[offset:]
    assert tx.data_ptr() % 16 == offset and rx.data_ptr() % 16 == offset
    wk = sw.FrameWorker(sw.frame_params(job_id=JOB, max_outstanding_pkts=Q), 1, P, dtype=torch.int32)
    wk.begin(x, out, tx, stride)
    verdict, sends = wk.poll(rx, n, tx, rx_stride=stride, tx_stride=stride)
    assert verdict.tolist() == [POSTED] * (n - 1) + [WRONG] and sends.tolist() == list(range(n - 1)) + [-1]
    want = np.full(2 * Q * P, 0x5A5A5A5A, dtype=np.int32)
    want[:(n - 1) * P] = pay[:n - 1].reshape(-1).view(">i4")
    assert np.array_equal(out.cpu().numpy(), want)
    bulk = O.build_frames_i32(x.cpu().numpy(), wk.params.frame, P).reshape(-1, fb)
    image = np.full((Q, stride), SENTINEL, dtype=np.uint8)
    image[:, :fb] = np.concatenate([bulk[Q:Q + n - 1], bulk[n - 1:Q]])
    assert np.array_equal(tx.cpu().numpy().reshape(Q, stride), image)
