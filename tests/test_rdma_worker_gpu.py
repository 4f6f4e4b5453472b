"""GPU tests of the RDMA worker's completion loop (sml_rdma_worker_* /
switchml_amd.RdmaWorker, DESIGN §9 F4 "Worker side").  W workers and one
RdmaSwitch run whole all-reduces as a chain of launches; the only host work is
the NIC's — turning a switch call's results into each worker's completions —
and the outputs are held bit for bit to the plane oracle (exponents ->
switch_exps -> quantize under the global exponents -> switch_payload ->
dequantize; INT32: the wrapping sum)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_rdma_worker_cpu import LOSSY, LOSSY_SEEDS, lossy_masks

pytestmark = pytest.mark.gpu

PPM, FIRST_SLOT, SENTINEL = 4, 3, 0x5A5A5A5A
WRONG, POSTED, FINISHED, IGNORED = range(4)
BROADCAST, RETRANSMIT = 1, 2


@pytest.fixture(scope="module")
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def inputs(dtype, W, M, n, seed):
    """(the workers' device tensors, the oracle's all-reduce of them as a tensor
    of the dtype, worker 0's payload plane as its messages carry it)."""
    import torch
    if dtype == "int32":
        rng = np.random.default_rng(seed)
        xs = [rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) for _ in range(W)]
        return [torch.from_numpy(x).cuda() for x in xs], torch.from_numpy(sum(xs[1:], xs[0])), O.bswap32(xs[0])
    tdt = getattr(torch, dtype)
    xd = [torch.from_numpy(O.splitmix_normal(seed + w, n) * np.float32(4.0 ** w)).cuda().to(tdt) for w in range(W)]
    xs = [x.float().cpu().numpy() for x in xd]                       # what the kernels widen to
    exps = O.switch_exps([O.exponents(x, M) for x in xs])
    planes = [O.quantize(x, M, W, global_exps=exps) for x in xs]
    want = O.dequantize(O.switch_payload(planes), exps, n, M, W)
    return xd, torch.from_numpy(want).to(tdt), planes[0]


class Loop:
    """W workers around one switch; `tx` is [W, Q, M] words, the switch's landing region."""

    def __init__(self, sw, dtype, W, M, Q, place="device"):
        import torch
        self.sw, self.W, self.M, self.Q, self.tdt = sw, W, M, Q, getattr(torch, dtype)
        make = (lambda: torch.full((W, Q * M), SENTINEL, dtype=torch.int32).pin_memory()) if place == "pinned" else \
            (lambda: torch.full((W, Q * M), SENTINEL, dtype=torch.int32, device="cuda"))
        self.tx = make()
        self.rx = self.tx if place == "same" else make()
        self.switch = sw.RdmaSwitch(W, FIRST_SLOT + Q, M, PPM)
        self.workers = [sw.RdmaWorker(u, W, Q, M, PPM, first_slot=FIRST_SLOT, src_base=u * Q, dtype=self.tdt)
                        for u in range(W)]
        self.late = [[] for _ in range(W)]

    def run(self, xs, rng=None):
        """One slice on every worker to completion; returns (outputs, worker 0's first payload-carrying message)."""
        import torch
        W, M, Q = self.W, self.M, self.Q
        outs = [torch.zeros_like(x) for x in xs]
        sends = [wk.begin(x, out, self.tx[u]) for u, (wk, x, out) in enumerate(zip(self.workers, xs, outs))]
        B = O.num_blocks(xs[0].numel(), M)
        b, total = min(B, Q), B if self.tdt == torch.int32 else B + min(B, Q)
        waiting = [set(range(b)) for _ in range(W)]               # QPs with a message outstanding
        done0 = [int(wk.counts[POSTED] + wk.counts[FINISHED]) for wk in self.workers]
        first = self.tx[0, :M].cpu().numpy().copy() if self.tdt == torch.int32 else None
        for rnd in range(400):
            if not any(waiting):
                break
            arrivals = torch.cat(sends)
            recs = arrivals.cpu().numpy().view(np.dtype(self.sw.rdma_switch.ARRIVAL_FIELDS)).reshape(-1)
            drop, twice, late = lossy_masks(rng, len(recs), W) if rng else (np.zeros((len(recs), W), bool),) * 3
            bits = torch.from_numpy((drop * (1 << np.arange(W))).sum(axis=1).astype(np.int32)).cuda()
            verdict, out_imm = self.switch.step(arrivals, self.tx.view(W * Q, M), self.rx, bits)
            verdict, out_imm = verdict.cpu().numpy(), out_imm.cpu().numpy().view(np.uint32)
            comps, self.late = self.late, [[] for _ in range(W)]  # the NIC: results -> completions
            for i in np.flatnonzero((verdict == BROADCAST) | (verdict == RETRANSMIT)):
                for u in (range(W) if verdict[i] == BROADCAST else [int(recs["worker"][i])]):
                    if not drop[i, u]:
                        c = ((int(recs["rkey"][i]) >> 1) // PPM - FIRST_SLOT, int(out_imm[i]))
                        comps[u] += [c] * (2 if twice[i, u] else 1)
                        self.late[u] += [c] * bool(late[i, u])
            sends = []
            for u, wk in enumerate(self.workers):
                c = np.array(comps[u], dtype=np.dtype(self.sw.rdma_worker.COMPLETION_FIELDS))
                v, s = wk.poll(c, self.rx[u], self.tx[u])
                v = v.cpu().numpy()
                accepted = {int(q) for q in c["qpn"][(v == POSTED) | (v == FINISHED)]}
                waiting[u] -= {int(q) for q in c["qpn"][v == FINISHED]}
                sends += [s, wk.resend(sorted(waiting[u] - accepted))]     # every timer fires every round
            if rnd == 0 and first is None:
                first = self.tx[0, :M].cpu().numpy().copy()
        assert not any(waiting)
        for wk, d in zip(self.workers, done0):
            assert int(wk.counts[POSTED] + wk.counts[FINISHED]) - d == total
        return outs, first.view(np.uint32)


def check_slices(loop, dtype, W, M, n, rng=None):
    """Two slices back to back on the same state and switch, no reset between: the pool flag must persist."""
    import torch
    for seed in (40, 50):
        xs, want, first = inputs(dtype, W, M, n, seed)
        outs, got_first = loop.run(xs, rng)
        for out in outs:
            assert torch.equal(out.cpu().view(torch.uint8), want.view(torch.uint8))
        assert rng is not None or np.array_equal(got_first, first[:M].view(np.uint32))


SHAPES = [(64, 2, 2 * 64 + 5), (1024, 2, 3 * 1024), (1024, 8, 2 * 1024 + 5), (256, 1, 256)]


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("M,Q,n", SHAPES)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "int32"])
def test_closed_loop_through_the_switch(sw, dtype, M, Q, n, W):
    check_slices(Loop(sw, dtype, W, M, Q), dtype, W, M, n)


@pytest.mark.parametrize("place", ["same", "pinned"])
def test_one_registered_buffer_and_pinned_host_buffers(sw, place):
    check_slices(Loop(sw, "float32", 2, 1024, 2, place), "float32", 2, 1024, 3 * 1024)


@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_closed_loop_under_loss_and_duplication(sw, seed):
    c = LOSSY
    loop = Loop(sw, "float32", c["W"], c["M"], c["Q"])
    check_slices(loop, "float32", c["W"], c["M"], c["blocks"] * c["M"], np.random.default_rng(seed))
    assert sum(int(wk.counts[WRONG]) for wk in loop.workers) > 0 and int(loop.switch.counts[RETRANSMIT]) > 0


def single(sw, M=64, Q=2, blocks=4):
    """One worker (W = 1) past its first batch by hand: messages 0 and 1 accepted with exponent 3."""
    import torch
    x = torch.from_numpy(O.splitmix_normal(9, blocks * M)).cuda()
    out = torch.full_like(x, float("nan"))
    buf = torch.from_numpy(np.random.default_rng(9).integers(-2 ** 31, 2 ** 31, (2, Q * M)).astype(np.int32)).cuda()
    wk = sw.RdmaWorker(0, 1, Q, M, PPM, first_slot=FIRST_SLOT)
    comp = lambda rows: np.array(rows, dtype=np.dtype(sw.rdma_worker.COMPLETION_FIELDS))    # noqa: E731
    begun = wk.begin(x, out, buf[0])
    verdict, posted = wk.poll(comp([(0, 0 | 3 << 16), (1, 1 | 3 << 16)]), buf[1], buf[0])
    assert verdict.tolist() == [POSTED, POSTED]
    return wk, x, out, buf, comp, (begun, posted)


def null_records(sends, which):
    got = sends.cpu().numpy()[which]
    return np.array_equal(got, np.broadcast_to(np.array([0xFFFFFFFF, 0, 0], dtype=np.int64), got.shape))


def test_verdict_rules_in_one_call(sw):
    M, e1 = 64, 5
    wk, x, out, buf, comp, _ = single(sw)
    before = buf.cpu().numpy().copy()
    verdict, sends = wk.poll(comp([(0, 2 | e1 << 16), (0, 2 | e1 << 16), (1, 5), (2, 2), (2 ** 31, 2)]), buf[1], buf[0])
    assert verdict.tolist() == [POSTED, WRONG, WRONG, IGNORED, IGNORED] and null_records(sends, slice(1, None))
    xs, after = x.cpu().numpy(), buf.cpu().numpy()
    # message 2 of QP 0: block 0 out of rx under the kept exponent 3, block 2 into tx under the received 5
    want = O.dequantize(before[1, :M].view(np.uint32), np.array([3], np.int8), M, M, 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[:M].view(np.uint32), want.view(np.uint32)) and np.isnan(got[M:]).all()
    assert np.array_equal(after[0, :M].view(np.uint32), O.quantize(xs[2 * M:3 * M], M, 1, np.array([e1], np.int8)))
    assert np.array_equal(after[0, M:], before[0, M:]) and np.array_equal(after[1], before[1])
    rec = sends.cpu().numpy().view(np.dtype(sw.rdma_switch.ARRIVAL_FIELDS)).reshape(-1)[0]
    assert (rec["worker"], rec["rkey"], rec["imm"], rec["src"], rec["addr"]) == (0, (FIRST_SLOT * PPM) << 1, 4, 0, 0)
    assert wk.poll(comp([(0, 2 | e1 << 16)]), buf[1], buf[0])[0].tolist() == [WRONG]       # the old id, a call later
    assert wk.poll(comp([(0, 4)]), buf[1], buf[0])[0].tolist() == [FINISHED]
    assert wk.poll(comp([(0, 4), (0, 6)]), buf[1], buf[0])[0].tolist() == [IGNORED, IGNORED]
    assert wk.counts.tolist() == [3, 3, 1, 4]


def test_resend_repeats_the_outstanding_record_and_changes_nothing(sw):
    import torch
    wk, x, out, buf, comp, (begun, posted) = single(sw, Q=3, blocks=2)  # b = 2 < Q: QP 2 idle
    assert null_records(begun, 2) and not null_records(begun, 0)
    assert np.array_equal(sw.RdmaWorker(0, 1, 3, 64, PPM, first_slot=FIRST_SLOT).resend([0]).cpu().numpy()[0],
                          [0xFFFFFFFF, 0, 0])                            # no slice begun
    held = (wk.state, buf, out.view(torch.int32))
    snap = [t.cpu().numpy().copy() for t in held]
    again = wk.resend([1, 0, 2, 7])
    assert np.array_equal(again[:2].cpu().numpy(), posted.cpu().numpy()[::-1]) and null_records(again, slice(2, None))
    rec = again.cpu().numpy().view(np.dtype(sw.rdma_switch.ARRIVAL_FIELDS)).reshape(-1)[1]
    assert (rec["rkey"], rec["imm"] & 0xFFFF, rec["addr"]) == ((FIRST_SLOT * PPM) << 1 | 1, 2, 0)
    assert all(np.array_equal(t.cpu().numpy(), s) for t, s in zip(held, snap))
    assert wk.poll(comp([(1, 3)]), buf[1], buf[0])[0].tolist() == [FINISHED] and null_records(wk.resend([1]), 0)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_record_counts_around_the_judge_workgroup(sw, n):
    """INT32, b = B = Q: every QP's only message; n of them accepted in one call, plus one duplicate."""
    import torch
    M, Q = 64, 257
    x = torch.arange(Q * M, dtype=torch.int32, device="cuda")
    out = torch.full_like(x, SENTINEL)
    tx = torch.zeros(Q * M, dtype=torch.int32, device="cuda")
    rx = torch.from_numpy(np.random.default_rng(n).integers(-2 ** 31, 2 ** 31, Q * M).astype(np.int32)).cuda()
    wk = sw.RdmaWorker(0, 1, Q, M, PPM, dtype=torch.int32)
    wk.begin(x, out, tx)
    comps = np.array([(q, q) for q in range(n - 1)] + [(0, 0)], dtype=np.dtype(sw.rdma_worker.COMPLETION_FIELDS))
    verdict, sends = wk.poll(comps, rx, tx)
    assert verdict.tolist() == [FINISHED] * (n - 1) + [WRONG] and null_records(sends, slice(None))
    want = np.full(Q * M, SENTINEL, dtype=np.int32)
    want[:(n - 1) * M] = O.bswap32(rx.cpu().numpy())[:(n - 1) * M].view(np.int32)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(tx.cpu().numpy(), O.bswap32(x.cpu().numpy()).view(np.int32))
