"""GPU tests of the RDMA worker's completion loop for long messages
(sml_msg_worker_* behind switchml_amd.RdmaWorker, DESIGN §9 F4 "Worker side",
"Long messages"), with the harness of tests/test_rdma_worker_gpu.py: W workers
closed through RdmaSwitch (sml_msg_switch at these lengths), bit for bit
against the plane oracle, at the smallest shapes at which a message dealt over
the waves of a workgroup can go wrong."""
import numpy as np
import pytest

from oracle import oracle as O
from test_rdma_worker_cpu import LOSSY, LOSSY_SEEDS
from test_rdma_worker_gpu import (FIRST_SLOT, IGNORED, POSTED, RETRANSMIT, WRONG, Loop, check_slices, null_records,
                                  sw)  # noqa: F401  (sw: the module's fixture)

pytestmark = pytest.mark.gpu

# M, Q, n: one wave, not a packet size, partial last block | 2 waves, 3 + 2 slices | 3 waves (no power of two), the
# last block ends inside wave 1's first slice, wave 2 idle but at the barrier, an idle QP | 5 waves, last slice 64
# words, Q = 1 | 16 waves full
SHAPES = [(192, 2, 2 * 192 + 5), (1280, 2, 3 * 1280), (2304, 3, 2 * 2304 + 1030), (4160, 1, 2 * 4160 + 5),
          (16384, 2, 2 * 16384)]


def records(sw, sends):
    return sends.cpu().numpy().view(np.dtype(sw.rdma_switch.ARRIVAL_FIELDS)).reshape(-1)


def completions(sw, rows):
    return np.array(rows, dtype=np.dtype(sw.rdma_worker.COMPLETION_FIELDS))


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("M,Q,n", SHAPES)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "int32"])
def test_closed_loop_through_the_switch(sw, dtype, M, Q, n, W):
    loop = Loop(sw, dtype, W, M, Q)
    assert {wk.entry for wk in loop.workers} == {"sml_msg_worker"} and loop.switch.entry == "sml_msg_switch"
    check_slices(loop, dtype, W, M, n)


@pytest.mark.parametrize("pos", [0, 255, 256, 1023, 1024, 2303])
def test_the_maximum_crosses_waves(sw, pos):
    """One spike per block, in another wave's slice or at a slice's edge each time: the exponent a record carries
    is the whole message's."""
    import torch
    M, Q, b = 2304, 2, 2
    x = O.splitmix_normal(11, 4 * M) * np.float32(2.0 ** -20)
    x[0 * M + pos] = x[(0 + b) * M + pos] = 2.0 ** 10
    exps = O.exponents(x, M)
    assert exps[0] == exps[2] == 11 and exps[1] < 0 and exps[3] < 0
    xd = torch.from_numpy(x).cuda()
    buf = torch.zeros(Q * M, dtype=torch.int32, device="cuda")
    wk = sw.RdmaWorker(0, 1, Q, M, 9)
    begun = records(sw, wk.begin(xd, torch.empty_like(xd), buf))
    assert [int(i) >> 16 for i in begun["imm"]] == [int(exps[0]) & 0xFF, int(exps[1]) & 0xFF]
    verdict, sends = wk.poll(completions(sw, [(0, 0 | 3 << 16), (1, 1 | 3 << 16)]), buf, buf)
    assert verdict.tolist() == [POSTED, POSTED]
    assert [int(i) >> 16 for i in records(sw, sends)["imm"]] == [int(exps[2]) & 0xFF, int(exps[3]) & 0xFF]


def by_hand(sw, M, ppm, e1=5):
    """One worker (W = 1, Q = 2) on a slice of two blocks and 5 words, by hand over random-filled buffers: begin;
    messages 0 and 1 accepted with exponent 3; then one call with message 2 of QP 0 (POSTED: block 0 out of rx, the
    5 real words of block 2 into tx), its duplicate, a wrong id and a qpn past b."""
    import torch
    Q, n = 2, 2 * M + 5
    x = torch.from_numpy(O.splitmix_normal(9, n)).cuda()
    out = torch.full_like(x, float("nan"))
    buf = torch.from_numpy(np.random.default_rng(9).integers(-2 ** 31, 2 ** 31, (2, Q * M)).astype(np.int32)).cuda()
    wk = sw.RdmaWorker(0, 1, Q, M, ppm, first_slot=FIRST_SLOT)
    sends, verdicts = [wk.begin(x, out, buf[0])], []
    before = None
    for rows in ([(0, 0 | 3 << 16), (1, 1 | 3 << 16)], [(0, 2 | e1 << 16), (0, 2 | e1 << 16), (1, 5), (2, 2)]):
        before = buf.cpu().numpy().copy()
        v, s = wk.poll(completions(sw, rows), buf[1], buf[0])
        verdicts.append(v.tolist())
        sends.append(s)
    return dict(wk=wk, x=x.cpu().numpy(), out=out.cpu().numpy(), before=before, after=buf.cpu().numpy(),
                verdicts=verdicts, sends=sends, records=np.concatenate([records(sw, s) for s in sends]))


def test_verdict_rules_and_real_words_only_at_a_long_message(sw):
    M, ppm, e1 = 2304, 3, 5
    r = by_hand(sw, M, ppm, e1)
    assert r["wk"].entry == "sml_msg_worker"
    assert r["verdicts"] == [[POSTED, POSTED], [POSTED, WRONG, WRONG, IGNORED]] and null_records(r["sends"][2], slice(1, 4))
    before, after, out = r["before"], r["after"], r["out"]
    # message 2 of QP 0: block 0 out of rx under the kept exponent 3, block 2's 5 words into tx under the received 5
    want = O.dequantize(before[1, :M].view(np.uint32), np.array([3], np.int8), M, M, 1)
    assert np.array_equal(out[:M].view(np.uint32), want.view(np.uint32)) and np.isnan(out[M:]).all()
    assert np.array_equal(after[0, :5].view(np.uint32), O.quantize(r["x"][2 * M:], M, 1, np.array([e1], np.int8))[:5])
    assert np.array_equal(after[0, 5:], before[0, 5:]) and np.array_equal(after[1], before[1])
    # reset 1 -> message 0: 0 -> message 2: 1 -> message 4: 0; block 4 does not exist: exponent 0
    rec = records(sw, r["sends"][2])[0]
    assert (rec["worker"], rec["rkey"], rec["imm"], rec["src"], rec["addr"]) == (0, (FIRST_SLOT * ppm) << 1, 4, 0, 0)
    again = r["wk"].resend([0, 2])
    assert np.array_equal(again[0].cpu().numpy(), r["sends"][2][0].cpu().numpy()) and null_records(again, 1)
    assert r["wk"].counts.tolist() == [2, 3, 0, 1]


@pytest.mark.parametrize("place", ["same", "pinned"])
def test_one_registered_buffer_and_pinned_host_buffers(sw, place):
    check_slices(Loop(sw, "float32", 2, 2304, 2, place), "float32", 2, 2304, 3 * 2304)


@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_closed_loop_under_loss_and_duplication(sw, seed):
    c, M = LOSSY, 1280
    loop = Loop(sw, "float32", c["W"], M, c["Q"])
    check_slices(loop, "float32", c["W"], M, c["blocks"] * M, np.random.default_rng(seed))
    assert sum(int(wk.counts[WRONG]) for wk in loop.workers) > 0 and int(loop.switch.counts[RETRANSMIT]) > 0


def test_same_bits_as_the_packet_family(sw):
    old, new = by_hand(sw, 1024, 4), by_hand(sw, 1024, 3)
    assert (old["wk"].entry, new["wk"].entry) == ("sml_rdma_worker", "sml_msg_worker")
    assert old["verdicts"] == new["verdicts"] and old["wk"].counts.tolist() == new["wk"].counts.tolist()
    for k in ("after", "out"):
        assert np.array_equal(old[k].view(np.uint32), new[k].view(np.uint32)), k
    for f in ("worker", "imm", "src", "addr"):
        assert np.array_equal(old["records"][f], new["records"][f]), f
    ro, rn = old["records"]["rkey"], new["records"]["rkey"]                   # slot * pkts_per_msg << 1 | flag
    assert np.array_equal(ro & 1, rn & 1) and np.array_equal((ro >> 1) * 3, (rn >> 1) * 4)
