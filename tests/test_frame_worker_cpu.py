"""CPU tests of the DPDK worker's calls: the ABI table and the params structure held to
include/switchml_frame_worker.h, the state's size, every argument status of the four calls (each returns before
any HIP call), and the seeds of the GPU's lossy closed loop on tests/switch_deliver_model.py alone."""
import ctypes

import numpy as np
import pytest

import switch_deliver_model as D
import switch_frames_model as M
import test_abi_cpu as A
from switchml_amd import abi
from switchml_amd import frame_wire as FW

INV, UNS, ALN, OK = abi.SML_ERR_INVALID_ARG, abi.SML_ERR_UNSUPPORTED, abi.SML_ERR_ALIGNMENT, abi.SML_OK
vp = ctypes.c_void_p

LOSSY = dict(W=3, P=64, Q=4, blocks=40, q=0.15, ring=16)
LOSSY_SEEDS = (1, 2, 3)


def lossy_loop(rng, W, total, backend, q=LOSSY["q"]):
    """The lossy closed loop's host side, for the model below and for the GPU: every round each slot with a frame
    outstanding is sent (again); an entry is left out of the switch's input with probability q, else entered twice
    with probability q; every bit of an entry's drop mask is set with probability q.  backend.begin() -> the
    (worker, slot) pairs to send; backend.round(batch, drop) -> (frames accepted per worker, the pairs outstanding)."""
    sends, done = backend.begin(), [0] * W
    for rnd in range(60 * total):
        if all(d == total for d in done):
            return rnd
        batch = [e for e in sends if rng.random() >= q]
        batch += [e for e in batch if rng.random() < q]
        batch = [batch[i] for i in rng.permutation(len(batch))]
        drop = [sum(1 << u for u in range(W) if rng.random() < q) for _ in batch]
        accepted, sends = backend.round(batch, drop)
        done = [d + a for d, a in zip(done, accepted)]
    raise AssertionError("the lossy loop did not finish")


class ModelLoop:
    """lossy_loop's backend on the model switch; the workers: a slot accepts the id it expects, once a round."""

    def __init__(self, W, P, Q, total):
        workers = M.default_workers(W)
        frames = [[FW.worker_frame(P, workers[w], p, FW.pool_index(p, Q), bytes(4 * P), src_port=4000 + w)
                   for p in range(total)] for w in range(W)]
        self.switch = D.ModelSwitch(frames, workers, Q, P, 1 << 30)
        self.W, self.b, self.total = W, min(Q, total), total
        self.expected = [list(range(self.b)) for _ in range(W)]
        self.retransmits = self.duplicates = 0

    def outstanding(self):
        return [(w, j) for w in range(self.W) for j in range(self.b) if self.expected[w][j] < self.total]

    begin = outstanding

    def round(self, batch, drop):
        verdicts, _, new = self.switch.call([(w, self.expected[w][j]) for w, j in batch], drop)
        self.retransmits += int((verdicts == M.RETRANSMIT).sum())
        accepted = []
        for w in range(self.W):
            slots = {p % self.b for p in new[w] if self.expected[w][p % self.b] == p}
            self.duplicates += len(new[w]) - len(slots)
            for j in slots:
                self.expected[w][j] += self.b
            accepted.append(len(slots))
        return accepted, self.outstanding()


@pytest.mark.parametrize("extra", [0, LOSSY["Q"]], ids=["int32", "float"])
@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_lossy_seeds_retransmit_and_duplicate_on_the_model(seed, extra):
    c = LOSSY
    loop = ModelLoop(c["W"], c["P"], c["Q"], c["blocks"] + extra)
    lossy_loop(np.random.default_rng(seed), c["W"], c["blocks"] + extra, loop)
    assert loop.retransmits > 0 and loop.duplicates > 0
    assert max(loop.switch.fill) > 0 and c["ring"] >= 4 * c["Q"]     # a round: <= Q broadcasts, <= 2 Q answers


def test_abi_table_and_params_layout_equal_the_header():
    protos = A.typed_prototypes(abi.FRAME_WORKER_HEADER_PATH)
    assert sorted(protos) == sorted(abi.FRAME_WORKER_SIGNATURES) == abi.header_symbols(abi.FRAME_WORKER_HEADER_PATH)
    L, T = abi.lib(), abi.FrameWorkerParams
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.FRAME_WORKER_SIGNATURES[name]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        for (base, depth), a in zip(params, argtypes):
            assert a in ({ctypes.POINTER(T), vp} if base == "sml_frame_worker_params" else A.allowed(base, depth)), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    assert ctypes.sizeof(T) == 64 and [getattr(T, n).offset for n, _ in T._fields_] == [0, 48, 50, 52, 56]
    assert T.frame.size == ctypes.sizeof(abi.FrameParams) == 48
    body = A.stripped(abi.FRAME_WORKER_HEADER_PATH).split("typedef struct sml_frame_worker_params")[1].split("}")[0]
    assert [d.split()[-1] for d in body.strip("{ \n").split(";") if d.strip()] == [n for n, _ in T._fields_]
    assert A.defines(abi.FRAME_WORKER_HEADER_PATH) == {
        "SML_FRAME_WORKER_WRONG": abi.FRAME_WORKER_WRONG, "SML_FRAME_WORKER_POSTED": abi.FRAME_WORKER_POSTED,
        "SML_FRAME_WORKER_FINISHED": abi.FRAME_WORKER_FINISHED, "SML_FRAME_WORKER_IGNORED": abi.FRAME_WORKER_IGNORED,
        "SML_FRAME_WORKER_NONE": abi.FRAME_WORKER_NONE}
    assert '#include "switchml_frame_worker.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


@pytest.mark.parametrize("Q,ok", [(1, True), (7, True), (16384, True), (0, False), (16385, False)])
def test_state_bytes(Q, ok):
    got = abi.lib().sml_frame_worker_state_bytes(Q)
    assert (got == 64 + 16 * Q) if ok else got == 0               # a slice header, a 16-byte record per slot: O(Q)


GOOD = dict(W=2, dt=abi.FLOAT32, P=64, Q=4, start=0, x=4096, out=8192, numel=300, st=16384, rx=1 << 20, tx=1 << 21,
            rxs=308, txs=308, sends=131072, live=262144, vd=524288, cnt=1048576, slots=1 << 22, n=3)
BAD_PARAMS = [("P", 100), ("P", 2048), ("Q", 0), ("Q", 16385), ("start", 16381), ("dt", 4)]
CASES = [
    *[(fn, "null params", dict(prm=None), INV) for fn in ("begin", "poll", "resend")],
    *[(fn, "no workers", dict(W=0), INV) for fn in ("begin", "poll", "resend")],
    *[("begin", f"null {k}", {k: None}, INV) for k in ("x", "out", "tx", "st", "sends")],
    *[("poll", f"null {k}", {k: None}, INV) for k in ("rx", "st", "tx", "sends", "vd")],
    *[("resend", f"null {k}", {k: None}, INV) for k in ("slots", "st", "sends")],
    *[(fn, f"bad {k}={v}", {k: v}, UNS) for fn in ("begin", "poll", "resend") for k, v in BAD_PARAMS],
    *[(fn, "too many frames", dict(n=2 ** 31), UNS) for fn in ("poll", "resend")],
    ("begin", "more frames than pkt_ids", dict(numel=2 ** 38), UNS),
    ("poll", "null wins over unsupported", dict(P=100, rx=None), INV),
    ("poll", "unsupported wins over alignment", dict(P=100, rx=(1 << 20) + 2), UNS),
    ("begin", "an empty slice still needs its state", dict(numel=0, x=None, out=None, tx=None, st=None), INV),
    ("poll", "nothing to do", dict(n=0, rx=None, st=None, tx=None, sends=None, vd=None, cnt=None, live=None), OK),
    ("resend", "nothing to do", dict(n=0, slots=None, st=None, sends=None), OK),
    ("poll", "nothing to do, bad parameters", dict(n=0, Q=0), UNS),
    ("poll", "rx inside tx", dict(rx=(1 << 21) + 616), INV),
    ("poll", "tx inside rx", dict(tx=(1 << 20) + 312), INV),
    *[("begin", f"misaligned {k}", {k: v}, ALN) for k, v in [("x", 4098), ("out", 8194), ("st", 16392),
                                                             ("tx", (1 << 21) + 2), ("txs", 310), ("txs", 304),
                                                             ("sends", 131076)]],
    ("begin", "a 16-bit slice at an odd byte", dict(dt=abi.BFLOAT16, x=4097), ALN),
    *[("poll", f"misaligned {k}", {k: v}, ALN) for k, v in [("st", 16392), ("rx", (1 << 20) + 2), ("rxs", 310),
                                                            ("rxs", 304), ("tx", (1 << 21) + 2), ("txs", 306),
                                                            ("live", 262148), ("sends", 131076), ("cnt", 1048580)]],
    *[("resend", f"misaligned {k}", {k: v}, ALN) for k, v in [("st", 16392), ("slots", (1 << 22) + 2),
                                                              ("sends", 131076)]],
]


@pytest.mark.parametrize("fn,name,change,status", CASES, ids=[f"{c[0]}: {c[1]}" for c in CASES])
def test_argument_status(fn, name, change, status):
    a = dict(GOOD, **change)
    prm = abi.FrameWorkerParams(abi.FrameParams(pool_index_start=a["start"], max_outstanding_pkts=a["Q"]), a["W"],
                                a["dt"], a["P"], 0)
    ptr = lambda k: None if a[k] is None else vp(a[k])                        # noqa: E731
    L, p = abi.lib(), None if "prm" in a else ctypes.byref(prm)
    if fn == "begin":
        got = L.sml_frame_worker_begin(p, ptr("x"), ptr("out"), a["numel"], ptr("st"), ptr("tx"), a["txs"],
                                       ptr("sends"), None)
    elif fn == "poll":
        got = L.sml_frame_worker_poll(p, ptr("rx"), a["n"], a["rxs"], ptr("live"), ptr("st"), ptr("tx"), a["txs"],
                                      ptr("sends"), ptr("vd"), ptr("cnt"), None)
    else:
        got = L.sml_frame_worker_resend(p, ptr("slots"), a["n"], ptr("st"), ptr("sends"), None)
    assert got == status                                                      # every case returns before a launch


@pytest.mark.parametrize("st,Q,status", [(None, 4, INV), (4096, 0, UNS), (4096, 16385, UNS), (None, 0, INV),
                                         (4104, 4, ALN), (4104, 0, UNS)])
def test_reset_argument_status(st, Q, status):
    assert abi.lib().sml_frame_worker_reset(None if st is None else vp(st), Q, None) == status
