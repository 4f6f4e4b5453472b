"""The RDMA switch in plain Python / numpy: the model sml_rdma_switch (DESIGN
§9 F4 "Switch side") is held to, bit for bit.

RdmaSwitchModel is strictly sequential, one completion record at a time, the
frame switch's SwitchModel at message granularity with p4/rdma_sender.p4's
results: the summed words written into the workers' receive regions and the
immediate.  model_call() puts the one rule of a GPU call on top of it with
switch_frames_model.deferred_indices, unchanged: per (slot, worker) the call
handles the set of the pair's lowest-index record, the pair's records of the
other set are DEFERRED.
"""
import numpy as np

from switch_frames_model import BROADCAST, CONSUMED, DEFERRED, IGNORED, RETRANSMIT, deferred_indices

ARRIVAL = np.dtype([("worker", "<u4"), ("rkey", "<u4"), ("imm", "<u4"), ("src", "<u4"), ("addr", "<u8")])
DROPPED = 5                                                   # counts[5]: copies a drop bit kept back


def rkey(slot, set_, ppm):
    return ((slot * ppm) << 1) | set_


def imm(msg_id, e0=0, e1=0):
    return (int(msg_id) & 0xFFFF) | ((int(e0) & 0xFF) << 16) | ((int(e1) & 0xFF) << 24)


def arrivals(rows):
    """Records from (worker, rkey, imm, src, addr) tuples."""
    return np.array([tuple(r) for r in rows], dtype=ARRIVAL)


class RdmaSwitchModel:
    def __init__(self, W, S, M, ppm):
        self.W, self.S, self.M, self.ppm = W, S, M, ppm
        self.landing_msgs = self.rx_bytes = 0                 # of the call under way
        self.reset()

    def reset(self):
        self.bitmap = [[0, 0] for _ in range(self.S)]
        self.count = [[0, 0] for _ in range(self.S)]
        self.acc = np.zeros((self.S, 2, self.M), dtype=np.uint32)       # host order
        self.exps = np.zeros((self.S, 2, 2), dtype=np.int8)

    def parse(self, a):
        """(w, s, v) or None for a record the switch ignores."""
        w, idx, v, addr = int(a["worker"]), int(a["rkey"]) >> 1, int(a["rkey"]) & 1, int(a["addr"])
        s = idx // self.ppm
        if (idx % self.ppm or s >= self.S or w >= self.W or int(a["src"]) >= self.landing_msgs or addr % 16
                or addr + 4 * self.M > self.rx_bytes):
            return None
        return w, s, v

    def record(self, a, landing, rx, drop):
        """One record: (verdict, out_imm or None, copies dropped); a result is written into rx."""
        key = self.parse(a)
        if key is None:
            return IGNORED, None, 0
        w, s, v = key
        W, bit = self.W, 1 << w
        before = self.bitmap[s][v]
        self.bitmap[s][v] |= bit
        self.bitmap[s][1 - v] &= ~bit
        if not before & bit:
            flag = self.count[s][v]
            self.count[s][v] = W - 1 if flag == 0 else flag - 1
            if W == 1:
                flag = 1
            words = landing[int(a["src"]), :4 * self.M].view(">u4").astype(np.uint32)
            e = np.array([int(a["imm"]) >> 16 & 0xFF, int(a["imm"]) >> 24], dtype=np.uint8).view(np.int8)
            if before == 0:
                self.acc[s, v] = words
                self.exps[s, v] = e
            else:
                self.acc[s, v] += words                                       # mod 2^32
                self.exps[s, v] = np.maximum(self.exps[s, v], e)
            verdict = BROADCAST if flag == 1 else CONSUMED
        else:
            flag = 0 if W == 1 else self.count[s][v]
            verdict = RETRANSMIT if flag == 0 else CONSUMED
        if verdict == CONSUMED:
            return verdict, None, 0
        to = range(W) if verdict == BROADCAST else [w]
        wire = self.acc[s, v].astype(">u4").view(np.uint8)
        addr, dropped = int(a["addr"]), 0
        for u in to:
            if drop >> u & 1:
                dropped += 1
            else:
                rx[u, addr:addr + 4 * self.M] = wire
        e0, e1 = self.exps[s, v].view(np.uint8)
        return verdict, imm(int(a["imm"]), int(e0), int(e1)), dropped


def model_call(model, records, landing, rx, drop=None):
    """One call: (verdicts, {index: out_imm}, counts[6]).  `landing`: uint8
    [landing_msgs, stride]; `rx`: uint8 [W, rx_bytes], written in place."""
    model.landing_msgs, model.rx_bytes = landing.shape[0], rx.shape[1]
    skip = deferred_indices(model, records)
    verdicts, out_imm, counts = [], {}, [0] * 6
    for i, a in enumerate(records):
        if i in skip:
            verdict, word, dropped = DEFERRED, None, 0
        else:
            verdict, word, dropped = model.record(a, landing, rx, 0 if drop is None else int(drop[i]))
        verdicts.append(verdict)
        counts[verdict] += 1
        counts[DROPPED] += dropped
        if word is not None:
            out_imm[i] = word
    return np.array(verdicts, dtype=np.uint8), out_imm, counts


class ClosedLoop:
    """The backend of switch_deliver_model.lossy_loop over RDMA records, INT32:
    worker w's message p lands at landing[w * N + p], goes to slot p % mop of
    set (p // mop) & 1 and names address p * 4 M.  `step(records, drop)` is the
    switch: (verdicts, out_imm by index).  The workers see only those two."""

    def __init__(self, step, xs, mop, M, ppm):
        self.step, self.W, self.N, self.mop, self.M, self.ppm = step, len(xs), xs[0].size // M, mop, M, ppm
        self.landing = np.concatenate([x.astype(">i4").view(np.uint8).reshape(self.N, 4 * M) for x in xs])
        self.fill = [0] * self.W
        self.verdicts = [0] * 5                               # how often each verdict came up

    def call(self, batch, drop):
        N, mop, M = self.N, self.mop, self.M
        recs = arrivals([(w, rkey(p % mop, p // mop & 1, self.ppm), imm(p), w * N + p, p * 4 * M) for w, p in batch])
        verdicts, out_imm = self.step(recs, np.array(drop, dtype=np.uint32))
        new = [[] for _ in range(self.W)]
        for i, (w, _) in enumerate(batch):
            self.verdicts[verdicts[i]] += 1
            if verdicts[i] in (BROADCAST, RETRANSMIT):
                for u in range(self.W) if verdicts[i] == BROADCAST else [w]:
                    if not drop[i] >> u & 1:
                        new[u].append(int(out_imm[i]) & 0xFFFF)
        self.fill = [f + len(ids) for f, ids in zip(self.fill, new)]
        return verdicts, list(self.fill), new
