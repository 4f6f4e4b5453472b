"""The wire on both sides of the frame switch in plain Python / numpy: the
model sml_frame_switch_deliver and sml_frame_gather (DESIGN §9 F3 "Switch
side", Egress) are held to, on top of switch_frames_model's SwitchModel.

deliver() is strictly sequential, one input frame at a time in index order,
one copy at a time in worker order: the multicast group of
next_step_selector.p4 with udp_sender.p4's per-port destination, a drop mask
(drop_simulator.p4's place) and one FIFO ring per worker.  Nothing in it
counts ahead: a copy's ring position is simply where its ring stands when the
copy arrives.
"""
import numpy as np

import switch_frames_model as M
from switchml_amd import frame_wire as FW

DELIVERED, DROPPED, OVERFLOW, UNROUTABLE = range(4)

# The lossy closed loop both test files run: the CPU file checks that the model
# alone finishes for these seeds — each with RETRANSMIT and DEFERRED verdicts on
# the way — and the GPU file replays them on the GPU.
LOSSY_SEEDS = (34, 47, 57, 63, 65)
LOSSY = dict(W=3, N=40, mop=8, P=64, q=0.1, ring_frames=16 * 40)


def worker_checksum(model, u):
    """The IPv4 header checksum of a result frame to worker u."""
    return FW.result_ipv4_checksum(model.P, model.switch_ip, model.workers[u][1])


def copy_for(model, r, u, ck=None):
    """The copy of BROADCAST result frame r that goes to worker u (`ck`:
    worker_checksum(model, u), where the caller has it at hand)."""
    mac, ip = model.workers[u]
    c = np.array(r, dtype=np.uint8, copy=True)
    FW.put(c, FW.DST_MAC, mac)
    FW.put(c, FW.IP_CHECKSUM, worker_checksum(model, u) if ck is None else ck)
    FW.put(c, FW.DST_IP, ip)
    return c


def asker(model, r):
    """The worker a RETRANSMIT answer r is addressed to (its destination
    address, first table match), or None."""
    dst = FW.get(r, FW.DST_IP)
    return next((u for u, (_, ip) in enumerate(model.workers) if ip == dst), None)


def deliver(model, frames, verdicts, results, drop, ring_counts, ring_frames):
    """One deliver call.  `frames`: the call's input frames (their count is
    all that is used: a result sits at its input frame's index); `verdicts`
    and `results` as model_call returned them ({index: result frame});
    `drop`: None or a mask per frame, bit u = the copy for worker u is lost;
    `ring_counts`: the frames already in each worker's ring.
    Returns (appended, counts, ring_counts after): appended[u] = the frames
    added to worker u's ring, in order; counts = [delivered, dropped,
    overflow, unroutable]."""
    W = model.W
    appended = [[] for _ in range(W)]
    fill = [int(c) for c in ring_counts]
    counts = [0, 0, 0, 0]
    cks = [worker_checksum(model, u) for u in range(W)]
    for i in range(len(frames)):
        v = int(verdicts[i])
        if v == M.BROADCAST:
            copies = [(u, None) for u in range(W)]
        elif v == M.RETRANSMIT:
            u = asker(model, results[i])
            if u is None:
                counts[UNROUTABLE] += 1
                continue
            copies = [(u, results[i])]
        else:
            continue
        lost = 0 if drop is None else int(drop[i])
        for u, ready in copies:
            if (lost >> u) & 1:
                counts[DROPPED] += 1
            elif fill[u] >= ring_frames:
                counts[OVERFLOW] += 1
            else:
                appended[u].append(ready if ready is not None else copy_for(model, results[i], u, cks[u]))
                fill[u] += 1
                counts[DELIVERED] += 1
    return appended, counts, fill


def gather(sets, set_idx, frame_idx):
    """sml_frame_gather: sets[s] = a list (or 2-D array) of frames.  Returns
    (out, skipped): out[j] = the frame, or None for an entry out of range."""
    out, skipped = [], 0
    for s, i in zip(set_idx, frame_idx):
        s, i = int(s), int(i)
        if 0 <= s < len(sets) and 0 <= i < len(sets[s]):
            out.append(sets[s][i])
        else:
            out.append(None)
            skipped += 1
    return out, skipped


def pkt_id(f):
    return FW.get(f, FW.PKT_ID)


# ------------------------------------------------------------ the closed loop

class ModelSwitch:
    """gather -> switch -> deliver on the model: the backend of lossy_loop
    that the GPU path is compared with, call by call.  `sets[w][p]` = worker
    w's tx frame of packet p."""

    def __init__(self, sets, workers, mop, P, ring_frames):
        self.sets, self.ring_frames = sets, ring_frames
        self.model = M.SwitchModel(workers, mop, P)
        self.fill = [0] * len(workers)
        self.rings = [[] for _ in workers]
        self.counts = [0, 0, 0, 0]
        self.verdicts = [0] * 5                               # how often each verdict came up

    def call(self, batch, drop):
        """`batch`: the gather list, (worker, packet) pairs; `drop`: a mask
        per entry.  Returns (verdicts, ring counts, the pkt_ids appended to
        each worker's ring)."""
        frames, _ = gather(self.sets, [w for w, _ in batch], [p for _, p in batch])
        verdicts, results, seen = M.model_call(self.model, frames)
        self.verdicts = [a + b for a, b in zip(self.verdicts, seen)]
        appended, counts, self.fill = deliver(self.model, frames, verdicts, results, drop, self.fill,
                                              self.ring_frames)
        for u, fs in enumerate(appended):
            self.rings[u] += fs
        self.counts = [a + b for a, b in zip(self.counts, counts)]
        return verdicts, list(self.fill), [[pkt_id(f) for f in fs] for fs in appended]


def lossy_loop(seed, W, N, mop, q, switch, max_call=None):
    """W workers run the DPDK window loop over N packets with mop slots
    against `switch` (a ModelSwitch, or anything with its call()), by
    lossy_stream's rules: a worker sends packet p + mop when it first finds
    packet p's result in its ring; a worker whose window stalls — packets
    unanswered, none of its frames waiting and no worker's frame for a packet
    of its window either — resends its oldest unanswered packet.  A call takes
    a random-length prefix of the waiting frames behind the frames the call
    before DEFERRED (resubmitted by index).  Ingress loss, as in lossy_stream:
    a frame a worker sends never enters a gather list with probability q and
    otherwise enters it twice with probability q (a duplicate that a call's
    cut separates from its twin can meet the worker's next packet for the
    slot in one call: the DEFERRED case).  Egress loss: every bit of a
    frame's drop mask is set with probability q.  The workers see only what
    switch.call returns: verdicts, ring counts, the new ring entries' pkt_ids.
    Returns the number of calls made; asserts that every worker got every
    packet within 100 N W rounds, lossy_stream's own cap."""
    rng = np.random.default_rng(seed)
    max_call = max_call or 2 * W * mop
    done = np.zeros((W, N), dtype=bool)

    def lossy(items):
        out = []
        for it in items:
            if rng.random() < q:
                continue
            out.append(it)
            if rng.random() < q:
                out.append(it)
        return [out[i] for i in rng.permutation(len(out))]

    queue = lossy([(w, p) for w in range(W) for p in range(min(mop, N))])
    deferred, seen, ncalls = [], [0] * W, 0
    for _ in range(100 * N * W):
        if done.all():
            break
        senders = {w for w, _ in queue + deferred}
        coming = {p for _, p in queue + deferred}

        def window(w):                                       # sent and not yet answered
            return [p for p in range(N) if not done[w, p] and (p < mop or done[w, p - mop])]

        queue += lossy([(w, window(w)[0]) for w in range(W)
                        if w not in senders and not done[w].all() and not coming & set(window(w))])
        take = int(rng.integers(1, max_call + 1))
        fresh, queue = queue[:take], queue[take:]
        batch = deferred + fresh
        if not batch:
            continue
        drop = [sum(1 << u for u in range(W) if rng.random() < q) for _ in batch]
        verdicts, fill, new_ids = switch.call(batch, drop)
        ncalls += 1
        deferred = [batch[i] for i in range(len(batch)) if verdicts[i] == M.DEFERRED]
        sends = []
        for w in range(W):
            assert fill[w] == seen[w] + len(new_ids[w])
            seen[w] = fill[w]
            for p in new_ids[w]:
                if not done[w, p]:                           # first copy wins
                    done[w, p] = True
                    if p + mop < N:
                        sends.append((w, p + mop))
        queue += lossy(sends)
    assert done.all(), "the closed loop did not finish"
    return ncalls
