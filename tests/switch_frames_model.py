"""The switch's frame pipeline in plain Python / numpy: the model the GPU frame
switch (sml_frame_switch, DESIGN §9 F3 "Switch side") is held to, and a seeded
generator of worker streams.

SwitchModel is strictly sequential, one frame at a time, as the P4 pipeline
sees them (bitmap_checker.p4, workers_counter.p4, processor.p4, exponents.p4,
next_step_selector.p4, udp_sender.p4): no batching, no deferral.  model_call()
puts the one rule of a GPU call on top of it — per (slot, worker) the call
handles the set of the pair's lowest-index frame, the pair's frames of the
other set are DEFERRED — by filtering the call's frames before the model sees
them.  Payloads and exponent bytes are opaque bytes to all of it.
"""
import numpy as np

from switchml_amd import frame_wire as FW
from switchml_amd.frame_wire import (SWITCH_IP, SWITCH_MAC, frame_bytes, ip_bytes, ipv4_checksum,
                                     pool_index, worker_frame)

CONSUMED, BROADCAST, RETRANSMIT, IGNORED, DEFERRED = range(5)


def default_workers(W):
    """(mac, ip) of W workers: 02:00:00:00:01:ww, 10.0.1.ww."""
    return [(bytes([2, 0, 0, 0, 1, w]), f"10.0.1.{w + 1}") for w in range(W)]


def window_frames(rng, P, workers, mop, packets):
    """One frame per (worker, packet), random bytes (per packet, per worker: the
    payload, then the two exponent bytes), workers interleaved and shuffled."""
    frames = []
    for p in packets:
        for w, worker in enumerate(workers):
            pay = rng.integers(0, 256, 4 * P, dtype=np.uint8)
            e = rng.integers(0, 256, 2, dtype=np.uint8)
            frames.append(worker_frame(P, worker, p, pool_index(p, mop), pay, e, src_port=4000 + w))
    order = rng.permutation(len(frames))
    return [frames[i] for i in order]


class SwitchModel:
    """The pipeline's registers and one frame through them."""

    def __init__(self, workers, num_slots, P, switch_mac=SWITCH_MAC, switch_ip=SWITCH_IP):
        self.workers = [(bytes(m), ip_bytes(ip)) for m, ip in workers]
        self.W, self.S, self.P = len(self.workers), num_slots, P
        self.switch_mac, self.switch_ip = bytes(switch_mac), ip_bytes(switch_ip)
        self.reset()

    def reset(self):
        self.bitmap = [[0, 0] for _ in range(self.S)]
        self.count = [[0, 0] for _ in range(self.S)]
        self.acc = np.zeros((self.S, 2, self.P), dtype=np.uint32)       # host order
        self.exps = np.zeros((self.S, 2, 2), dtype=np.int8)

    def parse(self, f):
        """(w, s, v) or None for a frame the switch ignores."""
        src = FW.get(f, FW.SRC_IP)
        w = next((i for i, (_, ip) in enumerate(self.workers) if ip == src), None)
        idx = FW.get(f, FW.POOL_INDEX)
        s, v = FW.pool_slot(idx), FW.pool_set(idx)
        if w is None or s >= self.S:
            return None
        return w, s, v

    def frame(self, f):
        """One frame: (verdict, result frame or None)."""
        key = self.parse(f)
        if key is None:
            return IGNORED, None
        w, s, v = key
        W, bit = self.W, 1 << key[0]
        before = self.bitmap[s][v]
        self.bitmap[s][v] |= bit
        self.bitmap[s][1 - v] &= ~bit
        if not before & bit:
            flag = self.count[s][v]
            self.count[s][v] = W - 1 if flag == 0 else flag - 1
            if W == 1:
                flag = 1
            words = FW.payload_words(f, self.P)
            e = f[FW.EXPS].view(np.int8)
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
            return verdict, None
        return verdict, self.result(f, w, s, v)

    def result(self, f, w, s, v):
        mac, ip = self.workers[w]
        r = np.zeros(frame_bytes(self.P), dtype=np.uint8)
        FW.put(r, FW.DST_MAC, mac)
        FW.put(r, FW.SRC_MAC, self.switch_mac)
        FW.put(r, FW.ETHERTYPE, b"\x08\x00")
        FW.put_ipv4_header(r, self.P, 64, self.switch_ip, ip)
        FW.put(r, FW.IP_CHECKSUM, ipv4_checksum(r[FW.IP_HEADER]))
        r[FW.SRC_PORT] = f[FW.DST_PORT]
        r[FW.DST_PORT] = f[FW.SRC_PORT]
        FW.put(r, FW.UDP_LEN, FW.udp_len(self.P))
        FW.put(r, FW.JOB_TYPE_SIZE, 0x10 | (FW.get(f, FW.JOB_TYPE_SIZE) & 7))
        r[FW.span(FW.JOB, FW.PKT_ID)] = f[FW.span(FW.JOB, FW.PKT_ID)]
        FW.put(r, FW.POOL_INDEX, FW.get(f, FW.POOL_INDEX) & ~FW.POOL_BIT14)
        r[FW.EXPS] = self.exps[s, v].view(np.uint8)
        FW.put_payload_words(r, self.P, self.acc[s, v])
        return r


def deferred_indices(model, frames):
    """The call rule: indices of the frames whose (slot, worker) pair carried
    the other set in the pair's lowest-index frame of the call."""
    call_set, out = {}, set()
    for i, f in enumerate(frames):
        key = model.parse(f)
        if key is None:
            continue
        w, s, v = key
        if call_set.setdefault((s, w), v) != v:
            out.add(i)
    return out


def model_call(model, frames):
    """One call: (verdicts, {index: result frame}, counts[5])."""
    skip = deferred_indices(model, frames)
    verdicts, results, counts = [], {}, [0] * 5
    for i, f in enumerate(frames):
        if i in skip:
            verdict, r = DEFERRED, None
        else:
            verdict, r = model.frame(f)
        verdicts.append(verdict)
        counts[verdict] += 1
        if r is not None:
            results[i] = r
    return np.array(verdicts, dtype=np.uint8), results, counts


def lossy_stream(seed, W, N, mop, P, q, max_call=None):
    """W workers run the DPDK window loop over N packets with mop slots against
    the model, closed loop, a call at a time.  Frames wait in one FIFO; a call
    takes a random-length prefix, runs model_call on it, puts the DEFERRED
    frames back at the front and hands the results to the workers (a BROADCAST
    to all of them).  Every frame to the switch and every result back is
    dropped with probability q and otherwise duplicated with probability q.  A
    worker sends packet p + mop when it first receives packet p's result.  A
    worker whose own window stalls — packets unanswered, none of its frames
    waiting and no worker's frame for a packet of its window either, so nothing
    under way can answer it — resends its oldest unanswered packet, behind the
    other workers' live traffic.  Frames a worker sends after a result queue behind
    everything already waiting, and a worker resends only a packet whose result
    it lacks, so no copy of packet p trails the worker's packet p + mop: the
    protocol's window.

    Returns (calls, payloads, exps): calls[i] = the frames that ARRIVE for call
    i (the caller prepends what call i - 1 deferred), payloads[w][p] the wire
    bytes and exps[w][p] the two exponent bytes worker w sends as packet p."""
    rng = np.random.default_rng(seed)
    workers = default_workers(W)
    model = SwitchModel(workers, mop, P)
    payloads = rng.integers(0, 256, size=(W, N, 4 * P), dtype=np.uint8)
    exps = rng.integers(0, 256, size=(W, N, 2), dtype=np.uint8)
    max_call = max_call or 2 * W * mop

    def frame_of(w, p):
        return worker_frame(P, workers[w], p, pool_index(p, mop), payloads[w, p], exps[w, p], src_port=4000 + w)

    def lossy(items):
        out = []
        for it in items:
            if rng.random() < q:
                continue
            out.append(it)
            if rng.random() < q:
                out.append(it)
        rng.shuffle(out)
        return out

    done = np.zeros((W, N), dtype=bool)
    queue = lossy([(w, p) for w in range(W) for p in range(min(mop, N))])
    deferred, calls = [], []
    for _ in range(100 * N * W):
        if done.all():
            break
        senders = {w for w, _ in queue + deferred}
        coming = {p for _, p in queue + deferred}

        def window(w):                                       # sent and not yet answered
            return [p for p in range(N) if not done[w, p] and (p < mop or done[w, p - mop])]

        stalled = [w for w in range(W) if w not in senders and not done[w].all() and not coming & set(window(w))]
        queue += lossy([(w, window(w)[0]) for w in stalled])
        if not queue and not deferred:
            continue
        take = int(rng.integers(1, max_call + 1))
        fresh, queue = queue[:take], queue[take:]
        calls.append([frame_of(w, p) for w, p in fresh])
        batch = deferred + fresh
        verdicts, results, _ = model_call(model, [frame_of(w, p) for w, p in batch])
        deferred = [batch[i] for i in range(len(batch)) if verdicts[i] == DEFERRED]
        sends = []
        for i in sorted(results):
            w, p = batch[i]
            for to in lossy(list(range(W)) if verdicts[i] == BROADCAST else [w]):
                if not done[to, p]:
                    done[to, p] = True
                    if p + mop < N:
                        sends.append((to, p + mop))
        queue += lossy(sends)
    assert done.all(), "the generated stream did not finish"
    return calls, payloads, exps
