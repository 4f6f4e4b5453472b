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
import socket
import struct

import numpy as np

CONSUMED, BROADCAST, RETRANSMIT, IGNORED, DEFERRED = range(5)
HEADER = 52


def frame_bytes(P):
    return HEADER + 4 * P


def ip_bytes(ip):
    return socket.inet_aton(ip)


def default_workers(W):
    """(mac, ip) of W workers: 02:00:00:00:01:ww, 10.0.1.ww."""
    return [(bytes([2, 0, 0, 0, 1, w]), f"10.0.1.{w + 1}") for w in range(W)]


SWITCH_MAC = bytes([2, 0, 0, 0, 0, 1])
SWITCH_IP = "10.0.0.253"


def pool_index(p, mop, start=0):
    """PktId2PoolIndex with shift 0: slot p % mop, sets alternate per window."""
    i = p % (2 * mop)
    return (start + i) & 0xffff if i < mop else ((start + i - mop) | 0x8000) & 0xffff


def worker_frame(P, worker, pkt_id, pool_idx, payload, exps=(0, 0), src_port=4000, dst_port=48879, job=0,
                 switch_mac=SWITCH_MAC, switch_ip=SWITCH_IP):
    """A frame as BuildPacket lays it out (the fields a switch reads, and the
    rest plausible): `worker` = (mac, ip), payload = 4P wire bytes (uint8 array
    or bytes), exps = the two bytes at 50-51."""
    n = frame_bytes(P)
    f = np.zeros(n, dtype=np.uint8)
    f[0:6] = list(switch_mac)
    f[6:12] = list(worker[0])
    f[12:14] = [0x08, 0x00]
    f[14] = 0x45
    f[16:18] = [(n - 14) >> 8, (n - 14) & 0xff]
    f[22], f[23] = 128, 17
    f[26:30] = list(ip_bytes(worker[1]))
    f[30:34] = list(ip_bytes(switch_ip))
    f[34:36] = [src_port >> 8, src_port & 0xff]
    f[36:38] = [dst_port >> 8, dst_port & 0xff]
    f[38:40] = [(n - 34) >> 8, (n - 34) & 0xff]
    f[42] = (1 << 4) + (0 if P < 64 else 1 if P < 128 else 2 if P < 256 else 3)
    f[43] = job & 0xff
    f[44:48] = list(struct.pack("<I", pkt_id))
    f[48:50] = [pool_idx >> 8, pool_idx & 0xff]
    f[50:52] = [exps[0] & 0xff, exps[1] & 0xff]
    f[52:] = np.frombuffer(bytes(payload), dtype=np.uint8) if not isinstance(payload, np.ndarray) else payload
    return f


def ipv4_checksum(hdr20):
    s = 0
    for i in range(0, 20, 2):
        s += (int(hdr20[i]) << 8) | int(hdr20[i + 1])
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return ~s & 0xffff


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
        src = bytes(f[26:30])
        w = next((i for i, (_, ip) in enumerate(self.workers) if ip == src), None)
        idx = (int(f[48]) << 8) | int(f[49])
        s, v = idx & 0x3fff, idx >> 15
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
            words = f[52:52 + 4 * self.P].view(">u4").astype(np.uint32)      # ntohl
            e = f[50:52].view(np.int8)
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
        n = frame_bytes(self.P)
        mac, ip = self.workers[w]
        r = np.zeros(n, dtype=np.uint8)
        r[0:6] = list(mac)
        r[6:12] = list(self.switch_mac)
        r[12:14] = [0x08, 0x00]
        r[14], r[15] = 0x45, 0x00
        r[16:18] = [(n - 14) >> 8, (n - 14) & 0xff]
        r[22], r[23] = 64, 17
        r[26:30] = list(self.switch_ip)
        r[30:34] = list(ip)
        ck = ipv4_checksum(r[14:34])
        r[24:26] = [ck >> 8, ck & 0xff]
        r[34:36] = f[36:38]
        r[36:38] = f[34:36]
        r[38:40] = [(n - 34) >> 8, (n - 34) & 0xff]
        r[42] = 0x10 | (int(f[42]) & 7)
        r[43:48] = f[43:48]
        r[48] = int(f[48]) & ~0x40 & 0xff
        r[49] = f[49]
        r[50:52] = self.exps[s, v].view(np.uint8)
        r[52:] = self.acc[s, v].astype(">u4").view(np.uint8)                  # htonl
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
