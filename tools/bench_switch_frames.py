#!/usr/bin/env python3
"""The frame switch (sml_frame_switch: claim, verdicts, apply, results) in
microseconds per call.  A SIDE measurement: bench.py and its headline do not
change.

  (a) a window: W = 8, mop = num_slots = 256, P = 256 — 2048 frames per call,
      every call completes its 256 slots (calls alternate the slots' two sets,
      as consecutive windows do).  Expected to be launch-bound: four launches.
  (b) a large batch: W = 8, num_slots = 16384, one frame per (slot, worker) —
      131072 frames, ~141 MB in, 16384 result frames out; 4 frame sets cycled
      (past the 256 MiB Infinity Cache), sets alternating.
For (b) also: the call's algorithmic bytes over its time (every input frame
read once, the slots' words written once and read once for the results, the
result frames written), beside sml_stream_copy moving the same number of bytes
(half read, half written) in the same process — the practical ceiling — and
beside K6 (sml_switch_aggregate, payload and exponent planes out) at W = 8 on
planes holding the same payload.  Interleaved rounds, medians with the rounds'
min-max, HIP events around `reps` calls.  Before anything is timed, one call of
each shape is checked: the verdict counts, and a result frame's words against
the sum of its slot's payloads.
--deliver: the egress (sml_frame_switch_deliver) on the same two shapes, alone
and behind the switch call, beside sml_stream_copy of its own algorithmic bytes
(main_deliver below); --deliver-trace: a few untimed calls of those arms, to
run under rocprofv3 --kernel-trace.
--rdma: the RDMA switch (sml_rdma_switch) on the same two shapes, beside the
copy and the frame path (main_rdma below); --rdma --msg-numel M[,M...]: the
RDMA switch at those message lengths, sml_msg_switch beside sml_rdma_switch
where both serve one and beside the copy (main_rdma_long below).
--rdma-worker: the RDMA worker's completion loop (sml_rdma_worker_poll) beside
the per-packet exchange bursts and the copy (main_rdma_worker below);
--rdma-worker --msg-numel M[,M...]: the loop at those message lengths,
sml_msg_worker_poll beside the copy and, at 1024, beside sml_rdma_worker_poll
(main_msg_worker below).
--frame-worker: the DPDK worker's receive loop (sml_frame_worker_poll) beside
the bulk tx + rx pair over as many frames and the copy (main_frame_worker below).
Usage: bench_switch_frames.py [OUT.json] | --deliver [OUT.json] | --deliver-trace | --rdma [OUT.json]
       | --rdma --msg-numel M[,M...] [OUT.json] | --rdma-worker [OUT.json]
       | --rdma-worker --msg-numel M[,M...] [OUT.json] | --frame-worker [OUT.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p4app-switchml_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import switchml_amd as sw  # noqa: E402
from switchml_amd import frame_wire as FW  # noqa: E402

WORKERS = [(bytes([2, 0, 0, 0, 1, w]), f"10.0.1.{w + 1}") for w in range(8)]


def header_block(S, W, P, set_bit, seed):
    """The headers of frame_set's frames, up to the exponents, on the host:
    one per (slot, worker) in a seeded arrival order, the fields a switch
    reads.  Returns (hdr [S W, bytes before the exponents], slot, w)."""
    F = S * W
    order = np.random.default_rng(seed).permutation(F)
    slot, w = order // W, order % W
    hdr = np.zeros((F, FW.EXP.start), dtype=np.uint8)
    FW.put(hdr, FW.ETHERTYPE, b"\x08\x00")
    FW.put(hdr, FW.IP_VER_TOS, b"\x45\x00")
    FW.put(hdr, FW.IP_PROTO, 17)
    FW.put(hdr, FW.SRC_IP, FW.ip_bytes("10.0.1.0"))
    hdr[:, FW.SRC_IP.stop - 1] = w + 1                               # 10.0.1.w+1, as WORKERS
    FW.put(hdr, FW.DST_IP, FW.ip_bytes(FW.SWITCH_IP))
    FW.put(hdr, FW.SRC_PORT, 4000 + w)
    FW.put(hdr, FW.DST_PORT, 48879)
    FW.put(hdr, FW.JOB_TYPE_SIZE, FW.job_type_size(P))
    FW.put(hdr, FW.PKT_ID, slot)
    FW.put(hdr, FW.POOL_INDEX, slot | (set_bit << 15))
    return hdr, slot, w


def frame_set(S, W, P, set_bit, seed, dev):
    """One frame per (slot, worker) in a seeded arrival order: random payload
    and exponent bytes on the device, the header fields a switch reads."""
    fb = sw.frame_bytes(P)
    F = S * W
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    frames = torch.randint(0, 256, (F, fb), dtype=torch.uint8, device=dev, generator=g)
    hdr, slot, w = header_block(S, W, P, set_bit, seed)
    frames[:, :FW.EXP.start] = torch.from_numpy(hdr).to(dev)
    return frames.reshape(-1), slot, w


def check_call(fs, frames, slot, S, W, P):
    """One call on fresh registers: W - 1 CONSUMED and one BROADCAST per slot,
    and slot 0's result carries the wrapping sum of its W payloads."""
    fb = sw.frame_bytes(P)
    fs.reset()
    fs.counts.zero_()
    out, verdict, counts = fs(frames, S * W)
    torch.cuda.synchronize()
    assert counts.tolist() == [S * (W - 1), S, 0, 0, 0], counts.tolist()
    fr = frames.view(-1, fb)
    mine = np.flatnonzero(slot == 0)
    words = FW.payload_words(fr[torch.from_numpy(mine).to(fr.device)].cpu().numpy(), P).sum(axis=0, dtype=np.uint32)
    i = int(mine[verdict[torch.from_numpy(mine).to(verdict.device)].cpu().numpy() == sw.VERDICT_BROADCAST][0])
    got = FW.payload_words(out.view(-1, fb)[i].cpu().numpy(), P)
    assert np.array_equal(got, words), "result words != sum of the slot's payloads"


def timed(fn, st, reps, step):
    for _ in range(4):                                       # (an even count: the sets keep alternating)
        fn(step[0])
        step[0] += 1
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn(step[0])
        step[0] += 1
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main(rounds=7, W=8, P=256):
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    fb = sw.frame_bytes(P)
    res = {}

    # ---- (a) a window per call ------------------------------------------
    Sa = 256
    fsa = sw.FrameSwitch(WORKERS, Sa, P, device=dev)
    seta = [frame_set(Sa, W, P, k & 1, 20 + k, dev) for k in range(2)]
    outa = torch.zeros(Sa * W * fb, dtype=torch.uint8, device=dev)
    vda = torch.empty(Sa * W, dtype=torch.uint8, device=dev)
    check_call(fsa, seta[0][0], seta[0][1], Sa, W, P)
    fsa.reset()

    def call_a(k):
        fsa(seta[k & 1][0], Sa * W, out=outa, verdict=vda, stream=st)

    # ---- (b) a large batch ----------------------------------------------
    Sb, nbuf = 16384, 4
    Fb = Sb * W
    fsb = sw.FrameSwitch(WORKERS, Sb, P, device=dev)
    setb = [frame_set(Sb, W, P, k & 1, 40 + k, dev) for k in range(nbuf)]
    outb = torch.zeros(Fb * fb, dtype=torch.uint8, device=dev)
    vdb = torch.empty(Fb, dtype=torch.uint8, device=dev)
    check_call(fsb, setb[0][0], setb[0][1], Sb, W, P)
    fsb.reset()

    def call_b(k):
        fsb(setb[k % nbuf][0], Fb, out=outb, verdict=vdb, stream=st)

    alg = Fb * fb + 2 * Sb * P * 4 + Sb * fb + Fb            # frames in, words out and back, results, verdicts
    half = (alg // 2 + 4095) // 4096 * 4096
    src = [torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(nbuf)]
    dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

    def copy(k):
        sw.stream_copy(src[k % nbuf], dst[k % nbuf], stream=st)

    # K6 on planes of the same payload: W planes of Sb * P words, cycled
    planes = [[torch.empty(Sb * P, dtype=torch.int32, device=dev).random_(-2 ** 31, 2 ** 31 - 1) for _ in range(W)]
              for _ in range(nbuf)]
    pexps = [[torch.randint(-60, 20, (Sb,), dtype=torch.int8, device=dev) for _ in range(W)] for _ in range(nbuf)]
    pout = torch.empty(Sb * P, dtype=torch.int32, device=dev)
    eout = torch.empty(Sb, dtype=torch.int8, device=dev)

    def k6(k):
        sw.switch_aggregate(planes[k % nbuf], pexps[k % nbuf], Sb * P, P, payload_out=pout, exps_out=eout, stream=st)

    k6_bytes = (W + 1) * Sb * P * 4 + (W + 1) * Sb
    arms = {"window": (call_a, 200), "batch": (call_b, 10), "stream_copy": (copy, 10), "k6_planes": (k6, 10)}
    times = {name: [] for name in arms}
    step = [0]
    for _ in range(rounds):
        for name, (fn, reps) in arms.items():
            assert step[0] % 2 == 0 and reps % 2 == 0        # a switch's calls alternate its slots' sets
            times[name].append(timed(fn, st, reps, step))
    for name, v in times.items():
        res[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    us = {name: statistics.median(v) for name, v in times.items()}
    res["window"]["frames_per_call"] = Sa * W
    res["batch"].update(frames_per_call=Fb, bytes_in=Fb * fb, algorithmic_bytes=alg,
                        TBps_algorithmic=round(alg / us["batch"] / 1e6, 3))
    res["stream_copy"].update(bytes_moved=2 * half, TBps=round(2 * half / us["stream_copy"] / 1e6, 3))
    res["k6_planes"].update(algorithmic_bytes=k6_bytes, TBps_algorithmic=round(k6_bytes / us["k6_planes"] / 1e6, 3))
    out = {"what": f"side measurement (not bench.py's headline): sml_frame_switch, W={W}, P={P}; window: num_slots=256, "
                   f"2048 frames per call; batch: num_slots=16384, one frame per (slot, worker), {nbuf} cycled frame "
                   f"sets (cold); {rounds} interleaved rounds, medians with the rounds' min-max, HIP events",
           "device": torch.cuda.get_device_name(0), "arms": res,
           "batch_time_over_stream_copy": round(us["batch"] / us["stream_copy"], 3),
           "batch_time_over_k6_planes": round(us["batch"] / us["k6_planes"], 3)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    return 0


def main_deliver(out_path=None, rounds=7, W=8, P=256, trace_only=False):
    """The egress (sml_frame_switch_deliver) on the same two shapes: deliver
    alone on one switch call's results, and switch + deliver, beside
    sml_stream_copy of deliver's algorithmic bytes (R result frames read once,
    W R copies written, the verdicts).  The rings are long enough for a timed
    run's calls and are emptied (reset_rings) before each, so every call
    appends and writes.  trace_only: a few untimed calls of each arm, for a
    rocprofv3 --kernel-trace run of its own."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    fb = sw.frame_bytes(P)
    shapes = {"window": (256, 2, 200), "batch": (16384, 4, 10)}     # num_slots, cycled frame sets, reps
    if trace_only:
        shapes = {k: (S, nb, 4) for k, (S, nb, _) in shapes.items()}
    arms, meta = {}, {}
    for name, (S, nbuf, reps) in shapes.items():
        F = S * W
        fs = sw.FrameSwitch(WORKERS, S, P, device=dev)
        sets = [frame_set(S, W, P, k & 1, 60 + k, dev) for k in range(nbuf)]
        out = torch.zeros(F * fb, dtype=torch.uint8, device=dev)
        vd = torch.empty(F, dtype=torch.uint8, device=dev)
        ring_frames = (reps + 4) * S
        rings = torch.zeros((W, ring_frames, fb), dtype=torch.uint8, device=dev)
        # checked before anything is timed: every ring gets the call's S results, addressed to its worker
        fs(sets[0][0], F, out=out, verdict=vd)
        fs.deliver(out, vd, F, rings=rings)
        torch.cuda.synchronize()
        assert fs.ring_count.tolist() == [S] * W and fs.deliver_counts.tolist() == [S * W, 0, 0, 0]
        src_frames = out.view(F, fb)[vd == sw.VERDICT_BROADCAST]
        for u in (0, W - 1):
            got = rings[u, :S]
            assert torch.equal(got[:, FW.SRC_PORT.start:], src_frames[:, FW.SRC_PORT.start:])
            assert bool((got[:, FW.DST_IP.stop - 1] == u + 1).all())             # 10.0.1.u+1
        fs.reset()

        def deliver_only(k, fs=fs, out=out, vd=vd, F=F, rings=rings):
            fs.deliver(out, vd, F, rings=rings, stream=st)

        def switch_deliver(k, fs=fs, sets=sets, nbuf=nbuf, out=out, vd=vd, F=F, rings=rings):
            fs(sets[k % nbuf][0], F, out=out, verdict=vd, stream=st)
            fs.deliver(out, vd, F, rings=rings, stream=st)

        alg = S * fb + W * S * fb + F
        half = (alg // 2 + 4095) // 4096 * 4096
        src = [torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(nbuf)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

        def copy(k, src=src, dst=dst, nbuf=nbuf):
            sw.stream_copy(src[k % nbuf], dst[k % nbuf], stream=st)

        # deliver alone runs on the results of the last switch call: switch_deliver leaves them in out / vd
        arms[name + "_switch_deliver"] = (switch_deliver, reps, fs)
        arms[name + "_deliver"] = (deliver_only, reps, fs)
        arms[name + "_stream_copy"] = (copy, reps, None)
        meta[name] = dict(frames_per_call=F, result_frames=S, copies_written=W * S, algorithmic_bytes=alg,
                          copy_bytes_moved=2 * half)
    times = {name: [] for name in arms}
    step = [0]
    for _ in range(1 if trace_only else rounds):
        for name, (fn, reps, fs) in arms.items():
            assert step[0] % 2 == 0 and reps % 2 == 0            # a switch's calls alternate its slots' sets
            if fs is not None:
                fs.reset_rings()
            times[name].append(timed(fn, st, reps, step))
    if trace_only:
        return 0
    res = {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    for name, m in meta.items():
        us = statistics.median(times[name + "_deliver"])
        cp = statistics.median(times[name + "_stream_copy"])
        res[name + "_deliver"].update(m, TBps_algorithmic=round(m["algorithmic_bytes"] / us / 1e6, 3),
                                      time_over_stream_copy=round(us / cp, 3))
        res[name + "_stream_copy"].update(TBps=round(m["copy_bytes_moved"] / cp / 1e6, 3))
    text = json.dumps({
        "what": f"side measurement (not bench.py's headline): sml_frame_switch_deliver, W={W}, P={P}, on "
                f"bench_switch_frames.py's two shapes (window: 256 slots, 2048 frames, 256 BROADCASTs; batch: 16384 "
                f"slots, 131072 frames, 16384 BROADCASTs); deliver alone, switch + deliver, and sml_stream_copy of "
                f"deliver's algorithmic bytes; {rounds} interleaved rounds, medians with the rounds' min-max, HIP "
                f"events; nothing here was measured before this file was written",
        "device": torch.cuda.get_device_name(0), "arms": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


def main_rdma(out_path=None, rounds=7, W=8, M=256):
    """The RDMA switch (sml_rdma_switch: claim, verdicts, apply + results) on
    the same two shapes, a message per (slot, worker), every call completing
    its slots and writing W results per slot: beside sml_stream_copy of its own
    algorithmic bytes (every message and record read once, the slots' words
    written once, W S results written) and beside the frame path, sml_frame_switch
    + sml_frame_switch_deliver at P = M, in the same process."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    fb = sw.frame_bytes(M)
    arms, meta = {}, {}
    for name, (S, nbuf, reps) in {"window": (256, 2, 200), "batch": (16384, 4, 10)}.items():
        F = S * W
        rs = sw.RdmaSwitch(W, S, M, 1, device=dev)
        landing = [torch.empty((F, 4 * M), dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(nbuf)]
        rx = torch.zeros((W, S * 4 * M), dtype=torch.uint8, device=dev)
        recs = []
        for k in range(nbuf):                                # message slot * W + w, in a seeded arrival order
            order = np.random.default_rng(80 + k).permutation(F)
            a = np.zeros(F, dtype=np.dtype(sw.rdma_switch.ARRIVAL_FIELDS))
            a["worker"], a["rkey"], a["imm"], a["src"] = order % W, (order // W) << 1 | (k & 1), order // W, order
            a["addr"] = (order // W) * 4 * M
            recs.append(torch.from_numpy(a.view(np.uint8)).to(dev))
        vd = torch.empty(F, dtype=torch.uint8, device=dev)
        imm = torch.zeros(F, dtype=torch.int32, device=dev)
        # checked before anything is timed: every slot completes, every region holds slot 0's wrapping sum
        rs.step(recs[0], landing[0], rx, verdict=vd, out_imm=imm)
        torch.cuda.synchronize()
        assert rs.counts.tolist() == [S * (W - 1), S, 0, 0, 0, 0], rs.counts.tolist()
        want = landing[0][:W].cpu().numpy().view(">u4").astype(np.uint32).sum(axis=0, dtype=np.uint32)
        for u in (0, W - 1):
            assert np.array_equal(rx[u, :4 * M].cpu().numpy().view(">u4").astype(np.uint32), want)
        rs.reset()

        fs = sw.FrameSwitch(WORKERS, S, M, device=dev)
        sets = [frame_set(S, W, M, k & 1, 60 + k, dev) for k in range(nbuf)]
        out = torch.zeros(F * fb, dtype=torch.uint8, device=dev)
        fvd = torch.empty(F, dtype=torch.uint8, device=dev)
        rings = torch.zeros((W, (reps + 4) * S, fb), dtype=torch.uint8, device=dev)

        def rdma(k, rs=rs, recs=recs, landing=landing, rx=rx, vd=vd, imm=imm, nbuf=nbuf):
            rs.step(recs[k % nbuf], landing[k % nbuf], rx, verdict=vd, out_imm=imm, stream=st)

        def frames(k, fs=fs, sets=sets, nbuf=nbuf, out=out, fvd=fvd, F=F, rings=rings):
            fs(sets[k % nbuf][0], F, out=out, verdict=fvd, stream=st)
            fs.deliver(out, fvd, F, rings=rings, stream=st)

        alg = F * 4 * M + 24 * F + S * 4 * M + W * S * 4 * M
        half = (alg // 2 + 4095) // 4096 * 4096
        src = [torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(nbuf)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

        def copy(k, src=src, dst=dst, nbuf=nbuf):
            sw.stream_copy(src[k % nbuf], dst[k % nbuf], stream=st)

        arms[name + "_rdma_switch"] = (rdma, reps, None)
        arms[name + "_frame_switch_deliver"] = (frames, reps, fs)
        arms[name + "_stream_copy"] = (copy, reps, None)
        meta[name] = dict(messages_per_call=F, results_written=W * S, algorithmic_bytes=alg, copy_bytes_moved=2 * half)
    times = {name: [] for name in arms}
    step = [0]
    for _ in range(rounds):
        for name, (fn, reps, fs) in arms.items():
            assert step[0] % 2 == 0 and reps % 2 == 0            # a switch's calls alternate its slots' sets
            if fs is not None:
                fs.reset_rings()
            times[name].append(timed(fn, st, reps, step))
    res = {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    for name, m in meta.items():
        us, cp = (statistics.median(times[name + a]) for a in ("_rdma_switch", "_stream_copy"))
        fr = statistics.median(times[name + "_frame_switch_deliver"])
        res[name + "_rdma_switch"].update(m, TBps_algorithmic=round(m["algorithmic_bytes"] / us / 1e6, 3),
                                          time_over_stream_copy=round(us / cp, 3),
                                          frame_path_over_rdma=round(fr / us, 3))
        res[name + "_stream_copy"].update(TBps=round(m["copy_bytes_moved"] / cp / 1e6, 3))
    text = json.dumps({
        "what": f"side measurement (not bench.py's headline): sml_rdma_switch, W={W}, msg_numel={M}, pkts_per_msg=1, "
                f"on bench_switch_frames.py's two shapes (window: 256 slots, 2048 arrivals; batch: 16384 slots, "
                f"131072 arrivals; every call completes its slots and writes W results per slot), beside "
                f"sml_stream_copy of its algorithmic bytes and sml_frame_switch + sml_frame_switch_deliver at P={M} "
                f"in the same process; {rounds} interleaved rounds, medians with the rounds' min-max, HIP events; "
                f"nothing here was measured before this file was written",
        "device": torch.cuda.get_device_name(0), "arms": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


def main_rdma_long(out_path, Ms, rounds=7, W=8):
    """The RDMA switch at the message lengths `Ms`, on main_rdma's method: a
    256-slot window, and a batch of 16384 * 1024 / M slots (the same bytes at
    every M), a message per (slot, worker), every call completing its slots and
    writing W results per slot.  M = 1024 runs both families on records that
    differ in pkts_per_msg alone (4: sml_rdma_switch, 3: sml_msg_switch); any
    other M the long path, beside sml_stream_copy of the call's algorithmic
    bytes (every message and record read once, the accumulators written once, W
    results per slot)."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    arms, meta = {}, {}
    for M in Ms:
        paths = {"sml_rdma_switch": 4, "sml_msg_switch": 3} if M == 1024 else {"sml_msg_switch": M // 256}
        for shape, (S, nbuf, reps) in {"window": (256, 2, 200), "batch": (16384 * 1024 // M, 4, 10)}.items():
            F, tag = S * W, f"m{M}_{shape}"
            landing = [torch.empty((F, 4 * M), dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(nbuf)]
            rx = torch.zeros((W, S * 4 * M), dtype=torch.uint8, device=dev)
            vd = torch.empty(F, dtype=torch.uint8, device=dev)
            imm = torch.zeros(F, dtype=torch.int32, device=dev)
            alg = F * 4 * M + 24 * F + S * 4 * M + W * S * 4 * M
            for entry, ppm in paths.items():
                rs = sw.RdmaSwitch(W, S, M, ppm, device=dev)
                assert rs.entry == entry
                recs = []
                for k in range(nbuf):                        # message slot * W + w, in a seeded arrival order
                    order = np.random.default_rng(80 + k).permutation(F)
                    a = np.zeros(F, dtype=np.dtype(sw.rdma_switch.ARRIVAL_FIELDS))
                    a["worker"], a["rkey"], a["imm"] = order % W, (order // W * ppm) << 1 | (k & 1), order // W
                    a["src"], a["addr"] = order, (order // W) * 4 * M
                    recs.append(torch.from_numpy(a.view(np.uint8)).to(dev))
                # checked before anything is timed: every slot completes, the regions hold slot 0's wrapping sum
                rs.step(recs[0], landing[0], rx, verdict=vd, out_imm=imm)
                torch.cuda.synchronize()
                assert rs.counts.tolist() == [S * (W - 1), S, 0, 0, 0, 0], rs.counts.tolist()
                want = landing[0][:W].cpu().numpy().view(">u4").astype(np.uint32).sum(axis=0, dtype=np.uint32)
                for u in (0, W - 1):
                    assert np.array_equal(rx[u, :4 * M].cpu().numpy().view(">u4").astype(np.uint32), want)
                rs.reset()

                def call(k, rs=rs, recs=recs, landing=landing, rx=rx, vd=vd, imm=imm, nbuf=nbuf):
                    rs.step(recs[k % nbuf], landing[k % nbuf], rx, verdict=vd, out_imm=imm, stream=st)

                arms[f"{tag}_{entry}"] = (call, reps)
            half = (alg // 2 + 4095) // 4096 * 4096
            src = [torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(nbuf)]
            dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

            def copy(k, src=src, dst=dst, nbuf=nbuf):
                sw.stream_copy(src[k % nbuf], dst[k % nbuf], stream=st)

            arms[tag + "_stream_copy"] = (copy, reps)
            meta[tag] = dict(msg_numel=M, num_slots=S, messages_per_call=F, results_written=W * S, algorithmic_bytes=alg,
                             copy_bytes_moved=2 * half, entries=list(paths))
    times = {name: [] for name in arms}
    step = [0]
    for _ in range(rounds):
        for name, (fn, reps) in arms.items():
            assert step[0] % 2 == 0 and reps % 2 == 0            # a switch's calls alternate its slots' sets
            times[name].append(timed(fn, st, reps, step))
    med = {name: statistics.median(v) for name, v in times.items()}
    res = {name: {"median_us": round(med[name], 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    for tag, m in meta.items():
        shape = tag.split("_")[1]
        old = f"m1024_{shape}_sml_rdma_switch"                     # time per byte against the existing kernel's
        for entry in m.pop("entries"):
            us = med[f"{tag}_{entry}"]
            res[f"{tag}_{entry}"].update(m, TBps_algorithmic=round(m["algorithmic_bytes"] / us / 1e6, 3),
                                         time_over_stream_copy=round(us / med[tag + "_stream_copy"], 3))
            if old in med:
                res[f"{tag}_{entry}"]["time_per_byte_over_m1024_sml_rdma_switch"] = round(
                    us / m["algorithmic_bytes"] / (med[old] / meta[f"m1024_{shape}"]["algorithmic_bytes"]), 3)
        res[tag + "_stream_copy"].update(TBps=round(m["copy_bytes_moved"] / med[tag + "_stream_copy"] / 1e6, 3))
    text = json.dumps({
        "what": f"side measurement (not bench.py's headline): the RDMA switch at msg_numel {Ms}, W={W}; window: 256 "
                f"slots; batch: 16384 * 1024 / msg_numel slots; a message per (slot, worker), every call completes "
                f"its slots and writes W results per slot; msg_numel 1024: sml_rdma_switch (pkts_per_msg 4) and "
                f"sml_msg_switch (pkts_per_msg 3) on the same messages, else sml_msg_switch (pkts_per_msg = "
                f"msg_numel / 256); beside sml_stream_copy of the call's algorithmic bytes; all arms in one process, "
                f"{rounds} interleaved rounds, every timing warmed, medians with the rounds' min-max, HIP events; "
                f"nothing here was measured before this file was written",
        "device": torch.cuda.get_device_name(0), "arms": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


def main_rdma_worker(out_path=None, rounds=7, W=8, M=1024, reps=10):
    """The RDMA worker's completion loop (sml_rdma_worker_poll: judge, accept)
    at Q = 16384 and Q = 64 queue pairs: FLOAT32, a slice of 4 Q M elements, a
    timed step = one poll in which every QP accepts a steady-state message
    (b <= m < B - b: block m - b out, block m in, block m + b's exponent).  A
    slice has two such polls per QP, so a timing is the two of them between one
    pair of HIP events, the QP state put back (untimed) before each pair; the
    other arms are timed the same way: (b) the same messages through
    ceil(Q / 64) prebuilt sml_exchange_burst launches, the host holding the
    ids; (c) sml_stream_copy of the poll's algorithmic bytes (20 KiB a message:
    result read, output written, two slice blocks read, message written; plus
    its records).  Call time from events, not kernel time."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    arms, meta = {}, {}
    for name, Q in {"q16384": 16384, "q64": 64}.items():
        n = 4 * Q * M
        x = torch.empty(n, dtype=torch.float32, device=dev).normal_()
        out = torch.empty_like(x)
        buf = torch.empty(Q * M, dtype=torch.int32, device=dev).random_(-2 ** 31, 2 ** 31 - 1)   # tx is rx
        wk = sw.RdmaWorker(0, W, Q, M, 4, dtype=torch.float32, device=dev)
        comps = []
        for r in range(3):                                   # messages r Q + q: the first batch, then two steady ones
            c = np.zeros(Q, dtype=np.dtype(sw.rdma_worker.COMPLETION_FIELDS))
            c["qpn"], c["imm"] = np.arange(Q), ((r * Q + np.arange(Q)) & 0xFFFF) | (3 << 16)
            comps.append(torch.from_numpy(c.view(np.int64)).to(dev))
        wk.begin(x, out, buf)
        verdict, _ = wk.poll(comps[0], buf, buf)
        assert bool((verdict == sw.RDMA_WORKER_POSTED).all())
        snap = wk.state.clone()
        for r in (1, 2):                                     # checked before anything is timed: both polls post
            assert bool((wk.poll(comps[r], buf, buf)[0] == sw.RDMA_WORKER_POSTED).all())

        recv = torch.full((4 * Q,), 3, dtype=torch.int8, device=dev)
        immw = torch.zeros(Q, dtype=torch.int32, device=dev)
        bursts = [[sw.packet_burst(x, out, M, W, Q, recv, list(range(r * Q + q0, r * Q + min(q0 + 64, Q))),
                                   [buf.data_ptr() + q * 4 * M for q in range(q0, min(q0 + 64, Q))],
                                   [immw.data_ptr() + 4 * q + 2 for q in range(q0, min(q0 + 64, Q))])
                   for q0 in range(0, Q, 64)] for r in (1, 2)]

        def poll(r, wk=wk, comps=comps, buf=buf):
            wk.poll(comps[r], buf, buf, stream=st)

        def burst(r, bursts=bursts):
            for bt in bursts[r - 1]:
                sw.exchange_burst(bt, stream=st)

        alg = Q * (5 * 4 * M + 8 + 24 + 1 + 2 * 32)
        half = (alg // 2 + 4095) // 4096 * 4096
        src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)

        def copy(r, src=src, dst=dst):
            sw.stream_copy(src, dst, stream=st)

        restore = lambda wk=wk, snap=snap: wk.state.copy_(snap)                       # noqa: E731
        arms[name + "_worker_poll"] = (poll, restore)
        arms[name + "_exchange_bursts"] = (burst, None)
        arms[name + "_stream_copy"] = (copy, None)
        meta[name] = dict(messages_per_call=Q, algorithmic_bytes=alg, copy_bytes_moved=2 * half,
                          burst_launches_per_call=(Q + 63) // 64, worker_launches_per_call=2)

    def pair(fn, restore):
        if restore:
            restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn(1)
        fn(2)
        b.record(st)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 2 * 1e3

    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, (fn, restore) in arms.items():
            pair(fn, restore)                                                         # warmed
            times[name].append(statistics.median(pair(fn, restore) for _ in range(reps)))
    res = {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    for name, m in meta.items():
        us, bu, cp = (statistics.median(times[name + a]) for a in ("_worker_poll", "_exchange_bursts", "_stream_copy"))
        res[name + "_worker_poll"].update(m, TBps_algorithmic=round(m["algorithmic_bytes"] / us / 1e6, 3),
                                          time_over_stream_copy=round(us / cp, 3),
                                          exchange_bursts_over_worker_poll=round(bu / us, 3))
        res[name + "_stream_copy"].update(TBps=round(m["copy_bytes_moved"] / cp / 1e6, 3))
    text = json.dumps({
        "what": f"side measurement (not bench.py's headline): sml_rdma_worker_poll, FLOAT32, W={W}, msg_numel={M}, a "
                f"slice of 4 Q M elements, tx == rx in device memory; one call = one poll in which every QP accepts "
                f"a steady-state message, beside the same messages through ceil(Q / 64) prebuilt sml_exchange_burst "
                f"launches and sml_stream_copy of the poll's algorithmic bytes, in the same process; a timing = two "
                f"calls between one pair of HIP events (call time, not kernel time), the median of {reps} such per "
                f"round, {rounds} interleaved rounds, medians with the rounds' min-max; the buffers are reused "
                f"between timings (not cold); nothing here was measured before this file was written",
        "device": torch.cuda.get_device_name(0), "arms": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


def main_msg_worker(out_path, Ms, rounds=7, W=8, reps=10):
    """The RDMA worker's completion loop at the message lengths `Ms`, on
    main_rdma_worker's method (one poll in which every QP accepts a steady-state
    message; two such polls between one pair of HIP events, the QP state put
    back, untimed, before each pair): sml_msg_worker_poll with Q = 16384 * 1024
    // M queue pairs (the same words at every M), and at M = 4096 also a window
    of Q = 64; beside sml_stream_copy of the poll's algorithmic bytes (20 M
    bytes a message plus its records) and, at M = 1024, sml_rdma_worker_poll on
    the same work (pkts_per_msg 4 against 3)."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    arms, meta = {}, {}
    shapes = [(M, 16384 * 1024 // M) for M in Ms] + ([(4096, 64)] if 4096 in Ms else [])
    for M, Q in shapes:
        tag = f"m{M}_q{Q}"
        x = torch.empty(4 * Q * M, dtype=torch.float32, device=dev).normal_()
        out = torch.empty_like(x)
        comps = []
        for r in range(3):                                   # messages r Q + q: the first batch, then two steady ones
            c = np.zeros(Q, dtype=np.dtype(sw.rdma_worker.COMPLETION_FIELDS))
            c["qpn"], c["imm"] = np.arange(Q), ((r * Q + np.arange(Q)) & 0xFFFF) | (3 << 16)
            comps.append(torch.from_numpy(c.view(np.int64)).to(dev))
        paths = {"sml_msg_worker": 3, "sml_rdma_worker": 4} if M == 1024 else {"sml_msg_worker": M // 256}
        for entry, ppm in paths.items():
            buf = torch.empty(Q * M, dtype=torch.int32, device=dev).random_(-2 ** 31, 2 ** 31 - 1)   # tx is rx
            wk = sw.RdmaWorker(0, W, Q, M, ppm, dtype=torch.float32, device=dev)
            assert wk.entry == entry
            wk.begin(x, out, buf)
            assert bool((wk.poll(comps[0], buf, buf)[0] == sw.RDMA_WORKER_POSTED).all())
            snap = wk.state.clone()
            for r in (1, 2):                                 # checked before anything is timed: both polls post
                assert bool((wk.poll(comps[r], buf, buf)[0] == sw.RDMA_WORKER_POSTED).all())

            def poll(r, wk=wk, comps=comps, buf=buf):
                wk.poll(comps[r], buf, buf, stream=st)

            arms[f"{tag}_{entry}_poll"] = (poll, lambda wk=wk, snap=snap: wk.state.copy_(snap))
        alg = Q * (5 * 4 * M + 8 + 24 + 1 + 2 * 32)
        half = (alg // 2 + 4095) // 4096 * 4096
        src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)

        def copy(r, src=src, dst=dst):
            sw.stream_copy(src, dst, stream=st)

        arms[tag + "_stream_copy"] = (copy, None)
        meta[tag] = dict(msg_numel=M, messages_per_call=Q, waves_per_message=(M + 1023) // 1024,
                         algorithmic_bytes=alg, copy_bytes_moved=2 * half, entries=list(paths))

    def pair(fn, restore):
        if restore:
            restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn(1)
        fn(2)
        b.record(st)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 2 * 1e3

    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, (fn, restore) in arms.items():
            pair(fn, restore)                                                         # warmed
            times[name].append(statistics.median(pair(fn, restore) for _ in range(reps)))
    med = {name: statistics.median(v) for name, v in times.items()}
    res = {name: {"median_us": round(med[name], 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    for tag, m in meta.items():
        for entry in m.pop("entries"):
            us = med[f"{tag}_{entry}_poll"]
            res[f"{tag}_{entry}_poll"].update(m, TBps_algorithmic=round(m["algorithmic_bytes"] / us / 1e6, 3),
                                              ns_per_KiB=round(us * 1e3 / (m["algorithmic_bytes"] / 1024), 4),
                                              time_over_stream_copy=round(us / med[tag + "_stream_copy"], 3))
        old = f"{tag}_sml_rdma_worker_poll"
        if old in med:
            res[f"{tag}_sml_msg_worker_poll"]["time_over_sml_rdma_worker_poll"] = round(
                med[f"{tag}_sml_msg_worker_poll"] / med[old], 3)
        res[tag + "_stream_copy"].update(TBps=round(m["copy_bytes_moved"] / med[tag + "_stream_copy"] / 1e6, 3))
    text = json.dumps({
        "what": f"side measurement (not bench.py's headline): sml_msg_worker_poll at msg_numel {Ms}, FLOAT32, W={W}, "
                f"Q = 16384 * 1024 // msg_numel queue pairs (and Q = 64 at 4096), a slice of 4 Q M elements, tx == rx "
                f"in device memory; one call = one poll in which every QP accepts a steady-state message; msg_numel "
                f"1024: sml_rdma_worker_poll (pkts_per_msg 4) on the same work; beside sml_stream_copy of the poll's "
                f"algorithmic bytes; all arms in one process; a timing = two calls between one pair of HIP events "
                f"(call time, not kernel time), the QP state restored untimed before each pair, the median of {reps} "
                f"per round, {rounds} interleaved rounds, medians with the rounds' min-max; the buffers are reused "
                f"between timings (not cold); nothing here was measured before this file was written",
        "device": torch.cuda.get_device_name(0), "arms": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


def main_frame_worker(out_path=None, rounds=7, W=8, P=256, reps=10):
    """The DPDK worker's receive loop (sml_frame_worker_poll: judge, accept) at
    Q = 16384 and Q = 64 tx slots: FLOAT32, a slice of 4 Q P elements, a timed
    step = one poll over Q received frames in which every slot accepts a
    steady-state packet (b <= p < B - b: block p - b out, block p into frame
    p + b, block p + b's exponent).  A slice has two such polls per slot, so a
    timing is the two of them between one pair of HIP events, the slot state put
    back (untimed) before each pair; the other arms are timed the same way:
    (b) the route that exists without it for as many frames, one
    sml_quantize_pack_frames building Q frames (Q / 2 blocks, batch_max Q / 2,
    global exponents given) plus one sml_dequantize_frames over Q received
    frames, its rx state cleared (untimed) before each pair; (c)
    sml_stream_copy of the poll's algorithmic bytes (per frame: the frame read,
    the output block written, two slice blocks read, the frame written).  Call
    time from events, not kernel time."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    fb = sw.frame_bytes(P)
    arms, meta = {}, {}
    for name, Q in {"q16384": 16384, "q64": 64}.items():
        n = 4 * Q * P
        x = torch.empty(n, dtype=torch.float32, device=dev).normal_()
        out = torch.empty_like(x)
        prm = sw.frame_params(job_id=5, max_outstanding_pkts=Q)
        wk = sw.FrameWorker(prm, W, P, dtype=torch.float32, device=dev)
        tx = torch.zeros(Q * fb, dtype=torch.uint8, device=dev)
        rings = []
        for r in range(3):                                   # packets r Q + q: the first batch, then two steady ones
            hdr = np.zeros((Q, FW.HEADER_BYTES), dtype=np.uint8)
            FW.put(hdr, FW.JOB, 5)
            FW.put(hdr, FW.PKT_ID, r * Q + np.arange(Q))
            FW.put(hdr, FW.EXP, 3)
            fr = torch.empty((Q, fb), dtype=torch.uint8, device=dev).random_(0, 256)
            fr[:, :FW.HEADER_BYTES] = torch.from_numpy(hdr).to(dev)
            rings.append(fr.reshape(-1))
        wk.begin(x, out, tx)
        assert bool((wk.poll(rings[0], Q, tx)[0] == sw.FRAME_WORKER_POSTED).all())
        snap = wk.state.clone()
        for r in (1, 2):                                     # checked before anything is timed: both polls post
            assert bool((wk.poll(rings[r], Q, tx)[0] == sw.FRAME_WORKER_POSTED).all())

        xb = x[:Q // 2 * P]
        gexp = torch.full((Q // 2,), 3, dtype=torch.int8, device=dev)
        bulk_tx = torch.zeros(Q * fb, dtype=torch.uint8, device=dev)
        rxs = [sw.RxSlice(Q // 2 * P, P, batch_max=Q // 2, device=dev) for _ in range(2)]
        bulk_rx = sw.quantize_pack_frames(xb, prm, P, W, batch_max=Q // 2, global_exps=gexp).clone()
        sw.dequantize_frames(bulk_rx, Q, rxs[0], num_workers=W, job_id=5)
        torch.cuda.synchronize()
        assert rxs[0].counts.tolist() == [Q, 0]              # every frame of the bulk pair is accepted too

        def poll(r, wk=wk, rings=rings, tx=tx, Q=Q):
            wk.poll(rings[r], Q, tx, stream=st)

        def bulk(r, xb=xb, prm=prm, gexp=gexp, bulk_tx=bulk_tx, bulk_rx=bulk_rx, rxs=rxs, Q=Q):
            sw.quantize_pack_frames(xb, prm, P, W, batch_max=Q // 2, global_exps=gexp, frames=bulk_tx, stream=st)
            sw.dequantize_frames(bulk_rx, Q, rxs[r - 1], num_workers=W, job_id=5, stream=st)

        alg = Q * (2 * fb + 3 * 4 * P)
        half = (alg // 2 + 4095) // 4096 * 4096
        src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)

        def copy(r, src=src, dst=dst):
            sw.stream_copy(src, dst, stream=st)

        arms[name + "_worker_poll"] = (poll, lambda wk=wk, snap=snap: wk.state.copy_(snap))
        arms[name + "_bulk_tx_rx"] = (bulk, lambda rxs=rxs: [rx.reset() for rx in rxs])
        arms[name + "_stream_copy"] = (copy, None)
        meta[name] = dict(frames_per_call=Q, algorithmic_bytes=alg, copy_bytes_moved=2 * half,
                          bulk_launches_per_call=3, worker_launches_per_call=2)

    def pair(fn, restore):
        if restore:
            restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn(1)
        fn(2)
        b.record(st)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 2 * 1e3

    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, (fn, restore) in arms.items():
            pair(fn, restore)                                                         # warmed
            times[name].append(statistics.median(pair(fn, restore) for _ in range(reps)))
    res = {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    for name, m in meta.items():
        us, bu, cp = (statistics.median(times[name + a]) for a in ("_worker_poll", "_bulk_tx_rx", "_stream_copy"))
        res[name + "_worker_poll"].update(m, TBps_algorithmic=round(m["algorithmic_bytes"] / us / 1e6, 3),
                                          time_over_stream_copy=round(us / cp, 3),
                                          bulk_tx_rx_over_worker_poll=round(bu / us, 3))
        res[name + "_stream_copy"].update(TBps=round(m["copy_bytes_moved"] / cp / 1e6, 3))
    text = json.dumps({
        "what": f"side measurement (not bench.py's headline): sml_frame_worker_poll, FLOAT32, W={W}, P={P}, a slice of "
                f"4 Q P elements, tx and rx in device memory; one call = one poll over Q frames in which every slot "
                f"accepts a steady-state packet, beside one sml_quantize_pack_frames (Q frames built) plus one "
                f"sml_dequantize_frames (Q frames received) and sml_stream_copy of the poll's algorithmic bytes, in "
                f"the same process; a timing = two calls between one pair of HIP events (call time, not kernel "
                f"time), the median of {reps} such per round, {rounds} interleaved rounds, medians with the rounds' "
                f"min-max; the buffers are reused between timings (not cold); nothing here was measured before this "
                f"file was written",
        "device": torch.cuda.get_device_name(0), "arms": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--frame-worker":
        sys.exit(main_frame_worker(sys.argv[2] if len(sys.argv) > 2 else None))
    if len(sys.argv) > 3 and sys.argv[1] == "--rdma-worker" and sys.argv[2] == "--msg-numel":
        sys.exit(main_msg_worker(sys.argv[4] if len(sys.argv) > 4 else None, [int(m) for m in sys.argv[3].split(",")]))
    if len(sys.argv) > 1 and sys.argv[1] == "--rdma-worker":
        sys.exit(main_rdma_worker(sys.argv[2] if len(sys.argv) > 2 else None))
    if len(sys.argv) > 3 and sys.argv[1] == "--rdma" and sys.argv[2] == "--msg-numel":
        sys.exit(main_rdma_long(sys.argv[4] if len(sys.argv) > 4 else None, [int(m) for m in sys.argv[3].split(",")]))
    if len(sys.argv) > 1 and sys.argv[1] == "--rdma":
        sys.exit(main_rdma(sys.argv[2] if len(sys.argv) > 2 else None))
    if len(sys.argv) > 1 and sys.argv[1] == "--deliver":
        sys.exit(main_deliver(sys.argv[2] if len(sys.argv) > 2 else None))
    if len(sys.argv) > 1 and sys.argv[1] == "--deliver-trace":
        sys.exit(main_deliver(trace_only=True))
    sys.exit(main())
