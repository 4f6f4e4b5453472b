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
Usage: bench_switch_frames.py [OUT.json] | --deliver [OUT.json] | --deliver-trace"""
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


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--deliver":
        sys.exit(main_deliver(sys.argv[2] if len(sys.argv) > 2 else None))
    if len(sys.argv) > 1 and sys.argv[1] == "--deliver-trace":
        sys.exit(main_deliver(trace_only=True))
    sys.exit(main())
