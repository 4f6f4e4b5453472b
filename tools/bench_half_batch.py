#!/usr/bin/env python3
"""bf16 gradient buckets through the batched round trip: one
sml_roundtrip_loopback_batch_typed call for every FIFO slice of the queued
jobs, against the route 16-bit jobs took before it — one
sml_roundtrip_loopback_typed launch per slice.  A SIDE measurement: bench.py
and its headline do not change.

Workload: the ResNet-50 bucket set of tools/bench_buckets.py (3 x 6 553 600 +
5 896 232 elements) as bf16, P = 256, W = 8, every bucket as T = 4 FIFO slices
(16 slices), out of place; the steps cycle 4 distinct bucket sets, so the data
is cold.  Interleaved rounds, medians over the rounds, HIP events; the spread
(min - max of the per-round figures) is the margin.  Arms:
  A  one typed batch call per iteration (16 bf16 slices, one launch)
  B  one sml_roundtrip_loopback_typed launch per slice, 16 launches
  C  the fp32 batch (sml_roundtrip_loopback_batch) of the same element counts
Every call's arguments are built once, before the timing: the loop pays the C
calls only.  A's output is checked equal to B's before anything is timed.

Then the same bf16 buckets through the client: posted with allreduce_async,
mode = fused, batch_jobs = 16 against batch_jobs = 0 (the threaded path), wall
clock per iteration, the two settings interleaved round by round.

Exit status 1 when arm A is slower than arm B beyond the spread.
Usage: bench_half_batch.py [OUT.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p4app-switchml_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402
import switchml_amd as sw  # noqa: E402
from switchml_amd import client as C  # noqa: E402
from bench_buckets import buckets  # noqa: E402


def fifo_slices(n, T):
    out = []
    for t in range(T):
        q, r = divmod(n, T)
        m = q + (t < r)
        out.append((t * m if t < r else t * m + r, m))
    return out


def summary(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(nsets=4, rounds=7, reps=20, P=256, W=8, T=4):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    sizes = buckets()
    bf = torch.bfloat16
    xb = [[torch.randn(n, device=dev, generator=g).mul_(1e-3).to(bf) for n in sizes] for _ in range(nsets)]
    ob = [[torch.empty_like(x) for x in s] for s in xb]
    xf = [[x.float() for x in s] for s in xb]
    of = [[torch.empty_like(x) for x in s] for s in xf]
    st = torch.cuda.current_stream()
    stp = ctypes.c_void_p(st.cuda_stream)
    L = sw.lib()

    # ---- the calls, built once ------------------------------------------
    typed, per_slice, plain = [], [], []
    for k in range(nsets):
        rows = [(x[off:off + m], o[off:off + m]) for x, o in zip(xb[k], ob[k]) for off, m in fifo_slices(x.numel(), T)]
        arr = (sw.TypedSlice * len(rows))(*[sw.TypedSlice(x.data_ptr(), o.data_ptr(), x.numel(), sw.BFLOAT16, 0)
                                            for x, o in rows])
        typed.append(arr)
        per_slice.append([(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(o.data_ptr()), sw.BFLOAT16, x.numel(), P, W,
                           None, None, 0, stp) for x, o in rows])
        rows = [(x[off:off + m], o[off:off + m]) for x, o in zip(xf[k], of[k]) for off, m in fifo_slices(x.numel(), T)]
        plain.append((sw.Slice * len(rows))(*[sw.Slice(x.data_ptr(), o.data_ptr(), x.numel()) for x, o in rows]))
    nsl = len(typed[0])

    def check(s):
        if s != sw.SML_OK:
            raise sw.SwitchMLError("bench_half_batch", s)

    def arm_a(k): check(L.sml_roundtrip_loopback_batch_typed(typed[k], nsl, P, W, 0, stp))

    def arm_b(k):
        for args in per_slice[k]:
            check(L.sml_roundtrip_loopback_typed(*args))

    def arm_c(k): check(L.sml_roundtrip_loopback_batch(plain[k], nsl, P, W, 0, stp))

    # ---- arm A's output equals arm B's ----------------------------------
    for k in range(nsets):
        arm_a(k)
        torch.cuda.synchronize()
        got = [o.clone() for o in ob[k]]
        for o in ob[k]:
            o.zero_()
        arm_b(k)
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got, ob[k])), "A != B"

    arms = {"A": arm_a, "B": arm_b, "C": arm_c}
    times = {name: [] for name in arms}
    step = 0
    for _ in range(40):
        arm_a(step % nsets)
        step += 1
    for _ in range(rounds):
        for name, fn in arms.items():
            for _ in range(4):
                fn(step % nsets)
                step += 1
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(reps):
                fn(step % nsets)
                step += 1
            b.record(st)
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / reps * 1e3)
    numel = sum(sizes)
    res = {name: dict(summary(v), unit="us per iteration") for name, v in times.items()}
    for name, nbytes in (("A", 4 * numel), ("B", 4 * numel), ("C", 8 * numel)):
        res[name]["TBps_algorithmic"] = round(nbytes / statistics.median(times[name]) / 1e6, 3)
    med = {name: statistics.median(v) for name, v in times.items()}
    slower = min(times["A"]) > max(times["B"])
    cmp = {"A_over_B_time": round(med["A"] / med["B"], 3), "A_faster": med["A"] < med["B"],
           "A_faster_beyond_spread": max(times["A"]) < min(times["B"]), "A_slower_beyond_spread": slower,
           "A_over_C_time": round(med["A"] / med["C"], 3), "byte_ratio_A_over_C": 0.5}

    # ---- through the client ---------------------------------------------
    def client_round(batch_jobs):
        C.start(C.make_config(num_workers=W, num_worker_threads=T, packet_numel=P, max_outstanding_packets=64 * T,
                              mode="fused", batch_jobs=batch_jobs, bandwidth=0))
        try:
            def iteration(k):
                jobs = [C.allreduce_async(x, o) for x, o in zip(xb[k], ob[k])]
                C.wait_for_all_jobs()
                return jobs
            for k in range(nsets):
                iteration(k)
            t0 = time.perf_counter()
            for i in range(reps):
                iteration(i % nsets)
            t = (time.perf_counter() - t0) / reps * 1e6
            return t, C.batch_stats()
        finally:
            C.stop()

    ctimes = {"batch_jobs=16": [], "batch_jobs=0": []}
    cstats = {}
    for _ in range(rounds):
        for name, bj in (("batch_jobs=16", 16), ("batch_jobs=0", 0)):
            t, cstats[name] = client_round(bj)
            ctimes[name].append(t)
    cres = {name: dict(summary(v, 1), unit="us wall clock per iteration", batch_stats_last_round=cstats[name])
            for name, v in ctimes.items()}
    cmed = {name: statistics.median(v) for name, v in ctimes.items()}
    cres["compare"] = {"batched_over_threaded_time": round(cmed["batch_jobs=16"] / cmed["batch_jobs=0"], 3),
                       "batched_faster_beyond_spread": max(ctimes["batch_jobs=16"]) < min(ctimes["batch_jobs=0"])}

    out = {"what": f"side measurement (not bench.py's headline): ResNet-50 buckets {sizes} as bf16, P={P}, W={W}, "
                   f"T={T} FIFO slices each ({nsl} slices), {nsets} cycled bucket sets (cold), {rounds} interleaved "
                   f"rounds x {reps} iterations, medians of the rounds with their min - max",
           "device": torch.cuda.get_device_name(0), "arms": res, "compare": cmp, "client": cres}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
