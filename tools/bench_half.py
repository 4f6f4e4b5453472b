#!/usr/bin/env python3
"""FLOAT16 / BFLOAT16 buckets: the kernels that convert inside (K1h, K4h, the
fused round trip on 16-bit elements) against the two-step route a caller had
before them — widen to fp32 with a torch copy, run the fp32 kernel, narrow
with a torch copy — and against the fp32 kernels on the same numel.  A SIDE
measurement: bench.py and its headline do not change.

64 Mi elements, P = 256, cold HBM: the steps cycle 4 distinct buckets with
their planes (past the 256 MiB Infinity Cache).  Interleaved rounds, medians,
HIP events.  Every fused arm's result is checked equal to its two-step arm's
before anything is timed.  Arms:
  a  K1h bf16                       b  x.float() into a preallocated fp32 buffer, then K1
  c  K1 fp32, the same numel        d  K4h into bf16
  e  K4 fp32, then .to(bf16)        k4 K4 fp32 alone
  f  the fused round trip, bf16 in place
  g  widen, fp32 round trip in place, narrow      rt the fp32 round trip alone
  h  K1h fp16                       i  (a) on a slice that starts at element offset 1
Exit status 1 when a fused arm is not faster than its two-step arm.
Usage: bench_half.py [OUT.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p4app-switchml_amd")]

import torch  # noqa: E402
import switchml_amd as sw  # noqa: E402


def main(N=64 << 20, nbuf=4, rounds=7, reps=20, P=256, W=1):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    B = sw.num_blocks(N, P)
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    # gradient-like bf16 buckets; +1 element so that arm i can start at offset 1
    big = [torch.randn(N + 1, device=dev, generator=g).mul_(0.01).to(bf) for _ in range(nbuf)]
    xb = [t[:N] for t in big]
    xo = [t[1:] for t in big]
    xh = [t.to(f16) for t in xb]
    xr = [t.clone() for t in xb]                      # round-trip buckets (rewritten in place)
    wide = [torch.empty(N, dtype=f32, device=dev) for _ in range(nbuf)]
    pls = [torch.empty(B * P, dtype=torch.int32, device=dev) for _ in range(nbuf)]
    exs = [torch.empty(B, dtype=torch.int8, device=dev) for _ in range(nbuf)]
    ob = [torch.empty(N, dtype=bf, device=dev) for _ in range(nbuf)]
    st = torch.cuda.current_stream()

    def k1(x, k):
        sw.quantize_pack(x, P, W, payload=pls[k], exps_out=exs[k], stream=st)

    def arm_a(k): k1(xb[k], k)
    def arm_b(k): wide[k].copy_(xb[k]); k1(wide[k], k)
    def arm_c(k): k1(wide[k], k)
    def arm_d(k): sw.dequantize(pls[k], exs[k], N, P, W, out=ob[k], stream=st)
    def arm_e(k): sw.dequantize(pls[k], exs[k], N, P, W, out=wide[k], stream=st); ob[k].copy_(wide[k])
    def arm_k4(k): sw.dequantize(pls[k], exs[k], N, P, W, out=wide[k], stream=st)
    def arm_f(k): sw.roundtrip_loopback(xr[k], P, W, out=xr[k], stream=st)

    def arm_g(k):
        wide[k].copy_(xr[k])
        sw.roundtrip_loopback(wide[k], P, W, out=wide[k], stream=st)
        xr[k].copy_(wide[k])

    def arm_rt(k): sw.roundtrip_loopback(wide[k], P, W, out=wide[k], stream=st)
    def arm_h(k): k1(xh[k], k)
    def arm_i(k): k1(xo[k], k)

    # ---- every fused arm's output equals its two-step arm's -------------
    def planes(fn):
        fn(0)
        torch.cuda.synchronize()
        return pls[0].clone(), exs[0].clone()

    pa, pb = planes(arm_a), planes(arm_b)
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]), "a != b"
    arm_d(0)
    od = ob[0].clone()
    arm_e(0)
    torch.cuda.synchronize()
    assert torch.equal(od.view(torch.int16), ob[0].view(torch.int16)), "d != e"
    keep = xr[0].clone()
    arm_f(0)
    of = xr[0].clone()
    xr[0].copy_(keep)
    arm_g(0)
    torch.cuda.synchronize()
    assert torch.equal(of.view(torch.int16), xr[0].view(torch.int16)), "f != g"
    xr[0].copy_(keep)
    ph = planes(arm_h)
    wide[0].copy_(xh[0])
    pw = planes(arm_c)
    assert torch.equal(ph[0], pw[0]) and torch.equal(ph[1], pw[1]), "h != widen + K1"
    pi = planes(arm_i)
    wide[0].copy_(xo[0])
    pw = planes(arm_c)
    assert torch.equal(pi[0], pw[0]) and torch.equal(pi[1], pw[1]), "i != widen + K1"
    for k in range(nbuf):                             # arm c / k4 / rt inputs: the widened buckets
        wide[k].copy_(xb[k])
        k1(xb[k], k)

    arms = {"a": arm_a, "b": arm_b, "c": arm_c, "d": arm_d, "e": arm_e, "k4": arm_k4, "f": arm_f, "g": arm_g,
            "rt": arm_rt, "h": arm_h, "i": arm_i}
    times = {name: [] for name in arms}
    step = [0]
    for _ in range(40):
        arm_a(step[0] % nbuf)
        step[0] += 1
    for _ in range(rounds):
        for name, fn in arms.items():
            for _ in range(4):
                fn(step[0] % nbuf)
                step[0] += 1
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(reps):
                fn(step[0] % nbuf)
                step[0] += 1
            b.record(st)
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / reps * 1e3)

    us = {name: statistics.median(v) for name, v in times.items()}
    # algorithmic bytes of the fused arms and the fp32 kernels
    alg = {"a": 6 * N + B, "h": 6 * N + B, "i": 6 * N + B, "c": 8 * N + B, "d": 6 * N + B, "k4": 8 * N + B,
           "f": 4 * N, "rt": 8 * N}
    res = {name: {"median_us": round(m, 2)} for name, m in us.items()}
    for name, nbytes in alg.items():
        res[name]["TBps_algorithmic"] = round(nbytes / us[name] / 1e6, 3)
    pairs = {"a": ("b", "c", 6 / 8), "d": ("e", "k4", 6 / 8), "f": ("g", "rt", 4 / 8)}
    ok = True
    cmp = {}
    for fused, (two, fp32, byte_ratio) in pairs.items():
        cmp[fused] = {"two_step_arm": two, "speedup_over_two_step": round(us[two] / us[fused], 3),
                      "fp32_arm": fp32, "time_over_fp32_kernel": round(us[fused] / us[fp32], 3),
                      "byte_ratio": byte_ratio, "faster_than_two_step": us[fused] < us[two]}
        ok = ok and us[fused] < us[two]
    cmp["h"] = {"fp16_over_bf16_K1h": round(us["h"] / us["a"], 3)}
    cmp["i"] = {"offset1_over_aligned_K1h": round(us["i"] / us["a"], 3)}
    out = {"what": f"side measurement (not bench.py's headline): 16-bit buckets, {N >> 20} Mi elements, P={P}, W={W}, "
                   f"{nbuf} cycled buckets (cold), {rounds} interleaved rounds x {reps} launches, medians, HIP events",
           "device": torch.cuda.get_device_name(0), "arms": res, "compare": cmp, "all_fused_arms_faster": ok}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
