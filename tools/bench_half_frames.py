#!/usr/bin/env python3
"""FLOAT16 / BFLOAT16 slices over DPDK frames: the frame kernels that convert
inside (sml_quantize_pack_frames_typed, sml_dequantize_frames_typed) against
the two-step route a DPDK worker had before them — a torch widening copy into
a preallocated fp32 buffer and the fp32 tx kernel; the fp32 rx kernels into a
preallocated fp32 buffer and a torch narrowing copy — and against the fp32
frame kernels on the same numel.  A SIDE measurement: bench.py and its
headline do not change.

64 Mi elements, bf16, P = 256, W = 1, cold HBM: the steps cycle 4 distinct
input / frame / output sets (past the 256 MiB Infinity Cache).  Interleaved
rounds, medians with the rounds' min-max, HIP events.  Every fused arm's bytes
are checked equal to its two-step arm's before anything is timed.  A receive
call is rte_bitmap_reset (sml_rx_reset) + the claim and apply passes over the
slice's frames in the switch's return order (W = 1: the frames as sent).  Arms:
  tx16  frames from bf16                 tx2   x.float() into fp32, then the fp32 tx kernel
  tx32  the fp32 tx kernel alone, the same numel
  rx16  frames into bf16                 rx2   the fp32 rx kernels, then .to(bf16)
  rx32  the fp32 rx kernels alone
Exit status 1 when a fused arm's median is not below its two-step arm's by
more than the two arms' min-max ranges.
Usage: bench_half_frames.py [OUT.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p4app-switchml_amd")]

import torch  # noqa: E402
import switchml_amd as sw  # noqa: E402


def main(N=64 << 20, nbuf=4, rounds=7, reps=20, P=256, W=1, bm=64):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    B = sw.num_blocks(N, P)
    F = B + min(B, bm)
    stride = sw.frame_bytes(P)
    bf, f32 = torch.bfloat16, torch.float32
    prm = sw.frame_params(job_id=5, max_outstanding_pkts=bm)
    xb = [torch.randn(N, device=dev, generator=g).mul_(0.01).to(bf) for _ in range(nbuf)]   # gradient-like
    wide = [torch.empty(N, dtype=f32, device=dev) for _ in range(nbuf)]
    frs = [torch.empty(F * stride, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    ob = [torch.empty(N, dtype=bf, device=dev) for _ in range(nbuf)]
    rx16 = [sw.RxSlice(N, P, bm, device=dev, out=ob[k]) for k in range(nbuf)]
    rx32 = [sw.RxSlice(N, P, bm, device=dev, out=wide[k]) for k in range(nbuf)]
    st = torch.cuda.current_stream()

    def tx(x, k):
        sw.quantize_pack_frames(x, prm, P, W, batch_max=bm, frames=frs[k], stride=stride, stream=st)

    def rx(r, k):
        r.reset(st)
        sw.dequantize_frames(frs[k], F, r, num_workers=W, job_id=5, stride=stride, stream=st)

    def arm_tx16(k): tx(xb[k], k)
    def arm_tx2(k): wide[k].copy_(xb[k]); tx(wide[k], k)
    def arm_tx32(k): tx(wide[k], k)
    def arm_rx16(k): rx(rx16[k], k)
    def arm_rx2(k): rx(rx32[k], k); ob[k].copy_(wide[k])
    def arm_rx32(k): rx(rx32[k], k)

    # ---- every fused arm's bytes equal its two-step arm's ---------------
    frs[0].fill_(0xAB)
    arm_tx16(0)
    torch.cuda.synchronize()
    f16 = frs[0].clone()
    frs[0].fill_(0xCD)
    arm_tx2(0)
    torch.cuda.synchronize()
    assert torch.equal(f16, frs[0]), "tx16 != tx2"
    ob[0].fill_(7.0)
    arm_rx16(0)
    torch.cuda.synchronize()
    o16, e16, c16 = ob[0].clone(), rx16[0].exps.clone(), rx16[0].counts.clone()
    ob[0].fill_(9.0)
    arm_rx2(0)
    torch.cuda.synchronize()
    assert torch.equal(o16.view(torch.int16), ob[0].view(torch.int16)), "rx16 != rx2"
    assert torch.equal(e16, rx32[0].exps) and torch.equal(c16, rx32[0].counts) and c16.tolist() == [F, 0]
    for k in range(nbuf):                               # the frame sets every rx arm reads; tx32's inputs
        wide[k].copy_(xb[k])
        tx(xb[k], k)

    arms = {"tx16": arm_tx16, "tx2": arm_tx2, "tx32": arm_tx32, "rx16": arm_rx16, "rx2": arm_rx2, "rx32": arm_rx32}
    times = {name: [] for name in arms}
    step = [0]
    for _ in range(40):
        arm_tx16(step[0] % nbuf)
        step[0] += 1
    for _ in range(rounds):
        for name, fn in arms.items():
            if name == "tx32":                          # rx2 / rx32 of the round before wrote `wide`
                for k in range(nbuf):
                    wide[k].copy_(xb[k])
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
    res = {name: {"median_us": round(us[name], 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    # algorithmic bytes: the typed buffer once, the frames once (rx: headers
    # of every frame in the claim pass, payloads in the apply pass), the state
    wire = F * stride
    alg = {"tx16": 2 * N + wire, "tx32": 4 * N + wire, "rx16": 2 * N + wire, "rx32": 4 * N + wire}
    for name, nbytes in alg.items():
        res[name]["TBps_algorithmic"] = round(nbytes / us[name] / 1e6, 3)
    ok = True
    cmp = {}
    for fused, two, fp32 in (("tx16", "tx2", "tx32"), ("rx16", "rx2", "rx32")):
        spread = (max(times[fused]) - min(times[fused])) + (max(times[two]) - min(times[two]))
        faster = us[two] - us[fused] > spread
        cmp[fused] = {"two_step_arm": two, "speedup_over_two_step": round(us[two] / us[fused], 3),
                      "median_gap_us": round(us[two] - us[fused], 2), "min_max_ranges_us": round(spread, 2),
                      "fp32_arm": fp32, "time_over_fp32_kernel": round(us[fused] / us[fp32], 3),
                      "byte_ratio": round(alg[fused] / alg[fp32], 3), "faster_than_two_step_beyond_ranges": faster}
        ok = ok and faster
    out = {"what": f"side measurement (not bench.py's headline): bf16 slices over DPDK frames, {N >> 20} Mi elements, "
                   f"P={P}, W={W}, batch_max={bm}, {nbuf} cycled input / frame / output sets (cold), {rounds} "
                   f"interleaved rounds x {reps} launches, medians with the rounds' min-max, HIP events; an rx call "
                   "is sml_rx_reset + claim + apply",
           "device": torch.cuda.get_device_name(0), "arms": res, "compare": cmp, "all_fused_arms_faster": ok}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
