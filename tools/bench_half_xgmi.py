#!/usr/bin/env python3
"""The in-node switch's multicast of a 16-bit slice: sml_copy_segments_typed
(2-byte elements, any 2-byte alignment) against sml_copy_segments on the same
element counts as fp32.  A SIDE measurement: bench.py and its headline do not
change.

One process, one GPU: every segment is local HBM, so this shows the kernel's
cost at odd alignment and its time against half the bytes — nothing about
xGMI (peers' planes, link rates, pull against push), which one GPU cannot show.

8 segments x 2 Mi elements, bf16, cold HBM: the steps cycle 4 distinct source
/ destination sets (past the 256 MiB Infinity Cache for the fp32 arm; the
16-bit arms move half the bytes per set).  Interleaved rounds, medians with
the rounds' min-max, HIP events.  Every arm's bytes are checked before
anything is timed.  Arms:
  A  sml_copy_segments_typed, bf16, destinations at element offset 1
  B  the same, destinations at element offset 0
  C  sml_copy_segments, the same element counts as fp32
  D  arm A through another build of the library (--other-lib PATH: the other
     vector width of the 16-bit kernel, a scratch build), when given
Usage: bench_half_xgmi.py [--other-lib PATH] [OUT.json]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p4app-switchml_amd")]

import torch  # noqa: E402
import switchml_amd as sw  # noqa: E402


def main(argv, nseg=8, n=2 << 20, nbuf=4, rounds=7, reps=20):
    other, out_path = None, None
    args = list(argv)
    if "--other-lib" in args:
        i = args.index("--other-lib")
        other = ctypes.CDLL(args[i + 1])
        del args[i:i + 2]
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        other.sml_copy_segments_typed.restype = ctypes.c_int
        other.sml_copy_segments_typed.argtypes = [vp, vp, vp, u32, ctypes.c_int, u32, vp]
    if args:
        out_path = args[0]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bf, i32 = torch.bfloat16, torch.int32
    pad = 64                                               # elements between segments: room for the offset
    # one buffer per set and side; segment s starts at s * (n + pad) (+ the offset)
    src16 = [torch.randn(nseg * (n + pad), device=dev, generator=g).to(bf) for _ in range(nbuf)]
    dst16 = [torch.zeros(nseg * (n + pad), dtype=bf, device=dev) for _ in range(nbuf)]
    src32 = [torch.randint(-2 ** 31, 2 ** 31 - 1, (nseg * (n + pad),), dtype=i32, device=dev, generator=g)
             for _ in range(nbuf)]
    dst32 = [torch.zeros(nseg * (n + pad), dtype=i32, device=dev) for _ in range(nbuf)]
    st = torch.cuda.current_stream()

    def pairs(src, dst, off):
        return [(src[s * (n + pad):s * (n + pad) + n], dst[s * (n + pad) + off:s * (n + pad) + off + n])
                for s in range(nseg)]

    pa = [pairs(src16[k], dst16[k], 1) for k in range(nbuf)]
    pb = [pairs(src16[k], dst16[k], 0) for k in range(nbuf)]
    pc = [pairs(src32[k], dst32[k], 0) for k in range(nbuf)]

    def tables(ps):
        s = (ctypes.c_void_p * nseg)(*[a.data_ptr() for a, _ in ps])
        d = (ctypes.c_void_p * nseg)(*[b.data_ptr() for _, b in ps])
        c = (ctypes.c_uint64 * nseg)(*[a.numel() for a, _ in ps])
        return s, d, c

    # every call's arguments are built before the loop and every arm calls
    # the C entry point itself: at 15-25 us per launch the Python wrappers'
    # table building would be what is timed
    ta, tb, tc = ([tables(p[k]) for k in range(nbuf)] for p in (pa, pb, pc))
    L, stp = sw.lib(), ctypes.c_void_p(st.cuda_stream)

    def typed(lib, t):
        s, d, c = t
        rc = lib.sml_copy_segments_typed(ctypes.cast(s, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p),
                                         ctypes.cast(c, ctypes.c_void_p), nseg, sw.BFLOAT16, 0, stp)
        assert rc == 0, rc

    def arm_a(k): typed(L, ta[k])
    def arm_b(k): typed(L, tb[k])

    def arm_c(k):
        s, d, c = tc[k]
        rc = L.sml_copy_segments(ctypes.cast(s, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p),
                                 ctypes.cast(c, ctypes.c_void_p), nseg, 0, stp)
        assert rc == 0, rc

    def arm_d(k): typed(other, ta[k])

    arms = {"A_bf16_dst_offset_1": arm_a, "B_bf16_dst_offset_0": arm_b, "C_fp32_words": arm_c}
    if other is not None:
        arms["D_bf16_dst_offset_1_other_width"] = arm_d

    # ---- every arm copies what it should --------------------------------
    for name, fn in arms.items():
        ps = pc[0] if name.startswith("C") else pb[0] if name.startswith("B") else pa[0]
        dst = dst32[0] if name.startswith("C") else dst16[0]
        dst.zero_()
        fn(0)
        torch.cuda.synchronize()
        for a, b in ps:
            assert torch.equal(a.view(torch.int16 if a.dtype == bf else i32),
                               b.view(torch.int16 if b.dtype == bf else i32)), name

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
    res = {}
    for name, v in times.items():
        nbytes = nseg * n * (4 if name.startswith("C") else 2) * 2          # read once, written once
        res[name] = {"median_us": round(us[name], 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                     "TBps_read_plus_write": round(nbytes / us[name] / 1e6, 3)}
    a, b, c = (us[k] for k in ("A_bf16_dst_offset_1", "B_bf16_dst_offset_0", "C_fp32_words"))
    cmp = {"A_over_C_time": round(a / c, 3), "byte_ratio": 0.5, "A_over_B_time": round(a / b, 3)}
    if other is not None:
        d = us["D_bf16_dst_offset_1_other_width"]
        va, vd = times["A_bf16_dst_offset_1"], times["D_bf16_dst_offset_1_other_width"]
        spread = (max(va) - min(va)) + (max(vd) - min(vd))
        cmp.update({"D_over_A_time": round(d / a, 3), "median_gap_A_minus_D_us": round(a - d, 2),
                    "min_max_ranges_us": round(spread, 2),
                    "other_width_faster_beyond_ranges": bool(a - d > spread)})
    out = {"what": f"side measurement (not bench.py's headline): the 16-bit multicast on ONE GPU (local HBM only, no "
                   f"xGMI): {nseg} segments x {n >> 20} Mi elements, bf16 against the same counts as fp32 words, "
                   f"{nbuf} cycled source / destination sets (cold), {rounds} interleaved rounds x {reps} launches, "
                   "medians with the rounds' min-max, HIP events; no pass mark",
           "device": torch.cuda.get_device_name(0), "arms": res, "compare": cmp}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
