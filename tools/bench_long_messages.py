#!/usr/bin/env python3
"""Long RDMA messages (sml_msg_*) against the packet kernels at P = 1024, whose
bytes per element they share (8 B/element plus one exponent byte per message).
A SIDE measurement: bench.py and its headline do not change.

fp32, 64 Mi elements (256 MiB), W = 1, cold HBM: the steps cycle 4 distinct
buckets with their planes (past the 256 MiB Infinity Cache).  Interleaved
rounds, HIP events, medians.  Arms, per msg_numel M: k1 = sml_msg_quantize_pack
(fused), k4 = sml_msg_dequantize, rt = sml_msg_roundtrip_loopback out of place.
Baselines in the same run on the same buffers: sml_quantize_pack,
sml_dequantize and sml_roundtrip_loopback at P = 1024, and sml_stream_copy of
the same bytes.  Each row gives its time over the baseline's; the baseline's
own spread over the rounds, (max - min) / median, says what a difference means.
Before anything is timed, at the timed size: M = 1024 through the new entry
points equals the packet kernels bit for bit, and for every M the fused round
trip equals K1 then K4.
The batched round trip (sml_msg_roundtrip_loopback_batch), per M of BATCH_MS: 64
fp32 slices that together cover the stream, in one call (batch), against the
same 64 slices as 64 sml_msg_roundtrip_loopback launches (loop) and against
rt_M, one launch over the whole stream (the floor); the three share buffers and
rounds.  The tables and the per-slice arguments are built before the timing, so
an arm's host side is its C calls.  Before the timing: batch equals loop bit
for bit.
Usage: bench_long_messages.py [OUT.json]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p4app-switchml_amd")]

import torch  # noqa: E402
import switchml_amd as sw  # noqa: E402

MS = (1024, 2048, 2304, 4096, 16384, 768)
BATCH_MS = (2304, 4096, 16384)
NSLICES = 64


def main(N=64 << 20, nbuf=4, rounds=9, reps=20, W=1):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    xs = [torch.randn(N, device=dev, generator=g).mul_(0.01) for _ in range(nbuf)]
    outs = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(nbuf)]
    words = max(-(-N // M) * M for M in MS)
    pls = [torch.empty(words, dtype=torch.int32, device=dev) for _ in range(nbuf)]
    exs = [torch.empty(-(-N // min(MS)), dtype=torch.int8, device=dev) for _ in range(nbuf)]
    st = torch.cuda.current_stream()

    def views(M, k):
        B = -(-N // M)
        return pls[k][:B * M], exs[k][:B]

    def msg_arms(M):
        def k1(k):
            p, e = views(M, k)
            sw.msg_quantize_pack(xs[k], M, W, payload=p, exps_out=e, stream=st)

        def k4(k):
            p, e = views(M, k)
            sw.msg_dequantize(p, e, N, M, W, out=outs[k], stream=st)

        def rt(k):
            sw.msg_roundtrip_loopback(xs[k], M, W, out=outs[k], stream=st)
        return {f"k1_M{M}": k1, f"k4_M{M}": k4, f"rt_M{M}": rt}

    # the stream cut into NSLICES slices at multiples of 64 elements (no multiple of any M of BATCH_MS)
    cuts = [N * i // NSLICES // 64 * 64 + (64 if 0 < i < NSLICES else 0) for i in range(NSLICES + 1)]
    tables = [sw.planes.typed_slice_table([(xs[k][a:b], outs[k][a:b]) for a, b in zip(cuts, cuts[1:])], st)[0]
              for k in range(nbuf)]
    L, sp = sw.abi.lib(), ctypes.c_void_p(st.cuda_stream)

    def batch_arms(M):
        def batch(k):
            sw.abi.call("sml_msg_roundtrip_loopback_batch", tables[k], NSLICES, M, W, 0, sp)

        def loop(k):
            for s in tables[k]:
                L.sml_msg_roundtrip_loopback(s.in_, s.out, sw.abi.FLOAT32, s.numel, M, W, None, None, 0, sp)
        return {f"batch_M{M}": batch, f"loop_M{M}": loop}

    def base_k1(k):
        p, e = views(1024, k)
        sw.quantize_pack(xs[k], 1024, W, payload=p, exps_out=e, stream=st)

    def base_k4(k):
        p, e = views(1024, k)
        sw.dequantize(p, e, N, 1024, W, out=outs[k], stream=st)

    def base_rt(k): sw.roundtrip_loopback(xs[k], 1024, W, out=outs[k], stream=st)
    def copy(k): sw.stream_copy(xs[k], outs[k], stream=st)

    # ---- results at the timed size, before any timing -------------------
    base_k1(0)
    want = [t.clone() for t in views(1024, 0)]
    base_k4(0)
    want_out = outs[0].clone()
    for M in MS:
        arms = msg_arms(M)
        arms[f"k1_M{M}"](0)
        got = [t.clone() for t in views(M, 0)]
        arms[f"k4_M{M}"](0)
        chain = outs[0].clone()
        arms[f"rt_M{M}"](0)
        torch.cuda.synchronize()
        assert torch.equal(chain.view(torch.int32), outs[0].view(torch.int32)), f"M={M}: round trip != K1 then K4"
        if M == 1024:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "M=1024 != the packet kernels"
            assert torch.equal(chain.view(torch.int32), want_out.view(torch.int32)), "M=1024 K4 != the packet K4"

    for M in BATCH_MS:
        b = batch_arms(M)
        b[f"loop_M{M}"](0)
        want_out = outs[0].clone()
        b[f"batch_M{M}"](0)
        torch.cuda.synchronize()
        assert torch.equal(want_out.view(torch.int32), outs[0].view(torch.int32)), f"M={M}: batch != per-slice launches"

    arms = {"base_k1": base_k1, "base_k4": base_k4, "base_rt": base_rt, "copy": copy}
    for M in MS:
        arms.update(msg_arms(M))
    for M in BATCH_MS:
        arms.update(batch_arms(M))
    for k in range(nbuf):                         # planes for the K4 arms, whichever arm ran last
        base_k1(k)
    times = {name: [] for name in arms}
    step = 0
    for _ in range(rounds + 1):                   # the first round warms every arm up and is dropped
        for name, fn in arms.items():
            if name.startswith("k4_M"):           # K4 reads planes cut at its own M
                for k in range(nbuf):
                    arms["k1" + name[2:]](k)
            for _ in range(4):
                fn(step % nbuf)
                step += 1
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(reps):
                fn(step % nbuf)
                step += 1
            b.record(st)
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / reps * 1e3)
    times = {name: v[1:] for name, v in times.items()}

    med = {name: statistics.median(v) for name, v in times.items()}
    spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
    res = {name: {"median_us": round(med[name], 2), "spread": round(spread[name], 4),
                  "TBps_algorithmic": round(8 * N / med[name] / 1e6, 3)} for name in arms}
    rows = {}
    for M in MS:
        rows[str(M)] = {k: {"time_over_P1024": round(med[f"{k}_M{M}"] / med[f"base_{k}"], 4),
                            "baseline_spread": round(spread[f"base_{k}"], 4),
                            "time_over_stream_copy": round(med[f"{k}_M{M}"] / med["copy"], 4)} for k in ("k1", "k4", "rt")}
    # batch and loop over the floor rt_M, whose own spread over the rounds says what a difference means
    batch_rows = {str(M): {"batch_us": res[f"batch_M{M}"]["median_us"], "loop_us": res[f"loop_M{M}"]["median_us"],
                           "one_launch_us": res[f"rt_M{M}"]["median_us"],
                           "batch_over_loop": round(med[f"batch_M{M}"] / med[f"loop_M{M}"], 4),
                           "batch_over_one_launch": round(med[f"batch_M{M}"] / med[f"rt_M{M}"], 4),
                           "batch_spread": round(spread[f"batch_M{M}"], 4),
                           "loop_spread": round(spread[f"loop_M{M}"], 4),
                           "one_launch_spread": round(spread[f"rt_M{M}"], 4)} for M in BATCH_MS}
    out = {"what": f"side measurement (not bench.py's headline): long RDMA messages, fp32, {N >> 20} Mi elements, "
                   f"W={W}, {nbuf} cycled buckets (cold), {rounds} interleaved rounds x {reps} launches after one "
                   "dropped round, medians, HIP events; spread = (max - min) / median over the rounds",
           "device": torch.cuda.get_device_name(0), "arms": res, "rows_by_msg_numel": rows,
           "batch_of_64_slices_by_msg_numel": batch_rows}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
