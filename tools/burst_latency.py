#!/usr/bin/env python3
"""Per-burst latency of the per-packet paths: one burst
launch + stream sync against one sml_burst_server_submit, for 1, 16 and 64
packets, packets in HBM and in pinned host memory.  --op exchange (the
default): each burst is a full exchange (post of q, pre of q + b into the
same buffer, FLAG_PROCESS_PACKET) over a fixed set of slots; --op pre / post:
sml_preprocess_burst / sml_postprocess_burst of the same packets.  Median of
`reps` bursts after a warm-up.  --dtype fp16 / bf16: the slice and the output
are 16-bit (the typed entry points convert); the burst server
takes no 16-bit slice, so only the launch arm runs.

Usage: python tools/burst_latency.py [--op pre|post|exchange] [--dtype fp32|fp16|bf16] [OUT.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "p4app-switchml_amd"))


def measure(op="exchange", reps=400, warmup=50, echo=True, dtype="fp32"):
    import numpy as np
    import torch
    import switchml_amd as sw
    dev = torch.device("cuda", 0)
    P, W, b = 256, 2, 64
    n = 4096 * P                         # B = 4096 blocks, far more than the bursts touch
    tdtype = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    x = torch.randn(n, device=dev).to(tdtype)
    out = torch.zeros(n, dtype=tdtype, device=dev)
    recv = torch.zeros(n // P, dtype=torch.int8, device=dev)
    launch, server_op, flags = {"pre": (sw.preprocess_burst, sw.BURST_PRE, 0),
                                "post": (sw.postprocess_burst, sw.BURST_POST, 0),
                                "exchange": (sw.exchange_burst, sw.BURST_EXCHANGE, sw.FLAG_PROCESS_PACKET)}[op]
    res = {}
    stream = torch.cuda.current_stream(dev)
    for place in ("device", "pinned"):
        if place == "device":
            ring = torch.zeros(b * P, dtype=torch.int32, device=dev)
            ex = torch.zeros(b * 2, dtype=torch.uint8, device=dev)
        else:
            ring = torch.zeros(b * P, dtype=torch.int32).pin_memory()
            ex = torch.zeros(b * 2, dtype=torch.uint8).pin_memory()
        for count in (1, 16, 64):
            ids = list(range(b, b + count))          # packets q >= b: payload and exponent halves both run
            bt = sw.packet_burst(x, out, P, W, b, recv, ids, [ring.data_ptr() + (q % b) * P * 4 for q in ids],
                                 [ex.data_ptr() + (q % b) * 2 for q in ids], flags=flags)
            for name in ("launch", "server") if dtype == "fp32" else ("launch",):
                srv = sw.BurstServer(P) if name == "server" else None

                def one():
                    if srv is None:
                        launch(bt, stream)
                        stream.synchronize()
                    else:
                        srv.submit(server_op, bt)
                for _ in range(warmup):
                    one()
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    one()
                    ts.append(time.perf_counter() - t0)
                if srv is not None:
                    srv.close()
                res[f"{place}_{count}pkt_{name}_us"] = round(float(np.median(ts)) * 1e6, 2)
                if echo:
                    print(place, count, name, res[f"{place}_{count}pkt_{name}_us"], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--op", choices=("pre", "post", "exchange"), default="exchange")
    ap.add_argument("--dtype", choices=("fp32", "fp16", "bf16"), default="fp32")
    ap.add_argument("out", nargs="?", help="write the JSON result here as well")
    args = ap.parse_args()
    s = json.dumps(measure(args.op, dtype=args.dtype), indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
