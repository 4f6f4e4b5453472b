#!/usr/bin/env python3
"""Host cost of one Python/ctypes launch of sml_quantize_pack (tiny input,
1000 launches, no sync inside the loop): shows the bench's eager launch path
cannot starve the GPU (8.5 us per launch on the MI355X box vs a 75 us kernel).

  launch_cost.py [--repeat N] [--package DIR] [OUT.json]

N runs of the loop (default 5); one JSON line with every run, the median and
the min-max in us per launch, also written to OUT.json.  --package: the
directory holding the switchml_amd package to time (default: this tree's)."""
import argparse, json, statistics
import sys, time, os
ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--package", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "p4app-switchml_amd"))
ap.add_argument("out", nargs="?")
opt = ap.parse_args()
sys.path.insert(0, opt.package)
import torch, switchml_amd as sw
dev = torch.device("cuda:0")
x = torch.randn(4096, device=dev)
B = sw.num_blocks(4096, 256)
p = torch.empty(B*256, dtype=torch.int32, device=dev); e = torch.empty(B, dtype=torch.int8, device=dev)
st = torch.cuda.current_stream()
for _ in range(100): sw.quantize_pack(x, 256, 1, payload=p, exps_out=e, stream=st)
runs = []
for _ in range(opt.repeat):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(1000): sw.quantize_pack(x, 256, 1, payload=p, exps_out=e, stream=torch.cuda.current_stream())
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    runs.append(round((t1 - t0) / 1000 * 1e6, 3))
res = {"metric": "host us per python launch of sw.quantize_pack (4096 elements, 1000 launches per run)",
       "package": os.path.relpath(os.path.dirname(os.path.abspath(sw.__file__))), "runs_us": runs,
       "median_us": statistics.median(runs), "min_us": min(runs), "max_us": max(runs)}
print(json.dumps(res))
if opt.out:
    with open(opt.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
