"""Region decode against the whole-grid decode (SIREN.decode_box vs SIREN.decode_grid), timed with device events in one process:
every call warmed up once, then the calls alternate (full, 1/8, 1/64, 1/512, ... of the volume) for --reps rounds; median per call.
Random-init nets (the time does not depend on the weights), u16 output with the fused epilogue as NFGR.decompress runs it.

    python tools/region_timing.py [--reps 3] [--configs 5x256@512,5x1494@1024] [--json out.json]

Boxes are centred cubes of edge dims / k (k = 2, 4, 8, 16, 32: 1/8 ... 1/32768 of the volume)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brief_pytorch_amd.networks import SIREN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="5x256@512,5x1494@1024", help="layersxfeatures@edge, comma-separated")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    kw = dict(out_kind="u16", scale=(0.0, 100.0), vrange=(0.0, 65535.0))
    rows = []
    for spec in args.configs.split(","):
        net, edge = spec.split("@")
        L, F = (int(v) for v in net.split("x"))
        edge = int(edge)
        dims = (edge, edge, edge)
        torch.manual_seed(0)
        m = SIREN(features=F, layers=L, w0=20).to("cuda")
        full_out = torch.empty((edge ** 3, 1), dtype=torch.uint16, device="cuda")
        calls = [("full", 1, lambda: m.decode_grid(dims, out=full_out, **kw))]
        for k in (2, 4, 8, 16, 32):
            e = edge // k
            b = (edge - e) // 2
            out = torch.empty((e, e, e, 1), dtype=torch.uint16, device="cuda")
            calls.append(("1/%d" % k ** 3, k ** 3, (lambda b=b, e=e, out=out: m.decode_box(dims, b, b + e, 1, out=out, **kw))))
        for _, _, fn in calls:      # warm: kernels loaded, scratch allocated, clocks up
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in calls}
        for _ in range(args.reps):
            for name, _, fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        full_ms = float(np.median(times["full"]))
        for name, frac, _ in calls:
            ms = float(np.median(times[name]))
            vox = edge ** 3 // frac
            r = {"net": "%dx%d" % (L - 1, F), "dims": list(dims), "box": name, "voxels": vox, "ms": ms, "ms_min": float(np.min(times[name])),
                 "ms_max": float(np.max(times[name])), "mvox_per_s": vox / ms / 1e3, "time_vs_full": ms / full_ms, "voxels_vs_full": 1.0 / frac}
            rows.append(r)
            print("%-8s %-16s box %-8s %12d voxels  %10.3f ms (%.3f .. %.3f)  %8.1f Mvox/s  time/full %.5f  voxels/full %.5f" % (
                r["net"], "x".join(map(str, dims)), name, vox, ms, r["ms_min"], r["ms_max"], r["mvox_per_s"], r["time_vs_full"], r["voxels_vs_full"]),
                flush=True)
        del m, full_out, calls
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"reps": args.reps, "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
