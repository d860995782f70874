"""Step cost of the quantised fine-tune (Fitter.run_quantised) against the plain step (Fitter.run) on the benchmark shape: a 4x256
SIREN, 100 000 samples per step.

    python tools/quantize_step_cost.py                      # alternating rounds of both, host clock around a device synchronise
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o quant -- python tools/quantize_step_cost.py --profile
                                                            # 200 quantised steps for the kernels' own times

The quantised step is five enqueue-only calls from a Python loop (ranges, apply, repack, train step, optimizer); the plain phase is
one C-ABI call for the whole run.  The last line times the plain step driven one call per step (Fitter.step), which separates what
the host loop costs from what the extra kernels cost.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brief_pytorch_amd.fit import Fitter           # noqa: E402
from brief_pytorch_amd.networks import SIREN       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--bits", type=int, default=12)
    ap.add_argument("--steps", type=int, default=500, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--profile", action="store_true", help="warm up, run 200 quantised steps and exit (for a kernel trace)")
    a = ap.parse_args()
    dims = (128, 128, 128)
    torch.manual_seed(0)
    tv = (torch.rand(dims[0] * dims[1] * dims[2], 1) * 100.0).cuda()

    def make():
        torch.manual_seed(0)
        m = SIREN(coords_channel=3, data_channel=1, features=a.features, layers=a.layers, w0=20).to("cuda")
        return Fitter(m, tv, dims, sampler="randompoint", sample_size=100000, seed=42)
    plain, quant = make(), make()
    plain.run(50)
    quant.run_quantised(50, a.bits)
    torch.cuda.synchronize()
    if a.profile:
        quant.run_quantised(200, a.bits)
        torch.cuda.synchronize()
        print("profiled 200 quantised steps")
        return
    res = {"plain": [], "quantised": []}
    for _ in range(a.rounds):
        for name, f in (("plain", plain), ("quantised", quant)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "plain":
                f.run(a.steps)
            else:
                f.run_quantised(a.steps, a.bits)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    for k, v in res.items():
        print("%s ms/step per round: %s  median %.4f" % (k, " ".join("%.4f" % x for x in v), statistics.median(v)))
    print("ratio quantised / plain (medians): %.4f" % (statistics.median(res["quantised"]) / statistics.median(res["plain"])))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        plain.step()
    torch.cuda.synchronize()
    print("plain, one C-ABI call per step (Fitter.step): %.4f ms/step" % ((time.perf_counter() - t0) / a.steps * 1e3))


if __name__ == "__main__":
    main()
