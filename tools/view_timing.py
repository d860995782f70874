"""Times the view decode on one MI355X and writes profiles/r16_view.md:

    python tools/view_timing.py [--edge 256] [--reps 5] [--out profiles/r16_view.md]

An edge^3 uint16 grid behind a 4x256 and a 4x22 fp32 SIREN (random init: the time does not depend on the weights).  Per net, interleaved
on one device in every repetition:
    (a)  view.render of the axis-aligned max view along z      against      mip.decode_mips of the same region (the projection decode,
         whose code this feature does not touch): the same voxels evaluated, through explicit coordinates here and in-kernel ones there;
    (b)  an oblique max view, the direction turned 45 degrees about z out of the x axis (a frame of a rotating MIP);
    (c)  an oblique slice through the centre, normal (1, 1, 1).
Host clock around each call, which ends in the device synchronise of its statistics (render) or in an explicit one (decode_mips); every
shape is warmed once; median and spread of the repetitions.  The images of (a) are compared before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from brief_pytorch_amd import mip, view      # noqa: E402
from brief_pytorch_amd.networks import SIREN      # noqa: E402

NETS = ((5, 256), (5, 22))
EPI = dict(scale=(-0.5, 0.5), vrange=(3.0, 60000.0))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_view.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_timing.py measures on a ROCm GPU; there is none here")
    dims = [args.edge] * 3
    full = ([0, 0, 0], dims, [1, 1, 1])
    views = {"a": view.make_view(dims, (1, 0, 0)),
             "b": view.make_view(dims, (0, np.sin(np.pi / 4), np.cos(np.pi / 4)), up=(1, 0, 0)),
             "c": view.make_view(dims, (1, 1, 1), depth=0.0)}
    rows = []
    for layers, feats in NETS:
        torch.manual_seed(0)
        m = SIREN(coords_channel=3, data_channel=1, features=feats, layers=layers, w0=20).to("cuda")
        calls = {
            "mip": lambda: mip.decode_mips(m, dims, *full, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"]),
            "a": lambda: view.render(m, views["a"], "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"]),
            "b": lambda: view.render(m, views["b"], "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"]),
            "c": lambda: view.render(m, views["c"], "slice", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"]),
        }
        first = {k: timed(f)[1] for k, f in calls.items()}      # warm every shape; and the results that must agree
        assert np.array_equal(first["a"][0].cpu().numpy(), first["mip"][0].cpu().numpy()), "the axis-aligned max view differs from the projection decode"
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                ms[k].append(timed(f)[0])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
        stats = {k: first[k][2] for k in "abc"}
        rows.append((layers, feats, med, spread, stats))
        print("%dx%d: " % (layers - 1, feats) + ", ".join("%s %.2f ms" % (k, med[k]) for k in calls) + ", ratio (a) %.3f" % (med["a"] / med["mip"]))
    with open(args.out, "w") as f:
        f.write("# View decode: times on one MI355X\n\n`python tools/view_timing.py --edge %d --reps %d`; %d^3 uint16 grid, fp32 SIREN, random "
                "init.  Host clock around a call that ends in a device synchronise; every shape warmed once; median (min .. max) of %d "
                "repetitions, the four calls interleaved in every repetition.\n\n" % (args.edge, args.reps, args.edge, args.reps))
        f.write("| net | `mip.decode_mips`, whole grid (ms) | (a) axis-aligned max view (ms) | ratio (a) / mip | (b) oblique 45 degree max view (ms) | (c) oblique slice (ms) |\n|---|---|---|---|---|---|\n")
        cell = lambda med, spread, k: "%.2f (%.2f .. %.2f)" % (med[k], spread[k][0], spread[k][1])
        for layers, feats, med, spread, stats in rows:
            f.write("| %dx%d | %s | %s | %.3f | %s | %s |\n" % (layers - 1, feats, cell(med, spread, "mip"), cell(med, spread, "a"), med["a"] / med["mip"],
                                                             cell(med, spread, "b"), cell(med, spread, "c")))
        f.write("\nSamples evaluated: " + "; ".join("(%s) %d of %d rays hit, %d samples" % (k, rows[0][4][k]["rays_hit"], rows[0][4][k]["rays"],
                                                                                         rows[0][4][k]["samples_evaluated"]) for k in "abc") + ".\n")
        f.write("\n(a) evaluates exactly the voxels the projection decode evaluates, so the ratio is the price of the explicit coordinates "
                "(12 B written and read per sample), of the ray clip and of folding one image instead of three.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
