"""Times the surface view on one MI355X and writes profiles/r17_surface.md:

    python tools/surface_timing.py [--edge 256] [--reps 5] [--parent <checkout of the parent commit, library built>] [--out profiles/r17_surface.md]

An edge^3 uint16 grid behind a 4x256 and a 4x22 fp32 SIREN (random init: the time does not depend on the weights), seen along a
direction turned 45 degrees about z out of the x axis (view_timing.py's rotating-MIP frame).  The level is the median over the rays of
the max view's image, so about half the rays hit.  Per net, interleaved on one device in every repetition:
    max       view.render(..., "max") of that geometry: what the march alone costs;
    first     view.render_surface, refine=0, no shading: the first-hit fold instead of the max fold;
    refine8   refine=8, no shading: plus eight dense rounds;
    shaded    refine=8 with normals and shade: plus one Jacobian pass over rows x cols points;
    shaded0   refine=0 with normals and shade.
With --parent the max view is ALSO timed by the parent commit's own code and library, in a child process on the same device (its
median is a run of its own, not interleaved with the others).  Host clock around each call, which ends in the device synchronise of
its statistics; every shape is warmed once; median and spread of the repetitions."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ((5, 256), (5, 22))
EPI = dict(scale=(-0.5, 0.5), vrange=(3.0, 60000.0))
DIRECTION = (0.0, float(np.sin(np.pi / 4)), float(np.cos(np.pi / 4)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def make(layers, feats):
    from brief_pytorch_amd.networks import SIREN
    torch.manual_seed(0)
    return SIREN(coords_channel=3, data_channel=1, features=feats, layers=layers, w0=20).to("cuda")


def max_only(edge, reps):
    """the max view alone, by whatever package sys.path finds first: {"LxF": [ms, ...]} as one JSON line (the --parent child)"""
    from brief_pytorch_amd import view
    v = view.make_view([edge] * 3, DIRECTION, up=(1, 0, 0))
    out = {}
    for layers, feats in NETS:
        m = make(layers, feats)
        call = lambda: view.render(m, v, "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
        timed(call)
        out["%dx%d" % (layers - 1, feats)] = [timed(call)[0] for _ in range(reps)]
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its view.render is timed too")
    ap.add_argument("--max-only", default=None, metavar="ROOT", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_surface.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_timing.py measures on a ROCm GPU; there is none here")
    sys.path.insert(0, args.max_only or ROOT)
    if args.max_only:
        return max_only(args.edge, args.reps)
    from brief_pytorch_amd import view
    parent = None
    if args.parent:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--edge", str(args.edge), "--reps", str(args.reps), "--max-only",
                            os.path.abspath(args.parent)], capture_output=True, text=True, cwd=os.path.abspath(args.parent))
        if r.returncode != 0:
            raise SystemExit("the parent's run failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    dims = [args.edge] * 3
    v = view.make_view(dims, DIRECTION, up=(1, 0, 0))
    rows = []
    for layers, feats in NETS:
        m = make(layers, feats)
        render = lambda: view.render(m, v, "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
        img, hits, _ = render()
        level = int(np.median(img.cpu().numpy()[..., 0][hits.cpu().numpy() > 0]))
        surf = lambda **kw: (lambda: view.render_surface(m, v, level, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"], **kw))
        calls = {"max": render, "first": surf(refine=0, shading=False), "refine8": surf(refine=8, shading=False),
                 "shaded": surf(refine=8, shading=True), "shaded0": surf(refine=0, shading=True)}
        first = {k: timed(f)[1] for k, f in calls.items()}      # warm every shape
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                ms[k].append(timed(f)[0])
        name = "%dx%d" % (layers - 1, feats)
        if parent is not None:
            ms["parent"] = parent[name]
        med = {k: float(np.median(x)) for k, x in ms.items()}
        spread = {k: (float(np.min(x)), float(np.max(x))) for k, x in ms.items()}
        rows.append((name, med, spread, first["shaded"]["stats"], level))
        print(name + ": " + ", ".join("%s %.2f ms" % (k, med[k]) for k in med))
    keys = ["max", "first", "refine8", "shaded", "shaded0"]
    heads = {"parent": "`view.render` max, parent commit (ms)", "max": "`view.render` max (ms)", "first": "surface, refine 0, no shading (ms)",
             "refine8": "surface, refine 8, no shading (ms)", "shaded": "surface, refine 8, shaded (ms)", "shaded0": "surface, refine 0, shaded (ms)"}
    if parent is not None:
        keys = ["parent"] + keys
    base = "parent" if parent is not None else "max"
    with open(args.out, "w") as f:
        f.write("# Surface view: times on one MI355X\n\n`python tools/surface_timing.py --edge %d --reps %d%s`; %d^3 uint16 grid, fp32 SIREN, random "
                "init, an orthographic view turned 45 degrees about z (%d x %d rays of %d samples).  Host clock around a call that ends in a "
                "device synchronise; every shape warmed once; median (min .. max) of %d repetitions, the calls of this tree interleaved in "
                "every repetition%s.\n\n" % (args.edge, args.reps, " --parent <parent checkout>" if parent is not None else "", args.edge, v.rows, v.cols,
                                            v.depth, args.reps, "; the parent commit's max view in a process of its own on the same device"
                                            if parent is not None else ""))
        f.write("| net | " + " | ".join(heads[k] for k in keys) + " | refine 0 / %s | refine 8 / %s | shaded / %s |\n" % (base, base, base))
        f.write("|---" * (len(keys) + 4) + "|\n")
        for name, med, spread, stats, level in rows:
            f.write("| %s | " % name + " | ".join("%.2f (%.2f .. %.2f)" % (med[k], spread[k][0], spread[k][1]) for k in keys)
                    + " | %.3f | %.3f | %.3f |\n" % (med["first"] / med[base], med["refine8"] / med[base], med["shaded"] / med[base]))
        for name, med, spread, stats, level in rows:
            f.write("\n%s: level %d; %d of %d rays meet the grid, %d hit the surface (%d cut), %d samples marched, %d refinement points "
                    "(%.4f of the march).\n" % (name, level, stats["rays_hit"], stats["rays"], stats["rays_surface"], stats["rays_cut"],
                                                 stats["samples_evaluated"], stats["refine_points"],
                                                 stats["refine_points"] / max(stats["samples_evaluated"], 1)))
        f.write("\nExpected from the code: the march costs what the max view costs; refinement adds (refine + 1) / depth of it (the rounds "
                "and the final coordinates), shading one Jacobian pass over rows x cols points.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
