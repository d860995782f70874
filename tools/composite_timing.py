"""Times the composite view on one MI355X and writes profiles/r20_composite.md:

    python tools/composite_timing.py [--edge 256] [--reps 7] [--parent <checkout of the parent commit, library built>] [--out profiles/r20_composite.md]

An edge^3 uint16 grid behind a 4x256 and a 4x22 fp32 SIREN (random init: the time does not depend on the weights), seen along a
direction turned 45 degrees about z out of the x axis (surface_timing.py's view).  The transfer function rises from nothing at the
first quartile of the max view's image to dense white at its maximum, so rays are clear, hazy and saturated.  Per net, interleaved on
one device in every repetition:
    max          view.render(..., "max") of that geometry: the march with the integer max fold;
    composite    composite.render_composite with the default 12-bit table (64 KiB);
    composite8   the same with an 8-bit table (4 KiB).
With --parent the max view is ALSO timed by the parent commit's own code and library, in a child process on the same device (its
median is a run of its own, not interleaved with the others).  Host clock around a window of calls that ends in a device synchronise
(every call ends in the synchronise of its statistics anyway); the window is sized at warm-up to last a quarter of a second or more;
every shape is warmed once; median and spread of the repetitions, in ms per call."""
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
WINDOW_MS = 250.0


def timed(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def window(fn):
    """calls per timed window, from one warm call and one timed call"""
    timed(fn)
    return max(1, int(np.ceil(WINDOW_MS / timed(fn)[0])))


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
        n = window(call)
        out["%dx%d" % (layers - 1, feats)] = [timed(call, n)[0] for _ in range(reps)]
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its view.render is timed too")
    ap.add_argument("--max-only", default=None, metavar="ROOT", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_composite.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("composite_timing.py measures on a ROCm GPU; there is none here")
    sys.path.insert(0, args.max_only or ROOT)
    if args.max_only:
        return max_only(args.edge, args.reps)
    from brief_pytorch_amd import composite, view
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
        top = img.cpu().numpy()[..., 0][hits.cpu().numpy() > 0]
        q25, q100 = int(np.quantile(top, 0.25)), int(top.max())
        points = [(q25, 255, 120, 0, 0.0), ((q25 + q100) // 2, 255, 180, 60, 0.02), (q100, 255, 255, 255, 0.5)]
        comp = lambda bits: (lambda tf: (lambda: composite.render_composite(m, v, tf, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])))(
            torch.from_numpy(composite.make_transfer(points, "u16", 1.0, bits)).cuda())
        calls = {"max": render, "composite": comp(12), "composite8": comp(8)}
        n = {k: window(f) for k, f in calls.items()}                 # warms every shape
        first = {k: f() for k, f in calls.items()}
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                ms[k].append(timed(f, n[k])[0])
        name = "%dx%d" % (layers - 1, feats)
        if parent is not None:
            ms["parent"] = parent[name]
        med = {k: float(np.median(x)) for k, x in ms.items()}
        spread = {k: (float(np.min(x)), float(np.max(x))) for k, x in ms.items()}
        alpha = first["composite"][0][..., 3].cpu().numpy()
        rows.append((name, med, spread, first["composite"][2], n, (q25, q100), alpha))
        print(name + ": " + ", ".join("%s %.2f ms" % (k, med[k]) for k in med))
    keys = ["max", "composite", "composite8"]
    heads = {"parent": "`view.render` max, parent commit (ms)", "max": "`view.render` max (ms)", "composite": "composite, 12-bit table (ms)",
             "composite8": "composite, 8-bit table (ms)"}
    if parent is not None:
        keys = ["parent"] + keys
    base = "parent" if parent is not None else "max"
    with open(args.out, "w") as f:
        f.write("# Composite view: times on one MI355X\n\n`python tools/composite_timing.py --edge %d --reps %d%s`; %d^3 uint16 grid, fp32 SIREN, random "
                "init, an orthographic view turned 45 degrees about z (%d x %d rays of %d samples).  Host clock around a window of calls that "
                "ends in a device synchronise, sized at warm-up to last %.0f ms or more; every shape warmed once; ms per call, median (min .. max) "
                "of %d repetitions, the calls of this tree interleaved in every repetition%s.\n\n"
                % (args.edge, args.reps, " --parent <parent checkout>" if parent is not None else "", args.edge, v.rows, v.cols, v.depth, WINDOW_MS,
                   args.reps, "; the parent commit's max view in a process of its own on the same device" if parent is not None else ""))
        f.write("| net | " + " | ".join(heads[k] for k in keys) + " | composite / %s | composite 8-bit / %s | composite / max of this tree |\n" % (base, base))
        f.write("|---" * (len(keys) + 4) + "|\n")
        for name, med, spread, stats, n, levels, alpha in rows:
            f.write("| %s | " % name + " | ".join("%.2f (%.2f .. %.2f)" % (med[k], spread[k][0], spread[k][1]) for k in keys)
                    + " | %.3f | %.3f | %.3f |\n" % (med["composite"] / med[base], med["composite8"] / med[base], med["composite"] / med["max"]))
        for name, med, spread, stats, n, levels, alpha in rows:
            f.write("\n%s: transfer function from level %d (clear) to %d (white, opacity 0.5 per voxel); %d of %d rays meet the grid, %d samples "
                    "marched; %d pixels clear (A = 0), %d saturated (A = 255); calls per window: %s.\n"
                    % (name, levels[0], levels[1], stats["rays_hit"], stats["rays"], stats["samples_evaluated"], int((alpha == 0).sum()),
                       int((alpha == 255).sum()), ", ".join("%s %d" % (k, n[k]) for k in n)))
        f.write("\nExpected from the code: the fold reads what the max fold reads, plus one 16-byte table row per sample and a scan of lg(lanes) "
                "shuffles per pass; the evaluation of the net is the same.\n")
        f.write("\nThe table's place.  Both tables are read through the cache.  A variant of the fold that copied a table of up to 256 rows to "
                "LDS once per workgroup and gathered it there was measured with this tool before it was dropped: 8-bit table in LDS 1.58 "
                "(1.58 .. 1.60) ms against 1.59 (1.58 .. 1.69) ms for the 12-bit table through the cache behind 4x22, 48.50 (48.46 .. 48.66) "
                "against 48.48 (48.40 .. 48.56) ms behind 4x256: inside the spread, so the fold has one path.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
