"""Times the shaded composite on one MI355X and writes profiles/r23_composite_shade.md:

    python tools/composite_shade_timing.py [--edge 256] [--reps 7] [--parent <checkout of the parent commit, library built>] [--out profiles/r23_composite_shade.md]

composite_timing.py's setting: an edge^3 uint16 grid behind a 4x256 and a 4x22 fp32 SIREN (random init: the time does not depend on
the weights), seen along a direction turned 45 degrees about z out of the x axis.  Two tables: composite_timing.py's SPARSE transfer
function (nothing below the first quartile of the max view's image, dense white at its maximum) and composite_partition_timing.py's
HALF table (every row tau = 2000 and a colour: no sample is transparent and no ray saturates, so every sample needs a gradient).  Per
net and table, interleaved on one device in every repetition:
    plain      composite.render_composite without shade: the parent commit's code path;
    compact    render_composite(shade=(0.2, 0.8)): select, scan, pick, the Jacobian on the selected samples, the shaded fold;
    dense      the same with compact=False: the Jacobian at every sample, slot = NULL.
With --parent the plain composite is ALSO timed by the parent commit's own code and library, in a child process on the same device
(a run of its own, not interleaved with the others).  Host clock around a window of calls that ends in a device synchronise (every
call ends in the synchronise of its statistics anyway); the window is sized at warm-up to last a quarter of a second or more; every
shape is warmed once; median and spread of the repetitions, in ms per call."""
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
HALF_TAU = 2000
SHADE = (0.2, 0.8)
TABLES = ("sparse", "half")


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


def tables(view, composite, m, v):
    """{"sparse": ..., "half": ...} on the device, and the sparse one's two levels"""
    img, hits, _ = view.render(m, v, "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
    top = img.cpu().numpy()[..., 0][hits.cpu().numpy() > 0]
    q25, q100 = int(np.quantile(top, 0.25)), int(top.max())
    points = [(q25, 255, 120, 0, 0.0), ((q25 + q100) // 2, 255, 180, 60, 0.02), (q100, 255, 255, 255, 0.5)]
    half = np.zeros((4096, 4), np.int32)
    half[:, 0] = HALF_TAU
    half[:, 1:] = np.rint(256.0 * np.array([255, 180, 60]) * (1.0 - 2.0 ** (-HALF_TAU / 65536.0)))
    return {"sparse": torch.from_numpy(composite.make_transfer(points, "u16", 1.0)).cuda(), "half": torch.from_numpy(half).cuda()}, (q25, q100)


def plain_only(edge, reps):
    """the plain composite alone, by whatever package sys.path finds first: {"LxF table": [ms, ...]} as one JSON line (the --parent child)"""
    from brief_pytorch_amd import composite, view
    v = view.make_view([edge] * 3, DIRECTION, up=(1, 0, 0))
    out = {}
    for layers, feats in NETS:
        m = make(layers, feats)
        tfs, _ = tables(view, composite, m, v)
        for t in TABLES:
            call = (lambda tf: (lambda: composite.render_composite(m, v, tf, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])))(tfs[t])
            n = window(call)
            out["%dx%d %s" % (layers - 1, feats, t)] = [timed(call, n)[0] for _ in range(reps)]
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its plain composite is timed too")
    ap.add_argument("--plain-only", default=None, metavar="ROOT", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_composite_shade.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("composite_shade_timing.py measures on a ROCm GPU; there is none here")
    sys.path.insert(0, args.plain_only or ROOT)
    if args.plain_only:
        return plain_only(args.edge, args.reps)
    from brief_pytorch_amd import composite, view
    parent = None
    if args.parent:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--edge", str(args.edge), "--reps", str(args.reps), "--plain-only",
                            os.path.abspath(args.parent)], capture_output=True, text=True, cwd=os.path.abspath(args.parent))
        if r.returncode != 0:
            raise SystemExit("the parent's run failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    v = view.make_view([args.edge] * 3, DIRECTION, up=(1, 0, 0))
    rows = []
    for layers, feats in NETS:
        m = make(layers, feats)
        tfs, levels = tables(view, composite, m, v)
        name = "%dx%d" % (layers - 1, feats)
        for t in TABLES:
            args_ = (m, v, tfs[t], -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
            calls = {"plain": lambda a=args_: composite.render_composite(*a),
                     "compact": lambda a=args_: composite.render_composite(*a, shade=SHADE),
                     "dense": lambda a=args_: composite.render_composite(*a, shade=SHADE, compact=False)}
            n = {k: window(f) for k, f in calls.items()}             # warms every shape
            first = {k: f() for k, f in calls.items()}
            assert torch.equal(first["compact"][0], first["dense"][0]) and torch.equal(first["compact"][0][..., 3], first["plain"][0][..., 3])
            ms = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, f in calls.items():
                    ms[k].append(timed(f, n[k])[0])
            if parent is not None:
                ms["parent"] = parent["%s %s" % (name, t)]
            rows.append((name, t, ms, first["compact"][2], n, levels))
            print("%s %s: " % (name, t) + ", ".join("%s %.2f ms" % (k, float(np.median(x))) for k, x in ms.items()))
    med = lambda x: float(np.median(x))
    cell = lambda x: "%.2f (%.2f .. %.2f)" % (med(x), float(np.min(x)), float(np.max(x)))
    keys = (["parent"] if parent is not None else []) + ["plain", "compact", "dense"]
    heads = {"parent": "plain, parent commit (ms)", "plain": "plain (ms)", "compact": "shaded, compacted (ms)", "dense": "shaded, dense (ms)"}
    with open(args.out, "w") as f:
        f.write("# Shaded composite: times on one MI355X\n\n`python tools/composite_shade_timing.py --edge %d --reps %d%s`; %d^3 uint16 grid, fp32 SIREN, "
                "random init, an orthographic view turned 45 degrees about z (%d x %d rays of %d samples), shade = %g,%g with the default light "
                "and scale.  Host clock around a window of calls that ends in a device synchronise, sized at warm-up to last %.0f ms or more; every "
                "shape warmed once; ms per call, median (min .. max) of %d repetitions, the calls of this tree interleaved in every repetition%s.\n\n"
                % (args.edge, args.reps, " --parent <parent checkout>" if parent is not None else "", args.edge, v.rows, v.cols, v.depth, SHADE[0],
                   SHADE[1], WINDOW_MS, args.reps,
                   "; the parent commit's plain composite in a process of its own on the same device" if parent is not None else ""))
        f.write("| net | table | shaded / evaluated | " + " | ".join(heads[k] for k in keys) + " | compact / plain | dense / plain | compact / dense | "
                "(compact - plain) / (dense - plain) |\n")
        f.write("|---" * (len(keys) + 7) + "|\n")
        for name, t, ms, stats, n, levels in rows:
            share = stats["samples_shaded"] / max(1, stats["samples_evaluated"])
            p, c, d = med(ms["plain"]), med(ms["compact"]), med(ms["dense"])
            f.write("| %s | %s | %.4f | " % (name, t, share) + " | ".join(cell(ms[k]) for k in keys)
                    + " | %.3f | %.3f | %.3f | %.3f |\n" % (c / p, d / p, c / d, (c - p) / (d - p)))
        for name, t, ms, stats, n, levels in rows:
            f.write("\n%s, %s table%s: %d of %d rays meet the grid, %d samples marched, %d of them inside, %d selected for a gradient; calls per "
                    "window: %s.\n" % (name, t, " (level %d clear to %d white, opacity 0.5 per voxel)" % levels if t == "sparse" else
                                       " (tau = %d in every row)" % HALF_TAU, stats["rays_hit"], stats["rays"], stats["samples_evaluated"],
                                       stats["samples_inside"], stats["samples_shaded"], ", ".join("%s %d" % (k, n[k]) for k in n)))
        f.write("\nExpected from the code: the dense render adds one Jacobian evaluation per sample (about four decodes, profiles/r18_hessian.md) "
                "and a select pass to the plain one; the compacted render adds the same Jacobian cost times the share of selected samples, the "
                "select pass, a scan, the pick and one host read per chunk.  The last column is the measured share of the dense render's extra "
                "time that the compacted one still pays: next to the share of selected samples it shows what the selection itself costs.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
