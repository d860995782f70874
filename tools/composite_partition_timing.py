"""Times the composite view of a partition on one MI355X and writes profiles/r21_composite_partition.md:

    python tools/composite_partition_timing.py [--edge 256] [--reps 5] [--parent <checkout of the parent commit, library built>]
                                               [--out profiles/r21_composite_partition.md]
    python tools/composite_partition_timing.py --split N [--table sparse|half]      (four calls of one case, for a kernel trace)

An edge^3 uint16 grid behind randomly initialised fp32 SIRENs (the time does not depend on the weights), seen along
composite_timing.py's view: turned 45 degrees about z out of the x axis.
  (a) ONE block that covers the grid through composite.render_composite_partition against composite.render_composite of the same
      net, behind a 4x256 and a 4x22 net: what the partition path itself costs.
  (b) n x n x n partitions (n = 2, 4, 8) of 4x22 nets: render_composite_partition against view.render_partition(..., "max") of the
      same partition and view, under composite_timing.py's sparse transfer function (clear below the first quartile of the max
      view's image, dense white at its maximum) and under a table that is half-transparent everywhere (every row tau = 2000: no ray
      saturates, so every segment behind a ray's first one is evaluated twice: the worst case of the second pass).
With --parent the max view of a partition is timed by the parent commit's own code and library, in a child process on the same device
(a run of its own, not interleaved with the others).  Host clock around a window of calls that ends in a device synchronise (every
call ends in the synchronise of its statistics anyway), sized at warm-up to last a quarter of a second or more; every shape is warmed
once; the calls of this tree are interleaved in every repetition; median and spread, in ms per call.  Images are compared before
timing: the one-block image with render_composite's, a partition's with the same partition in reversed block order.
The kernel-time split of a --split trace and the reading of the figures are kept by hand in profiles/r21_composite_partition_split.md,
a file of its own that a new run of this tool leaves alone."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI = dict(scale=(-0.5, 0.5), vrange=(3.0, 60000.0))
DIRECTION = (0.0, float(np.sin(np.pi / 4)), float(np.cos(np.pi / 4)))
SPLITS = (2, 4, 8)
HALF_TAU = 2000
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


def make(layers, feats, seed=0):
    from brief_pytorch_amd.networks import SIREN
    torch.manual_seed(seed)
    return SIREN(coords_channel=3, data_channel=1, features=feats, layers=layers, w0=20).to("cuda")


def partition(edge, n, layers=5, feats=22):
    """n x n x n equal blocks of the edge^3 grid, one net per block (seed = the block's number)"""
    step = edge // n
    assert step * n == edge and step >= 2
    return [(make(layers, feats, seed=i), [(i // (n * n)) * step, (i // n % n) * step, (i % n) * step], [step] * 3, -1.0, 1.0,
             EPI["scale"], EPI["vrange"]) for i in range(n ** 3)]


def max_only(edge, reps):
    """the max view of the partitions alone, by whatever package sys.path finds first: {"n": [ms, ...]} as one JSON line (the --parent child)"""
    from brief_pytorch_amd import view
    v = view.make_view([edge] * 3, DIRECTION, up=(1, 0, 0))
    out = {}
    for n in SPLITS:
        parts = partition(edge, n)
        call = lambda: view.render_partition(parts, v, "max", "u16")
        calls = window(call)
        out[str(n)] = [timed(call, calls)[0] for _ in range(reps)]
    print(json.dumps(out))
    return 0


def tables(view_mod, composite, parts, v):
    """{"sparse": composite_timing.py's transfer function on this partition's max image, "half": half-transparent everywhere} on the device"""
    img, hits, _ = view_mod.render_partition(parts, v, "max", "u16")
    top = img.cpu().numpy()[..., 0][hits.cpu().numpy() > 0]
    q25, q100 = int(np.quantile(top, 0.25)), int(top.max())
    points = [(q25, 255, 120, 0, 0.0), ((q25 + q100) // 2, 255, 180, 60, 0.02), (q100, 255, 255, 255, 0.5)]
    half = np.zeros((4096, 4), np.int32)
    half[:, 0] = HALF_TAU
    half[:, 1:] = np.rint(256.0 * np.array([255, 180, 60]) * (1.0 - 2.0 ** (-HALF_TAU / 65536.0)))
    return {"sparse": torch.from_numpy(composite.make_transfer(points, "u16", 1.0)).cuda(), "half": torch.from_numpy(half).cuda()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its view.render_partition is timed too")
    ap.add_argument("--max-only", default=None, metavar="ROOT", help=argparse.SUPPRESS)
    ap.add_argument("--split", type=int, default=None, metavar="N", help="run four calls of the N x N x N composite (one warm call and three more) and exit (for a kernel trace)")
    ap.add_argument("--table", default="half", choices=("sparse", "half"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_composite_partition.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("composite_partition_timing.py measures on a ROCm GPU; there is none here")
    sys.path.insert(0, args.max_only or ROOT)
    if args.max_only:
        return max_only(args.edge, args.reps)
    from brief_pytorch_amd import composite, view
    dims = [args.edge] * 3
    v = view.make_view(dims, DIRECTION, up=(1, 0, 0))
    if args.split is not None:
        parts = partition(args.edge, args.split)
        tf = tables(view, composite, parts, v)[args.table]
        for _ in range(4):                                       # (one warm call and three more)
            stats = composite.render_composite_partition(parts, v, tf, "u16")[2]
        torch.cuda.synchronize()
        print(json.dumps(stats))
        return 0
    parent = None
    if args.parent:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--edge", str(args.edge), "--reps", str(args.reps), "--max-only",
                            os.path.abspath(args.parent)], capture_output=True, text=True, cwd=os.path.abspath(args.parent))
        if r.returncode != 0:
            raise SystemExit("the parent's run failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    med = lambda x: float(np.median(x))
    cell = lambda x: "%.2f (%.2f .. %.2f)" % (med(x), min(x), max(x))
    # ---- (a) one block through the partition path
    rows_a = []
    for layers, feats in ((5, 256), (5, 22)):
        m = make(layers, feats)
        parts = [(m, [0, 0, 0], dims, -1.0, 1.0, EPI["scale"], EPI["vrange"])]
        tf = tables(view, composite, parts, v)["sparse"]
        calls = {"single": lambda: composite.render_composite(m, v, tf, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"]),
                 "partition": lambda: composite.render_composite_partition(parts, v, tf, "u16")}
        first = {k: f() for k, f in calls.items()}
        assert torch.equal(first["single"][0], first["partition"][0]) and torch.equal(first["single"][1], first["partition"][1])
        n = {k: window(f) for k, f in calls.items()}
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                ms[k].append(timed(f, n[k])[0])
        rows_a.append(("%dx%d" % (layers - 1, feats), ms, first["partition"][2]))
        print(rows_a[-1][0] + ": " + ", ".join("%s %.2f ms" % (k, med(x)) for k, x in ms.items()), flush=True)
    # ---- (b) n x n x n partitions of 4x22 nets
    rows_b = []
    for split in SPLITS:
        parts = partition(args.edge, split)
        tfs = tables(view, composite, parts, v)
        calls = {"max": lambda: view.render_partition(parts, v, "max", "u16")}
        for name, tf in tfs.items():
            calls[name] = (lambda tf: (lambda: composite.render_composite_partition(parts, v, tf, "u16")))(tf)
        first = {k: f() for k, f in calls.items()}
        for name, tf in tfs.items():
            back = composite.render_composite_partition(parts[::-1], v, tf, "u16")
            assert torch.equal(back[0], first[name][0]) and torch.equal(back[1], first[name][1]) and back[2] == first[name][2]
        n = {k: window(f) for k, f in calls.items()}
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                ms[k].append(timed(f, n[k])[0])
        if parent is not None:
            ms["parent"] = parent[str(split)]
        rows_b.append((split, ms, {k: first[k][2] for k in tfs}))
        print("%d^3 blocks: " % split + ", ".join("%s %.2f ms" % (k, med(x)) for k, x in ms.items()), flush=True)
    base = "parent" if parent is not None else "max"
    with open(args.out, "w") as f:
        f.write("# Composite view of a partition: times on one MI355X\n\n`python tools/composite_partition_timing.py --edge %d --reps %d%s`; %d^3 uint16 "
                "grid, fp32 SIRENs, random init, an orthographic view turned 45 degrees about z (%d x %d rays of %d samples).  Host clock around a "
                "window of calls that ends in a device synchronise, sized at warm-up to last %.0f ms or more; every shape warmed once; ms per call, "
                "median (min .. max) of %d repetitions, the calls of this tree interleaved in every repetition%s.  Images were compared before "
                "timing (one block: with `render_composite`'s; partitions: with the reversed block order), bit for bit.\n\n"
                % (args.edge, args.reps, " --parent <parent checkout>" if parent is not None else "", args.edge, v.rows, v.cols, v.depth, WINDOW_MS,
                   args.reps, "; the parent commit's `render_partition` in a process of its own on the same device" if parent is not None else ""))
        f.write("## (a) One block through the partition path\n\n| net | `render_composite` (ms) | `render_composite_partition`, one block (ms) | ratio |\n|---|---|---|---|\n")
        for name, ms, stats in rows_a:
            f.write("| %s | %s | %s | %.3f |\n" % (name, cell(ms["single"]), cell(ms["partition"]), med(ms["partition"]) / med(ms["single"])))
        f.write("\nSparse transfer function; %d samples marched, none twice.\n\n" % rows_a[0][2]["samples_evaluated"])
        f.write("## (b) Partitions of 4x22 nets\n\n| blocks | %s`render_partition` max (ms) | composite, sparse table (ms) | composite, half-transparent table (ms) | "
                "sparse / %s | half / %s | second pass / inside, sparse | second pass / inside, half | segments |\n|---|---|---|---|---|---|---|---|---|%s\n"
                % ("`render_partition` max, parent commit (ms) | " if parent is not None else "", base, base, "---|" if parent is not None else ""))
        for split, ms, stats in rows_b:
            f.write("| %d^3 | %s%s | %s | %s | %.3f | %.3f | %.3f | %.3f | %d |\n" % (
                split, cell(ms["parent"]) + " | " if parent is not None else "", cell(ms["max"]), cell(ms["sparse"]), cell(ms["half"]),
                med(ms["sparse"]) / med(ms[base]), med(ms["half"]) / med(ms[base]),
                stats["sparse"]["samples_second_pass"] / stats["sparse"]["samples_inside"],
                stats["half"]["samples_second_pass"] / stats["half"]["samples_inside"], stats["half"]["segments"]))
        f.write("\nExpected from the code: about 1 + (second pass / inside) times the max view, plus the per-block launches of the second pass and "
                "two more small reads; the carry and the gather loop over all blocks per window ray and per pixel.\n")
        f.write("\nThe kernel-time split of a call (a separate `rocprofv3 --kernel-trace --stats` run of `--split N`) and a reading of these figures "
                "are kept by hand in `profiles/r21_composite_partition_split.md`; this tool does not write that file.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
