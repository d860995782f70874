"""Times the surface view of a partition on one MI355X and writes profiles/r22_surface_partition.md:

    python tools/surface_partition_timing.py [--edge 256] [--reps 5] [--parent <checkout of the parent commit, library built>]
                                             [--out profiles/r22_surface_partition.md]

An edge^3 uint16 grid, fp32 SIRENs of random init, the orthographic view turned 45 degrees about z of profiles/r17_surface.md.
    (a)  ONE block through the partition path: view.render_surface_partition of a one-block partition against view.render_surface of the
         same net and view, behind 4x256 and 4x22, march only (refine 0, no shading) and with 8 rounds and shading: the overhead of the
         routed path at equal work;
    (b)  2x2x2, 4x4x4 and 8x8x8 partitions of 4x22 nets: the surface view march only, with 8 rounds, and refined and shaded, each against
         view.render_partition(..., "max") of the same partition and view, with refine_launch_blocks and rays_straddle beside them.
With --parent the parent commit's own code and library time ITS view.render_partition max and view.render_surface of the same nets and
view, in a child process on the same device that this process drives call by call: in every repetition the parent's calls and this
tree's alternate.  Host clock around each call, which ends in the device synchronise of its statistics and in an explicit one; every
shape is warmed once; median and spread of the repetitions.  The level is the median over the rays that meet the grid of the max view."""
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def net(features, seed):
    from brief_pytorch_amd.networks import SIREN
    torch.manual_seed(seed)
    return SIREN(coords_channel=3, data_channel=1, features=features, layers=5, w0=20).to("cuda")


def partition(edge, split, features=22):
    """split^3 equal blocks of the edge^3 grid, one net each (seed 100 + i): render_partition's parts"""
    n = edge // split
    return [(net(features, 100 + i), [(i // (split * split)) * n, (i // split % split) * n, (i % split) * n], [n] * 3, -1.0, 1.0, EPI["scale"],
             EPI["vrange"]) for i in range(split ** 3)]


def level_of(view, parts, v):
    img, hits, _ = view.render_partition(parts, v, "max", "u16")
    return int(np.median(img.cpu().numpy()[..., 0][hits.cpu().numpy() > 0]))


def shared_calls(view, parts, v):
    """what the parent commit has too: the max view of the partition and, for one block, the single-net surface view"""
    calls = {"max": lambda: view.render_partition(parts, v, "max", "u16")}
    if len(parts) == 1:
        level = level_of(view, parts, v)
        calls["single"] = lambda: view.render_surface(parts[0][0], v, level, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"], refine=8, shading=True)
    return calls


def serve(edge):
    """the --parent child: whatever package sys.path finds first, driven line by line over stdin: `parts SPLIT FEATURES`, `time KEY`, `quit`"""
    from brief_pytorch_amd import view
    v = view.make_view([edge] * 3, DIRECTION, up=(1, 0, 0))
    calls = {}
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        if word[0] == "parts":
            calls = shared_calls(view, partition(edge, int(word[1]), int(word[2])), v)
            for f in calls.values():
                timed(f)                                         # warm every shape
            print(json.dumps(sorted(calls)), flush=True)
        elif word[0] == "time":
            print(json.dumps(timed(calls[word[1]])[0]), flush=True)
    return 0


class Parent:
    """the child process that runs the parent commit's code"""

    def __init__(self, root, edge):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--edge", str(edge), "--serve", os.path.abspath(root)], cwd=os.path.abspath(root),
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        answer = self.p.stdout.readline()
        if not answer:
            raise SystemExit("the parent's process ended at %r" % line)
        return json.loads(answer)

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.close()
        self.p.wait(timeout=60)


def measure(calls, parent, reps):
    """{key: (median, min, max)} over `reps` repetitions in which the parent's calls ('parent KEY') and this tree's alternate"""
    first = {k: timed(f)[1] for k, f in calls.items()}          # warm every shape
    theirs = parent.keys if parent is not None else []
    ms = {k: [] for k in list(calls) + ["parent " + k for k in theirs]}
    for _ in range(reps):
        for k in theirs:
            ms["parent " + k].append(parent.ask("time " + k))
        for k, f in calls.items():
            ms[k].append(timed(f)[0])
    return {k: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k, x in ms.items()}, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splits", default="2,4,8")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its render_partition and render_surface are timed too")
    ap.add_argument("--serve", default=None, metavar="ROOT", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_surface_partition.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_partition_timing.py measures on a ROCm GPU; there is none here")
    sys.path.insert(0, args.serve or ROOT)
    if args.serve:
        return serve(args.edge)
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    from brief_pytorch_amd import view
    parent = Parent(args.parent, args.edge) if args.parent else None
    dims = [args.edge] * 3
    v = view.make_view(dims, DIRECTION, up=(1, 0, 0))
    cell = lambda t: "%.2f (%.2f .. %.2f)" % t
    theirs = (lambda t, k: cell(t["parent " + k]) if parent is not None else "not measured")
    lines = ["# Surface view of a partition: times on one MI355X\n",
             "`python tools/surface_partition_timing.py --edge %d --reps %d%s`; %d^3 uint16 grid, fp32 SIRENs, random init, an orthographic view turned "
             "45 degrees about z (%d x %d rays of %d samples).  Host clock around a call that ends in a device synchronise; every shape warmed once; "
             "median (min .. max) of %d repetitions, the calls of a table row interleaved in every repetition%s.\n"
             % (args.edge, args.reps, " --parent <parent checkout>" if parent is not None else "", args.edge, v.rows, v.cols, v.depth, args.reps,
                "; the parent commit's calls run in a process of its own on the same device, alternating with this tree's in every repetition"
                if parent is not None else ""),
             "## (a) One block through the partition path, against `view.render_surface` of the same net and view\n",
             "| net | `render_partition` max, parent (ms) | `render_partition` max (ms) | `render_surface` refine 8 shaded, parent (ms) | `render_surface` "
             "refine 8 shaded (ms) | partition path, march only (ms) | partition path, refine 8 shaded (ms) | shaded: partition / single |",
             "|---" * 8 + "|"]
    for feats in (256, 22):
        if parent is not None:
            parent.keys = parent.ask("parts 1 %d" % feats)
        one = partition(args.edge, 1, feats)
        level = level_of(view, one, v)
        calls = shared_calls(view, one, v)
        calls["march"] = lambda: view.render_surface_partition(one, v, level, "u16", refine=0, shading=False)
        calls["shaded"] = lambda: view.render_surface_partition(one, v, level, "u16", refine=8, shading=True)
        t, first = measure(calls, parent, args.reps)
        for key in ("first", "hits", "normal", "shade"):         # (the results that must agree; t is NaN without a hit)
            assert torch.equal(first["shaded"][key], first["single"][key]), key
        assert torch.equal(first["shaded"]["t"].nan_to_num(-1.0), first["single"]["t"].nan_to_num(-1.0))
        lines.append("| 4x%d | %s | %s | %s | %s | %s | %s | %.3f |" % (feats, theirs(t, "max"), cell(t["max"]), theirs(t, "single"), cell(t["single"]),
                                                                       cell(t["march"]), cell(t["shaded"]), t["shaded"][0] / t["single"][0]))
        print("(a) 4x%d: %s" % (feats, ", ".join("%s %.2f ms" % (k, x[0]) for k, x in t.items())), flush=True)
    lines += ["", "## (b) Partitions of 4x22 nets\n",
              "| blocks | `render_partition` max, parent (ms) | `render_partition` max (ms) | surface, march only (ms) | surface, refine 8 (ms) | surface, "
              "refine 8 shaded (ms) | march / max | refine 8 / max | shaded / max | refine_launch_blocks | rays_straddle | rays hit / bracketed |",
              "|---" * 12 + "|"]
    for split in [int(s) for s in args.splits.split(",")]:
        if parent is not None:
            parent.keys = parent.ask("parts %d 22" % split)
        parts = partition(args.edge, split)
        level = level_of(view, parts, v)
        surf = lambda **kw: (lambda: view.render_surface_partition(parts, v, level, "u16", **kw))
        calls = dict(shared_calls(view, parts, v), march=surf(refine=0, shading=False), refine8=surf(refine=8, shading=False), shaded=surf(refine=8, shading=True))
        t, first = measure(calls, parent, args.reps)
        s = first["shaded"]["stats"]
        base = t["parent max"][0] if parent is not None else t["max"][0]
        lines.append("| %dx%dx%d | %s | %s | %s | %s | %s | %.3f | %.3f | %.3f | %d | %d | %d / %d |" % (
            split, split, split, theirs(t, "max"), cell(t["max"]), cell(t["march"]), cell(t["refine8"]), cell(t["shaded"]), t["march"][0] / base,
            t["refine8"][0] / base, t["shaded"][0] / base, s["refine_launch_blocks"], s["rays_straddle"], s["rays_surface"],
            s["rays_surface"] - s["rays_cut"]))
        print("(b) %d^3 blocks: %s; launch blocks %d, straddle %d" % (split, ", ".join("%s %.2f ms" % (k, x[0]) for k, x in t.items()),
                                                                      s["refine_launch_blocks"], s["rays_straddle"]), flush=True)
    if parent is not None:
        parent.close()
    lines += ["", "The ratios of (b) are against the parent commit's max view where it was measured, else against this tree's.  A refinement round is one "
              "route launch, one sort and count with one host read, and coords, forward and step per block that received a point: "
              "refine_launch_blocks counts those blocks over the eight rounds."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
