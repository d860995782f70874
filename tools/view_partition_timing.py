"""Times the view decode of a partition on one MI355X and writes profiles/r19_view_partition.md:

    python tools/view_partition_timing.py [--edge 256] [--reps 5] [--out profiles/r19_view_partition.md]

An edge^3 uint16 grid, fp32 SIRENs of random init (the time does not depend on the weights).  Interleaved on one device in every
repetition:
    (a)  ONE block through the new path: a one-block partition of a 4x256 and of a 4x22 net through view.render_partition against
         view.render of the same net and view (the single-net path, which the partition path does not touch), for the axis-aligned max
         view along z and for a 45 degree rotating-MIP frame: the overhead of the new path at equal work;
    (b)  partitions of narrow nets: 2x2x2 and 4x4x4 blocks, a 4x22 net each; the axis-aligned max view along z against the per-block
         mip.decode_mips folds that decompress_divide_mip runs (three images there, one here), and the 45 degree frame.
Host clock around each call, which ends in the device synchronise of its statistics (render, render_partition) or in an explicit one
(decode_mips); every shape is warmed once; median and spread of the repetitions.  The images that must agree are compared before
anything is timed."""
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

EPI = dict(scale=(-0.5, 0.5), vrange=(3.0, 60000.0))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def net(features, seed):
    torch.manual_seed(seed)
    return SIREN(coords_channel=3, data_channel=1, features=features, layers=5, w0=20).to("cuda")


def partition(edge, split):
    """split^3 equal blocks of the edge^3 grid, a 4x22 net each: render_partition's parts"""
    n = edge // split
    return [(net(22, 100 + i), [(i // (split * split)) * n, (i // split % split) * n, (i % split) * n], [n] * 3, -1.0, 1.0, EPI["scale"], EPI["vrange"])
            for i in range(split ** 3)]


def block_mips(parts, edge):
    """the fold of decompress_divide_mip: every block's decode_mips into the three full images at its offset"""
    imgs = tuple(torch.zeros((edge, edge, 1), dtype=torch.uint16, device="cuda") for _ in range(3))
    for m, start, dims, lo, hi, scale, vrange in parts:
        mip.decode_mips(m, dims, [0, 0, 0], dims, [1, 1, 1], lo, hi, "u16", scale, vrange, into=imgs, origin=start)
    return imgs


def measure(calls, reps, agree):
    first = {k: timed(f)[1] for k, f in calls.items()}      # warm every shape; and the results that must agree
    for a, b in agree:
        assert np.array_equal(first[a][0].cpu().numpy(), first[b][0].cpu().numpy()), "%s and %s differ" % (a, b)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ms[k].append(timed(f)[0])
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_view_partition.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_partition_timing.py measures on a ROCm GPU; there is none here")
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    dims = [args.edge] * 3
    along_z = view.make_view(dims, (1, 0, 0))
    turned = view.make_view(dims, (0, np.sin(np.pi / 4), np.cos(np.pi / 4)), up=(1, 0, 0))
    cell = lambda t: "%.2f (%.2f .. %.2f)" % t
    lines = ["# View decode of a partition: times on one MI355X\n",
             "`python tools/view_partition_timing.py --edge %d --reps %d`; %d^3 uint16 grid, fp32 SIRENs, random init.  Host clock around a call "
             "that ends in a device synchronise; every shape warmed once; median (min .. max) of %d repetitions, the calls of a table row "
             "interleaved in every repetition; the images that must agree were compared before anything was timed.\n"
             % (args.edge, args.reps, args.edge, args.reps),
             "## (a) One block through the partition path, against `view.render` of the same net and view\n",
             "| net | view | `view.render` (ms) | `view.render_partition`, one block (ms) | ratio |", "|---|---|---|---|---|"]
    for feats in (256, 22):
        m = net(feats, 0)
        one = [(m, [0, 0, 0], dims, -1.0, 1.0, EPI["scale"], EPI["vrange"])]
        calls = {}
        for name, v in (("z", along_z), ("45", turned)):
            calls["single " + name] = lambda v=v: view.render(m, v, "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
            calls["part " + name] = lambda v=v: view.render_partition(one, v, "max", "u16")
        t, _ = measure(calls, args.reps, [("single z", "part z"), ("single 45", "part 45")])
        for name, label in (("z", "axis-aligned max along z"), ("45", "45 degree max")):
            ratio = t["part " + name][0] / t["single " + name][0]
            lines.append("| 4x%d | %s | %s | %s | %.3f |" % (feats, label, cell(t["single " + name]), cell(t["part " + name]), ratio))
            print("(a) 4x%d %s: ratio %.3f" % (feats, name, ratio))
    lines += ["", "## (b) Partitions of 4x22 nets\n",
              "| blocks | per-block `mip.decode_mips` folds, whole grid, three images (ms) | axis-aligned max view along z (ms) | ratio | 45 degree max view (ms) | "
              "rays clipped / rays (z, 45 degree) |", "|---|---|---|---|---|---|"]
    for split in (2, 4):
        parts = partition(args.edge, split)
        calls = {"mips": lambda: block_mips(parts, args.edge),
                 "z": lambda: view.render_partition(parts, along_z, "max", "u16"),
                 "45": lambda: view.render_partition(parts, turned, "max", "u16")}
        t, first = measure(calls, args.reps, [("mips", "z")])
        sz, s45 = first["z"][2], first["45"][2]
        assert sz["samples_evaluated"] == args.edge ** 3 and sz["blocks_hit"] == s45["blocks_hit"] == split ** 3
        lines.append("| %dx%dx%d | %s | %s | %.3f | %s | %.2f, %.2f |" % (split, split, split, cell(t["mips"]), cell(t["z"]), t["z"][0] / t["mips"][0], cell(t["45"]),
                                                                       sz["rays_clipped"] / sz["rays"], s45["rays_clipped"] / s45["rays"]))
        print("(b) %d^3 blocks: mips %.2f ms, z %.2f ms (ratio %.3f), 45 degrees %.2f ms" % (split, t["mips"][0], t["z"][0], t["z"][0] / t["mips"][0], t["45"][0]))
    lines += ["", "(a) is the overhead of the partition path at equal work: the same samples, one more test per sample in the fold, one more search and "
              "device read on the host.  In (b) both columns evaluate every voxel of the grid once; the view pays the explicit coordinates "
              "(12 B written and read per sample) and three launches per block and chunk, the projection decode folds three images."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
