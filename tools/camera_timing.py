"""Times the camera view on one MI355X and writes profiles/r24_camera.md:

    python tools/camera_timing.py [--edge 256] [--reps 5] [--parent <checkout of the parent commit, library built>] [--out profiles/r24_camera.md]

An edge^3 uint16 grid behind a 4x256 and a 4x22 fp32 SIREN (random init: the time does not depend on the weights).  The orthographic
view is surface_timing.py's (turned 45 degrees about z out of the x axis); the camera stands outside the volume on that view's axis, two
edges in front of the centre, and looks along the same direction with a 40 degree field of view, edge x edge pixels and unit spacing
along every ray.  Per net, interleaved on one device in every repetition:
    ortho     view.render(..., "max") of the orthographic view;
    camera    view.render_rays(..., "max") through the camera;
    first     view.render_surface_rays, refine=0, no shading;
    refine8   refine=8, no shading;
    shaded    refine=8 with normals and shade under the headlight at the eye.
The two max views evaluate different numbers of samples (both are reported), so they are compared in milliseconds per million
evaluated samples.  With --parent the orthographic max view is ALSO timed by the parent commit's own code and library, in a child process
on the same device: the regression check of the shared march (its margin is the parent's own min-to-max spread over its repetitions).
Host clock around each call, which ends in the device synchronise of its statistics; every shape is warmed once; median and spread of
the repetitions."""
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
FOV = 40.0


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
    """the orthographic max view alone, by whatever package sys.path finds first: {"LxF": [ms, ...]} as one JSON line (the --parent child)"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_camera.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camera_timing.py measures on a ROCm GPU; there is none here")
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
    centre = (np.array(dims, np.float64) - 1.0) / 2.0
    eye = centre - 2.0 * args.edge * np.array(DIRECTION)
    cam = view.make_camera(dims, eye, DIRECTION, up=(1, 0, 0), fov=FOV, size=(args.edge, args.edge))
    rows = []
    for layers, feats in NETS:
        m = make(layers, feats)
        ortho = lambda: view.render(m, v, "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
        camera = lambda: view.render_rays(m, cam, "max", -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"])
        img, hits, _ = camera()
        level = int(np.median(img.cpu().numpy()[..., 0][hits.cpu().numpy() > 0]))
        surf = lambda **kw: (lambda: view.render_surface_rays(m, cam, level, -1.0, 1.0, "u16", EPI["scale"], EPI["vrange"], **kw))
        calls = {"ortho": ortho, "camera": camera, "first": surf(refine=0, shading=False), "refine8": surf(refine=8, shading=False),
                 "shaded": surf(refine=8, shading=True)}
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
        rows.append((name, med, spread, first["ortho"][2], first["camera"][2], first["shaded"]["stats"], level))
        print(name + ": " + ", ".join("%s %.2f ms" % (k, med[k]) for k in med))
    keys = ["ortho", "camera", "first", "refine8", "shaded"]
    heads = {"parent": "`view.render` max, parent commit (ms)", "ortho": "`view.render` max (ms)", "camera": "`view.render_rays` max (ms)",
             "first": "camera surface, refine 0 (ms)", "refine8": "camera surface, refine 8 (ms)", "shaded": "camera surface, refine 8, shaded (ms)"}
    if parent is not None:
        keys = ["parent"] + keys
    with open(args.out, "w") as f:
        f.write("# Camera view: times on one MI355X\n\n`python tools/camera_timing.py --edge %d --reps %d%s`; %d^3 uint16 grid, fp32 SIREN, random "
                "init.  Orthographic view: turned 45 degrees about z, %d x %d rays of %d samples.  Camera: outside the volume on that view's "
                "axis, two edges in front of the centre, field of view %g degrees, %d x %d rays of %d samples at unit spacing.  Host clock "
                "around a call that ends in a device synchronise; every shape warmed once; median (min .. max) of %d repetitions, the calls "
                "of this tree interleaved in every repetition%s.\n\n" % (
                    args.edge, args.reps, " --parent <parent checkout>" if parent is not None else "", args.edge, v.rows, v.cols, v.depth, FOV,
                    cam.rows, cam.cols, cam.depth, args.reps,
                    "; the parent commit's max view in a process of its own on the same device" if parent is not None else ""))
        f.write("| net | " + " | ".join(heads[k] for k in keys) + " | ortho ms / M samples | camera ms / M samples | camera / ortho per sample |\n")
        f.write("|---" * (len(keys) + 4) + "|\n")
        for name, med, spread, so, sc, stats, level in rows:
            per_o, per_c = med["ortho"] / (so["samples_evaluated"] / 1e6), med["camera"] / (sc["samples_evaluated"] / 1e6)
            f.write("| %s | " % name + " | ".join("%.2f (%.2f .. %.2f)" % (med[k], spread[k][0], spread[k][1]) for k in keys)
                    + " | %.3f | %.3f | %.3f |\n" % (per_o, per_c, per_c / per_o))
        for name, med, spread, so, sc, stats, level in rows:
            f.write("\n%s: orthographic view %d of %d rays meet the grid, %d samples evaluated; camera %d of %d rays meet the grid, %d samples "
                    "evaluated (%d inside); surface level %d, %d rays hit the surface (%d cut), %d refinement points.\n" % (
                        name, so["rays_hit"], so["rays"], so["samples_evaluated"], sc["rays_hit"], sc["rays"], sc["samples_evaluated"],
                        sc["samples_inside"], level, stats["rays_surface"], stats["rays_cut"], stats["refine_points"]))
            if parent is not None:
                lo, hi = spread["parent"]
                margin = hi - lo
                verdict = "inside" if lo - margin <= med["ortho"] <= hi + margin else "OUTSIDE"
                f.write("%s regression check: this tree's orthographic max view, median %.2f ms, lies %s the parent's range %.2f .. %.2f ms "
                        "widened by its own spread %.2f ms.\n" % (name, med["ortho"], verdict, lo, hi, margin))
        f.write("\nExpected from the code: per evaluated sample the camera costs what the orthographic view costs where the net's evaluation "
                "dominates (4x256); its clip and coordinates read 24 bytes per ray where the orthographic kernels compute the foot from the "
                "lattice, and its folds test no sample again.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
