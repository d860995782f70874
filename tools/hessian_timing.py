"""Times the Hessian decode against the gradient decode and the plain decode on one MI355X, measures its distance from the float64
yardstick on the parity cases of tests/test_gpu_hessian.py, and writes profiles/r18_hessian.md:

    python tools/hessian_timing.py [--edge 256] [--reps 5] [--out profiles/r18_hessian.md]

A region of edge^3 voxels behind 4x256 and 4x22 fp32 SIRENs (random init: the time does not depend on the weights).  Per net, interleaved
on one device in every repetition: (a) SIREN.decode_hessian_box (Hessian only), (b) SIREN.decode_gradient_box (value + Jacobian), (c)
SIREN.decode_box(out_kind="f32").  Device events around each, every shape warmed once, median of the repetitions (all listed).  The
results are compared before anything is timed."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from brief_pytorch_amd.fit import Fitter                      # noqa: E402
from brief_pytorch_amd.networks import SIREN                  # noqa: E402
from brief_pytorch_amd.synthetic import make_volume           # noqa: E402
from tests._hessian import CASES, case_coords, reference, value_jacobian_hessian      # noqa: E402
from tests._jacobian import relerr                            # noqa: E402

NETS = ((5, 256), (5, 22))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def parity():
    """(case, hessian distance from float64, torch fp32's own distance) of the fourteen initialised cases and of the fitted one"""
    rows = []
    for case in CASES:
        m, x, _, _, h64, _, own = reference(case)
        torch.manual_seed(0)
        g = SIREN(coords_channel=case[0], data_channel=case[1], features=case[3], layers=case[2], w0=30, output_act=case[5])
        assert torch.equal(g.params, m.params)
        hess = g.to("cuda").spatial_hessian(x.to("cuda"))[2].cpu().numpy()
        rows.append((str(case), relerr(hess, h64), own))
    dims = (12, 20, 28)
    torch.manual_seed(2)
    m = SIREN(coords_channel=3, data_channel=1, features=48, layers=5, w0=30).to("cuda")
    vol = make_volume(dims, seed=3).astype(np.float32).reshape(-1, 1)
    vol = (vol - vol.min()) / (vol.max() - vol.min()) * 100.0
    Fitter(m, torch.from_numpy(vol).to("cuda"), dims, sampler="randompoint", sample_size=2000, optimizer="Adamax", lr=1e-3, seed=1).run(200)
    x = case_coords(300, 3, seed=9)
    _, _, h64 = value_jacobian_hessian(m, x, torch.float64)
    _, _, h32 = value_jacobian_hessian(m, x, torch.float32)
    rows.append(("4x48 after a 200-step fit, n = 300", relerr(m.spatial_hessian(x.to("cuda"))[2].cpu().numpy(), h64), relerr(h32, h64)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_hessian.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hessian_timing.py needs a GPU: a time taken elsewhere says nothing"
    dims = (args.edge,) * 3
    n = int(np.prod(dims))
    rows = []
    for layers, feats in NETS:
        torch.manual_seed(0)
        m = SIREN(coords_channel=3, data_channel=1, features=feats, layers=layers, w0=30).to("cuda")
        runs = {"hessian": lambda: m.decode_hessian_box(dims), "gradient": lambda: m.decode_gradient_box(dims),
                "decode": lambda: m.decode_box(dims, out_kind="f32")}
        # warm-up, and the comparison the timing rests on: the kernel's own value and Jacobian against the other two decodes
        hess, value, jac = m.decode_hessian_box(dims, want_value=True, want_jac=True)
        gj, gv = m.decode_gradient_box(dims)
        dec = m.decode_box(dims, out_kind="f32")
        err_j = float((jac - gj).abs().max() / gj.abs().max())
        err_v = float((value - dec.view_as(value)).abs().max() / dec.abs().max())
        del hess, value, jac, gj, gv, dec
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        rows.append((layers - 1, feats, med, err_j, err_v, times))
        print("%dx%d: hessian %.2f ms, gradient %.2f ms, decode %.2f ms; jacobian against decode_gradient_box %.2e, value against decode_box %.2e" % (
            layers - 1, feats, med["hessian"], med["gradient"], med["decode"], err_j, err_v), flush=True)
    par = parity()
    for what, got, own in par:
        print("%s: hessian relerr %.3e, torch fp32 against float64 %.3e" % (what, got, own), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# r18 — Hessian decode (`k_hess_fwd`, `SIREN.decode_hessian_box`)\n\n")
        f.write("`python tools/hessian_timing.py --edge %d --reps %d` on one MI355X (%s).  A %d³ region (%d voxels) behind fp32 SIRENs at random\n"
                "init, coordinates in [-1, 1].  Per net, interleaved in every repetition: `decode_hessian_box` (the six second derivatives, float32),\n"
                "`decode_gradient_box` (value and Jacobian; the kernel of the parent commit, unchanged) and `decode_box(out_kind=\"f32\")` of the same\n"
                "region.  Device events, every shape warmed once, median of %d (all repetitions listed).\n\n" % (
                    args.edge, args.reps, torch.cuda.get_device_name(0), args.edge, n, args.reps))
        f.write("| net | `decode_hessian_box` | `decode_gradient_box` | `decode_box` f32 | hessian / gradient | hessian / decode | ns per voxel (hessian) | Jacobian against `decode_gradient_box` | value against `decode_box` |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for L, F, med, err_j, err_v, _ in rows:
            f.write("| SIREN %d×%d | %.2f ms | %.2f ms | %.2f ms | %.2f | %.2f | %.2f | %.1e | %.1e |\n" % (
                L, F, med["hessian"], med["gradient"], med["decode"], med["hessian"] / med["gradient"], med["hessian"] / med["decode"],
                1e6 * med["hessian"] / n, err_j, err_v))
        f.write("\nRepetitions (ms):\n\n")
        for L, F, _, _, _, times in rows:
            f.write("* %d×%d: " % (L, F) + "; ".join("%s %s" % (k, ", ".join("%.2f" % t for t in v)) for k, v in times.items()) + "\n")
        f.write("\n## Distance from the float64 yardstick\n\n"
                "The parity cases of `tests/test_gpu_hessian.py` (`(cin, cout, layers, features, n, output_act)`), `relerr = max|a - b| / max|b|` of the\n"
                "Hessian against the float64 double-autograd restatement (`tests/_hessian.py`); `own` is torch's fp32 restatement against the same.\n"
                "The band is `max(1e-4, 3 × own)`.\n\n| case | `k_hess_fwd` | own (torch fp32) |\n|---|---|---|\n")
        for what, got, own in par:
            f.write("| %s | %.2e | %.2e |\n" % (what, got, own))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
