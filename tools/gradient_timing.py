"""Times the spatial-gradient decode against what a user can do without it, on one MI355X, and writes profiles/r15_gradient.md:

    python tools/gradient_timing.py [--edge 256] [--reps 3] [--out profiles/r15_gradient.md]

A region of edge^3 voxels behind 4x64, 4x256 and 4x1024 fp32 SIRENs (random init: the time does not depend on the weights).  Per net,
interleaved on one device in every repetition: (a) SIREN.decode_gradient_box (value + Jacobian), (b) SIREN.decode_box(out_kind="f32")
of the same region, (c) torch.autograd.grad of a plain-PyTorch restatement of the net on the same GPU, in chunks of 2^20 voxels.
Device events around each, every shape warmed once, median of the repetitions.  The results are compared before anything is timed."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from brief_pytorch_amd.networks import SIREN      # noqa: E402

NETS = ((5, 64), (5, 256), (5, 1024))
AUTOGRAD_CHUNK = 1 << 20


def torch_layers(m):
    out, off = [], 0
    for (o, i) in m._shapes:
        out.append((m.params[off:off + o * i].view(o, i).clone(), m.params[off + o * i:off + o * i + o].clone()))
        off += o * i + o
    return out


def torch_jacobian(m, layers, coords):
    """the Jacobian a user gets today: the net restated in PyTorch, autograd with respect to the coordinates, chunk by chunk"""
    jac = torch.empty((coords.shape[0], m.data_channel, m.coords_channel), dtype=torch.float32, device=coords.device)
    for off in range(0, coords.shape[0], AUTOGRAD_CHUNK):
        x = coords[off:off + AUTOGRAD_CHUNK].clone().requires_grad_(True)
        h = x
        for l, (W, b) in enumerate(layers[:-1]):
            h = torch.sin((m.w0 if l == 0 else 30.0) * torch.addmm(b, h, W.t()))
        y = torch.addmm(layers[-1][1], h, layers[-1][0].t())
        for c in range(m.data_channel):
            jac[off:off + AUTOGRAD_CHUNK, c] = torch.autograd.grad(y[:, c].sum(), x, retain_graph=c + 1 < m.data_channel)[0]
    return jac


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_gradient.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gradient_timing.py needs a GPU: a time taken elsewhere says nothing"
    dims = (args.edge,) * 3
    n = int(np.prod(dims))
    axes = [torch.linspace(-1.0, 1.0, d, device="cuda") for d in dims]
    coords = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    rows = []
    for layers, feats in NETS:
        torch.manual_seed(0)
        m = SIREN(coords_channel=3, data_channel=1, features=feats, layers=layers, w0=30).to("cuda")
        tl = torch_layers(m)
        runs = {"gradient": lambda: m.decode_gradient_box(dims), "decode": lambda: m.decode_box(dims, out_kind="f32"),
                "autograd": lambda: torch_jacobian(m, tl, coords)}
        # warm-up, and the comparison the timing rests on
        jac, value = m.decode_gradient_box(dims)
        dec = m.decode_box(dims, out_kind="f32")
        ref = torch_jacobian(m, tl, coords)
        err_j = float((jac.view(n, 1, 3) - ref).abs().max() / ref.abs().max())
        err_v = float((value - dec).abs().max() / dec.abs().max())
        del jac, value, dec, ref
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        rows.append((layers - 1, feats, med, err_j, err_v, times))
        print("%dx%d: gradient %.2f ms, decode %.2f ms, autograd %.2f ms; jacobian against torch fp32 %.2e, value against decode_box %.2e" % (
            layers - 1, feats, med["gradient"], med["decode"], med["autograd"], err_j, err_v), flush=True)
    with open(args.out, "w") as f:
        f.write("# r15 — spatial-gradient decode (`k_jac_fwd`, `SIREN.decode_gradient_box`)\n\n")
        f.write("`python tools/gradient_timing.py --edge %d --reps %d` on one MI355X (%s).  A %d³ region (%d voxels) behind fp32 SIRENs at random\n"
                "init, coordinates in [-1, 1].  Per net, interleaved in every repetition: `decode_gradient_box` (value and Jacobian, float32),\n"
                "`decode_box(out_kind=\"f32\")` of the same region, and `torch.autograd.grad` of a plain-PyTorch restatement on the same GPU in chunks\n"
                "of 2^20 voxels (what a user can do today).  Device events, every shape warmed once, median of %d (all repetitions listed).\n\n" % (
                    args.edge, args.reps, torch.cuda.get_device_name(0), args.edge, n, args.reps))
        f.write("| net | `decode_gradient_box` | `decode_box` f32 | gradient / decode | torch autograd | autograd / gradient | Jacobian against torch fp32 | value against `decode_box` |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        for L, F, med, err_j, err_v, _ in rows:
            f.write("| SIREN %d×%d | %.2f ms | %.2f ms | %.2f | %.2f ms | %.2f | %.1e | %.1e |\n" % (
                L, F, med["gradient"], med["decode"], med["gradient"] / med["decode"], med["autograd"], med["autograd"] / med["gradient"], err_j, err_v))
        f.write("\nRepetitions (ms):\n\n")
        for L, F, _, _, _, times in rows:
            f.write("* %d×%d: " % (L, F) + "; ".join("%s %s" % (k, ", ".join("%.2f" % t for t in v)) for k, v in times.items()) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
