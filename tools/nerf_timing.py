"""NeRF train-step time: the fused HIP step (brief_nerf_fit, one optimizer step per call, in-kernel randompoint draws) against the
reference's module under plain torch autograd (PosEncodingNeRF + nn.Linear stack with the skip concatenation, Adamax) on the same GPU
in the same process; plus a 512^3 decode of the 5x507 net.  Interleaved A/B rounds, each timed with device events around `steps`
back-to-back steps.  The widths are opt/SingleTask/nerf.yaml's budgets for 256^3 (166) and 512^3 (507).

    python tools/nerf_timing.py [--steps 20] [--rounds 5] [--n 100000]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import torch  # noqa: E402

from brief_pytorch_amd import _lib  # noqa: E402

from brief_pytorch_amd.fit import Fitter  # noqa: E402
from brief_pytorch_amd.networks import NeRF  # noqa: E402

PEAK_TF = 157.3


def flops(F, d, L, cout, n):
    """algorithmic FLOPs of one step (skip on): forward 2 (2 d F + (L-2) F^2 + F cout) per sample; backward = dgrad into the hidden
    inputs of every layer but the first (2 ((L-2) F^2 + F cout)) + weight gradients of every layer (2 (2 d F + (L-2) F^2 + F cout))"""
    fwd = 2 * (2 * d * F + (L - 2) * F * F + F * cout)
    dgrad = 2 * ((L - 2) * F * F + F * cout)
    return n * (2 * fwd + dgrad)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100000)
    a = ap.parse_args()
    dims = (256, 256, 256)
    pop = dims[0] * dims[1] * dims[2]
    vol = torch.rand(pop, 1, device="cuda")
    res = []
    for F in (166, 507):
        Lf, L = 10, 5
        d = 3 * (1 + 2 * Lf)
        torch.manual_seed(0)
        m = NeRF(coords_channel=3, data_channel=1, features=F, layers=L, frequencies=Lf, skip=True).to("cuda")
        fit = Fitter(m, vol, dims, sampler="randompoint", sample_size=a.n, optimizer="Adamax", lr=1e-3)
        # torch autograd: the reference's module and loop body (main.py:385-400), randompoint indices drawn on the device
        torch.manual_seed(0)
        sl = (L - 1) // 2
        net = torch.nn.ModuleList([torch.nn.Linear(d, F)] + [torch.nn.Linear(d + F if l == sl else F, F) for l in range(1, L - 1)]
                                  + [torch.nn.Linear(F, 1)]).cuda()
        opt = torch.optim.Adamax(net.parameters(), lr=1e-3)
        lin = [torch.linspace(-1, 1, dd, device="cuda") for dd in dims]

        def forward(x):
            enc = [x]
            for i in range(Lf):                       # PosEncodingNeRF: frequency loop outside, channel loop inside
                for j in range(3):
                    c = x[:, j:j + 1]
                    enc += [torch.sin((2 ** i) * math.pi * c), torch.cos((2 ** i) * math.pi * c)]
            codings = torch.cat(enc, -1)
            h = codings
            for l, layer in enumerate(net):
                if l == sl:
                    h = torch.cat([codings, h], 1)
                h = layer(h)
                if l < L - 1:
                    h = torch.relu(h)
            return h

        def torch_step():
            idx = torch.randint(0, pop, (a.n,), device="cuda")
            iz = idx // (dims[1] * dims[2])
            iy = (idx // dims[2]) % dims[1]
            ix = idx % dims[2]
            x = torch.stack([lin[0][iz], lin[1][iy], lin[2][ix]], -1)
            opt.zero_grad()
            loss = ((forward(x) - vol[idx]) ** 2).mean()
            loss.backward()
            opt.step()

        def fused_step():
            fit.step()

        for fn in (fused_step, torch_step):
            timed(fn, 5)
        fused, ref = [], []
        L_ = _lib.lib()
        kern_ms, kern_n = 0.0, 0
        for _ in range(a.rounds):
            _lib.check(L_.brief_profile_enable(1))          # in-library events around the fused forward / loss / dgrad launch
            fused.append(timed(fused_step, a.steps))
            tot, cnt = C.c_double(), C.c_int64()
            _lib.check(L_.brief_profile_fused(C.byref(tot), C.byref(cnt)))
            _lib.check(L_.brief_profile_enable(0))
            kern_ms += tot.value
            kern_n += cnt.value
            ref.append(timed(torch_step, a.steps))
        fused.sort()
        ref.sort()
        fl = flops(F, d, L, 1, a.n)
        row = {"net": "%dx%d" % (L, F), "frequencies": Lf, "skip": True, "n": a.n, "fused_ms_median": fused[len(fused) // 2], "fused_ms_min": fused[0],
               "torch_ms_median": ref[len(ref) // 2], "torch_ms_min": ref[0],
               "fused_frac_peak": fl / (fused[len(fused) // 2] * 1e-3) / (PEAK_TF * 1e12),
               "torch_frac_peak": fl / (ref[len(ref) // 2] * 1e-3) / (PEAK_TF * 1e12), "gflop_per_step": fl / 1e9,
               "fused_fwd_kernel_ms": kern_ms / max(kern_n, 1), "fused_fwd_kernel_launches": kern_n}
        if F == 507:
            g = (512, 512, 512)
            m.decode_grid(g, out_kind="u16", vrange=(0.0, 65535.0))
            dec = []
            for _ in range(3):
                dec.append(timed(lambda: m.decode_grid(g, out_kind="u16", vrange=(0.0, 65535.0)), 1))
            row["decode_512cube_ms_min"] = min(dec)
            row["decode_voxels_per_s"] = 512 ** 3 / (min(dec) * 1e-3)
        print(json.dumps(row), flush=True)
        res.append(row)
    return res


if __name__ == "__main__":
    main()
