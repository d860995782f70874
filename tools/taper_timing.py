"""Tapered-SIREN train-step time (SIREN_Pyramid, SIRENFT, SIRENPS): (1) the fused HIP step (brief_taper_fit through Fitter.step, in-kernel
randompoint draws) against (2) the reference's module and loop body restated with torch.nn under autograd (Adamax) on the same GPU in
the same process, and (3) the same shape zero-padded into a uniform SIREN of the widest layer on the existing fused SIREN path.  The
widths are what opt/SingleTask/siren_pyramid.yaml, sirenft.yaml and sirenps.yaml solve to on a 256^3 and a 512^3 uint16 volume.
SIRENFT's second sine carries w0, which a uniform SIREN cannot express: its row (3) is timed with w0 = 30 for all three paths' shapes
(the time does not depend on w0).  Interleaved A/B/C rounds, each timed with device events around `steps` back-to-back steps; medians.
Also: the fused forward / loss / dgrad kernel's own time (brief_profile_fused), its share of the fp32 MFMA peak from the real widths'
FLOPs, and a 512^3 u16 decode of the 512^3 nets.

    python tools/taper_timing.py [--steps 10] [--rounds 5] [--n 100000]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from brief_pytorch_amd import _lib  # noqa: E402
from brief_pytorch_amd.fit import Fitter  # noqa: E402
from brief_pytorch_amd.networks import SIREN, SIREN_Pyramid, SIRENFT, SIRENPS  # noqa: E402

PEAK_F32_MFMA = 157.3e12      # MI355X fp32 matrix peak, FLOP/s


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


class Sine(torch.nn.Module):
    def __init__(self, w0):
        super().__init__()
        self.w0 = w0

    def forward(self, x):
        return torch.sin(self.w0 * x)


def ref_net(widths, w0s, cin=3, cout=1):
    """the reference's module restated with torch.nn: Linear + Sine(w0_l) per hidden layer, a linear head"""
    mods, i = [], cin
    for o, w in zip(widths, w0s):
        mods += [torch.nn.Linear(i, o), Sine(w)]
        i = o
    mods.append(torch.nn.Linear(i, cout))
    return torch.nn.Sequential(*mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100000)
    a = ap.parse_args()
    dims = (256, 256, 256)
    pop = dims[0] * dims[1] * dims[2]
    vol = torch.rand(pop, 1, device="cuda")
    lin = [torch.linspace(-1, 1, dd, device="cuda") for dd in dims]
    kw = dict(coords_channel=3, data_channel=1, layers=5, res=False)
    specs = [(SIREN_Pyramid, {"features_dis": 10}), (SIRENFT, {"ratio": 2}), (SIRENPS, {"ratio": 1.5})]
    L_ = _lib.lib()
    for cls, extra in specs:
        for side in (256, 512):
            F = cls.calc_features(side ** 3 * 2 / 80 / 4, **kw, **extra)
            torch.manual_seed(0)
            m = cls(features=F, w0=20, **kw, **extra).to("cuda")
            fit = Fitter(m, vol, dims, sampler="randompoint", sample_size=a.n, optimizer="Adamax", lr=1e-3)
            wide = max(m.widths)
            torch.manual_seed(0)
            pad = SIREN(coords_channel=3, data_channel=1, features=wide, layers=5, w0=30 if cls is SIRENFT else 20).to("cuda")
            pfit = Fitter(pad, vol, dims, sampler="randompoint", sample_size=a.n, optimizer="Adamax", lr=1e-3)
            torch.manual_seed(0)
            net = ref_net(m.widths, m.w0s[:len(m.widths)]).cuda()
            opt = torch.optim.Adamax(net.parameters(), lr=1e-3)

            def torch_step():
                idx = torch.randint(0, pop, (a.n,), device="cuda")
                iz = idx // (dims[1] * dims[2])
                iy = (idx // dims[2]) % dims[1]
                ix = idx % dims[2]
                x = torch.stack([lin[0][iz], lin[1][iy], lin[2][ix]], -1)
                opt.zero_grad()
                loss = ((net(x) - vol[idx]) ** 2).mean()
                loss.backward()
                opt.step()

            fns = (fit.step, torch_step, pfit.step)
            for fn in fns:
                timed(fn, 3)
            t = [[], [], []]
            kern_ms, kern_n = 0.0, 0
            for _ in range(a.rounds):
                _lib.check(L_.brief_profile_enable(1))          # in-library events around the fused forward / loss / dgrad launch
                t[0].append(timed(fns[0], a.steps))
                tot, cnt = C.c_double(), C.c_int64()
                _lib.check(L_.brief_profile_fused(C.byref(tot), C.byref(cnt)))
                _lib.check(L_.brief_profile_enable(0))
                kern_ms += tot.value
                kern_n += cnt.value
                t[1].append(timed(fns[1], a.steps))
                t[2].append(timed(fns[2], a.steps))
            med = [sorted(v)[len(v) // 2] for v in t]
            ins, outs = [3] + m.widths, m.widths + [1]
            macs = sum(o * i for o, i in zip(outs[1:], ins[1:]))                  # hidden layers and head: the matrix work
            padded = 3 * wide * wide + wide
            kernel_ms = kern_ms / max(kern_n, 1)
            flops_fwd_kernel = 4.0 * a.n * macs                                 # forward and dgrad chains, real widths
            row = {"net": cls.kind, "volume": "%d^3" % side, "features": F, "widths": m.widths, "n": a.n,
                   "fused_ms": med[0], "torch_ms": med[1], "padded_siren_ms": med[2], "padded_width": wide,
                   "fused_over_torch": med[0] / med[1], "fused_over_padded": med[0] / med[2], "real_over_padded_macs": macs / padded,
                   "fwd_kernel_ms": kernel_ms, "fwd_kernel_share_of_step": kernel_ms / med[0],
                   "fwd_kernel_share_of_f32_mfma_peak": flops_fwd_kernel / (kernel_ms * 1e-3) / PEAK_F32_MFMA if kernel_ms > 0 else None}
            if side == 512:
                g = (512, 512, 512)
                m.decode_grid(g, out_kind="u16", vrange=(0.0, 65535.0))
                row["decode_512cube_ms_min"] = min(timed(lambda: m.decode_grid(g, out_kind="u16", vrange=(0.0, 65535.0)), 1) for _ in range(3))
            print(json.dumps(row), flush=True)
            del fit, pfit, m, pad, net, opt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
