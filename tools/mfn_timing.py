"""MFN train-step time: the fused HIP step (brief_mfn_fit, one optimizer step per call, in-kernel randompoint draws) against the
reference's module under plain torch autograd (MFNBase + FourierLayer / GaborLayer, Adamax) on the same GPU in the same process, both
kinds; plus a 512^3 decode of the 5x525 nets.  Interleaved A/B rounds, each timed with device events around `steps` back-to-back steps;
medians.  The widths are opt/SingleTask/mfn_fourier.yaml's budgets for 256^3 (184) and 512^3 (525).

    python tools/mfn_timing.py [--steps 20] [--rounds 5] [--n 100000]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import torch  # noqa: E402

from brief_pytorch_amd import _lib  # noqa: E402
from brief_pytorch_amd.fit import Fitter  # noqa: E402
from brief_pytorch_amd.networks import MFNFourier, MFNGabor  # noqa: E402


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


class RefMFN(torch.nn.Module):
    """the reference's module restated with torch.nn (utils/Networks.py:648-799), default init scales"""

    def __init__(self, F, L, gabor, cin=3, cout=1):
        super().__init__()
        self.gabor = gabor
        self.linear = torch.nn.ModuleList([torch.nn.Linear(F, F) for _ in range(L - 2)])
        self.output_linear = torch.nn.Linear(F, cout)
        self.filt = torch.nn.ModuleList([torch.nn.Linear(cin, F) for _ in range(L - 1)])
        with torch.no_grad():
            for f in self.filt:
                f.weight *= 256.0 / (L - 1) ** 0.5
        self.mu = torch.nn.ParameterList([torch.nn.Parameter(2 * torch.rand(F, cin) - 1) for _ in range(L - 1)]) if gabor else None
        self.gamma = torch.nn.ParameterList([torch.nn.Parameter(torch.rand(F) + 1) for _ in range(L - 1)]) if gabor else None

    def g(self, i, x):
        h = torch.sin(self.filt[i](x))
        if self.gabor:
            D = (x ** 2).sum(-1)[..., None] + (self.mu[i] ** 2).sum(-1)[None, :] - 2 * x @ self.mu[i].T
            h = h * torch.exp(-0.5 * D * self.gamma[i][None, :])
        return h

    def forward(self, x):
        out = self.g(0, x)
        for i in range(1, len(self.filt)):
            out = self.g(i, x) * self.linear[i - 1](out)
        return self.output_linear(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100000)
    a = ap.parse_args()
    dims = (256, 256, 256)
    pop = dims[0] * dims[1] * dims[2]
    vol = torch.rand(pop, 1, device="cuda")
    lin = [torch.linspace(-1, 1, dd, device="cuda") for dd in dims]
    res = []
    for cls in (MFNFourier, MFNGabor):
        for F in (184, 525):
            L = 5
            torch.manual_seed(0)
            m = cls(coords_channel=3, features=F, data_channel=1, layers=L).to("cuda")
            fit = Fitter(m, vol, dims, sampler="randompoint", sample_size=a.n, optimizer="Adamax", lr=1e-3)
            torch.manual_seed(0)
            net = RefMFN(F, L, cls is MFNGabor).cuda()
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
            row = {"net": "%s %dx%d" % (cls.kind, L, F), "n": a.n, "fused_ms_median": fused[len(fused) // 2], "fused_ms_min": fused[0],
                   "torch_ms_median": ref[len(ref) // 2], "torch_ms_min": ref[0],
                   "fused_fwd_kernel_ms": kern_ms / max(kern_n, 1), "fused_fwd_kernel_launches": kern_n}
            if F == 525:
                g = (512, 512, 512)
                m.decode_grid(g, out_kind="u16", vrange=(0.0, 65535.0))
                dec = [timed(lambda: m.decode_grid(g, out_kind="u16", vrange=(0.0, 65535.0)), 1) for _ in range(3)]
                row["decode_512cube_ms_min"] = min(dec)
            print(json.dumps(row), flush=True)
            res.append(row)
            del fit, m, net, opt
            torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
