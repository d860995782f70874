"""sha256 of the parameters after a short fit, per net width — run once per library build (BRIEF_LIB=...) and diff the outputs: a change that
claims 'same bits' (a re-vectorised k_reduce, a re-ordered launch plan, a refactored host driver) must print identical lines.
    python tools/lib_checksum.py L F1,F2,... [steps] [n] [family[,family...]] [--edge 128] [--embsize 256] [--skip 1]
family: siren (default), ffn, nerf, mfn_fourier, mfn_gabor, pyramid, ft, ps.  For the tapered nets F is the widest layer."""
import argparse
import hashlib
import sys
import torch
sys.path.insert(0, '.')
from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import FFN, MFNFourier, MFNGabor, NeRF, SIREN, SIREN_Pyramid, SIRENFT, SIRENPS

ap = argparse.ArgumentParser()
ap.add_argument("L", type=int)
ap.add_argument("Fs")
ap.add_argument("steps", type=int, nargs="?", default=30)
ap.add_argument("n", type=int, nargs="?", default=100000)
ap.add_argument("family", nargs="?", default="siren")
ap.add_argument("--edge", type=int, default=128, help="the fitted volume is edge^3")
ap.add_argument("--embsize", type=int, default=256, help="ffn: embedding size")
ap.add_argument("--skip", type=int, default=1, help="nerf: skip connection")
a = ap.parse_args()
L = a.L
MAKE = {
    "siren": lambda F: SIREN(features=F, layers=L, w0=20),
    "ffn": lambda F: FFN(features=F, layers=L, embsize=a.embsize),
    "nerf": lambda F: NeRF(features=F, layers=L, frequencies=10, skip=bool(a.skip)),
    "mfn_fourier": lambda F: MFNFourier(features=F, layers=L),
    "mfn_gabor": lambda F: MFNGabor(features=F, layers=L),
    "pyramid": lambda F: SIREN_Pyramid(features=F, layers=L, w0=20, features_dis=max(1, F // 8)),
    "ft": lambda F: SIRENFT(features=F / 2, layers=L, w0=20, ratio=2),
    "ps": lambda F: SIRENPS(features=F / 2 ** (L - 2), layers=L, w0=20, ratio=2),
}
dims = (a.edge,) * 3
torch.manual_seed(1)
tv = torch.rand(a.edge ** 3, 1, device='cuda') * 100
for family in a.family.split(','):
    tag = "" if family == "siren" else " %s%s" % (family, {"ffn": " E=%d" % a.embsize, "nerf": " skip=%d" % a.skip}.get(family, ""))
    for F in [int(v) for v in a.Fs.split(',')]:
        for opt in ('Adamax', 'Adam'):
            torch.manual_seed(7)
            m = MAKE[family](F).to('cuda')
            f = Fitter(m, tv, dims, sampler='randompoint', sample_size=a.n, optimizer=opt, lr=1e-3, seed=5)
            f.run(a.steps)
            torch.cuda.synchronize()
            h = hashlib.sha256(m.params.detach().cpu().numpy().tobytes()).hexdigest()[:16]
            hp = hashlib.sha256(m.packed.detach().cpu().numpy().tobytes()).hexdigest()[:16] if getattr(m, 'packed', None) is not None else '-'
            print("L=%d F=%d%s %s: params %s packed %s" % (L, F, tag, opt, h, hp), flush=True)
