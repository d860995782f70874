"""MFNFourier / MFNGabor on the fused HIP path, against the reference's own outputs (tests/golden/mfn.npz) and a float64 torch
restatement of its module (utils/Networks.py:648-799).

Bands are a multiple of the distance between the float32 and the float64 restatement of the SAME case, measured in the test itself
(as in tests/test_gpu_nerf.py), plus a small floor relative to the magnitude of the quantity.  The default init drives filter phases to
a few hundred radians, so both fp32 paths carry phase errors of ~1e-5; the band measures that instead of assuming it."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import MFNFourier, MFNGabor
from tests._family_ref import BAND_FACTOR, FLOOR, band_check, rand_coords, torch_loss, torch_mfn

pytestmark = pytest.mark.gpu
KINDS = {"fourier": MFNFourier, "gabor": MFNGabor}


def golden_band(got, gold, e32, scale, what):
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(gold, np.float64))))
    bound = (BAND_FACTOR + 1) * e32 + FLOOR * scale
    assert err <= bound, "%s: %.3e from the reference golden, bound %.3e (fp32 torch vs float64: %.3e)" % (what, err, bound, e32)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("k", range(10))
def test_forward_matches_reference_golden_and_float64(golden, kind, k):
    g = golden("mfn")
    cin, cout, L, F, oa = (int(v) for v in g["%s_fwd%d_cfg" % (kind, k)])
    torch.manual_seed(int(g["%s_fwd%d_seed" % (kind, k)]))
    m = KINDS[kind](coords_channel=cin, features=F, data_channel=cout, layers=L, output_act=bool(oa)).to("cuda")
    x = torch.from_numpy(g["%s_fwd%d_x" % (kind, k)])
    y = m.forward(x.cuda()).cpu().numpy()
    y64, _ = torch_mfn(m, x, torch.float64)
    y32, _ = torch_mfn(m, x, torch.float32)
    y64, y32 = y64.detach().numpy(), y32.detach().numpy()
    what = "%s forward %s" % (kind, (cin, cout, L, F, oa))
    band_check(y, y64, y32, what)
    gold = g["%s_fwd%d_y" % (kind, k)]
    golden_band(y, gold, float(np.max(np.abs(y32 - y64))), float(np.max(np.abs(gold))), what + " vs golden")


def _groups(m):
    """parameter groups checked separately: hidden W / b, head, filter W / b, and for Gabor mu / gamma"""
    out = {}
    for k, _, _ in m._entries:
        if k.startswith("linear."):
            grp = "hidden " + k.rsplit(".", 1)[1]
        elif k.startswith("output_linear"):
            grp = "head " + k.rsplit(".", 1)[1]
        else:
            grp = "filter " + k.rsplit(".", 1)[1]
        out.setdefault(grp, []).append(k)
    return out


@pytest.mark.parametrize("loss,weighted,thr", [("datal2", False, 0.0), ("datasmoothl1", True, 0.0), ("datal2", True, 0.3)])
@pytest.mark.parametrize("kind,cin,cout,L,F,oa,n", [
    ("fourier", 3, 1, 5, 31, 0, 2000), ("gabor", 3, 1, 5, 33, 1, 1500), ("fourier", 2, 3, 3, 64, 1, 1111), ("gabor", 2, 4, 4, 65, 0, 999),
    ("fourier", 3, 1, 2, 32, 0, 700), ("gabor", 3, 2, 2, 20, 1, 700), ("fourier", 3, 1, 5, 184, 0, 800), ("gabor", 3, 1, 5, 184, 0, 800),
    ("gabor", 3, 1, 3, 525, 0, 500), ("fourier", 3, 1, 3, 1024, 1, 300), ("gabor", 3, 1, 3, 1024, 0, 300)])
def test_train_step_band(kind, cin, cout, L, F, oa, n, loss, weighted, thr):
    torch.manual_seed(7)
    m = KINDS[kind](coords_channel=cin, features=F, data_channel=cout, layers=L, output_act=bool(oa)).to("cuda")
    x = rand_coords(n, cin, 11)
    g = torch.Generator().manual_seed(5)
    y = torch.rand(n, cout, generator=g)
    w = (torch.rand(n, cout, generator=g) * 3 + 0.5) if weighted else torch.ones(n, cout)
    lo, _ = m.train_step(n, y.cuda().contiguous(), coords=x.cuda().contiguous(), weights=w.cuda().contiguous() if weighted else None,
                         loss=loss, thr=thr, beta=0.05)
    got_loss = lo.item()
    got = m.grads.cpu().numpy()
    res = {}
    for dt in (torch.float64, torch.float32):
        yh, t = torch_mfn(m, x, dt)
        lt = torch_loss(yh, y.to(dt), w.to(dt), loss, thr, 0.05)
        lt.backward()
        res[dt] = (lt.item(), {k: v.grad.numpy() for k, v in t.items()})
    band_check([got_loss], [res[torch.float64][0]], [res[torch.float32][0]], "loss")
    off = {k: (o, int(np.prod(shp))) for k, o, shp in m._entries}
    for grp, keys in _groups(m).items():
        for k in keys:          # every tensor in its own band, reported under its group
            o, cnt = off[k]
            band_check(got[o:o + cnt], res[torch.float64][1][k].reshape(-1), res[torch.float32][1][k].reshape(-1), "%s grad (%s)" % (grp, k))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_decode_grid_chunks_forward_and_box_equals_slice(kind):
    cls = KINDS[kind]
    torch.manual_seed(3)
    m = cls(coords_channel=3, features=45, data_channel=1, layers=5).to("cuda")
    dims = (9, 13, 17)
    full = m.decode_grid(dims)
    lin = [torch.linspace(-1, 1, d) for d in dims]
    coords = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3)
    assert torch.equal(full.cpu(), m.forward(coords.cuda()).cpu())
    total = int(np.prod(dims))
    parts = [m.decode_grid(dims, offset=o, count=min(333, total - o)) for o in range(0, total, 333)]
    assert torch.equal(torch.cat(parts).cpu(), full.cpu()), "decode is invariant under chunking"
    box = m.decode_box(dims, start=(1, 2, 3), stop=(8, 12, 16), step=(2, 3, 1))
    assert torch.equal(box.cpu(), full.view(*dims, 1)[1:8:2, 2:12:3, 3:16].cpu())
    assert torch.equal(m.decode_box(dims, start=(1, 2, 3), stop=(8, 12, 16), step=(2, 3, 1), chunk=7).cpu(), box.cpu())
    u = m.decode_grid(dims, out_kind="u16", scale=(0.0, 100.0), vrange=(0.0, 65535.0))
    ub = m.decode_box(dims, start=(0, 5, 0), stop=(9, 6, 17), out_kind="u16", scale=(0.0, 100.0), vrange=(0.0, 65535.0))
    assert torch.equal(ub.cpu(), u.view(*dims, 1)[:, 5:6, :].cpu())
    rs = (20, 7, 11)      # a resampled grid
    assert torch.equal(m.decode_box(rs, start=(3, 0, 2), stop=(19, 7, 9)).cpu(), m.decode_grid(rs).view(*rs, 1)[3:19, :, 2:9].cpu())
    m2 = cls(coords_channel=2, features=20, data_channel=3, layers=3, output_act=True).to("cuda")      # 2-D
    f2 = m2.decode_grid((11, 19))
    assert torch.equal(m2.decode_box((11, 19), start=(2, 1), stop=(11, 19), step=(3, 2)).cpu(), f2.view(11, 19, 3)[2:11:3, 1:19:2].cpu())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fit_step_equals_fit_run_and_repeats(kind):
    dims = (8, 9, 10)
    vol = torch.rand(int(np.prod(dims)), 1, generator=torch.Generator().manual_seed(4)).cuda()
    out = []
    for mode in ("step", "run", "run"):
        torch.manual_seed(0)
        m = KINDS[kind](coords_channel=3, features=30, data_channel=1, layers=4).to("cuda")
        f = Fitter(m, vol, dims, sampler="randompoint", sample_size=500, optimizer="Adamax", lr=1e-3)
        if mode == "step":
            for _ in range(4):
                f.step()
        else:
            f.run(4)
        out.append(m.params.detach().cpu().clone())
    assert torch.equal(out[0], out[1]) and torch.equal(out[1], out[2])
    assert not torch.equal(out[0], KINDS[kind](coords_channel=3, features=30, data_channel=1, layers=4).params), "the fit moved the net"
