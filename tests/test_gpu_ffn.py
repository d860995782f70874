"""FFN (Fourier-feature net) on the fused HIP path, against a float64 torch restatement of the reference's module
(utils/Networks.py:138-207).

Bands: the kernels run fp32 with the embedding phase t = x . B in revolutions (|B| ~ 41 at scale 10, so |t| ~ 120 revolutions and
the fp32 rounding of t alone is ~5e-5 rad, which the reference's own fp32 module has too).  Every band below is therefore stated as
a multiple of the distance between the float32 and the float64 torch restatement of the SAME case, measured in the test itself:
the fused path must be no further from float64 than BAND_FACTOR times what plain fp32 torch gets, plus a small floor relative to
the magnitude of the quantity."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import FFN, init_phi
from tests._family_ref import BAND_FACTOR, FLOOR, band_check, rand_coords, torch_ffn, torch_loss      # noqa: F401 (BAND_FACTOR, FLOOR: test_gpu_ffn_framework.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FWD_CASES = [
    # (cin, cout, layers, features, embsize, n)
    (3, 1, 5, 2, 256, 1000),
    (3, 1, 5, 21, 256, 4133),
    (3, 1, 5, 119, 256, 3001),
    (2, 3, 3, 256, 16, 2048),
    (3, 3, 5, 449, 256, 1500),
    (3, 1, 2, 1024, 512, 777),
    (2, 1, 3, 100, 512, 999),
    (3, 2, 3, 33, 17, 65),
]


@pytest.mark.parametrize("cin,cout,L,F,E,n", FWD_CASES)
def test_forward_band(cin, cout, L, F, E, n):
    torch.manual_seed(cin * 1000 + F)
    m = FFN(coords_channel=cin, data_channel=cout, features=F, layers=L, embsize=E).to("cuda")
    x = rand_coords(n, cin, F)
    y = m.forward(x.cuda()).cpu()
    y64, _ = torch_ffn(m, x, torch.float64)
    y32, _ = torch_ffn(m, x, torch.float32)
    assert y.shape == (n, cout)
    band_check(y.numpy(), y64.detach().numpy(), y32.detach().numpy(), "forward %s" % ((cin, cout, L, F, E),))


@pytest.mark.parametrize("loss,weighted,thr", [("datal2", False, 0.0), ("datasmoothl1", True, 0.0), ("datal2", True, 0.3)])
@pytest.mark.parametrize("cin,cout,L,F,E,n", [(3, 1, 5, 21, 256, 3000), (3, 1, 5, 119, 256, 2500), (2, 3, 3, 70, 40, 1111),
                                               (3, 1, 3, 449, 256, 1200)])
def test_train_step_band(cin, cout, L, F, E, n, loss, weighted, thr):
    torch.manual_seed(7)
    m = FFN(coords_channel=cin, data_channel=cout, features=F, layers=L, embsize=E).to("cuda")
    x = rand_coords(n, cin, 11)
    g = torch.Generator().manual_seed(5)
    y = torch.rand(n, cout, generator=g)
    w = (torch.rand(n, cout, generator=g) * 3 + 0.5) if weighted else torch.ones(n, cout)
    bv0 = m.params[:m.bv_count].clone()
    lo, _ = m.train_step(n, y.cuda().contiguous(), coords=x.cuda().contiguous(), weights=w.cuda().contiguous() if weighted else None,
                         loss=loss, thr=thr, beta=0.05)
    got_loss = lo.item()
    got = m.grads.cpu().numpy()
    res = {}
    for dt in (torch.float64, torch.float32):
        yh, ws = torch_ffn(m, x, dt)
        lt = torch_loss(yh, y.to(dt), w.to(dt), loss, thr, 0.05)
        lt.backward()
        res[dt] = (lt.item(), np.concatenate([np.zeros(m.bv_count)] + [t.grad.numpy().reshape(-1) for t in ws]))
    band_check([got_loss], [res[torch.float64][0]], [res[torch.float32][0]], "loss")
    assert np.all(got[:m.bv_count] == 0.0), "bvals gets no gradient"
    off = m.bv_count
    for l, (o, i) in enumerate(m._shapes):      # every weight and bias tensor in its own band: a small layer cannot hide behind a large one
        for what, cnt in (("weight", o * i), ("bias", o)):
            band_check(got[off:off + cnt], res[torch.float64][1][off:off + cnt], res[torch.float32][1][off:off + cnt], "grad %s %d" % (what, l))
            off += cnt
    assert torch.equal(m.params[:m.bv_count], bv0)


def test_decode_grid_equals_forward_and_box_equals_slice():
    torch.manual_seed(3)
    m = FFN(coords_channel=3, data_channel=1, features=45, layers=4, embsize=64).to("cuda")
    dims = (9, 13, 17)
    full = m.decode_grid(dims)
    lin = [torch.linspace(-1, 1, d) for d in dims]
    coords = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3)
    assert torch.equal(full.cpu(), m.forward(coords.cuda()).cpu())
    box = m.decode_box(dims, start=(1, 2, 3), stop=(8, 12, 16), step=(2, 3, 1))
    assert torch.equal(box.cpu(), full.view(*dims, 1)[1:8:2, 2:12:3, 3:16].cpu())
    u = m.decode_grid(dims, out_kind="u16", scale=(0.0, 100.0), vrange=(0.0, 65535.0))
    ub = m.decode_box(dims, start=(0, 5, 0), stop=(9, 6, 17), out_kind="u16", scale=(0.0, 100.0), vrange=(0.0, 65535.0))
    assert torch.equal(ub.cpu(), u.view(*dims, 1)[:, 5:6, :].cpu())
    rs = (20, 7, 11)      # a resampled grid
    assert torch.equal(m.decode_box(rs, start=(3, 0, 2), stop=(19, 7, 9)).cpu(), m.decode_grid(rs).view(*rs, 1)[3:19, :, 2:9].cpu())


@pytest.mark.parametrize("opt,sched", [("Adamax", {"name": "MultiStepLR", "milestones": [3, 5], "gamma": 0.5}),
                                       ("Adam", {"name": "StepLR", "step_size": 2, "gamma": 0.7}),
                                       ("SGD", {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 1e-2, "step_size_up": 3})])
def test_fit_matches_torch_and_repeats(opt, sched):
    dims = (10, 12, 14)
    g = torch.Generator().manual_seed(2)
    vol = torch.rand(int(np.prod(dims)), 1, generator=g).cuda()
    runs = []
    for rep in range(2):
        torch.manual_seed(0)
        m = FFN(coords_channel=3, data_channel=1, features=37, layers=4, embsize=32).to("cuda")
        p0 = m.params.detach().cpu().clone()
        f = Fitter(m, vol, dims, sampler="full", optimizer=opt, lr=1e-3, scheduler=sched)
        losses = f.run(7, log=True).cpu().numpy()
        runs.append((m.params.detach().cpu().clone(), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0][:m.bv_count], p0[:m.bv_count]), "bvals is not optimised"
    # the same steps in float64 torch (full batch, torch optimizers and schedulers)
    lin = [torch.linspace(-1, 1, d) for d in dims]
    x = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3).double()
    y = vol.cpu().double()
    P = p0.double()
    E, cin = 32, 3
    B = P[:E * cin].view(E, cin)
    shapes = [(37, 64), (37, 37), (37, 37), (1, 37)]
    ws, off = [], E * cin
    for (o, i) in shapes:
        ws += [P[off:off + o * i].view(o, i).clone().requires_grad_(True), P[off + o * i:off + o * i + o].clone().requires_grad_(True)]
        off += o * i + o
    o_ = {"Adamax": torch.optim.Adamax, "Adam": torch.optim.Adam, "SGD": torch.optim.SGD}[opt](ws, lr=1e-3)
    s = dict(sched)
    name = s.pop("name")
    if name == "CyclicLR":
        s["cycle_momentum"] = False
    sch = getattr(torch.optim.lr_scheduler, name)(o_, **s)
    t = (2 * math.pi * x) @ B.T
    emb = torch.cat([torch.sin(t), torch.cos(t)], -1)
    ref_losses = []
    for _ in range(7):
        o_.zero_grad()
        h = emb
        for l in range(4):
            h = h @ ws[2 * l].T + ws[2 * l + 1]
            if l < 3:
                h = torch.relu(h)
        lt = ((h - y) ** 2).mean()
        lt.backward()
        ref_losses.append(lt.item())
        o_.step()
        sch.step()
    final = torch.cat([B.reshape(-1)] + [w.detach().reshape(-1) for w in ws])
    got = runs[0][0].double()
    # 7 optimizer steps of lr <= 1e-2: the trajectories agree to the fp32 gradient spread times the steps taken
    assert np.max(np.abs(runs[0][1] - np.array(ref_losses))) <= 1e-4 * max(ref_losses)
    assert torch.max(torch.abs(got - final)).item() <= 1e-4


def test_fit_step_equals_fit_run():
    dims = (8, 9, 10)
    vol = torch.rand(int(np.prod(dims)), 1, generator=torch.Generator().manual_seed(4)).cuda()
    out = []
    for mode in ("step", "run"):
        torch.manual_seed(0)
        m = FFN(coords_channel=3, data_channel=1, features=30, layers=3, embsize=20).to("cuda")
        f = Fitter(m, vol, dims, sampler="randompoint", sample_size=500, optimizer="Adamax", lr=1e-3)
        if mode == "step":
            for _ in range(4):
                f.step()
        else:
            f.run(4)
        out.append(m.params.detach().cpu().clone())
    assert torch.equal(out[0], out[1])


def test_refusals():
    with pytest.raises(NotImplementedError, match="skip"):
        FFN(skip=True)
    with pytest.raises(NotImplementedError, match="1..1024"):
        FFN(features=1412)
    with pytest.raises(NotImplementedError, match="1..512"):
        FFN(embsize=513)
    with pytest.raises(NotImplementedError):
        init_phi({"name": "NeRF"})
