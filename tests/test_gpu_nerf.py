"""NeRF (positional-encoding net) on the fused HIP path, against the reference's own outputs (tests/golden/nerf.npz) and a float64
torch restatement of its module (utils/Networks.py:64-136).

The encoding is defined by the reference's fp32 phase: torch.sin((2 ** i) * math.pi * c) on a float32 tensor is the sine of the
exact float p_i = 2^i fl32(fl32(pi) x).  The restatements below take that phase and evaluate sin / cos and the MLP at `dtype`; bands are
a multiple of the distance between the float32 and the float64 restatement of the SAME case, measured in the test itself (as in
tests/test_gpu_ffn.py), plus a small floor relative to the magnitude of the quantity."""
import math

import numpy as np
import pytest
import torch

from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import NeRF
from tests._family_ref import BAND_FACTOR, FLOOR, band_check, encoding, phases, rand_coords, torch_loss, torch_nerf      # noqa: F401 (encoding: test_gpu_nerf_framework.py)

pytestmark = pytest.mark.gpu
ENC_BAND = 1e-6       # encoding vs the reference's fp32 PosEncodingNeRF, absolute (sin / cos within a few ulp of |v| <= 1)


def golden_band(got, gold, e32, scale, what):
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(gold, np.float64))))
    bound = (BAND_FACTOR + 1) * e32 + FLOOR * scale
    assert err <= bound, "%s: %.3e from the reference golden, bound %.3e (fp32 torch vs float64: %.3e)" % (what, err, bound, e32)


def probe_columns(cin, frequencies, x):
    """every encoding column as the kernel's first layer sees it: a layers = 2 net with W0 one-hot (+1 / -1) on column c, head [1, -1],
    zero biases, so y = relu(e_c) - relu(-e_c) = e_c exactly"""
    d = NeRF.encoding_width(cin, frequencies)
    m = NeRF(coords_channel=cin, data_channel=1, frequencies=frequencies, features=2, layers=2, skip=False).to("cuda")
    cols = []
    for c in range(d):
        w0 = torch.zeros(2, d)
        w0[0, c], w0[1, c] = 1.0, -1.0
        m.net[0][0].weight.data = w0
        m.net[0][0].bias.data = torch.zeros(2)
        m.net[1][0].weight.data = torch.tensor([[1.0, -1.0]])
        m.net[1][0].bias.data = torch.zeros(1)
        cols.append(m.forward(x.cuda()).cpu()[:, 0])
    return torch.stack(cols, 1).numpy()


@pytest.mark.parametrize("k", range(3))
def test_encoding_matches_the_reference(golden, k):
    g = golden("nerf")
    cin, Lf = (int(v) for v in g["enc%d_cfg" % k])
    x = torch.from_numpy(g["enc%d_x" % k])
    got = probe_columns(cin, Lf, x)
    ref = g["enc%d_y" % k]
    assert got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert err.max() <= ENC_BAND, "encoding: %.3e from the reference's fp32 PosEncodingNeRF (column %d)" % (err.max(), int(err.max(0).argmax()))
    assert np.array_equal(got[:, :cin], x.numpy()), "the coordinate columns pass through unchanged"
    if Lf >= 10:
        # the test tells the reference's phase from the mathematical 2^i pi x: at i = 9 they differ by far more than ENC_BAND
        c = cin + 2 * (9 * cin + 0)                 # sin(2^9 pi x_0)
        naive = torch.sin((2.0 ** 9) * math.pi * x[:, 0].double()).numpy()
        assert np.max(np.abs(naive - ref[:, c])) > 20 * ENC_BAND
        assert np.max(np.abs(naive - got[:, c])) > 20 * ENC_BAND


@pytest.mark.parametrize("k", range(10))
def test_forward_matches_reference_golden_and_float64(golden, k):
    g = golden("nerf")
    cin, cout, L, F, Lf, skip = (int(v) for v in g["fwd%d_cfg" % k])
    torch.manual_seed(int(g["fwd%d_seed" % k]))
    m = NeRF(coords_channel=cin, data_channel=cout, layers=L, features=F, frequencies=Lf, skip=bool(skip)).to("cuda")
    x = torch.from_numpy(g["fwd%d_x" % k])
    y = m.forward(x.cuda()).cpu().numpy()
    y64, _ = torch_nerf(m, x, torch.float64)
    y32, _ = torch_nerf(m, x, torch.float32)
    y64, y32 = y64.detach().numpy(), y32.detach().numpy()
    what = "forward %s" % ((cin, cout, L, F, Lf, skip),)
    band_check(y, y64, y32, what)
    golden_band(y, g["fwd%d_y" % k], float(np.max(np.abs(y32 - y64))), float(np.max(np.abs(g["fwd%d_y" % k]))), what + " vs golden")


@pytest.mark.parametrize("loss,weighted,thr", [("datal2", False, 0.0), ("datasmoothl1", True, 0.0), ("datal2", True, 0.3)])
@pytest.mark.parametrize("cin,cout,L,F,Lf,skip,n", [(3, 1, 5, 48, 10, True, 3000), (3, 1, 5, 167, 10, True, 2500), (2, 3, 3, 70, 4, True, 1111),
                                                    (3, 1, 4, 33, 0, False, 999), (3, 2, 6, 100, 16, True, 1200), (3, 1, 3, 507, 10, True, 700)])
def test_train_step_band(cin, cout, L, F, Lf, skip, n, loss, weighted, thr):
    torch.manual_seed(7)
    m = NeRF(coords_channel=cin, data_channel=cout, features=F, layers=L, frequencies=Lf, skip=skip).to("cuda")
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
        yh, ws = torch_nerf(m, x, dt)
        lt = torch_loss(yh, y.to(dt), w.to(dt), loss, thr, 0.05)
        lt.backward()
        res[dt] = (lt.item(), [t.grad.numpy() for t in ws])
    band_check([got_loss], [res[torch.float64][0]], [res[torch.float32][0]], "loss")
    d = NeRF.encoding_width(cin, Lf)
    off = 0
    for l, (o, i) in enumerate(m._shapes):      # every weight and bias tensor in its own band; the skip layer's two halves separately
        gw = got[off:off + o * i].reshape(o, i)
        r64, r32 = res[torch.float64][1][2 * l], res[torch.float32][1][2 * l]
        halves = [(slice(0, d), "encoding half"), (slice(d, i), "hidden half")] if l == m.skip_layer else [(slice(0, i), "")]
        for sl, tag in halves:
            band_check(gw[:, sl], r64[:, sl], r32[:, sl], "grad weight %d %s" % (l, tag))
        off += o * i
        band_check(got[off:off + o], res[torch.float64][1][2 * l + 1], res[torch.float32][1][2 * l + 1], "grad bias %d" % l)
        off += o
    assert off == m.param_count


def test_decode_grid_chunks_forward_and_box_equals_slice():
    torch.manual_seed(3)
    m = NeRF(coords_channel=3, data_channel=1, features=45, layers=5, frequencies=10, skip=True).to("cuda")
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
    m2 = NeRF(coords_channel=2, data_channel=3, features=20, layers=3, frequencies=4).to("cuda")      # 2-D
    f2 = m2.decode_grid((11, 19))
    assert torch.equal(m2.decode_box((11, 19), start=(2, 1), stop=(11, 19), step=(3, 2)).cpu(), f2.view(11, 19, 3)[2:11:3, 1:19:2].cpu())


def test_fit_step_equals_fit_run_and_repeats():
    dims = (8, 9, 10)
    vol = torch.rand(int(np.prod(dims)), 1, generator=torch.Generator().manual_seed(4)).cuda()
    out = []
    for mode in ("step", "run", "run"):
        torch.manual_seed(0)
        m = NeRF(coords_channel=3, data_channel=1, features=30, layers=4, frequencies=6).to("cuda")
        f = Fitter(m, vol, dims, sampler="randompoint", sample_size=500, optimizer="Adamax", lr=1e-3)
        if mode == "step":
            for _ in range(4):
                f.step()
        else:
            f.run(4)
        out.append(m.params.detach().cpu().clone())
    assert torch.equal(out[0], out[1]) and torch.equal(out[1], out[2])
