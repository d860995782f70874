"""SIREN_Pyramid / SIRENFT / SIRENPS on the fused HIP path (k_taper_fwd / k_taper_wgrad / k_taper_repack), against the reference's own
outputs (tests/golden/taper.npz, written by tests/golden/make_golden_taper.py) and a torch restatement of its module
(utils/Networks.py:316-552) written here.

The bands are SIREN's (tests/test_gpu_parity.py), because the arithmetic is SIREN's: with relerr(a, b) = max|a - b| / max|b|, forward
< 2e-5, loss < 1e-4, every parameter tensor's gradient, each on its own, < max(1e-4, 3 x own), `own` being the distance between the
torch fp32 and the torch float64 restatement of the same tensor.  At most 0.15 of the gradient comparisons may need 3 x own > 1e-4 and
none a band above 1e-3 (the cap of tests/_bands.py); test_band_widening_cap asserts that on the CPU over every case of this file."""
import functools
import json

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import SIREN, SIREN_Pyramid, SIRENFT, SIRENPS
from tests._family_ref import relerr, torch_loss, torch_taper

pytestmark = pytest.mark.gpu
KINDS = {"pyramid": SIREN_Pyramid, "ft": SIRENFT, "ps": SIRENPS}
NCASE = {"pyramid": 6, "ft": 5, "ps": 6}
CASES = [(k, i) for k in sorted(KINDS) for i in range(NCASE[k])]
LOSSES = [("datal2", False, 0.0), ("datasmoothl1", True, 0.0), ("datal2", True, 0.3)]
FWD_TOL, LOSS_TOL, GRAD_TOL = 2e-5, 1e-4, 1e-4
MAX_WIDENED_FRACTION, MAX_BAND = 0.15, 1e-3      # tests/_bands.py


def build(golden, kind, i, device="cuda"):
    g = golden("taper")
    cfg = json.loads(str(g["%s_fwd%d_cfg" % (kind, i)]))
    torch.manual_seed(int(g["%s_fwd%d_seed" % (kind, i)]))
    m = KINDS[kind](**cfg)
    assert m.widths == [int(v) for v in g["%s_fwd%d_widths" % (kind, i)]]
    return (m.to(device) if device else m), cfg, g


def batch(m, seed=7):
    """uniform random coordinates, targets and weights; n between 300 and 2 000, smaller for the wide nets"""
    n = 300 if max(m.widths) > 512 else (800 if max(m.widths) > 128 else 2000)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, m.coords_channel, generator=gen) * 2 - 1
    y = torch.rand(n, m.data_channel, generator=gen)
    w = torch.rand(n, m.data_channel, generator=gen) * 3 + 0.5
    return n, x, y, w


_TORCH = {}


def torch_step(golden, kind, i, li):
    """loss and per-tensor gradients of the torch restatement in float32 and float64 (CPU; cached: the cap test and the GPU test share it)"""
    key = (kind, i, li)
    if key not in _TORCH:
        m, _, _ = build(golden, kind, i, device=None)
        loss, weighted, thr = LOSSES[li]
        n, x, y, w = batch(m)
        if not weighted:
            w = torch.ones_like(w)
        res = {}
        for dt in (torch.float64, torch.float32):
            yh, leaves = torch_taper(m, x, dt)
            lt = torch_loss(yh, y.to(dt), w.to(dt), loss, thr, 0.05)
            lt.backward()
            res[dt] = (lt.item(), [v.grad.numpy().astype(np.float64) for v in leaves])
        _TORCH[key] = res
    return _TORCH[key]


@pytest.mark.parametrize("kind,i", CASES)
def test_forward_matches_reference_golden_and_torch(golden, kind, i):
    m, cfg, g = build(golden, kind, i)
    x = torch.from_numpy(g["%s_fwd%d_x" % (kind, i)])
    y = m.forward(x.cuda()).cpu().numpy()
    gold = g["%s_fwd%d_y" % (kind, i)]
    y32, _ = torch_taper(m, x, torch.float32)
    e_gold, e_torch = relerr(y, gold), relerr(y, y32.detach().numpy())
    print("forward %s %s widths %s: vs golden %.2e, vs torch fp32 %.2e" % (kind, i, m.widths, e_gold, e_torch))
    assert e_gold < FWD_TOL and e_torch < FWD_TOL


@pytest.mark.parametrize("li", range(len(LOSSES)))
@pytest.mark.parametrize("kind,i", CASES)
def test_train_step_band(golden, kind, i, li):
    m, cfg, g = build(golden, kind, i)
    loss, weighted, thr = LOSSES[li]
    n, x, y, w = batch(m)
    lo, _ = m.train_step(n, y.cuda().contiguous(), coords=x.cuda().contiguous(), weights=w.cuda().contiguous() if weighted else None,
                         loss=loss, thr=thr, beta=0.05)
    got_loss, got = lo.item(), m.grads.cpu().numpy()
    res = torch_step(golden, kind, i, li)
    l32, g32 = res[torch.float32]
    _, g64 = res[torch.float64]
    e_loss = abs(got_loss - l32) / abs(l32)
    print("train %s %s widths %s %s: loss %.2e" % (kind, i, m.widths, LOSSES[li], e_loss))
    assert e_loss < LOSS_TOL
    off = 0
    for j, (a, b) in enumerate(zip(g32, g64)):
        own = relerr(a, b)
        tol = max(GRAD_TOL, 3.0 * own)
        e = relerr(got[off:off + a.size], a.reshape(-1))
        print("  tensor %d %s: hip vs torch fp32 %.2e, own %.2e, band %.1e" % (j, a.shape, e, own, tol))
        assert e < tol, "gradient of tensor %d %s: %.3e, band %.3e (own %.3e)" % (j, a.shape, e, tol, own)
        off += a.size
    assert off == m.param_count


def test_band_widening_cap(golden):
    """`own` involves no GPU: over every gradient comparison of test_train_step_band at most 0.15 need a band above 1e-4, none above 1e-3"""
    total = widened = 0
    worst = 0.0
    for kind, i in CASES:
        for li in range(len(LOSSES)):
            res = torch_step(golden, kind, i, li)
            for a, b in zip(res[torch.float32][1], res[torch.float64][1]):
                own = relerr(a, b)
                total += 1
                widened += 3.0 * own > GRAD_TOL
                worst = max(worst, 3.0 * own)
    print("gradient comparisons %d, widened %d, widest band %.2e" % (total, widened, max(worst, GRAD_TOL)))
    assert widened <= MAX_WIDENED_FRACTION * total and worst <= MAX_BAND


@pytest.mark.parametrize("F", [31, 64, 256])
def test_flat_pyramid_and_siren_kernels_agree_with_the_same_torch_result(F):
    """SIREN_Pyramid(features_dis=0) is a SIREN: both kernel families, on the same weights, are inside the bands of one torch result
    (not bitwise: the summation order differs)"""
    torch.manual_seed(11)
    p = SIREN_Pyramid(coords_channel=3, data_channel=1, features=F, layers=5, w0=20, features_dis=0)
    torch.manual_seed(11)
    s = SIREN(coords_channel=3, data_channel=1, features=F, layers=5, w0=20)
    assert torch.equal(p.params, s.params)
    p.to("cuda"), s.to("cuda")
    n, x, y, w = batch(p)
    yh, leaves = torch_taper(p, x, torch.float32)
    lt = torch_loss(yh, y, torch.ones_like(y), "datal2", 0.0, 0.05)
    lt.backward()
    yh64, leaves64 = torch_taper(p, x, torch.float64)
    torch_loss(yh64, y.double(), torch.ones_like(y).double(), "datal2", 0.0, 0.05).backward()
    for m in (p, s):
        assert relerr(m.forward(x.cuda()).cpu().numpy(), yh.detach().numpy()) < FWD_TOL
        lo, _ = m.train_step(n, y.cuda().contiguous(), coords=x.cuda().contiguous())
        assert abs(lo.item() - lt.item()) / lt.item() < LOSS_TOL
        got, off = m.grads.cpu().numpy(), 0
        for v, v64 in zip(leaves, leaves64):
            a = v.grad.numpy()
            tol = max(GRAD_TOL, 3.0 * relerr(a, v64.grad.numpy()))
            assert relerr(got[off:off + a.size], a.reshape(-1)) < tol, (type(m).__name__, tuple(a.shape))
            off += a.size


def _pad32(w):
    return (w + 31) // 32 * 32


def test_work_follows_the_widths():
    """the packed copy and the train workspace are sized by every layer's own width, not by the widest layer"""
    L = _lib.lib()
    for cls, kw_, n in ((SIRENPS, dict(features=125.45368822738716, ratio=1.5), 100000), (SIREN_Pyramid, dict(features=271, features_dis=10), 5000),
                        (SIRENFT, dict(features=43.936769251345325, ratio=2), 1000), (SIRENPS, dict(features=64, ratio=2, layers=6, data_channel=2), 777)):
        m = cls(**{"coords_channel": 3, "data_channel": 1, "layers": 5, "w0": 20, **kw_})
        bound = sum(2 * _pad32(o) * _pad32(i) for o, i in m._shapes) + 64 * sum(_pad32(o) for o, _ in m._shapes)
        assert 0 < L.brief_taper_packed_count(_lib.C.byref(m.desc)) <= bound, m.widths
    taper = SIRENPS(coords_channel=3, data_channel=1, layers=5, w0=20, features=125.45368822738716, ratio=1.5)
    flat = SIREN_Pyramid(coords_channel=3, data_channel=1, layers=5, w0=20, features=423, features_dis=0)
    assert taper.widths == [423, 282, 188, 125] and flat.widths == [423] * 4
    pt, pf = (L.brief_taper_packed_count(_lib.C.byref(m.desc)) for m in (taper, flat))
    assert pt < 0.45e6 * 1.05 and pf > 1.1e6
    for n in (1000, 100000):
        wt, wf = (L.brief_taper_train_workspace_bytes(_lib.C.byref(m.desc), n) for m in (taper, flat))
        assert wf - wt >= (4 * 448 - (448 + 288 + 192 + 128)) * n * 4, (n, wt, wf)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_decode_grid_chunks_forward_and_box_equals_slice(kind):
    cls = KINDS[kind]
    extra = {"pyramid": dict(features=45, features_dis=7), "ft": dict(features=30.5, ratio=2), "ps": dict(features=14.2, ratio=1.5)}[kind]
    torch.manual_seed(3)
    m = cls(coords_channel=3, data_channel=1, layers=5, w0=20, **extra).to("cuda")
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
    u = m.decode_grid(dims, out_kind="u16", scale=(0.0, 1.0), vrange=(0.0, 65535.0))
    assert u.cpu().to(torch.int32).unique().numel() > 10
    ub = m.decode_box(dims, start=(0, 5, 0), stop=(9, 6, 17), out_kind="u16", scale=(0.0, 1.0), vrange=(0.0, 65535.0))
    assert torch.equal(ub.cpu(), u.view(*dims, 1)[:, 5:6, :].cpu())
    us = m.decode_box(dims, start=(1, 0, 2), stop=(9, 13, 17), step=(3, 2, 4), out_kind="u16", scale=(0.0, 1.0), vrange=(0.0, 65535.0))
    assert torch.equal(us.cpu(), u.view(*dims, 1)[1:9:3, 0:13:2, 2:17:4].cpu())
    rs = (20, 7, 11)      # a resampled grid
    assert torch.equal(m.decode_box(rs, start=(3, 0, 2), stop=(19, 7, 9)).cpu(), m.decode_grid(rs).view(*rs, 1)[3:19, :, 2:9].cpu())
    m2 = cls(coords_channel=2, data_channel=3, layers=3, w0=20, output_act=True, **extra).to("cuda")      # 2-D
    f2 = m2.decode_grid((11, 19))
    assert torch.equal(m2.decode_box((11, 19), start=(2, 1), stop=(11, 19), step=(3, 2)).cpu(), f2.view(11, 19, 3)[2:11:3, 1:19:2].cpu())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_train_step_is_deterministic_and_batch_split_linear(kind):
    """two launches give identical bits (no float atomics), and the gradient of a batch is the count-weighted sum of the gradients
    of its two halves"""
    extra = {"pyramid": dict(features=271, features_dis=10), "ft": dict(features=100.3, ratio=2), "ps": dict(features=60.5, ratio=1.5)}[kind]
    torch.manual_seed(5)
    m = KINDS[kind](coords_channel=3, data_channel=1, layers=5, w0=20, **extra).to("cuda")
    n = 20000
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.uniform(0, 1, size=(n, 1)).astype(np.float32)).cuda()
    l1, _ = m.train_step(n, y, coords=x)
    g1 = m.grads.clone()
    l2, _ = m.train_step(n, y, coords=x)
    assert torch.equal(g1, m.grads) and l1.item() == l2.item()
    h = 12000
    m.train_step(h, y[:h].contiguous(), coords=x[:h].contiguous())
    ga = m.grads.clone().double()
    m.train_step(n - h, y[h:].contiguous(), coords=x[h:].contiguous())
    gb = m.grads.clone().double()
    comb = (ga * h + gb * (n - h)) / n
    assert relerr(comb.cpu().numpy(), g1.double().cpu().numpy()) < 2e-5


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fit_step_equals_fit_run_and_repeats(kind):
    extra = {"pyramid": dict(features=40, features_dis=5), "ft": dict(features=20.5, ratio=2), "ps": dict(features=14.2, ratio=1.5)}[kind]
    dims = (8, 9, 10)
    vol = torch.rand(int(np.prod(dims)), 1, generator=torch.Generator().manual_seed(4)).cuda()
    out = []
    for mode in ("step", "run", "run"):
        torch.manual_seed(0)
        m = KINDS[kind](coords_channel=3, data_channel=1, layers=4, w0=20, **extra).to("cuda")
        f = Fitter(m, vol, dims, sampler="randompoint", sample_size=500, optimizer="Adamax", lr=1e-3)
        if mode == "step":
            for _ in range(4):
                f.step()
        else:
            f.run(4)
        out.append(m.params.detach().cpu().clone())
    assert torch.equal(out[0], out[1]) and torch.equal(out[1], out[2])
    torch.manual_seed(0)
    assert not torch.equal(out[0], KINDS[kind](coords_channel=3, data_channel=1, layers=4, w0=20, **extra).params), "the fit moved the net"
