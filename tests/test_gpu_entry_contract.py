"""Three parts of the C-ABI contract that every kernel implements in its own copy of the code, on every kernel variant of
tests/_variants.py (the row id names the kernel reached): k_fused<1 / 4 / 8 / 12>, k_small, k_lean, k_wide, the bf16 and bf16x3 kernels,
k_ffn_*, k_nerf_*, both k_mfn_* filters and k_taper_*.

A, B  the integer epilogue (BRIEF_OUT_U8 / BRIEF_OUT_U16: subtract, divide, clip, multiply, add, truncate) against the oracle's epilogue,
      bit for bit: on a ragged 2^18-voxel grid with a window that clips 15 % of the samples on each side, and at chosen inputs: the
      clip edges and inputs whose pre-truncation float is the largest float32 below an integer.  The kernel's own f32 decode is only the
      epilogue's INPUT here (the forward tests hold it to float64); tests/test_entry_contract_host.py shows on the CPU that these parameter
      sets tell a reciprocal multiply, a fused multiply-add, double arithmetic and round-to-nearest from the right epilogue.
C     one batch named in every way a batch can be named (explicit coords / idx + coords / grid + idx / grid + offset / the in-kernel
      Philox stream) gives the same loss, yhat and gradients bit for bit: every kernel is bit-reproducible and the coordinates are the
      same bits.
D     BRIEF_LOSS_EXTERNAL: dL/dyhat formed on the host in the kernels' own order of operations gives the L2 step's gradient buffer bit
      for bit, a loss of exactly 0 and the same yhat; and the autograd route (requires_grad_(True), a torch MSE, backward()) lands within
      the project's gradient band (1e-4 of every parameter tensor's max-abs) of the fused L2 step.

Nothing here is a new band: the bitwise comparisons have exact expected results, the two band checks use the project's forward bands
(2e-5; 3e-2 for bf16) and its gradient band.  The printed lines (ENTRY-CONTRACT ...) are the measurements of profiles/r14_entry_contract.md."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from oracle import oracle as O

from . import _variants as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 67                     # elements on each side of an output: the view's pointer is then not 16-byte aligned for f32, u16 or u8
ALL = pytest.mark.parametrize("v", V.VARIANTS, ids=[v.label for v in V.VARIANTS])


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


# ---- outputs between guards
def _pattern(count, kind):
    """guard fill: values no decode writes (f32: below -7e4; u16 / u8: outside the value range), and not one value repeated"""
    i = np.arange(count)
    if kind == "f32":
        return (-(70000.0 + (i % 977))).astype(np.float32)
    if kind == "u16":
        return (60000 + (i * 13) % 4999).astype(np.uint16)
    return np.array([0, 1, 2, 251, 252, 253, 254, 255], np.uint8)[i % 8]


class _Guarded:
    """a buffer of GUARD + count + GUARD elements filled with the pattern; `.view` is the middle"""

    def __init__(self, count, kind):
        self.count, self.pat = count, _pattern(count + 2 * GUARD, kind)
        self.buf = torch.from_numpy(self.pat.copy()).to(DEV)
        self.view = self.buf[GUARD:GUARD + count]
        assert self.view.data_ptr() % 16 != 0

    def result(self):
        """the middle as numpy, after checking that both guards still hold the pattern"""
        got = self.buf.cpu().numpy()
        assert np.array_equal(got[:GUARD], self.pat[:GUARD]), "the guard in front of the output was written"
        assert np.array_equal(got[GUARD + self.count:], self.pat[GUARD + self.count:]), "the guard behind the output was written"
        return got[GUARD:GUARD + self.count]


def _decode(m, dims, kind, scale=(0.0, 100.0), offset=0, count=None):
    total = int(np.prod(dims)) - offset if count is None else count
    g = _Guarded(total * m.data_channel, kind)
    vr = V.VRANGE.get(kind, (0.0, 1.0))
    m.decode_grid(dims, offset=offset, count=total, out=g.view.view(total, m.data_channel), out_kind=kind, scale=scale, vrange=vr)
    return g.result().reshape(total, m.data_channel)


# ---- A: the integer decodes of a ragged grid against the oracle's epilogue
@ALL
def test_integer_decode_equals_the_oracle_epilogue(v):
    m = v.make(DEV)
    dims = (61, 67, 65) if v.cin == 3 else (509, 521)
    box = ((3, 5, 2), (58, 60, 63), (2, 3, 4)) if v.cin == 3 else ((5, 7), (500, 515), (3, 2))
    f32 = _decode(m, dims, "f32")
    assert np.isfinite(f32).all()
    q15, q85 = (np.float32(q) for q in np.quantile(f32.astype(np.float64), [0.15, 0.85]))
    scale = (float(q15), float(q85))
    den = np.float32(np.float64(q85) - np.float64(q15))
    lo, hi, inside = int((f32 < q15).sum()), int((f32 > q85).sum()), int(((f32 > q15) & (f32 < q85)).sum())
    print("ENTRY-CONTRACT A %-6s samples %d window (%.7g, %.7g) clipped below %d above %d strictly inside %d" % (v.id, f32.size, q15, q85, lo, hi, inside))
    # conditions that keep the case from going vacuous (not measurements)
    assert den > 0 and not V.is_power_of_two(den)
    assert lo >= 0.05 * f32.size and hi >= 0.05 * f32.size
    assert inside >= 150000
    ints = {}
    for kind in ("u16", "u8"):
        ints[kind] = _decode(m, dims, kind, scale)
        ref = O.invnormalize(f32, V.SIDE[kind], *scale)
        bad = int((ints[kind] != ref).sum())
        assert bad == 0, "%s: %d of %d samples differ from the oracle's epilogue" % (kind, bad, ref.size)
    # a strided box in ragged chunks is the slice of the grid decode
    start, stop, step = box
    sl = tuple(slice(a, b, s) for a, b, s in zip(start, stop, step))
    want = ints["u16"].reshape(*dims, v.cout)[sl]
    g = _Guarded(want.size, "u16")
    out = m.decode_box(dims, start, stop, step, out_kind="u16", scale=scale, vrange=V.VRANGE["u16"], out=g.view, chunk=4001)
    assert out.data_ptr() == g.view.data_ptr() and want.shape[:-1] == tuple(len(range(a, b, s)) for a, b, s in zip(start, stop, step))
    assert np.array_equal(g.result(), want.reshape(-1))


# ---- B: exact values at the clip edges and at truncation
@pytest.fixture(scope="module")
def edges():
    e = {k: V.edge_values(k) for k in ("u16", "u8")}
    vals = np.concatenate([e["u16"]["clip_lo"], e["u16"]["clip_hi"]] + [e[k][w] for k in ("u16", "u8") for w in ("below", "at")]).astype(np.float32)
    assert len(vals) >= 22 and not np.isnan(vals).any()
    return vals


NO_ACT = [v for v in V.VARIANTS if not v.output_act]


@pytest.mark.parametrize("v", NO_ACT, ids=[v.label for v in NO_ACT])
def test_epilogue_at_the_clip_edges_and_at_truncation(v, edges):
    """every parameter zero and the head bias b: every kernel returns b exactly, so the epilogue sees chosen inputs (scale (0, 100))"""
    m = v.make(DEV)
    for _, pv in V.param_views(m):
        pv.data = torch.zeros(pv.shape)
    assert not m.params.any() and m._stale
    dims, n = ((4, 3, 3) if v.cin == 3 else (6, 6)), 33
    smin, smax = np.float32(0.0), np.float32(100.0)
    for i in range(0, len(edges), v.cout):
        b = np.resize(edges[i:i + v.cout], v.cout)          # (a short last group repeats its values)
        V.head_bias(m).data = torch.from_numpy(b.copy())
        assert m._stale
        f32 = _decode(m, dims, "f32", count=n)
        assert np.array_equal(f32.view(np.int32), np.broadcast_to(b.view(np.int32), (n, v.cout))), (b, f32[0])
        for kind in ("u16", "u8"):
            got = _decode(m, dims, kind, (0.0, 100.0), count=n)
            ref = O.invnormalize(np.broadcast_to(b, (n, v.cout)), V.SIDE[kind])
            assert np.array_equal(got, ref), (kind, b, got[0], ref[0])
            vmin, vmax = V.VRANGE[kind]
            for c in range(v.cout):
                if b[c] <= smin:
                    assert (got[:, c] == vmin).all(), (kind, b[c])
                if b[c] >= smax:
                    assert (got[:, c] == vmax).all(), (kind, b[c])


# ---- C, D: one batch, every way of naming it; the external loss
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _step(m, n, **kw):
    loss, yhat = m.train_step(n, want_yhat=True, **kw)
    return loss.clone(), yhat, m.grads.clone()


def _same(a, b, what):
    for name, x, y in zip(("loss", "yhat", "gradient buffer"), a, b):
        assert not torch.isnan(x).any(), (what, name)
        assert torch.equal(x, y), "%s: %s differs in %d of %d elements" % (what, name, int((x != y).sum()), x.numel())


class _Pools:
    """a seeded volume of targets and weights in {0.25, 1} on a small ragged grid, and the oracle's coordinates of it"""

    def __init__(self, v, seed):
        self.rng = np.random.default_rng(seed)
        self.dims = (13, 17, 19) if v.cin == 3 else (53, 79)
        self.pop = int(np.prod(self.dims))
        self.coords = O.grid_coords(self.dims)
        self.targets, self.weights = self.draw(self.pop, v.cout)
        self.grid = (self.dims, -1.0, 1.0)
        self.t_dev, self.w_dev = _dev(self.targets), _dev(self.weights)

    def draw(self, rows, cout):
        y = self.rng.uniform(0, 100, size=(rows, cout)).astype(np.float32)
        w = np.where(self.rng.uniform(size=(rows, cout)) < 0.5, 0.25, 1.0).astype(np.float32)
        return y, w


def _thr(m, x):
    """a threshold both sides of which hold samples: the median of the net's output on the batch"""
    fwd = m.forward(_dev(x)).cpu().numpy()
    thr = float(np.median(fwd))
    assert thr != 0.0 and (fwd <= thr).any() and (fwd > thr).any()
    return thr, fwd


def _base(v, m, n, x, y, w):
    """the step that names the batch with explicit coords, targets and weights"""
    thr, fwd = _thr(m, x)
    base = _step(m, n, coords=_dev(x), targets=_dev(y), weights=_dev(w), thr=thr)
    yh = base[1].cpu().numpy()
    dist = relerr(yh, fwd)
    assert dist < v.band, dist
    assert (yh <= thr).any() and (yh > thr).any() and base[2].abs().max() > 0
    return base, thr, dist


CD_CASES = [(v, 1531) for v in V.VARIANTS] + [(V.BY_ID[i], 29) for i in ("s22", "s300", "b96", "mfng")]      # (n % 32 != 0; some below one tile)
CD = pytest.mark.parametrize("v,n", CD_CASES, ids=["%s-n%d" % (v.label, n) for v, n in CD_CASES])


@CD
def test_one_batch_named_every_way(v, n):
    m = v.make(DEV)
    p = _Pools(v, 100 + v.seed)
    rng = p.rng
    # (i) idx + coords: the batch's rows scattered over pools of 4099 rows
    x = rng.uniform(-1, 1, size=(n, v.cin)).astype(np.float32)
    y, w = p.draw(n, v.cout)
    base, thr, d1 = _base(v, m, n, x, y, w)
    rows = 4099
    cpool = rng.uniform(-1, 1, size=(rows, v.cin)).astype(np.float32)
    tpool, wpool = p.draw(rows, v.cout)
    pos = rng.permutation(rows)[:n].astype(np.int64)
    cpool[pos], tpool[pos], wpool[pos] = x, y, w
    _same(base, _step(m, n, idx=_dev(pos), coords=_dev(cpool), targets=_dev(tpool), weights=_dev(wpool), thr=thr), "idx + coords")
    # (ii) grid + idx: whole-volume pools of targets and weights
    idx = rng.integers(0, p.pop, size=n).astype(np.int64)
    base, thr, d2 = _base(v, m, n, p.coords[idx], p.targets[idx], p.weights[idx])
    _same(base, _step(m, n, idx=_dev(idx), grid=p.grid, targets=p.t_dev, weights=p.w_dev, thr=thr), "grid + idx")
    # (iii) grid + offset: a run that starts off a tile boundary
    off = 1003
    assert off % 32 != 0 and off + n <= p.pop
    base, thr, d3 = _base(v, m, n, p.coords[off:off + n], p.targets[off:off + n], p.weights[off:off + n])
    _same(base, _step(m, n, grid=p.grid, offset=off, targets=p.t_dev, weights=p.w_dev, thr=thr), "grid + offset")
    print("ENTRY-CONTRACT C %-6s n %-5d yhat against forward(): %.2e (band %.0e)" % (v.id, n, max(d1, d2, d3), v.band))


@CD
def test_in_kernel_philox_stream_is_the_index_kernels(v, n):
    """two fit_step(rng=(pop, seed, t)) steps equal two fit_step(idx=...) steps on the indices brief_sample_indices writes"""
    p = _Pools(v, 200 + v.seed)
    ma, mb = v.make(DEV), v.make(DEV)
    p0 = ma.params.clone()
    assert torch.equal(p0, mb.params)
    sa1, sa2, sb1, sb2 = (torch.zeros_like(ma.params) for _ in range(4))
    idx = torch.empty(n, dtype=torch.int64, device=DEV)
    for t in (1, 2):
        _lib.check(_lib.lib().brief_sample_indices(_lib.ptr(idx), n, p.pop, 99, t, _lib.stream_ptr()))
        la = ma.fit_step(n, p.t_dev, 0, sa1, sa2, 1e-3, t, idx=idx, weights=p.w_dev, grid=p.grid).clone()
        lb = mb.fit_step(n, p.t_dev, 0, sb1, sb2, 1e-3, t, weights=p.w_dev, grid=p.grid, rng=(p.pop, 99, t))
        assert not torch.isnan(la).any() and torch.equal(la, lb), (t, la.item(), lb.item())
        assert torch.equal(ma.params, mb.params) and torch.equal(sa1, sb1) and torch.equal(sa2, sb2), t
        assert torch.equal(ma.grads, mb.grads) and torch.equal(ma.packed, mb.packed), t
    assert not torch.equal(ma.params, p0) and 0 <= int(idx.min()) and int(idx.max()) < p.pop


@CD
def test_external_loss_equals_the_l2_step(v, n):
    """g = ((2 (yhat - y)) we) inv_count in float32, the kernels' own expression (built with -ffp-contract=off), handed back as
    BRIEF_LOSS_EXTERNAL targets"""
    m = v.make(DEV)
    p = _Pools(v, 300 + v.seed)
    x = p.rng.uniform(-1, 1, size=(n, v.cin)).astype(np.float32)
    y, w = p.draw(n, v.cout)
    base, thr, _ = _base(v, m, n, x, y, w)
    yh = base[1].cpu().numpy()
    we = np.where(yh <= np.float32(thr), np.float32(1.0), w).astype(np.float32)
    inv_count = np.float32(1.0 / (float(n) * v.cout))
    g = ((np.float32(2.0) * (yh - y)) * we) * inv_count
    assert g.dtype == np.float32 and (we != w).any() and (we == w).any()
    ext = _step(m, n, coords=_dev(x), targets=_dev(g), loss="external")
    assert ext[0].item() == 0.0
    assert torch.equal(ext[1], base[1]), "yhat of the external step differs"
    bad = int((ext[2] != base[2]).sum())
    assert bad == 0, "external-loss gradients differ from the L2 step's in %d of %d parameters" % (bad, ext[2].numel())


AUTOGRAD = [V.BY_ID[i] for i in ("s22", "s300", "ffn", "nerf", "mfnf", "mfng", "pyr", "ps")]


@pytest.mark.parametrize("v", AUTOGRAD, ids=[v.label for v in AUTOGRAD])
def test_autograd_route_equals_the_fused_l2_step(v):
    """the reference's own loop body on the module (forward, torch MSE, backward): only torch's rounding of dL/dyhat separates it from the fused L2 step"""
    n = 1531
    m = v.make(DEV)
    p = _Pools(v, 400 + v.seed)
    x = _dev(p.rng.uniform(-1, 1, size=(n, v.cin)).astype(np.float32))
    y = _dev(p.draw(n, v.cout)[0])
    m.train_step(n, y, coords=x)
    fused = m.grads.cpu().numpy().copy()
    m.requires_grad_(True)
    yhat = m(x)
    assert yhat.requires_grad and yhat.shape == (n, v.cout)
    torch.nn.functional.mse_loss(yhat, y).backward()
    auto = m.params.grad.detach().cpu().numpy()
    worst = 0.0
    for name, pv in V.param_views(m):
        a, f = auto[pv._off:pv._off + pv.numel()], fused[pv._off:pv._off + pv.numel()]
        if name == "bvals":      # FFN: the Fourier matrix is fixed
            assert not a.any() and not f.any()
            continue
        assert np.abs(f).max() > 0, name
        d = relerr(a, f)
        worst = max(worst, d)
        assert d < 1e-4, (name, d)
    print("ENTRY-CONTRACT D %-6s autograd against the fused L2 step, worst parameter tensor: %.2e (band 1e-4)" % (v.id, worst))
