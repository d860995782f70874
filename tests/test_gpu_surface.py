"""Surface view on the GPU (view.render_surface, csrc/brief_view.inc) on randomly initialised nets of every kernel family, with the
shapes of tests/test_gpu_view.py.  first, t_lo, t_hi, t, hits and stats are compared bitwise: the fold and every refinement decision
compare decoded integers.
  1  axis-aligned, unit spacing, refine=0: `first` is the index of the first voxel of decode_box's integer volume that passes the test;
  2  oblique: `first` equals the restatement (the net's integer forward on brief_view_sample_host's coordinates over the WHOLE lattice,
     then the first inside k that passes), whatever the chunking, and only the inside is evaluated;
  3  refinement: t_lo, t_hi, t equal a numpy bisection on brief_view_sample_t_host's coordinates; the bracket invariant holds;
  4  normals and shade (fp32 SIRENs) agree with m.spatial_gradient at the hits pushed through a float32 restatement of the shading;
  5  the entries refuse bad arguments before any launch.

The level is taken from the data: for side 'above' the median over the rays that meet the clip box of the per-ray MAXIMUM (the test's
own max view), so about half of those rays hit; for 'below' its mirror image, the median of the per-ray MINIMUM (with the maximum's
median nearly every ray would pass at its first sample, and nothing would be bracketed).  The integer window is the whole range of the
f32 decode plus 5 % on either side, so that no ray's maximum ties at the window's ceiling."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, gradient
from brief_pytorch_amd import view as VW
from tests import _variants as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (23, 31, 37)
BOX = "3:19,5:26,2:30"
BOX_SL = (slice(3, 19), slice(5, 26), slice(2, 30))
IDS = ["s22", "s256", "nerf", "mfnf", "pyr"]
JAC_IDS = ["s22", "s256"]                                    # what gradient.supported accepts
AXIS_DIR = {0: (1, 0, 0), 1: (0, -1, 0), 2: (0, 0, 1)}      # (AXIS_DIR[1] marches along -y)
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))
TORCH_DT = {"u16": torch.uint16, "u8": torch.uint8}
KIND = {"u8": _lib.OUT_U8, "u16": _lib.OUT_U16}
CASES = [(i, k, s, c) for i in IDS for k in ("u16", "u8") for s in VW.SIDES for c in ((0, 2) if i == "mfnf" else (0,))]
CASE = pytest.mark.parametrize("vid,kind,side,channel", CASES, ids=["%s-%s-%s-c%d" % c for c in CASES])
JAC_CASES = [c for c in CASES if c[0] in JAC_IDS]
JAC_CASE = pytest.mark.parametrize("vid,kind,side,channel", JAC_CASES, ids=["%s-%s-%s-c%d" % c for c in JAC_CASES])

_cache = {}


def _net(vid, kind):
    """the variant's net on the device, the integer window, and the integer decode of the whole grid, computed once"""
    if (vid, kind) not in _cache:
        if vid not in _cache:
            v = V.BY_ID[vid]
            assert v.cin == 3
            m = v.make(DEV)
            f32 = m.decode_grid(DIMS).cpu().numpy().astype(np.float64)
            assert np.isfinite(f32).all() and f32.max() > f32.min()
            span = f32.max() - f32.min()
            _cache[vid] = (m, (float(np.float32(f32.min() - 0.05 * span)), float(np.float32(f32.max() + 0.05 * span))))
        m, scale = _cache[vid]
        vol = m.decode_box(DIMS, out_kind=kind, scale=scale, vrange=V.VRANGE[kind]).cpu().numpy()
        assert vol.shape == DIMS + (m.data_channel,) and vol.dtype == V.NP_DTYPE[kind]
        _cache[(vid, kind)] = (m, scale, vol)
    return _cache[(vid, kind)]


def _forward_int(m, coords, kind, scale):
    """the net's forward entry on explicit coordinates with the integer epilogue"""
    c = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).to(DEV)
    n = c.shape[0]
    out = torch.empty((n, m.data_channel), dtype=TORCH_DT[kind], device=DEV)
    m.sync_packed()
    b = _lib.BatchDesc(c.data_ptr(), None, None, None, 0, n, 0, 0, 0)
    _lib.check(m._abi_forward(None, b, out, KIND[kind], scale, V.VRANGE[kind], n))
    return out.cpu().numpy().astype(np.int64)


def _restate(vid, kind):
    """the oblique view, and over its whole lattice (vals [rows, cols, depth, C] int64, inside [rows, cols, depth]); computed once"""
    key = ("oblique", vid, kind)
    if key not in _cache:
        m, scale, _ = _net(vid, kind)
        view = VW.make_view(DIMS, **OBLIQUE)
        row, col, k = np.meshgrid(np.arange(view.rows), np.arange(view.cols), np.arange(view.depth), indexing="ij")
        _, coord, inside = VW.sample_host(view, row, col, k)
        vals = _forward_int(m, coord, kind, scale).reshape(view.rows, view.cols, view.depth, -1)
        vals.setflags(write=False)
        _cache[key] = (view, vals, inside.reshape(view.rows, view.cols, view.depth))
    return _cache[key]


def _passes(x, level, side):
    return x >= level if side == "above" else x <= level


def _level(extreme, met, side):
    """the median over the rays that meet the box of the per-ray maximum ('above') or minimum ('below')"""
    return int(np.median(extreme[met]))


def _first_along(passing, axis):
    """the index of the first True along `axis`, -1 where there is none"""
    return np.where(passing.any(axis), passing.argmax(axis), -1).astype(np.int32)


def _surface(m, view, level, kind, scale, **kw):
    kw.setdefault("shading", False)
    out = VW.render_surface(m, view, level, -1.0, 1.0, kind, scale, V.VRANGE[kind], **kw)
    shape = (view.rows, view.cols)
    for key, dt in (("first", torch.int32), ("hits", torch.int32), ("t", torch.float32), ("t_lo", torch.float32), ("t_hi", torch.float32)):
        assert out[key].is_cuda and out[key].dtype == dt and tuple(out[key].shape) == shape, key
    assert tuple(out["position"].shape) == shape + (3,) and out["position"].dtype == torch.float32
    if not kw["shading"]:
        assert out["normal"] is None and out["shade"] is None
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}


def _not_vacuous(stats, what):
    share = stats["rays_surface"] / stats["rays_hit"]
    print("%s: %d of %d rays that meet the box hit the surface (%.3f), %d of them cut" % (what, stats["rays_surface"], stats["rays_hit"], share,
                                                                                         stats["rays_cut"]))
    assert 0.25 <= share <= 0.75, (what, share)
    assert stats["rays_surface"] - stats["rays_cut"] >= 0.25 * stats["rays_surface"], (what, stats)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1: axis-aligned views against decode_box's integer volume
@CASE
def test_axis_aligned_first_hit_is_the_first_voxel_that_passes(vid, kind, side, channel):
    m, scale, vol = _net(vid, kind)
    for region, sl in ((None, (slice(None),) * 3), (BOX, BOX_SL)):
        sub = vol[sl][..., channel].astype(np.int64)
        for a in range(3):
            march = np.flip(sub, 1) if a == 1 else sub             # k counts down the y axis
            level = _level(march.max(a) if side == "above" else march.min(a), np.ones(march.max(a).shape, bool), side)
            want = _first_along(_passes(march, level, side), a)
            view = VW.make_view(DIMS, AXIS_DIR[a], region=region)
            got = _surface(m, view, level, kind, scale, channel=channel, side=side, refine=0)
            assert np.array_equal(got["first"], want), (region, a, int((got["first"] != want).sum()))
            assert (got["hits"] == sub.shape[a]).all()
            hit = want >= 0
            assert np.isnan(got["t"][~hit]).all() and np.array_equal(got["t"][hit], want[hit].astype(np.float32))
            stats = got["stats"]
            assert stats["samples_evaluated"] == stats["samples_inside"] == sub.size and stats["refine_points"] == 0
            assert stats["rays_surface"] == int(hit.sum()) and stats["rays_cut"] == int((want == 0).sum())
            _not_vacuous(stats, "%s %s axis %d" % (vid, region, a))
            # the hit's position is the voxel itself
            idx = np.stack(np.nonzero(hit), 1)
            pos = got["position"][hit]
            start = [s.start or 0 for s in sl]
            depth_index = want[hit] if a != 1 else sub.shape[1] - 1 - want[hit]
            voxel = np.insert(idx + np.array([start[b] for b in range(3) if b != a]), a, depth_index + start[a], axis=1)
            assert np.array_equal(pos, voxel.astype(np.float32)) and np.isnan(got["position"][~hit]).all()


# ---- 2: the oblique view against the restatement
def _oblique_want(vid, kind, side, channel):
    view, vals, inside = _restate(vid, kind)
    x = vals[..., channel]
    met = inside.any(2)
    extreme = np.where(inside, x, -1).max(2) if side == "above" else np.where(inside, x, 1 << 40).min(2)
    level = _level(extreme, met, side)
    first = _first_along(inside & _passes(x, level, side), 2)
    k0 = np.where(met, inside.argmax(2), 0)
    return view, level, first, k0, inside


@CASE
def test_oblique_first_hit_equals_the_restatement(vid, kind, side, channel):
    m, scale, _ = _net(vid, kind)
    view, level, want, k0, inside = _oblique_want(vid, kind, side, channel)
    assert (view.rows * view.cols) % 64 != 0
    ref = None
    for chunk in (None, 1, 977, 30011, None):
        got = _surface(m, view, level, kind, scale, channel=channel, side=side, refine=0, chunk=chunk)
        assert np.array_equal(got["first"], want), (chunk, int((got["first"] != want).sum()))
        assert np.array_equal(got["hits"], inside.sum(2).astype(np.int32)), chunk
        stats = got["stats"]
        assert stats["samples_evaluated"] == stats["samples_inside"] == int(inside.sum()) and stats["rays"] == view.rows * view.cols
        assert stats["rays_hit"] == int(inside.any(2).sum()) and stats["rays_surface"] == int((want >= 0).sum())
        assert stats["rays_cut"] == int(((want >= 0) & (want == k0)).sum())
        if ref is None:
            ref = got
            _not_vacuous(stats, "%s oblique" % vid)
            assert not inside.all(2)[want >= 0].all(), "no hit ray leaves the box: the clip is not exercised"
        else:
            assert stats == ref["stats"] and all(np.array_equal(_bits(got[k]), _bits(ref[k])) for k in ("t", "t_lo", "t_hi", "position")), chunk
    # refine = 0: t is first wherever a ray hits
    hit = want >= 0
    assert np.array_equal(ref["t"][hit], want[hit].astype(np.float32)) and np.isnan(ref["t"][~hit]).all()
    assert np.array_equal(_bits(ref["t_hi"]), _bits(ref["t"]))
    assert np.array_equal(ref["t_lo"][hit], np.where(want > k0, want - 1, want)[hit].astype(np.float32))


# ---- 3: refinement against a numpy bisection
def _bisect(m, view, kind, scale, level, side, channel, first, k0, rounds):
    f = np.float32
    hit, bracket = first >= 0, (first >= 0) & (first > k0)
    t_hi = np.where(hit, first, np.nan).astype(f)
    t_lo = np.where(bracket, first - 1, t_hi).astype(f)
    row, col = np.nonzero(bracket)
    for _ in range(rounds):
        lo, hi = t_lo[bracket], t_hi[bracket]
        mid = lo + f(0.5) * (hi - lo)
        assert mid.dtype == f
        _, coord, _ = VW.sample_t_host(view, row, col, mid)
        ok = _passes(_forward_int(m, coord, kind, scale)[:, channel], level, side)
        t_hi[bracket], t_lo[bracket] = np.where(ok, mid, hi), np.where(ok, lo, mid)
    return t_lo, t_hi, bracket


@CASE
def test_refinement_equals_a_numpy_bisection(vid, kind, side, channel):
    m, scale, _ = _net(vid, kind)
    view, level, first, k0, _ = _oblique_want(vid, kind, side, channel)
    got = _surface(m, view, level, kind, scale, channel=channel, side=side, refine=8, chunk=30011)
    t_lo, t_hi, bracket = _bisect(m, view, kind, scale, level, side, channel, first, k0, 8)
    assert np.array_equal(got["first"], first)
    for key, want in (("t_lo", t_lo), ("t_hi", t_hi), ("t", t_hi)):
        assert np.array_equal(_bits(got[key]), _bits(want)), (key, int((_bits(got[key]) != _bits(want)).sum()))
    assert got["stats"]["refine_points"] == 8 * view.rows * view.cols
    hit, cut = first >= 0, (first >= 0) & (first == k0)
    assert np.array_equal(got["t"][cut], first[cut].astype(np.float32)) and np.array_equal(got["t_lo"][cut], got["t_hi"][cut])
    # the bracket: 2^-8 of a sample wide, the test fails at t_lo and passes at t_hi
    assert np.array_equal((got["t_hi"] - got["t_lo"])[bracket], np.full(int(bracket.sum()), 2.0 ** -8, np.float32))
    row, col = np.nonzero(bracket)
    for key, want in (("t_lo", False), ("t_hi", True)):
        _, coord, _ = VW.sample_t_host(view, row, col, got[key][bracket])
        assert (_passes(_forward_int(m, coord, kind, scale)[:, channel], level, side) == want).all(), key
    # position is the stated position at t, inside the clip box
    row, col = np.nonzero(hit)
    pos, _, inside = VW.sample_t_host(view, row, col, got["t"][hit])
    assert np.array_equal(_bits(got["position"][hit]), _bits(pos)) and inside.all() and np.isnan(got["position"][~hit]).all()
    # a repeat gives the same bits
    again = _surface(m, view, level, kind, scale, channel=channel, side=side, refine=8)
    assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in ("first", "t", "t_lo", "t_hi", "position"))


# ---- 4: normals and shade against m.spatial_gradient
def _np_shade(jac, channel, gscale, side, light):
    """the shading kernel's formula in numpy float32, one rounding per operation"""
    f = np.float32
    g = jac[:, channel, :].astype(f) * np.asarray(gscale, f)
    length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    ok = length > 0
    sign = f(1.0 if side == "below" else -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(ok[:, None], sign * g / length[:, None], f(0)).astype(f)
    l = np.asarray(light, f)
    d = -(n[:, 0] * l[0] + n[:, 1] * l[1] + n[:, 2] * l[2])
    return n, np.maximum(d, f(0)).astype(f)


@JAC_CASE
def test_normals_and_shade_agree_with_the_spatial_gradient(vid, kind, side, channel):
    m, scale, _ = _net(vid, kind)
    view, level, first, k0, _ = _oblique_want(vid, kind, side, channel)
    hit = first >= 0
    vs = np.array(OBLIQUE["voxel_size"], np.float64)
    gscale = gradient.voxel_scale(DIMS, -1.0, 1.0, scale, *V.VRANGE[kind]) / vs
    direction = np.array(OBLIQUE["direction"], np.float64)
    assert abs(np.linalg.norm(direction) - 1) < 1e-12
    row, col = np.nonzero(hit)
    for light in (direction, None, (0.0, 0.6, -0.8)):
        got = _surface(m, view, level, kind, scale, channel=channel, side=side, refine=8, shading=True, gscale=gscale, light=light)
        assert got["normal"].shape == (view.rows, view.cols, 3) and got["shade"].shape == (view.rows, view.cols)
        assert got["normal"].dtype == np.float32 and got["shade"].dtype == np.float32
        assert np.array_equal(got["first"], first)
        _, coord, _ = VW.sample_t_host(view, row, col, got["t"][hit])
        _, jac = m.spatial_gradient(torch.from_numpy(coord).to(DEV), want_value=False)
        if light is None:                                           # the default: the view's own direction, normalised
            l = np.array(list(view.ddepth), np.float64)
            l = l / np.linalg.norm(l)
        else:
            l = np.asarray(light, np.float64)
        want_n, want_s = _np_shade(jac.cpu().numpy(), channel, gscale, side, l)
        err_n, err_s = np.abs(got["normal"][hit] - want_n).max(), np.abs(got["shade"][hit] - want_s).max()
        print("%s %s %s light %s: max |normal - restatement| %.3g, max |shade - restatement| %.3g" % (vid, kind, side, light, err_n, err_s))
        assert err_n <= 1e-5 and err_s <= 1e-5
        length = np.linalg.norm(got["normal"][hit].astype(np.float64), axis=1)
        assert (np.abs(length - 1) <= 1e-5).all(), "unit normals (a zero gradient at a hit would be a coincidence)"
        assert not got["normal"][~hit].any() and not got["shade"][~hit].any() and (~hit).any()
        assert (got["shade"] >= 0).all() and (got["shade"] <= 1 + 1e-6).all()
    # lit along the physical view direction (the first pass above is kept last here): at a bracketed hit the tested channel rises
    # ('above') or falls ('below') along the ray, so the normal faces the viewer and the headlight lights it.  The decode is
    # truncated to integers and the bracket is 2^-8 samples wide, so a few hits may sit on a local extremum: nine in ten must be lit.
    got = _surface(m, view, level, kind, scale, channel=channel, side=side, refine=8, shading=True, gscale=gscale, light=direction)
    bracket = hit & (first > k0)
    lit = (got["shade"][bracket] > 0).mean()
    print("%s %s %s: %.3f of the bracketed hits are lit by the headlight" % (vid, kind, side, lit))
    assert lit >= 0.9


@pytest.mark.parametrize("vid", JAC_IDS)
def test_flipping_the_side_flips_the_normal(vid):
    """a ray whose first inside sample equals the level passes BOTH tests there: a cut ray on either side, with the same hit point, so
    the two normals are each other's negative, bit for bit"""
    kind = "u8"
    m, scale, _ = _net(vid, kind)
    view, vals, inside = _restate(vid, kind)
    met = inside.any(2)
    k0 = np.where(met, inside.argmax(2), 0)
    at_entry = np.take_along_axis(vals[..., 0], k0[..., None], 2)[..., 0]
    level = int(np.bincount(at_entry[met]).argmax())
    both = met & (at_entry == level)
    assert both.sum() >= 1
    out = {s: _surface(m, view, level, kind, scale, side=s, refine=8, shading=True) for s in VW.SIDES}
    for s in VW.SIDES:
        assert np.array_equal(out[s]["first"][both], k0[both]) and np.array_equal(out[s]["t"][both], k0[both].astype(np.float32))
        assert (out[s]["first"] >= 0).sum() > both.sum()            # both sides hit elsewhere too
    a, b = out["above"]["normal"][both], out["below"]["normal"][both]
    assert np.abs(a).max() > 0 and np.array_equal(_bits(a), _bits(-b))
    # the headlight lights exactly one of the two
    sa, sb = out["above"]["shade"][both], out["below"]["shade"][both]
    assert ((sa > 0) != (sb > 0))[(sa > 0) | (sb > 0)].all() and np.array_equal(np.maximum(sa, sb), np.abs(sa - sb))


# ---- 5: refusals before any launch
def test_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    view = VW.make_view(DIMS, (1, 0, 0))
    rays = view.rows * view.cols
    k0 = torch.zeros(rays, dtype=torch.int32, device=DEV)
    off = torch.zeros(rays + 1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(rays * 4, dtype=torch.float32, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    v = C.byref(view)
    f3 = (C.c_float * 3)(1.0, 0.0, 0.0)
    bad3 = (C.c_float * 3)(1.0, float("nan"), 0.0)
    fold = lambda **kw: L.brief_surface_fold(v, p(k0), p(off), 0, 4, 0, 1, kw.get("lanes", 1), kw.get("vals", p(buf)), kw.get("kind", _lib.OUT_U8),
                                             kw.get("channels", 2), kw.get("channel", 0), kw.get("level", 7), kw.get("side", 0), p(k0),
                                             kw.get("first", p(k0)), st)
    step = lambda **kw: L.brief_surface_step(v, p(buf), kw.get("kind", _lib.OUT_U16), 2, kw.get("channel", 0), kw.get("level", 7), kw.get("side", 1),
                                             kw.get("t_lo", p(buf)), p(buf), st)
    shade = lambda **kw: L.brief_surface_shade(v, p(buf), kw.get("jac", p(buf)), 1, kw.get("channel", 0), kw.get("side", 0), kw.get("gscale", f3),
                                               f3, p(buf), p(buf), st)
    for call, what in ((lambda: fold(vals=None), "null buffer"), (lambda: fold(first=None), "null buffer"),
                       (lambda: fold(channel=2), "channel must be 0 .. channels - 1"), (lambda: fold(channel=-1), "channel must be 0 .. channels - 1"),
                       (lambda: fold(channels=5), "channels must be 1..4"), (lambda: fold(level=256), "0 .. 255 for uint8"),
                       (lambda: fold(level=-1), "level must lie"), (lambda: fold(kind=_lib.OUT_U16, level=65536), "0 .. 65535 for uint16"),
                       (lambda: fold(side=2), "BRIEF_SURFACE_ABOVE (0) or BRIEF_SURFACE_BELOW (1)"), (lambda: fold(kind=_lib.OUT_F32), "elem_kind"),
                       (lambda: fold(lanes=3), "power of two"),
                       (lambda: L.brief_surface_bracket(v, p(k0), None, p(buf), p(buf), st), "null buffer"),
                       (lambda: L.brief_surface_coords(v, p(buf), p(buf), 1, None, None, st), "null buffer"),
                       (lambda: L.brief_surface_coords(v, p(buf), p(buf), 2, p(buf), None, st), "midpoint must be 0"),
                       (lambda: step(t_lo=None), "null buffer"), (lambda: step(channel=2), "channel must be 0 .. channels - 1"),
                       (lambda: step(side=-1), "BRIEF_SURFACE_ABOVE"), (lambda: step(level=70000), "0 .. 65535 for uint16"),
                       (lambda: shade(jac=None), "null buffer"), (lambda: shade(channel=1), "channel must be 0 .. channels - 1"),
                       (lambda: shade(side=3), "BRIEF_SURFACE_ABOVE"), (lambda: shade(gscale=bad3), "gscale and light must be finite")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and not k0.cpu().numpy().any()
    # the Python call: refine, side, level, channel and a net without the Jacobian kernel, before any decode
    m, scale, _ = _net("s22", "u16")
    call = lambda phi=m, **kw: VW.render_surface(phi, view, kw.pop("level", 20000), -1.0, 1.0, kw.pop("kind", "u16"), scale, V.VRANGE["u16"], **kw)
    for refine in (-1, 17, 2.5):
        with pytest.raises(ValueError, match="refine must be 0 \\.\\. 16"):
            call(refine=refine)
    with pytest.raises(ValueError, match="side 'front' is not one of above \\| below"):
        call(side="front")
    with pytest.raises(ValueError, match="channel 1 does not exist"):
        call(channel=1)
    with pytest.raises(ValueError, match="level 65536 lies outside"):
        call(level=65536)
    with pytest.raises(ValueError, match="level 256 lies outside"):
        call(level=256, kind="u8")
    with pytest.raises(ValueError, match="u8.*u16"):
        call(kind="f32")
    for vid in ("nerf", "mfnf", "pyr"):
        phi = _net(vid, "u16")[0]
        with pytest.raises(ValueError) as e:
            call(phi=phi)
        assert gradient.refusal(type(phi).kind, phi.precision, phi.features) in str(e.value) and "shading=False" in str(e.value)
