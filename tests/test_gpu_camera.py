"""Camera view on the GPU (view.render_rays / render_surface_rays, csrc/brief_rays.inc) on randomly initialised nets, with the grid, clip
box and voxel size of tests/test_gpu_view.py.  Every comparison of integers is bitwise.
  1  the anchor: a ray table filled from an oblique orthographic view (view.rays_from_view) reproduces view.render and
     view.render_surface bit for bit;
  2  a camera outside and one inside the volume equal the restatement: a numpy fold of the net's integer forward on
     brief_rays_sample_host's coordinates over ALL (row, col, k) with the host's inside flags, whatever the chunking;
  3  brief_rays_clip / brief_rays_coords equal the host's geometry, for five cameras and three lane counts;
  4  the surface through a camera: first hit, refinement (a numpy bisection on brief_rays_sample_t_host), position, distance, normals and
     shade under the per-ray headlight;
  5  the entries refuse bad arguments before any launch.
Projections use an integer window from the 0.15 quantile of the f32 decode to 5 % above its maximum (no ray's maximum saturates, so the
max image of a camera whose short rays all start at one point keeps its distinct values in uint8 too), surfaces that of
tests/test_gpu_surface.py (the whole range plus 5 %: no ray's maximum ties at the ceiling), and their levels: the median
over the rays that meet the box of the per-ray maximum ('above') or minimum ('below')."""
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
VS = (2, 1, 1)
# the coordinate range of the grid.  Every ray of a camera inside the volume starts at the eye, so where a smooth net falls along the
# whole cone the max image is that one value; over [-3, 3] these nets have structure on the scale of such a camera's short rays
LO, HI = -3.0, 3.0
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=VS)
OUTSIDE = dict(eye=(-20, 4, 52), direction=(0.85, 0.15, -0.5), fov=30, size=(37, 45), depth_spacing=0.5, region=BOX, voxel_size=VS)
CAMERAS = {
    "outside": OUTSIDE,
    "inside": dict(eye=(10.3, 14.6, 15.2), direction=(0.3, -0.5, 0.81), fov=100, size=(29, 35), depth_spacing=0.25, region=BOX, voxel_size=VS),
    "thin": dict(OUTSIDE, near=70, far=72),
    "plane": dict(OUTSIDE, near=71, far=71),
    "axis": dict(eye=(11, 15, -30), direction=(0, 0, 1), fov=30, size=(21, 27)),
}
IDS = ["s22", "s256", "nerf"]            # k_fused<1>, k_fused<8>, NeRF (cout 2; projections only: it has no Jacobian kernel)
JAC_IDS = ["s22", "s256"]
TORCH_DT = {"u16": torch.uint16, "u8": torch.uint8}
KIND = {"u8": _lib.OUT_U8, "u16": _lib.OUT_U16}
CASES = [(i, k) for i in IDS for k in ("u16", "u8")]
CASE = pytest.mark.parametrize("vid,kind", CASES, ids=["%s-%s" % c for c in CASES])
SURFACE_CASES = [(c, i, k, s) for c in ("outside", "inside") for i in JAC_IDS for k in ("u16", "u8") for s in VW.SIDES]
SURFACE_CASE = pytest.mark.parametrize("name,vid,kind,side", SURFACE_CASES, ids=["%s-%s-%s-%s" % c for c in SURFACE_CASES])

_cache = {}


def _net(vid, window):
    """the variant's net on the device and its integer window: 'view' (from the 0.15 quantile of the f32 decode to 5 % above its maximum)
    or 'surface' (the whole range plus 5 % on either side); computed once"""
    if vid not in _cache:
        v = V.BY_ID[vid]
        assert v.cin == 3
        m = v.make(DEV)
        f32 = m.decode_grid(DIMS, LO, HI).cpu().numpy().astype(np.float64)
        assert np.isfinite(f32).all() and f32.max() > f32.min()
        span = f32.max() - f32.min()
        _cache[vid] = (m, {"view": (float(np.float32(np.quantile(f32, 0.15))), float(np.float32(f32.max() + 0.05 * span))), "surface": (float(np.float32(f32.min() - 0.05 * span)), float(np.float32(f32.max() + 0.05 * span)))})
    m, scales = _cache[vid]
    return m, scales[window]


def _camera(name):
    if ("cam", name) not in _cache:
        cam = VW.make_camera(DIMS, **CAMERAS[name])
        cam.desc.lo, cam.desc.hi = LO, HI                           # (what the host restatements read; render_rays sets its own)
        _cache[("cam", name)] = cam
    return _cache[("cam", name)]


def _forward_int(m, coords, kind, scale):
    """the net's forward entry on explicit coordinates with the integer epilogue"""
    c = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).to(DEV)
    n = c.shape[0]
    out = torch.empty((n, m.data_channel), dtype=TORCH_DT[kind], device=DEV)
    m.sync_packed()
    b = _lib.BatchDesc(c.data_ptr(), None, None, None, 0, n, 0, 0, 0)
    _lib.check(m._abi_forward(None, b, out, KIND[kind], scale, V.VRANGE[kind], n))
    return out.cpu().numpy().astype(np.int64)


def _restate(name, vid, kind, window):
    """(cam, vals [rows, cols, depth, C] int64, inside [rows, cols, depth]) over the camera's whole lattice; computed once, read-only"""
    key = ("restate", name, vid, kind, window)
    if key not in _cache:
        m, scale = _net(vid, window)
        cam = _camera(name)
        row, col, k = np.meshgrid(np.arange(cam.rows), np.arange(cam.cols), np.arange(cam.depth), indexing="ij")
        _, coord, inside = VW.rays_sample_host(cam, row, col, k)
        vals = _forward_int(m, coord, kind, scale).reshape(cam.rows, cam.cols, cam.depth, -1)
        inside = inside.reshape(cam.rows, cam.cols, cam.depth)
        vals.setflags(write=False)
        inside.setflags(write=False)
        _cache[key] = (cam, vals, inside)
    return _cache[key]


def _fold(vals, inside, mode, dtype):
    hits = inside.sum(2).astype(np.int32)
    w = inside[..., None]
    if mode == "max":
        img = np.where(w, vals, -1).max(2)
    elif mode == "min":
        img = np.where(w, vals, 1 << 40).min(2)
    else:
        s = np.where(w, vals, 0).sum(2)
        img = (s.astype(np.float64) / np.maximum(hits, 1)[..., None]).astype(np.float32)
    img = np.where(hits[..., None] > 0, img, 0)
    return img.astype(np.float32 if mode == "mean" else dtype), hits


def _render_rays(m, cam, mode, kind, scale, chunk=None):
    img, hits, stats = VW.render_rays(m, cam, mode, LO, HI, kind, scale, V.VRANGE[kind], chunk=chunk)
    assert img.is_cuda and hits.dtype == torch.int32 and tuple(hits.shape) == (cam.rows, cam.cols)
    assert tuple(img.shape) == (cam.rows, cam.cols, m.data_channel) and img.dtype == (torch.float32 if mode == "mean" else TORCH_DT[kind])
    return img.cpu().numpy(), hits.cpu().numpy(), stats


def _surface_rays(m, cam, level, kind, scale, **kw):
    kw.setdefault("shading", False)
    out = VW.render_surface_rays(m, cam, level, LO, HI, kind, scale, V.VRANGE[kind], **kw)
    shape = (cam.rows, cam.cols)
    for key, dt in (("first", torch.int32), ("hits", torch.int32), ("t", torch.float32), ("t_lo", torch.float32), ("t_hi", torch.float32),
                    ("distance", torch.float32)):
        assert out[key].is_cuda and out[key].dtype == dt and tuple(out[key].shape) == shape, key
    assert tuple(out["position"].shape) == shape + (3,) and out["position"].dtype == torch.float32
    if not kw["shading"]:
        assert out["normal"] is None and out["shade"] is None
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}


def _np(out):
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _passes(x, level, side):
    return x >= level if side == "above" else x <= level


# ---- 1: the anchor
@CASE
def test_rays_of_an_orthographic_view_reproduce_the_orthographic_renderers(vid, kind):
    view = VW.make_view(DIMS, **OBLIQUE)
    cam = VW.rays_from_view(view)
    assert (view.rows * view.cols) % 64 != 0
    m, scale = _net(vid, "view")
    images = {}
    for mode in ("max", "min", "mean"):
        img, hits, stats = VW.render(m, view, mode, LO, HI, kind, scale, V.VRANGE[kind])
        for chunk in (None, 4001):
            img2, hits2, stats2 = _render_rays(m, cam, mode, kind, scale, chunk=chunk)
            assert np.array_equal(img2.view(np.uint8), img.cpu().numpy().view(np.uint8)), (mode, chunk)
            assert np.array_equal(hits2, hits.cpu().numpy()) and stats2 == stats, (mode, chunk)
        images[mode] = img.cpu().numpy().astype(np.int64)
    assert stats["samples_inside"] >= 10000 and 0 < stats["rays_hit"] < stats["rays"] and len(np.unique(images["max"])) >= 50
    # the surface, in the surface window: the level from the max / min view, shaded where the net has a Jacobian kernel
    met = hits.cpu().numpy() > 0
    direction = np.array(OBLIQUE["direction"], np.float64)
    shading = vid in JAC_IDS
    m, scale = _net(vid, "surface")
    gscale = gradient.voxel_scale(DIMS, LO, HI, scale, *V.VRANGE[kind]) / np.array(VS, np.float64)
    for side in VW.SIDES:
        extreme = _render_rays(m, cam, "max" if side == "above" else "min", kind, scale)[0].astype(np.int64)
        level = int(np.median(extreme[..., 0][met]))
        for refine in (0, 8):
            kw = dict(channel=0, side=side, refine=refine, shading=shading, light=direction, gscale=gscale)
            want = _np(VW.render_surface(m, view, level, LO, HI, kind, scale, V.VRANGE[kind], **kw))
            got = _surface_rays(m, cam, level, kind, scale, chunk=30011, **kw)
            for key in ("first", "hits", "t_lo", "t_hi", "t", "position"):
                assert np.array_equal(_bits(got[key]), _bits(want[key])), (side, refine, key)
            assert got["stats"] == want["stats"] and 0 < want["stats"]["rays_surface"] < want["stats"]["rays_hit"]
            assert np.array_equal(_bits(got["distance"]), _bits(want["t"]))          # near 0, depth_spacing 1: the depth in samples
            if shading:
                assert np.abs(got["normal"] - want["normal"]).max() <= 1e-5 and np.abs(got["shade"] - want["shade"]).max() <= 1e-5
                assert want["shade"].max() > 0


# ---- 2: the camera against the restatement
@CASE
@pytest.mark.parametrize("name", ["outside", "inside"])
def test_camera_projections_equal_the_restatement(name, vid, kind):
    m, scale = _net(vid, "view")
    cam, vals, inside = _restate(name, vid, kind, "view")
    got = {}
    for mode in ("max", "min", "mean"):
        want, want_hits = _fold(vals, inside, mode, V.NP_DTYPE[kind])
        img, hits, stats = _render_rays(m, cam, mode, kind, scale)
        assert np.array_equal(hits, want_hits), mode
        assert np.array_equal(img, want), (mode, int((img != want).sum()))
        assert stats["samples_evaluated"] == stats["samples_inside"] == int(inside.sum()) and stats["rays"] == cam.rows * cam.cols
        assert stats["rays_hit"] == int((want_hits > 0).sum())
        for chunk in (37, 4001, None):                              # chunk-invariant and repeatable
            img2, hits2, stats2 = _render_rays(m, cam, mode, kind, scale, chunk=chunk)
            assert np.array_equal(img2.view(np.uint8), img.view(np.uint8)) and np.array_equal(hits2, hits) and stats2 == stats, (mode, chunk)
        got[mode] = (img, hits, stats)
    # what keeps this from being vacuous
    img, hits, stats = got["max"]
    hit = hits > 0
    assert len(np.unique(img)) >= 50
    assert ((got["min"][0] < img).any(-1) & hit).sum() >= 0.5 * hit.sum()
    if name == "outside":
        assert cam.rows * cam.cols == 1665 and 0.3 <= hit.mean() <= 0.8 and stats["samples_inside"] >= 10000 and not hit.all()
        assert not inside[..., 0].any() and not inside[..., -1].any()
        assert VW._lanes(stats["samples_evaluated"] / stats["rays_hit"]) == 64
    else:
        assert hit.all() and inside[..., 0].all() and not inside[..., -1].any() and stats["samples_inside"] >= 30000


# ---- 3: device geometry equals host geometry
@pytest.mark.parametrize("name", list(CAMERAS))
def test_device_clip_and_coords_equal_the_host(name):
    L, st = _lib.lib(), _lib.stream_ptr()
    cam = VW.make_camera(DIMS, **CAMERAS[name])
    cam.desc.lo, cam.desc.hi = (-1.0, 1.0) if name != "inside" else (0.0, 1.0)
    rays = cam.rows * cam.cols
    table = torch.from_numpy(cam.rays).to(DEV)
    k0, cnt = torch.full((rays,), -7, dtype=torch.int32, device=DEV), torch.full((rays,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.brief_rays_clip(C.byref(cam.desc), _lib.ptr(table), _lib.ptr(k0), _lib.ptr(cnt), st))
    hk0, hcnt = VW.rays_clip_host(cam)
    assert np.array_equal(k0.cpu().numpy(), hk0.ravel()) and np.array_equal(cnt.cpu().numpy(), hcnt.ravel())
    off = torch.zeros(rays + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(cnt, 0, dtype=torch.int64, out=off[1:])
    total = int(off[-1].item())
    assert total == int(hcnt.sum()) > 0
    ray = np.repeat(np.arange(rays), hcnt.ravel())
    k = np.concatenate([np.arange(a, a + n) for a, n in zip(hk0.ravel(), hcnt.ravel())])
    _, want, inside = VW.rays_sample_host(cam, ray // cam.cols, ray % cam.cols, k)
    assert inside.all()
    host_off = np.concatenate([[0], np.cumsum(hcnt.ravel(), dtype=np.int64)])
    natural = VW._lanes(total / int((hcnt > 0).sum()))
    for lanes in sorted({1, 8, 64, natural}):
        for cuts in ([0, total], [0, total // 3, total // 3 + 1, total]):
            got = torch.full((total, 3), float("nan"), dtype=torch.float32, device=DEV)
            for s0, s1 in zip(cuts[:-1], cuts[1:]):
                if s1 == s0:
                    continue
                r0 = int(np.searchsorted(host_off[1:], s0, side="right"))
                r1 = int(np.searchsorted(host_off[:-1], s1, side="left"))
                chunk = torch.full((s1 - s0, 3), float("nan"), dtype=torch.float32, device=DEV)
                _lib.check(L.brief_rays_coords(C.byref(cam.desc), _lib.ptr(table), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(chunk), st))
                got[s0:s1] = chunk
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (lanes, cuts)


def test_the_cameras_exercise_three_lane_counts():
    seen = set()
    for name in ("outside", "thin", "plane"):
        k0, cnt = VW.rays_clip_host(VW.make_camera(DIMS, **CAMERAS[name]))
        seen.add(VW._lanes(cnt.sum() / (cnt > 0).sum()))
    assert len(seen) == 3 and {1, 64} <= seen, seen
    m, scale = _net("s22", "view")
    for name in ("thin", "plane"):                                  # the short rays fold to the restatement too
        cam, vals, inside = _restate(name, "s22", "u16", "view")
        for mode in ("max", "mean"):
            want, want_hits = _fold(vals, inside, mode, np.uint16)
            img, hits, stats = _render_rays(m, cam, mode, "u16", scale, chunk=211)
            assert np.array_equal(img, want) and np.array_equal(hits, want_hits) and stats["samples_evaluated"] == stats["samples_inside"] > 0


# ---- 4: the surface through the camera
def _first_along(passing):
    return np.where(passing.any(2), passing.argmax(2), -1).astype(np.int32)


def _want_surface(name, vid, kind, side):
    cam, vals, inside = _restate(name, vid, kind, "surface")
    x = vals[..., 0]
    met = inside.any(2)
    extreme = np.where(inside, x, -1).max(2) if side == "above" else np.where(inside, x, 1 << 40).min(2)
    level = int(np.median(extreme[met]))
    first = _first_along(inside & _passes(x, level, side))
    k0 = np.where(met, inside.argmax(2), 0)
    return cam, level, first, k0, inside


def _bisect(m, cam, kind, scale, level, side, first, k0, rounds):
    f = np.float32
    hit, bracket = first >= 0, (first >= 0) & (first > k0)
    t_hi = np.where(hit, first, np.nan).astype(f)
    t_lo = np.where(bracket, first - 1, t_hi).astype(f)
    row, col = np.nonzero(bracket)
    for _ in range(rounds if bracket.any() else 0):
        lo, hi = t_lo[bracket], t_hi[bracket]
        mid = lo + f(0.5) * (hi - lo)
        assert mid.dtype == f
        _, coord, _ = VW.rays_sample_t_host(cam, row, col, mid)
        ok = _passes(_forward_int(m, coord, kind, scale)[:, 0], level, side)
        t_hi[bracket], t_lo[bracket] = np.where(ok, mid, hi), np.where(ok, lo, mid)
    return t_lo, t_hi, bracket


def _np_shade(jac, gscale, side, light):
    """the shading kernel's formula in numpy float32, one rounding per operation, with a light per ray"""
    f = np.float32
    g = jac[:, 0, :].astype(f) * np.asarray(gscale, f)
    length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    ok = length > 0
    sign = f(1.0 if side == "below" else -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(ok[:, None], sign * g / length[:, None], f(0)).astype(f)
    l = np.asarray(light, f)
    d = -(n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1] + n[:, 2] * l[:, 2])
    return n, np.maximum(d, f(0)).astype(f)


@SURFACE_CASE
def test_camera_surface_equals_the_restatement(name, vid, kind, side):
    m, scale = _net(vid, "surface")
    cam, level, first, k0, inside = _want_surface(name, vid, kind, side)
    hit = first >= 0
    # the first hit, at refine 0, whatever the chunking
    ref = None
    for chunk in (None, 977, None):
        got = _surface_rays(m, cam, level, kind, scale, side=side, refine=0, chunk=chunk)
        assert np.array_equal(got["first"], first), (chunk, int((got["first"] != first).sum()))
        assert np.array_equal(got["hits"], inside.sum(2).astype(np.int32))
        stats = got["stats"]
        assert stats["samples_evaluated"] == stats["samples_inside"] == int(inside.sum()) and stats["rays_hit"] == int(inside.any(2).sum())
        assert stats["rays_surface"] == int(hit.sum()) and stats["rays_cut"] == int((hit & (first == k0)).sum()) and stats["refine_points"] == 0
        if ref is None:
            ref = got
        else:
            assert stats == ref["stats"] and all(np.array_equal(_bits(got[k]), _bits(ref[k])) for k in ("t", "t_lo", "t_hi", "position", "distance"))
    assert np.array_equal(ref["t"][hit], first[hit].astype(np.float32)) and np.isnan(ref["t"][~hit]).all()
    share = stats["rays_surface"] / stats["rays_hit"]
    print("%s %s %s %s: level %d, %d of %d rays that meet the box hit the surface (%.3f), %d of them cut" % (
        name, vid, kind, side, level, stats["rays_surface"], stats["rays_hit"], share, stats["rays_cut"]))
    assert 0.25 <= share <= 0.75, share
    if name == "outside":                                           # (every ray of the inside camera starts in the box: its hits may all be cut)
        assert stats["rays_surface"] - stats["rays_cut"] >= 0.25 * stats["rays_surface"] and (~hit).any()
    # eight rounds of refinement against a numpy bisection
    gscale = gradient.voxel_scale(DIMS, LO, HI, scale, *V.VRANGE[kind]) / np.array(VS, np.float64)
    got = _surface_rays(m, cam, level, kind, scale, side=side, refine=8, shading=True, gscale=gscale, chunk=30011)
    t_lo, t_hi, bracket = _bisect(m, cam, kind, scale, level, side, first, k0, 8)
    assert np.array_equal(got["first"], first)
    for key, want in (("t_lo", t_lo), ("t_hi", t_hi), ("t", t_hi)):
        assert np.array_equal(_bits(got[key]), _bits(want)), (key, int((_bits(got[key]) != _bits(want)).sum()))
    assert got["stats"]["refine_points"] == (8 * cam.rows * cam.cols if bracket.any() else 0)
    assert np.array_equal((got["t_hi"] - got["t_lo"])[bracket], np.full(int(bracket.sum()), 2.0 ** -8, np.float32))
    # position and distance
    row, col = np.nonzero(hit)
    pos, coord, ins = VW.rays_sample_t_host(cam, row, col, got["t"][hit])
    assert np.array_equal(_bits(got["position"][hit]), _bits(pos)) and ins.all() and np.isnan(got["position"][~hit]).all()
    want_d = np.float32(cam.near) + got["t"] * np.float32(cam.depth_spacing)
    assert want_d.dtype == np.float32 and np.array_equal(_bits(got["distance"]), _bits(want_d)) and np.isnan(got["distance"][~hit]).all()
    phys = np.linalg.norm((pos.astype(np.float64) - np.array(CAMERAS[name]["eye"])) * np.array(VS), axis=1)
    assert np.allclose(phys, got["distance"][hit], rtol=1e-5, atol=1e-4)                   # it IS the distance from the eye
    # normals and shade under the per-ray headlight
    _, jac = m.spatial_gradient(torch.from_numpy(coord).to(DEV), want_value=False)
    want_n, want_s = _np_shade(jac.cpu().numpy(), gscale, side, cam.light[hit])
    err_n, err_s = np.abs(got["normal"][hit] - want_n).max(), np.abs(got["shade"][hit] - want_s).max()
    print("max |normal - restatement| %.3g, max |shade - restatement| %.3g" % (err_n, err_s))
    assert err_n <= 1e-5 and err_s <= 1e-5
    length = np.linalg.norm(got["normal"][hit].astype(np.float64), axis=1)
    assert (np.abs(length - 1) <= 1e-5).all()
    assert not got["normal"][~hit].any() and not got["shade"][~hit].any()
    assert (got["shade"] >= 0).all() and (got["shade"] <= 1 + 1e-6).all()
    # at a bracketed hit the tested channel rises ('above') or falls ('below') along the ray, so the normal faces the eye and the
    # headlight lights it; the decode is truncated to integers and the bracket is 2^-8 samples wide, so a few hits may sit on a
    # local extremum: nine in ten must be lit (the condition of tests/test_gpu_surface.py)
    if bracket.any():
        lit = (got["shade"][bracket] > 0).mean()
        print("%.3f of the %d bracketed hits are lit by the headlight" % (lit, bracket.sum()))
        assert lit >= 0.9
    # a constant light is one direction for every ray
    const = _surface_rays(m, cam, level, kind, scale, side=side, refine=8, shading=True, gscale=gscale, light=(0.0, 0.6, -0.8))
    want_n, want_s = _np_shade(jac.cpu().numpy(), gscale, side, np.broadcast_to(np.array([0.0, 0.6, -0.8], np.float32), (int(hit.sum()), 3)))
    assert np.array_equal(_bits(const["t"]), _bits(got["t"])) and np.abs(const["shade"][hit] - want_s).max() <= 1e-5


def test_shading_is_refused_before_any_decode_behind_a_net_without_a_jacobian():
    m, scale = _net("nerf", "surface")
    cam = _camera("outside")
    with pytest.raises(ValueError, match="analytic Jacobian.*shading=False"):
        VW.render_surface_rays(m, cam, 100, LO, HI, "u8", scale, V.VRANGE["u8"])
    got = _surface_rays(m, cam, 100, "u8", scale, shading=False, refine=2)
    assert got["stats"]["samples_evaluated"] > 0
    with pytest.raises(ValueError, match="slice.*out of scope"):
        VW.render_rays(m, cam, "slice", LO, HI, "u8", scale, V.VRANGE["u8"])


# ---- 5: refusals before any launch
def test_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    cam = VW.make_camera(DIMS, **CAMERAS["axis"])
    rays = cam.rows * cam.cols
    table = torch.from_numpy(cam.rays).to(DEV)
    k0 = torch.zeros(rays, dtype=torch.int32, device=DEV)
    off = torch.zeros(rays + 1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(max(64, 3 * rays), dtype=torch.float32, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    d, tb = C.byref(cam.desc), p(table)
    bad = _lib.RaysDesc.from_buffer_copy(cam.desc)
    bad.depth = 1 << 24
    g = (C.c_float * 3)(1.0, 1.0, 1.0)
    nan3 = (C.c_float * 3)(1.0, float("nan"), 1.0)
    coords, fold, sfold = L.brief_rays_coords, L.brief_rays_fold, L.brief_rays_surface_fold
    for call, what in ((lambda: L.brief_rays_clip(d, None, p(k0), p(k0), st), "null"),
                       (lambda: L.brief_rays_clip(None, tb, p(k0), p(k0), st), "null descriptor"),
                       (lambda: L.brief_rays_clip(C.byref(bad), tb, p(k0), p(k0), st), "2^24"),
                       (lambda: coords(d, tb, p(k0), p(off), 0, 0, 0, 1, 1, p(buf), st), "sample range"),
                       (lambda: coords(d, tb, p(k0), p(off), 0, 4, 0, rays + 1, 1, p(buf), st), "ray range"),
                       (lambda: coords(d, tb, p(k0), p(off), 0, 4, 0, 1, 3, p(buf), st), "power of two"),
                       (lambda: coords(d, None, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), st), "null"),
                       (lambda: fold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_F32, 1, 0, p(k0), p(buf), st), "elem_kind"),
                       (lambda: fold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 5, 0, p(k0), p(buf), st), "channels"),
                       (lambda: fold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 3, p(k0), p(buf), st), "BRIEF_VIEW_SLICE"),
                       (lambda: fold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 4, p(k0), p(buf), st), "mode"),
                       (lambda: fold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 0, None, p(buf), st), "null"),
                       (lambda: sfold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 1, 0, 0, p(k0), p(k0), st), "channel"),
                       (lambda: sfold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 0, 256, 0, p(k0), p(k0), st), "level"),
                       (lambda: sfold(d, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 0, 0, 2, p(k0), p(k0), st), "BRIEF_SURFACE_ABOVE"),
                       (lambda: L.brief_rays_surface_coords(d, tb, p(buf), p(buf), 2, p(buf), None, st), "midpoint"),
                       (lambda: L.brief_rays_surface_coords(d, tb, p(buf), None, 0, p(buf), None, st), "null"),
                       (lambda: L.brief_rays_surface_shade(d, p(buf), p(buf), 1, 0, 0, nan3, p(buf), p(buf), p(buf), st), "gscale must be finite"),
                       (lambda: L.brief_rays_surface_shade(d, p(buf), p(buf), 1, 0, 0, g, None, p(buf), p(buf), st), "null")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and not k0.cpu().numpy().any()
    # a following valid call still works
    cnt = torch.zeros(rays, dtype=torch.int32, device=DEV)
    _lib.check(L.brief_rays_clip(d, tb, p(k0), p(cnt), st))
    hk0, hcnt = VW.rays_clip_host(cam)
    assert np.array_equal(k0.cpu().numpy(), hk0.ravel()) and np.array_equal(cnt.cpu().numpy(), hcnt.ravel()) and hcnt.sum() > 0
