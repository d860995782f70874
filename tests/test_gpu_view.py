"""View decode on the GPU (brief_pytorch_amd/view.py, csrc/brief_view.inc) on randomly initialised nets of every kernel family.  Every
comparison is bitwise: the folds are integer folds.
  1  axis-aligned views of unit spacing equal the existing decodes: a slice is a plane of decode_box, a max view an image of decode_mips;
  2  an oblique view equals the restatement: a numpy fold of the net's forward on brief_view_sample_host's coordinates over ALL
     (row, col, k), inside or not, with the host's inside flags;
  3  chunking and repetition change nothing;  4  only the inside is evaluated;  5  the oblique case is not vacuous."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, mip
from brief_pytorch_amd import view as VW
from tests import _variants as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (23, 31, 37)
BOX = "3:19,5:26,2:30"
BOX_SL = (slice(3, 19), slice(5, 26), slice(2, 30))
IDS = ["s22", "s256", "nerf", "mfnf", "pyr"]          # k_fused<1> (the narrow SIREN of k_small's class), k_fused<8>, NeRF (cout 2), MFN (cout 4), a taper
CASES = [(i, k) for i in IDS for k in ("u16", "u8")]
CASE = pytest.mark.parametrize("vid,kind", CASES, ids=["%s-%s" % c for c in CASES])
# looking along +z, -y, +x gives the orientations of mip_ops' three images (view.frame)
AXIS_DIR = {0: (1, 0, 0), 1: (0, -1, 0), 2: (0, 0, 1)}
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))
TORCH_DT = {"u16": torch.uint16, "u8": torch.uint8}

_cache = {}


def _net(vid, kind):
    """the variant's net on the device, an integer window that does not leave the images flat (the 0.15 / 0.85 quantiles of the f32
    decode), and the integer decode of the whole grid, computed once"""
    if (vid, kind) not in _cache:
        if vid not in _cache:
            v = V.BY_ID[vid]
            assert v.cin == 3
            m = v.make(DEV)
            f32 = m.decode_grid(DIMS).cpu().numpy()
            assert np.isfinite(f32).all()
            q15, q85 = (float(np.float32(q)) for q in np.quantile(f32.astype(np.float64), [0.15, 0.85]))
            assert q85 > q15
            _cache[vid] = (m, (q15, q85))
        m, scale = _cache[vid]
        vol = m.decode_box(DIMS, out_kind=kind, scale=scale, vrange=V.VRANGE[kind]).cpu().numpy()
        assert vol.shape == DIMS + (m.data_channel,) and vol.dtype == V.NP_DTYPE[kind]
        _cache[(vid, kind)] = (m, scale, vol)
    return _cache[(vid, kind)]


def _render(m, view, mode, kind, scale, chunk=None):
    img, hits, stats = VW.render(m, view, mode, -1.0, 1.0, kind, scale, V.VRANGE[kind], chunk=chunk)
    assert img.is_cuda and hits.dtype == torch.int32 and tuple(hits.shape) == (view.rows, view.cols)
    assert tuple(img.shape) == (view.rows, view.cols, m.data_channel)
    assert img.dtype == (torch.float32 if mode == "mean" else TORCH_DT[kind])
    return img.cpu().numpy(), hits.cpu().numpy(), stats


# ---- 1: equals the existing decodes
@CASE
def test_axis_aligned_views_equal_the_existing_decodes(vid, kind):
    m, scale, vol = _net(vid, kind)
    centre = [(n - 1) // 2 for n in DIMS]
    for region, sl in ((None, (slice(None),) * 3), (BOX, BOX_SL)):
        start = [s.start or 0 for s in sl]
        stop = [s.stop if s.stop is not None else n for s, n in zip(sl, DIMS)]
        mips = [t.cpu().numpy() for t in mip.decode_mips(m, DIMS, start, stop, [1, 1, 1], -1.0, 1.0, kind, scale, V.VRANGE[kind])]
        sub = vol[sl]
        for a in range(3):
            view = VW.make_view(DIMS, AXIS_DIR[a], region=region)
            img, hits, stats = _render(m, view, "max", kind, scale)
            assert np.array_equal(img, mips[a]) and np.array_equal(img, sub.max(a)), (region, a)
            assert (hits == sub.shape[a]).all() and stats["samples_evaluated"] == stats["samples_inside"] == sub.size // m.data_channel
            for plane in {start[a], (start[a] + stop[a]) // 2, DIMS[a] // 2 - 1, DIMS[a] // 2, stop[a] - 1}:      # both sides of n / 2
                off = (plane - centre[a]) * (-1 if a == 1 else 1)
                view = VW.make_view(DIMS, AXIS_DIR[a], region=region, depth=float(off))
                assert view.depth == 1
                img, hits, stats = _render(m, view, "slice", kind, scale)
                assert np.array_equal(img, vol.take(plane, axis=a)[tuple(s for i, s in enumerate(sl) if i != a)]), (region, a, plane)
                assert (hits == 1).all() and stats["samples_evaluated"] == hits.size
        # a plane outside the clip box: nothing is evaluated, the image is 0
        if region is not None:
            view = VW.make_view(DIMS, AXIS_DIR[0], region=region, depth=float(20 - centre[0]))
            img, hits, stats = _render(m, view, "slice", kind, scale)
            assert not img.any() and not hits.any() and stats["samples_evaluated"] == 0 and stats["rays_hit"] == 0


# ---- 2 .. 5: the oblique view against the restatement
def _forward_int(m, coords, kind, scale):
    """the net's forward entry on explicit coordinates with the integer epilogue"""
    c = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).to(DEV)
    n = c.shape[0]
    out = torch.empty((n, m.data_channel), dtype=TORCH_DT[kind], device=DEV)
    m.sync_packed()
    b = _lib.BatchDesc(c.data_ptr(), None, None, None, 0, n, 0, 0, 0)
    _lib.check(m._abi_forward(None, b, out, {"u8": _lib.OUT_U8, "u16": _lib.OUT_U16}[kind], scale, V.VRANGE[kind], n))
    return out.cpu().numpy()


def _restate(m, view, kind, scale):
    """(vals [rows, cols, depth, C] int64, inside [rows, cols, depth]) over the whole lattice"""
    row, col, k = np.meshgrid(np.arange(view.rows), np.arange(view.cols), np.arange(view.depth), indexing="ij")
    _, coord, inside = VW.sample_host(view, row, col, k)
    vals = _forward_int(m, coord, kind, scale).astype(np.int64)
    return vals.reshape(view.rows, view.cols, view.depth, -1), inside.reshape(view.rows, view.cols, view.depth)


def _fold(vals, inside, mode, dtype):
    hits = inside.sum(2).astype(np.int32)
    w = inside[..., None]
    if mode in ("max", "slice"):
        img = np.where(w, vals, -1).max(2)
    elif mode == "min":
        img = np.where(w, vals, 1 << 40).min(2)
    else:
        s = np.where(w, vals, 0).sum(2)
        img = (s.astype(np.float64) / np.maximum(hits, 1)[..., None]).astype(np.float32)
    img = np.where(hits[..., None] > 0, img, 0)
    return img.astype(np.float32 if mode == "mean" else dtype), hits


@CASE
def test_oblique_view_equals_the_restatement(vid, kind):
    m, scale, _ = _net(vid, kind)
    view = VW.make_view(DIMS, **OBLIQUE)
    assert (view.rows * view.cols) % 64 != 0 and view.rows % 64 != 0 and view.cols % 64 != 0
    vals, inside = _restate(m, view, kind, scale)
    got = {}
    for mode in ("max", "min", "mean"):
        want, want_hits = _fold(vals, inside, mode, V.NP_DTYPE[kind])
        img, hits, stats = _render(m, view, mode, kind, scale)
        assert np.array_equal(hits, want_hits), mode
        assert np.array_equal(img, want), (mode, int((img != want).sum()))
        assert stats["samples_inside"] == int(inside.sum()) and stats["rays"] == view.rows * view.cols
        assert stats["rays_hit"] == int((want_hits > 0).sum())
        # 4: only the inside is evaluated
        assert stats["samples_evaluated"] <= stats["samples_inside"] + 2 * stats["rays_hit"]
        # 3: chunk-invariant and repeatable
        for chunk in (4001, None):
            img2, hits2, stats2 = _render(m, view, mode, kind, scale, chunk=chunk)
            assert np.array_equal(img2.view(np.uint8), img.view(np.uint8)) and np.array_equal(hits2, hits) and stats2 == stats, (mode, chunk)
        got[mode] = (img, hits, stats)
    # an oblique plane, off the centre
    plane = VW.make_view(DIMS, depth=1.3, **OBLIQUE)
    assert plane.depth == 1
    pv, pin = _restate(m, plane, kind, scale)
    want, want_hits = _fold(pv, pin, "slice", V.NP_DTYPE[kind])
    img, hits, stats = _render(m, plane, "slice", kind, scale)
    assert np.array_equal(img, want) and np.array_equal(hits, want_hits) and 0 < stats["rays_hit"] < stats["rays"]
    # 5: what keeps all this from being vacuous
    img, hits, stats = got["max"]
    assert stats["rays_hit"] >= 0.2 * stats["rays"] and stats["rays"] - stats["rays_hit"] >= 0.1 * stats["rays"]
    assert stats["samples_inside"] >= 10000
    assert len(np.unique(img)) >= 50
    hit = hits > 0
    assert ((got["min"][0] < img).any(-1) & hit).sum() >= 0.5 * hit.sum()
    assert not inside.all(2)[hit].all(), "no hit ray leaves the box: the clip is not exercised"


def test_group_sizes_and_a_clip_box_inside_the_volume():
    """the lanes that share a ray follow the mean samples per ray: 1 (a plane), a few (a thin slab) and 64 (a long projection) all
    (8, 64 and 16 lanes here) fold to the same restatement, with a clip box that cuts rays short at both ends"""
    m, scale, _ = _net("s22", "u16")
    seen = set()
    for kw in (dict(OBLIQUE, region=BOX, depth=(-1.0, 1.0)), dict(OBLIQUE, region=BOX, depth_spacing=0.05, spacing=2.9),
               dict(direction=(1.0, 1e-5, -3e-6), region=BOX)):
        view = VW.make_view(DIMS, **kw)
        vals, inside = _restate(m, view, "u16", scale)
        for mode in ("max", "mean"):
            want, want_hits = _fold(vals, inside, mode, np.uint16)
            img, hits, stats = _render(m, view, mode, "u16", scale, chunk=30011)
            assert np.array_equal(img, want) and np.array_equal(hits, want_hits), (kw, mode)
            assert stats["samples_evaluated"] == stats["samples_inside"] > 0
        seen.add(VW._lanes(stats["samples_evaluated"] / stats["rays_hit"]))
    assert len(seen) == 3 and 64 in seen, seen


def test_entries_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    L = _lib.lib()
    view = VW.make_view(DIMS, (1, 0, 0))
    rays = view.rows * view.cols
    k0 = torch.zeros(rays, dtype=torch.int32, device=DEV)
    off = torch.zeros(rays + 1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    v, coords, fold = C.byref(view), L.brief_view_coords, L.brief_view_fold
    for call, what in ((lambda: L.brief_view_clip(v, None, p(k0), st), "null"),
                       (lambda: coords(v, p(k0), p(off), 0, 0, 0, 1, 1, p(buf), st), "sample range"),
                       (lambda: coords(v, p(k0), p(off), 0, 4, 0, rays + 1, 1, p(buf), st), "ray range"),
                       (lambda: coords(v, p(k0), p(off), 0, 4, 0, 1, 3, p(buf), st), "power of two"),
                       (lambda: fold(v, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_F32, 1, 0, p(k0), p(buf), st), "elem_kind"),
                       (lambda: fold(v, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 5, 0, p(k0), p(buf), st), "channels"),
                       (lambda: fold(v, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 4, p(k0), p(buf), st), "mode"),
                       (lambda: L.brief_view_finish(v, _lib.OUT_U8, 1, 0, p(k0), None, p(buf), st), "null")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and not k0.cpu().numpy().any()
    with pytest.raises(ValueError, match="depth 1"):
        VW.render(_net("s22", "u16")[0], view, "slice", -1.0, 1.0, "u16", (0.0, 1.0), V.VRANGE["u16"])
    with pytest.raises(ValueError, match="u8.*u16"):
        VW.render(_net("s22", "u16")[0], view, "max", -1.0, 1.0, "f32", (0.0, 1.0), V.VRANGE["u16"])
