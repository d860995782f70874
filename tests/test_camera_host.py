"""Host side of the camera view (view.make_camera / rays_from_view, csrc/brief_rays.h, decompress.py --view-eye): make_camera against
its own definition in float64, the ray geometry of csrc/brief_rays.h against a numpy fp32 restatement and against the orthographic
header, the refusals, the C-ABI's declaration.  Nothing here needs a GPU: brief_rays_sample_host / _sample_t_host / _clip_host run the
header the kernels run, on the host CPU."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from brief_pytorch_amd import _lib
from brief_pytorch_amd import view as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (23, 31, 37)
BOX = "3:19,5:26,2:30"
VS = (2, 1, 1)
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=VS)
OUTSIDE = dict(eye=(-20, 4, 52), direction=(0.85, 0.15, -0.5), fov=30, size=(37, 45), depth_spacing=0.5, region=BOX, voxel_size=VS)
CAMERAS = {
    "outside": OUTSIDE,
    "inside": dict(eye=(10.3, 14.6, 15.2), direction=(0.3, -0.5, 0.81), fov=100, size=(29, 35), depth_spacing=0.25, region=BOX, voxel_size=VS),
    "thin": dict(OUTSIDE, near=70, far=72),
    "plane": dict(OUTSIDE, near=71, far=71),
    "axis": dict(eye=(11, 15, -30), direction=(0, 0, 1), fov=30, size=(21, 27)),
}

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")


def _lattice(cam):
    return np.meshgrid(np.arange(cam.rows), np.arange(cam.cols), np.arange(cam.depth), indexing="ij")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1: make_camera against its own definition
def _definition(dims, eye, direction, up=None, fov=60.0, size=(256, 256), near=0.0, far=None, depth_spacing=1.0, voxel_size=(1, 1, 1), region=None):
    """make_camera's documented formulas in float64, pixel by pixel: (table [rows, cols, 6], unit [rows, cols, 3], depth)"""
    rows, cols = size
    vs, e = np.array(voxel_size, np.float64), np.array(eye, np.float64)
    row_dir, col_dir, d = V.frame(direction, up)
    s = 2.0 * np.tan(np.radians(fov) / 2.0) / rows
    table, unit = np.empty((rows, cols, 6)), np.empty((rows, cols, 3))
    for i in range(rows):
        for j in range(cols):
            w = d + (i - (rows - 1) / 2.0) * s * row_dir + (j - (cols - 1) / 2.0) * s * col_dir
            unit[i, j] = w / np.sqrt(np.dot(w, w))
            table[i, j, :3] = e + near * unit[i, j] / vs
            table[i, j, 3:] = depth_spacing * unit[i, j] / vs
    if far is None:
        sl = [slice(None)] * 3 if region is None else [slice(*(int(x) if x else None for x in part.split(":"))) for part in region.split(",")]
        lo = np.array([s_.start or 0 for s_ in sl], np.float64)
        hi = np.array([(s_.stop if s_.stop is not None else n) - 1 for s_, n in zip(sl, dims)], np.float64)
        corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
        far = max(np.sqrt((((corners - e) * vs) ** 2).sum(1)).max(), near)
    return table, unit, int(np.floor((far - near) / depth_spacing + 1e-9)) + 1


@pytest.mark.parametrize("name", list(CAMERAS))
def test_make_camera_equals_its_definition(name):
    kw = CAMERAS[name]
    cam = V.make_camera(DIMS, **kw)
    table, unit, depth = _definition(DIMS, **kw)
    rows, cols = kw["size"]
    assert (cam.rows, cam.cols, cam.depth) == (rows, cols, depth) == (cam.desc.rows, cam.desc.cols, cam.desc.depth)
    assert cam.rays.shape == (rows, cols, 6) and cam.rays.dtype == np.float32 and cam.light.shape == (rows, cols, 3) and cam.light.dtype == np.float32
    for got, want in ((cam.rays, table), (cam.light, unit)):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp).all()
    vs = np.array(kw.get("voxel_size", (1, 1, 1)), np.float64)
    step = np.linalg.norm(cam.rays[..., 3:].astype(np.float64) * vs, axis=2)
    assert np.allclose(step, kw.get("depth_spacing", 1.0), rtol=1e-6, atol=0) and np.allclose(np.linalg.norm(cam.light.astype(np.float64), axis=2), 1, rtol=1e-6, atol=0)
    assert list(cam.desc.dims) == list(DIMS) and cam.near == float(np.float32(kw.get("near", 0.0))) and cam.depth_spacing == kw.get("depth_spacing", 1.0)
    if "region" in kw:
        assert list(cam.desc.box_lo) == [3.0, 5.0, 2.0] and list(cam.desc.box_hi) == [18.0, 25.0, 29.0]
    else:
        assert list(cam.desc.box_lo) == [0.0, 0.0, 0.0] and list(cam.desc.box_hi) == [22.0, 30.0, 36.0]


def test_make_camera_frame_fov_and_scaling():
    d = np.array(OUTSIDE["direction"], np.float64)
    d = d / np.linalg.norm(d)
    # an odd size has a centre pixel: its ray is along `direction`
    cam = V.make_camera(DIMS, **OUTSIDE)
    assert np.allclose(cam.light[18, 22].astype(np.float64), d, atol=1e-6)
    # rows run along `up` made orthogonal to the direction, cols along direction x row_dir: frame()'s handedness
    up = (0.0, 1.0, 0.2)
    cam = V.make_camera(DIMS, **dict(OUTSIDE, up=up, voxel_size=(1, 1, 1)))
    row_dir, col_dir, dd = V.frame(OUTSIDE["direction"], up)
    l = cam.light.astype(np.float64)
    down, right = l[-1, 22] - l[0, 22], l[18, -1] - l[18, 0]
    assert np.dot(down, row_dir) > 0 and abs(np.dot(down, col_dir)) < 1e-6 and np.dot(right, col_dir) > 0 and abs(np.dot(right, row_dir)) < 1e-6
    assert np.dot(np.cross(dd, down), right) > 0 and np.dot(row_dir, np.array(up) - np.dot(up, dd) * dd) > 0
    # the first and the last row subtend fov * (rows - 1) / rows in the tangent-plane formula: tan(half) = (rows - 1) / rows * tan(fov / 2)
    for fov, rows in ((30.0, 37), (100.0, 29), (170.0, 8)):
        cam = V.make_camera(DIMS, (5, 5, 5), (1, 0, 0), fov=fov, size=(rows, 3))
        a, b = cam.light[0, 1].astype(np.float64), cam.light[-1, 1].astype(np.float64)
        got = np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))
        assert abs(got - 2 * np.arctan((rows - 1) / rows * np.tan(np.radians(fov) / 2))) < 1e-6, (fov, rows)
    # an anisotropic voxel_size scales index steps, not physical ones
    a = V.make_camera(DIMS, **dict(OUTSIDE, voxel_size=(1, 1, 1)))
    b = V.make_camera(DIMS, **dict(OUTSIDE, voxel_size=(2, 1, 1), far=100.0, near=3.0))
    assert np.array_equal(a.light, b.light)
    assert np.allclose(b.rays[..., 3].astype(np.float64) * 2, a.rays[..., 3], rtol=1e-6) and np.allclose(b.rays[..., 4:], a.rays[..., 4:], rtol=1e-6)
    assert np.allclose((b.rays[..., :3].astype(np.float64) - np.array(OUTSIDE["eye"])) * np.array([2, 1, 1]), 3.0 * b.light.astype(np.float64), atol=1e-5)
    assert b.depth == int(np.floor((100.0 - 3.0) / 0.5 + 1e-9)) + 1
    # sample k of every ray lies at the physical distance near + k * depth_spacing from the eye
    pos = V.rays_sample_host(b, [0, 36, 7], [0, 44, 9], [0, 194, 50])[0].astype(np.float64) if os.path.exists(_lib.LIB_PATH) else None
    if pos is not None:
        dist = np.linalg.norm((pos - np.array(OUTSIDE["eye"])) * np.array([2, 1, 1]), axis=1)
        assert np.allclose(dist, [3.0, 3.0 + 194 * 0.5, 3.0 + 25.0], rtol=1e-5)


def test_make_camera_refusals():
    ok = dict(eye=(1, 2, 3), direction=(1, 0, 0))
    for kw, words in ((dict(fov=0.0), "fov"), (dict(fov=180.0), "fov"), (dict(fov=float("nan")), "fov"), (dict(eye=(1, float("inf"), 3)), "eye"),
                      (dict(eye=(1, 2)), "eye"), (dict(near=-0.5), "near"), (dict(near=5.0, far=4.0), "far"), (dict(size=(1 << 24, 8)), "2\\^24"),
                      (dict(size=(0, 8)), "at least 1 x 1"), (dict(depth_spacing=1e-6), "depth.*2\\^24"), (dict(depth_spacing=0.0), "depth_spacing"),
                      (dict(region="::2,:,:"), "steps other than 1"), (dict(direction=(0, 0, 0)), "zero vector"),
                      (dict(up=(2, 0, 0)), "parallel"), (dict(voxel_size=(1, 0, 1)), "voxel_size")):
        with pytest.raises(ValueError, match=words):
            V.make_camera(DIMS, **dict(ok, **kw))
    with pytest.raises(ValueError, match="3-D data only"):
        V.make_camera((31, 37), **ok)
    with pytest.raises(ValueError, match="at least 2 voxels"):
        V.make_camera((23, 1, 37), **ok)


# ---- 2: the position rule, each operation rounded on its own
def _np_sample(cam, row, col, k, real=False):
    f = np.float32
    ray = cam.rays[row, col]
    kk = k.astype(f)
    pos = np.stack([ray[:, a] + kk * ray[:, 3 + a] for a in range(3)], 1)
    assert pos.dtype == f
    d = cam.desc
    coord, inside = np.empty_like(pos), np.ones(len(pos), bool)
    for a in range(3):
        n = int(d.dims[a])
        step = f(f(d.hi) - f(d.lo)) / f(n - 1)
        p = pos[:, a].astype(np.float64)
        fma = lambda x, y, z: (np.float64(x) * y + np.float64(z)).astype(f)        # (a product of two floats is exact in a double; one rounding of
        coord[:, a] = np.where(pos[:, a] < f(n // 2), fma(step, p, d.lo), fma(-step, (f(n - 1) - pos[:, a]).astype(np.float64), d.hi))   # the sum: see below)
        inside &= (f(d.box_lo[a]) <= pos[:, a]) & (pos[:, a] <= f(d.box_hi[a]))
    return pos, coord, inside


@needs_lib
@pytest.mark.parametrize("name", list(CAMERAS))
def test_sample_host_equals_the_fp32_restatement(name):
    cam = V.make_camera(DIMS, **CAMERAS[name])
    cam.desc.lo, cam.desc.hi = (-1.0, 1.0) if name != "inside" else (0.0, 1.0)
    row, col, k = (x.ravel() for x in _lattice(cam))
    pos, coord, inside = V.rays_sample_host(cam, row, col, k)
    want_pos, want_coord, want_inside = _np_sample(cam, row, col, k)
    assert np.array_equal(_bits(pos), _bits(want_pos)) and np.array_equal(inside, want_inside)
    # the fma of a coordinate rounds once; float64 holds step * p exactly but its sum with lo rounds before the fp32 rounding: a
    # double rounding can differ from the fma by one ulp, so the coordinate is compared within 1 ulp here and bit for bit against
    # the orthographic header below (test_orthographic_equivalence_on_the_host)
    assert (np.abs(coord.astype(np.float64) - want_coord) <= np.spacing(np.abs(want_coord))).all()
    # at an integer t the real-depth rule is the sample's own
    pos_t, coord_t, inside_t = V.rays_sample_t_host(cam, row, col, k.astype(np.float32))
    assert np.array_equal(_bits(pos_t), _bits(pos)) and np.array_equal(_bits(coord_t), _bits(coord)) and np.array_equal(inside_t, inside)
    # between two samples: p = fl(base + fl(t * dd))
    t = (k[: 500] + np.float32(0.375)).astype(np.float32)
    t = np.minimum(t, np.float32(cam.depth - 1))
    ray = cam.rays[row[:500], col[:500]]
    want = np.stack([ray[:, a] + t * ray[:, 3 + a] for a in range(3)], 1)
    assert np.array_equal(_bits(V.rays_sample_t_host(cam, row[:500], col[:500], t)[0]), _bits(want))


# ---- 3: the ray range is the interval of the inside flags
@needs_lib
@pytest.mark.parametrize("name", list(CAMERAS))
def test_ray_ranges_hold_exactly_the_inside_samples(name):
    cam = V.make_camera(DIMS, **CAMERAS[name])
    k0, cnt = V.rays_clip_host(cam)
    assert k0.dtype == np.int32 and k0.shape == (cam.rows, cam.cols) and (k0 >= 0).all() and (cnt >= 0).all() and (k0 + cnt <= cam.depth).all()
    inside = V.rays_sample_host(cam, *_lattice(cam))[2].reshape(cam.rows, cam.cols, cam.depth)
    kk = np.arange(cam.depth)[None, None, :]
    assert np.array_equal(inside, (kk >= k0[..., None]) & (kk < (k0 + cnt)[..., None]))        # one interval, and exactly the clip's
    assert (k0[cnt == 0] == 0).all()
    hit = cnt > 0
    lanes = V._lanes(cnt.sum() / hit.sum())
    if name == "outside":
        assert cam.rows * cam.cols == 1665 and 0.3 <= hit.mean() <= 0.8 and cnt.sum() >= 10000 and not hit.all() and lanes == 64
        assert not inside[..., 0].any() and not inside[..., -1].any()
    elif name == "inside":
        assert hit.all() and (k0 == 0).all() and (k0 + cnt < cam.depth).all() and cnt.sum() >= 30000
    elif name == "thin":
        assert 1 < cam.depth <= 8 and hit.any() and lanes not in (1, 64)
    elif name == "plane":
        assert cam.depth == 1 and hit.any() and not hit.all() and lanes == 1
    else:
        c = cam.rays[10, 13]
        assert c[3] == 0.0 and c[4] == 0.0 and c[5] == 1.0 and cnt[10, 13] == DIMS[2]        # two step components exactly zero


@needs_lib
def test_a_bad_table_is_refused_on_the_host_and_keeps_the_range_within_depth():
    cam = V.make_camera(DIMS, **CAMERAS["axis"])
    for bad in (np.nan, np.inf):
        broken = V.RayView(cam.desc, cam.rays.copy(), cam.light, cam.near, cam.depth_spacing)
        broken.rays[3, 4, 2] = bad
        with pytest.raises(_lib.BriefError, match="ray table must be finite"):
            V.rays_clip_host(broken)
        with pytest.raises(_lib.BriefError, match="ray table must be finite"):
            V.rays_sample_host(broken, [3], [4], [0])
        V.rays_sample_host(broken, [3], [5], [0])                       # another ray of the same table is served
    # huge but finite entries: positions overflow to inf along the ray; the range still lies within 0 .. depth
    wild = V.RayView(cam.desc, cam.rays.copy(), cam.light, cam.near, cam.depth_spacing)
    wild.rays[..., 3:] *= np.float32(3e38)
    wild.rays[::2, :, :3] = np.float32(-3e38)
    k0, cnt = V.rays_clip_host(wild)
    assert (k0 >= 0).all() and (cnt >= 0).all() and (k0.astype(np.int64) + cnt <= cam.depth).all()


# ---- 4: a table filled from an orthographic view reproduces the orthographic header
@needs_lib
@pytest.mark.parametrize("kw", [OBLIQUE, dict(OBLIQUE, region=BOX, spacing=0.9), dict(direction=(0, -1, 0)), dict(direction=(1, 0, 0), region=BOX)],
                         ids=["oblique", "oblique_box", "aligned", "aligned_box"])
def test_orthographic_equivalence_on_the_host(kw):
    view = V.make_view(DIMS, **kw)
    view.lo, view.hi = -1.0, 1.0
    cam = V.rays_from_view(view)
    assert (cam.rows, cam.cols, cam.depth) == (view.rows, view.cols, view.depth) and cam.near == 0.0 and cam.depth_spacing == 1.0
    assert np.array_equal(cam.rays[..., 3:], np.broadcast_to(np.array(list(view.ddepth), np.float32), cam.rays[..., 3:].shape))
    l = np.array(list(view.ddepth), np.float64)
    assert np.allclose(cam.light.astype(np.float64), l / np.linalg.norm(l), atol=1e-7)
    k0, cnt = V.clip_host(view)
    r0, rcnt = V.rays_clip_host(cam)
    assert np.array_equal(k0, r0) and np.array_equal(cnt, rcnt) and (cnt > 0).any()
    row, col, k = _lattice(cam)
    pos, coord, inside = V.sample_host(view, row, col, k)
    rpos, rcoord, rinside = V.rays_sample_host(cam, row, col, k)
    assert np.array_equal(_bits(pos), _bits(rpos)) and np.array_equal(_bits(coord), _bits(rcoord)) and np.array_equal(inside, rinside)
    t = np.minimum(k.ravel().astype(np.float32) + np.float32(0.3), np.float32(view.depth - 1))
    a, b = V.sample_t_host(view, row, col, t), V.rays_sample_t_host(cam, row, col, t)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


# ---- 5: header, ctypes, exports
ENTRIES = {
    "brief_rays_clip": (["const brief_rays_desc *desc", "const float *rays", "int32_t *k0", "int32_t *cnt", "void *stream"], "rvvvv"),
    "brief_rays_coords": (["const brief_rays_desc *desc", "const float *rays", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1",
                           "int64_t r0", "int64_t r1", "int32_t lanes", "float *coords", "void *stream"], "rvvvllllivv"),
    "brief_rays_fold": (["const brief_rays_desc *desc", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
                         "int64_t r1", "int32_t lanes", "const void *vals", "int elem_kind", "int32_t channels", "int32_t mode", "int32_t *hits",
                         "void *acc", "void *stream"], "rvvllllivniivvv"),
    "brief_rays_surface_fold": (["const brief_rays_desc *desc", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
                                 "int64_t r1", "int32_t lanes", "const void *vals", "int elem_kind", "int32_t channels", "int32_t channel",
                                 "int32_t level", "int32_t side", "int32_t *hits", "int32_t *first", "void *stream"], "rvvllllivniiiivvv"),
    "brief_rays_surface_coords": (["const brief_rays_desc *desc", "const float *rays", "const float *t_lo", "const float *t_hi", "int32_t midpoint",
                                   "float *coords", "float *pos", "void *stream"], "rvvvivvv"),
    "brief_rays_surface_shade": (["const brief_rays_desc *desc", "const float *t", "const float *jac", "int32_t channels", "int32_t channel",
                                  "int32_t side", "const float *gscale", "const float *light", "float *normal", "float *shade", "void *stream"],
                                 "rvviiifvvvv"),
    "brief_rays_sample_host": (["const brief_rays_desc *desc", "const float *rays", "const int32_t *row", "const int32_t *col", "const int32_t *k",
                                "int64_t n", "float *pos", "float *coord", "uint8_t *inside"], "rvvvvlvvv"),
    "brief_rays_sample_t_host": (["const brief_rays_desc *desc", "const float *rays", "const int32_t *row", "const int32_t *col", "const float *t",
                                  "int64_t n", "float *pos", "float *coord", "uint8_t *inside"], "rvvvvlvvv"),
    "brief_rays_clip_host": (["const brief_rays_desc *desc", "const float *rays", "int32_t *k0", "int32_t *cnt"], "rvvv"),
}


def test_header_exports_and_ctypes_signatures_agree():
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    assert "#define BRIEF_VERSION 130" in text
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    codes = {"r": C.POINTER(_lib.RaysDesc), "v": C.c_void_p, "l": C.c_int64, "i": C.c_int32, "n": C.c_int, "f": C.POINTER(C.c_float)}
    declared = sorted(set(re.findall(r"\b(brief_rays_[a-z0-9_]+)\s*\(", plain)))
    assert declared == sorted(ENTRIES)
    for name, (want, sig) in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, plain, flags=re.S)
        assert proto, "%s is not declared in include/brief_hip.h" % name
        assert [" ".join(p.split()) for p in proto.group(1).split(",")] == want, name
        if os.path.exists(_lib.LIB_PATH):
            fn = getattr(_lib.lib(), name)
            assert list(fn.argtypes) == [codes[c] for c in sig], name
            assert fn.restype is C.c_int
    body = re.search(r"typedef struct \{([^}]*)\} brief_rays_desc;", plain, flags=re.S).group(1)
    fields = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.RaysDesc._fields_]
    assert C.sizeof(_lib.RaysDesc) == 24 + 4 * (2 + 4 + 6)
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().brief_version() == 130


@needs_lib
def test_host_entries_refuse_bad_arguments_by_name():
    L = _lib.lib()
    cam = V.make_camera(DIMS, **CAMERAS["axis"])
    for field, value, words in (("depth", 1 << 24, "2\\^24"), ("rows", 0, "2\\^24"), ("lo", float("nan"), "finite")):
        bad = V.RayView(_lib.RaysDesc.from_buffer_copy(cam.desc), cam.rays, cam.light, 0.0, 1.0)
        setattr(bad.desc, field, value)
        with pytest.raises(_lib.BriefError, match=words):
            V.rays_clip_host(bad)
    bad = V.RayView(_lib.RaysDesc.from_buffer_copy(cam.desc), cam.rays, cam.light, 0.0, 1.0)
    bad.desc.box_hi[1] = 31.0
    with pytest.raises(_lib.BriefError, match="clip box"):
        V.rays_sample_host(bad, [0], [0], [0])
    bad.desc.box_hi[1] = 30.0
    bad.desc.dims[2] = 1
    with pytest.raises(_lib.BriefError, match="grid dim"):
        V.rays_sample_host(bad, [0], [0], [0])
    with pytest.raises(_lib.BriefError, match="outside rows x cols x depth"):
        V.rays_sample_host(cam, [0], [cam.cols], [0])
    with pytest.raises(_lib.BriefError, match="outside rows x cols x depth"):
        V.rays_sample_host(cam, [0], [0], [cam.depth])
    with pytest.raises(_lib.BriefError, match="depth - 1"):
        V.rays_sample_t_host(cam, [0], [0], [cam.depth - 0.5])
    with pytest.raises(_lib.BriefError, match="depth - 1"):
        V.rays_sample_t_host(cam, [0], [0], [np.nan])
    k0 = np.zeros(cam.rows * cam.cols, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.brief_rays_clip_host(None, p(cam.rays), p(k0), p(k0)) == -1 and b"null descriptor" in L.brief_last_error()
    assert L.brief_rays_clip_host(C.byref(cam.desc), None, p(k0), p(k0)) == -1 and b"null" in L.brief_last_error()
    assert L.brief_rays_sample_host(C.byref(cam.desc), p(cam.rays), None, p(k0), p(k0), 1, None, None, None) == -1 and b"null" in L.brief_last_error()
    assert L.brief_rays_sample_host(C.byref(cam.desc), p(cam.rays), p(k0), p(k0), p(k0), 1, None, None, None) == 0       # every output may be NULL
    with pytest.raises(ValueError, match="one entry per sample"):
        V.rays_sample_host(cam, [0, 1], [0], [0])


# ---- refusals of the renderers and the artefact entries that need no GPU
def _opt():
    from brief_pytorch_amd import config
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    opt.CompressFramework.Decompress.postprocess.denoise.close = False
    return opt


def _side(**kw):
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


def test_artefact_refusals_are_raised_by_name_before_any_decode(tmp_path):
    from brief_pytorch_amd import framework
    from brief_pytorch_amd.framework import NFGR
    mod = str(tmp_path / "module")
    for cam in (lambda o, s, **kw: NFGR.decompress_camera(o, mod, s, (4, 4, -9), (0, 0, 1), **kw),
                lambda o, s, **kw: framework.decompress_camera_surface(o, mod, s, (4, 4, -9), (0, 0, 1), 100, **kw)):
        with pytest.raises(ValueError, match="camera view of a partition is a follow-up"):
            cam(_opt(), {"data_shape": [8, 8, 8, 1]})
        with pytest.raises(ValueError, match="error-bounded.*error_bound 3"):
            cam(_opt(), _side(error_bound=3))
        with pytest.raises(ValueError, match="3-D data only"):
            cam(_opt(), _side(data_shape=[50, 61, 3]))
        with pytest.raises(ValueError, match="uint8 / uint16 data only.*float32"):
            cam(_opt(), _side(dtype="float32"))
        with pytest.raises(ValueError, match="fov"):
            cam(_opt(), _side(), fov=200)
        with pytest.raises(ValueError, match="outside"):
            cam(_opt(), _side(), region="0:9,:,:")
    view = lambda o, s, **kw: NFGR.decompress_camera(o, mod, s, (4, 4, -9), (0, 0, 1), **kw)
    with pytest.raises(ValueError, match="slice.*out of scope"):
        view(_opt(), _side(), mode="slice")
    with pytest.raises(ValueError, match="not one of"):
        view(_opt(), _side(), mode="median")
    o = _opt()
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    with pytest.raises(ValueError, match="mean view.*does not.*commute"):
        view(o, _side(), mode="mean")
    surface = lambda o, s, **kw: NFGR.decompress_camera_surface(o, mod, s, (4, 4, -9), (0, 0, 1), kw.pop("level", 100), **kw)
    with pytest.raises(ValueError, match="level 70000 lies outside"):
        surface(_opt(), _side(), level=70000)
    with pytest.raises(ValueError, match="analytic Jacobian.*shading=False"):
        surface(_opt(), _side(phi_name="NeRF"))
    os.makedirs(str(tmp_path / "sideinfos"))
    with pytest.raises(ValueError, match="camera view of a partition is a follow-up"):
        view(_opt(), _side())
    assert sorted(os.listdir(str(tmp_path))) == ["sideinfos"]


def test_render_rays_refuses_a_slice_and_other_modes_by_name():
    cam = V.make_camera(DIMS, **CAMERAS["plane"])
    with pytest.raises(ValueError, match="slice.*out of scope"):
        V.render_rays(None, cam, "slice", -1.0, 1.0, "u8", (0.0, 1.0), (0, 255))
    with pytest.raises(ValueError, match="not one of max \\| min \\| mean"):
        V.render_rays(None, cam, "composite", -1.0, 1.0, "u8", (0.0, 1.0), (0, 255))
    with pytest.raises(ValueError, match="out_kind"):
        V.render_rays(None, cam, "max", -1.0, 1.0, "f32", (0.0, 1.0), (0, 255))


# ---- 6: the command line refuses by name and writes nothing
def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


EYE = ["--view", "0.85,0.15,-0.5", "--view-eye=-20,4,52"]      # (a value that begins with a minus sign is attached with `=`)


@pytest.mark.parametrize("extra,words", [
    (["--view-eye", "1,2,3"], ["--view-eye 1,2,3", "--view dz,dy,dx"]),
    (["--view-fov", "40", "--view", "1,0,0"], ["--view-fov", "--view-eye z,y,x"]),
    (["--view-near", "2", "--view", "1,0,0"], ["--view-near", "--view-eye z,y,x"]),
    (["--view-far", "9"], ["--view-far", "--view-eye z,y,x"]),
    (EYE + ["--view-spacing", "2"], ["--view-eye with --view-spacing"]),
    (EYE + ["--view-offset", "2"], ["--view-eye with --view-offset"]),
    (EYE + ["--view-mode", "slice"], ["--view-eye with --view-mode slice", "out of scope"]),
    (EYE + ["--view-composite", "0:0,0,0,0;255:255,255,255,1"], ["--view-eye with --view-composite", "out of scope"]),
    (EYE + ["--view-composite-shade", "0.2,0.8"], ["--view-eye with --view-composite"]),
    (EYE + ["--view-background", "1,2,3"], ["--view-eye with --view-composite"]),
    (EYE + ["--view-owner", "nearest"], ["--view-eye with --view-owner", "a camera view of a partition is a follow-up"]),
    (EYE + ["--mip"], ["--view-eye with --mip"]),
    (EYE + ["--gradient", "magnitude"], ["--view-eye with --gradient"]),
    (EYE + ["--hessian", "laplacian"], ["--view-eye with --hessian"]),
    (EYE + ["--shape", "8,8,8"], ["--view-eye with --shape"]),
    (EYE + ["--step", "2"], ["--view-eye with --step 2"]),
    (["--view", "1,0,0", "--view-eye", "1,2"], ["--view-eye 1,2", "3 comma-separated numbers"]),
    (EYE + ["--view-mode", "mean"], ["--view-mode mean", ".npy only"]),
    (EYE + ["--view-mode", "median"], ["--view-mode median", "unknown mode"]),
    (EYE + ["--view-surface", "100", "--view-mode", "min"], ["--view-surface with --view-mode min"]),
])
def test_cli_refusals_write_nothing(tmp_path, extra, words):
    out = tmp_path / "out" / "view.tif"
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:", "-o", str(out)] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))


def test_cli_refuses_a_divide_artefact(tmp_path):
    os.makedirs(str(tmp_path / "art" / "sideinfos"))
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:",
            "-o", str(tmp_path / "out" / "view.tif")] + EYE
    for extra in ([], ["--view-surface", "100"]):
        with pytest.raises(SystemExit, match="a camera view of a partition is a follow-up"):
            _cli().main(argv + extra)
    assert not os.listdir(str(tmp_path / "out"))
