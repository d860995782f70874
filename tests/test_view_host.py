"""Host side of the view decode (brief_pytorch_amd/view.py, decompress.py --view): the geometry of csrc/brief_view.h against exact
arithmetic, make_view, the refusals, the C-ABI's declaration.  Nothing here needs a GPU: brief_view_sample_host and brief_view_clip_host
run the header the kernels run, on the host CPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

from brief_pytorch_amd import _lib, config
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))
DIMS = (23, 31, 37)

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")


# ---- exact arithmetic: one correctly rounded fp32 result per stated operation
def fl(x):
    """the float32 nearest to the rational x (ties to even), as a Fraction"""
    x = Fr(x)
    if x == 0:
        return x
    e = 0
    while abs(x) >= Fr(2) ** (e + 1):
        e += 1
    while abs(x) < Fr(2) ** e:
        e -= 1
    q = Fr(2) ** (max(e, -126) - 23)
    n = x / q
    f = n.numerator // n.denominator
    r = n - f
    if r > Fr(1, 2) or (r == Fr(1, 2) and f % 2 == 1):
        f += 1
    return f * q


def test_fl_is_float32_rounding():
    rng = np.random.default_rng(0)
    for x in np.concatenate([rng.standard_normal(50) * 1e3, [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -130, 16777217.0]]):
        assert fl(Fr(float(x))) == Fr(float(np.float32(x))), x


def _exact(v, row, col, k):
    """(pos, coord, inside) of one sample from the descriptor's own floats, every operation of csrc/brief_view.h rounded once"""
    f = lambda x: Fr(float(x))
    pos, coord, inside = [], [], True
    for a in range(3):
        p = fl(fl(fl(f(v.origin[a]) + fl(row * f(v.drow[a]))) + fl(col * f(v.dcol[a]))) + fl(k * f(v.ddepth[a])))
        n = int(v.dims[a])
        step = fl(fl(f(v.hi) - f(v.lo)) / (n - 1))
        x = fl(step * p + f(v.lo)) if p < n // 2 else fl(-step * fl((n - 1) - p) + f(v.hi))
        inside = inside and f(v.box_lo[a]) <= p <= f(v.box_hi[a])
        pos.append(p)
        coord.append(x)
    return pos, coord, inside


@needs_lib
@pytest.mark.parametrize("name", ["oblique", "aligned", "oblique_box"])
def test_geometry_against_exact_arithmetic(name):
    kw = {"oblique": OBLIQUE, "aligned": dict(direction=(0, -1, 0)), "oblique_box": dict(OBLIQUE, region="3:19,5:26,:30", spacing=0.9)}[name]
    v = V.make_view(DIMS, **kw)
    v.lo, v.hi = (-1.0, 1.0) if name != "oblique_box" else (0.0, 1.0)
    rng = np.random.default_rng(5)
    n = 200
    row, col, k = rng.integers(0, v.rows, n), rng.integers(0, v.cols, n), rng.integers(0, v.depth, n)
    pos, coord, inside = V.sample_host(v, row, col, k)
    seen = set()
    for i in range(n):
        p, x, ins = _exact(v, int(row[i]), int(col[i]), int(k[i]))
        assert [Fr(float(t)) for t in pos[i]] == p, (i, pos[i], [float(t) for t in p])
        assert [Fr(float(t)) for t in coord[i]] == x, (i, coord[i], [float(t) for t in x])
        assert bool(inside[i]) == ins, i
        seen.add(ins)
    assert seen == {True, False} or name == "aligned"      # (an axis-aligned view of the whole grid has no sample outside)


@needs_lib
@pytest.mark.parametrize("name", ["oblique", "oblique_box", "skim"])
def test_ray_ranges_hold_exactly_the_inside_samples(name):
    """brief_view_clip_host (the bisection of brief_view_ray_range) against the inside flag of every sample of every ray; 'skim': a
    direction a hair off an axis, whose rays run along two faces of the box for thousands of samples' worth of rounding"""
    kw = {"oblique": OBLIQUE, "oblique_box": dict(OBLIQUE, region="3:19,5:26,:30", spacing=0.9),
          "skim": dict(direction=(1.0, 1e-5, -3e-6), spacing=1.0, depth_spacing=0.25)}[name]
    v = V.make_view(DIMS, **kw)
    k0, cnt = V.clip_host(v)
    row, col, k = np.meshgrid(np.arange(v.rows), np.arange(v.cols), np.arange(v.depth), indexing="ij")
    inside = V.sample_host(v, row, col, k)[2].reshape(v.rows, v.cols, v.depth)
    kk = np.arange(v.depth)[None, None, :]
    assert np.array_equal(inside, (kk >= k0[..., None]) & (kk < (k0 + cnt)[..., None]))
    assert (k0[cnt == 0] == 0).all() and (cnt > 0).any()


@needs_lib
@pytest.mark.parametrize("direction,perm", [((1, 0, 0), (2, 0, 1)), ((0, -1, 0), (0, 2, 1)), ((0, 0, 1), (0, 1, 2))])
@pytest.mark.parametrize("lohi", [(-1.0, 1.0), (0.0, 1.0)])
def test_axis_aligned_view_reproduces_the_grid(direction, perm, lohi):
    """unit spacing along an axis: every sample sits on a voxel, on both sides of n / 2, and its coordinates are the grid's own bits"""
    dims = (5, 6, 7)
    v = V.make_view(dims, direction)
    v.lo, v.hi = lohi
    row, col, k = np.meshgrid(np.arange(v.rows), np.arange(v.cols), np.arange(v.depth), indexing="ij")
    pos, coord, inside = V.sample_host(v, row, col, k)
    assert inside.all() and v.rows * v.cols * v.depth == int(np.prod(dims))
    assert np.array_equal(pos, np.round(pos))
    idx = pos.astype(np.int64)
    assert len({tuple(i) for i in idx}) == len(idx) and (idx.min(0) == 0).all() and (idx.max(0) == np.array(dims) - 1).all()
    grid = O.grid_coords(dims, *lohi).reshape(*dims, 3)
    assert np.array_equal(coord.view(np.int32), grid[idx[:, 0], idx[:, 1], idx[:, 2]].view(np.int32))
    # the image axes are those of mip_ops' image for that direction: (row, col, k) -> (z, y, x) by `perm`
    lattice = np.stack([row.ravel(), col.ravel(), k.ravel()], 1)
    want = lattice[:, list(perm)]
    if direction == (0, -1, 0):
        want[:, 1] = dims[1] - 1 - want[:, 1]                    # looking along -y: k counts down the axis
    assert np.array_equal(idx, want)


def test_make_view_frame_size_and_scaling():
    f32 = lambda a: np.array(list(a), np.float64)
    v = V.make_view(DIMS, **OBLIQUE)
    vs = np.array(OBLIQUE["voxel_size"], np.float64)
    r, c, d = f32(v.drow) * vs, f32(v.dcol) * vs, f32(v.ddepth) * vs          # back to physical steps
    for a, b in ((r, c), (r, d), (c, d)):
        assert abs(np.dot(a, b)) < 1e-6
    assert np.allclose([np.linalg.norm(r), np.linalg.norm(c), np.linalg.norm(d)], [1.7, 1.7, 0.5], rtol=1e-6)
    assert np.allclose(d / np.linalg.norm(d), np.array(OBLIQUE["direction"]) / np.linalg.norm(OBLIQUE["direction"]), atol=1e-6)
    assert np.dot(np.cross(d, r), c) > 0                                     # a proper rotation: never mirrored
    # the default size covers the clip box: every corner of it projects onto the image and into the depth range
    for region in (None, "3:19,5:26,:30"):
        v = V.make_view(DIMS, region=region, **OBLIQUE)
        lo, hi = f32(v.box_lo), f32(v.box_hi)
        m = np.stack([f32(v.drow), f32(v.dcol), f32(v.ddepth)], 1)
        for i in range(8):
            corner = np.array([(lo, hi)[(i >> a) & 1][a] for a in range(3)])
            t = np.linalg.solve(m, corner - f32(v.origin))
            assert (t > -1e-3).all() and (t < np.array([v.rows, v.cols, v.depth]) - 1 + 1 + 1e-3).all(), (region, corner, t)
        smaller = V.make_view(DIMS, region=region, **dict(OBLIQUE, spacing=3.4))
        assert smaller.rows in (v.rows // 2, v.rows // 2 + 1) and smaller.cols in (v.cols // 2, v.cols // 2 + 1)
    # voxel_size divides the steps per axis; the direction is physical
    a = V.make_view(DIMS, (1, 1, 0), voxel_size=(1, 1, 1))
    b = V.make_view(DIMS, (1, 1, 0), voxel_size=(2, 1, 1))
    assert np.allclose(f32(a.ddepth), [2 ** -0.5, 2 ** -0.5, 0]) and np.allclose(f32(b.ddepth), [2 ** -0.5 / 2, 2 ** -0.5, 0])
    # an explicit size is centred on the centre; a single depth is one plane
    v = V.make_view(DIMS, (1, 0, 0), size=(5, 9), depth=2.0, centre=(10, 15, 18))
    assert (v.rows, v.cols, v.depth) == (5, 9, 1) and list(v.origin) == [12.0, 13.0, 14.0]
    v = V.make_view(DIMS, (1, 0, 0), region="2:9,:,:")
    assert (v.rows, v.cols, v.depth) == (31, 37, 7) and list(v.origin) == [2.0, 0.0, 0.0] and list(v.box_lo) == [2.0, 0.0, 0.0] \
        and list(v.box_hi) == [8.0, 30.0, 36.0]


def test_make_view_refusals():
    with pytest.raises(ValueError, match="zero vector"):
        V.make_view(DIMS, (0, 0, 0))
    with pytest.raises(ValueError, match="parallel"):
        V.make_view(DIMS, (0, 1, 1), up=(0, -2, -2))
    with pytest.raises(ValueError, match="steps other than 1"):
        V.make_view(DIMS, (1, 0, 0), region="::2,:,:")
    with pytest.raises(ValueError, match="2\\^24"):
        V.make_view(DIMS, (1, 0, 0), size=(1 << 24, 8))
    with pytest.raises(ValueError, match="2\\^24"):
        V.make_view(DIMS, (1, 0, 0), spacing=1e-6)
    with pytest.raises(ValueError, match="2\\^24"):
        V.make_view(DIMS, (1, 0, 0), depth_spacing=1e-6)
    with pytest.raises(ValueError, match="at least 2 voxels"):
        V.make_view((1, 31, 37), (1, 0, 0))
    with pytest.raises(ValueError, match="3-D data only"):
        V.make_view((31, 37), (1, 0, 0))
    with pytest.raises(ValueError, match="outside"):
        V.make_view(DIMS, (1, 0, 0), region="0:24,:,:")


@needs_lib
def test_library_refuses_a_bad_descriptor():
    v = V.make_view(DIMS, (1, 0, 0))
    v.depth = 1 << 24
    with pytest.raises(_lib.BriefError, match="2\\^24"):
        V.clip_host(v)
    v = V.make_view(DIMS, (1, 0, 0))
    v.box_hi[1] = 31.0
    with pytest.raises(_lib.BriefError, match="clip box"):
        V.sample_host(v, [0], [0], [0])
    v = V.make_view(DIMS, (1, 0, 0))
    with pytest.raises(_lib.BriefError, match="outside rows x cols x depth"):
        V.sample_host(v, [0], [v.cols], [0])


ENTRIES = {
    "brief_view_clip": (["const brief_view_desc *view", "int32_t *k0", "int32_t *cnt", "void *stream"], "wvvv"),
    "brief_view_coords": (["const brief_view_desc *view", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
                           "int64_t r1", "int32_t lanes", "float *coords", "void *stream"], "wvvllllivv"),
    "brief_view_fold": (["const brief_view_desc *view", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
                         "int64_t r1", "int32_t lanes", "const void *vals", "int elem_kind", "int32_t channels", "int32_t mode", "int32_t *hits",
                         "void *acc", "void *stream"], "wvvllllivniivvv"),
    "brief_view_finish": (["const brief_view_desc *view", "int elem_kind", "int32_t channels", "int32_t mode", "const int32_t *hits",
                           "const void *acc", "void *out", "void *stream"], "wniivvvv"),
    "brief_view_sample_host": (["const brief_view_desc *view", "const int32_t *row", "const int32_t *col", "const int32_t *k", "int64_t n",
                                "float *pos", "float *coord", "uint8_t *inside"], "wvvvlvvv"),
    "brief_view_clip_host": (["const brief_view_desc *view", "int32_t *k0", "int32_t *cnt"], "wvv"),
}


def test_header_exports_and_ctypes_signatures_agree():
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    assert "#define BRIEF_VERSION 130" in text
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    codes = {"w": C.POINTER(_lib.ViewDesc), "v": C.c_void_p, "l": C.c_int64, "i": C.c_int32, "n": C.c_int}
    for name, (want, sig) in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, plain, flags=re.S)
        assert proto, "%s is not declared in include/brief_hip.h" % name
        assert [" ".join(p.split()) for p in proto.group(1).split(",")] == want, name
        if os.path.exists(_lib.LIB_PATH):                        # the signature the loaded library was given
            fn = getattr(_lib.lib(), name)
            assert list(fn.argtypes) == [codes[c] for c in sig], name
            assert fn.restype is C.c_int
    # the struct as the header lays it out: 8 + 2 + 12 floats / ints behind three int64, no padding
    body = re.search(r"typedef struct \{([^}]*)\} brief_view_desc;", plain, flags=re.S).group(1)
    fields = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.ViewDesc._fields_]
    assert C.sizeof(_lib.ViewDesc) == 24 + 4 * (2 + 12 + 4 + 6)
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().brief_version() == 130


# ---- refusals
def _opt():
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    opt.CompressFramework.Decompress.postprocess.denoise.close = False
    return opt


def _side(**kw):
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


def test_artefact_refusals_are_raised_by_name_before_any_decode(tmp_path):
    """each on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    mod = str(tmp_path / "module")
    view = lambda o, s, **kw: NFGR.decompress_view(o, mod, s, (1, 0, 0), **kw)
    with pytest.raises(ValueError, match="DivideTask.*follow-up"):
        view(_opt(), {"data_shape": [8, 8, 8, 1]})
    with pytest.raises(ValueError, match="error-bounded.*error_bound 3.*fitted grid \\[8, 9, 10\\] only"):
        view(_opt(), _side(error_bound=3))
    with pytest.raises(ValueError, match="3-D data only"):
        view(_opt(), _side(data_shape=[50, 61, 3]))
    with pytest.raises(ValueError, match="uint8 / uint16 data only.*float32"):
        view(_opt(), _side(dtype="float32"))
    o = _opt()
    o.CompressFramework.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmaxany_a_b.*minmax01"):
        view(o, _side())
    o = _opt()
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    o.CompressFramework.Decompress.postprocess.denoise.close = [2, 2, 2]
    with pytest.raises(ValueError, match="not local to a voxel"):
        view(o, _side())
    with pytest.raises(ValueError, match="at least 2 voxels"):
        view(_opt(), _side(data_shape=[8, 1, 10, 1]))
    o = _opt()
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    with pytest.raises(ValueError, match="mean view.*does not.*commute"):
        view(o, _side(), mode="mean")
    with pytest.raises(ValueError, match="not one of"):
        view(_opt(), _side(), mode="median")
    # the geometry's and the region's own rules, still before any decode
    with pytest.raises(ValueError, match="outside"):
        view(_opt(), _side(), region="0:9,:,:")
    with pytest.raises(ValueError, match="zero vector"):
        NFGR.decompress_view(_opt(), mod, _side(), (0, 0, 0))
    with pytest.raises(ValueError, match="offset"):
        view(_opt(), _side(), mode="max", offset=1.0)
    # a DivideTask artefact on disk: blocks beside the module directory
    os.makedirs(str(tmp_path / "sideinfos" / "d_0_3-h_0_7-w_0_7"))
    with pytest.raises(ValueError, match="DivideTask"):
        view(_opt(), _side())
    assert sorted(os.listdir(str(tmp_path))) == ["sideinfos"]


def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,words", [
    (["--mip"], ["--view with --mip"]),
    (["--gradient", "magnitude"], ["--view with --gradient"]),
    (["--shape", "8,8,8"], ["--view with --shape"]),
    (["--step", "2"], ["--view with --step 2"]),
    (["--view-mode", "mean"], ["--view-mode mean", ".npy only", ".tif"]),
    (["--view-mode", "median"], ["--view-mode median", "unknown mode"]),
    (["--view-mode", "min", "--view-offset", "2"], ["--view-offset", "slice"]),
    (["--view-up", "1,0"], ["--view-up 1,0", "3 comma-separated numbers"]),
])
def test_cli_refusals_write_nothing(tmp_path, extra, words):
    out = tmp_path / "out" / "view.tif"
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:", "--view", "0.48,-0.6,0.64",
            "-o", str(out)] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))


def test_cli_refuses_a_divide_artefact_and_stray_view_options(tmp_path):
    os.makedirs(str(tmp_path / "art" / "sideinfos"))
    os.makedirs(str(tmp_path / "out"))
    base = [sys.executable, os.path.join(ROOT, "decompress.py"), "-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"),
            "--region", ":,:,:", "-o", str(tmp_path / "out" / "view.tif")]
    r = subprocess.run(base + ["--view", "1,0,0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--view" in r.stderr and "DivideTask" in r.stderr and "follow-up" in r.stderr
    with pytest.raises(SystemExit, match="describe a --view"):
        _cli().main(base[2:] + ["--view-mode", "slice"])
    assert not os.listdir(str(tmp_path / "out"))
