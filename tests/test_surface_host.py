"""Host side of the surface view (view.render_surface, NFGR.decompress_surface, decompress.py --view-surface): the position at a real
depth t against brief_view_sample_host and a numpy float32 restatement, the C-ABI's declarations, and every refusal that is raised
before a file is read.  Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

from brief_pytorch_amd import _lib, config, gradient
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))
DIMS = (23, 31, 37)

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")


# ---- the position at a real t
def _views():
    a = V.make_view(DIMS, **OBLIQUE)
    b = V.make_view(DIMS, region="3:19,5:26,2:30", **dict(OBLIQUE, spacing=0.9))
    b.lo, b.hi = 0.0, 1.0
    return a, b, V.make_view(DIMS, (0, -1, 0))


@needs_lib
def test_an_integer_t_is_the_sample_itself_bit_for_bit():
    for v in _views():
        row, col, k = (x.ravel() for x in np.meshgrid(np.arange(v.rows), np.arange(v.cols), np.arange(v.depth), indexing="ij"))
        want = V.sample_host(v, row, col, k)
        got = V.sample_t_host(v, row, col, k.astype(np.float32))
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
        assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
        assert np.array_equal(got[2], want[2]) and (want[2].any() and not want[2].all() or v.depth == DIMS[1])


def np_position(v, row, col, t):
    """p_a = fl(base_a + fl(t * ddepth_a)), base_a = fl(fl(origin_a + fl(row * drow_a)) + fl(col * dcol_a)): numpy float32, one rounding
    per operation"""
    f = np.float32
    row, col, t = np.asarray(row).astype(f), np.asarray(col).astype(f), np.asarray(t, f)
    pos = np.empty((len(t), 3), f)
    for a in range(3):
        base = (f(v.origin[a]) + row * f(v.drow[a])) + col * f(v.dcol[a])
        pos[:, a] = base + t * f(v.ddepth[a])
    return pos


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


def exact_coord(v, a, p):
    """brief_view_coord of the float32 position p on axis a, the fma rounded once"""
    f = lambda x: Fr(float(x))
    n = int(v.dims[a])
    step = fl(fl(f(v.hi) - f(v.lo)) / (n - 1))
    return fl(step * f(p) + f(v.lo)) if f(p) < n // 2 else fl(-step * fl((n - 1) - f(p)) + f(v.hi))


@needs_lib
def test_a_fractional_t_is_the_stated_formula():
    rng = np.random.default_rng(7)
    for v in _views():
        n = 4000
        row, col = rng.integers(0, v.rows, n), rng.integers(0, v.cols, n)
        t = (rng.random(n) * (v.depth - 1)).astype(np.float32)
        t[:8] = [0.0, v.depth - 1, 0.5, 1.0 / 3, 2.0 ** -16, v.depth - 1 - 2.0 ** -10, 1.75, 0.999999]
        pos, coord, inside = V.sample_t_host(v, row, col, t)
        want = np_position(v, row, col, t)
        assert np.array_equal(pos.view(np.int32), want.view(np.int32))
        lo, hi = np.array(list(v.box_lo), np.float32), np.array(list(v.box_hi), np.float32)
        assert np.array_equal(inside, ((want >= lo) & (want <= hi)).all(1))
        # the coordinate is brief_view_coord of that position, in exact arithmetic with one rounding per stated operation
        for i in range(300):
            assert [Fr(float(x)) for x in coord[i]] == [exact_coord(v, a, want[i, a]) for a in range(3)], i
        # ... and at positions that are samples it is sample_host's, bit for bit (the first test); between two samples it lies between
        k = np.floor(t).astype(np.int32)
        k1 = np.minimum(k + 1, v.depth - 1)
        c0, c1 = V.sample_host(v, row, col, k)[1], V.sample_host(v, row, col, k1)[1]
        assert ((coord >= np.minimum(c0, c1)) & (coord <= np.maximum(c0, c1))).all()


@needs_lib
def test_the_midpoint_formula_never_leaves_its_bracket():
    """t_mid = fl(t_lo + fl(0.5f * fl(t_hi - t_lo))) as the refinement's numpy restatement computes it"""
    f = np.float32
    rng = np.random.default_rng(3)
    lo = rng.integers(0, 1 << 20, 20000).astype(f)
    hi = lo + f(1)
    for _ in range(V.MAX_REFINE):
        mid = lo + f(0.5) * (hi - lo)
        assert mid.dtype == f and ((lo <= mid) & (mid <= hi)).all()
        up = rng.random(len(lo)) < 0.5
        lo, hi = np.where(up, lo, mid), np.where(up, mid, hi)


@needs_lib
def test_sample_t_host_refuses_a_t_outside_the_ray():
    v = V.make_view(DIMS, **OBLIQUE)
    for t in (-0.25, v.depth - 0.5, np.nan):
        with pytest.raises(_lib.BriefError, match="outside rows x cols x \\[0, depth - 1\\]"):
            V.sample_t_host(v, [0], [0], [t])
    with pytest.raises(ValueError, match="one entry per sample"):
        V.sample_t_host(v, [0, 1], [0], [0.5])


# ---- declarations
ENTRIES = {
    "brief_surface_fold": (["const brief_view_desc *view", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
                            "int64_t r1", "int32_t lanes", "const void *vals", "int elem_kind", "int32_t channels", "int32_t channel",
                            "int32_t level", "int32_t side", "int32_t *hits", "int32_t *first", "void *stream"], "wvvllllivniiiivvv"),
    "brief_surface_bracket": (["const brief_view_desc *view", "const int32_t *k0", "const int32_t *first", "float *t_lo", "float *t_hi",
                               "void *stream"], "wvvvvv"),
    "brief_surface_coords": (["const brief_view_desc *view", "const float *t_lo", "const float *t_hi", "int32_t midpoint", "float *coords",
                              "float *pos", "void *stream"], "wvvivvv"),
    "brief_surface_step": (["const brief_view_desc *view", "const void *vals", "int elem_kind", "int32_t channels", "int32_t channel",
                            "int32_t level", "int32_t side", "float *t_lo", "float *t_hi", "void *stream"], "wvniiiivvv"),
    "brief_surface_shade": (["const brief_view_desc *view", "const float *t", "const float *jac", "int32_t channels", "int32_t channel",
                             "int32_t side", "const float *gscale", "const float *light", "float *normal", "float *shade", "void *stream"],
                            "wvviiiffvvv"),
    "brief_view_sample_t_host": (["const brief_view_desc *view", "const int32_t *row", "const int32_t *col", "const float *t", "int64_t n",
                                  "float *pos", "float *coord", "uint8_t *inside"], "wvvvlvvv"),
}


def test_header_exports_and_ctypes_signatures_agree():
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    assert "#define BRIEF_VERSION 130" in text
    assert "enum { BRIEF_SURFACE_ABOVE = 0, BRIEF_SURFACE_BELOW = 1 };" in text and _lib.SURFACE_SIDE == {"above": 0, "below": 1}
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    codes = {"w": C.POINTER(_lib.ViewDesc), "v": C.c_void_p, "l": C.c_int64, "i": C.c_int32, "n": C.c_int, "f": C.POINTER(C.c_float)}
    for name, (want, sig) in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, plain, flags=re.S)
        assert proto, "%s is not declared in include/brief_hip.h" % name
        assert [" ".join(p.split()) for p in proto.group(1).split(",")] == want, name
        if os.path.exists(_lib.LIB_PATH):
            fn = getattr(_lib.lib(), name)
            assert list(fn.argtypes) == [codes[c] for c in sig], name
            assert fn.restype is C.c_int
    # every entry's contract is written down in the header's surface block
    block = text[text.index("surface view: first-hit depth"):]
    for name in ENTRIES:
        assert block.count(name) >= 2, name
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().brief_version() == 130


# ---- refusals before any file is read
def _opt():
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    opt.CompressFramework.Decompress.postprocess.denoise.close = False
    return opt


def _side(**kw):
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


def test_artefact_refusals_are_raised_by_name_before_any_file_is_read(tmp_path):
    """on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    mod = str(tmp_path / "module")
    surf = lambda o, s, level=30000, **kw: NFGR.decompress_surface(o, mod, s, (1, 0, 0), level, **kw)
    # what check_envelope refuses
    with pytest.raises(ValueError, match="DivideTask.*follow-up"):
        surf(_opt(), {"data_shape": [8, 8, 8, 1]})
    with pytest.raises(ValueError, match="error-bounded.*error_bound 3"):
        surf(_opt(), _side(error_bound=3))
    with pytest.raises(ValueError, match="3-D data only"):
        surf(_opt(), _side(data_shape=[50, 61, 3]))
    with pytest.raises(ValueError, match="uint8 / uint16 data only.*float32"):
        surf(_opt(), _side(dtype="float32"))
    o = _opt()
    o.CompressFramework.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmaxany_a_b.*minmax01"):
        surf(o, _side())
    o = _opt()
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    o.CompressFramework.Decompress.postprocess.denoise.close = [2, 2, 2]
    with pytest.raises(ValueError, match="not local to a voxel"):
        surf(o, _side())
    with pytest.raises(ValueError, match="at least 2 voxels"):
        surf(_opt(), _side(data_shape=[8, 1, 10, 1]))
    # the surface's own arguments
    with pytest.raises(ValueError, match="level 65536 lies outside.*0 \\.\\. 65535"):
        surf(_opt(), _side(), level=65536)
    o = _opt()
    o.CompressFramework.Decompress.postprocess.clip = [0, 255]
    with pytest.raises(ValueError, match="level 256 lies outside.*0 \\.\\. 255"):
        surf(o, _side(dtype="uint8", max=250.0), level=256)
    with pytest.raises(ValueError, match="level -1 lies outside"):
        surf(_opt(), _side(), level=-1)
    with pytest.raises(ValueError, match="integer grey level"):
        surf(_opt(), _side(), level=10.5)
    with pytest.raises(ValueError, match="channel 1 does not exist.*0 \\.\\. 0"):
        surf(_opt(), _side(), channel=1)
    with pytest.raises(ValueError, match="channel -1 does not exist"):
        surf(_opt(), _side(), channel=-1)
    with pytest.raises(ValueError, match="side 'inside' is not one of above \\| below"):
        surf(_opt(), _side(), side="inside")
    for refine in (-1, 17):
        with pytest.raises(ValueError, match="refine must be 0 \\.\\. 16"):
            surf(_opt(), _side(), refine=refine)
    # shading behind a net or a precision without the Jacobian kernel: gradient.refusal's reason
    for kw in (dict(phi_name="NeRF"), dict(phi_precision="bf16"), dict(phi_features=1100), dict(phi_name="SIREN_Pyramid")):
        side = _side(**kw)
        assert not gradient.supported(side["phi_name"], side.get("phi_precision", "fp32"), side["phi_features"])
        why = gradient.refusal(side["phi_name"], side.get("phi_precision", "fp32"), side["phi_features"])
        with pytest.raises(ValueError) as e:
            surf(_opt(), side)
        assert why in str(e.value) and "shading=False" in str(e.value)
    # the geometry's own rules, still before any decode
    with pytest.raises(ValueError, match="zero vector"):
        NFGR.decompress_surface(_opt(), mod, _side(), (0, 0, 0), 30000)
    with pytest.raises(ValueError, match="light must not be the zero vector"):
        surf(_opt(), _side(), light=(0, 0, 0))
    with pytest.raises(ValueError, match="outside"):
        surf(_opt(), _side(), region="0:9,:,:")
    assert not os.listdir(str(tmp_path))
    # with everything in order the next thing it does is to read the module
    with pytest.raises((OSError, FileNotFoundError)):
        surf(_opt(), _side(phi_precision="bf16"), shading=False)


def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VIEW = ["--view", "0.48,-0.6,0.64"]


@pytest.mark.parametrize("extra,words", [
    (["--view-surface", "300"], ["--view-surface", "--view dz,dy,dx"]),                          # without --view
    (["--view-refine", "3"], ["--view-refine", "--view dz,dy,dx"]),
    (VIEW + ["--view-surface", "300", "--view-mode", "min"], ["--view-surface with --view-mode min"]),
    (VIEW + ["--view-surface", "300", "--mip"], ["--view with --mip"]),
    (VIEW + ["--view-surface", "300", "--gradient", "magnitude"], ["--view with --gradient"]),
    (VIEW + ["--view-surface", "300", "--shape", "8,8,8"], ["--view with --shape"]),
    (VIEW + ["--view-surface", "300", "--step", "2"], ["--view with --step 2"]),
    (VIEW + ["--view-surface", "300", "--view-offset", "2"], ["--view-surface with --view-offset"]),
    (VIEW + ["--view-refine", "3"], ["--view-refine", "--view-surface LEVEL"]),                    # surface options without a level
    (VIEW + ["--view-surface-side", "below"], ["--view-surface-side", "--view-surface LEVEL"]),
    (VIEW + ["--view-channel", "1"], ["--view-channel", "--view-surface LEVEL"]),
    (VIEW + ["--view-light", "1,0,0"], ["--view-light", "--view-surface LEVEL"]),
    (VIEW + ["--view-surface", "300", "--view-surface-side", "inside"], ["--view-surface-side inside", "above"]),
    (VIEW + ["--view-surface", "300", "--view-refine", "17"], ["--view-refine 17", "0 .. 16"]),
    (VIEW + ["--view-surface", "70000"], ["--view-surface 70000", "0 .. 65535"]),
    (VIEW + ["--view-surface", "300", "--view-channel", "-1"], ["--view-channel -1"]),
    (VIEW + ["--view-surface", "300", "--view-light", "1,0"], ["--view-light 1,0", "3 comma-separated numbers"]),
])
def test_cli_refusals_write_nothing(tmp_path, extra, words):
    out = tmp_path / "out" / "surface.png"
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
            "-o", str(tmp_path / "out" / "surface.png")] + VIEW + ["--view-surface", "300"]
    with pytest.raises(SystemExit, match="DivideTask"):
        _cli().main(argv)
    assert not os.listdir(str(tmp_path / "out"))
