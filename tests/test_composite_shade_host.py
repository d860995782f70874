"""Host side of the shaded composite (composite.render_composite with shade, decompress.py --view-composite-shade): the Lambert term
of csrc/brief_composite.h against a numpy fp32 restatement and against float64, brief_view_composite_shade_host against a
restatement in Python integers, the identity with the plain composite, and the refusals of the entries, the Python calls and the CLI.
Nothing here needs a GPU: the host entries run the header the kernels run, on the host CPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from brief_pytorch_amd import _lib, config
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR
from tests._composite import TAU_SAT, W, finish, random_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (8, 9, 10)
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=0.9, depth_spacing=0.7, voxel_size=(2, 1, 1))
GSCALE = (310.5, 977.25, -1204.0)
LIGHT = tuple(np.array([0.48, -0.6, 0.64]) / np.linalg.norm([0.48, -0.6, 0.64]))

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")
f32 = np.float32


# ---- the Lambert term
def _cos_q(jac, gscale, light):
    """c_q of the header, restated in numpy float32: every operation rounds on its own (numpy fuses nothing)"""
    j, gs, l = np.asarray(jac, f32), np.asarray(gscale, f32), np.asarray(light, f32)
    with np.errstate(all="ignore"):
        g = [j[:, a] * gs[a] for a in range(3)]
        d = (g[0] * l[0] + g[1] * l[1]) + g[2] * l[2]
        q = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        length = np.sqrt(q)
        u = (np.abs(d) / length) * f32(256) + f32(0.5)
        assert all(x.dtype == f32 for x in (d, q, length, u))
        lit = (length > 0) & np.isfinite(length) & (u < f32(256))
        return np.where(lit, np.where(lit, u, 0).astype(np.int32), 256).astype(np.int32)


def _shade_q(jac, gscale, light, ka_q, kd_q):
    return np.minimum(256, ka_q + ((kd_q * _cos_q(jac, gscale, light).astype(np.int64) + 128) >> 8)).astype(np.int32)


def _rows(rng):
    """Jacobian rows: random ones over many magnitudes, zero, denormal, +-inf, NaN, huge, near-axis-aligned, and rows orthogonal and
    parallel to the light"""
    tiny = np.finfo(f32).tiny
    special = np.array([[0, 0, 0], [-0.0, 0, 0], [tiny / 4, 0, 0], [tiny / 8, -tiny / 2, tiny / 16], [1e-30, 1e-30, 1e-30],
                        [np.inf, 1, 1], [1, -np.inf, 0], [np.inf, np.inf, -np.inf], [np.nan, 1, 1], [1, 2, np.nan], [3e38, 3e38, 3e38],
                        [1e30, -1e30, 1e30], [1e15, 0, 0], [1, 1e-7, 0], [1e-7, 1, 1e-8], [0, 1e-9, 1], [1, 0, 0], [0, -1, 0], [0, 0, 1],
                        [0.6 / 310.5, 0.48 / 977.25, 0], [0.48 / 310.5, -0.6 / 977.25, 0.64 / -1204.0]], f32)
    rand = (rng.standard_normal((4000, 3)) * 10.0 ** rng.integers(-12, 9, (4000, 1))).astype(f32)
    axis = rand[:300].copy()
    axis[np.arange(300), rng.integers(0, 3, 300)] *= f32(1e6)
    return np.concatenate([special, rand, axis])


@needs_lib
def test_shade_q_equals_the_numpy_fp32_restatement_bit_for_bit():
    jac = _rows(np.random.default_rng(1))
    for gscale, light in ((GSCALE, LIGHT), ((1, 1, 1), (1, 0, 0)), ((2e-20, 5e10, -3.0), (0, -0.6, 0.8)), ((0, 0, 0), LIGHT), (GSCALE, (0, 0, 0))):
        c = CP.shade_q_host(jac, gscale, light, 0, 256)            # ka_q = 0, kd_q = 256: s_q is c_q itself
        want = _cos_q(jac, gscale, light)
        assert c.dtype == np.int32 and np.array_equal(c, want), np.flatnonzero(c != want)[:5]
        assert c.min() >= 0 and c.max() == 256
        for ka_q, kd_q in ((77, 179), (256, 256), (0, 0), (256, 0), (13, 1), (0, 255)):
            assert np.array_equal(CP.shade_q_host(jac, gscale, light, ka_q, kd_q), _shade_q(jac, gscale, light, ka_q, kd_q)), (ka_q, kd_q)
    c = CP.shade_q_host(jac, GSCALE, LIGHT, 0, 256)
    # a row without a direction is lit fully: zero, denormals whose squares vanish, inf, NaN, a length that overflows
    assert (c[:12] == 256).all() and c[12] < 256
    assert c[19] == 0 and c[20] == 256, "orthogonal to the light, and along it"
    assert len(np.unique(c)) >= 200, "most values of c_q occur"
    assert (CP.shade_q_host(jac, GSCALE, LIGHT, 256, 0) == 256).all() and (CP.shade_q_host(jac, GSCALE, LIGHT, 0, 0) == 0).all()


@needs_lib
def test_cos_q_is_within_one_of_float64_and_two_sided():
    rng = np.random.default_rng(2)
    jac = (rng.standard_normal((20000, 3)) * 10.0 ** rng.integers(-6, 6, (20000, 1))).astype(f32)
    light = np.asarray(LIGHT, f32)
    c = CP.shade_q_host(jac, GSCALE, light, 0, 256)
    g = jac.astype(np.float64) * np.asarray(GSCALE, f32).astype(np.float64)
    cos = np.abs(g @ light.astype(np.float64)) / np.linalg.norm(g, axis=1)
    # every fp32 step is within half an ulp of a value at most 257: together far below 1e-3 of a level; the rounding to an integer adds 1/2
    assert np.abs(c - 256.0 * cos).max() <= 1.0 and np.abs(c - 256.0 * cos).max() > 0.4
    assert np.array_equal(CP.shade_q_host(jac, GSCALE, -light, 0, 256), c), "light and -light give the same values"
    assert np.array_equal(CP.shade_q_host(-jac, GSCALE, light, 0, 256), c)
    assert np.array_equal(CP.shade_q_host(jac, GSCALE, -light, 40, 200), CP.shade_q_host(jac, GSCALE, light, 40, 200))


# ---- brief_view_composite_shade_host against Python integers
def _table(rng, bits):
    """random_table with what the selection rule reads: rows that absorb without emitting, rows that emit without absorbing"""
    tf = random_table(rng, bits)
    n = len(tf)
    dark = rng.random(n) < 0.3
    tf[dark, 1:] = 0
    if n >= 8:
        tf[rng.permutation(n)[:max(1, n // 8)], 0] = 0
    return tf


def _restate(view, k0, off, vals, tf, jac, channel, bg, gscale, light, ka_q, kd_q):
    rays = view.rows * view.cols
    shift = 8 * vals.dtype.itemsize - (len(tf).bit_length() - 1)
    cnt = np.diff(off)
    r = np.repeat(np.arange(rays), cnt)
    k = np.repeat(k0, cnt) + (np.arange(int(off[-1])) - np.repeat(off[:-1], cnt))
    inside = V.sample_host(view, r // view.cols, r % view.cols, k)[2]
    s_q = _shade_q(jac[:, channel], gscale, light, ka_q, kd_q)
    img, hits, runs, accs = np.zeros((rays, 4), np.uint8), np.zeros(rays, np.int32), np.zeros(rays, np.int32), np.zeros((rays, 3), np.uint64)
    need, behind = np.zeros(int(off[-1]), np.int32), np.zeros(int(off[-1]), bool)
    for ray in range(rays):
        run, acc, n = 0, [0, 0, 0], 0
        for s in range(int(off[ray]), int(off[ray + 1])):
            if not inside[s]:
                continue
            n += 1
            tau, *e = (int(x) for x in tf[int(vals[s, channel]) >> shift])
            behind[s] = run >= TAU_SAT
            if any(e) and run < TAU_SAT:
                need[s] = 1
                acc = [a + W(run) * ((x * int(s_q[s]) + 128) >> 8) for a, x in zip(acc, e)]
            run = min(run + tau, TAU_SAT)
        img[ray] = finish(run, acc, bg)
        hits[ray], runs[ray], accs[ray] = n, run, [a % (1 << 64) for a in acc]
    shape = (view.rows, view.cols)
    return (img.reshape(*shape, 4), hits.reshape(shape), runs.reshape(shape), accs.reshape(*shape, 3), need), inside, behind


def _lists(rng, view, dtype, channels):
    rays = view.rows * view.cols
    cnt = rng.integers(0, view.depth + 1, rays).astype(np.int32)
    cnt[rng.random(rays) < 0.2] = 0
    cnt[rng.random(rays) < 0.1] = 1
    k0 = (rng.random(rays) * (view.depth - cnt + 1)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    vals = rng.integers(0, np.iinfo(dtype).max + 1, (int(off[-1]), channels)).astype(dtype)
    jac = (rng.standard_normal((int(off[-1]), channels, 3)) * 10.0 ** rng.integers(-3, 3, (int(off[-1]), 1, 1))).astype(f32)
    return k0, cnt, off, vals, jac


@needs_lib
@pytest.mark.parametrize("dtype,channels,channel,bits", [(np.uint8, 1, 0, 8), (np.uint8, 2, 1, 5), (np.uint16, 1, 0, 12), (np.uint16, 2, 1, 16),
                                                         (np.uint16, 3, 2, 4)])
def test_host_shaded_composite_equals_python_integers(dtype, channels, channel, bits):
    rng = np.random.default_rng(bits * 11 + channels)
    view = V.make_view(DIMS, **OBLIQUE)
    tf = _table(rng, bits)
    bg = (12, 200, 255)
    k0, cnt, off, vals, jac = _lists(rng, view, dtype, channels)
    assert (cnt == 0).any() and (cnt == 1).any() and cnt.max() > 8
    plain = CP.composite_host(view, k0, off, vals, tf, channel=channel, background=bg)
    for ka_q, kd_q in ((51, 205), (0, 256)):
        got = CP.composite_shade_host(view, k0, off, vals, tf, jac, GSCALE, LIGHT, ka_q, kd_q, channel=channel, background=bg)
        want, inside, behind = _restate(view, k0, off, vals, tf, jac, channel, bg, GSCALE, LIGHT, ka_q, kd_q)
        for g, w, what in zip(got, want, ("image", "hits", "tau_run", "acc", "need")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, ka_q, kd_q)
        img, hits, run, acc, need = got
        # opacity is the plain composite's: hits, tau_run and A, bit for bit; the colours are not
        assert np.array_equal(hits, plain[1]) and np.array_equal(run, plain[2]) and np.array_equal(img[..., 3], plain[0][..., 3])
        assert (acc <= plain[3]).all() and (acc < plain[3]).any() and not np.array_equal(img, plain[0])
        # the selection: nothing outside the box, nothing behind a saturated prefix, nothing that emits nothing; and each kind occurs
        assert not need[~inside].any() and (~inside).any()
        assert not need[behind].any() and behind.sum() > 20, "no sample behind a saturated prefix: rays do not saturate midway"
        assert 0 < need.sum() < inside.sum() - behind.sum(), "no inside sample in front of saturation emits nothing"
        assert (run == TAU_SAT).any() and ((run > 0) & (run < TAU_SAT)).any() and (hits == 0).any() and (hits == 1).any()


@needs_lib
@pytest.mark.parametrize("dtype,channels,channel,bits", [(np.uint8, 2, 1, 8), (np.uint16, 1, 0, 12)])
def test_full_ambient_and_no_diffuse_is_the_plain_composite_whatever_the_jacobian_holds(dtype, channels, channel, bits):
    rng = np.random.default_rng(bits)
    view = V.make_view(DIMS, **OBLIQUE)
    tf = _table(rng, bits)
    k0, cnt, off, vals, jac = _lists(rng, view, dtype, channels)
    jac[rng.random(len(jac)) < 0.3] = np.nan
    jac[rng.random(len(jac)) < 0.1] = np.inf
    jac[rng.random(len(jac)) < 0.1] = 0
    plain = CP.composite_host(view, k0, off, vals, tf, channel=channel, background=(1, 2, 3))
    got = CP.composite_shade_host(view, k0, off, vals, tf, jac, GSCALE, LIGHT, 256, 0, channel=channel, background=(1, 2, 3))
    for g, w, what in zip(got[:4], plain, ("image", "hits", "tau_run", "acc")):
        assert np.array_equal(g, w), what
    assert 0 < got[4].sum() < len(vals) and len(np.unique(got[0][..., :3])) > 20
    # a sample without a gradient direction is lit fully: a NaN Jacobian under any weights is ka + kd, clamped
    nan = np.full_like(jac, np.nan)
    full = CP.composite_shade_host(view, k0, off, vals, tf, nan, GSCALE, LIGHT, 100, 200, channel=channel, background=(1, 2, 3))
    assert np.array_equal(full[0], plain[0]) and np.array_equal(full[3], plain[3])


# ---- refusals of the entries
@needs_lib
def test_host_entries_refuse_bad_arguments_by_name():
    L = _lib.lib()
    view = V.make_view(DIMS, (1, 0, 0))
    rays = view.rows * view.cols
    k0, off = np.zeros(rays, np.int32), np.arange(rays + 1, dtype=np.int64)
    vals, out = np.zeros((rays, 2), np.uint8), np.zeros((rays, 4), np.uint8)
    jac = np.ones((rays, 2, 3), f32)
    tf = np.zeros((256, 4), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    bg = (C.c_int32 * 3)(0, 0, 0)

    def shade(gscale=GSCALE, light=LIGHT, ka_q=100, kd_q=100):
        sh = _lib.CompositeShade()
        sh.gscale[:], sh.light[:], sh.ka_q, sh.kd_q = gscale, light, ka_q, kd_q
        return sh

    def call(k0=k0, vals=vals, jac=jac, tf=tf, out=out, sh=shade(), channel=1, off=off):
        return L.brief_view_composite_shade_host(C.byref(view), p(k0), p(off), p(vals), _lib.OUT_U8, 2, channel, p(tf), 8, bg, p(jac),
                                                 C.byref(sh) if sh is not None else None, None, None, None, None, p(out))
    assert call() == 0
    off2 = off.copy()
    off2[0] = 1
    bad_tau = tf.copy()
    bad_tau[3, 0] = TAU_SAT + 1
    for kw, what in ((dict(k0=None), "null buffer"), (dict(vals=None), "null buffer"), (dict(jac=None), "null buffer"), (dict(out=None), "null buffer"),
                     (dict(sh=None), "null shade descriptor"), (dict(tf=None), "null transfer table"), (dict(channel=2), "channel must be 0 .. channels - 1"),
                     (dict(sh=shade(ka_q=257)), "ka_q and kd_q must be 0 .. 256"), (dict(sh=shade(ka_q=-1)), "ka_q and kd_q must be 0 .. 256"),
                     (dict(sh=shade(kd_q=257)), "ka_q and kd_q must be 0 .. 256"), (dict(sh=shade(kd_q=-3)), "ka_q and kd_q must be 0 .. 256"),
                     (dict(sh=shade(gscale=(1, np.inf, 1))), "gscale and light must be finite"),
                     (dict(sh=shade(gscale=(np.nan, 1, 1))), "gscale and light must be finite"),
                     (dict(sh=shade(light=(0, 0, -np.inf))), "gscale and light must be finite"),
                     (dict(sh=shade(light=(0, np.nan, 0))), "gscale and light must be finite"),
                     (dict(tf=bad_tau), "tau lies outside"), (dict(off=off2), "off[0]")):
        assert call(**kw) == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    assert not out.any()
    s_q = np.zeros(4, np.int32)
    q = lambda jac=jac, n=4, sh=shade(), s_q=s_q: L.brief_composite_shade_q_host(p(jac), n, C.byref(sh) if sh is not None else None, p(s_q))
    assert q() == 0 and (s_q > 0).all()
    for kw, what in ((dict(jac=None), "null buffer"), (dict(s_q=None), "null buffer"), (dict(n=0), "n must be >= 1"), (dict(sh=None), "null shade descriptor"),
                     (dict(sh=shade(kd_q=300)), "ka_q and kd_q must be 0 .. 256"), (dict(sh=shade(light=(np.inf, 0, 0))), "gscale and light must be finite")):
        assert q(**kw) == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())


def test_header_exports_and_ctypes_signatures_agree():
    import re
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#define BRIEF_VERSION 130" in text
    counts = {"brief_view_composite_select": 17, "brief_view_composite_pick": 6, "brief_view_composite_shade_fold": 22,
              "brief_view_composite_shade_host": 17, "brief_composite_shade_q_host": 4}
    for name, n in counts.items():
        assert name in _lib.EXPORTS, name
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, plain, flags=re.S)
        assert proto and len(proto.group(1).split(",")) == n, name
        if os.path.exists(_lib.LIB_PATH):
            fn = getattr(_lib.lib(), name)
            assert len(fn.argtypes) == n and fn.restype is C.c_int, name
    assert C.sizeof(_lib.CompositeShade) == 32
    head = open(os.path.join(ROOT, "brief_pytorch_amd", "csrc", "brief_composite.h")).read()
    for fn in ("brief_composite_cos_q", "brief_composite_shade_q", "brief_composite_lit", "brief_composite_need"):
        assert "BRIEF_HD" in head and fn in head, fn


# ---- refusals of the Python calls and the CLI
def test_shade_quant_rounds_and_refuses_by_name():
    assert CP.shade_quant((1, 0)) == (256, 0) and CP.shade_quant((0.2, 0.8)) == (51, 205) and CP.shade_quant(("0.5", 0.001)) == (128, 0)
    assert CP.shade_quant((0.002, 1.0)) == (1, 256)
    for bad in ((1.5, 0), (0, -0.1), (float("nan"), 0), (0, float("inf"))):
        with pytest.raises(ValueError, match="must each lie in \\[0, 1\\]"):
            CP.shade_quant(bad)
    for bad in ((1,), (1, 0, 0), "ab", None, 0.5):
        with pytest.raises(ValueError, match="two numbers KA,KD"):
            CP.shade_quant(bad)


def _opt():
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    pp = opt.CompressFramework.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 0, False, [0, 65535]
    return opt


def _side(**kw):
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


TF = "0:0,0,0,0;65535:255,255,255,0.5"


class _Net:
    """what render_composite reads of a net before it asks for the GPU"""
    coords_channel, data_channel, precision, features = 3, 1, "fp32", 22

    def _require_gpu(self):
        raise AssertionError("the GPU path was reached")


def test_python_calls_refuse_by_name_before_any_decode(tmp_path):
    """each on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    mod = str(tmp_path / "module")
    call = lambda s, **kw: NFGR.decompress_composite(_opt(), mod, s, (1, 0, 0), TF, **kw)
    with pytest.raises(ValueError, match="light describes the shaded composite.*shade=\\(KA, KD\\)"):
        call(_side(), light=(1, 0, 0))
    with pytest.raises(ValueError, match="must each lie in \\[0, 1\\]"):
        call(_side(), shade=(0.5, 1.5))
    with pytest.raises(ValueError, match="two numbers KA,KD"):
        call(_side(), shade=(0.5,))
    with pytest.raises(ValueError, match="light must not be the zero vector"):
        call(_side(), shade=(0.5, 0.5), light=(0, 0, 0))
    with pytest.raises(ValueError, match="light must be three"):
        call(_side(), shade=(0.5, 0.5), light=(0, 1))
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*FFN"):
        call(_side(phi_name="FFN"), shade=(0.2, 0.8))
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*bf16"):
        call(_side(phi_precision="bf16"), shade=(0.2, 0.8))
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*1024"):
        call(_side(phi_features=1500), shade=(0.2, 0.8))
    with pytest.raises(ValueError, match="shaded composite of a DivideTask artefact is refused.*second.*follow-up"):
        CP.decompress_divide_composite(_opt(), {}, mod, mod, (1, 0, 0), TF, shade=(0.2, 0.8))
    # render_composite's own keywords
    view = V.make_view(DIMS, (1, 0, 0))
    tf = np.zeros((4096, 4), np.int32)
    render = lambda net=_Net(), **kw: CP.render_composite(net, view, tf, -1.0, 1.0, "u16", (0.0, 1.0), (0.0, 60000.0), **kw)
    for kw, what in ((dict(light=(1, 0, 0)), "light describes the shaded composite"), (dict(gscale=(1, 1, 1)), "gscale describes the shaded composite"),
                     (dict(compact=False), "compact=False describes the shaded composite"), (dict(shade=(2, 0)), "must each lie in \\[0, 1\\]"),
                     (dict(shade=(0.5, 0.5), light=(0, 0, 0)), "light must not be the zero vector"),
                     (dict(shade=(0.5, 0.5), gscale=(1, np.nan, 1)), "gscale must be three finite numbers"),
                     (dict(shade=(0.5, 0.5), channel=1), "channel 1 does not exist")):
        with pytest.raises(ValueError, match=what):
            render(**kw)
    bf16 = _Net()
    bf16.precision = "bf16"
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*bf16"):
        render(bf16, shade=(0.5, 0.5))
    assert not os.listdir(str(tmp_path))


def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VIEW = ["--view", "0.48,-0.6,0.64"]
COMPOSITE = VIEW + ["--view-composite", TF]


@pytest.mark.parametrize("extra,words", [
    (VIEW + ["--view-composite-shade", "0.2,0.8"], ["--view-composite-shade", "give its transfer function with --view-composite SPEC"]),
    (VIEW + ["--view-composite-light", "1,0,0"], ["--view-composite-light", "give its transfer function with --view-composite SPEC"]),
    (["--view-composite-shade", "0.2,0.8"], ["--view-composite SPEC"]),
    (COMPOSITE + ["--view-composite-light", "1,0,0"], ["--view-composite-light names the direction", "--view-composite-shade KA,KD"]),
    (COMPOSITE + ["--view-composite-shade", "0.2"], ["--view-composite-shade 0.2", "2 comma-separated numbers"]),
    (COMPOSITE + ["--view-composite-shade", "0.2,0.3,0.4"], ["--view-composite-shade 0.2,0.3,0.4", "2 comma-separated numbers"]),
    (COMPOSITE + ["--view-composite-shade", "a,b"], ["--view-composite-shade a,b", "2 comma-separated numbers"]),
    (COMPOSITE + ["--view-composite-shade", "0.2,1.01"], ["--view-composite-shade:", "must each lie in [0, 1]"]),
    (COMPOSITE + ["--view-composite-shade=-0.1,1"], ["--view-composite-shade:", "must each lie in [0, 1]"]),
    (COMPOSITE + ["--view-composite-shade", "nan,1"], ["--view-composite-shade:", "must each lie in [0, 1]"]),
    (COMPOSITE + ["--view-composite-shade", "0.2,0.8", "--view-composite-light", "1,0"], ["--view-composite-light 1,0", "3 comma-separated numbers"]),
    (COMPOSITE + ["--view-composite-shade", "0.2,0.8", "--view-composite-light", "0,0,0"], ["--view-composite-light must not be the zero vector"]),
    (COMPOSITE + ["--view-composite-shade", "0.2,0.8", "--view-light", "1,0,0"], ["--view-composite with --view-light"]),
])
def test_cli_refusals_write_nothing(tmp_path, extra, words):
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:",
            "-o", str(tmp_path / "out" / "c.png")] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))


def test_cli_refuses_a_divide_artefact_and_a_net_without_the_jacobian_kernel(tmp_path):
    import yaml
    yml = str(tmp_path / "run.yaml")
    config.save(_opt(), yml)                                       # (an identity postprocess: a composite refuses anything else first)
    argv = ["-p", yml, "--region", ":,:,:", "-o", str(tmp_path / "c.png")] + COMPOSITE
    os.makedirs(str(tmp_path / "div" / "sideinfos"))
    with pytest.raises(SystemExit, match="--view-composite-shade: a shaded composite of a DivideTask artefact is refused.*follow-up"):
        _cli().main(argv + ["-c", str(tmp_path / "div"), "--view-owner", "nearest", "--view-composite-shade", "0.2,0.8"])
    with pytest.raises(SystemExit, match="--view-composite: a composite view of a DivideTask artefact.*follow-up"):
        _cli().main(argv + ["-c", str(tmp_path / "div"), "--view-composite-shade", "0.2,0.8"])
    os.makedirs(str(tmp_path / "ffn"))
    with open(str(tmp_path / "ffn" / "sideinfos.yaml"), "w") as f:
        yaml.safe_dump(_side(phi_name="FFN", data_shape=[24, 28, 32, 1]), f)
    with pytest.raises(SystemExit, match="--view-composite: a shaded composite needs the analytic Jacobian: .*FFN"):
        _cli().main(argv + ["-c", str(tmp_path / "ffn"), "--view-composite-shade", "0.2,0.8"])
    assert sorted(os.listdir(str(tmp_path))) == ["div", "ffn", "run.yaml"]
