"""Host side of the composite view (brief_pytorch_amd/composite.py, decompress.py --view-composite): the constants and the
transmittance of csrc/brief_composite.h against exact arithmetic, brief_view_composite_host against a restatement in Python integers,
make_transfer, parse_transfer, the refusals and the PNG's byte order.  Nothing here needs a GPU: brief_view_composite_host runs the
header the kernels run, on the host CPU."""
import ctypes as C
import importlib.util
import os
import re
import struct
import zlib
from decimal import Decimal, getcontext

import numpy as np
import pytest

from brief_pytorch_amd import _lib, config
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR
from brief_pytorch_amd.tool import read_png
from tests._composite import TAU_SAT, A, B, W, finish, fold_ray, random_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (8, 9, 10)
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=0.9, depth_spacing=0.7, voxel_size=(2, 1, 1))

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")


# ---- the constants and W (tests/_composite.py: from decimal at 60 digits)
def test_header_constants_equal_decimal_at_60_digits():
    text = open(os.path.join(ROOT, "brief_pytorch_amd", "csrc", "brief_composite.h")).read()
    for name, want in (("A", A), ("B", B)):
        body = re.search(r"static const uint32_t %s\[256\] = \{(.*?)\};" % name, text, flags=re.S).group(1)
        got = [int(x.strip().rstrip("u")) for x in body.split(",")]
        assert got == want, name
    assert "#define BRIEF_COMPOSITE_TAU_SAT (32 << 16)" in text and "#define BRIEF_COMPOSITE_E_MAX 65280" in text
    assert CP.TAU_SAT == TAU_SAT and CP.E_MAX == 65280


def test_w_is_exact_at_the_ends_and_does_not_increase():
    assert W(0) == 1 << 32 and W(TAU_SAT) == 0 and W(TAU_SAT + 5) == 0 and W(TAU_SAT - 1) == 1 and W(31 << 16) == 2 and W(1 << 16) == 1 << 31
    prev = W(0)
    for tau in range(1, 3 * 65536 + 2):                             # every fraction, and the carries into q
        w = W(tau)
        assert w <= prev, tau
        prev = w
    rng = np.random.default_rng(0)
    taus = np.unique(np.concatenate([rng.integers(0, TAU_SAT + 1, 4000), np.arange(0, TAU_SAT + 1, 65536), np.arange(65535, TAU_SAT, 65536)]))
    ws = [W(int(t)) for t in taus]
    assert all(a >= b for a, b in zip(ws[:-1], ws[1:]))
    getcontext().prec = 60
    for t, w in zip(taus[::97], ws[::97]):                           # the header's bound on W's distance from the real transmittance
        real = (Decimal(2).ln() * (Decimal(32) - Decimal(int(t)) / 65536)).exp()
        assert abs(Decimal(w) - real) < 4, t


# ---- brief_view_composite_host against Python integers
def _restate(view, k0, off, vals, tf, channel, bg):
    rays = view.rows * view.cols
    width = 8 * vals.dtype.itemsize
    shift = width - (len(tf).bit_length() - 1)
    cnt = np.diff(off)
    r = np.repeat(np.arange(rays), cnt)
    k = np.repeat(k0, cnt) + (np.arange(int(off[-1])) - np.repeat(off[:-1], cnt))
    inside = V.sample_host(view, r // view.cols, r % view.cols, k)[2]
    img, hits, runs, accs = np.zeros((rays, 4), np.uint8), np.zeros(rays, np.int32), np.zeros(rays, np.int32), np.zeros((rays, 3), np.uint64)
    for ray in range(rays):
        mine = [s for s in range(int(off[ray]), int(off[ray + 1])) if inside[s]]
        run, acc = fold_ray([tf[int(vals[s, channel]) >> shift] for s in mine])
        img[ray] = finish(run, acc, bg)
        hits[ray], runs[ray], accs[ray] = len(mine), run, [a % (1 << 64) for a in acc]
    shape = (view.rows, view.cols)
    return img.reshape(*shape, 4), hits.reshape(shape), runs.reshape(shape), accs.reshape(*shape, 3)


@needs_lib
@pytest.mark.parametrize("dtype,channels,channel,bits", [(np.uint8, 1, 0, 8), (np.uint8, 3, 2, 5), (np.uint16, 1, 0, 12), (np.uint16, 3, 1, 16),
                                                         (np.uint16, 3, 2, 7), (np.uint16, 1, 0, 1)])
def test_host_composite_equals_python_integers(dtype, channels, channel, bits):
    rng = np.random.default_rng(bits * 7 + channels)
    view = V.make_view(DIMS, **OBLIQUE)
    rays = view.rows * view.cols
    assert view.depth < 32
    tf = random_table(rng, bits)
    bg = (12, 200, 255)
    for lists in ("clipped", "random"):
        if lists == "clipped":                                       # the view's own list: every sample inside
            k0, cnt = (x.ravel() for x in V.clip_host(view))
        else:                                                        # any interval of k: the inside test is the fold's own
            cnt = rng.integers(0, view.depth + 1, rays).astype(np.int32)
            cnt[rng.random(rays) < 0.2] = 0
            k0 = (rng.random(rays) * (view.depth - cnt + 1)).astype(np.int32)
        assert (cnt == 0).any() and (cnt == 1).any() and cnt.max() > 8
        off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
        vals = rng.integers(0, np.iinfo(dtype).max + 1, (int(off[-1]), channels)).astype(dtype)
        got = CP.composite_host(view, k0, off, vals, tf, channel=channel, background=bg)
        want = _restate(view, k0, off, vals, tf, channel, bg)
        for g, w, what in zip(got, want, ("image", "hits", "tau_run", "acc")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (lists, what)
        img, hits, run, _ = got
        if lists == "random":
            assert (hits.ravel() < cnt).any(), "no sample outside the clip box: the inside test is not exercised"
        assert (run == TAU_SAT).any() and ((run > 0) & (run < TAU_SAT)).any(), "no saturating ray, or nothing else"
        assert (img[hits == 0] == np.array(bg + (0,), np.uint8)).all() and (hits == 0).any()
        assert len(np.unique(img[..., :3])) > 20 or bits == 1


@needs_lib
def test_host_entry_refuses_bad_arguments_by_name():
    L = _lib.lib()
    view = V.make_view(DIMS, (1, 0, 0))
    rays = view.rows * view.cols
    k0, off = np.zeros(rays, np.int32), np.arange(rays + 1, dtype=np.int64)
    vals, out = np.zeros((rays, 2), np.uint8), np.zeros((rays, 4), np.uint8)
    tf = np.zeros((256, 4), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bg = (C.c_int32 * 3)(0, 0, 0)

    def call(k0=k0, off=off, vals=vals, kind=_lib.OUT_U8, channels=2, channel=1, tf=tf, bits=8, bg=bg, out=out):
        return L.brief_view_composite_host(C.byref(view), p(k0) if k0 is not None else None, p(off), p(vals), kind, channels, channel,
                                           p(tf) if tf is not None else None, bits, bg, None, None, None, p(out) if out is not None else None)
    assert call() == 0
    bad_tau, bad_e, neg = tf.copy(), tf.copy(), tf.copy()
    bad_tau[3, 0], bad_e[200, 2], neg[0, 0] = TAU_SAT + 1, 65281, -1
    off2 = off.copy()
    off2[0] = 1
    for kw, what in ((dict(k0=None), "null buffer"), (dict(out=None), "null buffer"), (dict(tf=None), "null transfer table"),
                     (dict(kind=_lib.OUT_F32), "elem_kind"), (dict(channel=2), "channel must be 0 .. channels - 1"),
                     (dict(channel=-1), "channel must be 0 .. channels - 1"), (dict(channels=5), "channels must be 1..4"),
                     (dict(bits=0), "tf_bits"), (dict(bits=9), "tf_bits"), (dict(tf=bad_tau), "tau lies outside"),
                     (dict(tf=neg), "tau lies outside"), (dict(tf=bad_e), "emission lies outside"),
                     (dict(bg=(C.c_int32 * 3)(0, 256, 0)), "background"), (dict(off=off2), "off[0]"),
                     (dict(k0=np.full(rays, view.depth, np.int32)), "inside 0 .. depth - 1")):
        assert call(**kw) == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    assert call(kind=_lib.OUT_U16, vals=np.zeros((rays, 2), np.uint16), tf=np.zeros((1 << 16, 4), np.int32), bits=16) == 0
    assert not out.any()


ENTRIES = {
    "brief_view_composite_fold": (["const brief_view_desc *view", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
                                   "int64_t r1", "int32_t lanes", "const void *vals", "int elem_kind", "int32_t channels", "int32_t channel",
                                   "const int32_t *tf", "int32_t tf_bits", "int32_t *hits", "int32_t *tau_run", "uint64_t *acc", "void *stream"],
                                  "wvvllllivniivivvvv"),
    "brief_view_composite_finish": (["const brief_view_desc *view", "const int32_t *background", "const int32_t *hits", "const int32_t *tau_run",
                                     "const uint64_t *acc", "uint8_t *out", "void *stream"], "wbvvvvv"),
    "brief_view_composite_host": (["const brief_view_desc *view", "const int32_t *k0", "const int64_t *off", "const void *vals", "int elem_kind",
                                   "int32_t channels", "int32_t channel", "const int32_t *tf", "int32_t tf_bits", "const int32_t *background",
                                   "int32_t *hits", "int32_t *tau_run", "uint64_t *acc", "uint8_t *out"], "wvvvniivibvvvv"),
}


def test_header_exports_and_ctypes_signatures_agree():
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    codes = {"w": C.POINTER(_lib.ViewDesc), "v": C.c_void_p, "l": C.c_int64, "i": C.c_int32, "n": C.c_int, "b": C.POINTER(C.c_int32)}
    for name, (want, sig) in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, plain, flags=re.S)
        assert proto, "%s is not declared in include/brief_hip.h" % name
        assert [" ".join(p.split()) for p in proto.group(1).split(",")] == want, name
        assert len(sig) == len(want), name
        if os.path.exists(_lib.LIB_PATH):                        # the signature the loaded library was given
            fn = getattr(_lib.lib(), name)
            assert list(fn.argtypes) == [codes[c] for c in sig], name
            assert fn.restype is C.c_int


# ---- make_transfer and parse_transfer
def test_make_transfer_interpolates_and_corrects_the_opacity_for_the_spacing():
    pts = [(0, 255, 0, 0, 0.0), (100, 255, 0, 0, 0.0), (200, 0, 255, 64, 0.5), (255, 0, 0, 255, 1.0)]
    tf = CP.make_transfer(pts, "u8", 1.0)
    assert tf.dtype == np.int32 and tf.shape == (256, 4)
    assert not tf[:101].any(), "a = 0 gives a zero row"
    assert tf[255, 0] == TAU_SAT and list(tf[255, 1:]) == [0, 0, 65280], "a = 1 is TAU_SAT, and opaque blue is 256 * 255"
    assert tf[200, 0] == 65536 and list(tf[200, 1:]) == [0, round(256 * 255 * 0.5), round(256 * 64 * 0.5)]
    assert (np.diff(tf[100:, 0]) >= 0).all() and tf[150, 0] == round(-np.log2(0.75) * 65536)
    # e is computed from the quantised tau
    alpha = 1.0 - 2.0 ** (-tf[:, 0].astype(np.float64) / 65536)
    colour = np.stack([np.interp(np.arange(256.0), [p[0] for p in pts], [p[1 + c] for p in pts]) for c in range(3)], 1)
    assert np.abs(tf[:, 1:] - 256.0 * colour * alpha[:, None]).max() <= 0.5 + 1e-6
    # the header's premise for the accumulator's width: e < 2^17 * alpha
    assert (tf[:, 1:] <= 2.0 ** 17 * alpha[:, None]).all()
    # doubling depth_spacing doubles tau up to rounding and the clamp
    for spacing in (0.3, 1.0, 2.5):
        one, two = CP.make_transfer(pts, "u8", spacing)[:, 0].astype(np.int64), CP.make_transfer(pts, "u8", 2 * spacing)[:, 0].astype(np.int64)
        free = two < TAU_SAT
        assert free.sum() > 100 and (np.abs(two - 2 * one)[free] <= 1).all() and (2 * one[~free] >= TAU_SAT - 1).all()
        assert one[255] == two[255] == TAU_SAT and not one[:101].any() and not two[:101].any()
    # fewer bits than the dtype has: a row stands for the middle of its values; uint16 defaults to 12 bits
    tf5 = CP.make_transfer(pts, "u8", 1.0, bits=5)
    assert tf5.shape == (32, 4)
    a = np.interp(np.arange(32) * 8 + 3.5, [p[0] for p in pts], [p[4] for p in pts])
    assert np.array_equal(tf5[:, 0], np.rint(np.minimum(-np.log2(1 - np.minimum(a, 1 - 1e-300)) * 65536, TAU_SAT)).astype(np.int32))
    tf16 = CP.make_transfer([(0, 10, 20, 30, 0.0), (65535, 10, 20, 30, 0.25)], "u16", 1.0)
    assert tf16.shape == (4096, 4) and tf16[0, 0] < tf16[-1, 0] <= round(-np.log2(0.75) * 65536)
    assert CP.make_transfer([(7, 1, 2, 3, 0.5)], "u16", 1.0, bits=16).shape == (65536, 4)
    for kw, what in ((dict(bits=9), "bits = 9"), (dict(bits=0), "bits = 0"), (dict(depth_spacing=0.0), "depth_spacing")):
        with pytest.raises(ValueError, match=what):
            CP.make_transfer(pts, "u8", **{"depth_spacing": 1.0, **kw})
    with pytest.raises(ValueError, match="0 .. 255, strictly ascending"):
        CP.make_transfer([(0, 1, 2, 3, 0.5), (300, 1, 2, 3, 0.5)], "u8", 1.0)
    with pytest.raises(ValueError, match="out_kind must be 'u8' or 'u16'"):
        CP.make_transfer(pts, "f32", 1.0)
    bad = tf.copy()
    bad[4, 0] = TAU_SAT + 1
    with pytest.raises(ValueError, match="tau must lie in 0 .. TAU_SAT"):
        CP.check_transfer(bad, "u8")
    bad = tf.copy()
    bad[4, 3] = 65281
    with pytest.raises(ValueError, match="emission must lie in 0 .. 65280"):
        CP.check_transfer(bad, "u8")
    with pytest.raises(ValueError, match="2\\^bits"):
        CP.check_transfer(tf[:100], "u8")


def test_parse_transfer_reads_points_and_refuses_by_name(tmp_path):
    assert CP.parse_transfer("0:0,0,0,0; 120:255,128,0,0.25 ;65535:255,255,255,1") == [(0, 0.0, 0.0, 0.0, 0.0), (120, 255.0, 128.0, 0.0, 0.25),
                                                                                   (65535, 255.0, 255.0, 255.0, 1.0)]
    path = tmp_path / "tf.txt"
    path.write_text("10:1,2,3,0.5\n20:4,5,6,0.75;30:7,8,9,1\n\n")
    assert CP.parse_transfer("@" + str(path)) == [(10, 1.0, 2.0, 3.0, 0.5), (20, 4.0, 5.0, 6.0, 0.75), (30, 7.0, 8.0, 9.0, 1.0)]
    for text, what in (("", "at least one point"), ("10:1,2,3", "level:r,g,b,a"), ("1.5:1,2,3,0.5", "level:r,g,b,a"), ("x", "level:r,g,b,a"),
                       ("10:1,2,3,0.5;10:1,2,3,0.5", "strictly ascending"), ("20:1,2,3,0.5;10:1,2,3,0.5", "strictly ascending"),
                       ("10:1,2,256,0.5", "colour must lie in 0 .. 255"), ("10:1,-2,3,0.5", "colour must lie in 0 .. 255"),
                       ("10:1,2,3,1.5", "opacity must lie in \\[0, 1\\]"), ("70000:1,2,3,0.5", "outside the range of the integer decode, 0 .. 65535"),
                       ("-1:1,2,3,0.5", "outside the range"), ("@" + str(tmp_path / "none.txt"), "does not exist")):
        with pytest.raises(ValueError, match=what):
            CP.parse_transfer(text)
    with pytest.raises(ValueError, match="0 .. 255"):
        CP.parse_transfer("300:1,2,3,0.5", "u8")


# ---- refusals of the artefact calls and the CLI
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


def test_artefact_refusals_are_raised_by_name_before_any_decode(tmp_path):
    """each on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    mod = str(tmp_path / "module")
    call = lambda o, s, tf=TF, **kw: NFGR.decompress_composite(o, mod, s, (1, 0, 0), tf, **kw)
    with pytest.raises(ValueError, match="composite view of a DivideTask artefact.*prefix.*follow-up"):
        call(_opt(), {"data_shape": [8, 8, 8, 1]})
    with pytest.raises(ValueError, match="error-bounded.*error_bound 3"):
        call(_opt(), _side(error_bound=3))
    with pytest.raises(ValueError, match="3-D data only"):
        call(_opt(), _side(data_shape=[50, 61, 3]))
    with pytest.raises(ValueError, match="uint8 / uint16 data only.*float32"):
        call(_opt(), _side(dtype="float32"))
    o = _opt()
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    with pytest.raises(ValueError, match="composite view with a Decompress.postprocess that changes values.*denoise.level 500"):
        call(o, _side())
    o = _opt()
    o.CompressFramework.Decompress.postprocess.clip = [100, 65535]
    with pytest.raises(ValueError, match="composite view with a Decompress.postprocess that changes values"):
        call(o, _side())
    with pytest.raises(ValueError, match="channel 1 does not exist"):
        call(_opt(), _side(), channel=1)
    with pytest.raises(ValueError, match="background must be three integers"):
        call(_opt(), _side(), background=(0, 0, 300))
    with pytest.raises(ValueError, match="strictly ascending"):
        call(_opt(), _side(), tf="5:1,2,3,0.5;5:1,2,3,0.5")
    o = _opt()
    o.CompressFramework.Decompress.postprocess.clip = [0, 255]
    with pytest.raises(ValueError, match="outside the range of the integer decode, 0 .. 255"):
        call(o, _side(dtype="uint8", max=250.0), tf="300:1,2,3,0.5")
    with pytest.raises(ValueError, match="bits = 17"):
        call(_opt(), _side(), bits=17)
    with pytest.raises(ValueError, match="zero vector"):
        NFGR.decompress_composite(_opt(), mod, _side(), (0, 0, 0), TF)
    os.makedirs(str(tmp_path / "sideinfos" / "d_0_3-h_0_7-w_0_7"))
    with pytest.raises(ValueError, match="composite view of a DivideTask artefact"):
        call(_opt(), _side())
    assert sorted(os.listdir(str(tmp_path))) == ["sideinfos"]


def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VIEW = ["--view", "0.48,-0.6,0.64"]


@pytest.mark.parametrize("extra,out,words", [
    (["--view-composite", TF], "c.png", ["--view-composite renders a --view", "--view dz,dy,dx"]),
    (VIEW + ["--view-composite-channel", "0"], "c.png", ["--view-composite-channel", "give its transfer function with --view-composite SPEC"]),
    (VIEW + ["--view-background", "1,2,3"], "c.png", ["--view-background", "--view-composite SPEC"]),
    (VIEW + ["--view-composite-bits", "8"], "c.png", ["--view-composite-bits", "--view-composite SPEC"]),
    (["--view-composite-bits", "8"], "c.png", ["--view-composite SPEC"]),
    (VIEW + ["--view-composite", TF, "--view-mode", "min"], "c.png", ["--view-composite with --view-mode min"]),
    (VIEW + ["--view-composite", TF, "--view-offset", "2"], "c.png", ["--view-composite with --view-offset"]),
    (VIEW + ["--view-composite", TF, "--view-surface", "100"], "c.png", ["--view-composite with --view-surface"]),
    (VIEW + ["--view-composite", TF, "--view-surface-side", "below"], "c.png", ["--view-composite with --view-surface-side"]),
    (VIEW + ["--view-composite", TF, "--view-refine", "2"], "c.png", ["--view-composite with --view-refine"]),
    (VIEW + ["--view-composite", TF, "--view-channel", "0"], "c.png", ["--view-composite with --view-channel", "--view-composite-channel"]),
    (VIEW + ["--view-composite", TF, "--view-light", "1,0,0"], "c.png", ["--view-composite with --view-light"]),
    (VIEW + ["--view-composite", TF, "--view-owner", "nearest"], "c.png", ["--view-composite with --view-owner"]),
    (VIEW + ["--view-composite", TF, "--mip"], "c.png", ["--view-composite with --mip"]),
    (VIEW + ["--view-composite", TF, "--gradient", "magnitude"], "c.npy", ["--view-composite with --gradient"]),
    (VIEW + ["--view-composite", TF, "--hessian", "laplacian"], "c.npy", ["--view-composite with --hessian"]),
    (VIEW + ["--view-composite", TF, "--shape", "8,8,8"], "c.png", ["--view-composite with --shape"]),
    (VIEW + ["--view-composite", TF, "--step", "2"], "c.png", ["--view-composite with --step 2"]),
    (VIEW + ["--view-composite", TF], "c.tif", ["--view-composite writes", ".png", ".npy", "got .tif", "one channel per page"]),
    (VIEW + ["--view-composite", TF], "c.jpg", ["--view-composite writes", "got .jpg"]),
    (VIEW + ["--view-composite", "5:1,2,3"], "c.png", ["--view-composite:", "level:r,g,b,a"]),
    (VIEW + ["--view-composite", "9:1,2,3,1;5:1,2,3,1"], "c.png", ["--view-composite:", "strictly ascending"]),
    (VIEW + ["--view-composite", TF, "--view-background", "0,0"], "c.png", ["--view-background 0,0", "3 comma-separated numbers"]),
    (VIEW + ["--view-composite", TF, "--view-background", "0,0,256"], "c.png", ["--view-composite:", "background must be three integers"]),
    (VIEW + ["--view-composite", TF, "--view-composite-channel", "-1"], "c.png", ["--view-composite-channel -1"]),
    (VIEW + ["--view-composite", TF, "--view-composite-bits", "17"], "c.png", ["--view-composite-bits 17"]),
    (VIEW + ["--view-composite", TF, "--view-up", "1,0"], "c.png", ["--view-up 1,0", "3 comma-separated numbers"]),
])
def test_cli_refusals_write_nothing(tmp_path, extra, out, words):
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:",
            "-o", str(tmp_path / "out" / out)] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))


def test_cli_refuses_a_divide_artefact_in_the_composites_words(tmp_path):
    os.makedirs(str(tmp_path / "art" / "sideinfos"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:", "-o", str(tmp_path / "c.png")]
    with pytest.raises(SystemExit, match="--view-composite: a composite view of a DivideTask artefact.*follow-up"):
        _cli().main(argv + VIEW + ["--view-composite", TF])
    assert sorted(os.listdir(str(tmp_path))) == ["art"]


def test_existing_view_messages_do_not_change(tmp_path):
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:", "-o", str(tmp_path / "v.tif")]
    with pytest.raises(SystemExit, match="^--view with --mip: a view is one image"):
        _cli().main(argv + VIEW + ["--mip"])
    with pytest.raises(SystemExit, match="^--hessian with --view: each writes"):
        _cli().main(argv[:-1] + [str(tmp_path / "v.npy")] + VIEW + ["--hessian", "laplacian"])
    with pytest.raises(SystemExit, match="describe a --view: give its direction"):
        _cli().main(argv + ["--view-mode", "slice"])


# ---- the PNG's byte order
def test_png_holds_r_g_b_in_that_order(tmp_path):
    rgb = np.zeros((2, 3, 3), np.uint8)
    rgb[0, 0], rgb[0, 1], rgb[0, 2], rgb[1, 0] = (255, 0, 0), (0, 200, 0), (0, 0, 100), (10, 20, 30)
    path = str(tmp_path / "c.png")
    _cli()._write_rgb_png(path, rgb)
    buf = open(path, "rb").read()
    assert buf[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(buf):
        n, kind = struct.unpack(">I4s", buf[pos:pos + 8])
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", buf[pos + 8:pos + 8 + n])
        if kind == b"IDAT":
            idat += buf[pos + 8:pos + 8 + n]
        pos += 12 + n
    assert hdr == (3, 2, 8, 2, 0, 0, 0)                              # 3 x 2, 8 bits, colour type 2: truecolour, samples R, G, B (PNG spec 6.1)
    raw = zlib.decompress(idat)
    assert len(raw) == 2 * (1 + 9) and raw[0] in (0, 2)              # (row 0: no filter, or Up against the zero row: the bytes themselves)
    assert list(raw[1:10]) == [255, 0, 0, 0, 200, 0, 0, 0, 100]
    back = read_png(path)                                           # cv2's order: B, G, R
    assert np.array_equal(back[..., ::-1], rgb) and not np.array_equal(back, rgb)
