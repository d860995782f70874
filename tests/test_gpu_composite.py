"""Composite view on the GPU (brief_pytorch_amd/composite.py, csrc/brief_composite.inc) on randomly initialised nets.  Every comparison
is bitwise: the fold is an integer fold.
  1  GPU fold + finish equals brief_view_composite_host on the same values, behind a SIREN, an MFN, an FFN and a bf16 SIREN, uint8 and
     uint16, tables of 2^3 to 2^16 rows; a repeat gives the same bits;
  2  every chunk and every number of lanes per ray gives one image and one state;
  3  ties to the existing views: a step table is the max view's threshold, a zero table the background, a uniform table the closed form
     of the hits image;  4  along +z at unit spacing the image is the integer composite of decode_box's volume."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import networks as N
from brief_pytorch_amd import view as VW
from tests import _variants as V
from tests._composite import TAU_SAT, W, finish, fold_ray, random_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (8, 9, 10)
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=0.9, depth_spacing=0.7, voxel_size=(2, 1, 1))      # 21 x 14 rays of up to 19 samples
TORCH_DT = {"u16": torch.uint16, "u8": torch.uint8}
KIND = {"u8": _lib.OUT_U8, "u16": _lib.OUT_U16}
BG = (12, 200, 255)

_cache = {}


def _make(vid):
    if vid == "ffn3":                                                # (tests/_variants.py's FFN takes two coordinates)
        torch.manual_seed(10)
        return N.FFN(coords_channel=3, data_channel=3, features=70, embsize=40, layers=4).to(DEV)
    return V.BY_ID[vid].make(DEV)


def _net(vid):
    """the net on the device and an integer window that does not leave the images flat (the 0.15 / 0.85 quantiles of the f32 decode)"""
    if vid not in _cache:
        m = _make(vid)
        f32 = m.decode_grid(DIMS).cpu().numpy()
        assert np.isfinite(f32).all()
        q15, q85 = (float(np.float32(q)) for q in np.quantile(f32.astype(np.float64), [0.15, 0.85]))
        assert q85 > q15
        _cache[vid] = (m, (q15, q85))
    return _cache[vid]


def _list(vid, kind, view):
    """(k0, off, vals) of the view's compacted sample list as device tensors, the whole list evaluated once"""
    key = (vid, kind, bytes(view))
    if key not in _cache:
        m, scale = _net(vid)
        got = {}

        def keep(k0, off, s0, s1, r0, r1, lanes, vals):
            assert s0 == 0 and "vals" not in got
            got.update(k0=k0, off=off, vals=vals[:s1].clone(), lanes=lanes)
        v = VW._with_range(view, -1.0, 1.0)
        _, total, _ = VW._march(m, v, KIND[kind], TORCH_DT[kind], scale, V.VRANGE[kind], 1 << 30, keep)
        assert total == len(got["vals"]) > 0
        _cache[key] = got
    g = _cache[key]
    return g["k0"], g["off"], g["vals"], g["lanes"]


def _random_table(seed, bits):
    return random_table(np.random.default_rng(seed), bits)


def _render(vid, kind, view, tf, channel=0, background=BG, chunk=None):
    m, scale = _net(vid)
    img, hits, stats = CP.render_composite(m, view, tf, -1.0, 1.0, kind, scale, V.VRANGE[kind], channel=channel, background=background, chunk=chunk)
    assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (view.rows, view.cols, 4)
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (view.rows, view.cols)
    return img.cpu().numpy(), hits.cpu().numpy(), stats


# ---- 1: the device against the host on the same values
@pytest.mark.parametrize("vid,kind,bits,channel", [("s22", "u8", 8, 0), ("s22", "u16", 12, 0), ("s22", "u16", 7, 0), ("mfnf", "u16", 16, 3),
                                                    ("mfnf", "u8", 3, 1), ("ffn3", "u16", 12, 2), ("b96", "u8", 8, 1)])
def test_device_fold_and_finish_equal_the_host_on_the_same_values(vid, kind, bits, channel):
    view = VW.make_view(DIMS, **OBLIQUE)
    assert 12 <= view.rows <= 24 and 12 <= view.cols <= 24 and view.depth < 32 and (view.rows * view.cols) % 64 != 0
    k0, off, vals, _ = _list(vid, kind, view)
    tf = _random_table(bits, bits)
    want_img, want_hits, want_run, _ = CP.composite_host(VW._with_range(view, -1.0, 1.0), k0.cpu().numpy(), off.cpu().numpy(), vals.cpu().numpy(), tf,
                                                         channel=channel, background=BG)
    img, hits, stats = _render(vid, kind, view, tf, channel)
    assert np.array_equal(hits, want_hits) and np.array_equal(img, want_img), int((img != want_img).sum())
    assert stats["samples_inside"] == int(want_hits.sum()) == stats["samples_evaluated"] and stats["rays"] == view.rows * view.cols
    # a repeat gives the same bits; so does the table as a device tensor
    img2, hits2, stats2 = _render(vid, kind, view, torch.from_numpy(tf).to(DEV), channel)
    assert np.array_equal(img2, img) and np.array_equal(hits2, hits) and stats2 == stats
    # what keeps this from being vacuous: rays that miss, rays of one sample and of many, saturated and half-transparent pixels, colours
    assert (want_hits == 0).any() and (want_hits == 1).any() and want_hits.max() >= 12
    assert (img[want_hits == 0] == np.array(BG + (0,), np.uint8)).all()
    assert (want_run == TAU_SAT).any() and ((want_run > 0) & (want_run < TAU_SAT)).any()
    assert len(np.unique(img[..., :3])) >= 20 and len(np.unique(img[..., 3])) >= 5


# ---- 2: chunks and lanes
def _fold_direct(view, kind, ch, k0, off, vals, tf, bits, channel, lanes, chunk):
    """fold + finish through the entries themselves: every chunk names ALL rays (a ray without a sample in the chunk folds nothing)"""
    L, st = _lib.lib(), _lib.stream_ptr()
    v = VW._with_range(view, -1.0, 1.0)
    rays, total = view.rows * view.cols, len(vals)
    hits = torch.zeros(rays, dtype=torch.int32, device=DEV)
    run = torch.zeros(rays, dtype=torch.int32, device=DEV)
    acc = torch.zeros((rays, 3), dtype=torch.int64, device=DEV)
    for s0 in range(0, total, chunk):
        s1 = min(s0 + chunk, total)
        part = vals[s0:s1].contiguous()
        _lib.check(L.brief_view_composite_fold(C.byref(v), _lib.ptr(k0), _lib.ptr(off), s0, s1, 0, rays, lanes, _lib.ptr(part), KIND[kind], ch, channel,
                                               _lib.ptr(tf), bits, _lib.ptr(hits), _lib.ptr(run), _lib.ptr(acc), st))
    img = torch.empty((rays, 4), dtype=torch.uint8, device=DEV)
    _lib.check(L.brief_view_composite_finish(C.byref(v), (C.c_int32 * 3)(*BG), _lib.ptr(hits), _lib.ptr(run), _lib.ptr(acc), _lib.ptr(img), st))
    return [t.cpu().numpy() for t in (img, hits, run, acc)]


@pytest.mark.parametrize("kind,bits", [("u8", 8), ("u16", 12)])
def test_every_chunk_and_every_number_of_lanes_give_one_image(kind, bits):
    view = VW.make_view(DIMS, **OBLIQUE)
    k0, off, vals, default_lanes = _list("s22", kind, view)
    tf = _random_table(100 + bits, bits)
    want = CP.composite_host(VW._with_range(view, -1.0, 1.0), k0.cpu().numpy(), off.cpu().numpy(), vals.cpu().numpy(), tf, background=BG)
    want = [want[0].reshape(-1, 4), want[1].ravel(), want[2].ravel(), want[3].reshape(-1, 3).view(np.int64)]
    table = torch.from_numpy(tf).to(DEV)
    assert 1 < default_lanes < 64 and len(vals) > 64 * 4
    for lanes in (1, 2, 8, 64):
        for chunk in (7, 64, len(vals)):
            got = _fold_direct(view, kind, 1, k0, off, vals, table, bits, 0, lanes, chunk)
            for g, w, what in zip(got, want, ("image", "hits", "tau_run", "acc")):
                assert np.array_equal(g, w), (lanes, chunk, what)
    base = _render("s22", kind, view, tf)
    assert np.array_equal(base[0].reshape(-1, 4), want[0])
    for chunk in (1, 7, 64, len(vals)):
        img, hits, stats = _render("s22", kind, view, tf, chunk=chunk)
        assert np.array_equal(img, base[0]) and np.array_equal(hits, base[1]) and stats == base[2], chunk


# ---- 3: ties to the existing views
@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_step_zero_and_uniform_tables_tie_to_the_max_view_and_the_hits_image(kind):
    m, scale = _net("s22")
    view = VW.make_view(DIMS, **OBLIQUE)
    width = 8 if kind == "u8" else 16
    top, hits_img, _ = VW.render(m, view, "max", -1.0, 1.0, kind, scale, V.VRANGE[kind])
    top, hits_img = top.cpu().numpy()[..., 0].astype(np.int64), hits_img.cpu().numpy()
    hit = hits_img > 0
    level = int(np.median(top[hit]))
    # a step: opaque white from `level` on, nothing below, over black
    tf = np.zeros((1 << width, 4), np.int32)
    tf[level:] = [TAU_SAT, 65280, 65280, 65280]
    img, hits, _ = _render("s22", kind, view, tf, background=(0, 0, 0))
    above = hit & (top >= level)
    assert np.array_equal(hits, hits_img) and 0.25 * hit.sum() <= above.sum() <= 0.75 * hit.sum()
    assert (img[above] == 255).all() and not img[~above].any()
    # nothing: the background, A = 0
    img, hits, _ = _render("s22", kind, view, np.zeros((1 << width, 4), np.int32))
    assert (img == np.array(BG + (0,), np.uint8)).all() and np.array_equal(hits, hits_img)
    # one tau and one colour everywhere: the closed form of the hits image, whatever the values are
    for tau0, e, bits in ((9000, (500, 7, 65280 // 9), 4), (TAU_SAT // 3, (65000, 1, 300), 8), (1, (1, 0, 1), 1)):
        tf = np.tile(np.array([[tau0, *e]], np.int32), (1 << bits, 1))
        img, hits, _ = _render("s22", kind, view, tf)
        want = np.empty(img.shape, np.uint8)
        for n in np.unique(hits_img):
            acc = [sum(W(min(j * tau0, TAU_SAT)) for j in range(int(n))) * c for c in e]
            want[hits_img == n] = finish(min(int(n) * tau0, TAU_SAT), acc, BG)
        assert np.array_equal(img, want) and np.array_equal(hits, hits_img), (tau0, e)
    assert len(np.unique(hits_img)) >= 10


# ---- 4: the grid's own voxels
@pytest.mark.parametrize("vid,kind,channel", [("s22", "u16", 0), ("mfnf", "u8", 2)])
def test_along_z_at_unit_spacing_it_is_the_composite_of_the_decoded_volume(vid, kind, channel):
    m, scale = _net(vid)
    vol = m.decode_box(DIMS, out_kind=kind, scale=scale, vrange=V.VRANGE[kind]).cpu().numpy()
    assert vol.shape == DIMS + (m.data_channel,)
    bits = 6
    tf = _random_table(7, bits)
    shift = (8 if kind == "u8" else 16) - bits
    view = VW.make_view(DIMS, (1, 0, 0))
    assert (view.rows, view.cols, view.depth) == (DIMS[1], DIMS[2], DIMS[0])
    img, hits, stats = _render(vid, kind, view, tf, channel)
    want = np.empty(img.shape, np.uint8)
    for y in range(DIMS[1]):
        for x in range(DIMS[2]):
            want[y, x] = finish(*fold_ray([tf[int(v) >> shift] for v in vol[:, y, x, channel]]), BG)
    assert np.array_equal(img, want) and (hits == DIMS[0]).all() and stats["samples_evaluated"] == int(np.prod(DIMS))
    assert len(np.unique(img.reshape(-1, 4), axis=0)) >= 20
    # looking the other way composites the same voxels back to front: another image
    back, _, _ = _render(vid, kind, VW.make_view(DIMS, (-1, 0, 0), up=(0, 1, 0)), tf, channel)
    for y in range(DIMS[1]):
        for x in range(DIMS[2]):
            want[y, x] = finish(*fold_ray([tf[int(v) >> shift] for v in vol[::-1, y, x, channel]]), BG)
    assert sorted(map(tuple, back.reshape(-1, 4))) == sorted(map(tuple, want.reshape(-1, 4))) and not np.array_equal(back, img)


# ---- refusals
def test_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    view = VW.make_view(DIMS, (1, 0, 0))
    rays = view.rows * view.cols
    k0 = torch.zeros(rays, dtype=torch.int32, device=DEV)
    off = torch.zeros(rays + 1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(4 * rays, dtype=torch.int64, device=DEV)
    tf = torch.zeros((256, 4), dtype=torch.int32, device=DEV)
    p, st, v = _lib.ptr, _lib.stream_ptr(), C.byref(view)
    bg = (C.c_int32 * 3)(0, 0, 0)

    def fold(vals=buf, kind=_lib.OUT_U8, channels=2, channel=1, table=tf, bits=8, hits=k0, run=k0, acc=buf, lanes=1):
        return L.brief_view_composite_fold(v, p(k0), p(off), 0, 4, 0, 1, lanes, p(vals), kind, channels, channel, p(table), bits, p(hits), p(run), p(acc), st)
    unaligned = C.c_void_p(tf.data_ptr() + 4)
    for call, what in ((lambda: fold(vals=None), "null buffer"), (lambda: fold(run=None), "null buffer"), (lambda: fold(acc=None), "null buffer"),
                       (lambda: fold(table=None), "null transfer table"), (lambda: fold(kind=_lib.OUT_F32), "elem_kind"),
                       (lambda: fold(channel=2), "channel must be 0 .. channels - 1"), (lambda: fold(channel=-1), "channel must be 0 .. channels - 1"),
                       (lambda: fold(channels=0), "channels must be 1..4"), (lambda: fold(bits=0), "tf_bits"), (lambda: fold(bits=9), "tf_bits"),
                       (lambda: fold(kind=_lib.OUT_U16, bits=17), "tf_bits"), (lambda: fold(lanes=3), "power of two"),
                       (lambda: L.brief_view_composite_fold(v, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 0, unaligned, 8, p(k0), p(k0), p(buf), st),
                        "16-byte aligned"),
                       (lambda: L.brief_view_composite_finish(v, bg, p(k0), p(k0), None, p(buf), st), "null buffer"),
                       (lambda: L.brief_view_composite_finish(v, None, p(k0), p(k0), p(buf), p(buf), st), "null background"),
                       (lambda: L.brief_view_composite_finish(v, (C.c_int32 * 3)(0, -1, 0), p(k0), p(k0), p(buf), p(buf), st), "background must be 0 .. 255")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and not k0.cpu().numpy().any()
    m, scale = _net("s22")
    args = (-1.0, 1.0, "u16", scale, V.VRANGE["u16"])
    good = np.zeros((4096, 4), np.int32)
    with pytest.raises(ValueError, match="out_kind must be 'u8' or 'u16'"):
        CP.render_composite(m, view, good, -1.0, 1.0, "f32", scale, V.VRANGE["u16"])
    with pytest.raises(ValueError, match="channel 1 does not exist"):
        CP.render_composite(m, view, good, *args, channel=1)
    with pytest.raises(ValueError, match="background must be three integers"):
        CP.render_composite(m, view, good, *args, background=(0, 0))
    with pytest.raises(ValueError, match="2\\^bits"):
        CP.render_composite(m, view, good[:100], *args)
    bad = good.copy()
    bad[5, 0] = TAU_SAT + 1
    with pytest.raises(ValueError, match="tau must lie in 0 .. TAU_SAT"):
        CP.render_composite(m, view, bad, *args)
    with pytest.raises(ValueError, match="contiguous int32"):
        CP.render_composite(m, view, torch.zeros((4096, 4), dtype=torch.int64, device=DEV), *args)
