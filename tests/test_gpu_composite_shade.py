"""Shaded composite on the GPU (composite.render_composite with shade, csrc/brief_composite.inc) on randomly initialised SIRENs.  Every
comparison is bitwise: the selection and the fold are integer, and the Lambert term is the header's on both sides.
  1  select, pick and shade_fold (compacted and dense) equal brief_view_composite_shade_host fed the device's own values and the
     device's dense Jacobian, for uint8 and uint16 and 1, 4 and 64 lanes per ray;
  2  render_composite(shade=...) equals the host fold fed spatial_gradient of every sample, whatever the chunk: ragged counts of
     selected samples, a chunk that selects one sample, a chunk that selects none; a repeat gives the same bits;
  3  full ambient without diffuse is the plain composite; any shade leaves A and hits alone; a transparent table calls no Jacobian.
Every test asserts that the selection is exercised: 0 < samples_shaded < samples_inside, and a ray reaches TAU_SAT."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import mip
from brief_pytorch_amd import networks as N
from brief_pytorch_amd import view as VW
from tests._composite import TAU_SAT
from tests._variants import VRANGE

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (9, 12, 10)
VIEWS = {"oblique": dict(direction=(0.48, -0.6, 0.64), spacing=0.75, depth_spacing=0.75),      # a few hundred rays of up to ~25 samples
         "axis": dict(direction=(1, 0, 0))}                                                     # 12 x 10 rays of 9 samples each
NETS = {"s22": (dict(layers=4, features=22, data_channel=1), 0, 21),
        "s40": (dict(layers=3, features=40, data_channel=1), 0, 22),                            # two feature tiles
        "s22c2": (dict(layers=4, features=22, data_channel=2), 1, 23)}
TORCH_DT = {"u16": torch.uint16, "u8": torch.uint8}
KIND = {"u8": _lib.OUT_U8, "u16": _lib.OUT_U16}
BITS = {"u8": 8, "u16": 12}
BG = (12, 200, 255)
GSCALE = (3.5, 1.25, -2.0)
LIGHT = (0.3, -0.5, 0.8)
SHADE = (0.2, 0.8)

_cache = {}


def _net(nid):
    if nid not in _cache:
        kw, channel, seed = NETS[nid]
        torch.manual_seed(seed)
        m = N.SIREN(coords_channel=3, features=kw["features"], layers=kw["layers"], data_channel=kw["data_channel"], w0=20).to(DEV)
        f32 = m.decode_grid(DIMS).cpu().numpy()[..., channel]
        q15, q85 = (float(np.float32(q)) for q in np.quantile(f32.astype(np.float64), [0.15, 0.85]))
        assert np.isfinite(f32).all() and q85 > q15
        _cache[nid] = (m, (q15, q85), channel)
    return _cache[nid]


def _table(levels, kind):
    """a table from the quantiles of the device's own integer decode of the view's samples: transparent below the 40 % quantile, a
    ramp of growing density and changing colour, opaque from the 95 % quantile on"""
    bits = BITS[kind]
    idx = levels.astype(np.int64) >> ((8 if kind == "u8" else 16) - bits)
    q40, q95 = (int(q) for q in np.quantile(idx, [0.4, 0.95]))
    assert 0 < q40 < q95 - 4, (q40, q95)
    tf = np.zeros((1 << bits, 4), np.int32)
    rows = np.arange(q40, q95)
    t = (rows - q40 + 1.0) / (q95 - q40)
    tau = np.rint(300 + 50000 * t * t)
    alpha = 1.0 - 2.0 ** (-tau / 65536.0)
    tf[rows, 0] = tau
    tf[rows, 1:] = np.rint(256.0 * np.stack([255 * t, 40 + 160 * (1 - t), 255 * (1 - t)], 1) * alpha[:, None])
    tf[q95:] = [TAU_SAT, 65280, 61000, 52000]
    return CP.check_transfer(tf, kind)[0]


def _setup(nid, kind, vid="oblique"):
    """everything a comparison needs, computed once and left unchanged: the net, the view, the device's compacted list with its values
    and coordinates, the dense Jacobian of every sample, the table, and the host's shaded fold of all that"""
    key = (nid, kind, vid)
    if key not in _cache:
        m, scale, channel = _net(nid)
        view = VW.make_view(DIMS, **VIEWS[vid])
        v = VW._with_range(view, -1.0, 1.0)
        got = {}

        def keep(k0, off, s0, s1, r0, r1, lanes, vals, coords):
            assert s0 == 0 and not got
            got.update(k0=k0, off=off, vals=vals[:s1].clone(), coords=coords[:s1].clone(), lanes=lanes)
        _, total, _ = VW._march(m, v, KIND[kind], TORCH_DT[kind], scale, VRANGE[kind], 1 << 30, keep, with_coords=True)
        assert total == len(got["vals"]) > 1500 if vid == "oblique" else total == 9 * 120
        _, jac = m.spatial_gradient(got["coords"], want_value=False)
        vals = got["vals"].cpu().numpy()
        tf = _table(vals[:, channel], kind)
        ka_q, kd_q = CP.shade_quant(SHADE)
        host = CP.composite_shade_host(v, got["k0"].cpu().numpy(), got["off"].cpu().numpy(), vals, tf, jac.cpu().numpy(), GSCALE, VW._unit3(LIGHT, "light"),
                                       ka_q, kd_q, channel=channel, background=BG)
        s = dict(got, m=m, scale=scale, channel=channel, view=view, v=v, jac=jac, tf=tf, host=host, total=total, kind=kind, ch=m.data_channel)
        _check_selection(s)
        _cache[key] = s
    return _cache[key]


def _check_selection(s):
    """what keeps every test from being vacuous: some samples are selected and some inside samples are not, and a ray saturates"""
    img, hits, run, acc, need = s["host"]
    assert 0 < need.sum() < hits.sum(), (need.sum(), hits.sum())
    assert (run == TAU_SAT).any() and ((run > 0) & (run < TAU_SAT)).any()
    assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) >= 20


def _render(s, **kw):
    kw = {"shade": SHADE, "light": LIGHT, "gscale": GSCALE, **kw}
    img, hits, stats = CP.render_composite(s["m"], s["view"], kw.pop("tf", s["tf"]), -1.0, 1.0, s["kind"], s["scale"], VRANGE[s["kind"]],
                                           channel=s["channel"], background=BG, **kw)
    assert img.is_cuda and img.dtype == torch.uint8 and hits.dtype == torch.int32
    return img.cpu().numpy(), hits.cpu().numpy(), stats


def _shade_desc():
    ka_q, kd_q = CP.shade_quant(SHADE)
    return CP._shade_desc(GSCALE, VW._unit3(LIGHT, "light"), ka_q, kd_q)


def _direct(s, lanes, chunk, compact):
    """select, scan, pick, the Jacobian and shade_fold through the entries themselves, every chunk naming ALL rays; returns the state,
    the image, need and the picked coordinates of the whole list"""
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    v, k0, off, vals, coords, total, ch = s["v"], s["k0"], s["off"], s["vals"], s["coords"], s["total"], s["ch"]
    rays = v.rows * v.cols
    table = torch.from_numpy(s["tf"]).to(DEV)
    sh = _shade_desc()
    hits, run = torch.zeros(rays, dtype=torch.int32, device=DEV), torch.zeros(rays, dtype=torch.int32, device=DEV)
    acc = torch.zeros((rays, 3), dtype=torch.int64, device=DEV)
    needs, picked = [], []
    for s0 in range(0, total, chunk):
        s1 = min(s0 + chunk, total)
        n = s1 - s0
        part, xyz = vals[s0:s1].contiguous(), coords[s0:s1].contiguous()
        head = (C.byref(v), p(k0), p(off), s0, s1, 0, rays, lanes, p(part), KIND[s["kind"]], ch, s["channel"], p(table), BITS[s["kind"]])
        need = torch.full((n,), 7, dtype=torch.int32, device=DEV)
        _lib.check(L.brief_view_composite_select(*head, p(run), p(need), st))
        needs.append(need)
        incl = torch.cumsum(need, 0, dtype=torch.int64)
        m = int(incl[-1].item())
        if m == 0:
            _lib.check(L.brief_view_composite_fold(*head, p(hits), p(run), p(acc), st))
            continue
        if compact:
            slot = incl - need
            sel = torch.full((n, 3), float("nan"), dtype=torch.float32, device=DEV)
            _lib.check(L.brief_view_composite_pick(p(need), p(slot), p(xyz), n, p(sel), st))
            picked.append(sel[:m])
            assert torch.isnan(sel[m:]).all(), "pick wrote behind the selected samples"
            _, jac = s["m"].spatial_gradient(sel[:m], want_value=False)
            _lib.check(L.brief_view_composite_shade_fold(*head, p(need), p(slot), p(jac), C.byref(sh), p(hits), p(run), p(acc), st))
        else:
            jac = s["jac"][s0:s1].contiguous()
            _lib.check(L.brief_view_composite_shade_fold(*head, p(need), None, p(jac), C.byref(sh), p(hits), p(run), p(acc), st))
    img = torch.empty((rays, 4), dtype=torch.uint8, device=DEV)
    _lib.check(L.brief_view_composite_finish(C.byref(v), (C.c_int32 * 3)(*BG), p(hits), p(run), p(acc), p(img), st))
    out = [t.cpu().numpy() for t in (img, hits, run, acc)] + [torch.cat(needs).cpu().numpy()]
    return out, (torch.cat(picked).cpu().numpy() if picked else None)


def _want(s):
    img, hits, run, acc, need = s["host"]
    return [img.reshape(-1, 4), hits.ravel(), run.ravel(), acc.reshape(-1, 3).view(np.int64), need]


# ---- 1: the entries against the host, bit for bit
@pytest.mark.parametrize("nid,kind,vid", [("s22", "u8", "oblique"), ("s22", "u16", "oblique"), ("s40", "u16", "oblique"), ("s22c2", "u8", "oblique"),
                                          ("s22c2", "u16", "axis"), ("s40", "u8", "axis")])
def test_select_pick_and_shade_fold_equal_the_host_on_the_devices_own_values(nid, kind, vid):
    s = _setup(nid, kind, vid)
    want = _want(s)
    need = want[4].astype(bool)
    coords = s["coords"].cpu().numpy()
    for lanes in (1, 4, 64):
        for chunk, compact in ((s["total"], True), (s["total"], False), (61, True), (61, False)):
            got, picked = _direct(s, lanes, chunk, compact)
            for g, w, what in zip(got, want, ("image", "hits", "tau_run", "acc", "need")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (lanes, chunk, compact, what, int((g != w).sum()))
            if compact:                                              # the selected samples, in the list's order
                assert np.array_equal(picked.view(np.int32), coords[need].view(np.int32)), (lanes, chunk)
    if vid == "axis":
        assert (np.diff(s["off"].cpu().numpy()) == DIMS[0]).all(), "rays of equal length"


# ---- 2: the render, compacted and dense, under every chunking
@pytest.mark.parametrize("nid,kind", [("s22", "u16"), ("s40", "u8"), ("s22c2", "u16")])
def test_render_equals_the_host_fold_of_the_dense_jacobian_under_every_chunking(nid, kind):
    s = _setup(nid, kind)
    want_img, want_hits, _, _, need = s["host"]
    m7 = np.add.reduceat(need, np.arange(0, len(need), 7))          # the selected samples of every chunk of 7
    assert (m7 == 0).any() and (m7 == 1).any() and (m7 % 8 != 0).any() and need.sum() % 8 != 0, "no empty, single or ragged selection"
    base = None
    for chunk in (7, 61, 4096, None):
        img, hits, stats = _render(s, chunk=chunk)
        assert np.array_equal(img, want_img) and np.array_equal(hits, want_hits), (chunk, int((img != want_img).sum()))
        assert stats["samples_shaded"] == int(need.sum()) and stats["samples_inside"] == int(want_hits.sum()) == stats["samples_evaluated"]
        assert 0 < stats["samples_shaded"] < stats["samples_inside"]
        base = base or stats
        assert stats == base
    again = _render(s, chunk=61)
    assert np.array_equal(again[0], want_img) and again[2] == base, "a repeat gives other bits"
    dense = _render(s, chunk=61, compact=False)
    assert np.array_equal(dense[0], want_img) and np.array_equal(dense[1], want_hits) and dense[2] == base
    # the options reach the fold: another light, another scale and other weights give other images
    for kw in (dict(light=(1, 0, 0)), dict(gscale=(1, 1, 1)), dict(shade=(0.5, 0.5))):
        other = _render(s, **kw)
        assert not np.array_equal(other[0][..., :3], want_img[..., :3]) and np.array_equal(other[0][..., 3], want_img[..., 3]), kw
    # the defaults: the view's own direction as the light, voxels of extent 1
    from brief_pytorch_amd import gradient
    default = _render(s, light=None, gscale=None)
    named = _render(s, light=list(s["view"].ddepth), gscale=gradient.voxel_scale(list(DIMS), -1.0, 1.0, s["scale"], *VRANGE[kind]))
    assert np.array_equal(default[0], named[0]) and not np.array_equal(default[0], want_img)


# ---- 3: identities
@pytest.mark.parametrize("nid,kind", [("s22", "u8"), ("s22c2", "u16")])
def test_full_ambient_is_the_plain_composite_and_no_shade_touches_opacity(nid, kind):
    s = _setup(nid, kind)
    plain = _render(s, shade=None, light=None, gscale=None)
    assert "samples_shaded" not in plain[2]
    same = _render(s, shade=(1, 0))
    assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1], plain[1])
    assert 0 < same[2]["samples_shaded"] < same[2]["samples_inside"]
    for shade in (SHADE, (0, 1), (0, 0), (0.6, 0.9)):
        img, hits, stats = _render(s, shade=shade, chunk=97)
        assert np.array_equal(img[..., 3], plain[0][..., 3]) and np.array_equal(hits, plain[1]), shade
        assert stats["samples_shaded"] == same[2]["samples_shaded"], "the selection does not depend on the weights"
        assert (img[..., :3] <= plain[0][..., :3]).all(), "a lit emission is at most the emission"
    dark = _render(s, shade=(0, 0))
    lit = plain[1] > 0
    assert not np.array_equal(dark[0], plain[0]) and (dark[0][lit][:, :3].astype(int) <= plain[0][lit][:, :3]).all()


def test_a_transparent_table_shades_nothing_and_calls_no_jacobian(monkeypatch):
    s = _setup("s22", "u16")
    empty = np.zeros_like(s["tf"])
    absorbing = s["tf"].copy()
    absorbing[:, 1:] = 0                                             # absorbs, emits nothing: still no sample needs a gradient

    def never(*a, **kw):
        raise AssertionError("the Jacobian was evaluated")
    monkeypatch.setattr(s["m"], "spatial_gradient", never)
    for tf in (empty, absorbing):
        for chunk in (61, None):
            img, hits, stats = _render(s, tf=tf, chunk=chunk)
            assert stats["samples_shaded"] == 0 and stats["samples_inside"] == int(s["host"][1].sum()) > 0
            assert np.array_equal(hits, s["host"][1])
            plain = _render(s, tf=tf, chunk=chunk, shade=None, light=None, gscale=None)
            assert np.array_equal(img, plain[0])
    img, _, _ = _render(s, tf=empty)
    assert (img == np.array(BG + (0,), np.uint8)).all()
    monkeypatch.undo()
    assert 0 < _render(s)[2]["samples_shaded"] < int(s["host"][1].sum()) and (s["host"][2] == TAU_SAT).any()


# ---- refusals
def test_entries_refuse_bad_arguments_before_any_launch():
    s = _setup("s22", "u8")
    assert 0 < s["host"][4].sum() < s["host"][1].sum() and (s["host"][2] == TAU_SAT).any()
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    v, rays = s["v"], s["v"].rows * s["v"].cols
    i32 = torch.zeros(rays, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(3 * rays, dtype=torch.int64, device=DEV)
    table = torch.from_numpy(s["tf"]).to(DEV)
    head = (C.byref(v), p(s["k0"]), p(s["off"]), 0, 4, 0, 1, 1, p(s["vals"]), KIND["u8"], 1, 0, p(table), 8)
    sh = _shade_desc()

    def desc(**kw):
        d = _shade_desc()
        for k, x in kw.items():
            if k in ("ka_q", "kd_q"):
                setattr(d, k, x)
            else:
                getattr(d, k)[:] = x
        return C.byref(d)
    jac, xyz = s["jac"], s["coords"]
    fold = lambda need=i32, slot=None, j=jac, d=C.byref(sh), hits=i32, run=i32, acc=i64: L.brief_view_composite_shade_fold(
        *head, p(need), p(slot), p(j), d, p(hits), p(run), p(acc), st)
    for call, what in ((lambda: L.brief_view_composite_select(*head, None, p(i32), st), "null buffer"),
                       (lambda: L.brief_view_composite_select(*head, p(i32), None, st), "null buffer"),
                       (lambda: L.brief_view_composite_select(*head[:7], 3, *head[8:], p(i32), p(i32), st), "power of two"),
                       (lambda: L.brief_view_composite_select(*head[:11], 1, *head[12:], p(i32), p(i32), st), "channel must be 0 .. channels - 1"),
                       (lambda: L.brief_view_composite_pick(None, p(i64), p(xyz), 4, p(xyz), st), "null buffer"),
                       (lambda: L.brief_view_composite_pick(p(i32), None, p(xyz), 4, p(xyz), st), "null buffer"),
                       (lambda: L.brief_view_composite_pick(p(i32), p(i64), None, 4, p(xyz), st), "null buffer"),
                       (lambda: L.brief_view_composite_pick(p(i32), p(i64), p(xyz), 4, None, st), "null buffer"),
                       (lambda: L.brief_view_composite_pick(p(i32), p(i64), p(xyz), 0, p(xyz), st), "n must be >= 1"),
                       (lambda: fold(need=None), "null buffer"), (lambda: fold(j=None), "null buffer"), (lambda: fold(acc=None), "null buffer"),
                       (lambda: fold(run=None), "null buffer"), (lambda: fold(d=None), "null shade descriptor"),
                       (lambda: fold(d=desc(ka_q=257)), "ka_q and kd_q must be 0 .. 256"), (lambda: fold(d=desc(kd_q=-1)), "ka_q and kd_q must be 0 .. 256"),
                       (lambda: fold(d=desc(gscale=(1, float("inf"), 1))), "gscale and light must be finite"),
                       (lambda: fold(d=desc(light=(float("nan"), 0, 1))), "gscale and light must be finite")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not i32.cpu().numpy().any() and not i64.cpu().numpy().any()
    # the Python call: a net without the Jacobian kernel is refused before any decode
    torch.manual_seed(3)
    half = N.SIREN(coords_channel=3, features=96, layers=4, data_channel=1, w0=20, precision="bf16").to(DEV)
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*bf16"):
        CP.render_composite(half, s["view"], s["tf"], -1.0, 1.0, "u8", s["scale"], VRANGE["u8"], shade=SHADE)
    with pytest.raises(ValueError, match="light describes the shaded composite"):
        CP.render_composite(s["m"], s["view"], s["tf"], -1.0, 1.0, "u8", s["scale"], VRANGE["u8"], light=LIGHT)
    assert mip.DEFAULT_CHUNK > s["total"]
