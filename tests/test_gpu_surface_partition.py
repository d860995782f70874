"""Surface view of a partition on the GPU (view.render_surface_partition, csrc/brief_surface_part.inc): one randomly initialised 4 x 22
SIREN per block, a distinct seed, integer window and value range per block.  first, t_lo, t_hi, owner, hits, position, normal and shade
are compared BITWISE: the fold and every refinement decision compare decoded integers, a point has one owner, and the shading is the
single-net kernel's arithmetic.
  1  a partition of ONE block covering the grid equals view.render_surface of that net;
  2  the partitions EIGHT and MIX (tests/test_view_partition_host.py, on their own 23 x 31 x 37 volume) equal a numpy restatement: the
     march over the whole lattice (tests/test_gpu_view_partition._restate), the bracket, and a bisection whose every point goes through
     its OWNER's forward entry on brief_view_part_sample_t_host's block-local coordinates;
  3  a face and a gap placed by hand between slabs of constant nets on a 16 x 12 x 10 volume: the hit is exactly the face;
  4  the order of the blocks, chunking and repetition change no bit;  5  mixed net kinds;  6  blocks of different dims scale their own
     normals.
The level is taken from the decoded values: the median over the rays that meet the clip box of the per-ray maximum ('above') or minimum
('below'), so about half of those rays hit; in 2 the quantile nearest that median at which, by the numpy march alone, a quarter of the
rays hit and a bracket straddles a face (_pick_level)."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, gradient, mip
from brief_pytorch_amd import view as VW
from tests import _variants as V
from tests.test_gpu_surface import _np_shade
from tests.test_gpu_view_partition import _forward_int, _restate
from tests.test_view_partition_host import EIGHT, MIX

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (23, 31, 37)
SMALL = (16, 12, 10)
BOX = "3:19,5:26,2:30"
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))
KEYS = ("first", "t_lo", "t_hi", "t", "position", "hits", "owner")
F = np.float32

_cache = {}


def _net(vid, seed):
    torch.manual_seed(seed)
    v = V.BY_ID[vid]
    assert v.cin == 3
    return v.cls(**v.kwargs).to(DEV)


def _block(m, start, dims, kind, i):
    """(phi, start, dims, lo, hi, scale, vrange): the integer window is the 0.15 / 0.85 quantiles of the net's f32 decode of its own grid"""
    f32 = m.decode_grid(dims).cpu().numpy().astype(np.float64)
    q15, q85 = (float(F(q)) for q in np.quantile(f32, [0.15, 0.85]))
    assert np.isfinite(f32).all() and q85 > q15
    lo, hi = V.VRANGE[kind]
    return (m, list(start), list(dims), -1.0, 1.0, (q15, q85), (lo + 2.0 * i, hi - 3.0 * i))


def _partition(name, kind, vid="s22"):
    key = (name, kind, vid)
    if key not in _cache:
        boxes = {"eight": EIGHT, "mix": MIX, "one": [((0, 0, 0), tuple(n - 1 for n in DIMS))]}[name]
        _cache[key] = [_block(_net(vid, 2000 + i), s, [b - a + 1 for a, b in zip(s, e)], kind, i) for i, (s, e) in enumerate(boxes)]
    return _cache[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _render(parts, view, level, kind, **kw):
    out = VW.render_surface_partition(parts, view, level, kind, **kw)
    shape = (view.rows, view.cols)
    for key, dt in (("first", torch.int32), ("hits", torch.int32), ("owner", torch.int32), ("t", torch.float32), ("t_lo", torch.float32),
                    ("t_hi", torch.float32)):
        assert out[key].is_cuda and out[key].dtype == dt and tuple(out[key].shape) == shape, key
    assert tuple(out["position"].shape) == shape + (3,) and out["position"].dtype == torch.float32
    if kw.get("shading", True):
        assert tuple(out["normal"].shape) == shape + (3,) and tuple(out["shade"].shape) == shape
    else:
        assert out["normal"] is None and out["shade"] is None
    assert out["stats"]["blocks"] == len(parts) and out["stats"]["rays"] == view.rows * view.cols
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}


def _passes(x, level, side):
    return x >= level if side == "above" else x <= level


def _level(parts, view, kind, side, channel=0):
    """the median over the rays that meet the clip box of the partition's own max ('above') or min ('below') view"""
    img, hits, _ = VW.render_partition(parts, view, "max" if side == "above" else "min", kind)
    return int(np.median(img.cpu().numpy()[..., channel][hits.cpu().numpy() > 0]))


# ---- 1: one block equals the single-net view
@pytest.mark.parametrize("kind", ["u16", "u8"])
@pytest.mark.parametrize("side", VW.SIDES)
def test_one_block_equals_the_single_net_view(kind, side):
    parts = _partition("one", kind)
    m, _, _, lo, hi, scale, vrange = parts[0]
    bracketed = 0
    for geom in (OBLIQUE, dict(direction=(0, -1, 0)), dict(OBLIQUE, region=BOX), dict(direction=(0, 0, 1), region=BOX)):
        view = VW.make_view(DIMS, **geom)
        level = _level(parts, view, kind, side)
        for refine in (0, 1, 8):
            want = VW.render_surface(m, view, level, lo, hi, kind, scale, vrange, side=side, refine=refine)
            want = {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in want.items()}
            got = _render(parts, view, level, kind, side=side, refine=refine)
            for key in ("first", "t_lo", "t_hi", "position", "normal", "shade", "hits"):
                assert np.array_equal(_bits(got[key]), _bits(want[key])), (geom, refine, key, int((_bits(got[key]) != _bits(want[key])).sum()))
            hit = want["first"] >= 0
            assert np.array_equal(got["owner"], np.where(hit, 0, -1)) and got["stats"]["rays_straddle"] == 0
            for key in ("rays", "rays_hit", "samples_inside", "samples_evaluated", "rays_surface", "rays_cut"):
                assert got["stats"][key] == want["stats"][key], key
            assert got["stats"]["blocks_hit"] == 1 and got["stats"]["refine_launch_blocks"] == (refine if got["stats"]["refine_points"] else 0)
            assert got["stats"]["refine_points"] == refine * (want["stats"]["rays_surface"] - want["stats"]["rays_cut"])
            bracketed += want["stats"]["rays_surface"] - want["stats"]["rays_cut"]
            assert hit.any() and np.abs(got["normal"][hit]).max() > 0
    assert bracketed > 100


# ---- 2: partitions equal the restatement
def _images(parts, view):
    """per block the view with its lo / hi and the descriptor whose window is the whole image (the window plays no part on the host)"""
    return [(VW._with_range(view, p[3], p[4]), VW.make_part(view, p[1], p[2], "image")) for p in parts]


def _points(parts, images, row, col, t):
    """(owner [n] int32, coord [n, 3], pos [n, 3]) of the points (row, col, t): the owner by every block's own half-open cell test, the
    coordinates block-local, all from brief_view_part_sample_t_host"""
    n = len(row)
    owner, coord, pos = np.full(n, -1, np.int32), np.zeros((n, 3), F), np.full((n, 3), np.nan, F)
    if n:
        for i, (v, pt) in enumerate(images):
            p, _, c, _, owned = VW.part_sample_t_host(v, pt, row, col, t)
            assert (owner[owned] == -1).all(), "a point with two owners"
            owner[owned], coord[owned], pos = i, c[owned], p
    return owner, coord, pos


def _values(parts, kind, owner, coord, channel):
    out = np.zeros(len(owner), np.int64)
    for i, (m, _, _, _, _, scale, vrange) in enumerate(parts):
        sel = owner == i
        if sel.any():
            out[sel] = _forward_int(m, coord[sel], kind, scale, vrange)[:, channel]
    return out


def _march_np(parts, view, lattice, level, side, channel=0):
    """the march and the bracket in numpy: (first, hit, bracket, t_lo, t_hi, the owners of the brackets' two ends)"""
    vals, evaluated = lattice
    ok = evaluated & _passes(vals[..., channel], level, side)
    first = np.where(ok.any(2), ok.argmax(2), -1).astype(np.int32)
    k0, _ = VW.clip_host(view)
    hit, bracket = first >= 0, (first >= 0) & (first > k0)
    t_hi = np.where(hit, first, np.nan).astype(F)
    t_lo = np.where(bracket, first - 1, t_hi).astype(F)
    row, col = np.nonzero(bracket)
    ends = [_points(parts, _images(parts, view), row, col, t[bracket])[0] for t in (t_lo, t_hi)]
    return first, hit, bracket, t_lo, t_hi, ends


def _pick_level(parts, view, lattice, side, channel=0):
    """a level taken from the decoded values alone: the quantile nearest the median of the per-ray maximum ('above') or minimum ('below')
    over the rays that meet the clip box at which, by the numpy march, at least a quarter of those rays hit and a bracket straddles"""
    vals, evaluated = lattice
    x, met = vals[..., channel], evaluated.any(2)
    extreme = np.where(evaluated, x, -1).max(2) if side == "above" else np.where(evaluated, x, 1 << 40).min(2)
    for q in (0.5, 0.45, 0.55, 0.4, 0.6, 0.35, 0.65, 0.3, 0.7):
        level = int(np.quantile(extreme[met], q))
        _, hit, _, _, _, ends = _march_np(parts, view, lattice, level, side, channel)
        if hit.sum() >= 0.25 * met.sum() and (ends[0] != ends[1]).any():
            return level
    raise AssertionError("no level near the median gives a straddling bracket: the view does not exercise the routing")


def _restate_surface(parts, view, lattice, kind, level, side, refine, channel=0, voxel_size=(1, 1, 1), light=None, shading=True):
    """the whole view in numpy: march, bracket, bisection, hit and shading.  lattice: _restate's (vals, evaluated)"""
    evaluated = lattice[1]
    first, hit, bracket, t_lo, t_hi, ends = _march_np(parts, view, lattice, level, side, channel)
    images = _images(parts, view)
    row, col = np.nonzero(bracket)
    assert (ends[1] >= 0).all()
    facts = dict(rays_straddle=int((ends[0] != ends[1]).sum()), refine_points=0, refine_launch_blocks=0, gap_points=0, far_side=0)
    for _ in range(refine):
        lo, hi = t_lo[bracket], t_hi[bracket]
        mid = lo + F(0.5) * (hi - lo)
        assert mid.dtype == F
        owner, coord, _ = _points(parts, images, row, col, mid)
        passed = (owner >= 0) & _passes(_values(parts, kind, owner, coord, channel), level, side)      # the gap rule: an unowned point fails
        t_hi[bracket], t_lo[bracket] = np.where(passed, mid, hi), np.where(passed, lo, mid)
        facts["refine_points"] += int((owner >= 0).sum())
        facts["refine_launch_blocks"] += len(set(owner[owner >= 0].tolist()))
        facts["gap_points"] += int((owner < 0).sum())
        facts["far_side"] += int((owner != ends[1]).sum())         # points evaluated by another block than the first hit's
    row, col = np.nonzero(hit)
    owner, coord, pos = _points(parts, images, row, col, t_hi[hit])
    assert (owner >= 0).all()
    shape = first.shape
    out = dict(first=first, t_lo=t_lo, t_hi=t_hi, t=t_hi, hits=evaluated.sum(2).astype(np.int32), owner=np.full(shape, -1, np.int32),
               position=np.full(shape + (3,), np.nan, F), normal=None, shade=None, facts=facts)
    out["owner"][hit], out["position"][hit] = owner, pos
    if shading:
        l = np.array(list(view.ddepth), np.float64) if light is None else np.asarray(light, np.float64)
        l = l / np.linalg.norm(l)
        normal, shade = np.zeros((len(row), 3), F), np.zeros(len(row), F)
        for i, (m, _, dims, lo, hi, scale, vrange) in enumerate(parts):
            sel = owner == i
            if sel.any():
                _, jac = m.spatial_gradient(torch.from_numpy(coord[sel]).to(DEV), want_value=False)
                g = gradient.voxel_scale(dims, lo, hi, scale, *vrange) / np.asarray(voxel_size, np.float64)
                normal[sel], shade[sel] = _np_shade(jac.cpu().numpy(), channel, g, side, l)
        out["normal"], out["shade"] = np.zeros(shape + (3,), F), np.zeros(shape, F)
        out["normal"][hit], out["shade"][hit] = normal, shade
    return out


def _lattice(name, kind, geom_key, view):
    key = ("lattice", name, kind, geom_key)
    if key not in _cache:
        vals, evaluated, _ = _restate(_partition(name, kind), view, kind)
        vals.setflags(write=False)
        _cache[key] = (vals, evaluated)
    return _cache[key]


GEOMS = {"oblique": [OBLIQUE], "box": [dict(OBLIQUE, region=BOX, depth_spacing=0.3, spacing=2.3)]}
# axis-aligned, half a voxel between samples: every other sample lies exactly on a plane s - 0.5, so a bracket that straddles a face ends
# ON it.  Whether a ray's first hit is the first sample behind a face depends on the nets: the clip box starts a voxel or two in front of
# a face of both partitions (z = 11.5, y = 13.5, x = 20.5), and the first of these views whose numpy march straddles is taken
GEOMS["axis"] = [dict(direction=d, spacing=1.5, depth_spacing=0.5, region=r) for d, r in (
    ((1, 0, 0), "10:23,:,:"), ((1, 0, 0), "11:23,:,:"), ((0, 0, 1), ":,:,19:37"), ((0, 0, 1), ":,:,20:37"), ((0, 1, 0), ":,12:31,:"),
    ((0, 1, 0), ":,13:31,:"), ((1, 0, 0), None), ((0, 0, 1), None), ((0, 1, 0), None), ((-1, 0, 0), None), ((0, 0, -1), None))]


def _compare(got, want, keys, what):
    for key in keys:
        a, b = _bits(got[key]), _bits(want[key])
        print("%s %s: %d of %d entries differ" % (what, key, int((a != b).sum()), a.size))
    for key in keys:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (what, key)


@pytest.mark.parametrize("name,kind,side", [("eight", "u16", "above"), ("mix", "u8", "below"), ("mix", "u16", "above")])
def test_partitions_equal_the_restatement(name, kind, side):
    parts = _partition(name, kind)
    for gname, geoms in GEOMS.items():
        for i, geom in enumerate(geoms):
            view = VW.make_view(DIMS, **geom)
            lattice = _lattice(name, kind, (gname, i), view)
            try:
                level = _pick_level(parts, view, lattice, side)
                break
            except AssertionError:
                assert i + 1 < len(geoms), "no %s view of this partition has a bracket that straddles a face" % gname
        vs = geom.get("voxel_size", (1, 1, 1))
        want = _restate_surface(parts, view, lattice, kind, level, side, 8, voxel_size=vs)
        got = _render(parts, view, level, kind, side=side, refine=8, voxel_size=vs)
        _compare(got, want, KEYS + ("normal", "shade"), "%s %s %s %s" % (name, kind, side, gname))
        stats, facts = got["stats"], want["facts"]
        hit = want["first"] >= 0
        print("%s: %d of %d rays that meet the box hit, %d straddle, %d refinement points on the far side of a face" % (
            gname, int(hit.sum()), stats["rays_hit"], facts["rays_straddle"], facts["far_side"]))
        # what keeps this from being vacuous: at least a quarter of the rays hit, a bracket straddles a face
        assert stats["rays_surface"] == int(hit.sum()) >= 0.25 * stats["rays_hit"] and stats["rays_straddle"] == facts["rays_straddle"] >= 1
        assert stats["refine_points"] == facts["refine_points"] > 0 and stats["refine_launch_blocks"] == facts["refine_launch_blocks"]
        assert facts["gap_points"] == 0 and stats["samples_evaluated"] == stats["samples_inside"] == int(lattice[1].sum())
        assert stats["blocks_hit"] == len(parts) and stats["rays_clipped"] < len(parts) * stats["rays"]
        assert len(set(got["owner"][hit].tolist())) >= 2 and (got["owner"][~hit] == -1).all()
        unit = np.linalg.norm(got["normal"][hit].astype(np.float64), axis=1)
        assert (np.abs(unit - 1) <= 1e-5).all() and not got["normal"][~hit].any() and not got["shade"][~hit].any()
        # refine 0 and 1 on the same march
        for refine in (0, 1):
            want = _restate_surface(parts, view, lattice, kind, level, side, refine, shading=False)
            got = _render(parts, view, level, kind, side=side, refine=refine, shading=False)
            _compare(got, want, KEYS, "%s refine %d" % (gname, refine))


# ---- 3: a face and a gap, analytically
def _constant(value):
    """a 4 x 22 SIREN whose output is `value` everywhere: all weights zero, the head's bias set"""
    m = _net("s22", 1)
    m.params.zero_()
    V.head_bias(m).data = torch.tensor([value])
    return m


def _slab(m, z0, z1, vrange=(0.0, 60000.0)):
    return (m, [z0, 0, 0], [z1 - z0 + 1, SMALL[1], SMALL[2]], -1.0, 1.0, (-1.0, 1.0), vrange)


def _decoded(part):
    return int(_forward_int(part[0], np.zeros((1, 3), F), "u16", part[5], part[6])[0, 0])


def test_the_face_analytically():
    s = 7
    parts = [_slab(_constant(-0.5), 0, s - 1), _slab(_constant(0.5), s, SMALL[0] - 1)]
    below, level = _decoded(parts[0]), _decoded(parts[1])
    assert below < level                                         # the lower block decodes below the level, the upper AT it
    view = VW.make_view(SMALL, (1, 0, 0))                        # unit view along +z: sample k sits at z = k
    assert (view.rows, view.cols, view.depth) == (SMALL[1], SMALL[2], SMALL[0])
    for order in (parts, parts[::-1]):
        upper = order.index(parts[1])
        for refine in (0, 1, 2, 8, 16):
            got = _render(order, view, level, "u16", refine=refine)
            assert (got["first"] == s).all() and (got["owner"] == upper).all() and (got["hits"] == SMALL[0]).all()
            assert (got["t"] == (s - 0.5 if refine else s)).all(), refine
            assert (got["position"][..., 0] == got["t"]).all()
            assert not got["normal"].any() and not got["shade"].any()      # the gradient of a constant is zero
            if refine:
                assert (got["t_lo"] == F(s - 0.5) - F(2.0 ** -refine)).all()
            stats = got["stats"]
            assert stats["rays_straddle"] == stats["rays_surface"] == stats["rays"] and stats["rays_cut"] == 0
            assert stats["refine_points"] == refine * stats["rays"]
            assert stats["refine_launch_blocks"] == refine        # every round's points lie in ONE block: the upper first, then the lower
    # 'below' from the other end of the volume: the first sample of the lower block, met from above
    back = VW.make_view(SMALL, (-1, 0, 0))
    got = _render(parts, back, below, "u16", side="below", refine=8)
    k = SMALL[0] - 1 - (s - 1)                                   # sample k sits at z = 15 - k
    assert (got["first"] == k).all() and (got["owner"] == 0).all()
    # the midpoint k - 0.5 is z = 7 - 0.5, the UPPER block's: it fails 'below'; every later midpoint is the lower block's and passes
    assert (got["t_lo"] == k - 0.5).all() and (got["t"] == F(k - 0.5) + F(2.0 ** -8)).all()
    assert (got["position"][..., 0] == F(s - 0.5) - F(2.0 ** -8)).all()


def test_the_gap_rule():
    a, b = 5, 10                                                 # slabs 0 .. 4 and 10 .. 15; 5 .. 9 is left out
    near, far = _slab(_constant(-0.5), 0, a - 1), _slab(_constant(0.5), b, SMALL[0] - 1)
    level = _decoded(far)
    assert _decoded(near) < level
    view = VW.make_view(SMALL, (1, 0, 0))
    owned = (a + SMALL[0] - b) * view.rows * view.cols
    for parts in ([near, far], [far, near]):
        upper = parts.index(far)
        for refine in (0, 1, 3, 8):
            got = _render(parts, view, level, "u16", refine=refine)
            assert (got["first"] == b).all() and (got["owner"] == upper).all() and (got["hits"] == a + SMALL[0] - b).all()
            assert (got["t"] == (b - 0.5 if refine else b)).all()      # exactly the far slab's lower face
            stats = got["stats"]
            assert stats["samples_evaluated"] == stats["samples_inside"] == owned      # nothing in the gap is evaluated
            assert stats["rays_straddle"] == stats["rays"]                 # the lower end of every bracket, 9, lies in the gap
            assert stats["refine_points"] == (stats["rays"] if refine else 0) and stats["refine_launch_blocks"] == min(refine, 1)
            if refine:
                assert (got["t_lo"] == F(b - 0.5) - F(2.0 ** -refine)).all()
    # the clip box starts inside the far slab: every ray is cut, nothing is refined
    cut = VW.make_view(SMALL, (1, 0, 0), region="12:16,:,:")
    got = _render([near, far], cut, level, "u16", refine=8)
    stats = got["stats"]
    assert (got["first"] == 0).all() and (got["t"] == 0).all() and (got["t_lo"] == 0).all() and (got["position"][..., 0] == 12).all()
    assert stats["rays_cut"] == stats["rays_surface"] == stats["rays"] and stats["refine_points"] == 0 and stats["rays_straddle"] == 0
    assert stats["blocks_hit"] == 1 and (got["owner"] == 1).all()
    # a ray that meets only the gap finds nothing
    gap = VW.make_view(SMALL, (0, 0, 1), region="6:9,:,:")
    got = _render([near, far], gap, level, "u16", refine=8)
    assert (got["first"] == -1).all() and np.isnan(got["t"]).all() and (got["owner"] == -1).all() and got["stats"]["samples_evaluated"] == 0


# ---- 4: block order, chunking and repetition
def test_block_order_chunking_and_repetition_change_no_bit(monkeypatch):
    parts = _partition("eight", "u16")
    view = VW.make_view(DIMS, depth=(-5.0, 5.0), size=(12, 14), **OBLIQUE)
    level = _level(parts, view, "u16", "above")
    ref = _render(parts, view, level, "u16", refine=8, voxel_size=OBLIQUE["voxel_size"])
    total = ref["stats"]["samples_evaluated"]
    assert total > 500 and ref["stats"]["rays_straddle"] >= 1 and ref["stats"]["rays_surface"] > ref["stats"]["rays_cut"]
    shuffled = [parts[i] for i in np.random.default_rng(3).permutation(len(parts))]
    keys = KEYS + ("normal", "shade")

    def same(order, **kw):
        got = _render(order, view, level, "u16", refine=8, voxel_size=OBLIQUE["voxel_size"], **kw)
        index = np.array([parts.index(p) for p in order] + [-1], np.int32)      # the owner is an index in the order given
        got["owner"] = index[got["owner"]]
        for key in keys:
            assert np.array_equal(_bits(got[key]), _bits(ref[key])), (key, kw)
        assert got["stats"] == ref["stats"]
    for order in (parts, parts[::-1], shuffled):
        for chunk in (None, 257, total) + ((1,) if order is shuffled else ()):
            same(order, chunk=chunk)
    monkeypatch.setattr(mip, "DEFAULT_CHUNK", 5)                 # the buckets of a round are cut into lists of 5 rays
    same(shuffled)


# ---- 5: mixed kinds
def test_mixed_kinds_are_refused_with_shading_and_served_without():
    kind = "u16"
    boxes = [((0, 0, 0), (11, 30, 36)), ((12, 0, 0), (22, 30, 36))]
    nets = [_net("s22", 31), V.BY_ID["mfnf"].cls(**dict(V.BY_ID["mfnf"].kwargs, data_channel=1)).to(DEV)]
    parts = [_block(m, s, [b - a + 1 for a, b in zip(s, e)], kind, i) for i, (m, (s, e)) in enumerate(zip(nets, boxes))]
    view = VW.make_view(DIMS, **OBLIQUE)
    seen = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="block at \\[12, 0, 0\\] has none.*MFNFourier.*shading=False"):
        VW.render_surface_partition(parts, view, 20000, kind, voxel_size=OBLIQUE["voxel_size"])
    assert torch.cuda.memory_allocated() == seen                 # refused before any buffer of the march exists
    level = _level(parts, view, kind, "above")
    vals, evaluated, _ = _restate(parts, view, kind)
    want = _restate_surface(parts, view, (vals, evaluated), kind, level, "above", 8, shading=False)
    got = _render(parts, view, level, kind, refine=8, shading=False)
    _compare(got, want, KEYS, "mixed")
    hit = want["first"] >= 0
    assert set(got["owner"][hit].tolist()) == {0, 1} and got["stats"]["rays_straddle"] == want["facts"]["rays_straddle"] >= 1


# ---- 6: blocks of different dims
def test_blocks_of_different_dims_scale_their_own_normals():
    kind = "u16"
    vol = (12, 12, 10)
    boxes = [((0, 0, 0), (7, 11, 9)), ((8, 0, 0), (11, 11, 9))]      # 8 and 4 voxels along z
    parts = [_block(_net("s22", 41 + i), s, [b - a + 1 for a, b in zip(s, e)], kind, i) for i, (s, e) in enumerate(boxes)]
    vs = (0.5, 1.0, 2.0)
    scales = [gradient.voxel_scale(p[2], p[3], p[4], p[5], *p[6]) / np.array(vs) for p in parts]
    assert not np.allclose(scales[0][0], scales[1][0])
    view = VW.make_view(vol, (0.3, 0.5, -0.81), spacing=0.9, depth_spacing=0.5, voxel_size=vs)
    level = _level(parts, view, kind, "above")
    vals, evaluated, _ = _restate(parts, view, kind)
    light = (0.0, 0.6, -0.8)
    want = _restate_surface(parts, view, (vals, evaluated), kind, level, "above", 8, voxel_size=vs, light=light)
    got = _render(parts, view, level, kind, refine=8, voxel_size=vs, light=light)
    _compare(got, want, KEYS + ("normal", "shade"), "dims")
    hit = want["first"] >= 0
    assert set(got["owner"][hit].tolist()) == {0, 1}
    # a normal is its OWNER's gradient under its owner's scale: with the other block's scale the restatement differs
    swapped = [(p[0], p[1], q[2], p[3], p[4], p[5], p[6]) for p, q in zip(parts, parts[::-1])]
    images = _images(parts, view)
    row, col = np.nonzero(hit)
    owner, coord, _ = _points(parts, images, row, col, got["t"][hit])
    differ = 0
    for i, p in enumerate(swapped):
        sel = owner == i
        _, jac = p[0].spatial_gradient(torch.from_numpy(coord[sel]).to(DEV), want_value=False)
        g = gradient.voxel_scale(p[2], p[3], p[4], p[5], *p[6]) / np.array(vs)
        differ += int((_np_shade(jac.cpu().numpy(), 0, g, "above", light)[0] != got["normal"][hit][sel]).any(1).sum())
    assert differ > 0
