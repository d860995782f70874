"""Host side of the surface view of a partition (view.render_surface_partition / decompress_divide_surface, decompress.py
--view-surface-gap): the routing rule of csrc/brief_view.h against a float32 numpy restatement, the entries' and the artefact path's
refusals.  Nothing here needs a GPU: brief_surface_part_route_host and brief_view_part_sample_t_host run the header the kernels run, on
the host CPU.  The partitions are EIGHT and MIX of tests/test_view_partition_host.py on their own 23 x 31 x 37 volume (their blocks are
index ranges of it), and slabs of a 16 x 12 x 10 volume where a face or a gap is placed by hand."""
import ctypes as C
import importlib.util
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from brief_pytorch_amd import _lib
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR, decompress_divide_surface
from tests import _variants
from tests.test_view_host import fl
from tests.test_view_partition_host import DIMS, EIGHT, MIX, OBLIQUE, TWO, _opt, _parts, _side, _tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTITIONS = {"eight": EIGHT, "mix": MIX}
VIEWS = {"oblique": OBLIQUE, "z": dict(direction=(1, 0, 0)), "z@0.5": dict(direction=(1, 0, 0), spacing=0.5, depth_spacing=0.5),
         "-y": dict(direction=(0, -1, 0))}
SMALL = (16, 12, 10)
F = np.float32

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")


# ---- the header's rules in float32 numpy: every operation rounds once (numpy's float32 arithmetic), nothing is fused
def _f3(x):
    return np.array(list(x), F)


def np_mid(lo, hi):
    return (lo + F(0.5) * (hi - lo)).astype(F)


def np_pos(view, row, col, t):
    """p_a = fl(fl(fl(origin + fl(row * drow)) + fl(col * dcol)) + fl(t * ddepth)), [n, 3]"""
    row, col, t = (np.asarray(x, F).ravel()[:, None] for x in (row, col, t))
    base = (_f3(view.origin) + row * _f3(view.drow)) + col * _f3(view.dcol)
    return (base + t * _f3(view.ddepth)).astype(F)


def np_owned(start, dims, p):
    s, n = np.array(start, F), np.array(dims, F)
    return ((s - F(0.5) <= p) & (p < (s + n) - F(0.5))).all(1)


def np_route(view, boxes, t_lo, t_hi, mid):
    """(owner, t_lo, owners per point) of one round, per image ray: the restatement of brief_view_part_route"""
    rows, cols = view.rows, view.cols
    row, col = (x.ravel() for x in np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij"))
    lo, hi = np.array(t_lo, F).ravel().copy(), np.array(t_hi, F).ravel()
    with np.errstate(invalid="ignore"):
        live = (lo < hi) if mid else ~np.isnan(hi)
        t = np.where(lo < hi, np_mid(lo, hi), hi) if mid else hi
    p = np_pos(view, row, col, np.where(live, t, F(0)))
    owner, count = np.full(rows * cols, -1, np.int32), np.zeros(rows * cols, np.int32)
    for i, (s, e) in reversed(list(enumerate(boxes))):            # (the first block that owns a point wins)
        own = np_owned(s, [b - a + 1 for a, b in zip(s, e)], p) & live
        owner[own] = i
        count += own
    if mid:
        gap = live & (owner < 0)
        lo[gap] = t[gap]
    return owner.reshape(rows, cols), lo.reshape(rows, cols), count.reshape(rows, cols), live.reshape(rows, cols), p


def _brackets(view, rng):
    """a bracket per ray as the march leaves it: (first - 1, first) for a random inside sample, (first, first) for a cut ray, NaN where
    the ray misses the clip box or finds nothing"""
    k0, cnt = V.clip_host(view)
    first = k0 + (rng.random(k0.shape) * cnt).astype(np.int32)
    hi = first.astype(F)
    lo = np.where(first > k0, first - 1, first).astype(F)
    none = (cnt == 0) | (rng.random(k0.shape) < 0.1)
    lo[none] = hi[none] = np.nan
    return lo, hi


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@needs_lib
@pytest.mark.parametrize("vname", list(VIEWS))
@pytest.mark.parametrize("pname", list(PARTITIONS))
def test_route_equals_the_numpy_restatement_and_every_point_has_one_owner(pname, vname):
    boxes = PARTITIONS[pname]
    rng = np.random.default_rng(5)
    for region in (None, "3:19,5:26,2:30"):
        view = V.make_view(DIMS, region=region, **VIEWS[vname])
        pts = _parts(view, boxes)
        lo, hi = _brackets(view, rng)
        routed = 0
        for rnd in range(4):
            owner, lo2 = V.route_host(view, pts, lo, hi, True)
            want, want_lo, count, live, _ = np_route(view, boxes, lo, hi, True)
            assert np.array_equal(owner, want) and _same(lo2, want_lo), (pname, vname, region, rnd)
            # a tiling partition: every point inside the clip box has exactly ONE owner, and t_lo never moves
            assert (count[live] == 1).all() and (owner[live] >= 0).all() and (owner[~live] == -1).all() and _same(lo2, lo)
            routed += int(live.sum())
            mid = np_mid(lo, hi)
            passes = rng.random(lo.shape) < 0.5                   # step the brackets as a decode might
            lo, hi = np.where(live & ~passes, mid, lo).astype(F), np.where(live & passes, mid, hi).astype(F)
        assert routed > 100
        owner, lo2 = V.route_host(view, pts, lo, hi, False)       # the hit itself
        want, _, count, live, _ = np_route(view, boxes, lo, hi, False)
        assert np.array_equal(owner, want) and _same(lo2, lo) and (count[live] == 1).all() and np.array_equal(live, ~np.isnan(hi))


def _exact_coord(view, part, p):
    """the block-local coordinate of the fp32 position p, every operation of csrc/brief_view.h rounded once (exact rationals)"""
    f = lambda x: Fr(float(x))
    out = []
    for a in range(3):
        s, n = int(part.start[a]), int(part.dims[a])
        q = fl(f(p[a]) - s)
        step = fl(fl(f(view.hi) - f(view.lo)) / (n - 1))
        out.append(fl(step * q + f(view.lo)) if q < n // 2 else fl(-step * fl((n - 1) - q) + f(view.hi)))
    return out


@needs_lib
@pytest.mark.parametrize("vname", ["oblique", "z@0.5"])
def test_sample_t_equals_the_restatement_and_the_integer_sample(vname):
    view = V.make_view(DIMS, region="3:19,5:26,2:30", **VIEWS[vname])
    view.lo, view.hi = 0.0, 1.0
    rng = np.random.default_rng(11)
    n = 400
    row, col = rng.integers(0, view.rows, n), rng.integers(0, view.cols, n)
    k = rng.integers(0, view.depth, n)
    t = np.where(rng.random(n) < 0.5, k, rng.random(n) * (view.depth - 1)).astype(F)
    t[:8] = k[:8] + F(0.5) if view.depth > 9 else t[:8]
    t = np.minimum(t, F(view.depth - 1))
    seen = set()
    for (s, e), part in list(zip(MIX, _parts(view, MIX)))[::2]:
        pos, local, coord, inside, owned = V.part_sample_t_host(view, part, row, col, t)
        p = np_pos(view, row, col, t)
        assert _same(pos, p) and _same(local, (p - np.array(s, F)).astype(F))
        assert np.array_equal(owned, np_owned(s, [b - a + 1 for a, b in zip(s, e)], p))
        assert np.array_equal(inside, ((_f3(view.box_lo) <= p) & (p <= _f3(view.box_hi))).all(1))
        for i in range(0, n, 7):
            assert [Fr(float(x)) for x in coord[i]] == _exact_coord(view, part, pos[i]), (s, i)
        seen |= set(zip(inside.tolist(), owned.tolist()))
        whole = t == np.floor(t)                                  # at an integer t: part_sample_host's sample, bit for bit
        assert whole.sum() > 100
        for got, want in zip((pos, local, coord, inside, owned), V.part_sample_host(view, part, row[whole], col[whole], t[whole].astype(np.int32))):
            assert np.array_equal(got[whole].view(np.uint8), want.view(np.uint8))
    assert len(seen) >= (2 if "@" in vname else 3)               # (an axis-aligned view of the clip box has no point outside it)


def _slabs(view, z_ranges):
    return [V.make_part(view, (a, 0, 0), (b - a + 1, SMALL[1], SMALL[2])) for a, b in z_ranges]


@needs_lib
def test_a_point_exactly_on_a_face_goes_to_the_upper_block():
    view = V.make_view(SMALL, (1, 0, 0))                        # rays along +z, sample k at z = k
    assert (view.rows, view.cols, view.depth) == (SMALL[1], SMALL[2], SMALL[0])
    pts = _slabs(view, [(0, 6), (7, 15)])
    shape = (view.rows, view.cols)
    lo, hi = np.full(shape, 6, F), np.full(shape, 7, F)
    owner, lo2 = V.route_host(view, pts, lo, hi, True)            # the midpoint 6.5 is the face 7 - 0.5
    assert (owner == 1).all() and _same(lo2, lo)
    pos, local, _, inside, owned = V.part_sample_t_host(view, pts[1], [3], [4], [6.5])
    assert pos[0, 0] == 6.5 and local[0, 0] == -0.5 and owned[0] and inside[0]
    assert not V.part_sample_t_host(view, pts[0], [3], [4], [6.5])[4][0]
    for t_hi, want in ((6.5, 1), (np.nextafter(F(6.5), F(0)), 0), (15.0, 1), (0.0, 0)):
        assert (V.route_host(view, pts, lo, np.full(shape, t_hi, F), False)[0] == want).all(), t_hi
    # the other direction: positions fall with k, the face is met from above
    back = V.make_view(SMALL, (-1, 0, 0))
    pts = _slabs(back, [(0, 6), (7, 15)])
    lo, hi = np.full(shape, 15 - 7, F), np.full(shape, 15 - 6, F)
    assert np_pos(back, [0], [0], [8.5])[0, 0] == 6.5
    assert (V.route_host(back, pts, lo, hi, True)[0] == 1).all()


@needs_lib
def test_a_point_in_a_gap_has_no_owner_and_moves_t_lo():
    view = V.make_view(SMALL, (1, 0, 0))
    pts = _slabs(view, [(0, 4), (10, 15)])                        # the slab 5 .. 9 is left out: the gap is 4.5 <= z < 9.5
    shape = (view.rows, view.cols)
    lo, hi = np.full(shape, 9, F), np.full(shape, 10, F)
    lo[0, :], hi[0, :] = 6, 8                                     # a bracket wholly inside the gap
    lo[1, :], hi[1, :] = np.nan, np.nan
    lo[2, :], hi[2, :] = 3, 3                                     # a cut ray
    owner, lo2 = V.route_host(view, pts, lo, hi, True)
    assert (owner[3:] == 1).all() and _same(lo2[3:], lo[3:])      # 9.5 is the far slab's lower face: owned
    assert (owner[:3] == -1).all() and (lo2[0] == 7).all() and np.isnan(lo2[1]).all() and (lo2[2] == 3).all()
    lo, hi = np.full(shape, 9, F), np.full(shape, 9.5, F)          # the next round: 9.25 lies in the gap
    owner, lo2 = V.route_host(view, pts, lo, hi, True)
    assert (owner == -1).all() and (lo2 == 9.25).all()
    assert (V.route_host(view, pts, lo, np.full(shape, 7.0, F), False)[0] == -1).all() and (V.route_host(view, pts, lo, hi, False)[0] == 1).all()
    want = np_route(view, [((0, 0, 0), (4, 11, 9)), ((10, 0, 0), (15, 11, 9))], lo, hi, True)
    assert np.array_equal(owner, want[0]) and _same(lo2, want[1])


# ---- the entries refuse bad arguments by name, before any work
@needs_lib
def test_entries_refuse_bad_arguments_by_name():
    L = _lib.lib()
    view = V.make_view(SMALL, (1, 0, 0))
    pts = _slabs(view, [(0, 6), (7, 15)])
    rays = view.rows * view.cols
    arr = V._part_array(pts)
    table = C.cast(arr, C.c_void_p)
    f = np.zeros((4, rays * 3), F)
    i32, i64 = np.zeros(rays, np.int32), np.zeros(rays + 1, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    v, pt = C.byref(view), C.byref(pts[0])
    three = (C.c_float * 3)(1, 1, 1)
    nan3 = (C.c_float * 3)(1, float("nan"), 1)
    bad = _lib.ViewPart.from_buffer_copy(pts[0])
    bad.dims[0] = 40
    bad_table = C.cast(V._part_array([pts[1], bad]), C.c_void_p)
    big = V.make_view((1 << 23, 4, 4), (0, 0, 1), size=(4, 4))
    small_part = C.byref(V.make_part(view, (0, 0, 0), (4, 4, 4)))
    fold, route, coords, step, shade = (getattr(L, "brief_surface_part_" + n) for n in ("fold", "route", "coords", "step", "shade"))
    host, sample = L.brief_surface_part_route_host, L.brief_view_part_sample_t_host
    n_w = pts[0].wrows * pts[0].wcols
    for call, what in (
            (lambda: host(v, table, 0, p(f[0]), p(f[1]), 1, p(i32)), "nparts must be 1 .. 2^31 - 1"),
            (lambda: host(v, table, -3, p(f[0]), p(f[1]), 1, p(i32)), "nparts"),
            (lambda: host(v, None, 2, p(f[0]), p(f[1]), 1, p(i32)), "null buffer"),
            (lambda: host(v, table, 2, None, p(f[1]), 1, p(i32)), "null buffer"),
            (lambda: host(v, table, 2, p(f[0]), p(f[1]), 1, None), "null buffer"),
            (lambda: host(v, table, 2, p(f[0]), p(f[1]), 2, p(i32)), "midpoint must be 0"),
            (lambda: host(v, bad_table, 2, p(f[0]), p(f[1]), 1, p(i32)), "start + dims"),
            (lambda: host(C.byref(big), table, 2, p(f[0]), p(f[1]), 1, p(i32)), "2^23"),
            (lambda: host(None, table, 2, p(f[0]), p(f[1]), 1, p(i32)), "null descriptor"),
            (lambda: route(v, table, 0, p(f[0]), p(f[1]), 1, p(i32), None), "nparts"),
            (lambda: route(v, table, 2, p(f[0]), None, 1, p(i32), None), "null buffer"),
            (lambda: route(v, table, 2, p(f[0]), p(f[1]), -1, p(i32), None), "midpoint"),
            (lambda: route(C.byref(big), table, 2, p(f[0]), p(f[1]), 1, p(i32), None), "2^23"),
            (lambda: sample(v, pt, p(i32), p(i32), None, 1, p(f[0]), None, None, None, None), "null index buffer"),
            (lambda: sample(v, pt, p(i32), p(i32), p(np.array([view.depth - 0.5], F)), 1, p(f[0]), None, None, None, None), "[0, depth - 1]"),
            (lambda: sample(v, pt, p(i32), p(i32), p(np.array([np.nan], F)), 1, p(f[0]), None, None, None, None), "[0, depth - 1]"),
            (lambda: sample(v, C.byref(bad), p(i32), p(i32), p(f[1]), 1, p(f[0]), None, None, None, None), "start + dims"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 0, 0, 1, 1, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(i32), p(i32), None), "sample range"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, n_w + 1, 1, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(i32), p(i32), None), "wrows * wcols"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, 1, 3, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(i32), p(i32), None), "power of two"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, 1, 1, p(i32), _lib.OUT_F32, 1, 0, 9, 0, p(i32), p(i32), None), "elem_kind"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, 1, 1, p(i32), _lib.OUT_U8, 1, 0, 256, 0, p(i32), p(i32), None), "level"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, 1, 1, p(i32), _lib.OUT_U8, 1, 1, 9, 0, p(i32), p(i32), None), "channel must be"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, 1, 1, p(i32), _lib.OUT_U8, 1, 0, 9, 2, p(i32), p(i32), None), "side"),
            (lambda: fold(v, pt, p(i32), p(i64), 0, 4, 0, 1, 1, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(i32), None, None), "null buffer"),
            (lambda: fold(v, C.byref(bad), p(i32), p(i64), 0, 4, 0, 1, 1, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(i32), p(i32), None), "start + dims"),
            (lambda: coords(v, pt, p(f[0]), p(f[1]), 1, None, 4, p(f[2]), None, None), "list of rays"),
            (lambda: coords(v, pt, p(f[0]), p(f[1]), 1, p(i64), 0, p(f[2]), None, None), "n >= 1"),
            (lambda: coords(v, pt, p(f[0]), p(f[1]), 3, p(i64), 4, p(f[2]), None, None), "midpoint"),
            (lambda: coords(v, pt, p(f[0]), p(f[1]), 1, p(i64), 4, None, None, None), "pos alone may be NULL"),
            (lambda: coords(C.byref(big), small_part, p(f[0]), p(f[1]), 1, p(i64), 4, p(f[2]), None, None), "2^23"),
            (lambda: step(None, 4, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(f[0]), p(f[1]), None), "list of rays"),
            (lambda: step(p(i64), -1, p(i32), _lib.OUT_U8, 1, 0, 9, 0, p(f[0]), p(f[1]), None), "n >= 1"),
            (lambda: step(p(i64), 4, None, _lib.OUT_U8, 1, 0, 9, 0, p(f[0]), p(f[1]), None), "null buffer"),
            (lambda: step(p(i64), 4, p(i32), _lib.OUT_U16, 1, 0, 65536, 0, p(f[0]), p(f[1]), None), "level"),
            (lambda: step(p(i64), 4, p(i32), _lib.OUT_U8, 5, 0, 9, 0, p(f[0]), p(f[1]), None), "channels must be 1..4"),
            (lambda: shade(p(i64), 0, p(f[0]), p(f[1]), 1, 0, 0, three, three, p(f[2]), p(f[3]), None), "n >= 1"),
            (lambda: shade(p(i64), 4, p(f[0]), None, 1, 0, 0, three, three, p(f[2]), p(f[3]), None), "null buffer"),
            (lambda: shade(p(i64), 4, p(f[0]), p(f[1]), 1, 0, 0, None, three, p(f[2]), p(f[3]), None), "null buffer"),
            (lambda: shade(p(i64), 4, p(f[0]), p(f[1]), 1, 0, 0, nan3, three, p(f[2]), p(f[3]), None), "finite"),
            (lambda: shade(p(i64), 4, p(f[0]), p(f[1]), 1, 2, 0, three, three, p(f[2]), p(f[3]), None), "channel must be"),
            (lambda: shade(p(i64), 4, p(f[0]), p(f[1]), 1, 0, 7, three, three, p(f[2]), p(f[3]), None), "side")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, rc, L.brief_last_error())
    assert not f.any() and not i32.any()                          # nothing was written
    # a block the clip box misses has an empty window: allowed in the route's table, refused where a window is walked
    empty = V.make_part(V.make_view(SMALL, (1, 0, 0), region="0:5,:,:"), (7, 0, 0), (9, SMALL[1], SMALL[2]))
    assert (empty.wrows, empty.wcols) == (0, 0)
    owner, _ = V.route_host(view, [pts[0], empty], np.full((view.rows, view.cols), 7.0, F), np.full((view.rows, view.cols), 8.0, F), True)
    assert (owner == 1).all()
    assert coords(v, C.byref(empty), p(f[0]), p(f[1]), 1, p(i64), 4, p(f[2]), None, None) == -1 and "window" in L.brief_last_error().decode()


# ---- refusals of render_surface_partition and of the artefact path, raised before any net file is read
def _cpu_parts(kinds=("s22", "s22")):
    """two slabs of SMALL along z with nets that live on the CPU: reaching a decode would fail differently (there is no CPU fallback)"""
    boxes = [((0, 0, 0), (6, 11, 9)), ((7, 0, 0), (15, 11, 9))]
    return [(_variants.BY_ID[k].make(), list(s), [b - a + 1 for a, b in zip(s, e)], -1.0, 1.0, (-0.5, 0.5), (0.0, 60000.0))
            for k, (s, e) in zip(kinds, boxes)]


def test_render_surface_partition_refuses_by_name_before_any_decode():
    view = V.make_view(SMALL, (1, 0, 0))
    parts = _cpu_parts()
    go = lambda parts=parts, level=300, kind="u16", **kw: V.render_surface_partition(parts, view, level, kind, **kw)
    for gap in ("nearest", "interpolate", None):
        with pytest.raises(ValueError, match="gap .* is not a gap rule.*empty"):
            go(gap=gap)
    with pytest.raises(ValueError, match="u8.*u16"):
        go(kind="f32")
    with pytest.raises(ValueError, match="at least one block"):
        go(parts=[])
    with pytest.raises(ValueError, match="level 65536 lies outside.*0 \\.\\. 65535"):
        go(level=65536)
    with pytest.raises(ValueError, match="level 256 lies outside.*0 \\.\\. 255"):
        go(level=256, kind="u8")
    with pytest.raises(ValueError, match="integer grey level"):
        go(level=10.5)
    with pytest.raises(ValueError, match="channel 1 does not exist.*0 \\.\\. 0"):
        go(channel=1)
    with pytest.raises(ValueError, match="side 'inside' is not one of above \\| below"):
        go(side="inside")
    for refine in (-1, 17):
        with pytest.raises(ValueError, match="refine must be 0 \\.\\. 16"):
            go(refine=refine)
    with pytest.raises(ValueError, match="voxel_size must be positive"):
        go(voxel_size=(1, 0, 1))
    mixed = _cpu_parts(("s22", "pyr"))
    with pytest.raises(ValueError, match="block at \\[7, 0, 0\\] has none.*SIREN_Pyramid.*shading=False"):
        go(parts=mixed)
    with pytest.raises(ValueError, match="overlap"):
        go(parts=parts + [parts[1]], shading=False)
    with pytest.raises(ValueError, match="chunk must be >= 1"):
        go(chunk=-1)


def _surf(opt, args, level=30000, **kw):
    return decompress_divide_surface(opt, *args, (1, 0, 0), level, **kw)


@pytest.mark.parametrize("case,words", [
    ("gap", "gap 'nearest' is not a gap rule.*empty"),
    ("error_bound", "error-bounded.*error_bound 3"),
    ("overlap", "d_0_3-h_0_7-w_0_7 and d_3_7-h_0_7-w_0_7 overlap"),
    ("axis1", "at least 2 voxels"),
    ("2d", "3-D data only"),
    ("dtype", "one dtype for all blocks"),
    ("level", "level 65536 lies outside.*0 \\.\\. 65535"),
    ("level8", "level 256 lies outside.*0 \\.\\. 255"),
    ("channel", "channel 1 does not exist"),
    ("side", "side 'inside' is not one of"),
    ("refine", "refine must be 0 \\.\\. 16"),
    ("shading", "block d_4_7-h_0_7-w_0_7 has none.*NeRF.*shading=False"),
    ("shading_bf16", "block d_0_3-h_0_7-w_0_7 has none.*bf16.*shading=False"),
    ("light", "light must not be the zero vector"),
])
def test_artefact_refusals_are_raised_before_any_net_is_opened(tmp_path, case, words):
    blocks, shape, opt, kw = dict(TWO), [8, 8, 8, 1], _opt(), {}
    if case == "gap":
        kw = dict(gap="nearest")
    elif case == "error_bound":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], error_bound=3)
    elif case == "overlap":
        blocks = {"d_0_3-h_0_7-w_0_7": _side([4, 8, 8, 1]), "d_3_7-h_0_7-w_0_7": _side([5, 8, 8, 1])}
    elif case == "axis1":
        blocks = {"d_0_6-h_0_7-w_0_7": _side([7, 8, 8, 1]), "d_7_7-h_0_7-w_0_7": _side([1, 8, 8, 1])}
    elif case == "2d":
        blocks, shape = {"h_0_3-w_0_7": _side([4, 8, 1]), "h_4_7-w_0_7": _side([4, 8, 1])}, [8, 8, 1]
    elif case == "dtype":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], dtype="uint8")
    elif case == "level":
        kw = dict(level=65536)
    elif case == "level8":
        blocks = {n: dict(s, dtype="uint8", max=250.0) for n, s in blocks.items()}
        opt.CompressFramework.Decompress.postprocess.clip = [0, 255]
        kw = dict(level=256)
    elif case == "channel":
        kw = dict(channel=1)
    elif case == "side":
        kw = dict(side="inside")
    elif case == "refine":
        kw = dict(refine=17)
    elif case == "shading":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], phi_name="NeRF")
    elif case == "shading_bf16":
        blocks["d_0_3-h_0_7-w_0_7"] = _side([4, 8, 8, 1], phi_precision="bf16")
    elif case == "light":
        kw = dict(light=(0, 0, 0))
    args = _tree(tmp_path, blocks, shape)
    with pytest.raises(ValueError, match=words):
        _surf(opt, args, **kw)
    assert callable(NFGR.decompress_divide_surface)
    assert all(not os.listdir(os.path.join(args[1], n)) for n in os.listdir(args[1]))


def test_with_everything_in_order_the_next_thing_is_to_read_a_net(tmp_path):
    blocks = dict(TWO)
    blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], phi_name="NeRF")
    args = _tree(tmp_path, blocks, [8, 8, 8, 1])
    with pytest.raises((OSError, FileNotFoundError)):
        _surf(_opt(), args, shading=False)


def test_the_divide_refusal_names_the_new_option_and_keeps_its_words():
    for w in ("DivideTask", "--view-owner nearest", "decompress_divide_view", "follow-up", "--view-surface-gap empty", "decompress_divide_surface"):
        assert w in V.DIVIDE_REFUSAL, w
    assert "surface view of a partition is a follow-up" not in V.DIVIDE_REFUSAL


def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SURFACE = ["--view", "1,0,0", "--view-surface", "100"]


@pytest.mark.parametrize("divide,extra,words", [
    # the pinned three-option refusal keeps its words and now names the option that lifts it
    (True, SURFACE + ["--view-owner", "nearest"], ["--view-surface with --view-owner", "per-point routing", "--view-surface-gap empty"]),
    (True, ["--view", "1,0,0", "--view-owner", "nearest", "--view-surface-gap", "empty"], ["--view-surface-gap", "--view-surface LEVEL"]),
    (True, ["--view-surface-gap", "empty"], ["--view-surface-gap", "--view dz,dy,dx"]),
    (False, SURFACE + ["--view-surface-gap", "empty"], ["--view-surface-gap empty", "SingleTask"]),
    (True, SURFACE + ["--view-owner", "nearest", "--view-surface-gap", "filled"], ["--view-surface-gap filled", "unknown rule", "empty"]),
    (True, SURFACE + ["--view-surface-gap", "empty"], ["--view", "DivideTask", "--view-owner nearest"]),      # the gap rule without the owner rule
    (True, ["--view", "1,0,0", "--view-composite", "0:0,0,0,0;255:255,255,255,1", "--view-owner", "nearest", "--view-surface-gap", "empty"],
     ["--view-composite with --view-surface-gap"]),
])
def test_cli_refusals_of_the_gap_option_write_nothing(tmp_path, divide, extra, words):
    os.makedirs(str(tmp_path / "art" / ("sideinfos" if divide else "module")))
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:",
            "-o", str(tmp_path / "out" / "surface.png")] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))
    assert "--view-surface-gap" in _cli().main.__globals__["__doc__"]
