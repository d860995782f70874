"""Host side of the view decode of a partition (view.render_partition / decompress_divide_view, decompress.py --view-owner): the
ownership rule of csrc/brief_view.h against the single-net geometry and against exact arithmetic, the ray windows, the refusals.
Nothing here needs a GPU: brief_view_part_clip_host and brief_view_part_sample_host run the header the kernels run, on the host CPU."""
import ctypes as C
import importlib.util
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from brief_pytorch_amd import _lib, config
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR, decompress_divide_view
from brief_pytorch_amd.io import save_yaml
from oracle import oracle as O
from tests.test_view_host import fl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (23, 31, 37)
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))      # tests/test_gpu_view.py's
SKIM = dict(direction=(1.0, 1e-5, -3e-6), spacing=1.0, depth_spacing=0.25)                               # a hair off the z axis


def _boxes(z, y, x):
    return [((a[0], b[0], c[0]), (a[1], b[1], c[1])) for a in z for b in y for c in x]


# (first voxel, last voxel) per block.  EIGHT: 2 x 2 x 2 unequal blocks, split after the planes 11, 13 and 20.  MIX: seven blocks on three
# levels with T-junctions: the lower half of z whole; the quarter above it at y <= 13 split once (along x); the other quarter split
# twice (along z and x)
Z, Y, X = [(0, 11), (12, 22)], [(0, 13), (14, 30)], [(0, 20), (21, 36)]
EIGHT = _boxes(Z, Y, X)
MIX = [((0, 0, 0), (11, 30, 36))] + _boxes([(12, 22)], [(0, 13)], X) + _boxes([(12, 17), (18, 22)], [(14, 30)], X)
PARTITIONS = {"eight": EIGHT, "mix": MIX}
VIEWS = {"oblique": OBLIQUE, "skim": SKIM}
for _s in (1.0, 0.5):                                        # at spacing 0.5 the samples of an axis-aligned view land exactly on s - 0.5
    for _n, _d in (("z", (1, 0, 0)), ("-y", (0, -1, 0)), ("x", (0, 0, 1))):
        VIEWS["%s@%g" % (_n, _s)] = dict(direction=_d, spacing=_s, depth_spacing=_s)

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")


def test_the_partitions_tile_the_grid():
    for name, boxes in PARTITIONS.items():
        count = np.zeros(DIMS, np.int32)
        for s, e in boxes:
            count[tuple(slice(a, b + 1) for a, b in zip(s, e))] += 1
        assert (count == 1).all(), name
    assert len(EIGHT) == 8 and len(MIX) == 7 and len({tuple(np.subtract(e, s)) for s, e in MIX}) >= 3


def _parts(view, boxes, window=None):
    return [V.make_part(view, s, [b - a + 1 for a, b in zip(s, e)], window) for s, e in boxes]


def _on_image(view, part, k0, cnt):
    """a window's arrays on the whole image (empty outside the window)"""
    K0, CNT = np.zeros((view.rows, view.cols), np.int32), np.zeros((view.rows, view.cols), np.int32)
    sl = (slice(part.row0, part.row0 + part.wrows), slice(part.col0, part.col0 + part.wcols))
    K0[sl], CNT[sl] = k0, cnt
    return K0, CNT


def _lattice(view):
    return np.meshgrid(np.arange(view.rows), np.arange(view.cols), np.arange(view.depth), indexing="ij")


@needs_lib
@pytest.mark.parametrize("vname", list(VIEWS))
@pytest.mark.parametrize("pname", list(PARTITIONS))
def test_every_sample_inside_the_clip_box_has_one_owner(pname, vname):
    """per ray the blocks' intervals are disjoint and their union is the ray's own interval (brief_view_clip_host); the windows are
    conservative: the range computed over the WHOLE image is empty on every ray outside the host's window and equal inside it"""
    boxes = PARTITIONS[pname]
    for region in (None, "3:19,5:26,2:30"):
        view = V.make_view(DIMS, region=region, **VIEWS[vname])
        K0, CNT = V.clip_host(view)
        assert (CNT > 0).any()
        total = np.zeros_like(CNT)
        lo = np.full(CNT.shape, np.iinfo(np.int32).max, np.int64)      # the union's ends, and the sum of the lengths: disjoint and gapless
        hi = np.zeros(CNT.shape, np.int64)
        clipped = 0
        for part, full in zip(_parts(view, boxes), _parts(view, boxes, "image")):
            k0, cnt = _on_image(view, part, *V.part_clip_host(view, part))
            k0f, cntf = V.part_clip_host(view, full)
            assert np.array_equal(cnt, cntf) and np.array_equal(k0, k0f), (pname, vname, list(part.start))
            assert (k0[cnt == 0] == 0).all()
            clipped += part.wrows * part.wcols
            total += cnt
            live = cnt > 0
            lo[live] = np.minimum(lo[live], k0[live])
            hi[live] = np.maximum(hi[live], (k0 + cnt)[live])
        assert np.array_equal(total, CNT), (pname, vname, region)
        live = CNT > 0
        assert np.array_equal(lo[live], K0[live]) and np.array_equal(hi[live], (K0 + CNT)[live])
        assert clipped < len(boxes) * view.rows * view.cols or len(boxes) == 1
        if pname == "eight":
            assert clipped < 8 * view.rows * view.cols


@needs_lib
@pytest.mark.parametrize("vname", ["oblique", "skim", "z@0.5", "-y@0.5", "x@0.5"])
def test_ranges_hold_exactly_the_owned_samples_and_a_face_belongs_to_the_upper_block(vname):
    """the interval of every ray and block against the flags of every sample of the lattice; each sample inside the clip box is owned by
    exactly one block; a sample exactly at s - 0.5 is the upper block's"""
    view = V.make_view(DIMS, region="3:19,5:26,2:30" if vname == "oblique" else None, **VIEWS[vname])
    row, col, k = _lattice(view)
    shape = (view.rows, view.cols, view.depth)
    kk = np.arange(view.depth)[None, None, :]
    owners = np.zeros(shape, np.int32)
    on_face = 0
    for (s, e), part in zip(EIGHT, _parts(view, EIGHT)):
        pos, local, _, inside, owned = V.part_sample_host(view, part, row, col, k)
        k0, cnt = _on_image(view, part, *V.part_clip_host(view, part))
        want = (inside & owned).reshape(shape)
        assert np.array_equal(want, (kk >= k0[..., None]) & (kk < (k0 + cnt)[..., None])), (vname, s)
        owners += owned.reshape(shape)
        assert np.array_equal(local, pos - np.array(s, np.float32))
        for a in range(3):
            if s[a] > 0:                                     # the face below this block: exactly s - 0.5 is OURS, not the lower block's
                face = pos[:, a] == np.float32(s[a] - 0.5)
                on_face += int(face.sum())
                inner = np.ones(len(pos), bool)
                for b in range(3):
                    if b != a:
                        inner &= (pos[:, b] >= s[b] - 0.5) & (pos[:, b] < e[b] + 0.5)
                assert owned[face & inner].all() and (local[face & inner, a] == -0.5).all()
            top = pos[:, a] == np.float32(e[a] + 0.5)        # ... and exactly e + 0.5 is not
            assert not owned[top].any()
    inside = V.sample_host(view, row, col, k)[2].reshape(shape)
    assert (owners[inside] == 1).all() and (owners <= 1).all()
    if vname.endswith("@0.5"):
        assert on_face > 0, "no sample lands on a face: the tie is not exercised"


def _exact(view, part, row, col, k):
    """(pos, local, coord, inside, owned) of one sample, every fp32 operation of csrc/brief_view.h rounded once (exact rationals)"""
    f = lambda x: Fr(float(x))
    pos, local, coord, inside, owned = [], [], [], True, True
    for a in range(3):
        p = fl(fl(fl(f(view.origin[a]) + fl(row * f(view.drow[a]))) + fl(col * f(view.dcol[a]))) + fl(k * f(view.ddepth[a])))
        s, n = int(part.start[a]), int(part.dims[a])
        q = fl(p - s)
        step = fl(fl(f(view.hi) - f(view.lo)) / (n - 1))
        x = fl(step * q + f(view.lo)) if q < n // 2 else fl(-step * fl((n - 1) - q) + f(view.hi))
        inside = inside and f(view.box_lo[a]) <= p <= f(view.box_hi[a])
        owned = owned and s - Fr(1, 2) <= p < s + n - Fr(1, 2)
        pos.append(p)
        local.append(q)
        coord.append(x)
    return pos, local, coord, inside, owned


@needs_lib
@pytest.mark.parametrize("vname", ["oblique", "skim", "x@0.5"])
def test_sample_restatement_against_exact_arithmetic(vname):
    view = V.make_view(DIMS, region="3:19,5:26,2:30", **VIEWS[vname])
    view.lo, view.hi = (-1.0, 1.0) if vname != "skim" else (0.0, 1.0)
    rng = np.random.default_rng(9)
    seen, below = set(), 0
    for part in _parts(view, MIX)[1::2]:
        n = 120
        row, col, k = rng.integers(0, view.rows, n), rng.integers(0, view.cols, n), rng.integers(0, view.depth, n)
        pos, local, coord, inside, owned = V.part_sample_host(view, part, row, col, k)
        for i in range(n):
            p, q, x, ins, own = _exact(view, part, int(row[i]), int(col[i]), int(k[i]))
            assert [Fr(float(t)) for t in pos[i]] == p and [Fr(float(t)) for t in local[i]] == q, i
            assert [Fr(float(t)) for t in coord[i]] == x, (i, coord[i], [float(t) for t in x])
            assert bool(inside[i]) == ins and bool(owned[i]) == own, i
            seen.add((ins, own))
            below += own and min(q) < 0
    assert len(seen) >= (2 if "@" in vname else 3) and below > 0      # (an axis-aligned view of the clip box has no sample outside it)


@needs_lib
@pytest.mark.parametrize("lohi", [(-1.0, 1.0), (0.0, 1.0)])
def test_integer_positions_get_the_block_grids_own_coordinates(lohi):
    """an axis-aligned view of unit spacing: every sample sits on a voxel, and its owner's coordinate is that block's linspace
    coordinate bit for bit, on both sides of n / 2 of every block"""
    for direction in ((1, 0, 0), (0, -1, 0), (0, 0, 1)):
        view = V.make_view(DIMS, direction)
        view.lo, view.hi = lohi
        row, col, k = _lattice(view)
        done = 0
        for (s, e), part in zip(MIX, _parts(view, MIX)):
            n = [b - a + 1 for a, b in zip(s, e)]
            pos, local, coord, inside, owned = V.part_sample_host(view, part, row, col, k)
            assert inside.all() and owned.sum() == int(np.prod(n))
            q = local[owned].astype(np.int64)
            assert np.array_equal(q, local[owned]) and (q.min(0) == 0).all() and (q.max(0) == np.array(n) - 1).all()
            grid = O.grid_coords(n, *lohi).reshape(*n, 3)
            assert np.array_equal(coord[owned].view(np.int32), grid[q[:, 0], q[:, 1], q[:, 2]].view(np.int32)), (direction, s)
            done += int(owned.sum())
        assert done == int(np.prod(DIMS))


@needs_lib
def test_a_gap_owns_nothing():
    """with one block removed the per-ray sums fall short by exactly that block's samples; rays that met only that block meet nothing"""
    view = V.make_view(DIMS, **OBLIQUE)
    CNT = V.clip_host(view)[1]
    parts = _parts(view, EIGHT)
    cnts = [_on_image(view, p, *V.part_clip_host(view, p))[1] for p in parts]
    gone = 3                                                 # a block on this view's silhouette: some rays meet it alone
    rest = sum(c for i, c in enumerate(cnts) if i != gone)
    assert cnts[gone].sum() > 0 and np.array_equal(CNT - rest, cnts[gone])
    assert ((rest == 0) & (CNT > 0)).any(), "no ray meets the removed block alone"


@needs_lib
def test_library_refuses_a_bad_block():
    view = V.make_view(DIMS, (1, 0, 0))
    good = V.make_part(view, (12, 0, 0), (11, 31, 37))
    buf = np.zeros((2, view.rows * view.cols), np.int32)
    for name, value in (("wrows", 0), ("row0", view.rows), ("wcols", view.cols + 1), ("col0", -1)):
        part = _lib.ViewPart.from_buffer_copy(good)
        setattr(part, name, value)
        rc = _lib.lib().brief_view_part_clip_host(C.byref(view), C.byref(part), buf[0].ctypes.data_as(C.c_void_p), buf[1].ctypes.data_as(C.c_void_p))
        assert rc == -1 and "window" in _lib.lib().brief_last_error().decode(), (name, _lib.lib().brief_last_error())
    assert not buf.any()
    part = _lib.ViewPart.from_buffer_copy(good)
    part.dims[0] = 12
    with pytest.raises(_lib.BriefError, match="start \\+ dims"):
        V.part_clip_host(view, part)
    big = V.make_view((1 << 23, 4, 4), (0, 0, 1), size=(4, 4))
    with pytest.raises(ValueError, match="2\\^23"):
        V.make_part(big, (0, 0, 0), (4, 4, 4))
    part = _lib.ViewPart.from_buffer_copy(V.make_part(view, (0, 0, 0), (4, 4, 4)))
    with pytest.raises(_lib.BriefError, match="2\\^23"):
        V.part_clip_host(big, part)
    with pytest.raises(ValueError, match="inside the volume"):
        V.make_part(view, (12, 0, 0), (12, 31, 37))
    with pytest.raises(ValueError, match="at least 2 voxels"):
        V.make_part(view, (12, 0, 0), (1, 31, 37))


# ---- refusals of the artefact path, raised before any net is opened
def _opt():
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    opt.CompressFramework.Decompress.postprocess.denoise.close = False
    return opt


def _side(shape, **kw):
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": list(shape), "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


def _tree(tmp_path, blocks, data_shape):
    """the side-info tree of a DivideTask artefact without a single stored net: module/<name>/ is an empty directory"""
    root = tmp_path / "compressed"
    for name, side in blocks.items():
        os.makedirs(str(root / "module" / name))
        os.makedirs(str(root / "sideinfos" / name))
        save_yaml(side, str(root / "sideinfos" / name / "sideinfos.yaml"))
    return {"data_shape": list(data_shape)}, str(root / "module"), str(root / "sideinfos")


TWO = {"d_0_3-h_0_7-w_0_7": _side([4, 8, 8, 1]), "d_4_7-h_0_7-w_0_7": _side([4, 8, 8, 1])}


@pytest.mark.parametrize("case,words", [
    ("error_bound", "error-bounded.*error_bound 3"),
    ("overlap", "d_0_3-h_0_7-w_0_7 and d_3_7-h_0_7-w_0_7 overlap"),
    ("axis1", "at least 2 voxels"),
    ("2d", "3-D data only"),
    ("dtype", "one dtype for all blocks"),
    ("float", "uint8 / uint16 data only"),
    ("mean_postprocess", "mean view.*does not.*commute"),
    ("shape", "not its index range"),
])
def test_artefact_refusals_are_raised_before_any_net_is_opened(tmp_path, case, words):
    blocks, shape, opt, kw = dict(TWO), [8, 8, 8, 1], _opt(), {}
    if case == "error_bound":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], error_bound=3)
    elif case == "overlap":
        blocks = {"d_0_3-h_0_7-w_0_7": _side([4, 8, 8, 1]), "d_3_7-h_0_7-w_0_7": _side([5, 8, 8, 1])}
    elif case == "axis1":
        blocks = {"d_0_6-h_0_7-w_0_7": _side([7, 8, 8, 1]), "d_7_7-h_0_7-w_0_7": _side([1, 8, 8, 1])}
    elif case == "2d":
        blocks, shape = {"h_0_3-w_0_7": _side([4, 8, 1]), "h_4_7-w_0_7": _side([4, 8, 1])}, [8, 8, 1]
    elif case == "dtype":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], dtype="uint8")
    elif case == "float":
        blocks = {n: dict(s, dtype="float32") for n, s in blocks.items()}
    elif case == "mean_postprocess":
        opt.CompressFramework.Decompress.postprocess.denoise.level = 500
        kw = dict(mode="mean")
    elif case == "shape":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 7, 1])
    args = _tree(tmp_path, blocks, shape)
    with pytest.raises(ValueError, match=words):
        decompress_divide_view(opt, *args, (1, 0, 0), **kw)
    assert callable(NFGR.decompress_divide_view)                 # (the method needs a GPU to construct its NFGR: tests/test_gpu_view_partition_framework.py)
    assert all(not os.listdir(os.path.join(args[1], n)) for n in os.listdir(args[1]))


def test_the_single_artefact_entry_still_refuses_and_names_the_option():
    with pytest.raises(ValueError, match="DivideTask.*--view-owner nearest.*decompress_divide_view.*follow-up"):
        NFGR.decompress_view(_opt(), "nowhere", {"data_shape": [8, 8, 8, 1]}, (1, 0, 0))


def _cli():
    spec = importlib.util.spec_from_file_location("_decompress_cli", os.path.join(ROOT, "decompress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("divide,extra,words", [
    (True, ["--view", "1,0,0"], ["--view", "DivideTask", "--view-owner nearest", "follow-up"]),
    (True, ["--view", "1,0,0", "--view-owner", "farthest"], ["--view-owner farthest", "unknown rule", "nearest"]),
    (True, ["--view", "1,0,0", "--view-owner", "nearest", "--view-surface", "100"], ["--view-surface with --view-owner", "per-point routing"]),
    (False, ["--view", "1,0,0", "--view-owner", "nearest"], ["--view-owner nearest", "SingleTask"]),
    (True, ["--view-owner", "nearest"], ["--view-owner", "--view dz,dy,dx"]),
    (True, ["--mip", "--view-owner", "nearest"], ["--view-owner", "--view dz,dy,dx"]),
])
def test_cli_refusals_of_the_owner_option_write_nothing(tmp_path, divide, extra, words):
    os.makedirs(str(tmp_path / "art" / ("sideinfos" if divide else "module")))
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:",
            "-o", str(tmp_path / "out" / "view.tif")] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))
    assert "--view-owner" in _cli().main.__globals__["__doc__"]
