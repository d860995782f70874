"""View decode of a partition on the GPU (view.render_partition, csrc/brief_view.inc k_view_part_*): one randomly initialised net per
block, a distinct seed per block, blocks of different kernel families side by side.  Every comparison is bitwise: the folds are integer
folds, and a sample has one owner.
  1  a partition of ONE block covering the grid equals view.render of that net;
  2  partitions equal the restatement: every sample of the whole lattice through its OWNER's forward entry on
     brief_view_part_sample_host's coordinates, folded in numpy with the host's flags;
  3  axis-aligned views of unit spacing equal the per-block decodes (decode_mips folded into one image, decode_box pasted);
  4  chunking, the order of the blocks and repetition change nothing;  5  a gap owns nothing."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, mip
from brief_pytorch_amd import view as VW
from tests import _variants as V
from tests.test_gpu_view import _fold
from tests.test_view_partition_host import EIGHT, MIX

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (23, 31, 37)
BOX = "3:19,5:26,2:30"
AXIS_DIR = {0: (1, 0, 0), 1: (0, -1, 0), 2: (0, 0, 1)}
OBLIQUE = dict(direction=(0.48, -0.6, 0.64), spacing=1.7, depth_spacing=0.5, voxel_size=(2, 1, 1))
TORCH_DT = {"u16": torch.uint16, "u8": torch.uint8}
KINDS = {"c1": ("s22", "s256", "pyr"), "c4": ("mfnf",)}          # the net kinds of a partition's blocks, in turn
CASES = [("c1", "u16"), ("c1", "u8"), ("c4", "u8"), ("c4", "u16")]
CASE = pytest.mark.parametrize("family,kind", CASES, ids=["%s-%s" % c for c in CASES])
MODES = ("max", "min", "mean")

_cache = {}


def _partition(name, family, kind):
    """the blocks (phi, start, dims, lo, hi, scale, vrange) of a partition: block i is of kind KINDS[family][i % ..] with seed 1000 + i,
    its own integer window (the 0.15 / 0.85 quantiles of its f32 decode) and its own value range"""
    key = (name, family, kind)
    if key not in _cache:
        parts = []
        for i, (s, e) in enumerate({"eight": EIGHT, "mix": MIX, "one": [((0, 0, 0), tuple(n - 1 for n in DIMS))]}[name]):
            n = [b - a + 1 for a, b in zip(s, e)]
            v = V.BY_ID[KINDS[family][i % len(KINDS[family])]]
            assert v.cin == 3
            torch.manual_seed(1000 + i)
            m = v.cls(**v.kwargs).to(DEV)
            f32 = m.decode_grid(n).cpu().numpy()
            assert np.isfinite(f32).all()
            q15, q85 = (float(np.float32(q)) for q in np.quantile(f32.astype(np.float64), [0.15, 0.85]))
            assert q85 > q15
            lo, hi = V.VRANGE[kind]
            parts.append((m, list(s), n, -1.0, 1.0, (q15, q85), (lo + 2.0 * i, hi - 3.0 * i)))
        _cache[key] = parts
    return _cache[key]


def _render(parts, view, mode, kind, chunk=None):
    img, hits, stats = VW.render_partition(parts, view, mode, kind, chunk=chunk)
    ch = parts[0][0].data_channel
    assert img.is_cuda and hits.dtype == torch.int32 and tuple(hits.shape) == (view.rows, view.cols)
    assert tuple(img.shape) == (view.rows, view.cols, ch) and img.dtype == (torch.float32 if mode == "mean" else TORCH_DT[kind])
    assert stats["blocks"] == len(parts) and stats["rays"] == view.rows * view.cols
    return img.cpu().numpy(), hits.cpu().numpy(), stats


def _forward_int(m, coords, kind, scale, vrange):
    """the net's forward entry on explicit coordinates with the block's integer epilogue"""
    c = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).to(DEV)
    n = c.shape[0]
    out = torch.empty((n, m.data_channel), dtype=TORCH_DT[kind], device=DEV)
    if n:
        m.sync_packed()
        b = _lib.BatchDesc(c.data_ptr(), None, None, None, 0, n, 0, 0, 0)
        _lib.check(m._abi_forward(None, b, out, {"u8": _lib.OUT_U8, "u16": _lib.OUT_U16}[kind], scale, vrange, n))
    return out.cpu().numpy()


def _restate(parts, view, kind):
    """(vals [rows, cols, depth, C] int64, evaluated [rows, cols, depth], facts) over the whole lattice: a sample is evaluated by the block
    whose host flags say inside and owned, on the host's block-local coordinates"""
    row, col, k = np.meshgrid(np.arange(view.rows), np.arange(view.cols), np.arange(view.depth), indexing="ij")
    n, ch = row.size, parts[0][0].data_channel
    vals, owners = np.zeros((n, ch), np.int64), np.zeros(n, np.int32)
    crossed = np.zeros((view.rows, view.cols), np.int32)
    q_min, lanes = 0.0, set()
    for m, start, dims, lo, hi, scale, vrange in parts:
        v = VW._with_range(view, lo, hi)
        _, local, coord, inside, owned = VW.part_sample_host(v, VW.make_part(v, start, dims, "image"), row, col, k)
        sel = inside & owned
        vals[sel] = _forward_int(m, coord[sel], kind, scale, vrange)
        owners += sel
        per_ray = sel.reshape(view.rows, view.cols, view.depth).sum(2)
        crossed += per_ray > 0
        if sel.any():
            q_min = min(q_min, float(local[sel].min()))
            lanes.add(VW._lanes(sel.sum() / (per_ray > 0).sum()))
    assert owners.max() <= 1
    shape = (view.rows, view.cols, view.depth)
    return vals.reshape(*shape, ch), (owners == 1).reshape(shape), dict(crossed=int(crossed.max()), q_min=q_min, lanes=lanes)


# ---- 1: one block equals the single-net view
@CASE
def test_one_block_equals_the_single_net_view(family, kind):
    parts = _partition("one", family, kind)
    m, _, _, lo, hi, scale, vrange = parts[0]
    centre_off = 1.3
    for geom in (OBLIQUE, dict(direction=AXIS_DIR[1]), dict(OBLIQUE, region=BOX), dict(direction=AXIS_DIR[2], region=BOX)):
        for mode in MODES + ("slice",):
            view = VW.make_view(DIMS, **(dict(geom, depth=centre_off) if mode == "slice" else geom))
            want, want_hits, want_stats = VW.render(m, view, mode, lo, hi, kind, scale, vrange)
            img, hits, stats = _render(parts, view, mode, kind)
            assert np.array_equal(img.view(np.uint8), want.cpu().numpy().view(np.uint8)), (geom, mode)
            assert np.array_equal(hits, want_hits.cpu().numpy())
            assert {k: stats[k] for k in want_stats} == want_stats and stats["samples_evaluated"] > 0
            assert stats["blocks_hit"] == 1 and stats["rays_clipped"] <= stats["rays"]


# ---- 2: partitions equal the restatement
@pytest.mark.parametrize("name,family,kind", [("eight", "c1", "u16"), ("eight", "c1", "u8"), ("eight", "c4", "u8"), ("mix", "c1", "u16"),
                                               ("mix", "c4", "u16")])
def test_partitions_equal_the_restatement(name, family, kind):
    parts = _partition(name, family, kind)
    assert len({(type(p[0]), p[0].params.numel()) for p in parts}) == len(KINDS[family])      # the kinds sit side by side
    lanes = set()
    for geom in (OBLIQUE, dict(OBLIQUE, region=BOX, depth_spacing=0.1, spacing=2.9)):
        view = VW.make_view(DIMS, **geom)
        vals, evaluated, facts = _restate(parts, view, kind)
        for mode in MODES:
            want, want_hits = _fold(vals, evaluated, mode, V.NP_DTYPE[kind])
            img, hits, stats = _render(parts, view, mode, kind)
            assert np.array_equal(hits, want_hits), (geom, mode)
            assert np.array_equal(img, want), (geom, mode, int((img != want).sum()))
            assert stats["samples_inside"] == stats["samples_evaluated"] == int(evaluated.sum())
            assert stats["rays_hit"] == int((want_hits > 0).sum()) and stats["blocks_hit"] == len(parts)
            assert stats["rays_clipped"] < len(parts) * stats["rays"]
        # what keeps this from being vacuous: a ray through three blocks or more, a sample below its block's grid
        assert facts["crossed"] >= 3 and facts["q_min"] < 0, facts
        lanes |= facts["lanes"]
        assert len(np.unique(img)) >= 50 and evaluated.sum() >= 10000
        # every sample inside the clip box was evaluated: the partition tiles the grid
        row, col, k = np.meshgrid(np.arange(view.rows), np.arange(view.cols), np.arange(view.depth), indexing="ij")
        assert np.array_equal(VW.sample_host(view, row, col, k)[2].reshape(evaluated.shape), evaluated)
    # an oblique plane, off the centre: one lane per ray
    plane = VW.make_view(DIMS, depth=1.3, **OBLIQUE)
    assert plane.depth == 1
    vals, evaluated, facts = _restate(parts, plane, kind)
    want, want_hits = _fold(vals, evaluated, "slice", V.NP_DTYPE[kind])
    img, hits, stats = _render(parts, plane, "slice", kind)
    assert np.array_equal(img, want) and np.array_equal(hits, want_hits) and 0 < stats["rays_hit"] < stats["rays"]
    lanes |= facts["lanes"]
    assert 1 in lanes and 64 in lanes, lanes


# ---- 3: axis-aligned views of unit spacing equal the per-block decodes
def _block_decodes(parts, kind, start, stop):
    """(the pasted decode_box volume of all blocks, the three images of the per-block decode_mips over the box start:stop folded
    into one frame, the blocks that meet the box)"""
    ch = parts[0][0].data_channel
    vol = np.zeros(DIMS + (ch,), V.NP_DTYPE[kind])
    ext = [b - a for a, b in zip(start, stop)]
    dt = TORCH_DT[kind]
    images = (torch.zeros((ext[1], ext[2], ch), dtype=dt, device=DEV), torch.zeros((ext[0], ext[2], ch), dtype=dt, device=DEV),
              torch.zeros((ext[0], ext[1], ch), dtype=dt, device=DEV))
    met = 0
    for m, s, n, lo, hi, scale, vrange in parts:
        sl = tuple(slice(a, a + b) for a, b in zip(s, n))
        vol[sl] = m.decode_box(n, out_kind=kind, scale=scale, vrange=vrange).cpu().numpy()
        b_lo = [max(a, c) for a, c in zip(start, s)]
        b_hi = [min(a, c + d) for a, c, d in zip(stop, s, n)]
        if all(h > l for l, h in zip(b_lo, b_hi)):
            met += 1
            mip.decode_mips(m, n, [l - c for l, c in zip(b_lo, s)], [h - c for h, c in zip(b_hi, s)], [1, 1, 1], lo, hi, kind, scale, vrange,
                            into=images, origin=[l - a for l, a in zip(b_lo, start)])
    return vol, [t.cpu().numpy() for t in images], met


@pytest.mark.parametrize("name,family,kind", [("eight", "c1", "u16"), ("mix", "c1", "u8"), ("eight", "c4", "u16")])
def test_axis_aligned_views_equal_the_per_block_decodes(name, family, kind):
    parts = _partition(name, family, kind)
    centre = [(n - 1) // 2 for n in DIMS]
    # the whole grid; a clip box that cuts through blocks; one that misses the upper half of z entirely
    for region, sl in ((None, (slice(0, 23), slice(0, 31), slice(0, 37))), (BOX, (slice(3, 19), slice(5, 26), slice(2, 30))),
                       ("1:12,2:31,0:37", (slice(1, 12), slice(2, 31), slice(0, 37)))):
        start, stop = [s.start for s in sl], [s.stop for s in sl]
        vol, mips, met = _block_decodes(parts, kind, start, stop)
        assert met == len(parts) or region == "1:12,2:31,0:37"
        sub = vol[sl]
        for a in range(3):
            view = VW.make_view(DIMS, AXIS_DIR[a], region=region)
            img, hits, stats = _render(parts, view, "max", kind)
            assert np.array_equal(img, mips[a]) and np.array_equal(img, sub.max(a)), (region, a)
            assert (hits == sub.shape[a]).all() and stats["samples_evaluated"] == stats["samples_inside"] == sub.size // sub.shape[-1]
            assert stats["blocks_hit"] == met                    # a block the clip box misses launches nothing: its window is empty
            empty = sum(1 for _, s, n, *_ in parts if VW.part_window(view, s, n) == (0, 0, 0, 0))
            assert empty == len(parts) - met and stats["rays_clipped"] < len(parts) * stats["rays"]
            for plane in {start[a], 11, 12, 13, 14, 20, 21, DIMS[a] // 2, stop[a] - 1}:      # the faces' both sides, and n / 2 of the blocks
                if not start[a] <= plane < stop[a]:
                    continue
                off = (plane - centre[a]) * (-1 if a == 1 else 1)
                view = VW.make_view(DIMS, AXIS_DIR[a], region=region, depth=float(off))
                assert view.depth == 1
                img, hits, stats = _render(parts, view, "slice", kind)
                assert np.array_equal(img, vol.take(plane, axis=a)[tuple(s for i, s in enumerate(sl) if i != a)]), (region, a, plane)
                assert (hits == 1).all() and stats["samples_evaluated"] == hits.size


# ---- 4: chunking, block order and repetition change no bit
def test_chunking_block_order_and_repetition_change_nothing():
    parts = _partition("eight", "c1", "u16")
    for geom, chunks in ((OBLIQUE, (1000, None)), (dict(OBLIQUE, depth=(-1.0, 1.0), size=(12, 14)), (1, 1000, None))):
        view = VW.make_view(DIMS, **geom)
        for mode in MODES:
            img, hits, stats = _render(parts, view, mode, "u16")
            assert stats["samples_evaluated"] > (1000 if geom is OBLIQUE else 100)
            for chunk in chunks:
                for order in (parts, parts[::-1]):
                    img2, hits2, stats2 = _render(order, view, mode, "u16", chunk=chunk)
                    assert np.array_equal(img2.view(np.uint8), img.view(np.uint8)) and np.array_equal(hits2, hits) and stats2 == stats, (mode, chunk)


# ---- 5: a gap owns nothing
def test_a_gap_is_neither_evaluated_nor_folded():
    whole = _partition("eight", "c1", "u16")
    parts = whole[:3] + whole[4:]                                # (block 3 is on this view's silhouette: some rays meet it alone)
    view = VW.make_view(DIMS, **OBLIQUE)
    vals, evaluated, _ = _restate(parts, view, "u16")
    full = _restate(whole, view, "u16")[1]
    assert evaluated.sum() < full.sum()
    dark = 0
    for mode in MODES:
        want, want_hits = _fold(vals, evaluated, mode, np.uint16)
        img, hits, stats = _render(parts, view, mode, "u16")
        assert np.array_equal(img, want) and np.array_equal(hits, want_hits), mode
        lost = (hits == 0) & (full.sum(2) > 0)                   # rays that met the removed block alone
        dark = int(lost.sum())
        assert not img[hits == 0].any() and stats["samples_evaluated"] == int(evaluated.sum()) and stats["blocks_hit"] == 7
    assert dark > 0


def test_entries_and_render_partition_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    L = _lib.lib()
    parts = _partition("eight", "c1", "u16")
    view = VW.make_view(DIMS, (1, 0, 0))
    part = VW.make_part(view, parts[7][1], parts[7][2])
    n = part.wrows * part.wcols
    k0 = torch.zeros(n, dtype=torch.int32, device=DEV)
    off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    v, pt, coords, fold = C.byref(view), C.byref(part), L.brief_view_part_coords, L.brief_view_part_fold
    for call, what in ((lambda: L.brief_view_part_clip(v, pt, None, p(k0), st), "null"),
                       (lambda: L.brief_view_part_clip(v, None, p(k0), p(k0), st), "null block"),
                       (lambda: coords(v, pt, p(k0), p(off), 0, 0, 0, 1, 1, p(buf), st), "sample range"),
                       (lambda: coords(v, pt, p(k0), p(off), 0, 4, 0, n + 1, 1, p(buf), st), "ray range"),
                       (lambda: coords(v, pt, p(k0), p(off), 0, 4, 0, 1, 3, p(buf), st), "power of two"),
                       (lambda: fold(v, pt, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_F32, 1, 0, p(k0), p(buf), st), "elem_kind"),
                       (lambda: fold(v, pt, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 5, 0, p(k0), p(buf), st), "channels"),
                       (lambda: fold(v, pt, p(k0), p(off), 0, 4, 0, 1, 1, p(buf), _lib.OUT_U8, 1, 4, p(k0), p(buf), st), "mode")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and not k0.cpu().numpy().any()
    with pytest.raises(ValueError, match="depth 1"):
        VW.render_partition(parts, view, "slice", "u16")
    with pytest.raises(ValueError, match="u8.*u16"):
        VW.render_partition(parts, view, "max", "f32")
    with pytest.raises(ValueError, match="overlap"):
        VW.render_partition(parts + [parts[3]], view, "max", "u16")
    with pytest.raises(ValueError, match="channel count"):
        VW.render_partition(parts[:7] + [_partition("eight", "c4", "u16")[7]], view, "max", "u16")
