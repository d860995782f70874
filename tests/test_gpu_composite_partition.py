"""Composite view of a partition on the GPU (composite.render_composite_partition, csrc/brief_composite.inc k_composite_part_*): one
randomly initialised net per block, blocks of different kernel families side by side (tests/test_gpu_view_partition.py's partitions).
Every comparison is bitwise: the fold is an integer fold, and the carry follows k0.
  1  a partition of ONE block equals composite.render_composite of that net, and nothing is evaluated twice;
  2  partitions equal the restatement: every sample through its OWNER's forward entry, folded per ray in Python integers in ascending
     k, and through brief_view_composite_host on the merged list;
  3  along +z at unit spacing the image is the integer composite of the pasted per-block decode_box volume;
  4  chunking, the order of the blocks and repetition change nothing;  5  a gap contributes nothing;  6  refusals.
The vacuity guards (a second pass that is neither empty nor everything, saturated and half-transparent pixels, one lane and 64 lanes
per ray) are asserted on the device's own results where the cases run."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import view as VW
from tests import _variants as V
from tests._composite import TAU_SAT, finish, fold_ray
from tests.test_gpu_view_partition import BOX, DIMS, OBLIQUE, _block_decodes, _partition, _restate

pytestmark = pytest.mark.gpu
DEV = "cuda"
BG = (12, 200, 255)
BITS = {"u8": 8, "u16": 12}


def _table(parts, view, kind, channel=0, seed=3):
    """a table made for the values this partition shows along this view: transparent below their middle (the median over the hit pixels
    of the mean view's image), faint above it (a ray stays half-transparent over tens of samples) with every eighth row there dense (a
    long ray saturates), so that segments behind clear, hazy and opaque ones all occur.  The emissions are make_transfer's form,
    e_c = rint(256 * colour_c * (1 - 2^(-tau / 65536))) of a random colour per row; the host tests cover emissions that fit nothing."""
    mean, hits, _ = VW.render_partition(parts, view, "mean", kind)
    mid = int(np.median(mean.cpu().numpy()[..., channel][hits.cpu().numpy() > 0])) >> ((8 if kind == "u8" else 16) - BITS[kind])
    rng = np.random.default_rng(seed)
    n = 1 << BITS[kind]
    assert 0 < mid < n - 8
    tf = np.zeros((n, 4), np.int32)
    tf[mid:, 0] = rng.integers(200, 9000, n - mid)
    tf[mid::8, 0] = rng.integers(TAU_SAT // 40, TAU_SAT // 6, len(tf[mid::8]))
    alpha = 1.0 - np.exp2(-tf[:, 0] / 65536.0)
    tf[:, 1:] = np.rint(256.0 * rng.integers(0, 256, (n, 3)) * alpha[:, None])
    return CP.check_transfer(tf, kind)[0]


def _render(parts, view, tf, kind, channel=0, chunk=None):
    img, hits, stats = CP.render_composite_partition(parts, view, tf, kind, channel=channel, background=BG, chunk=chunk)
    assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (view.rows, view.cols, 4)
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (view.rows, view.cols)
    assert stats["blocks"] == len(parts) and stats["rays"] == view.rows * view.cols
    assert stats["samples_evaluated"] == stats["samples_inside"] + stats["samples_second_pass"] and stats["segments"] >= stats["rays_hit"]
    return img.cpu().numpy(), hits.cpu().numpy(), stats


def _python(vals, evaluated, tf, kind, channel):
    """(image, hits, tau_run) from the restated samples: per ray the evaluated ones in ascending k, in Python integers"""
    shift = (8 if kind == "u8" else 16) - (len(tf).bit_length() - 1)
    rows, cols = evaluated.shape[:2]
    img, hits, runs = np.zeros((rows, cols, 4), np.uint8), evaluated.sum(2).astype(np.int32), np.zeros((rows, cols), np.int64)
    for r in range(rows):
        for c in range(cols):
            run, acc = fold_ray([tf[int(v) >> shift] for v in vals[r, c, evaluated[r, c], channel]])
            img[r, c], runs[r, c] = finish(run, acc, BG), run
    return img, hits, runs


# ---- 1: one block equals the single-net composite
@pytest.mark.parametrize("family,kind,channel", [("c1", "u16", 0), ("c1", "u8", 0), ("c4", "u8", 3)])
def test_one_block_equals_the_single_net_composite(family, kind, channel):
    parts = _partition("one", family, kind)
    m, _, _, lo, hi, scale, vrange = parts[0]
    for geom in (OBLIQUE, dict(OBLIQUE, region=BOX), dict(direction=(0, -1, 0))):
        view = VW.make_view(DIMS, **geom)
        tf = _table(parts, view, kind, channel)
        want, want_hits, want_stats = CP.render_composite(m, view, tf, lo, hi, kind, scale, vrange, channel=channel, background=BG)
        img, hits, stats = _render(parts, view, tf, kind, channel)
        assert np.array_equal(img, want.cpu().numpy()) and np.array_equal(hits, want_hits.cpu().numpy()), geom
        assert {k: stats[k] for k in want_stats} == want_stats and stats["samples_evaluated"] > 0
        assert stats["samples_second_pass"] == 0 and stats["blocks_hit"] == 1 and stats["segments"] == stats["rays_hit"]
        assert len(np.unique(img[..., :3])) >= 20


# ---- 2: partitions equal the restatement
@pytest.mark.parametrize("name,family,kind,channel", [("eight", "c1", "u16", 0), ("eight", "c1", "u8", 0), ("eight", "c4", "u8", 2),
                                                       ("mix", "c1", "u16", 0), ("mix", "c4", "u16", 1)])
def test_partitions_equal_the_restatement(name, family, kind, channel):
    parts = _partition(name, family, kind)
    tf = _table(parts, VW.make_view(DIMS, **OBLIQUE), kind, channel)
    lanes, runs = set(), []
    for geom in (OBLIQUE, dict(OBLIQUE, region=BOX, depth_spacing=0.1, spacing=2.9)):      # (the second: a clip box that cuts through blocks)
        view = VW.make_view(DIMS, **geom)
        vals, evaluated, facts = _restate(parts, view, kind)
        lanes |= facts["lanes"]
        want, want_hits, want_run = _python(vals, evaluated, tf, kind, channel)
        runs.append(want_run)
        img, hits, stats = _render(parts, view, tf, kind, channel)
        assert np.array_equal(hits, want_hits), geom
        assert np.array_equal(img, want), (geom, int((img != want).sum()))
        # the merged list through the single-list host: the partition tiles the grid, so a ray's segments are its own interval
        K0, CNT = VW.clip_host(view)
        assert np.array_equal(CNT, want_hits)
        off = np.concatenate([[0], np.cumsum(CNT.ravel(), dtype=np.int64)])
        r = np.repeat(np.arange(view.rows * view.cols), CNT.ravel())
        k = np.repeat(K0.ravel(), CNT.ravel()) + (np.arange(int(off[-1])) - np.repeat(off[:-1], CNT.ravel()))
        merged = np.ascontiguousarray(vals[r // view.cols, r % view.cols, k]).astype(V.NP_DTYPE[kind])
        host = CP.composite_host(view, K0.ravel(), off, merged, tf, channel=channel, background=BG)
        assert np.array_equal(img, host[0]) and np.array_equal(hits, host[1]) and np.array_equal(host[2], want_run)
        # what keeps this from being vacuous
        assert stats["samples_inside"] == int(evaluated.sum()) >= 5000 and stats["rays_hit"] == int((want_hits > 0).sum())
        assert 0 < stats["samples_second_pass"] < stats["samples_inside"], stats
        assert stats["segments"] > stats["rays_hit"] and facts["crossed"] >= 3 and stats["blocks_hit"] == len(parts)
        assert (img[want_hits == 0] == np.array(BG + (0,), np.uint8)).all() and (want_hits == 0).any()
        assert len(np.unique(img[..., :3])) >= 20 and len(np.unique(img[..., 3])) >= 5
    # an oblique plane, off the centre: one lane per ray, one sample per pixel, nothing to carry
    plane = VW.make_view(DIMS, depth=1.3, **OBLIQUE)
    vals, evaluated, facts = _restate(parts, plane, kind)
    lanes |= facts["lanes"]
    want, want_hits, _ = _python(vals, evaluated, tf, kind, channel)
    img, hits, stats = _render(parts, plane, tf, kind, channel)
    assert np.array_equal(img, want) and np.array_equal(hits, want_hits) and stats["samples_second_pass"] == 0 and 0 < stats["rays_hit"] < stats["rays"]
    runs = np.concatenate([x.ravel() for x in runs])
    assert (runs == TAU_SAT).any() and ((runs > 0) & (runs < TAU_SAT)).any(), "no saturated pixel, or no half-transparent one"
    assert 1 in lanes and 64 in lanes, lanes


# ---- 3: the grid's own voxels
@pytest.mark.parametrize("name,family,kind,channel", [("eight", "c1", "u16", 0), ("mix", "c4", "u8", 2)])
def test_along_z_at_unit_spacing_it_is_the_composite_of_the_pasted_block_decodes(name, family, kind, channel):
    parts = _partition(name, family, kind)
    vol = _block_decodes(parts, kind, [0, 0, 0], list(DIMS))[0]
    shift = (8 if kind == "u8" else 16) - BITS[kind]
    view = VW.make_view(DIMS, (1, 0, 0))
    assert (view.rows, view.cols, view.depth) == (DIMS[1], DIMS[2], DIMS[0])
    tf = _table(parts, view, kind, channel, seed=8)
    img, hits, stats = _render(parts, view, tf, kind, channel)
    want = np.empty(img.shape, np.uint8)
    for y in range(DIMS[1]):
        for x in range(DIMS[2]):
            want[y, x] = finish(*fold_ray([tf[int(v) >> shift] for v in vol[:, y, x, channel]]), BG)
    assert np.array_equal(img, want) and (hits == DIMS[0]).all() and stats["samples_inside"] == int(np.prod(DIMS))
    assert len(np.unique(img.reshape(-1, 4), axis=0)) >= 20 and stats["samples_second_pass"] > 0
    # looking the other way composites the same voxels back to front: another image.  Along -z with the rows along +y the columns run
    # along -x (view.frame: col_dir = direction x row_dir), so pixel (y, c) is the ray through x = DIMS[2] - 1 - c, from z = DIMS[0] - 1 down
    reverse = VW.make_view(DIMS, (-1, 0, 0), up=(0, 1, 0))
    assert (list(reverse.origin), list(reverse.drow), list(reverse.dcol), list(reverse.ddepth)) == \
        ([DIMS[0] - 1.0, 0.0, DIMS[2] - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0])
    back, back_hits, _ = _render(parts, reverse, tf, kind, channel)
    for y in range(DIMS[1]):
        for x in range(DIMS[2]):
            want[y, x] = finish(*fold_ray([tf[int(v) >> shift] for v in vol[::-1, y, x, channel]]), BG)
    assert np.array_equal(back, want[:, ::-1]) and (back_hits == DIMS[0]).all() and not np.array_equal(back, img)


# ---- 4: chunking, block order and repetition change no bit
def test_chunking_block_order_and_repetition_change_nothing():
    parts = _partition("eight", "c1", "u16")
    tf = _table(parts, VW.make_view(DIMS, **OBLIQUE), "u16")
    for geom, chunks in ((OBLIQUE, (1000, None)), (dict(OBLIQUE, depth=(-1.0, 1.0), size=(12, 14)), (1, 1000, None))):
        view = VW.make_view(DIMS, **geom)
        img, hits, stats = _render(parts, view, tf, "u16")
        assert stats["samples_inside"] > (1000 if geom is OBLIQUE else 100) and (stats["samples_second_pass"] > 0 or geom is not OBLIQUE)
        for chunk in chunks:
            for order in (parts, parts[::-1]):
                img2, hits2, stats2 = _render(order, view, tf, "u16", chunk=chunk)
                assert np.array_equal(img2, img) and np.array_equal(hits2, hits) and stats2 == stats, (chunk, order is parts)


# ---- 5: a gap contributes nothing
def test_a_gap_is_neither_evaluated_nor_composited():
    whole = _partition("eight", "c1", "u16")
    parts = whole[:3] + whole[4:]                                # (block 3 is on this view's silhouette: some rays meet it alone)
    view = VW.make_view(DIMS, **OBLIQUE)
    tf = _table(whole, view, "u16")
    vals, evaluated, _ = _restate(parts, view, "u16")
    full = _restate(whole, view, "u16")[1]
    assert evaluated.sum() < full.sum()
    want, want_hits, _ = _python(vals, evaluated, tf, "u16", 0)
    img, hits, stats = _render(parts, view, tf, "u16")
    assert np.array_equal(img, want) and np.array_equal(hits, want_hits)
    lost = (hits == 0) & (full.sum(2) > 0)                       # rays that met the removed block alone: the background, A = 0
    assert lost.any() and (img[hits == 0] == np.array(BG + (0,), np.uint8)).all()
    assert stats["samples_inside"] == int(evaluated.sum()) and stats["blocks_hit"] == 7 and stats["samples_second_pass"] > 0
    assert not np.array_equal(img, _render(whole, view, tf, "u16")[0])


# ---- 6: refusals, before any launch
def test_entries_and_render_composite_partition_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    parts = _partition("eight", "c1", "u16")
    view = VW.make_view(DIMS, (1, 0, 0))
    part = VW.make_part(view, parts[7][1], parts[7][2])
    n, rays = part.wrows * part.wcols, view.rows * view.cols
    k0 = torch.zeros(max(n, rays), dtype=torch.int32, device=DEV)
    off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(4 * max(n, rays), dtype=torch.int64, device=DEV)
    tf = torch.zeros((256, 4), dtype=torch.int32, device=DEV)
    wins, window_rays = CP.windows_table([part])
    d_wins = torch.frombuffer(bytearray(bytes(wins)), dtype=torch.uint8).to(DEV)
    p, st, v, pt = _lib.ptr, _lib.stream_ptr(), C.byref(view), C.byref(part)

    def fold(part=pt, vals=buf, kind=_lib.OUT_U8, channels=2, channel=1, table=tf, bits=8, hits=k0, run=k0, acc=buf, lanes=1, s1=4, r1=1):
        return L.brief_view_composite_part_fold(v, part, p(k0), p(off), 0, s1, 0, r1, lanes, p(vals), kind, channels, channel, p(table), bits, p(hits), p(run),
                                                p(acc), st)

    def carry(w=d_wins, blocks=1, wr=window_rays, cnt=k0, out=k0):
        return L.brief_view_composite_part_carry(v, p(w), blocks, wr, p(k0), p(cnt), p(k0), p(out), p(out), st)

    def gather(w=d_wins, blocks=1, wr=window_rays, acc2=buf, out=buf):
        return L.brief_view_composite_part_gather(v, p(w), blocks, wr, p(k0), p(k0), p(buf), p(k0), p(acc2), p(k0), p(k0), p(out), st)
    for call, what in ((lambda: fold(part=None), "null block"), (lambda: fold(vals=None), "null buffer"), (lambda: fold(run=None), "null buffer"),
                       (lambda: fold(acc=None), "null buffer"), (lambda: fold(table=None), "null transfer table"), (lambda: fold(kind=_lib.OUT_F32), "elem_kind"),
                       (lambda: fold(channel=2), "channel must be 0 .. channels - 1"), (lambda: fold(channels=5), "channels must be 1..4"),
                       (lambda: fold(bits=9), "tf_bits"), (lambda: fold(lanes=3), "power of two"), (lambda: fold(s1=0), "sample range"),
                       (lambda: fold(r1=n + 1), "ray range"),
                       (lambda: carry(w=None), "null table"), (lambda: carry(blocks=0), "blocks must be"), (lambda: carry(wr=0), "window_rays must be"),
                       (lambda: carry(cnt=None), "null buffer"), (lambda: carry(out=None), "null buffer"),
                       (lambda: gather(w=None), "null table"), (lambda: gather(blocks=-1), "blocks must be"), (lambda: gather(wr=0), "window_rays must be"),
                       (lambda: gather(acc2=None), "null buffer"), (lambda: gather(out=None), "null buffer")):
        rc = call()
        assert rc == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and not k0.cpu().numpy().any()
    good = np.zeros((4096, 4), np.int32)
    with pytest.raises(ValueError, match="out_kind must be 'u8' or 'u16'"):
        CP.render_composite_partition(parts, view, good, "f32")
    with pytest.raises(ValueError, match="overlap"):
        CP.render_composite_partition(parts + [parts[3]], view, good, "u16")
    with pytest.raises(ValueError, match="channel count"):
        CP.render_composite_partition(parts[:7] + [_partition("eight", "c4", "u16")[7]], view, good, "u16")
    with pytest.raises(ValueError, match="channel 1 does not exist"):
        CP.render_composite_partition(parts, view, good, "u16", channel=1)
    with pytest.raises(ValueError, match="2\\^bits"):
        CP.render_composite_partition(parts, view, good[:100], "u16")
    bad = good.copy()
    bad[5, 0] = TAU_SAT + 1
    with pytest.raises(ValueError, match="tau must lie in 0 .. TAU_SAT"):
        CP.render_composite_partition(parts, view, bad, "u16")
    with pytest.raises(ValueError, match="at least one block"):
        CP.render_composite_partition([], view, good, "u16")
