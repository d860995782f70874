"""Host side of the composite view of a partition (composite.render_composite_partition / decompress_divide_composite, decompress.py
--view-composite ... --view-owner nearest): the chain part clip -> fold per block -> carry -> fold over the second-pass counts ->
gather -> finish, run by the host restatements brief_view_composite_part_{fold,carry,gather}_host, against the single-list host
composite of the merged list and against Python integers; the order of the blocks; gaps; the carry alone; the header; the refusals.
Nothing here needs a GPU.  Sample values are random integers of the lattice: the fold does not care where values come from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from brief_pytorch_amd import _lib
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import view as V
from brief_pytorch_amd.framework import NFGR, decompress_divide_composite
from tests._composite import TAU_SAT, finish, fold_ray, random_table
from tests.test_view_partition_host import DIMS, EIGHT, MIX, OBLIQUE, ROOT, TWO, VIEWS, _cli, _opt, _side, _tree

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libbrief_hip.so is not built")
BG = (12, 200, 255)
BOX = "3:19,5:26,2:30"


def _dims(box):
    return [b - a + 1 for a, b in zip(*box)]


def _clip(view, boxes):
    """(block descriptors, table of windows, window_rays, k0, cnt, row, col) of the partition, the arrays block-major over the windows"""
    pts = [V.make_part(view, s, _dims((s, e))) for s, e in boxes]
    wins, window_rays = CP.windows_table(pts)
    k0, cnt = np.zeros(window_rays, np.int32), np.zeros(window_rays, np.int32)
    row, col = np.zeros(window_rays, np.int64), np.zeros(window_rays, np.int64)
    for w, pt in zip(wins, pts):
        n = pt.wrows * pt.wcols
        if n:
            a, b = V.part_clip_host(view, pt)
            sl = slice(w.base, w.base + n)
            k0[sl], cnt[sl] = a.ravel(), b.ravel()
            r, c = np.divmod(np.arange(n), pt.wcols)
            row[sl], col[sl] = pt.row0 + r, pt.col0 + c
    return pts, wins, window_rays, k0, cnt, row, col


def _march(view, pts, wins, k0, counts, row, col, lattice, tf, channel, hits_w, tau_w, acc_w):
    """one pass of the host chain: every block's list (the window rays with counts > 0) through brief_view_composite_part_fold_host"""
    off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    for w, pt in zip(wins, pts):
        n = pt.wrows * pt.wcols
        if not n:
            continue
        sl = slice(w.base, w.base + n)
        cnt_b = counts[sl]
        r = np.repeat(np.arange(w.base, w.base + n), cnt_b)
        k = np.repeat(k0[sl], cnt_b) + (np.arange(int(cnt_b.sum())) - np.repeat(off[sl] - off[w.base], cnt_b))
        vals = np.ascontiguousarray(lattice[row[r], col[r], k])
        CP.part_fold_host(view, pt, k0[sl], off[w.base:w.base + n + 1], vals, tf, None if hits_w is None else hits_w[sl], tau_w[sl], acc_w[sl], channel)


def _chain(view, boxes, lattice, tf, channel=0, bg=BG):
    """(image, hits, tau_run, acc, facts) of the whole host chain"""
    pts, wins, window_rays, k0, cnt, row, col = _clip(view, boxes)
    hits_w, tau_w, acc_w = np.zeros(window_rays, np.int32), np.zeros(window_rays, np.int32), np.zeros((window_rays, 3), np.uint64)
    _march(view, pts, wins, k0, cnt, row, col, lattice, tf, channel, hits_w, tau_w, acc_w)
    assert np.array_equal(hits_w, cnt)                               # (a window ray's interval holds owned samples only)
    carry, cnt2 = CP.part_carry_host(view, wins, window_rays, k0, cnt, tau_w)
    tau_w2, acc_w2 = carry.copy(), np.zeros((window_rays, 3), np.uint64)
    _march(view, pts, wins, k0, cnt2, row, col, lattice, tf, channel, None, tau_w2, acc_w2)
    hits, tau_run, acc = CP.part_gather_host(view, wins, window_rays, hits_w, tau_w, acc_w, carry, acc_w2)
    img = np.array([finish(int(t), [int(x) for x in a], bg) for t, a in zip(tau_run.ravel(), acc.reshape(-1, 3))], np.uint8).reshape(view.rows, view.cols, 4)
    live = cnt > 0
    per_pixel = np.bincount(row[live] * view.cols + col[live], minlength=view.rows * view.cols)
    # a segment with C == 0 that lies behind another one: everything in front of it is transparent
    order = np.lexsort((k0[live], row[live] * view.cols + col[live]))
    pix, first = (row[live] * view.cols + col[live])[order], np.ones(int(live.sum()), bool)
    first[1:] = pix[1:] != pix[:-1]
    facts = dict(segments=int(live.sum()), most=int(per_pixel.max()), behind_clear=int(((carry[live][order] == 0) & ~first).sum()),
                 partly=int(((carry > 0) & (carry < TAU_SAT) & live).sum()), hidden=int(((carry == TAU_SAT) & live).sum()),
                 first=int(cnt.sum()), second=int(cnt2.sum()))
    assert facts["second"] == int(cnt[(carry > 0) & (carry < TAU_SAT)].sum()) and not cnt2[(carry == 0) | (carry == TAU_SAT)].any()
    return img, hits, tau_run, acc, facts


def _merged(view, boxes):
    """per pixel the owned samples in ascending k, from the blocks' intervals: (owned [rows, cols, depth] bool, owner int)"""
    owner = np.full((view.rows, view.cols, view.depth), -1, np.int32)
    for b, (s, e) in enumerate(boxes):
        pt = V.make_part(view, s, _dims((s, e)))
        if pt.wrows * pt.wcols == 0:
            continue
        k0, cnt = V.part_clip_host(view, pt)
        for wr, wc in zip(*np.nonzero(cnt)):
            seg = owner[pt.row0 + wr, pt.col0 + wc, k0[wr, wc]:k0[wr, wc] + cnt[wr, wc]]
            assert (seg == -1).all()
            seg[:] = b
    return owner


def _python(view, owner, lattice, tf, channel, bg=BG):
    """the definition in Python integers: a pixel's owned samples in ascending k through tests/_composite.py's fold and finish"""
    shift = 8 * lattice.dtype.itemsize - (len(tf).bit_length() - 1)
    img = np.zeros((view.rows, view.cols, 4), np.uint8)
    hits, runs = np.zeros((view.rows, view.cols), np.int32), np.zeros((view.rows, view.cols), np.int32)
    accs = np.zeros((view.rows, view.cols, 3), np.uint64)
    for r in range(view.rows):
        for c in range(view.cols):
            ks = np.nonzero(owner[r, c] >= 0)[0]
            run, acc = fold_ray([tf[int(lattice[r, c, k, channel]) >> shift] for k in ks])
            img[r, c], hits[r, c], runs[r, c], accs[r, c] = finish(run, acc, bg), len(ks), run, [a % (1 << 64) for a in acc]
    return img, hits, runs, accs


def _lattice(view, dtype, channels, seed, owner=None, clear=()):
    """random integers on the whole lattice; the samples of the blocks in `clear` are drawn from the lower half of the dtype's range"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max + 1
    lat = rng.integers(0, top, (view.rows, view.cols, view.depth, channels)).astype(dtype)
    for b in clear:
        lat[owner == b] = rng.integers(0, top // 2, (int((owner == b).sum()), channels)).astype(dtype)
    return lat


def _step_table(bits, seed, dense=False):
    """the lower half of the rows transparent (tau = 0, with emissions that must not count), the upper half faint (a ray stays
    half-transparent over a segment) or, dense, mixed with rows that saturate within a few samples"""
    rng = np.random.default_rng(seed)
    n = 1 << bits
    tf = np.zeros((n, 4), np.int32)
    tf[:, 1:] = rng.integers(0, 65281, (n, 3))
    tf[n // 2:, 0] = rng.integers(200, 9000, n - n // 2)
    if dense:
        tf[n // 2::3, 0] = rng.integers(TAU_SAT // 6, TAU_SAT // 2, len(tf[n // 2::3]))
    return tf


# ---- the whole host chain against the single-list host and against Python integers
@needs_lib
@pytest.mark.parametrize("pname,vname,region,dtype,channels,channel,table", [
    ("eight", "oblique", None, np.uint8, 1, 0, ("random", 8)), ("eight", "oblique", BOX, np.uint16, 3, 2, ("random", 12)),
    ("mix", "oblique", None, np.uint16, 1, 0, ("random", 5)), ("mix", "skim", None, np.uint8, 2, 1, ("random", 3)),
    ("eight", "oblique", None, np.uint16, 1, 0, ("step", 12)), ("mix", "oblique", BOX, np.uint8, 1, 0, ("step", 8)),
    ("mix", "oblique", None, np.uint8, 1, 0, ("dense", 6)), ("eight", "z@1", None, np.uint16, 1, 0, ("dense", 16)),
    ("eight", "x@0.5", BOX, np.uint8, 1, 0, ("random", 1))])
def test_host_chain_equals_the_single_list_host_and_python_integers(pname, vname, region, dtype, channels, channel, table):
    boxes = {"eight": EIGHT, "mix": MIX}[pname]
    view = V.make_view(DIMS, region=region, **VIEWS[vname])
    owner = _merged(view, boxes)
    lattice = _lattice(view, dtype, channels, len(pname) + channels, owner, clear=(0, 5) if table[0] != "random" else ())
    tf = random_table(np.random.default_rng(table[1]), table[1]) if table[0] == "random" else _step_table(table[1], 3, dense=table[0] == "dense")
    img, hits, tau_run, acc, facts = _chain(view, boxes, lattice, tf, channel)
    # the merged list: for a tiling partition the union of a ray's segments is the ray's own interval
    K0, CNT = V.clip_host(view)
    assert np.array_equal((owner >= 0).sum(2), CNT)
    off = np.concatenate([[0], np.cumsum(CNT.ravel(), dtype=np.int64)])
    r = np.repeat(np.arange(view.rows * view.cols), CNT.ravel())
    k = np.repeat(K0.ravel(), CNT.ravel()) + (np.arange(int(off[-1])) - np.repeat(off[:-1], CNT.ravel()))
    vals = np.ascontiguousarray(lattice[r // view.cols, r % view.cols, k])
    want = CP.composite_host(view, K0.ravel(), off, vals, tf, channel=channel, background=BG)
    for g, w, what in zip((img, hits, tau_run, acc), want, ("image", "hits", "tau_run", "acc")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, int((g != w).sum()))
    for g, w, what in zip((img, hits, tau_run, acc), _python(view, owner, lattice, tf, channel), ("image", "hits", "tau_run", "acc")):
        assert np.array_equal(g, w), what
    # what keeps this from being vacuous
    assert facts["most"] >= 3 or "@" in vname, facts
    assert 0 < facts["second"] < facts["first"] or table == ("random", 1), facts
    assert (hits == 0).any() or "@" in vname
    if table[0] != "random":
        assert facts["behind_clear"] > 0 and facts["partly"] > 0, facts
        assert ((tau_run > 0) & (tau_run < TAU_SAT)).any()
    if table[0] != "step":
        assert facts["hidden"] > 0 and (tau_run == TAU_SAT).any(), facts
    if table[0] == "dense":
        assert facts["behind_clear"] > 0 and facts["partly"] > 0 and facts["hidden"] > 0, facts


# ---- the order of the blocks
@needs_lib
def test_the_order_of_the_blocks_changes_no_bit():
    view = V.make_view(DIMS, **OBLIQUE)
    owner = _merged(view, MIX)
    tf = _step_table(8, 11, dense=True)
    lattice = _lattice(view, np.uint8, 1, 4, owner, clear=(0, 5))
    base = _chain(view, MIX, lattice, tf)
    assert base[4]["partly"] > 0 and base[4]["hidden"] > 0 and base[4]["behind_clear"] > 0
    for order in (list(range(len(MIX)))[::-1], list(np.random.default_rng(5).permutation(len(MIX)))):
        got = _chain(view, [MIX[i] for i in order], lattice, tf)
        for g, w in zip(got[:4], base[:4]):
            assert np.array_equal(g, w), order
        assert got[4] == base[4]


# ---- gaps
@needs_lib
@pytest.mark.parametrize("gone", [3, 0])
def test_a_gap_contributes_nothing(gone):
    view = V.make_view(DIMS, **OBLIQUE)
    boxes = EIGHT[:gone] + EIGHT[gone + 1:]
    owner, full = _merged(view, boxes), _merged(view, EIGHT)
    assert (owner >= 0).sum() < (full >= 0).sum()
    tf = _step_table(8, 12, dense=True)
    lattice = _lattice(view, np.uint8, 1, 6, full, clear=(1, 6))
    img, hits, tau_run, acc, facts = _chain(view, boxes, lattice, tf)
    for g, w, what in zip((img, hits, tau_run, acc), _python(view, owner, lattice, tf, 0), ("image", "hits", "tau_run", "acc")):
        assert np.array_equal(g, w), what
    whole = _chain(view, EIGHT, lattice, tf)
    assert not np.array_equal(whole[0], img)
    lost = (hits == 0) & ((full >= 0).sum(2) > 0)                # rays that met the removed block alone show the background, A = 0
    assert (lost.any() or gone == 0) and (img[hits == 0] == np.array(BG + (0,), np.uint8)).all()
    assert facts["partly"] > 0 and facts["second"] > 0


# ---- the carry alone, on hand-made totals
@needs_lib
def test_carry_orders_by_k0_saturates_and_skips_what_needs_no_second_pass():
    view = V.make_view((8, 8, 8), (1, 0, 0))
    rays = view.rows * view.cols
    pts = [V.make_part(view, (0, 0, 0), (8, 8, 8), "image") for _ in range(4)]      # four windows over the whole image: any segments can be named
    pts[2] = V.make_part(view, (0, 0, 0), (8, 8, 8), (2, 3, 4, 5))                # ... and one that holds some pixels only
    wins, window_rays = CP.windows_table(pts)
    assert window_rays == 3 * rays + 20 and [w.base for w in wins] == [0, rays, 2 * rays, 2 * rays + 20]
    rng = np.random.default_rng(1)
    k0 = rng.permuted(np.tile(np.arange(4, dtype=np.int32) * 2, (rays, 1)), axis=1)      # per pixel the four blocks in a random depth order
    cnt = rng.integers(0, 3, (rays, 4)).astype(np.int32)
    tau = np.array([0, 0, 1, 700, TAU_SAT // 2, TAU_SAT // 2 + 1, TAU_SAT], np.int32)[rng.integers(0, 7, (rays, 4))]
    tau[cnt == 0] = 0
    K0, CNT, TAU = (np.zeros(window_rays, np.int32) for _ in range(3))
    where = np.full((rays, 4), -1, np.int64)
    for b, (w, pt) in enumerate(zip(wins, pts)):
        for i in range(pt.wrows * pt.wcols):
            pixel = (pt.row0 + i // pt.wcols) * view.cols + pt.col0 + i % pt.wcols
            where[pixel, b] = w.base + i
            K0[w.base + i], CNT[w.base + i], TAU[w.base + i] = k0[pixel, b], cnt[pixel, b], tau[pixel, b]
    carry, cnt2 = CP.part_carry_host(view, wins, window_rays, K0, CNT, TAU)
    kinds = set()
    for pixel in range(rays):
        for b in range(4):
            x = where[pixel, b]
            if x < 0:
                continue
            front = [int(tau[pixel, o]) for o in range(4) if where[pixel, o] >= 0 and cnt[pixel, o] > 0 and k0[pixel, o] < k0[pixel, b]]
            want = min(sum(front), TAU_SAT) if cnt[pixel, b] > 0 else 0
            assert carry[x] == want, (pixel, b)
            assert cnt2[x] == (cnt[pixel, b] if 0 < want < TAU_SAT else 0), (pixel, b)
            if cnt[pixel, b] > 0:
                kinds.add(("zero", "partly", "sat")[(want > 0) + (want == TAU_SAT)] + ("+front" if front else ""))
                if sum(front) > TAU_SAT:
                    kinds.add("clamped")
    assert kinds == {"zero", "zero+front", "partly+front", "sat+front", "clamped"}, kinds
    # the table itself is checked where it is host memory
    L, p = _lib.lib(), (lambda a: a.ctypes.data_as(C.c_void_p))
    out = np.zeros((2, window_rays), np.int32)
    for b, field, value, what in ((2, "base", 1, "bases"), (2, "wrows", -1, "at least 1 x 1"), (2, "row0", 7, "inside the image"),
                                  (3, "wcols", 7, "window_rays rays together")):
        bad = (_lib.CompositeWindow * 4).from_buffer_copy(wins)
        setattr(bad[b], field, value)
        rc = L.brief_view_composite_part_carry_host(C.byref(view), bad, 4, window_rays, p(K0), p(CNT), p(TAU), p(out[0]), p(out[1]))
        assert rc == -1 and what in L.brief_last_error().decode(), (field, L.brief_last_error())
    for call, what in ((lambda: L.brief_view_composite_part_carry_host(C.byref(view), None, 4, window_rays, p(K0), p(CNT), p(TAU), p(out[0]), p(out[1])), "null table"),
                       (lambda: L.brief_view_composite_part_carry_host(C.byref(view), wins, 0, window_rays, p(K0), p(CNT), p(TAU), p(out[0]), p(out[1])), "blocks must be"),
                       (lambda: L.brief_view_composite_part_carry_host(C.byref(view), wins, 4, 0, p(K0), p(CNT), p(TAU), p(out[0]), p(out[1])), "window_rays must be"),
                       (lambda: L.brief_view_composite_part_carry_host(C.byref(view), wins, 4, window_rays, p(K0), None, p(TAU), p(out[0]), p(out[1])), "null buffer"),
                       (lambda: L.brief_view_composite_part_gather_host(C.byref(view), wins, 4, window_rays, p(K0), p(TAU), None, p(K0), p(K0), p(out[0]), p(out[1]),
                                                                        p(out[0])), "null buffer")):
        assert call() == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    assert not out.any()


@needs_lib
def test_fold_host_refuses_bad_arguments_by_name():
    L, p = _lib.lib(), (lambda a: a.ctypes.data_as(C.c_void_p))
    view = V.make_view(DIMS, (1, 0, 0))
    part = V.make_part(view, (12, 0, 0), (11, 31, 37))
    n = part.wrows * part.wcols
    k0, off = np.full(n, 12, np.int32), np.arange(n + 1, dtype=np.int64) + 5      # one owned sample per window ray
    vals, tf = np.zeros((n, 2), np.uint8), np.zeros((256, 4), np.int32)
    state = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.uint64)]

    def call(part=part, k0=k0, off=off, vals=vals, kind=_lib.OUT_U8, channels=2, channel=1, tf=tf, bits=8, tau_w=state[1]):
        return L.brief_view_composite_part_fold_host(C.byref(view), C.byref(part) if part is not None else None, p(k0), p(off), p(vals) if vals is not None else None,
                                                     kind, channels, channel, p(tf) if tf is not None else None, bits, p(state[0]), p(tau_w), p(state[2]))
    assert call() == 0
    bad_part = _lib.ViewPart.from_buffer_copy(part)
    bad_part.wcols = view.cols + 1
    for kw, what in ((dict(part=None), "null block"), (dict(part=bad_part), "window"), (dict(vals=None), "null buffer"), (dict(tf=None), "null transfer table"),
                     (dict(kind=_lib.OUT_F32), "elem_kind"), (dict(channel=2), "channel must be 0 .. channels - 1"), (dict(channels=5), "channels must be 1..4"),
                     (dict(bits=9), "tf_bits"), (dict(off=off[::-1].copy()), "off must not decrease"), (dict(k0=np.full(n, view.depth, np.int32)), "inside 0 .. depth - 1"),
                     (dict(tau_w=np.full(n, TAU_SAT + 1, np.int32)), "carry-in")):
        assert call(**kw) == -1 and what in L.brief_last_error().decode(), (what, L.brief_last_error())
    assert (state[0] == 1).all() and not state[1].any() and not state[2].any()      # the one good call, and nothing since


# ---- the header
ENTRIES = {
    "brief_view_composite_part_fold": (
        ["const brief_view_desc *view", "const brief_view_part *part", "const int32_t *k0", "const int64_t *off", "int64_t s0", "int64_t s1", "int64_t r0",
         "int64_t r1", "int32_t lanes", "const void *vals", "int elem_kind", "int32_t channels", "int32_t channel", "const int32_t *tf", "int32_t tf_bits",
         "int32_t *hits_w", "int32_t *tau_w", "uint64_t *acc_w", "void *stream"], "wpvvllllivniivivvvv"),
    "brief_view_composite_part_carry": (
        ["const brief_view_desc *view", "const brief_composite_window *wins", "int32_t blocks", "int64_t window_rays", "const int32_t *k0", "const int32_t *cnt",
         "const int32_t *tau_w", "int32_t *carry", "int32_t *cnt2", "void *stream"], "wvilvvvvvv"),
    "brief_view_composite_part_gather": (
        ["const brief_view_desc *view", "const brief_composite_window *wins", "int32_t blocks", "int64_t window_rays", "const int32_t *hits_w",
         "const int32_t *tau_w", "const uint64_t *acc_w", "const int32_t *carry", "const uint64_t *acc_w2", "int32_t *hits", "int32_t *tau_run", "uint64_t *acc",
         "void *stream"], "wvilvvvvvvvvv"),
    "brief_view_composite_part_fold_host": (
        ["const brief_view_desc *view", "const brief_view_part *part", "const int32_t *k0", "const int64_t *off", "const void *vals", "int elem_kind",
         "int32_t channels", "int32_t channel", "const int32_t *tf", "int32_t tf_bits", "int32_t *hits_w", "int32_t *tau_w", "uint64_t *acc_w"], "wpvvvniivivvv"),
    "brief_view_composite_part_carry_host": (
        ["const brief_view_desc *view", "const brief_composite_window *wins", "int32_t blocks", "int64_t window_rays", "const int32_t *k0", "const int32_t *cnt",
         "const int32_t *tau_w", "int32_t *carry", "int32_t *cnt2"], "wvilvvvvv"),
    "brief_view_composite_part_gather_host": (
        ["const brief_view_desc *view", "const brief_composite_window *wins", "int32_t blocks", "int64_t window_rays", "const int32_t *hits_w",
         "const int32_t *tau_w", "const uint64_t *acc_w", "const int32_t *carry", "const uint64_t *acc_w2", "int32_t *hits", "int32_t *tau_run", "uint64_t *acc"],
        "wvilvvvvvvvv"),
}


def test_header_exports_and_ctypes_signatures_agree():
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    codes = {"w": C.POINTER(_lib.ViewDesc), "p": C.POINTER(_lib.ViewPart), "v": C.c_void_p, "l": C.c_int64, "i": C.c_int32, "n": C.c_int}
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
    fields = re.search(r"typedef struct \{([^}]*)\} brief_composite_window;", plain).group(1)
    assert " ".join(fields.split()) == "int64_t base; int32_t row0, col0, wrows, wcols;"
    assert [f[0] for f in _lib.CompositeWindow._fields_] == ["base", "row0", "col0", "wrows", "wcols"] and C.sizeof(_lib.CompositeWindow) == 24
    assert "#define BRIEF_VERSION 130" in text                    # the entries are additive


# ---- refusals, with nothing written and no net opened
TF = "0:0,0,0,0;40000:255,128,0,0.3"


@pytest.mark.parametrize("case,words", [
    ("postprocess", "composite view with a Decompress.postprocess that changes values"),
    ("channel", "channel 1 does not exist"),
    ("background", "background must be three integers"),
    ("transfer", "levels must be strictly ascending"),
    ("error_bound", "error-bounded.*error_bound 3"),
    ("overlap", "d_0_3-h_0_7-w_0_7 and d_3_7-h_0_7-w_0_7 overlap"),
    ("2d", "3-D data only"),
    ("dtype", "one dtype for all blocks"),
    ("channels", "not its index range of a volume with 1 channels"),
])
def test_artefact_refusals_are_raised_before_any_net_is_opened(tmp_path, case, words):
    blocks, shape, opt, kw, tf = dict(TWO), [8, 8, 8, 1], _opt(), {}, TF
    if case == "postprocess":
        opt.CompressFramework.Decompress.postprocess.denoise.level = 500
    elif case == "channel":
        kw = dict(channel=1)
    elif case == "background":
        kw = dict(background=(0, 0, 256))
    elif case == "transfer":
        tf = "5:0,0,0,0;5:1,1,1,1"
    elif case == "error_bound":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], error_bound=3)
    elif case == "overlap":
        blocks = {"d_0_3-h_0_7-w_0_7": _side([4, 8, 8, 1]), "d_3_7-h_0_7-w_0_7": _side([5, 8, 8, 1])}
    elif case == "2d":
        blocks, shape = {"h_0_3-w_0_7": _side([4, 8, 1]), "h_4_7-w_0_7": _side([4, 8, 1])}, [8, 8, 1]
    elif case == "dtype":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 1], dtype="uint8")
    elif case == "channels":
        blocks["d_4_7-h_0_7-w_0_7"] = _side([4, 8, 8, 2])
    args = _tree(tmp_path, blocks, shape)
    with pytest.raises(ValueError, match=words):
        decompress_divide_composite(opt, *args, (1, 0, 0), tf, **kw)
    assert callable(NFGR.decompress_divide_composite)            # (the method needs a GPU to construct its NFGR: tests/test_gpu_composite_partition_framework.py)
    assert all(not os.listdir(os.path.join(args[1], n)) for n in os.listdir(args[1]))


def test_the_single_artefact_entries_still_refuse_a_divide_artefact():
    with pytest.raises(ValueError, match="composite view of a DivideTask artefact.*prefix.*follow-up.*--view-owner nearest"):
        NFGR.decompress_composite(_opt(), "nowhere", {"data_shape": [8, 8, 8, 1]}, (1, 0, 0), TF)
    with pytest.raises(ValueError, match="composite view of a DivideTask artefact"):
        CP.open_single(_opt(), "nowhere", {"data_shape": [8, 8, 8, 1]})


@pytest.mark.parametrize("divide,extra,out,words", [
    (False, ["--view-owner", "nearest"], "c.png", ["--view-composite with --view-owner: a composite is a view of its own"]),
    (False, ["--view-owner", "farthest"], "c.png", ["--view-composite with --view-owner: a composite is a view of its own"]),
    (True, ["--view-owner", "farthest"], "c.png", ["--view-owner farthest", "unknown rule", "nearest"]),
    (True, ["--view-owner", "nearest"], "c.tif", ["--view-composite writes an RGB image as .png or the RGBA array as .npy (got .tif)"]),
    (True, [], "c.png", ["--view-composite: a composite view of a DivideTask artefact", "follow-up", "--view-owner nearest"]),
    (True, ["--view-owner", "nearest", "--view-mode", "mean"], "c.npy", ["--view-composite with --view-mode mean"]),
    (True, ["--view-owner", "nearest", "--view-surface", "100"], "c.png", ["--view-composite with --view-surface"]),
])
def test_cli_refusals_write_nothing(tmp_path, divide, extra, out, words):
    os.makedirs(str(tmp_path / "art" / ("sideinfos" if divide else "module")))
    os.makedirs(str(tmp_path / "out"))
    argv = ["-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"), "-c", str(tmp_path / "art"), "--region", ":,:,:",
            "-o", str(tmp_path / "out" / out), "--view", "1,0,0", "--view-composite", TF] + extra
    with pytest.raises(SystemExit) as e:
        _cli().main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.listdir(str(tmp_path / "out"))
    doc = _cli().main.__globals__["__doc__"]
    assert "--view-composite SPEC --view-owner nearest" in doc
