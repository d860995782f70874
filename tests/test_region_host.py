"""Region decode, host side (no GPU): region / shape parsing and its refusals, the block-intersection arithmetic of
decompress_divide_region against numpy slicing of a merged volume, and brief_grid_box's layout in the ctypes binding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from brief_pytorch_amd import _lib
from brief_pytorch_amd.misc import chunk_name, divide_data, merge_divided_data, parse_chunk_name
from brief_pytorch_amd.region import block_intersection, extents, normalize_region, parse_region, parse_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_region_forms():
    assert parse_region("0:4,2:9,1:3") == (slice(0, 4), slice(2, 9), slice(1, 3))
    assert parse_region(" 3:7 , : ") == (slice(3, 7), slice(None, None))
    assert parse_region("5:,:6,1:9:2") == (slice(5, None), slice(None, 6), slice(1, 9, 2))
    for bad in ("0:4,x:9", "4", "1:2:3:4", "0:4,,1:2"):
        with pytest.raises(ValueError):
            parse_region(bad)
    assert parse_shape("63,64,65") == [63, 64, 65]
    for bad in ("63,0,4", "a,b", "3.5,2"):
        with pytest.raises(ValueError):
            parse_shape(bad)


def test_normalize_region_matches_numpy_and_refuses():
    dims = (11, 13, 7)
    vol = np.arange(np.prod(dims)).reshape(dims)
    for reg, step in [((slice(None),) * 3, 1), ((slice(2, 9), slice(0, 13), slice(6, 7)), 1), ((slice(1, 11), slice(3, 12), slice(0, 7)), 3),
                      ((slice(0, 11, 7), slice(5, 6), slice(None, None, 2)), 1), ("10:11,12:13,6:7", 2)]:
        b, e, s = normalize_region(dims, reg, step)
        ext = extents(b, e, s)
        sl = tuple(slice(x, y, z) for x, y, z in zip(b, e, s))
        assert list(vol[sl].shape) == ext
        if not isinstance(reg, str):
            want = vol[tuple(slice(r.start, r.stop, r.step if r.step is not None else step) for r in reg)]
            np.testing.assert_array_equal(vol[sl], want)
    for reg, step in [((slice(0, 12), slice(None), slice(None)), 1),       # past the end
                      ((slice(-1, 5), slice(None), slice(None)), 1),       # negative bound: refused, not wrapped
                      ((slice(4, 4), slice(None), slice(None)), 1),        # empty
                      ((slice(5, 2), slice(None), slice(None)), 1),        # reversed
                      ((slice(None), slice(None), slice(None)), 0),        # step 0
                      ((slice(None, None, -1), slice(None), slice(None)), 1),
                      ((slice(None), slice(None)), 1),                     # wrong rank
                      ((slice(0.5, 3), slice(None), slice(None)), 1)]:
        with pytest.raises(ValueError):
            normalize_region(dims, reg, step)


def _merged_region(data, chunks, region, step):
    """what decompress_divide_region does, on synthetic block arrays instead of decoded ones"""
    dims = list(data.shape[:-1])
    b, e, s = normalize_region(dims, region, step)
    ext = extents(b, e, s)
    axes = "dhw" if len(dims) == 3 else "hw"
    out = np.zeros(ext + [data.shape[-1]], np.float32)
    dtype = None
    for c in sorted(chunks, key=lambda c: c["name"]):
        r = parse_chunk_name(c["name"])
        dtype = dtype or c["data"].dtype
        hit = block_intersection(b, s, ext, [r[a][0] for a in axes], [r[a][1] for a in axes])
        if hit is None:
            continue
        o_lo, o_hi, l_b, l_e = hit
        out[tuple(slice(x, y) for x, y in zip(o_lo, o_hi))] += c["data"][tuple(slice(x, y, z) for x, y, z in zip(l_b, l_e, s))]
    return out.clip(None, np.iinfo(dtype).max).astype(dtype)


def _blocks(data, divide_type, prune=()):
    chunks, _ = divide_data(data, divide_type)
    out = []
    for i, c in enumerate(chunks):
        if i in prune:
            continue              # an adaptive partition drops blocks: their voxels decode to 0
        out.append({"name": chunk_name(c), "data": c["data"], **parse_chunk_name(chunk_name(c))})
    return out


@pytest.mark.parametrize("shape,divide_type,prune", [((20, 17, 23, 1), "total_2_2_2", ()), ((20, 17, 23, 1), "total_3_2_4", ()),
                                                      ((21, 16, 18, 1), "every_8_8_8", ()), ((24, 24, 24, 1), "every_8_8_8", (1, 5, 13)),
                                                      ((17, 29, 1), "total_3_2", ()), ((17, 29, 1), "every_6_8", (2,))])
def test_block_intersection_equals_slice_of_merge(shape, divide_type, prune):
    rng = np.random.default_rng(len(shape) * 100 + sum(shape))
    data = rng.integers(0, 65535, size=shape, dtype=np.uint16)
    chunks = _blocks(data, divide_type, prune)
    whole = merge_divided_data(chunks, list(shape))
    dims = shape[:-1]
    regions = [tuple(slice(None) for _ in dims)]
    for _ in range(12):
        reg = []
        for n in dims:
            a = int(rng.integers(0, n))
            reg.append(slice(a, int(rng.integers(a + 1, n + 1))))
        regions.append(tuple(reg))
    for reg in regions:
        for step in (1, 2, 3, 7):
            got = _merged_region(data, chunks, reg, step)
            want = whole[tuple(slice(r.start, r.stop, step) for r in reg)]
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want, err_msg="%s %s step %d" % (divide_type, reg, step))


def test_block_intersection_misses_and_lattice():
    # region 1:20:3 -> samples 1, 4, 7, 10, 13, 16, 19; block [5, 9] holds 7 (i = 2), block [8, 9] none, block [19, 30] holds 19 (i = 6)
    assert block_intersection([1], [3], [7], [5], [9]) == ([2], [3], [2], [3])
    assert block_intersection([1], [3], [7], [8], [9]) is None
    assert block_intersection([1], [3], [7], [19], [30]) == ([6], [7], [0], [1])
    assert block_intersection([10], [1], [5], [0], [9]) is None               # block entirely before the region
    assert block_intersection([10], [2], [5], [11], [17]) == ([1], [4], [1], [6])


_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "brief_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(brief_grid_box), offsetof(brief_grid_box, grid), offsetof(brief_grid_box, start),
           offsetof(brief_grid_box, step), offsetof(brief_grid_box, extent));
    return 0;
}
"""


def test_grid_box_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B = _lib.GridBox
    assert got == [C.sizeof(B), B.grid.offset, B.start.offset, B.step.offset, B.extent.offset]
    assert C.sizeof(_lib.GridDesc) == B.start.offset                 # brief_grid_desc unchanged, the box fields right behind it
    assert "brief_siren_forward_box" in _lib.EXPORTS
