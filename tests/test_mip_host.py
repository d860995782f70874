"""Host side of the projection decode (brief_pytorch_amd/mip.py, decompress.py --mip): chunk planning, the refusals, the C-ABI's
declaration.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from brief_pytorch_amd import _lib, config, mip
from brief_pytorch_amd.framework import NFGR, decompress_divide_mip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extent", [(1, 1, 1), (5, 7, 9), (3, 300, 5), (70, 45, 133)])
@pytest.mark.parametrize("limit", [1, 7, 1000, 10 ** 9])
def test_plan_chunks_tiles_the_box_exactly_and_in_order(extent, limit):
    pieces = mip.plan_chunks(extent, limit)
    seen = np.zeros(extent, np.int32)
    order = np.arange(int(np.prod(extent))).reshape(extent)
    last = -1
    for lo, hi in pieces:
        assert len(lo) == len(hi) == 3 and all(0 <= a < b <= n for a, b, n in zip(lo, hi, extent)), (lo, hi)
        assert np.prod([b - a for a, b in zip(lo, hi)]) <= limit, (lo, hi)
        seen[tuple(slice(a, b) for a, b in zip(lo, hi))] += 1
        first = int(order[tuple(lo)])
        assert first > last, "pieces are not in z-major order"
        last = first
        # whole slices first, then whole rows of one slice, then pieces of one row
        if hi[2] - lo[2] < extent[2]:
            assert extent[2] > limit and hi[0] - lo[0] == 1 and hi[1] - lo[1] == 1
        elif hi[1] - lo[1] < extent[1]:
            assert extent[1] * extent[2] > limit and hi[0] - lo[0] == 1
    assert (seen == 1).all()
    if limit >= np.prod(extent):
        assert pieces == [((0, 0, 0), tuple(extent))]


def test_plan_chunks_refuses_nonsense():
    for extent, limit in (((4, 4), 10), ((0, 4, 4), 10), ((4, 4, 4), 0)):
        with pytest.raises(ValueError):
            mip.plan_chunks(extent, limit)


def _opt():
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    opt.CompressFramework.Decompress.postprocess.denoise.close = False
    return opt


def _side(**kw):
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


def test_refusals_are_raised_by_name_before_any_decode(tmp_path):
    """each on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    mod = str(tmp_path / "module")
    with pytest.raises(ValueError, match="3-D data only"):
        NFGR.decompress_mip(_opt(), mod, _side(data_shape=[50, 61, 3]))
    with pytest.raises(ValueError, match="uint8 / uint16 data only.*float32"):
        NFGR.decompress_mip(_opt(), mod, _side(dtype="float32"))
    o = _opt()
    o.CompressFramework.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmaxany_a_b.*minmax01"):
        NFGR.decompress_mip(o, mod, _side())
    o = _opt()
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    o.CompressFramework.Decompress.postprocess.denoise.close = [2, 2, 2]
    with pytest.raises(ValueError, match="not local to a voxel"):
        NFGR.decompress_mip(o, mod, _side())
    with pytest.raises(ValueError, match="resampled view"):
        mip.decompress_mip(_opt(), mod, _side(), shape=(16, 18, 20))
    # a promised bound without its corrections file raises, as everywhere
    from brief_pytorch_amd.corrections import CorrectionsError
    with pytest.raises(CorrectionsError, match="missing"):
        NFGR.decompress_mip(_opt(), mod, _side(error_bound=3))
    # a region outside the grid is refused by the region's own rules
    with pytest.raises(ValueError, match="outside"):
        NFGR.decompress_mip(_opt(), mod, _side(), region="0:9,:,:")


def _write_blocks(tmp_path, names, **side_kw):
    import yaml
    for n in names:
        os.makedirs(str(tmp_path / "module" / n))
        os.makedirs(str(tmp_path / "sideinfos" / n))
        with open(str(tmp_path / "sideinfos" / n / "sideinfos.yaml"), "w") as f:
            yaml.safe_dump(_side(**side_kw), f)
    return {"data_shape": [8, 8, 8, 1]}, str(tmp_path / "module"), str(tmp_path / "sideinfos")


def test_divide_refusals(tmp_path):
    args = _write_blocks(tmp_path / "a", ["d_0_4-h_0_7-w_0_7", "d_4_7-h_0_7-w_0_7"])
    with pytest.raises(ValueError, match="overlap"):
        decompress_divide_mip(_opt(), *args)
    args = _write_blocks(tmp_path / "b", ["d_0_3-h_0_7-w_0_7", "d_4_7-h_0_7-w_0_7"], dtype="float32")
    with pytest.raises(ValueError, match="uint8 / uint16 data only"):
        decompress_divide_mip(_opt(), *args)
    args = _write_blocks(tmp_path / "c", ["h_0_3-w_0_7", "h_4_7-w_0_7"])
    with pytest.raises(ValueError, match="3-D data only"):
        decompress_divide_mip(_opt(), {"data_shape": [8, 8, 1]}, *args[1:])
    args = _write_blocks(tmp_path / "d", ["d_0_3-h_0_7-w_0_7", "d_4_7-h_0_7-w_0_7"])
    with pytest.raises(ValueError, match="resampled view"):
        mip.decompress_divide_mip(_opt(), *args, shape=(4, 4, 4))


def test_header_exports_and_ctypes_signature_agree():
    assert "brief_mip_accumulate" in _lib.EXPORTS
    text = open(os.path.join(ROOT, "include", "brief_hip.h")).read()
    assert "#define BRIEF_VERSION 130" in text
    proto = re.search(r"int\s+brief_mip_accumulate\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    assert proto, "brief_mip_accumulate is not declared in include/brief_hip.h"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    assert params == ["const void *src", "int elem_kind", "const int64_t extent[3]", "int32_t channels", "void *mip_d", "void *mip_h",
                      "void *mip_w", "const int64_t origin[3]", "const int64_t frame[3]", "void *stream"]
    if os.path.exists(_lib.LIB_PATH):                            # the signature the loaded library was given
        fn = _lib.lib().brief_mip_accumulate
        i3 = C.POINTER(C.c_int64)
        assert list(fn.argtypes) == [C.c_void_p, C.c_int, i3, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, i3, i3, C.c_void_p]
        assert fn.restype is C.c_int


def test_cli_rejects_mip_with_shape(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"),
                        "-c", str(tmp_path), "--region", ":,:,:", "--mip", "--shape", "8,8,8", "-o", str(tmp_path / "out.tif")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "resampled view" in r.stderr and "--mip" in r.stderr
    assert not os.listdir(str(tmp_path))
