"""The artefact reader on the host (brief_pytorch_amd/artefact.py): what open_artefact makes of option and side-info dicts, that it
touches nothing under the module path, and the DivideTask block walker against a directory tree and a brute-force index comparison.
No GPU and no library."""
import copy
import os

import numpy as np
import pytest
import yaml

from brief_pytorch_amd import artefact, config
from brief_pytorch_amd import region as region_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt():
    return config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))


def _side(**kw):
    side = {"dtype": "uint16", "min": 3.0, "max": 60000.0, "data_shape": [8, 9, 10, 2], "phi_features": 22, "phi_name": "SIREN"}
    side.update(kw)
    return side


def test_every_field_of_a_uint16_minmaxany_artefact(tmp_path):
    opt, side, mod = _opt(), _side(), str(tmp_path / "module")
    art = artefact.open_artefact(opt, mod, side)
    assert art.side is side and art.module_path == mod
    assert art.data_shape == [8, 9, 10, 2] and art.dims == [8, 9, 10] and art.cout == 2 and art.dtype == "uint16"
    assert (art.phi_name, art.phi_features, art.precision) == ("SIREN", 22, "fp32")
    assert (art.lo, art.hi) == (-1.0, 1.0) and art.norm_range == (0.0, 100.0) and art.vrange == (3.0, 60000.0)
    assert art.integer is True and art.out_kind == "u16"
    assert art.postprocess == opt.CompressFramework.Decompress.postprocess
    # the private copy is patched to the stored net; the caller's tree is not
    assert art.cf is not opt.CompressFramework and art.cf.Module.phi.features == 22 and art.cf.Module.phi.name == "SIREN"
    assert artefact.open_artefact(opt, mod, _side(dtype="uint8")).out_kind == "u8"
    o = _opt()
    o.CompressFramework.Compress.coords_mode = "0p1"
    assert (lambda a: (a.lo, a.hi))(artefact.open_artefact(o, mod, side)) == (0.0, 1.0)


def test_not_integer_for_float_data_and_for_other_normalisations():
    art = artefact.open_artefact(_opt(), "module", _side(dtype="float32"))
    assert art.integer is False and art.out_kind is None and art.norm_range == (0.0, 100.0)
    o = _opt()
    o.CompressFramework.Normalize.name = "minmax01"
    art = artefact.open_artefact(o, "module", _side())
    assert art.integer is False and art.out_kind is None and art.norm_range is None


def test_precision_precedence():
    """side info over default_precision over Compress.precision over fp32"""
    plain, bf16 = _opt(), _opt()
    bf16.CompressFramework.Compress.precision = "bf16"
    for opt, side_kw, kw, want in (
            (plain, {}, {}, "fp32"),
            (bf16, {}, {}, "bf16"),
            (bf16, {"phi_precision": "bf16x3"}, {}, "bf16x3"),
            (plain, {}, {"default_precision": "bf16"}, "bf16"),
            (bf16, {}, {"default_precision": "fp32"}, "fp32"),
            (bf16, {"phi_precision": "bf16x3"}, {"default_precision": "fp32"}, "bf16x3")):
        assert artefact.open_artefact(opt, "module", _side(**side_kw), **kw).precision == want, (side_kw, kw)


def test_missing_phi_name():
    side = _side()
    del side["phi_name"]
    with pytest.raises(KeyError, match="phi_name"):
        artefact.open_artefact(_opt(), "module", side)
    art = artefact.open_artefact(_opt(), "module", side, default_name="SIRENFT")
    assert art.phi_name == "SIRENFT" and art.cf.Module.phi.name == "SIRENFT"
    assert artefact.open_artefact(_opt(), "module", _side(phi_name="NeRF"), default_name="SIRENFT").phi_name == "NeRF"


def test_option_forms_are_equal_and_the_callers_trees_are_left_alone(tmp_path):
    opt, side = _opt(), _side(phi_precision="bf16")
    opt_before, side_before = copy.deepcopy(opt), copy.deepcopy(side)
    whole = artefact.open_artefact(opt, "module", side)
    bare = artefact.open_artefact(opt.CompressFramework, "module", side)
    assert whole == bare and whole != artefact.open_artefact(opt, "elsewhere", side)
    yml, side_yml = str(tmp_path / "run.yaml"), str(tmp_path / "sideinfos.yaml")
    config.save(opt, yml)
    with open(side_yml, "w") as f:
        yaml.safe_dump(side, f)
    assert artefact.open_artefact(yml, "module", side_yml) == whole
    assert opt == opt_before and side == side_before
    assert "features" not in opt.CompressFramework.Module.phi


def test_opening_needs_no_module_directory(tmp_path):
    from brief_pytorch_amd.corrections import CorrectionsError
    mod = str(tmp_path / "nowhere" / "module")
    art = artefact.open_artefact(_opt(), mod, _side(data_shape=[8, 9, 10, 1], error_bound=3))
    assert not os.path.exists(os.path.dirname(mod)) and art.integer
    with pytest.raises(CorrectionsError, match="missing"):
        art.corrections()
    assert artefact.open_artefact(_opt(), mod, _side()).corrections() is None
    with pytest.raises(OSError):
        art.load_phi("cpu")
    assert not os.listdir(str(tmp_path))


def test_check_envelope_checks_what_it_is_given_in_its_order():
    art = artefact.open_artefact(_opt(), "module", _side(dtype="float32", data_shape=[1, 9, 1], error_bound=3))
    artefact.check_envelope(art)
    with pytest.raises(ValueError, match="^bound 3 on \\[1, 9\\]$"):
        artefact.check_envelope(art, no_error_bound="bound %s on %s", need_3d="%d-D %s", need_integer="holds %s")
    with pytest.raises(ValueError, match="^2-D \\[1, 9, 1\\]$"):
        artefact.check_envelope(art, need_3d="%d-D %s", need_integer="holds %s")
    with pytest.raises(ValueError, match="^holds float32$"):
        artefact.check_envelope(art, need_integer="holds %s", min_axis=(2, "short %s"))
    with pytest.raises(ValueError, match="^short \\[1, 9\\]$"):
        artefact.check_envelope(art, need_minmaxany="not %s", min_axis=(2, "short %s"))
    o = _opt()
    o.CompressFramework.Normalize.name = "minmax01"
    o.CompressFramework.Decompress.postprocess.denoise.level = 500
    art = artefact.open_artefact(o, "module", _side())
    with pytest.raises(ValueError, match="^not minmax01$"):
        artefact.check_envelope(art, need_minmaxany="not %s", local_postprocess=True)
    with pytest.raises(ValueError, match="not local to a voxel"):
        artefact.check_envelope(art, local_postprocess=True)


# ---- the block walker --------------------------------------------------------------------------------------------------------------
def _tree(tmp_path, names, dtypes=None):
    for i, n in enumerate(names):
        os.makedirs(str(tmp_path / "module" / n))
        os.makedirs(str(tmp_path / "sideinfos" / n))
        with open(str(tmp_path / "sideinfos" / n / "sideinfos.yaml"), "w") as f:
            yaml.safe_dump(_side(dtype=(dtypes or ["uint16"] * len(names))[i], min=float(i)), f)
    os.makedirs(str(tmp_path / "module"), exist_ok=True)
    return str(tmp_path / "module"), str(tmp_path / "sideinfos")


def test_blocks_come_in_sorted_order_with_their_ranges_and_paths(tmp_path):
    names = ["d_4_7-h_0_7-w_0_7", "d_0_3-h_0_7-w_0_7", "d_10_11-h_0_7-w_0_7"]
    mdir, sdir = _tree(tmp_path, names)
    shape, blocks = artefact.divide_blocks({"data_shape": [12, 8, 8, 1]}, mdir, sdir, one_dtype="the projection decode")
    assert shape == [12, 8, 8, 1]
    assert [b.name for b in blocks] == sorted(names) == ["d_0_3-h_0_7-w_0_7", "d_10_11-h_0_7-w_0_7", "d_4_7-h_0_7-w_0_7"]
    assert [b.ranges for b in blocks] == [{"d": [0, 3], "h": [0, 7], "w": [0, 7]}, {"d": [10, 11], "h": [0, 7], "w": [0, 7]},
                                          {"d": [4, 7], "h": [0, 7], "w": [0, 7]}]
    assert [b.side["min"] for b in blocks] == [1.0, 2.0, 0.0]
    assert blocks[0].module_path == os.path.join(mdir, "d_0_3-h_0_7-w_0_7", "module")
    assert artefact.block_paths(mdir, sdir, "x") == (os.path.join(mdir, "x", "module"), os.path.join(sdir, "x", "sideinfos.yaml"))
    # the job's side info may be a path
    with open(str(tmp_path / "sideinfos.yaml"), "w") as f:
        yaml.safe_dump({"data_shape": [12, 8, 8, 1], "chunks_numbers": 3}, f)
    assert artefact.divide_blocks(str(tmp_path / "sideinfos.yaml"), mdir, sdir) == (shape, blocks)


def test_no_blocks_and_mixed_dtypes_are_refused(tmp_path):
    mdir, sdir = _tree(tmp_path / "empty", [])
    with pytest.raises(ValueError, match="no blocks under .*module"):
        artefact.divide_blocks({"data_shape": [8, 8, 8, 1]}, mdir, sdir)
    names = ["d_0_3-h_0_7-w_0_7", "d_4_7-h_0_7-w_0_7"]
    mdir, sdir = _tree(tmp_path / "mixed", names, ["uint16", "uint8"])
    with pytest.raises(ValueError, match="the projection decode needs one dtype for all blocks \\(d_0_3-h_0_7-w_0_7 is uint16, d_4_7-h_0_7-w_0_7 is uint8\\)"):
        artefact.divide_blocks({"data_shape": [8, 8, 8, 1]}, mdir, sdir, one_dtype="the projection decode")
    assert len(artefact.divide_blocks({"data_shape": [8, 8, 8, 1]}, mdir, sdir)[1]) == 2      # only where the decode needs it


def _blocks(names):
    from brief_pytorch_amd.misc import parse_chunk_name
    return [artefact.Block(n, {}, parse_chunk_name(n), n) for n in names]


def test_first_overlap_in_two_and_three_dimensions():
    touching3 = _blocks(["d_0_3-h_0_7-w_0_7", "d_4_7-h_0_3-w_0_7", "d_4_7-h_4_7-w_0_7"])
    assert artefact.first_overlap(touching3, "dhw") is None
    over3 = _blocks(["d_0_3-h_0_7-w_0_7", "d_4_7-h_0_4-w_0_7", "d_4_7-h_4_7-w_0_7"])      # h 0..4 and 4..7 share row 4
    assert [b.name for b in artefact.first_overlap(over3, "dhw")] == [over3[1].name, over3[2].name]
    touching2 = _blocks(["h_0_3-w_0_7", "h_4_7-w_0_3", "h_4_7-w_4_7"])
    assert artefact.first_overlap(touching2, "hw") is None
    over2 = _blocks(["h_0_4-w_0_7", "h_4_7-w_0_3", "h_4_7-w_4_7"])
    assert [b.name for b in artefact.first_overlap(over2, "hw")] == [over2[0].name, over2[1].name]
    # overlapping on some axes only is no overlap
    assert artefact.first_overlap(_blocks(["d_0_5-h_0_3-w_0_7", "d_2_7-h_4_7-w_0_7"]), "dhw") is None


@pytest.mark.parametrize("dims,names,region,meets", [
    # a strided region that straddles the block face at z 4|5, and the face at y 5|6
    ([9, 10, 11], ["d_0_4-h_0_5-w_0_10", "d_0_4-h_6_9-w_0_10", "d_5_8-h_0_9-w_0_10"], (slice(1, 9, 2), slice(2, 10, 3), slice(0, 11, 2)), [0, 1, 2]),
    # one that misses the last block entirely
    ([9, 10, 11], ["d_0_4-h_0_5-w_0_10", "d_0_4-h_6_9-w_0_10", "d_5_8-h_0_9-w_0_10"], (slice(0, 5, 3), slice(0, 10), slice(3, 4)), [0, 1]),
    # a stride that steps over a whole block, 2-D
    ([12, 7], ["h_0_4-w_0_6", "h_5_6-w_0_6", "h_7_11-w_0_6"], (slice(3, 12, 5), slice(1, 7, 2)), [0, 2]),
])
def test_meeting_against_a_brute_force_index_comparison(dims, names, region, meets):
    blocks = _blocks(names)
    axes = "dhw"[-len(dims):]
    start, stop, step = region_mod.normalize_region(dims, region)
    ext = region_mod.extents(start, stop, step)
    owner = -np.ones(dims, np.int64)                     # which block holds a voxel, and its flat index inside that block
    local = -np.ones(dims, np.int64)
    for i, b in enumerate(blocks):
        sl = tuple(slice(b.ranges[a][0], b.ranges[a][1] + 1) for a in axes)
        owner[sl] = i
        local[sl] = np.arange(owner[sl].size).reshape(owner[sl].shape)
    want_owner, want_local = owner[region], local[region]
    got_owner, got_local = -np.ones(ext, np.int64), -np.ones(ext, np.int64)
    met = []
    for b, o_lo, o_hi, l_start, l_stop in artefact.meeting(blocks, start, step, ext):
        i = names.index(b.name)
        met.append(i)
        shape = [b.ranges[a][1] - b.ranges[a][0] + 1 for a in axes]
        inside = np.arange(int(np.prod(shape))).reshape(shape)[tuple(slice(lo, hi, s) for lo, hi, s in zip(l_start, l_stop, step))]
        out = tuple(slice(lo, hi) for lo, hi in zip(o_lo, o_hi))
        assert (got_owner[out] == -1).all()
        got_owner[out], got_local[out] = i, inside
    assert np.array_equal(got_owner, want_owner) and np.array_equal(got_local, want_local)
    assert met == meets == sorted(set(want_owner.ravel().tolist()))       # in block order, and no block that the region misses
