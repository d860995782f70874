"""View decode of a stored DivideTask artefact: decompress_divide_view and decompress.py --view ... --view-owner nearest against the
existing decodes of the same artefact (decompress_divide_mip's images, planes of decompress_divide_region), Decompress.postprocess
included, and an oblique mean against the restatement.  A fitted `total_2_2_2` artefact of a 32 x 48 x 64 volume, the recipe of
tests/test_gpu_mip.py.  Every comparison is bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import artefact, config
from brief_pytorch_amd import view as VW
from brief_pytorch_amd.framework import NFGR, MyLogger, decompress_divide_mip, decompress_divide_region, decompress_divide_view
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img
from tests.test_gpu_view import _fold
from tests.test_gpu_view_partition import _restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, STEPS = (32, 48, 64), 2000      # (2000 steps: before that the decode of these nets is one grey level, tests/test_gpu_mip.py)
AXIS_DIR = {0: (1, 0, 0), 1: (0, -1, 0), 2: (0, 0, 1)}      # +z, -y, +x: the orientations of mip_ops' three images (view.frame)
OBLIQUE = dict(up=(1, 0.2, 0), spacing=0.8, depth_spacing=0.5, voxel_size=(2, 1, 1))
DIRECTION = (0.48, -0.6, 0.64)


@pytest.fixture(scope="module")
def divided(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("view_divide")
    vol = make_volume(SHAPE, seed=7)
    path = str(tmp_path / "d.tif")
    save_img(path, vol)
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    cf = opt.CompressFramework
    cf.Compress.max_steps = STEPS
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = 40000.0
    cf.Compress.loss_log_freq = STEPS
    cf.Compress.divide.divide_type = "total_2_2_2"
    cf.Compress.divide.param_alloc = "by_size"
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp_path / "outputs")
    opt.Log.time = False
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    fw.compress_divide(path, opt)
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    cdir = os.path.join(Log.logdir, "steps%d" % STEPS, "compressed")
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    assert len(os.listdir(args[1])) == 8
    return fw, opt, cdir, yml, args


def _with_postprocess(opt, whole):
    """a threshold and a narrowing clip inside the decode's own range"""
    o2 = config.to_opt(config.to_plain(opt))
    pp = o2.CompressFramework.Decompress.postprocess
    vmin, span = int(whole.min()), int(whole.max()) - int(whole.min())
    lo, level, hi = vmin + span // 8, vmin + span // 4, vmin + span // 2
    assert span >= 64 and 0 < lo < level < hi < whole.max(), "the fit is too short for a decode with structure"
    pp.denoise.level, pp.denoise.close, pp.clip = level, False, [lo, hi]
    return o2


def test_axis_aligned_views_equal_the_projections_and_planes(divided):
    fw, opt, _, _, args = divided
    whole = decompress_divide_region(opt, *args, ":,:,:")
    assert whole.dtype == np.uint16 and whole.shape == SHAPE + (1,)
    centre = [(n - 1) / 2 for n in SHAPE]
    for o in (opt, _with_postprocess(opt, whole)):
        for region, sl in ((None, (slice(None),) * 3), ("5:30,10:40,7:60", (slice(5, 30), slice(10, 40), slice(7, 60))),
                           ("0:16,0:24,0:32", (slice(0, 16), slice(0, 24), slice(0, 32)))):
            mips = decompress_divide_mip(o, *args, region)
            box = decompress_divide_region(o, *args, region if region is not None else ":,:,:")
            for a in range(3):
                img, hits, stats = decompress_divide_view(o, *args, AXIS_DIR[a], mode="max", region=region, return_hits=True)
                assert img.dtype == np.uint16 and np.array_equal(img, mips[a]), (region, a)
                assert (hits == box.shape[a]).all() and stats["samples_evaluated"] == box.size
                assert stats["blocks"] == 8 and stats["blocks_hit"] == (1 if region == "0:16,0:24,0:32" else 8)
                for plane in {(sl[a].start or 0) + 2, SHAPE[a] // 2 - 1, SHAPE[a] // 2} - ({SHAPE[a] // 2} if region == "0:16,0:24,0:32" else set()):
                    off = (plane - centre[a]) * (-1 if a == 1 else 1)
                    img = decompress_divide_view(o, *args, AXIS_DIR[a], mode="slice", region=region, offset=off)
                    assert np.array_equal(img, box.take(plane - (sl[a].start or 0), axis=a)), (region, a, plane)
    # the method of an NFGR: its own options and device
    img = fw.decompress_divide_view(*args, AXIS_DIR[2], opt=opt)
    assert np.array_equal(img, decompress_divide_mip(opt, *args)[2])


def test_oblique_mean_equals_the_restatement(divided):
    _, opt, _, _, args = divided
    data_shape, blocks = artefact.divide_blocks(*args)
    parts = []
    for b in blocks:
        art = artefact.open_artefact(opt, b.module_path, b.side)
        parts.append((art.load_phi("cuda"), [b.ranges[a][0] for a in "dhw"], art.dims, art.lo, art.hi, art.norm_range, art.vrange))
    assert len({p[6] for p in parts}) > 1, "every block has the same value range: the per-block epilogue is not exercised"
    view = VW.make_view(data_shape[:-1], DIRECTION, region="3:29,5:43,1:60", **OBLIQUE)
    vals, evaluated, facts = _restate(parts, view, "u16")
    assert facts["crossed"] >= 3
    for mode in ("mean", "max"):
        want, want_hits = _fold(vals, evaluated, mode, np.uint16)
        img, hits, stats = decompress_divide_view(opt, *args, DIRECTION, mode=mode, region="3:29,5:43,1:60", return_hits=True, **OBLIQUE)
        assert np.array_equal(hits, want_hits) and stats["samples_evaluated"] == int(evaluated.sum()) > 10000
        assert img.dtype == want.dtype and np.array_equal(img.astype(np.float64), want.astype(np.float64)), mode


def _cli(yml, cdir, out, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", "3:29,5:43,1:60", "-o", out] + list(extra),
                          capture_output=True, text=True, timeout=300)


def test_cli_writes_the_python_calls_pixels_and_refuses_without_the_option(divided, tmp_path):
    _, opt, cdir, yml, args = divided
    flags = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "0.8", "--view-depth-spacing", "0.5", "--voxel-size", "2,1,1"]
    r = _cli(yml, cdir, str(tmp_path / "no.tif"), *flags)
    assert r.returncode != 0 and "DivideTask" in r.stderr and "--view-owner nearest" in r.stderr
    want = decompress_divide_view(opt, *args, DIRECTION, mode="max", region="3:29,5:43,1:60", **OBLIQUE)
    assert want.dtype == np.uint16 and len(np.unique(want)) > 20
    r = _cli(yml, cdir, str(tmp_path / "mip.tif"), "--view-owner", "nearest", *flags)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DivideTask" in r.stdout and "8 of 8 blocks hit" in r.stdout and "rays hit" in r.stdout
    assert np.array_equal(read_img(str(tmp_path / "mip.tif")).reshape(want.shape), want)
    want = decompress_divide_view(opt, *args, DIRECTION, mode="slice", offset=-2.5, size=(19, 33), region="3:29,5:43,1:60", **OBLIQUE)
    r = _cli(yml, cdir, str(tmp_path / "slice.npy"), "--view-owner", "nearest", "--view-mode", "slice", "--view-offset", "-2.5", "--view-size", "19,33", *flags)
    assert r.returncode == 0, r.stderr[-2000:]
    assert want.shape == (19, 33, 1) and np.array_equal(np.load(str(tmp_path / "slice.npy")), want)
    assert sorted(os.listdir(str(tmp_path))) == ["mip.tif", "slice.npy"]
