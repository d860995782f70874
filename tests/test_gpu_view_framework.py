"""View decode of stored artefacts: NFGR.decompress_view and decompress.py --view against the existing decodes of the same artefact
(decompress_mip's images, planes of decompress_region), Decompress.postprocess included, for a plain and a 12-bit quantised artefact.
Every comparison is bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, quantize
from brief_pytorch_amd.framework import NFGR, MyLogger
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, STEPS = (24, 28, 32), 2000      # (2000 steps: before that the decode of these nets is one grey level, tests/test_gpu_mip.py)
AXIS_DIR = {0: (1, 0, 0), 1: (0, -1, 0), 2: (0, 0, 1)}      # the orientations of mip_ops' three images (view.frame)
REGION, REGION_SL = "3:20,5:23,1:30", (slice(3, 20), slice(5, 23), slice(1, 30))


def _fit(tmp_path, quant=None):
    vol = make_volume(SHAPE, seed=11)
    assert vol.dtype == np.uint16
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    cf = opt.CompressFramework
    cf.Compress.max_steps = STEPS
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = 12000.0
    cf.Compress.loss_log_freq = STEPS
    if quant is not None:
        cf.Compress.quantize = config.to_opt(quant)
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp_path / "outputs")
    opt.Log.time = False
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    NFGR(cf, Log=Log).compress(path)
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    return opt, os.path.join(Log.logdir, "steps%d" % STEPS, "compressed"), yml


@pytest.fixture(scope="module")
def artefact(tmp_path_factory):
    return _fit(tmp_path_factory.mktemp("view_single"))


def _with_postprocess(opt, whole):
    """a threshold and a narrowing clip inside the decode's own range"""
    o2 = config.to_opt(config.to_plain(opt))
    pp = o2.CompressFramework.Decompress.postprocess
    vmin, span = int(whole.min()), int(whole.max()) - int(whole.min())
    lo, level, hi = vmin + span // 8, vmin + span // 4, vmin + span // 2
    assert span >= 64 and 0 < lo < level < hi < whole.max(), "the fit is too short for a decode with structure"
    pp.denoise.level, pp.denoise.close, pp.clip = level, False, [lo, hi]
    return o2


def _check(opt, cdir):
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    whole = NFGR.decompress(opt, mod, side)
    assert whole.dtype == np.uint16 and whole.shape == SHAPE + (1,)
    centre = [(n - 1) / 2 for n in SHAPE]
    for o in (opt, _with_postprocess(opt, whole)):
        for region, sl in ((None, (slice(None),) * 3), (REGION, REGION_SL)):
            mips = NFGR.decompress_mip(o, mod, side, region)
            box = NFGR.decompress_region(o, mod, side, region if region is not None else ":,:,:")
            for a in range(3):
                img, hits, stats = NFGR.decompress_view(o, mod, side, AXIS_DIR[a], mode="max", region=region, return_hits=True)
                assert img.dtype == np.uint16 and np.array_equal(img, mips[a]), (region, a)
                assert (hits == box.shape[a]).all() and stats["samples_evaluated"] == box.size
                lo_img = NFGR.decompress_view(o, mod, side, AXIS_DIR[a], mode="min", region=region)
                assert np.array_equal(lo_img, box.min(a)), (region, a)
                plane = (sl[a].start or 0) + 2
                off = (plane - centre[a]) * (-1 if a == 1 else 1)
                img = NFGR.decompress_view(o, mod, side, AXIS_DIR[a], mode="slice", region=region, offset=off)
                assert np.array_equal(img, box.take(plane - (sl[a].start or 0), axis=a)), (region, a, plane)
    # a mean over the whole depth of an axis-aligned view is the mean of the voxels, in the stated rounding
    mean = NFGR.decompress_view(opt, mod, side, AXIS_DIR[0], mode="mean")
    assert mean.dtype == np.float32
    assert np.array_equal(mean, (whole.astype(np.int64).sum(0).astype(np.float64) / SHAPE[0]).astype(np.float32))
    return whole


def test_views_of_a_fitted_artefact_equal_its_projections_and_planes(artefact):
    opt, cdir, _ = artefact
    _check(opt, cdir)


def test_quantised_artefact_renders_the_same_way(tmp_path):
    opt, cdir, _ = _fit(tmp_path, {"bits": 12, "finetune_steps": 500})
    assert os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    assert config.load(os.path.join(cdir, "sideinfos.yaml"))["quantize"]["bits"] == 12
    _check(opt, cdir)


def _cli(yml, cdir, out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", out] + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "view" in r.stdout and "rays hit" in r.stdout
    return np.load(out) if out.endswith(".npy") else read_img(out)


def test_cli_writes_the_python_calls_pixels(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    geom = dict(up=(1, 0.2, 0), spacing=0.8, depth_spacing=0.5, voxel_size=(2, 1, 1), region=REGION)
    flags = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "0.8", "--view-depth-spacing", "0.5", "--voxel-size", "2,1,1"]
    want = NFGR.decompress_view(opt, mod, side, (0.48, -0.6, 0.64), mode="max", **geom)
    assert want.dtype == np.uint16 and len(np.unique(want)) > 20
    got = _cli(yml, cdir, str(tmp_path / "mip.tif"), *flags)
    assert np.array_equal(got.reshape(want.shape), want)
    want = NFGR.decompress_view(opt, mod, side, (0.48, -0.6, 0.64), mode="slice", offset=-2.5, size=(19, 33), **geom)
    got = _cli(yml, cdir, str(tmp_path / "slice.png"), "--view-mode", "slice", "--view-offset", "-2.5", "--view-size", "19,33", *flags)
    assert want.shape == (19, 33, 1) and np.array_equal(got.reshape(want.shape), want)
    want = NFGR.decompress_view(opt, mod, side, (0.48, -0.6, 0.64), mode="mean", **geom)
    got = _cli(yml, cdir, str(tmp_path / "mean.npy"), "--view-mode", "mean", *flags)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert sorted(os.listdir(str(tmp_path))) == ["mean.npy", "mip.tif", "slice.png"]
