"""Composite view of a stored DivideTask artefact, end to end: NFGR(...).decompress_divide_composite, framework.decompress_divide_composite
and decompress.py --view-composite ... --view-owner nearest give one image, and it is composite.render_composite_partition on the
loaded blocks.  A fitted `total_2_1_1` artefact (two blocks) of a 24 x 28 x 32 volume, the recipe of
tests/test_gpu_view_partition_framework.py.  Every comparison is bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import artefact, config
from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import view as VW
from brief_pytorch_amd.framework import NFGR, MyLogger, decompress_divide_composite, decompress_divide_region
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, STEPS = (24, 28, 32), 2000      # (2000 steps: before that the decode of these nets is one grey level, tests/test_gpu_mip.py)
REGION = "3:20,5:23,1:30"
DIRECTION = (0.48, -0.6, 0.64)
GEOM = dict(up=(1, 0.2, 0), spacing=2.4, depth_spacing=1.6, voxel_size=(2, 1, 1), region=REGION)
FLAGS = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "2.4", "--view-depth-spacing", "1.6", "--voxel-size", "2,1,1"]
BG = (10, 40, 90)


@pytest.fixture(scope="module")
def divided(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("composite_divide")
    vol = make_volume(SHAPE, seed=11)
    path = str(tmp_path / "d.tif")
    save_img(path, vol)
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    cf = opt.CompressFramework
    cf.Compress.max_steps = STEPS
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = 16000.0
    cf.Compress.loss_log_freq = STEPS
    cf.Compress.divide.divide_type = "total_2_1_1"
    cf.Compress.divide.param_alloc = "by_size"
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    pp = cf.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 0, False, [0, 65535]       # the identity: a composite refuses anything else
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
    assert len(os.listdir(args[1])) == 2
    whole = decompress_divide_region(opt, *args, ":,:,:")
    vmin, span = int(whole.min()), int(whole.max()) - int(whole.min())
    assert whole.dtype == np.uint16 and span >= 64, "the fit is too short for a decode with structure"
    # nothing in the decode's lowest quarter, a warm haze up to the middle, dense and white from three quarters on
    text = "%d:255,120,0,0;%d:255,160,40,0.1;%d:255,255,255,0.6" % (vmin + span // 4, vmin + span // 2, vmin + 3 * span // 4)
    return fw, opt, cdir, yml, args, text


def test_method_function_and_render_composite_partition_agree(divided):
    fw, opt, _, _, args, text = divided
    data_shape, blocks = artefact.divide_blocks(*args)
    parts = []
    for b in blocks:
        art = artefact.open_artefact(opt, b.module_path, b.side)
        parts.append((art.load_phi("cuda"), [b.ranges[a][0] for a in "dhw"], art.dims, art.lo, art.hi, art.norm_range, art.vrange))
    view = VW.make_view(data_shape[:-1], DIRECTION, **GEOM)
    for kw in ({}, dict(background=BG, bits=9, chunk=501)):
        img, hits, stats = decompress_divide_composite(opt, *args, DIRECTION, text, return_hits=True, **GEOM, **kw)
        tf = CP.make_transfer(CP.parse_transfer(text), "u16", GEOM["depth_spacing"], kw.get("bits"))
        want, want_hits, want_stats = CP.render_composite_partition(parts, view, tf, "u16", background=kw.get("background", (0, 0, 0)))
        assert img.dtype == np.uint8 and img.shape == (view.rows, view.cols, 4) and np.array_equal(img, want.cpu().numpy())
        assert np.array_equal(hits, want_hits.cpu().numpy()) and stats == want_stats
        assert np.array_equal(fw.decompress_divide_composite(*args, DIRECTION, text, opt=opt, **GEOM, **kw), img)
        # not vacuous: both blocks seen, some of the rear block's samples behind a haze, rays that miss and show the background
        alpha = img[..., 3]
        print("%s: %s; A == 0 on %d of the hit rays, 20 < A < 235 on %d, A >= 250 on %d" % (
            text, stats, (alpha[hits > 0] == 0).sum(), ((alpha > 20) & (alpha < 235)).sum(), (alpha >= 250).sum()))
        assert stats["blocks"] == stats["blocks_hit"] == 2 and stats["segments"] > stats["rays_hit"]
        assert 0 < stats["samples_second_pass"] < stats["samples_inside"]
        assert ((alpha > 20) & (alpha < 235)).sum() >= 10 and (alpha >= 250).any()
        assert (hits == 0).any() and (img[hits == 0] == np.array(tuple(kw.get("background", (0, 0, 0))) + (0,), np.uint8)).all()
        assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) >= 30


def _cli(yml, cdir, out, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", out] + FLAGS + list(extra),
                          capture_output=True, text=True, timeout=300)


def test_cli_writes_the_python_calls_pixels_and_refuses_without_the_option(divided, tmp_path):
    fw, opt, cdir, yml, args, text = divided
    r = _cli(yml, cdir, str(tmp_path / "no.png"), "--view-composite", text)
    assert r.returncode != 0 and "--view-composite: a composite view of a DivideTask artefact" in r.stderr and "--view-owner nearest" in r.stderr
    want = decompress_divide_composite(opt, *args, DIRECTION, text, background=BG, **GEOM)
    assert np.array_equal(want, fw.decompress_divide_composite(*args, DIRECTION, text, opt=opt, background=BG, **GEOM))
    for out in ("c.npy", "c.png"):
        r = _cli(yml, cdir, str(tmp_path / out), "--view-composite", text, "--view-owner", "nearest", "--view-background", "%d,%d,%d" % BG)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "DivideTask (2 of 2 blocks hit, owner nearest" in r.stdout and "composite view" in r.stdout and "rays hit" in r.stdout
    got = np.load(str(tmp_path / "c.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    png = read_img(str(tmp_path / "c.png"))                        # cv2's order: B, G, R
    assert png.dtype == np.uint8 and np.array_equal(png[..., ::-1], want[..., :3]) and not np.array_equal(png, want[..., :3])
    assert sorted(os.listdir(str(tmp_path))) == ["c.npy", "c.png"]
