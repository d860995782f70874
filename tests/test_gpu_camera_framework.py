"""Camera view of stored artefacts: NFGR.decompress_camera / decompress_camera_surface against view.render_rays / render_surface_rays
on the loaded net, decompress.py --view ... --view-eye ... against the Python calls, a 12-bit quantised artefact, and the refusals of
a DivideTask directory and an error-bounded artefact.  Every comparison is bitwise."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, quantize
from brief_pytorch_amd import view as VW
from brief_pytorch_amd.framework import NFGR, MyLogger, decompress_camera, decompress_camera_surface
from brief_pytorch_amd.io import load_yaml, save_yaml
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, STEPS = (24, 28, 32), 2000      # (the fit of tests/test_gpu_view_framework.py)
REGION = "3:20,5:23,1:30"
EYE, DIRECTION = (-14.0, 6.5, 47.0), (0.8, 0.2, -0.56)
GEOM = dict(up=(1, 0.2, 0), fov=35.0, size=(33, 41), depth_spacing=0.5, voxel_size=(2, 1, 1), region=REGION)
FLAGS = ["--view", "0.8,0.2,-0.56", "--view-eye=-14,6.5,47", "--view-up", "1,0.2,0", "--view-fov", "35", "--view-size", "33,41",
         "--view-depth-spacing", "0.5", "--voxel-size", "2,1,1"]


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
    return _fit(tmp_path_factory.mktemp("camera_single"))


def _level(opt, mod, side):
    """the median over the rays that meet the box of the per-ray maximum: about half of them hit"""
    img, hits, _ = NFGR.decompress_camera(opt, mod, side, EYE, DIRECTION, mode="max", return_hits=True, **GEOM)
    return int(np.median(img[..., 0][hits > 0]))


def _check(opt, cdir):
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    art = VW.open_single_camera(opt, mod, side)
    phi = art.load_phi("cuda")
    cam = VW.make_camera(art.dims, EYE, DIRECTION, **GEOM)
    args = (art.lo, art.hi, art.out_kind, art.norm_range, art.vrange)
    for mode in ("max", "min", "mean"):
        want, want_hits, want_stats = VW.render_rays(phi, cam, mode, *args)
        img, hits, stats = NFGR.decompress_camera(opt, mod, side, EYE, DIRECTION, mode=mode, return_hits=True, **GEOM)
        assert img.dtype == (np.float32 if mode == "mean" else np.uint16) and img.shape == (33, 41, 1)
        assert np.array_equal(img, want.cpu().numpy()) and np.array_equal(hits, want_hits.cpu().numpy()) and stats == want_stats, mode
        assert np.array_equal(decompress_camera(opt, mod, side, EYE, DIRECTION, mode=mode, **GEOM), img)
        assert 0 < stats["rays_hit"] < stats["rays"] and stats["samples_evaluated"] == stats["samples_inside"] >= 5000
        if mode == "max":
            assert len(np.unique(img)) > 20
    level = _level(opt, mod, side)
    from brief_pytorch_amd import gradient
    gscale = gradient.voxel_scale(art.dims, art.lo, art.hi, art.norm_range, art.vrange[0], art.vrange[1]) / np.array(GEOM["voxel_size"], np.float64)
    for fn in (NFGR.decompress_camera_surface, decompress_camera_surface):
        got = fn(opt, mod, side, EYE, DIRECTION, level, **GEOM)
        want = VW.render_surface_rays(phi, cam, level, *args, gscale=gscale)
        for key in ("first", "t_lo", "t_hi", "t", "distance", "position", "normal", "shade", "hits"):
            assert isinstance(got[key], np.ndarray) and np.array_equal(got[key].view(np.int32), want[key].cpu().numpy().view(np.int32)), key
        assert got["stats"] == want["stats"] and 0 < got["stats"]["rays_surface"] < got["stats"]["rays_hit"]
        assert got["stats"]["rays_surface"] > got["stats"]["rays_cut"] and got["shade"].max() > 0
    return level


def test_camera_views_of_a_fitted_artefact_equal_the_renderers_on_its_net(artefact):
    opt, cdir, _ = artefact
    _check(opt, cdir)


def test_postprocess_acts_on_the_image_as_for_the_orthographic_view(artefact):
    opt, cdir, _ = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    plain, hits, _ = NFGR.decompress_camera(opt, mod, side, EYE, DIRECTION, mode="max", return_hits=True, **GEOM)
    o2 = config.to_opt(config.to_plain(opt))
    pp = o2.CompressFramework.Decompress.postprocess
    vmin, span = int(plain[hits > 0].min()), int(plain.max()) - int(plain[hits > 0].min())
    lo, level, hi = vmin + span // 8, vmin + span // 4, vmin + span // 2
    assert span >= 64 and 0 < lo < level < hi < plain.max()
    pp.denoise.level, pp.denoise.close, pp.clip = level, False, [lo, hi]
    img = NFGR.decompress_camera(o2, mod, side, EYE, DIRECTION, mode="max", **GEOM)
    want = np.clip(np.where(plain <= level, 0, plain), lo, hi).astype(np.uint16)
    want[hits == 0] = 0
    assert np.array_equal(img, want) and len(np.unique(img)) > 5
    with pytest.raises(ValueError, match="mean view.*does not.*commute"):
        NFGR.decompress_camera(o2, mod, side, EYE, DIRECTION, mode="mean", **GEOM)


def test_quantised_artefact_renders_the_same_way(tmp_path):
    opt, cdir, _ = _fit(tmp_path, {"bits": 12, "finetune_steps": 500})
    assert os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    _check(opt, cdir)


def _cli(yml, cdir, out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", out] + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "camera" in r.stdout and "rays hit" in r.stdout
    return np.load(out) if out.endswith(".npy") else read_img(out)


def test_cli_writes_the_python_calls_arrays(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    want = NFGR.decompress_camera(opt, mod, side, EYE, DIRECTION, mode="min", near=20.0, far=45.0, **GEOM)
    got = _cli(yml, cdir, str(tmp_path / "min.tif"), "--view-mode", "min", "--view-near", "20", "--view-far", "45", *FLAGS)
    assert want.dtype == np.uint16 and np.array_equal(got.reshape(want.shape), want) and len(np.unique(want)) > 20
    level = _level(opt, mod, side)
    res = NFGR.decompress_camera_surface(opt, mod, side, EYE, DIRECTION, level, **GEOM)
    got = _cli(yml, cdir, str(tmp_path / "surface.npy"), "--view-surface", str(level), *FLAGS)
    want = np.concatenate([res["distance"][..., None], res["normal"], res["shade"][..., None]], axis=-1).astype(np.float32)
    assert got.shape == (33, 41, 5) and np.array_equal(got.view(np.int32), want.view(np.int32))
    got = _cli(yml, cdir, str(tmp_path / "surface.png"), "--view-surface", str(level), "--view-surface-side", "above", "--view-refine", "8", *FLAGS)
    assert np.array_equal(got.reshape(33, 41), np.floor(255.0 * res["shade"].astype(np.float64) + 0.5).astype(np.uint8))
    assert sorted(os.listdir(str(tmp_path))) == ["min.tif", "surface.npy", "surface.png"]


def test_divide_and_error_bounded_artefacts_are_refused_by_name(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    bounded = dict(load_yaml(side), error_bound=3)
    for call in (lambda s, m=mod: NFGR.decompress_camera(opt, m, s, EYE, DIRECTION, **GEOM),
                 lambda s, m=mod: NFGR.decompress_camera_surface(opt, m, s, EYE, DIRECTION, 1000, **GEOM)):
        with pytest.raises(ValueError, match="error-bounded.*error_bound 3"):
            call(bounded)
    # on disk: a copy of the artefact with the bound in its side info, and one with blocks beside the module
    copy = str(tmp_path / "bounded")
    shutil.copytree(cdir, copy)
    save_yaml(bounded, os.path.join(copy, "sideinfos.yaml"))
    divided = str(tmp_path / "divided")
    shutil.copytree(cdir, divided)
    os.makedirs(os.path.join(divided, "sideinfos"))
    with pytest.raises(ValueError, match="a camera view of a partition is a follow-up"):
        NFGR.decompress_camera(opt, os.path.join(divided, "module"), os.path.join(divided, "sideinfos.yaml"), EYE, DIRECTION, **GEOM)
    os.makedirs(str(tmp_path / "out"))
    for c, words in ((copy, "error-bounded"), (divided, "a camera view of a partition is a follow-up")):
        for extra in ([], ["--view-surface", "1000"]):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", c, "--region", REGION,
                                "-o", str(tmp_path / "out" / "view.npy")] + FLAGS + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode != 0 and "--view-eye" in r.stderr and words in r.stderr, r.stderr[-2000:]
    assert not os.listdir(str(tmp_path / "out"))
