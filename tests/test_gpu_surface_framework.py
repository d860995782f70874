"""Surface view of stored artefacts: NFGR.decompress_surface against view.render_surface on the loaded net, and decompress.py
--view-surface against the Python call's pixels, for a plain and a 12-bit quantised artefact.  Every comparison is bitwise."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, gradient, quantize
from brief_pytorch_amd import view as VW
from brief_pytorch_amd.framework import NFGR, MyLogger, _coords_range
from brief_pytorch_amd.io import load_yaml, minmaxany_range
from brief_pytorch_amd.mip import _load_phi
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, STEPS = (24, 28, 32), 2000      # (2000 steps: before that the decode of these nets is one grey level, tests/test_gpu_mip.py)
REGION = "3:20,5:23,1:30"
DIRECTION = (0.48, -0.6, 0.64)
GEOM = dict(up=(1, 0.2, 0), spacing=0.8, depth_spacing=0.5, voxel_size=(2, 1, 1), region=REGION)
FLAGS = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "0.8", "--view-depth-spacing", "0.5", "--voxel-size", "2,1,1"]
ARRAYS = ("first", "t_lo", "t_hi", "t", "position", "normal", "shade", "hits")


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
    return _fit(tmp_path_factory.mktemp("surface_single"))


def _levels(opt, cdir):
    """(above, below): the medians over the rays that meet the clip box of the per-ray maximum / minimum of the integer decode"""
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    o = config.to_opt(config.to_plain(opt))
    pp = o.CompressFramework.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 0, False, [0, 65535]       # the raw integer decode
    out = []
    for mode in ("max", "min"):
        img, hits, _ = NFGR.decompress_view(o, mod, side, DIRECTION, mode=mode, return_hits=True, **GEOM)
        out.append(int(np.median(img[..., 0][hits > 0])))
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_python_call(opt, cdir):
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    side = load_yaml(side_path)
    assert gradient.supported(side["phi_name"], str(side.get("phi_precision", "fp32")), side["phi_features"])
    above, below = _levels(opt, cdir)
    cf = copy.deepcopy(opt.CompressFramework)
    phi = _load_phi(cf, mod, side, "cuda")
    lo, hi = _coords_range(cf.Compress.coords_mode)
    rng = minmaxany_range(cf.Normalize.name)
    view = VW.make_view(SHAPE, DIRECTION, **GEOM)
    gscale = gradient.voxel_scale(SHAPE, lo, hi, rng, side["min"], side["max"]) / np.array(GEOM["voxel_size"], np.float64)
    results = {}
    for name, level, kw in (("above", above, {}), ("below", below, dict(side="below", refine=3)),
                            ("lit", above, dict(light=(0.0, 0.6, -0.8), refine=0)), ("plain", above, dict(shading=False))):
        res = NFGR.decompress_surface(opt, mod, side_path, DIRECTION, level, **GEOM, **kw)
        light = kw.get("light", VW.frame(DIRECTION, GEOM["up"])[2])
        want = VW.render_surface(phi, view, level, lo, hi, "u16", rng, (side["min"], side["max"]), gscale=gscale,
                                 **{**kw, "light": light})
        for key in ARRAYS:
            if want[key] is None:
                assert res[key] is None and name == "plain", (name, key)
            else:
                assert _same(res[key], want[key].cpu().numpy()), (name, key)
        assert res["stats"] == want["stats"]
        assert _same(res["depth"], res["t"] * np.float32(GEOM["depth_spacing"]))
        hit = res["first"] >= 0
        assert np.isnan(res["depth"][~hit]).all() and np.isfinite(res["depth"][hit]).all()
        stats = res["stats"]
        share = stats["rays_surface"] / stats["rays_hit"]
        print("%s: level %d, %.3f of the rays that meet the box hit, %d cut" % (name, level, share, stats["rays_cut"]))
        if name != "below":         # (the level is the median of the per-ray maximum: what keeps these comparisons from being vacuous)
            assert 0.25 <= share <= 0.75 and stats["rays_surface"] - stats["rays_cut"] >= 0.25 * stats["rays_surface"]
        assert stats["rays_surface"] > stats["rays_cut"] > 0
        results[name] = res
    assert results["above"]["shade"].max() > 0.5 and len(np.unique(results["above"]["shade"])) > 50
    assert _same(results["plain"]["t"], results["above"]["t"])
    return above, below, results


def test_the_python_call_equals_render_surface_on_the_loaded_net(artefact):
    opt, cdir, _ = artefact
    _check_python_call(opt, cdir)


def test_quantised_artefact_renders_through_the_same_call(tmp_path):
    opt, cdir, _ = _fit(tmp_path, {"bits": 12, "finetune_steps": 500})
    assert os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    assert config.load(os.path.join(cdir, "sideinfos.yaml"))["quantize"]["bits"] == 12
    _check_python_call(opt, cdir)


def _cli(yml, cdir, out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", out] + FLAGS + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "surface view" in r.stdout and "rays hit the surface" in r.stdout
    return (np.load(out) if out.endswith(".npy") else read_img(out)), r.stdout


def _pack(res):
    return np.concatenate([res["depth"][..., None], res["normal"], res["shade"][..., None]], axis=-1).astype(np.float32)


def test_cli_writes_the_python_calls_pixels(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    above, below = _levels(opt, cdir)
    want = NFGR.decompress_surface(opt, mod, side, DIRECTION, above, **GEOM)
    got, _ = _cli(yml, cdir, str(tmp_path / "surface.npy"), "--view-surface", str(above))
    assert got.dtype == np.float32 and got.shape == want["shade"].shape + (5,) and _same(got, _pack(want))
    got, _ = _cli(yml, cdir, str(tmp_path / "surface.png"), "--view-surface", str(above))
    image = np.floor(255.0 * want["shade"].astype(np.float64) + 0.5).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got.reshape(image.shape), image) and len(np.unique(image)) > 50
    # --view-refine 0 and --view-surface-side below reach the kernels; so do the channel and the light
    want = NFGR.decompress_surface(opt, mod, side, DIRECTION, below, side="below", refine=0, light=(0.0, 0.6, -0.8), **GEOM)
    got, text = _cli(yml, cdir, str(tmp_path / "below.npy"), "--view-surface", str(below), "--view-surface-side", "below", "--view-refine", "0",
                     "--view-channel", "0", "--view-light", "0,0.6,-0.8")
    assert _same(got, _pack(want)) and "0 refinement points" in text and "below" in text
    hit = want["first"] >= 0
    assert np.array_equal(want["t"][hit], want["first"][hit].astype(np.float32))
    refined = NFGR.decompress_surface(opt, mod, side, DIRECTION, below, side="below", **GEOM)
    assert not _same(refined["t"], want["t"]) and np.array_equal(refined["first"], want["first"])
    got, _ = _cli(yml, cdir, str(tmp_path / "below.tif"), "--view-surface", str(below), "--view-surface-side", "below")
    image = np.floor(255.0 * refined["shade"].astype(np.float64) + 0.5).astype(np.uint8)
    assert np.array_equal(got.reshape(image.shape), image)
    assert sorted(os.listdir(str(tmp_path))) == ["below.npy", "below.tif", "surface.npy", "surface.png"]
    # a channel the artefact does not have is refused by name, and nothing is written
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", str(tmp_path / "c1.npy")]
                       + FLAGS + ["--view-surface", str(above), "--view-channel", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--view-surface" in r.stderr and "channel 1 does not exist" in r.stderr
    assert not os.path.exists(str(tmp_path / "c1.npy"))
