"""Composite view of stored artefacts: NFGR.decompress_composite against composite.render_composite on the loaded net, and decompress.py
--view-composite against the Python call's pixels, for a plain and a 12-bit quantised artefact; the refusals of the artefact kinds the
composite does not serve.  Every comparison is bitwise."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import composite as CP
from brief_pytorch_amd import config, quantize
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
GEOM = dict(up=(1, 0.2, 0), spacing=2.4, depth_spacing=1.6, voxel_size=(2, 1, 1), region=REGION)
FLAGS = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "2.4", "--view-depth-spacing", "1.6", "--voxel-size", "2,1,1"]
BG = (10, 40, 90)


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
    pp = cf.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 0, False, [0, 65535]       # the identity: a composite refuses anything else
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
    return _fit(tmp_path_factory.mktemp("composite_single"))


def _transfer(opt, cdir):
    """a transfer function over the decode's own range: nothing in its lowest quarter, a warm haze up to the middle, dense and white
    from three quarters on"""
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    whole = NFGR.decompress(opt, mod, side)
    vmin, span = int(whole.min()), int(whole.max()) - int(whole.min())
    assert span >= 64, "the fit is too short for a decode with structure"
    return "%d:255,120,0,0;%d:255,160,40,0.1;%d:255,255,255,0.6" % (vmin + span // 4, vmin + span // 2, vmin + 3 * span // 4)


def _check_python_call(opt, cdir):
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    side = load_yaml(side_path)
    text = _transfer(opt, cdir)
    cf = copy.deepcopy(opt.CompressFramework)
    phi = _load_phi(cf, mod, side, "cuda")
    lo, hi = _coords_range(cf.Compress.coords_mode)
    rng = minmaxany_range(cf.Normalize.name)
    view = VW.make_view(SHAPE, DIRECTION, **GEOM)
    assert view.rows * view.cols <= 24 * 24 and view.depth <= 32
    for kw in ({}, dict(background=BG, bits=9, chunk=501)):
        img, hits, stats = NFGR.decompress_composite(opt, mod, side_path, DIRECTION, text, return_hits=True, **GEOM, **kw)
        tf = CP.make_transfer(CP.parse_transfer(text), "u16", GEOM["depth_spacing"], kw.get("bits"))
        assert tf.shape == (1 << kw.get("bits", 12), 4)
        want, want_hits, want_stats = CP.render_composite(phi, view, tf, lo, hi, "u16", rng, (side["min"], side["max"]),
                                                          background=kw.get("background", (0, 0, 0)))
        assert img.dtype == np.uint8 and img.shape == (view.rows, view.cols, 4) and np.array_equal(img, want.cpu().numpy())
        assert np.array_equal(hits, want_hits.cpu().numpy()) and stats == want_stats
        assert np.array_equal(NFGR.decompress_composite(opt, mod, side_path, DIRECTION, text, **GEOM, **kw), img)
        # not vacuous: hazy and dense pixels, and rays that miss the clip box and show the background
        alpha = img[..., 3]
        print("%s: %d rays hit, A == 0 on %d of them, 20 < A < 235 on %d, A >= 250 on %d; %d colours" % (
            text, (hits > 0).sum(), (alpha[hits > 0] == 0).sum(), ((alpha > 20) & (alpha < 235)).sum(), (alpha >= 250).sum(),
            len(np.unique(img[..., :3].reshape(-1, 3), axis=0))))
        assert ((alpha > 20) & (alpha < 235)).sum() >= 10 and (alpha >= 250).any()
        assert (hits == 0).any() and (img[hits == 0] == np.array(tuple(kw.get("background", (0, 0, 0))) + (0,), np.uint8)).all()
        assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) >= 30
    return text


def test_the_python_call_equals_render_composite_on_the_loaded_net(artefact):
    opt, cdir, _ = artefact
    _check_python_call(opt, cdir)


def test_quantised_artefact_renders_through_the_same_call(tmp_path):
    opt, cdir, _ = _fit(tmp_path, {"bits": 12, "finetune_steps": 500})
    assert os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    assert config.load(os.path.join(cdir, "sideinfos.yaml"))["quantize"]["bits"] == 12
    _check_python_call(opt, cdir)


def _cli(yml, cdir, out, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", out] + FLAGS + list(extra),
                          capture_output=True, text=True, timeout=300)


def test_cli_writes_the_python_calls_pixels(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    text = _transfer(opt, cdir)
    want = NFGR.decompress_composite(opt, mod, side, DIRECTION, text, background=BG, **GEOM)
    spec = tmp_path / "tf.txt"
    spec.write_text(text.replace(";", "\n") + "\n")
    # the .npy from the text itself; the .png from a file, with a coarser table: the channel and the bits reach the call
    for out, extra in (("c.npy", ["--view-composite", text]),
                       ("c.png", ["--view-composite", "@" + str(spec), "--view-composite-channel", "0", "--view-composite-bits", "4"])):
        r = _cli(yml, cdir, str(tmp_path / out), "--view-background", "%d,%d,%d" % BG, *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "composite view" in r.stdout and "rays hit" in r.stdout
    got = np.load(str(tmp_path / "c.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    coarse = NFGR.decompress_composite(opt, mod, side, DIRECTION, text, background=BG, bits=4, **GEOM)
    assert not np.array_equal(coarse, want)
    png = read_img(str(tmp_path / "c.png"))                        # cv2's order: B, G, R
    assert png.dtype == np.uint8 and np.array_equal(png[..., ::-1], coarse[..., :3]) and not np.array_equal(png, coarse[..., :3])
    assert sorted(os.listdir(str(tmp_path))) == ["c.npy", "c.png", "tf.txt"]


def test_artefacts_the_composite_does_not_serve_are_refused_by_name(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    side = load_yaml(side_path)
    text = _transfer(opt, cdir)
    call = lambda o, s: NFGR.decompress_composite(o, mod, s, DIRECTION, text, **GEOM)
    assert call(opt, dict(side)).shape[-1] == 4                   # (the side info as a dict is served)
    with pytest.raises(ValueError, match="composite view of a DivideTask artefact.*prefix.*follow-up"):
        call(opt, {"data_shape": list(SHAPE) + [1]})
    with pytest.raises(ValueError, match="error-bounded.*error_bound 3"):
        call(opt, dict(side, error_bound=3))
    with pytest.raises(ValueError, match="3-D data only"):
        NFGR.decompress_composite(opt, mod, dict(side, data_shape=[28, 32, 1]), DIRECTION, text)
    o = config.to_opt(config.to_plain(opt))
    o.CompressFramework.Decompress.postprocess.denoise.level = 300
    with pytest.raises(ValueError, match="composite view with a Decompress.postprocess that changes values.*denoise.level 300"):
        call(o, side_path)
    o = config.to_opt(config.to_plain(opt))
    o.CompressFramework.Decompress.postprocess.clip = [0, 40000]
    with pytest.raises(ValueError, match="composite view with a Decompress.postprocess that changes values.*40000"):
        call(o, side_path)
    # the CLI on a DivideTask artefact's directory
    os.makedirs(str(tmp_path / "art" / "sideinfos"))
    r = _cli(yml, str(tmp_path / "art"), str(tmp_path / "d.png"), "--view-composite", text)
    assert r.returncode != 0 and "--view-composite: a composite view of a DivideTask artefact" in r.stderr and "follow-up" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["art"]
