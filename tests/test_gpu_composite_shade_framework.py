"""Shaded composite of stored artefacts: NFGR.decompress_composite with shade against composite.render_composite on the loaded net, and
decompress.py --view-composite-shade against the Python call's pixels, for a plain and a 12-bit quantised artefact; --voxel-size and
--view-composite-light reach the gradient's scale and the light; the artefact kinds without a Jacobian kernel are refused before any
decode.  Every comparison is bitwise."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import composite as CP
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
GEOM = dict(up=(1, 0.2, 0), spacing=2.4, depth_spacing=1.6, voxel_size=(2, 1, 1), region=REGION)
FLAGS = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "2.4", "--view-depth-spacing", "1.6"]
BG = (10, 40, 90)
SHADE, LIGHT = (0.25, 0.75), (0.2, 0.9, -0.4)


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
    return _fit(tmp_path_factory.mktemp("composite_shade_single"))


def _transfer(opt, cdir):
    """(text, the level from which a sample is opaque): nothing in the decode's lowest quarter, a warm haze up to the middle, dense from
    three quarters on and opaque in the top eighth, so that rays saturate and what lies behind needs no gradient"""
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    whole = NFGR.decompress(opt, mod, side)
    vmin, span = int(whole.min()), int(whole.max()) - int(whole.min())
    assert span >= 64, "the fit is too short for a decode with structure"
    opaque = vmin + 7 * span // 8
    return "%d:255,120,0,0;%d:255,160,40,0.1;%d:255,255,255,0.6;%d:200,220,255,1" % (vmin + span // 4, vmin + span // 2, vmin + 3 * span // 4, opaque), opaque


def _not_vacuous(opt, cdir, opaque, stats, img, plain):
    """the selection is exercised: some samples are lit, some inside samples are not, a ray meets an opaque sample (a table row stands
    for 16 levels: a value 16 above the opaque level has an opaque row), and the shading shows"""
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    assert 0 < stats["samples_shaded"] < stats["samples_inside"], stats
    top = NFGR.decompress_view(opt, mod, side, DIRECTION, mode="max", **GEOM)
    assert (top >= opaque + 16).any(), "no ray reaches TAU_SAT"
    assert np.array_equal(img[..., 3], plain[..., 3]) and (img[..., :3] <= plain[..., :3]).all()
    assert (img[..., :3] != plain[..., :3]).any(axis=-1).sum() >= 30


def _check_python_call(opt, cdir):
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    side = load_yaml(side_path)
    text, opaque = _transfer(opt, cdir)
    cf = copy.deepcopy(opt.CompressFramework)
    phi = _load_phi(cf, mod, side, "cuda")
    lo, hi = _coords_range(cf.Compress.coords_mode)
    rng = minmaxany_range(cf.Normalize.name)
    view = VW.make_view(SHAPE, DIRECTION, **GEOM)
    assert view.rows * view.cols <= 24 * 24 and view.depth <= 32
    tf = CP.make_transfer(CP.parse_transfer(text), "u16", GEOM["depth_spacing"])
    plain = NFGR.decompress_composite(opt, mod, side_path, DIRECTION, text, background=BG, **GEOM)
    gscale = gradient.voxel_scale(list(SHAPE), lo, hi, rng, side["min"], side["max"]) / np.array(GEOM["voxel_size"], np.float64)
    for light, physical in ((None, VW.frame(DIRECTION, GEOM["up"])[2]), (LIGHT, VW._unit3(LIGHT, "light"))):
        img, hits, stats = NFGR.decompress_composite(opt, mod, side_path, DIRECTION, text, background=BG, return_hits=True, shade=SHADE, light=light,
                                                     chunk=501, **GEOM)
        want, want_hits, want_stats = CP.render_composite(phi, view, tf, lo, hi, "u16", rng, (side["min"], side["max"]), background=BG, shade=SHADE,
                                                          light=physical, gscale=gscale)
        assert img.dtype == np.uint8 and img.shape == (view.rows, view.cols, 4) and np.array_equal(img, want.cpu().numpy())
        assert np.array_equal(hits, want_hits.cpu().numpy()) and stats == want_stats
        _not_vacuous(opt, cdir, opaque, stats, img, plain)
    return text, opaque


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


def test_cli_writes_the_python_calls_pixels_and_its_options_reach_the_shading(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    text, opaque = _transfer(opt, cdir)
    geom = {k: v for k, v in GEOM.items() if k != "voxel_size"}
    call = lambda **kw: NFGR.decompress_composite(opt, mod, side, DIRECTION, text, background=BG, return_hits=True, **{**geom, **kw})
    plain = call(voxel_size=(2, 1, 1))[0]
    want, _, stats = call(voxel_size=(2, 1, 1), shade=SHADE)
    _not_vacuous(opt, cdir, opaque, stats, want, plain)
    lit = call(voxel_size=(2, 1, 1), shade=SHADE, light=LIGHT)[0]
    assert not np.array_equal(lit, want), "the light does not reach the shading"
    base = ["--view-composite", text, "--view-background", "%d,%d,%d" % BG, "--view-composite-shade", "%g,%g" % SHADE]
    runs = (("l.npy", base + ["--voxel-size", "2,1,1", "--view-composite-light", "%g,%g,%g" % LIGHT], lit), ("c.png", base + ["--voxel-size", "2,1,1"], want))
    for out, extra, ref in runs:
        r = _cli(yml, cdir, str(tmp_path / out), *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "composite view" in r.stdout and "of them shaded (%g,%g)" % SHADE in r.stdout
        if out.endswith(".npy"):
            got = np.load(str(tmp_path / out))
            assert got.dtype == np.uint8 and np.array_equal(got, ref), out
        else:
            png = read_img(str(tmp_path / out))                    # cv2's order: B, G, R
            assert png.dtype == np.uint8 and np.array_equal(png[..., ::-1], ref[..., :3])
    # equal settings by either route give equal bits: the default light is the view direction, named or not
    named = call(voxel_size=(2, 1, 1), shade=SHADE, light=VW.frame(DIRECTION, GEOM["up"])[2])[0]
    assert np.array_equal(named, want)
    # other voxels by either route (--voxel-size moves the rays too: test_gscale_follows_the_voxel_size holds the view and moves gscale alone)
    other = call(voxel_size=(1, 1, 1), shade=SHADE, light=(1, 0, 0))
    other_plain = call(voxel_size=(1, 1, 1))[0]
    r = _cli(yml, cdir, str(tmp_path / "v.npy"), *base, "--view-composite-light", "1,0,0")      # (--voxel-size defaults to 1,1,1)
    assert r.returncode == 0 and np.array_equal(np.load(str(tmp_path / "v.npy")), other[0]), r.stderr[-2000:]
    assert not np.array_equal(other[0], other_plain) and np.array_equal(other[0][..., 3], other_plain[..., 3])
    assert sorted(os.listdir(str(tmp_path))) == ["c.png", "l.npy", "v.npy"]


def test_gscale_follows_the_voxel_size(artefact):
    """the view is fixed by hand (render_composite on one view), so that only gscale moves: the voxel size that decompress_composite
    divides into it changes the normals, and with them the image"""
    opt, cdir, _ = artefact
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    side = load_yaml(side_path)
    text, opaque = _transfer(opt, cdir)
    art = VW.open_single(opt, mod, side_path)
    view = VW.make_view(SHAPE, DIRECTION, **GEOM)
    tf = CP.make_transfer(CP.parse_transfer(text), "u16", GEOM["depth_spacing"])
    phi = art.load_phi("cuda")
    imgs = []
    for voxel in ((2, 1, 1), (1, 1, 3)):
        light, gscale = VW.physical_shading(art, DIRECTION, GEOM["up"], LIGHT, voxel)
        assert np.allclose(gscale * np.array(voxel), gradient.voxel_scale(art.dims, art.lo, art.hi, art.norm_range, *art.vrange))
        img, _, stats = CP.render_composite(phi, view, tf, art.lo, art.hi, "u16", art.norm_range, art.vrange, background=BG, shade=SHADE, light=light,
                                            gscale=gscale)
        assert 0 < stats["samples_shaded"] < stats["samples_inside"]
        imgs.append(img.cpu().numpy())
    assert not np.array_equal(imgs[0], imgs[1]) and np.array_equal(imgs[0][..., 3], imgs[1][..., 3])
    top = NFGR.decompress_view(opt, mod, side_path, DIRECTION, mode="max", **GEOM)
    assert (top >= opaque + 16).any(), "no ray reaches TAU_SAT"
    assert side["phi_name"] == "SIREN"


def test_artefacts_without_a_jacobian_kernel_are_refused_by_name_before_any_decode(artefact, tmp_path):
    opt, cdir, yml = artefact
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    side = load_yaml(side_path)
    text, opaque = _transfer(opt, cdir)
    none = str(tmp_path / "no_module")                            # (reaching the decode would fail on the missing file instead)
    call = lambda s, **kw: NFGR.decompress_composite(opt, none, s, DIRECTION, text, shade=SHADE, **GEOM, **kw)
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*FFN"):
        call(dict(side, phi_name="FFN"))
    with pytest.raises(ValueError, match="shaded composite needs the analytic Jacobian: .*bf16"):
        call(dict(side, phi_precision="bf16"))
    with pytest.raises(ValueError, match="must each lie in \\[0, 1\\]"):
        NFGR.decompress_composite(opt, none, dict(side), DIRECTION, text, shade=(0.5, 2), **GEOM)
    # the served artefact through the same call, so that the refusals above are not the call's own failure
    img, _, stats = NFGR.decompress_composite(opt, mod, dict(side), DIRECTION, text, shade=SHADE, return_hits=True, **GEOM)
    assert 0 < stats["samples_shaded"] < stats["samples_inside"] and img.shape[-1] == 4
    top = NFGR.decompress_view(opt, mod, side_path, DIRECTION, mode="max", **GEOM)
    assert (top >= opaque + 16).any(), "no ray reaches TAU_SAT"
    # the CLI on a DivideTask artefact's directory, with and without the ownership rule
    os.makedirs(str(tmp_path / "art" / "sideinfos"))
    for extra, words in ((["--view-owner", "nearest"], "--view-composite-shade: a shaded composite of a DivideTask artefact is refused"),
                         ([], "--view-composite: a composite view of a DivideTask artefact")):
        r = _cli(yml, str(tmp_path / "art"), str(tmp_path / "d.png"), "--view-composite", text, "--view-composite-shade", "0.2,0.8", *extra)
        assert r.returncode != 0 and words in r.stderr and "follow-up" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["art"]
