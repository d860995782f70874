"""Surface view of a stored DivideTask artefact: decompress_divide_surface against view.render_surface_partition on the loaded nets, and
decompress.py --view ... --view-owner nearest --view-surface LEVEL --view-surface-gap empty against the Python call's pixels; one block
re-written as a 12-bit quantised artefact is served like the others.  A fitted `total_2_2_2` artefact of a 32 x 48 x 64 volume, the
recipe of tests/test_gpu_view_partition_framework.py.  Every comparison is bitwise."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import artefact, config, quantize
from brief_pytorch_amd import view as VW
from brief_pytorch_amd.framework import NFGR, MyLogger, decompress_divide_surface, decompress_divide_view
from brief_pytorch_amd.modelsave import save_model
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, STEPS = (32, 48, 64), 2000      # (2000 steps: before that the decode of these nets is one grey level, tests/test_gpu_mip.py)
REGION = "3:29,5:43,1:60"
DIRECTION = (0.48, -0.6, 0.64)
GEOM = dict(up=(1, 0.2, 0), spacing=0.8, depth_spacing=0.5, voxel_size=(2, 1, 1), region=REGION)
FLAGS = ["--view", "0.48,-0.6,0.64", "--view-up", "1,0.2,0", "--view-spacing", "0.8", "--view-depth-spacing", "0.5", "--voxel-size", "2,1,1",
         "--view-owner", "nearest", "--view-surface-gap", "empty"]
ARRAYS = ("first", "t_lo", "t_hi", "t", "position", "normal", "shade", "hits", "owner")


@pytest.fixture(scope="module")
def divided(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("surface_divide")
    path = str(tmp_path / "d.tif")
    save_img(path, make_volume(SHAPE, seed=7))
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
    assert len(os.listdir(os.path.join(cdir, "module"))) == 8
    return fw, opt, cdir, yml


def _args(cdir):
    return os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos")


def _level(opt, cdir):
    """the median over the rays that meet the clip box of the max view of the raw integer decode"""
    o = config.to_opt(config.to_plain(opt))
    pp = o.CompressFramework.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 0, False, [0, 65535]
    img, hits, _ = decompress_divide_view(o, *_args(cdir), DIRECTION, mode="max", return_hits=True, **GEOM)
    return int(np.median(img[..., 0][hits > 0]))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_python_call(opt, cdir, level):
    args = _args(cdir)
    data_shape, blocks = artefact.divide_blocks(*args)
    parts = []
    for b in blocks:
        art = artefact.open_artefact(opt, b.module_path, b.side)
        parts.append((art.load_phi("cuda"), [b.ranges[a][0] for a in "dhw"], art.dims, art.lo, art.hi, art.norm_range, art.vrange))
    assert len({p[6] for p in parts}) > 1, "every block has the same value range: the per-block epilogue is not exercised"
    view = VW.make_view(data_shape[:-1], DIRECTION, **GEOM)
    results = {}
    for name, kw in (("above", {}), ("lit", dict(light=(0.0, 0.6, -0.8), refine=1)), ("plain", dict(shading=False, refine=0))):
        res = decompress_divide_surface(opt, *args, DIRECTION, level, **GEOM, **kw)
        light = kw.get("light", VW.frame(DIRECTION, GEOM["up"])[2])
        want = VW.render_surface_partition(parts, view, level, "u16", voxel_size=GEOM["voxel_size"], **{**kw, "light": light})
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
        print("%s: level %d, %d of %d rays that meet the box hit, %d cut, %d straddle, owners %s" % (
            name, level, stats["rays_surface"], stats["rays_hit"], stats["rays_cut"], stats["rays_straddle"], sorted(set(res["owner"][hit].tolist()))))
        assert stats["rays_surface"] >= 0.25 * stats["rays_hit"] and stats["rays_surface"] > stats["rays_cut"]
        assert stats["blocks"] == 8 and stats["blocks_hit"] == 8 and len(set(res["owner"][hit].tolist())) >= 3 and (res["owner"][~hit] == -1).all()
        results[name] = res
    assert results["above"]["stats"]["rays_straddle"] >= 1 and results["above"]["stats"]["refine_points"] > 0
    assert results["above"]["shade"].max() > 0.5 and len(np.unique(results["above"]["shade"])) > 50
    assert np.array_equal(results["plain"]["first"], results["above"]["first"])
    return results


def test_the_python_call_equals_render_surface_partition_on_the_loaded_nets(divided):
    fw, opt, cdir, _ = divided
    level = _level(opt, cdir)
    results = _check_python_call(opt, cdir, level)
    # the method of an NFGR: its own options and device
    res = fw.decompress_divide_surface(*_args(cdir), DIRECTION, level, opt=opt, **GEOM)
    assert all(_same(res[k], results["above"][k]) for k in ARRAYS + ("depth",))


def test_a_quantised_block_is_served(divided, tmp_path):
    _, opt, cdir, _ = divided
    copy = str(tmp_path / "compressed")
    shutil.copytree(cdir, copy)
    args = _args(copy)
    _, blocks = artefact.divide_blocks(*args)
    b = blocks[3]
    art = artefact.open_artefact(opt, b.module_path, b.side)
    phi = art.load_phi("cuda")
    save_model(phi, b.module_path, "cuda", quantize_bits=12)
    assert os.listdir(b.module_path) == [quantize.FILE_NAME]
    level = _level(opt, cdir)
    results = _check_python_call(opt, copy, level)                # (the nets it compares against are loaded from the same files)
    plain = decompress_divide_surface(opt, *_args(cdir), DIRECTION, level, **GEOM)
    hit = results["above"]["first"] >= 0
    assert (results["above"]["owner"][hit] == 3).any()
    assert not _same(results["above"]["t"], plain["t"]) or not _same(results["above"]["normal"], plain["normal"])      # 12 bits move the block's surface


def _cli(yml, cdir, out, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", out] + FLAGS + list(extra),
                          capture_output=True, text=True, timeout=300)


def test_cli_writes_the_python_calls_pixels(divided, tmp_path):
    _, opt, cdir, yml = divided
    level = _level(opt, cdir)
    want = decompress_divide_surface(opt, *_args(cdir), DIRECTION, level, **GEOM)
    packed = np.concatenate([want["depth"][..., None], want["normal"], want["shade"][..., None]], axis=-1).astype(np.float32)
    r = _cli(yml, cdir, str(tmp_path / "surface.npy"), "--view-surface", str(level))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DivideTask" in r.stdout and "8 of 8 blocks hit" in r.stdout and "owner nearest" in r.stdout and "gap empty" in r.stdout
    assert "surface view" in r.stdout and "rays hit the surface" in r.stdout
    got = np.load(str(tmp_path / "surface.npy"))
    assert got.dtype == np.float32 and got.shape == want["shade"].shape + (5,) and _same(got, packed)
    r = _cli(yml, cdir, str(tmp_path / "surface.png"), "--view-surface", str(level))
    assert r.returncode == 0, r.stderr[-2000:]
    image = np.floor(255.0 * want["shade"].astype(np.float64) + 0.5).astype(np.uint8)
    got = read_img(str(tmp_path / "surface.png"))
    assert got.dtype == np.uint8 and np.array_equal(got.reshape(image.shape), image) and len(np.unique(image)) > 50
    assert sorted(os.listdir(str(tmp_path))) == ["surface.npy", "surface.png"]
    # without the gap rule the pinned refusal stands, and nothing is written
    flags = [f for f in FLAGS if f not in ("--view-surface-gap", "empty")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", REGION, "-o", str(tmp_path / "no.png")]
                       + flags + ["--view-surface", str(level)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--view-surface with --view-owner" in r.stderr and "--view-surface-gap empty" in r.stderr
    assert not os.path.exists(str(tmp_path / "no.png"))
