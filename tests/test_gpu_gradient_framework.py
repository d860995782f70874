"""Spatial gradients of stored artefacts on the GPU: NFGR.decompress_gradient / decompress_divide_gradient and decompress.py
--gradient against voxel_scale x the float64 Jacobian (tests/_jacobian.py) of the weights the artefact loads, inside the Jacobian band
of tests/test_gpu_gradient.py, and bitwise against the slice of the whole-volume call."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, gradient, mip, quantize
from brief_pytorch_amd.framework import NFGR, MyLogger, decompress_divide_gradient
from brief_pytorch_amd.io import load_yaml
from brief_pytorch_amd.networks import SIREN
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import save_img

from ._jacobian import JAC_TOL, relerr, value_and_jacobian

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, SHAPE, FEATURES = 100, (20, 24, 28), 24
PARAMS = SIREN.calc_param_count(3, 1, FEATURES, 5)
REGION = "3:18,2:22:2,1:27:3"
REGION_SLICES = (slice(3, 18), slice(2, 22, 2), slice(1, 27, 3))


def _opt(tmp_path, yaml="default.yaml", given=4.0 * PARAMS, **compress):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", yaml))
    cf = opt.CompressFramework
    cf.Compress.max_steps = STEPS
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = float(given)
    cf.Compress.loss_log_freq = STEPS
    for k, v in compress.items():
        setattr(cf.Compress, k, v)
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp_path / "outputs")
    opt.Log.time = False
    return opt


def _fit(tmp_path, shape=SHAPE, divide=None, **kw):
    os.makedirs(str(tmp_path), exist_ok=True)
    vol = make_volume(shape, seed=11)
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    opt = _opt(tmp_path, **kw)
    if divide:
        opt.CompressFramework.Compress.divide.divide_type = divide
        opt.CompressFramework.Compress.divide.param_alloc = "equal"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    fw = NFGR(opt.CompressFramework, Log=Log)
    if divide:
        fw.compress_divide(path, opt)
    else:
        fw.compress(path)
    cdir = os.path.join(Log.logdir, "steps%d" % STEPS, "compressed")
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    return opt, cdir, yml


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    return _fit(tmp_path_factory.mktemp("grad_single"))


def _grid_coords(dims, lo=-1.0, hi=1.0):
    axes = [torch.linspace(lo, hi, n) for n in dims]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


def _reference(opt, mod, side, dims):
    """voxel_scale x the float64 Jacobian of the weights the artefact loads, over the whole linspace grid `dims`, and torch's own fp32
    distance from it"""
    side = load_yaml(side) if isinstance(side, str) else side
    cf = config.to_opt(config.to_plain(opt)).CompressFramework
    phi = mip._load_phi(cf, mod, side, "cpu")
    x = _grid_coords(dims).reshape(-1, 3)
    _, j64 = value_and_jacobian(phi, x, torch.float64)
    _, j32 = value_and_jacobian(phi, x, torch.float32)
    scale = gradient.voxel_scale(dims, -1.0, 1.0, (0.0, 100.0), side["min"], side["max"])
    return (j64 * scale).reshape(*dims, 1, 3), relerr(j32, j64), phi


def _check_artefact(opt, cdir):
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    whole = NFGR.decompress_gradient(opt, mod, side)
    assert whole.dtype == np.float32 and whole.shape == SHAPE + (1, 3)
    want, own, phi = _reference(opt, mod, side, SHAPE)
    got, band = relerr(whole, want), max(JAC_TOL, 3 * own)
    print("whole volume: gradient relerr %.3e (band %.3e; torch fp32 against float64 %.3e), max |g| %.3f grey levels per voxel" % (
        got, band, own, float(np.abs(want).max())))
    assert got < band
    assert np.abs(want).max() > 1e-3, "the fitted net is flat: the comparison is vacuous"
    # a region is the slice of the whole, bit for bit; a stride keeps the per-voxel unit
    assert np.array_equal(NFGR.decompress_gradient(opt, mod, side, REGION), whole[REGION_SLICES])
    assert np.array_equal(NFGR.decompress_gradient(opt, mod, side, ":,:,:", 2), whole[::2, ::2, ::2])
    # a resampled view: the resampled grid's spacing
    shape = (10, 31, 14)
    view = NFGR.decompress_gradient(opt, mod, side, shape=shape)
    want, own, _ = _reference(opt, mod, side, shape)
    assert view.shape == shape + (1, 3) and relerr(view, want) < max(JAC_TOL, 3 * own)
    return whole, phi


def test_singletask_gradient_in_grey_levels_per_voxel(single):
    opt, cdir, _ = single
    assert load_yaml(os.path.join(cdir, "sideinfos.yaml"))["phi_features"] == FEATURES
    _check_artefact(opt, cdir)


def test_quantised_artefact_gives_the_gradient_of_the_dequantised_weights(tmp_path, single):
    bits = 12
    given = quantize.overhead_bytes(5) + quantize.code_bytes(PARAMS, bits)
    opt, cdir, _ = _fit(tmp_path, given=given, quantize={"bits": bits, "finetune_steps": 0})
    assert os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    assert load_yaml(os.path.join(cdir, "sideinfos.yaml"))["phi_features"] == FEATURES
    _, phi = _check_artefact(opt, cdir)                 # (the reference is built from load_model's dequantised weights)
    masters = mip._load_phi(config.to_opt(config.to_plain(single[0])).CompressFramework, os.path.join(single[1], "module"),
                            load_yaml(os.path.join(single[1], "sideinfos.yaml")), "cpu")
    assert not torch.equal(phi.params, masters.params)


def test_error_bounded_artefact_gives_the_gradient_of_the_net_alone(tmp_path, single):
    """the same fit with error_bound: 300 stores byte-identical weights plus corrections, which have no derivative"""
    opt, cdir, _ = _fit(tmp_path, error_bound=300)
    assert os.path.isfile(os.path.join(cdir, "corrections.bin")) and "error_bound" in load_yaml(os.path.join(cdir, "sideinfos.yaml"))
    got = NFGR.decompress_gradient(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"), REGION)
    want = NFGR.decompress_gradient(single[0], os.path.join(single[1], "module"), os.path.join(single[1], "sideinfos.yaml"), REGION)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def divided(tmp_path_factory):
    return _fit(tmp_path_factory.mktemp("grad_divide"), shape=(24, 24, 28), divide="total_2_1_1", given=8.0 * PARAMS)


def test_dividetask_blocks_keep_their_own_grid_and_scale(divided, tmp_path):
    opt, cdir, _ = divided
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    names = sorted(os.listdir(args[1]))
    assert names == ["d_0_11-h_0_23-w_0_27", "d_12_23-h_0_23-w_0_27"]
    # a region across the block face, part by part: each block's own decompress_gradient on its module directory
    got = decompress_divide_gradient(opt, *args, "8:17,2:20:2,:")
    assert got.dtype == np.float32 and got.shape == (9, 9, 28, 1, 3)
    parts = [NFGR.decompress_gradient(opt, os.path.join(args[1], n, "module"), os.path.join(args[2], n, "sideinfos.yaml"), r)
             for n, r in zip(names, ("8:12,2:20:2,:", "0:5,2:20:2,:"))]
    assert np.array_equal(got[:4], parts[0]) and np.array_equal(got[4:], parts[1])
    assert np.abs(got).max() > 0
    whole = decompress_divide_gradient(opt, *args)
    assert whole.shape == (24, 24, 28, 1, 3) and np.array_equal(whole[8:17, 2:20:2], got)
    # a partition with a block missing: voxels no block covers are 0
    gap = str(tmp_path / "gap")
    shutil.copytree(cdir, gap)
    for sub in ("module", "sideinfos"):
        shutil.rmtree(os.path.join(gap, sub, names[1]))
    g = decompress_divide_gradient(opt, os.path.join(gap, "sideinfos.yaml"), os.path.join(gap, "module"), os.path.join(gap, "sideinfos"), "8:17,2:20:2,:")
    assert np.array_equal(g[:4], parts[0]) and not g[4:].any()
    # overlapping blocks are refused by name
    over = str(tmp_path / "over")
    shutil.copytree(cdir, over)
    for sub in ("module", "sideinfos"):
        os.rename(os.path.join(over, sub, names[1]), os.path.join(over, sub, "d_11_22-h_0_23-w_0_27"))
    with pytest.raises(ValueError, match="overlap"):
        decompress_divide_gradient(opt, os.path.join(over, "sideinfos.yaml"), os.path.join(over, "module"), os.path.join(over, "sideinfos"))


def _cli(yml, cdir, region, mode, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", region, "--gradient", mode, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "spatial gradient" in r.stdout and "float32" in r.stdout
    return np.load(out)


def test_cli_writes_components_and_magnitude(single, tmp_path):
    opt, cdir, yml = single
    comp = _cli(yml, cdir, REGION, "components", str(tmp_path / "c.npy"))
    assert comp.dtype == np.float32 and comp.shape == (15, 10, 9, 1, 3)
    assert np.array_equal(comp, NFGR.decompress_gradient(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"), REGION))
    mag = _cli(yml, cdir, REGION, "magnitude", str(tmp_path / "m.npy"))
    assert mag.dtype == np.float32 and mag.shape == (15, 10, 9, 1)
    assert np.allclose(mag, np.sqrt((comp.astype(np.float64) ** 2).sum(-1)), rtol=1e-6)


def test_other_nets_and_precisions_are_refused_before_any_decode(tmp_path):
    """on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    mod = str(tmp_path / "module")
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    with pytest.raises(ValueError, match=r"spatial gradients exist for fp32 SIREN up to 1024 features \(this net is FFN"):
        NFGR.decompress_gradient(opt, mod, dict(side, phi_name="FFN"))
    with pytest.raises(ValueError, match=r"spatial gradients exist for fp32 SIREN.*bf16"):
        NFGR.decompress_gradient(opt, mod, dict(side, phi_precision="bf16"))
    with pytest.raises(ValueError, match="1500 features"):
        NFGR.decompress_gradient(opt, mod, dict(side, phi_features=1500))
    o = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    o.CompressFramework.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmaxany_a_b.*minmax01"):
        NFGR.decompress_gradient(o, mod, side)
    # stored artefacts of an FFN and of a bf16 fit
    opt, cdir, _ = _fit(tmp_path / "ffn", yaml="ffn.yaml", given=20000.0)
    with pytest.raises(ValueError, match=r"spatial gradients exist for fp32 SIREN up to 1024 features \(this net is FFN"):
        NFGR.decompress_gradient(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"))
    opt, cdir, _ = _fit(tmp_path / "bf16", precision="bf16")
    assert load_yaml(os.path.join(cdir, "sideinfos.yaml"))["phi_precision"] == "bf16"
    with pytest.raises(ValueError, match=r"spatial gradients exist for fp32 SIREN.*bf16"):
        NFGR.decompress_gradient(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"))
