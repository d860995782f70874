"""Hessians of stored artefacts on the GPU: NFGR.decompress_hessian / decompress_divide_hessian and decompress.py --hessian.  A region is
the slice of the whole bit for bit, the laplacian is the trace of the components exactly, and the UNIT (grey levels per voxel step
squared) is checked against the central difference of decompress_gradient on a grid resampled four times finer: that guards the
step_a x step_b scaling, not the kernel (tests/test_gpu_hessian.py does that)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, gradient, hessian, mip, quantize
from brief_pytorch_amd.framework import NFGR, MyLogger
from brief_pytorch_amd.io import load_yaml
from brief_pytorch_amd.networks import SIREN
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import save_img

from ._hessian import HESS_TOL, value_jacobian_hessian
from ._jacobian import relerr, value_and_jacobian

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, SHAPE, FEATURES = 100, (20, 24, 28), 24
PARAMS = SIREN.calc_param_count(3, 1, FEATURES, 5)
REGION = "3:18,2:22:2,1:27:3"
REGION_SLICES = (slice(3, 18), slice(2, 22, 2), slice(1, 27, 3))
REGION_SHAPE = (15, 10, 9)


def _opt(tmp_path, given=4.0 * PARAMS, **compress):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
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
    path = str(tmp_path / "vol.tif")
    save_img(path, make_volume(shape, seed=11))
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
    return opt, cdir, yml, fw


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    return _fit(tmp_path_factory.mktemp("hess_single"))


def _paths(cdir):
    return os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")


def _grid_coords(dims, lo=-1.0, hi=1.0):
    axes = [torch.linspace(lo, hi, n, dtype=torch.float64) for n in dims]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(dims))


def _load_cpu(opt, cdir):
    mod, side = _paths(cdir)
    side = load_yaml(side)
    return mip._load_phi(config.to_opt(config.to_plain(opt)).CompressFramework, mod, side, "cpu"), side


def _check_artefact(opt, cdir):
    """components against voxel_scale x the float64 Hessian of the weights the artefact loads; region, stride and the derived maps"""
    mod, side = _paths(cdir)
    whole = NFGR.decompress_hessian(opt, mod, side)
    assert whole.dtype == np.float32 and whole.shape == SHAPE + (1, 6)
    phi, sd = _load_cpu(opt, cdir)
    x = _grid_coords(SHAPE)
    _, _, h64 = value_jacobian_hessian(phi, x, torch.float64)
    _, _, h32 = value_jacobian_hessian(phi, x, torch.float32)
    scale = hessian.voxel_scale(SHAPE, -1.0, 1.0, (0.0, 100.0), sd["min"], sd["max"])
    want, own = (h64 * scale).reshape(*SHAPE, 1, 6), relerr(h32, h64)
    got, band = relerr(whole, want), max(HESS_TOL, 3 * own)
    print("whole volume: hessian relerr %.3e (band %.3e; torch fp32 against float64 %.3e), max |h| %.3f grey levels per voxel^2" % (
        got, band, own, float(np.abs(want).max())))
    assert got < band
    assert np.abs(want).max() > 1e-3, "the fitted net is flat: the comparison is vacuous"
    # a region is the slice of the whole, bit for bit; a stride keeps the unit
    reg = NFGR.decompress_hessian(opt, mod, side, REGION)
    assert reg.shape == REGION_SHAPE + (1, 6) and np.array_equal(reg, whole[REGION_SLICES])
    assert np.array_equal(NFGR.decompress_hessian(opt, mod, side, ":,:,:", 2), whole[::2, ::2, ::2])
    # the laplacian is the trace of the components, exactly; the eigenvalues sum to it
    lap = NFGR.decompress_hessian(opt, mod, side, REGION, mode="laplacian")
    assert lap.shape == REGION_SHAPE + (1,) and np.array_equal(lap, reg[..., 0] + reg[..., 3] + reg[..., 5])
    ev = NFGR.decompress_hessian(opt, mod, side, REGION, mode="eigenvalues")
    assert ev.shape == REGION_SHAPE + (1, 3) and np.all(np.diff(np.abs(ev), axis=-1) >= 0)
    full = hessian.full(torch.from_numpy(reg)).numpy().astype(np.float64)
    assert np.abs(np.sort(ev.astype(np.float64), -1) - np.linalg.eigvalsh(full)).max() <= 1e-5 * np.abs(ev).max()
    ves = NFGR.decompress_hessian(opt, mod, side, REGION, mode="vesselness")
    assert ves.shape == REGION_SHAPE + (1,) and ves.dtype == np.float32 and ves.min() >= 0 and ves.max() <= 1 and ves.max() > 0
    # (the same float64 formula on the host: exp, acos and cos may differ in their last float64 bit between the two, which can move the
    #  rounding to float32 by one unit in the last place)
    assert np.allclose(ves, hessian.vesselness(torch.from_numpy(reg)).numpy(), rtol=2.0 ** -22, atol=1e-12)
    return whole, phi


def test_singletask_hessian_region_and_derived_maps(single):
    opt, cdir = single[:2]
    assert load_yaml(os.path.join(cdir, "sideinfos.yaml"))["phi_features"] == FEATURES
    _check_artefact(opt, cdir)


def test_the_unit_is_grey_levels_per_voxel_step_squared(single):
    """components[..., (a, a)] on the fitted grid against the central difference along axis a of decompress_gradient[..., a] on a grid four
    times finer (shape = 4 (n - 1) + 1: every fitted voxel is a voxel of the fine grid).  In fine-grid units the gradient is per fine
    step, so  H_aa ~ 16 (g_a[i + 1] - g_a[i - 1]) / 2  per fitted step squared.  The tolerance is the error of that same finite
    difference applied to the float64 restatement (its truncation error), times 3, printed."""
    opt, cdir = single[:2]
    mod, side = _paths(cdir)
    fine = tuple(4 * (n - 1) + 1 for n in SHAPE)
    comp = NFGR.decompress_hessian(opt, mod, side).astype(np.float64)
    grad = NFGR.decompress_gradient(opt, mod, side, shape=list(fine)).astype(np.float64)
    assert grad.shape == fine + (1, 3)
    phi, sd = _load_cpu(opt, cdir)
    _, j64 = value_and_jacobian(phi, _grid_coords(fine), torch.float64)
    j64 = (j64 * gradient.voxel_scale(fine, -1.0, 1.0, (0.0, 100.0), sd["min"], sd["max"])).reshape(*fine, 1, 3)
    _, _, h64 = value_jacobian_hessian(phi, _grid_coords(SHAPE), torch.float64)
    h64 = (h64 * hessian.voxel_scale(SHAPE, -1.0, 1.0, (0.0, 100.0), sd["min"], sd["max"])).reshape(*SHAPE, 1, 6)
    for a, k in ((0, 0), (1, 3), (2, 5)):
        def fd(g):
            g = np.moveaxis(g[..., 0, a], a, 0)                               # [fine_a, ...]
            d = 16.0 * (g[5::4] - g[3:-4:4]) / 2.0                            # at the fitted voxels 1 .. n - 2 of axis a
            other = [slice(None, None, 4)] * 2
            return np.moveaxis(d[(slice(None), *other)], 0, a)
        inner = tuple(slice(1, -1) if ax == a else slice(None) for ax in range(3))
        ref = h64[inner][..., 0, k]
        tol = 3 * np.abs(fd(j64) - ref).max() / np.abs(ref).max()
        err = np.abs(fd(grad) - comp[inner][..., 0, k]).max() / np.abs(ref).max()
        print("axis %d: hessian against the finite difference of the gradient %.3e (tolerance %.3e = 3 x the float64 restatement's)" % (a, err, tol))
        assert err < tol, (a, err, tol)
        # the wrong power of the step would be off by (n_a - 1) / 2 or its inverse: far outside
        assert tol < 0.5


def test_quantised_artefact_decodes(tmp_path, single):
    bits = 12
    given = quantize.overhead_bytes(5) + quantize.code_bytes(PARAMS, bits)
    opt, cdir = _fit(tmp_path, given=given, quantize={"bits": bits, "finetune_steps": 0})[:2]
    assert os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    _, phi = _check_artefact(opt, cdir)                 # (the reference is built from load_model's dequantised weights)
    masters, _ = _load_cpu(single[0], single[1])
    assert not torch.equal(phi.params, masters.params)


@pytest.fixture(scope="module")
def divided(tmp_path_factory):
    return _fit(tmp_path_factory.mktemp("hess_divide"), shape=(24, 24, 28), divide="total_2_1_1", given=8.0 * PARAMS)


def test_dividetask_blocks_keep_their_own_grid_and_scale(divided):
    opt, cdir, _, fw = divided
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    names = sorted(os.listdir(args[1]))
    assert names == ["d_0_11-h_0_23-w_0_27", "d_12_23-h_0_23-w_0_27"]
    whole = fw.decompress_divide_hessian(*args, opt=opt)
    assert whole.dtype == np.float32 and whole.shape == (24, 24, 28, 1, 6) and np.abs(whole).max() > 0
    # a region across the block face equals the slice of the whole bit for bit, and each part is its block's own decompress_hessian
    got = fw.decompress_divide_hessian(*args, region="8:17,2:20:2,:", opt=opt)
    assert got.shape == (9, 9, 28, 1, 6) and np.array_equal(got, whole[8:17, 2:20:2])
    parts = [NFGR.decompress_hessian(opt, os.path.join(args[1], n, "module"), os.path.join(args[2], n, "sideinfos.yaml"), r)
             for n, r in zip(names, ("8:12,2:20:2,:", "0:5,2:20:2,:"))]
    assert np.array_equal(got[:4], parts[0]) and np.array_equal(got[4:], parts[1])
    lap = fw.decompress_divide_hessian(*args, region="8:17,2:20:2,:", mode="laplacian", opt=opt)
    assert np.array_equal(lap, got[..., 0] + got[..., 3] + got[..., 5])


def _cli(yml, cdir, region, mode, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", region, "--hessian", mode, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Hessian" in r.stdout and "float32" in r.stdout
    return np.load(out)


def test_cli_writes_the_four_modes(single, tmp_path):
    opt, cdir, yml = single[:3]
    mod, side = _paths(cdir)
    for mode, tail in (("components", (1, 6)), ("laplacian", (1,)), ("eigenvalues", (1, 3)), ("vesselness", (1,))):
        got = _cli(yml, cdir, REGION, mode, str(tmp_path / (mode + ".npy")))
        assert got.dtype == np.float32 and got.shape == REGION_SHAPE + tail, mode
        assert np.array_equal(got, NFGR.decompress_hessian(opt, mod, side, REGION, mode=mode)), mode


def test_other_nets_and_precisions_are_refused_before_any_decode(tmp_path):
    """on option and side-info dicts alone: the module path does not exist, so reaching the decode would fail differently"""
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    mod = str(tmp_path / "module")
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "data_shape": [8, 9, 10, 1], "phi_features": 22, "phi_name": "SIREN"}
    with pytest.raises(ValueError, match=r"spatial Hessians exist for fp32 SIREN up to 1024 features \(this net is FFN"):
        NFGR.decompress_hessian(opt, mod, dict(side, phi_name="FFN"))
    with pytest.raises(ValueError, match=r"spatial Hessians exist for fp32 SIREN.*bf16"):
        NFGR.decompress_hessian(opt, mod, dict(side, phi_precision="bf16"))
    with pytest.raises(ValueError, match="1500 features"):
        NFGR.decompress_hessian(opt, mod, dict(side, phi_features=1500))
    with pytest.raises(ValueError, match="unknown Hessian mode"):
        NFGR.decompress_hessian(opt, mod, side, mode="magnitude")
    o = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    o.CompressFramework.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmaxany_a_b.*minmax01"):
        NFGR.decompress_hessian(o, mod, side)
