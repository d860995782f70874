"""Region decode on the GPU (brief_siren_forward_box, SIREN.decode_box, NFGR.decompress_region / decompress_divide_region, decompress.py).
Every comparison is bitwise: a box of the grid must give exactly the values the whole-grid decode gives those voxels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, config
from brief_pytorch_amd.framework import NFGR, MyLogger
from brief_pytorch_amd.modelsave import save_model
from brief_pytorch_amd.networks import SIREN
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI = dict(scale=(-0.5, 0.5), vrange=(3.0, 60000.0))      # the integer epilogues see a spread of values, both clip ends included


def _net(L, F, cin, cout, precision="fp32", seed=0):
    torch.manual_seed(seed)
    return SIREN(coords_channel=cin, data_channel=cout, features=F, layers=L, w0=20, precision=precision).to(DEV)


def _boxes(dims):
    """(start, stop, step): the whole grid, one voxel, the far corner (upper half of the two-sided linspace), odd extents, steps 2, 3, 7"""
    nd = len(dims)
    last = [n - 1 for n in dims]
    return [([0] * nd, list(dims), 1),
            ([n // 3 for n in dims], [n // 3 + 1 for n in dims], 1),
            ([n - 3 for n in dims], list(dims), 1),
            ([1] * nd, [min(n, 1 + e) for n, e in zip(dims, (7, 5, 13)[:nd])], 1),
            ([0] * nd, list(dims), 2),
            ([2] * nd, last, 3),
            ([1] * nd, list(dims), 7)]


# every inference kernel family: 22 features (one tile), 65 (three tiles, three channels), 256 (k_fused<8>), 527 (k_lean, run-time tile
# count, 2-D), 1100 (k_wide, through the scratch), bf16 256 and 512 (k16; CO = 4 with three channels), split precision 128 (k_fused_x3)
@pytest.mark.parametrize("L,F,cin,cout,prec", [(4, 22, 3, 1, "fp32"), (3, 65, 3, 3, "fp32"), (5, 256, 3, 1, "fp32"), (3, 527, 2, 1, "fp32"),
                                               (3, 1100, 3, 1, "fp32"), (4, 256, 3, 1, "bf16"), (3, 512, 2, 3, "bf16"), (4, 128, 3, 1, "bf16x3")])
def test_box_equals_slice_of_the_grid_decode(L, F, cin, cout, prec):
    m = _net(L, F, cin, cout, prec, seed=F)
    dims = (19, 23, 29) if cin == 3 else (67, 91)
    kinds = ("f32", "u8", "u16") if F in (22, 256, 527) else ("f32", "u16")
    for kind in kinds:
        kw = {} if kind == "f32" else EPI
        full = m.decode_grid(dims, out_kind=kind, **kw).view(*dims, cout)
        for b, e, s in _boxes(dims):
            got = m.decode_box(dims, b, e, s, out_kind=kind, **kw)
            want = full[tuple(slice(x, y, s) for x, y in zip(b, e))]
            assert got.shape == want.shape and got.dtype == want.dtype
            assert torch.equal(got, want), (kind, b, e, s)
        # chunked calls (offset / n) give what one call gives
        one = m.decode_box(dims, [1] * len(dims), list(dims), 2, out_kind=kind, **kw)
        assert torch.equal(m.decode_box(dims, [1] * len(dims), list(dims), 2, out_kind=kind, chunk=333, **kw), one)


def _forward_box(m, dims, start, step, extent, offset, n, ws=None):
    box = _lib.GridBox()
    box.grid = SIREN._grid(dims, -1.0, 1.0)
    for a in range(len(dims)):
        box.start[a], box.step[a], box.extent[a] = start[a], step[a], extent[a]
    out = torch.empty((n, m.data_channel), dtype=torch.float32, device=DEV)
    m.sync_packed()
    p, nb = ws if ws is not None else m._forward_scratch(n)
    rc = _lib.lib().brief_siren_forward_box(C.byref(m.desc), _lib.ptr(m.packed), C.byref(box), offset, n, _lib.ptr(out), _lib.OUT_F32,
                                            0.0, 1.0, 0.0, 1.0, p, nb, _lib.stream_ptr())
    return rc, out


@pytest.mark.parametrize("L,F,prec", [(4, 65, "fp32"), (5, 256, "fp32"), (3, 256, "bf16")])
def test_boxes_of_a_grid_beyond_2_32_voxels(L, F, prec):
    """a virtual 2048^3 grid (2^33 voxels, never decoded whole): boxes at the origin, across flattened index 2^32 and at the far corner
    equal forward() on the oracle's coordinates of the same voxels; a chunk of a box of 2^32 voxels or more takes the 64-bit split"""
    m = _net(L, F, 3, 1, prec, seed=7)
    dims = (2048, 2048, 2048)
    for b, e, s in [((0, 0, 0), (4, 5, 7), 1), ((1023, 2046, 2040), (1025, 2048, 2048), 1), ((2041, 2040, 2030), (2048, 2048, 2048), 3),
                    ((1000, 0, 5), (1048, 2048, 2048), (16, 97, 301))]:
        got = m.decode_box(dims, b, e, s)
        ax = [np.arange(x, y, s if np.isscalar(s) else s[i]) for i, (x, y) in enumerate(zip(b, e))]
        idx = np.ravel_multi_index(np.meshgrid(*ax, indexing="ij"), dims).reshape(-1)
        want = m.forward(torch.from_numpy(O.grid_coords(dims, idx=idx)).to(DEV)).view(got.shape)
        assert torch.equal(got, want), (b, e, s)
    # the whole 2^33-voxel grid as a box; a call of 300 samples around box index 2^32 (and one at the very end)
    for off in ((1 << 32) - 150, (1 << 33) - 300):
        rc, got = _forward_box(m, dims, (0, 0, 0), (1, 1, 1), dims, off, 300)
        assert rc == 0, _lib.lib().brief_last_error()
        want = m.forward(torch.from_numpy(O.grid_coords(dims, idx=np.arange(off, off + 300))).to(DEV))
        assert torch.equal(got, want)
    # a strided box of 2^32 voxels (2048 x 2048 x 1024, every second w from 1): the 64-bit split, box indices above 2^31
    rc, got = _forward_box(m, dims, (0, 0, 1), (1, 1, 2), (2048, 2048, 1024), (1 << 32) - 207, 200)
    assert rc == 0, _lib.lib().brief_last_error()
    i = np.unravel_index(np.arange((1 << 32) - 207, (1 << 32) - 7), (2048, 2048, 1024))
    idx = np.ravel_multi_index((i[0], i[1], 1 + 2 * i[2]), dims)
    assert torch.equal(got, m.forward(torch.from_numpy(O.grid_coords(dims, idx=idx)).to(DEV)))


def test_resampled_views_equal_forward_on_the_same_linspace():
    m = _net(4, 65, 3, 1, seed=3)
    for shape in ((2 * 24 - 1, 32, 40), (37, 101, 9)):
        b, e, s = (2, 3, 1), (shape[0], shape[1] - 1, shape[2]), 2
        got = m.decode_box(shape, b, e, s)
        ax = [np.arange(x, y, s) for x, y in zip(b, e)]
        idx = np.ravel_multi_index(np.meshgrid(*ax, indexing="ij"), shape).reshape(-1)
        want = m.forward(torch.from_numpy(O.grid_coords(shape, idx=idx)).to(DEV)).view(got.shape)
        assert torch.equal(got, want), shape


def test_forward_box_refusals():
    m = _net(3, 64, 3, 1)
    L = _lib.lib()
    dims = (8, 9, 10)
    for start, step, extent, off, n, what in [((0, 0, 0), (1, 1, 1), (8, 9, 11), 0, 1, "exceeds the grid"),
                                              ((0, 0, 0), (0, 1, 1), (1, 1, 1), 0, 1, "step"),
                                              ((0, 0, 0), (1, 1, 1), (0, 1, 1), 0, 1, "extent"),
                                              ((0, 1, 0), (1, 4, 1), (8, 3, 10), 0, 1, "exceeds the grid"),
                                              ((-1, 0, 0), (1, 1, 1), (1, 1, 1), 0, 1, "exceeds the grid"),
                                              ((0, 0, 0), (1, 1, 1), (2, 2, 2), 5, 4, "offset + n"),
                                              ((0, 0, 0), (1, 1, 1), (2, 2, 2), -1, 2, "offset + n"),
                                              ((0, 0, 0), (1, 1, 1), (2, 2, 2), 0, 0, "empty")]:
        rc, _ = _forward_box(m, dims, start, step, extent, off, max(n, 1)) if n > 0 else (None, None)
        if n == 0:
            box = _lib.GridBox()
            box.grid = SIREN._grid(dims, -1.0, 1.0)
            for a in range(3):
                box.start[a], box.step[a], box.extent[a] = start[a], step[a], extent[a]
            out = torch.empty(8, device=DEV)
            rc = L.brief_siren_forward_box(C.byref(m.desc), _lib.ptr(m.packed), C.byref(box), 0, 0, _lib.ptr(out), 0, 0.0, 1.0, 0.0, 1.0,
                                           None, 0, _lib.stream_ptr())
        assert rc == -1 and what in L.brief_last_error().decode(), (start, step, extent, off, n, L.brief_last_error())
    # grid.ndim must equal cin; dims of 2^31 refused
    rc, _ = _forward_box(m, (8, 9), (0, 0), (1, 1), (2, 2), 0, 1)
    assert rc == -1 and "ndim" in L.brief_last_error().decode()
    rc, _ = _forward_box(m, (1 << 31, 4, 4), (0, 0, 0), (1, 1, 1), (1, 1, 1), 0, 1)
    assert rc == -1 and "2^31" in L.brief_last_error().decode()
    # more than 1024 features without the scratch: BRIEF_ERR_WORKSPACE
    w = _net(3, 1100, 3, 1)
    rc, _ = _forward_box(w, dims, (0, 0, 0), (1, 1, 1), dims, 0, 100, ws=(None, 0))
    assert rc == -3 and "scratch" in L.brief_last_error().decode()
    with pytest.raises(ValueError):
        m.decode_box(dims, (0, 0, 0), (9, 9, 10))
    with pytest.raises(ValueError):
        m.decode_box(dims, (0, 0, 0), (8, 9, 10), (1, -1, 1))


# ---- framework ------------------------------------------------------------------------------------------------------------------
def _single_opt(tmp_path, steps, given):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    cf = opt.CompressFramework
    cf.Compress.max_steps = steps
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = given
    cf.Compress.loss_log_freq = steps
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp_path / "outputs")
    opt.Log.time = False
    return opt


_REGIONS = [((slice(None),) * 3, 1), ((slice(3, 17), slice(0, 31), slice(20, 40)), 1), ((slice(1, 24), slice(2, 30), slice(0, 40)), 3),
            ((slice(23, 24), slice(31, 32), slice(39, 40)), 1), ((slice(0, 24), slice(5, 6), slice(None)), 7)]


@pytest.fixture(scope="module")
def single_artefact(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("single")
    vol = make_volume((24, 32, 40), seed=11)
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, 30, 4.0 * SIREN.calc_param_count(3, 1, 40, 5))
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    NFGR(opt.CompressFramework, Log=Log).compress(path)
    cdir = os.path.join(Log.logdir, "steps30", "compressed")
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    return opt, cdir, yml


def test_singletask_region_equals_slice_of_decompress(single_artefact, tmp_path):
    opt, cdir, _ = single_artefact
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    whole = NFGR.decompress(opt, mod, side)
    assert whole.dtype == np.uint16
    for reg, step in _REGIONS:
        got = NFGR.decompress_region(opt, mod, side, reg, step)
        want = whole[tuple(slice(r.start, r.stop, step) for r in reg)]
        assert got.dtype == want.dtype and np.array_equal(got, want), (reg, step)
    # the host branch: another normalisation of the same artefact (f32 decode + invnormalize_data), and a narrowing clip
    o2 = config.to_opt(config.to_plain(opt))
    o2.CompressFramework.Normalize.name = "minmax01"
    o2.CompressFramework.Decompress.postprocess.clip = [100, 30000]
    whole2 = NFGR.decompress(o2, mod, side)
    for reg, step in _REGIONS[1:3]:
        assert np.array_equal(NFGR.decompress_region(o2, mod, side, reg, step), whole2[tuple(slice(r.start, r.stop, step) for r in reg)])
    # resampled views: the region of the u16 decode of the net on another linspace grid
    from brief_pytorch_amd.modelsave import load_model
    sd = config.load(side)
    phi = SIREN(coords_channel=3, data_channel=1, features=sd["phi_features"], layers=5, w0=20)
    load_model(phi, mod, "cpu")
    phi.to(DEV)
    for shape in ((47, 32, 40), (30, 17, 55)):
        full = phi.decode_grid(shape, out_kind="u16", scale=(0.0, 100.0), vrange=(sd["min"], sd["max"])).view(*shape, 1).cpu().numpy()
        reg = (slice(1, shape[0]), slice(0, shape[1] - 2), slice(3, shape[2]))
        got = NFGR.decompress_region(opt, mod, side, reg, 2, shape=shape)
        assert np.array_equal(got, full[tuple(slice(r.start, r.stop, 2) for r in reg)]), shape
    # a denoise through a binary opening is not local to a voxel: refused
    o3 = config.to_opt(config.to_plain(opt))
    o3.CompressFramework.Decompress.postprocess.denoise.level = 500
    with pytest.raises(ValueError, match="not local"):
        NFGR.decompress_region(o3, mod, side, _REGIONS[1][0])
    with pytest.raises(ValueError):
        NFGR.decompress_region(opt, mod, side, (slice(0, 25), slice(None), slice(None)))


def test_singletask_region_of_a_float32_artefact(tmp_path):
    """float32 data: always the host branch (f32 decode, invnormalize_data, threshold + clip of the postprocess)"""
    m = _net(4, 48, 3, 1, seed=5)
    mod = str(tmp_path / "module")
    save_model(m, mod)
    side = {"dtype": "float32", "min": -20.0, "max": 900.0, "normalized_min": 0.0, "normalized_max": 100.0, "data_shape": [20, 21, 22, 1],
            "phi_features": 48, "phi_name": "SIREN"}
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    opt.CompressFramework.Module.phi.layers = 4
    # a normalisation range inside the net's output range, so that both clips (invnormalize's and the postprocess's) act
    y = m.decode_grid((20, 21, 22)).cpu().numpy()
    opt.CompressFramework.Normalize.name = "minmaxany_%r_%r" % (float(np.percentile(y, 30)), float(np.percentile(y, 70)))
    opt.CompressFramework.Decompress.postprocess.clip = [0, 500]
    whole = NFGR.decompress(opt, mod, dict(side))
    assert whole.dtype == np.float32 and (whole == 0).any() and (whole == 500).any()
    for reg, step in [((slice(None),) * 3, 1), ((slice(2, 19), slice(0, 21), slice(5, 22)), 3), ((slice(19, 20), slice(20, 21), slice(0, 22)), 2)]:
        got = NFGR.decompress_region(opt, mod, dict(side), reg, step)
        assert np.array_equal(got, whole[tuple(slice(r.start, r.stop, step) for r in reg)]), (reg, step)


def _divide(tmp_path, vol, divide_type, steps, given, ext=".tif", mutate=None):
    path = str(tmp_path / ("d" + ext))
    save_img(path, vol)
    opt = _single_opt(tmp_path, steps, given)
    cf = opt.CompressFramework
    cf.Compress.divide.divide_type = divide_type
    cf.Compress.divide.param_alloc = "by_size"
    if mutate is not None:
        mutate(cf)
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    fw.compress_divide(path, opt)
    return fw, opt, os.path.join(Log.logdir, "steps%d" % steps, "compressed")


@pytest.mark.parametrize("kind", ["uniform", "adaptive"])
def test_dividetask_region_equals_slice_of_decompress_divide(tmp_path, kind):
    if kind == "uniform":
        vol = make_volume((21, 26, 30), seed=3)                                  # total_2_2_2 with remainder blocks
        fw, opt, cdir = _divide(tmp_path, vol, "total_2_2_2", 20, 40000.0)
        regions = [((slice(None),) * 3, 1), ((slice(5, 16), slice(10, 20), slice(12, 19)), 1), ((slice(0, 21), slice(1, 26), slice(2, 30)), 3),
                   ((slice(9, 11), slice(12, 14), slice(14, 16)), 1), ((slice(10, 11), slice(None), slice(None)), 7)]
    else:
        vol = make_volume((32, 48, 48), seed=52)
        vol[16:32, 24:48, 24:48] = 0                                             # pruned: no block covers it
        fw, opt, cdir = _divide(tmp_path, vol, "adaptive_-1_-1_0_0_20", 20, 90000.0)
        regions = [((slice(None),) * 3, 1), ((slice(8, 30), slice(20, 40), slice(20, 44)), 1), ((slice(1, 32), slice(0, 48), slice(3, 47)), 3),
                   ((slice(15, 17), slice(23, 25), slice(23, 25)), 1)]
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    whole = fw.decompress_divide(*args)
    if kind == "adaptive":
        assert (whole[16:32, 24:48, 24:48] == 0).all()
    for reg, step in regions:
        got = fw.decompress_divide_region(*args, reg, step)
        assert np.array_equal(got, whole[tuple(slice(r.start, r.stop, step) for r in reg)]), (reg, step)
    with pytest.raises(ValueError):
        fw.decompress_divide_region(*args, regions[1][0], 1, shape=(40, 40, 40))


def test_dividetask_region_2d(tmp_path):
    """a 2-D RGB image (coords_channel 2, data_channel 3, uint8 .png) in 2 x 3 blocks with remainders"""
    rng = np.random.default_rng(9)
    yy, xx = np.meshgrid(np.linspace(0, 1, 50), np.linspace(0, 1, 61), indexing="ij")
    img = np.stack([120 + 100 * np.sin(6 * xx + 2 * yy), 128 + 90 * np.cos(5 * yy), 100 + 80 * np.sin(4 * (xx + yy))], -1)
    img = np.clip(img + rng.normal(0, 2, img.shape), 0, 255).astype(np.uint8)

    def rgb(cf):
        cf.Module.phi.coords_channel, cf.Module.phi.data_channel, cf.Module.phi.layers = 2, 3, 4
        cf.Compress.preprocess.clip = [0, 255]
        cf.Decompress.postprocess.clip = [0, 255]
        cf.Compress.loss.weight = ["value_255_255_1"]
        cf.Compress.loss.weight_thres = 255
    fw, opt, cdir = _divide(tmp_path, img, "total_2_3", 20, 20000.0, ext=".png", mutate=rgb)
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    whole = fw.decompress_divide(*args)
    for reg, step in [((slice(None),) * 2, 1), ((slice(10, 40), slice(15, 50)), 1), ((slice(1, 50), slice(0, 61)), 3)]:
        assert np.array_equal(fw.decompress_divide_region(*args, reg, step), whole[tuple(slice(r.start, r.stop, step) for r in reg)])


def test_cli_writes_the_region(single_artefact, tmp_path):
    opt, cdir, yml = single_artefact
    whole = NFGR.decompress(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"))
    for out, region, step in ((str(tmp_path / "roi.npy"), "2:20,5:30,1:39", 2), (str(tmp_path / "roi.tif"), "0:24,:,7:8", 1)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", region, "--step", str(step),
                            "-o", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "shape" in r.stdout and "uint16" in r.stdout
        sl = tuple(slice(int(a) if a else None, int(b) if b else None, step) for a, b in (p.split(":") for p in region.split(",")))
        got = read_img(out)
        want = whole[sl]
        assert np.array_equal(got.reshape(want.shape), want)
