"""Error-bounded mode on the GPU: brief_correct_count / _emit / _apply against their numpy restatement (exact, in values and in order),
and the bound itself through NFGR.compress / decompress / decompress_region / compress_divide: max |x - x^| <= eps, exactly."""
import csv
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, config, corrections
from brief_pytorch_amd.framework import NFGR, MyLogger
from brief_pytorch_amd.io import get_folder_size
from brief_pytorch_amd.networks import FFN, SIREN
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(dtype, n, kind, seed):
    """(decoded, source) host arrays: kind 'none' (no outliers at any bound), 'all' (every element off by more than the bound the
    case uses), 'mixed' (small noise, sparse far outliers, both ends of the range)"""
    rng = np.random.default_rng(seed)
    tmax = np.iinfo(dtype).max
    src = rng.integers(0, tmax + 1, n).astype(dtype)
    if kind == "none":
        return src.copy(), src
    if kind == "all":
        off = rng.integers(20, 60, n) * rng.choice([-1, 1], n)
        dec = src.astype(np.int64) + off
        dec = np.where((dec < 0) | (dec > tmax), src.astype(np.int64) - off, dec)      # reflected back into range: still off by >= 20
        return dec.astype(dtype), src
    noise = rng.integers(-12, 13, n)
    far = (rng.random(n) < 0.01) * rng.integers(-tmax, tmax + 1, n)
    return np.clip(src.astype(np.int64) + noise + far, 0, tmax).astype(dtype), src


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _chunk(dtype):
    return int(_lib.lib().brief_correct_chunk_elems(np.dtype(dtype).itemsize))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_find_equals_numpy_exactly(dtype):
    per = _chunk(dtype)
    assert per == 32768 // np.dtype(dtype).itemsize
    sizes = [1, 63, 64, 4097, per - 1, per, per + 1, 3 * per, 3_000_017]
    for n in sizes:
        for kind, eps in (("none", 0), ("none", 5), ("all", 0), ("all", 19), ("mixed", 0), ("mixed", 3), ("mixed", 12), ("mixed", 200)):
            dec, src = _pair(dtype, n, kind, seed=n % 1000 + eps)
            want_i, want_q = corrections.find_host(dec, src, eps)
            if kind == "none":
                assert want_i.size == 0
            if kind == "all":
                assert want_i.size == n
            idx, q = corrections.find(_dev(dec), _dev(src), eps)
            assert idx.dtype == torch.int64 and q.dtype == torch.int32
            assert np.array_equal(idx.cpu().numpy(), want_i), (n, kind, eps)
            assert np.array_equal(q.cpu().numpy(), want_q), (n, kind, eps)
    # the arrays "at" an offset above 2^32 of a larger volume: the same code path a volume of that size takes
    for n, base in ((4097, (1 << 32) + 12345), (2 * per + 77, (1 << 39) + 1), (1000, (1 << 40) - 1000)):
        dec, src = _pair(dtype, n, "mixed", seed=5)
        want_i, want_q = corrections.find_host(dec, src, 4, base=base)
        assert want_i.size and want_i.max() >= 1 << 32
        idx, q = corrections.find(_dev(dec), _dev(src), 4, base=base)
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(q.cpu().numpy(), want_q)
    # views that do not start on a 16-byte boundary are handled (copied) by the binding
    dec, src = _pair(dtype, 10000, "mixed", seed=6)
    idx, q = corrections.find(_dev(dec)[3:], _dev(src)[3:], 2)
    want_i, want_q = corrections.find_host(dec[3:], src[3:], 2)
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(q.cpu().numpy(), want_q)


def test_c_abi_refusals_name_the_limit():
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.uint16, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    for args, what in (((_lib.ptr(a), _lib.ptr(a), 4, 64, 0, 0), "elem_bytes"), ((_lib.ptr(a), _lib.ptr(a), 2, 0, 0, 0), "n >= 1"),
                       ((_lib.ptr(a), _lib.ptr(a), 2, 64, 65536, 0), "bound"), ((_lib.ptr(a), _lib.ptr(a), 2, 64, 0, (1 << 40) - 63), "2^40"),
                       ((_lib.ptr(a[1:]), _lib.ptr(a), 2, 63, 0, 0), "aligned"), ((None, _lib.ptr(a), 2, 64, 0, 0), "null")):
        assert L.brief_correct_count(*args, _lib.ptr(cnt), st) == -1 and what in L.brief_last_error().decode(), what
    assert L.brief_correct_chunk_elems(3) == -1
    with pytest.raises(corrections.CorrectionsError):
        corrections.find(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), 1)
    with pytest.raises(corrections.CorrectionsError):
        corrections.find(a, a[:10], 1)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_apply_equals_numpy_with_saturation(dtype):
    rng = np.random.default_rng(3)
    tmax = np.iinfo(dtype).max
    for n, eps, base in ((1, 0, 0), (5000, 3, 0), (70001, 100 if dtype == np.uint16 else 9, (1 << 33) + 5)):
        out = rng.integers(0, tmax + 1, n).astype(dtype)
        k = max(1, n // 3)
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64) + base
        qmax = tmax // (2 * eps + 1) + 2                      # far enough to run into both ends of the range
        q = rng.integers(-qmax, qmax + 1, k).astype(np.int32)
        want = corrections.apply_host(out, idx, q, eps, base=base)
        assert (want == 0).any() and (want == tmax).any() or n == 1
        t = _dev(out)
        got = corrections.apply(t, _dev(idx), _dev(q), eps, base=base)
        assert got is t and np.array_equal(t.cpu().numpy(), want)
        # host arrays are taken too
        t2 = _dev(out)
        corrections.apply(t2, idx, q, eps, base=base)
        assert np.array_equal(t2.cpu().numpy(), want)
    # find + apply: the bound holds, eps = 0 restores the source
    for eps in (0, 1, 7):
        dec, src = _pair(dtype, 200003, "mixed", seed=eps)
        t = _dev(dec)
        idx, q = corrections.find(t, _dev(src), eps)
        corrections.apply(t, idx, q, eps)
        err = np.abs(t.cpu().numpy().astype(np.int64) - src.astype(np.int64)).max()
        assert err <= eps and corrections.max_abs_diff(t, _dev(src)) == err
        if eps == 0:
            assert np.array_equal(t.cpu().numpy(), src)
    # indices outside [base, base + n) are never written
    t = _dev(np.full(16, 7, dtype))
    corrections.apply(t, np.array([-1, 16, 99], np.int64), np.array([1, 1, 1], np.int32), 0)
    assert (t.cpu().numpy() == 7).all()


def test_find_is_reproducible():
    dec, src = _pair(np.uint16, 5_000_011, "mixed", seed=9)
    a, b = _dev(dec), _dev(src)
    i0, q0 = corrections.find(a, b, 5)
    for _ in range(3):
        i1, q1 = corrections.find(a, b, 5)
        assert torch.equal(i0, i1) and torch.equal(q0, q1)
    assert i0.numel() > 1000 and bool((i0[1:] > i0[:-1]).all())


# ---- framework ------------------------------------------------------------------------------------------------------------------
def _single_opt(tmp_path, tag, steps, given, eps, yaml="default.yaml"):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", yaml))
    cf = opt.CompressFramework
    cf.Compress.max_steps = steps
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = given
    cf.Compress.loss_log_freq = steps
    if eps is not None:
        cf.Compress.error_bound = eps
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp_path / ("outputs_" + tag))
    opt.Log.time = False
    return opt


def _metrics(logdir):
    with open(os.path.join(logdir, "metrics.csv")) as f:
        return {r["name"]: float(r["value"]) for r in csv.DictReader(f)}


def _same_tree(a, b):
    cmp = filecmp.dircmp(a, b)
    if cmp.left_only or cmp.right_only or cmp.funny_files:
        return False
    _, mismatch, errors = filecmp.cmpfiles(a, b, cmp.common_files, shallow=False)
    return not mismatch and not errors and all(_same_tree(os.path.join(a, d), os.path.join(b, d)) for d in cmp.common_dirs)


STEPS = 1500
_REGIONS = [((slice(None),) * 3, 1), ((slice(3, 17), slice(0, 31), slice(20, 40)), 1), ((slice(1, 24), slice(2, 30), slice(0, 40)), 3),
            ((slice(23, 24), slice(31, 32), slice(39, 40)), 1), ((slice(0, 24), slice(5, 6), slice(None)), 7), ((slice(7, 8), slice(None), slice(None)), 1)]


def _run_single(tmp_path, vol, path, eps, tag, yaml="default.yaml", given=None):
    opt = _single_opt(tmp_path, tag, STEPS, given or 4.0 * SIREN.calc_param_count(3, 1, 40, 5), eps, yaml)
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    res = NFGR(opt.CompressFramework, Log=Log).compress(path)
    return opt, Log.logdir, os.path.join(Log.logdir, "steps%d" % STEPS, "compressed"), res


def test_singletask_bound_holds_exactly(tmp_path):
    """a 24 x 32 x 40 volume with N(0, 200) noise and a 40-wide SIREN after 1500 steps: the plain decode is hundreds of grey levels
    off in places (the net cannot fit the noise), so every bound below leaves work for the corrections (asserted: the test cannot
    pass vacuously)"""
    vol = make_volume((24, 32, 40), seed=11)
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    _, plain_log, plain_dir, plain_res = _run_single(tmp_path, vol, path, None, "off")
    assert not os.path.exists(os.path.join(plain_dir, "corrections.bin"))
    plain_side = config.load(os.path.join(plain_dir, "sideinfos.yaml"))
    assert "error_bound" not in plain_side and "corrections" not in plain_side and "max_abs_error" not in plain_res[STEPS]
    orig_bytes = os.path.getsize(path)
    for eps in (0, 50, 400):
        opt, logdir, cdir, res = _run_single(tmp_path, vol, path, eps, "eps%d" % eps)
        mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
        # the weights do not know about the mode: byte-equal to the run of the same seed without the key
        assert _same_tree(mod, os.path.join(plain_dir, "module"))
        side = config.load(side_path)
        cpath = os.path.join(cdir, "corrections.bin")
        assert os.path.isfile(cpath) and side["error_bound"] == eps
        assert side["corrections"]["bytes"] == os.path.getsize(cpath)
        idx, q, head = corrections.read(cpath)
        assert side["corrections"]["count"] == head["count"] == idx.size and head["bound"] == eps and head["n"] == vol.size
        # every reported ratio counts the corrections
        m = _metrics(logdir)
        assert m["compress_ratio/actual"] == pytest.approx(orig_bytes / (os.path.getsize(side_path) + get_folder_size(mod) + os.path.getsize(cpath)), rel=1e-12)
        assert m["compress_ratio/actual"] < _metrics(plain_log)["compress_ratio/actual"]
        assert m["compress_ratio/theory"] < _metrics(plain_log)["compress_ratio/theory"]
        # without corrections the stored weights violate the bound ...
        raw = NFGR._decode_integer(opt.CompressFramework, mod, side).cpu().numpy().reshape(vol.shape)
        raw_err = np.abs(raw.astype(np.int64) - vol.astype(np.int64))
        assert raw_err.max() > eps and idx.size == int((raw_err > eps).sum()) > 0
        # ... with them it holds, exactly
        dec = NFGR.decompress(opt, mod, side_path)
        assert dec.dtype == vol.dtype and dec.shape == vol.shape
        err = np.abs(dec.astype(np.int64) - vol.astype(np.int64)).max()
        print("eps %d: K = %d, corrections %d bytes, max error before %d, after %d" % (eps, idx.size, os.path.getsize(cpath), raw_err.max(), err))
        assert err <= eps
        if eps == 0:
            assert np.array_equal(dec, vol)
        # the evaluation reused the corrected decode: same numbers, same file
        assert res[STEPS]["max_abs_error"] == err == m["max_abs_error"]
        assert np.array_equal(read_img(os.path.join(logdir, "steps%d" % STEPS, "decompressed", "vol_decompressed.tif")).reshape(vol.shape), dec)
        with open(os.path.join(logdir, "performance.csv")) as f:
            assert "max_abs_error" in f.readline()
        # regions of the corrected artefact: the slice of the whole decode, bit for bit
        for reg, step in _REGIONS:
            got = NFGR.decompress_region(opt, mod, side_path, reg, step)
            want = dec[tuple(slice(r.start, r.stop, step) for r in reg)]
            assert got.dtype == want.dtype and np.array_equal(got, want), (eps, reg, step)
        with pytest.raises(ValueError, match="resampled"):
            NFGR.decompress_region(opt, mod, side_path, _REGIONS[1][0], 1, shape=(30, 30, 30))
        # a decoder that finds the promise but not the file raises
        os.rename(cpath, cpath + ".away")
        with pytest.raises(corrections.CorrectionsError, match="corrections.bin"):
            NFGR.decompress(opt, mod, side_path)
        os.rename(cpath + ".away", cpath)
    with open(os.path.join(plain_log, "performance.csv")) as f:
        assert "max_abs_error" not in f.readline()


def test_singletask_cli_region_and_unevaluated_checkpoint(tmp_path):
    """decompress.py --region on a corrected artefact; the correction step runs whether or not the checkpoint is evaluated"""
    vol = make_volume((24, 32, 40), seed=11)
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, "noeval", STEPS, 4.0 * SIREN.calc_param_count(3, 1, 40, 5), 20)
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    res = NFGR(opt.CompressFramework, Log=Log).compress(path, evaluate=False)
    assert res == {}
    cdir = os.path.join(Log.logdir, "steps%d" % STEPS, "compressed")
    assert os.path.isfile(os.path.join(cdir, "corrections.bin"))
    whole = NFGR.decompress(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"))
    assert np.abs(whole.astype(np.int64) - vol.astype(np.int64)).max() <= 20
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    out = str(tmp_path / "roi.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", "2:20,5:30,1:39", "--step", "2", "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = whole[2:20:2, 5:30:2, 1:39:2]
    assert np.array_equal(read_img(out).reshape(want.shape), want)


def test_uint8_multichannel_image(tmp_path):
    """2-D RGB uint8 (coords_channel 2, data_channel 3): the corrections index elements, channels included"""
    rng = np.random.default_rng(9)
    yy, xx = np.meshgrid(np.linspace(0, 1, 50), np.linspace(0, 1, 61), indexing="ij")
    img = np.stack([120 + 100 * np.sin(6 * xx + 2 * yy), 128 + 90 * np.cos(5 * yy), 100 + 80 * np.sin(4 * (xx + yy))], -1)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    path = str(tmp_path / "img.png")
    save_img(path, img)
    for eps in (0, 4):
        opt = _single_opt(tmp_path, "rgb%d" % eps, STEPS, 20000.0, eps)
        cf = opt.CompressFramework
        cf.Module.phi.coords_channel, cf.Module.phi.data_channel, cf.Module.phi.layers = 2, 3, 4
        cf.Compress.preprocess.clip = [0, 255]
        cf.Decompress.postprocess.clip = [0, 255]
        cf.Compress.loss.weight = ["value_255_255_1"]
        cf.Compress.loss.weight_thres = 255
        Log = MyLogger(**opt.Log)
        torch.manual_seed(1)
        res = NFGR(cf, Log=Log).compress(path)
        cdir = os.path.join(Log.logdir, "steps%d" % STEPS, "compressed")
        mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
        raw = NFGR._decode_integer(cf, mod, config.load(side)).cpu().numpy().reshape(img.shape)
        assert np.abs(raw.astype(int) - img.astype(int)).max() > eps
        dec = NFGR.decompress(opt, mod, side)
        assert dec.dtype == np.uint8 and np.abs(dec.astype(int) - img.astype(int)).max() <= eps and res[STEPS]["max_abs_error"] <= eps
        if eps == 0:
            assert np.array_equal(dec, img)
        for reg, step in (((slice(None),) * 2, 1), ((slice(10, 40), slice(15, 50)), 1), ((slice(1, 50), slice(0, 61)), 3), ((slice(49, 50), slice(None)), 1)):
            assert np.array_equal(NFGR.decompress_region(opt, mod, side, reg, step), dec[tuple(slice(r.start, r.stop, step) for r in reg)])


def test_unsupported_data_is_refused_at_prepare_fit(tmp_path):
    vol = make_volume((12, 16, 20), seed=2)
    path = str(tmp_path / "v.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, "refuse", 10, 8000.0, 3)
    opt.CompressFramework.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmax01"):
        NFGR(opt.CompressFramework, Log=MyLogger(**opt.Log)).compress(path)
    opt = _single_opt(tmp_path, "refuse2", 10, 8000.0, 3)
    opt.CompressFramework.Decompress.postprocess.clip = [0, 30000]
    with pytest.raises(ValueError, match="postprocess"):
        NFGR(opt.CompressFramework, Log=MyLogger(**opt.Log)).compress(path)
    opt = _single_opt(tmp_path, "refuse3", 10, 8000.0, 3)
    with pytest.raises(ValueError, match="float32"):
        NFGR(opt.CompressFramework, Log=MyLogger(**opt.Log)).compress(path, data=vol.astype(np.float32))


@pytest.mark.parametrize("eps", [0, 60])
def test_dividetask_bound_holds_on_the_merged_volume(tmp_path, eps):
    vol = make_volume((21, 26, 30), seed=3)                                  # total_2_2_2 with remainder blocks
    path = str(tmp_path / "d.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, "div", 600, 40000.0, eps)
    cf = opt.CompressFramework
    cf.Compress.divide.divide_type = "total_2_2_2"
    cf.Compress.divide.param_alloc = "by_size"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    res = fw.compress_divide(path, opt)
    cdir = os.path.join(Log.logdir, "steps600", "compressed")
    blocks = sorted(os.listdir(os.path.join(cdir, "module")))
    assert len(blocks) == 12                  # 21 x 26 x 30 in blocks of 10 x 13 x 15: 3 x 2 x 2
    total = 0
    for b in blocks:
        assert sorted(os.listdir(os.path.join(cdir, "module", b))) == ["corrections.bin", "module"]
        side = config.load(os.path.join(cdir, "sideinfos", b, "sideinfos.yaml"))
        assert side["error_bound"] == eps and side["corrections"]["bytes"] == os.path.getsize(os.path.join(cdir, "module", b, "corrections.bin"))
        total += side["corrections"]["count"]
    assert total > 0, "the fit must leave work for the corrections, or the bound is vacuous"
    # the z-sharded evaluation (the _decode_slab path) saw the bound hold
    assert res[600]["max_abs_error"] <= eps
    m = _metrics(Log.logdir)
    assert m["max_abs_error"] == res[600]["max_abs_error"]
    assert m["compress_ratio/actual"] == pytest.approx(os.path.getsize(path) / get_folder_size(cdir), rel=1e-12)
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    whole = fw.decompress_divide(*args)
    err = np.abs(whole.astype(np.int64) - vol.astype(np.int64)).max()
    assert err <= eps and err == res[600]["max_abs_error"]
    if eps == 0:
        assert np.array_equal(whole, vol)
    assert np.array_equal(read_img(os.path.join(Log.logdir, "steps600", "decompressed", "d_decompressed.tif")).reshape(vol.shape), whole)
    for reg, step in [((slice(None),) * 3, 1), ((slice(5, 16), slice(10, 20), slice(12, 19)), 1), ((slice(0, 21), slice(1, 26), slice(2, 30)), 3),
                      ((slice(9, 11), slice(12, 14), slice(14, 16)), 1), ((slice(10, 11), slice(None), slice(None)), 7)]:
        got = fw.decompress_divide_region(*args, reg, step)
        assert np.array_equal(got, whole[tuple(slice(r.start, r.stop, step) for r in reg)]), (reg, step)
    # a slab decode cut inside the blocks equals the merged volume's slices
    slab = fw._decode_slab(os.path.join(Log.logdir, "steps600"), [{"name": b} for b in blocks], 4, 17, list(vol.shape), vol.dtype)
    assert np.array_equal(slab.cpu().numpy(), whole[4:17])
    # a block that lost its corrections: the decoder raises
    os.remove(os.path.join(cdir, "module", blocks[3], "corrections.bin"))
    with pytest.raises(corrections.CorrectionsError, match="corrections.bin"):
        fw.decompress_divide(*args)


def test_the_mode_is_net_agnostic_ffn(tmp_path):
    """an FFN through the same path: the corrections act on decoded integers behind the net"""
    vol = make_volume((16, 24, 24), seed=5)
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, "ffn", STEPS, 4.0 * FFN.calc_param_count(3, 1, 48, embsize=256, layers=5), 30, yaml="ffn.yaml")
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    res = NFGR(opt.CompressFramework, Log=Log).compress(path)
    cdir = os.path.join(Log.logdir, "steps%d" % STEPS, "compressed")
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    assert config.load(side)["phi_name"] == "FFN" and config.load(side)["corrections"]["count"] > 0
    dec = NFGR.decompress(opt, mod, side)
    assert np.abs(dec.astype(np.int64) - vol.astype(np.int64)).max() <= 30 and res[STEPS]["max_abs_error"] <= 30
    reg = (slice(2, 15), slice(0, 24), slice(5, 20))
    assert np.array_equal(NFGR.decompress_region(opt, mod, side, reg, 2), dec[2:15:2, 0:24:2, 5:20:2])
