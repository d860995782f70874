"""Compress.quantize through NFGR: the artefact is module/quantized.bin, and every decode path reads it through load_model — whole,
region, max-intensity projections, error-bound corrections, DivideTask, init_net_path.  With the key absent or `none` nothing changes."""
import csv
import filecmp
import os

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, quantize
from brief_pytorch_amd.framework import NFGR, MyLogger
from brief_pytorch_amd.io import get_folder_size
from brief_pytorch_amd.misc import mip_ops
from brief_pytorch_amd.modelsave import load_model
from brief_pytorch_amd.networks import init_phi
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import save_img

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, STEPS, FT, BITS, GIVEN = (24, 40, 56), 60, 20, 8, 6000.0
QUANT = {"bits": BITS, "finetune_steps": FT}


def _opt(tmp, tag, quant="absent", eps=None, yaml="default.yaml"):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", yaml))
    cf = opt.CompressFramework
    cf.Compress.max_steps = STEPS
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = GIVEN
    cf.Compress.loss_log_freq = STEPS
    if quant != "absent":
        cf.Compress.quantize = config.to_opt(quant)
    if eps is not None:
        cf.Compress.error_bound = eps
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp / ("outputs_" + tag))
    opt.Log.time = False
    return opt


def _metrics(logdir):
    with open(os.path.join(logdir, "metrics.csv")) as f:
        return {r["name"]: float(r["value"]) for r in csv.DictReader(f)}


def _compress(opt, path, seed=1):
    Log = MyLogger(**opt.Log)
    torch.manual_seed(seed)
    res = NFGR(opt.CompressFramework, Log=Log).compress(path)
    return Log.logdir, os.path.join(Log.logdir, "steps%d" % STEPS, "compressed"), res


@pytest.fixture(scope="module")
def volume(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("quantize_fw")
    vol = make_volume(DIMS, seed=2)
    assert vol.dtype == np.uint16 and vol.shape == DIMS + (1,)
    path = str(tmp / "vol.tif")
    save_img(path, vol)
    return tmp, vol, path


@pytest.fixture(scope="module")
def single(volume):
    tmp, vol, path = volume
    opt = _opt(tmp, "q", QUANT)
    logdir, cdir, res = _compress(opt, path)
    return opt, logdir, cdir, res


def _loaded_net(opt, mod, side):
    cf = opt.CompressFramework
    phi = init_phi({**dict(cf.Module.phi), "features": side["phi_features"], "name": side["phi_name"]})
    return load_model(phi, mod).to("cuda")


def test_artefact_side_info_and_decodes(volume, single):
    tmp, vol, path = volume
    opt, logdir, cdir, res = single
    mod, side_path = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    assert os.listdir(mod) == [quantize.FILE_NAME]
    size = os.path.getsize(os.path.join(mod, quantize.FILE_NAME))
    assert size <= GIVEN
    side = config.load(side_path)
    assert dict(side["quantize"]) == {"bits": BITS, "tensors": 10}
    net = _loaded_net(opt, mod, side)
    assert size == quantize.overhead_bytes(5) + quantize.code_bytes(net.param_count, BITS)
    m = _metrics(logdir)
    assert m["compress_ratio/actual"] == pytest.approx(m["compress_ratio/theory"], rel=1e-12)      # the artefact spends what the budget rule counts
    assert m["compress_ratio/actual"] == pytest.approx(os.path.getsize(path) / (os.path.getsize(side_path) + size), rel=1e-12)
    # whole decode == the decode of the loaded net
    whole = NFGR.decompress(opt, mod, side_path)
    assert whole.dtype == np.uint16 and whole.shape == vol.shape
    want = net.decode_grid(list(DIMS), -1.0, 1.0, out_kind="u16", scale=(0.0, 100.0), vrange=(side["min"], side["max"]))
    assert np.array_equal(whole, want.cpu().numpy().reshape(vol.shape))
    assert STEPS in res and np.isfinite(res[STEPS]["psnr"])
    # a region == the slice of the whole decode
    for reg, step in (((slice(3, 17), slice(0, 31), slice(20, 40)), 1), ((slice(1, 24), slice(2, 30), slice(0, 56)), 3)):
        got = NFGR.decompress_region(opt, mod, side_path, reg, step)
        assert np.array_equal(got, whole[tuple(slice(r.start, r.stop, step) for r in reg)]), (reg, step)
    # projections == mip_ops of the decode
    for g, w in zip(NFGR.decompress_mip(opt, mod, side_path), mip_ops(whole)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    reg = (slice(2, 20), slice(5, 33), slice(7, 50))
    for g, w in zip(NFGR.decompress_mip(opt, mod, side_path, reg), mip_ops(whole[reg])):
        assert np.array_equal(g, w)


def test_init_net_path_onto_a_quantised_directory(volume, single):
    tmp, vol, path = volume
    opt0, _, cdir0, _ = single
    mod0 = os.path.join(cdir0, "module")
    opt = _opt(tmp, "init", QUANT)
    opt.CompressFramework.Compress.param.init_net_path = mod0
    torch.manual_seed(77)
    fw = NFGR(opt.CompressFramework, Log=MyLogger(**opt.Log))
    ctx = fw.prepare_fit(path)
    side = config.load(os.path.join(cdir0, "sideinfos.yaml"))
    assert torch.equal(ctx["phi"].params, _loaded_net(opt0, mod0, side).params)


def test_error_bound_on_a_quantised_artefact(volume):
    tmp, vol, path = volume
    eps = 300
    opt = _opt(tmp, "eb", QUANT, eps=eps)
    logdir, cdir, res = _compress(opt, path)
    assert sorted(os.listdir(cdir)) == ["corrections.bin", "module", "sideinfos.yaml"] and os.listdir(os.path.join(cdir, "module")) == [quantize.FILE_NAME]
    assert res[STEPS]["max_abs_error"] <= eps
    side = config.load(os.path.join(cdir, "sideinfos.yaml"))
    assert side["corrections"]["count"] > 0, "the fit must leave work for the corrections, or the bound is vacuous"
    dec = NFGR.decompress(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"))
    assert np.abs(dec.astype(np.int64) - vol.astype(np.int64)).max() <= eps


def test_dividetask_round_trips(volume):
    tmp, vol, path = volume
    opt = _opt(tmp, "div", QUANT)
    cf = opt.CompressFramework
    cf.Compress.param.given_size = 4 * GIVEN
    cf.Compress.divide.divide_type = "every_24_20_28"                          # 1 x 2 x 2 blocks
    cf.Compress.divide.param_alloc = "by_size"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    res = fw.compress_divide(path, opt)
    cdir = os.path.join(Log.logdir, "steps%d" % STEPS, "compressed")
    blocks = sorted(os.listdir(os.path.join(cdir, "module")))
    assert len(blocks) == 4
    total = 0
    for b in blocks:
        assert os.listdir(os.path.join(cdir, "module", b)) == ["module"] and os.listdir(os.path.join(cdir, "module", b, "module")) == [quantize.FILE_NAME]
        side = config.load(os.path.join(cdir, "sideinfos", b, "sideinfos.yaml"))
        assert side["quantize"]["bits"] == BITS
        total += get_folder_size(os.path.join(cdir, "module", b))
    assert total <= 4 * GIVEN
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    whole = fw.decompress_divide(*args)
    assert whole.shape == vol.shape and whole.dtype == vol.dtype
    # the z-sharded evaluation read the same artefacts: its PSNR is the merged volume's
    mse = np.mean((whole.astype(np.float64) - vol.astype(np.float64)) ** 2)
    assert res[STEPS]["psnr"] == pytest.approx(10.0 * np.log10(65535.0 ** 2 / mse), abs=1e-6)
    # every block is the decode of its own loaded net
    side = config.load(os.path.join(cdir, "sideinfos", blocks[0], "sideinfos.yaml"))
    net = _loaded_net(opt, os.path.join(cdir, "module", blocks[0], "module"), side)
    shape = list(side["data_shape"])
    blk = net.decode_grid(shape[:-1], -1.0, 1.0, out_kind="u16", scale=(0.0, 100.0), vrange=(side["min"], side["max"])).cpu().numpy().reshape(shape)
    assert any(np.array_equal(blk, whole[:, y:y + 20, x:x + 28]) for y in (0, 20) for x in (0, 28))
    reg = (slice(5, 16), slice(10, 30), slice(12, 41))
    assert np.array_equal(fw.decompress_divide_region(*args, reg, 1), whole[reg])


def _same_tree(a, b):
    cmp = filecmp.dircmp(a, b)
    if cmp.left_only or cmp.right_only or cmp.funny_files:
        return False
    _, mismatch, errors = filecmp.cmpfiles(a, b, cmp.common_files, shallow=False)
    return not mismatch and not errors and all(_same_tree(os.path.join(a, d), os.path.join(b, d)) for d in cmp.common_dirs)


def test_none_writes_the_bytes_of_a_run_without_the_key(volume):
    tmp, vol, path = volume
    _, plain, _ = _compress(_opt(tmp, "plain"), path)
    _, none, _ = _compress(_opt(tmp, "none", "none"), path)
    assert sorted(os.listdir(os.path.join(plain, "module")))[0].startswith("bias-0-") and quantize.FILE_NAME not in os.listdir(os.path.join(none, "module"))
    assert _same_tree(plain, none)
    assert "quantize" not in config.load(os.path.join(none, "sideinfos.yaml"))


def test_the_shipped_yaml_runs(volume):
    """opt/SingleTask/quantize.yaml (12 bits, a fine-tune) end to end, shortened"""
    tmp, vol, path = volume
    opt = _opt(tmp, "yaml", yaml="quantize.yaml")
    assert dict(opt.CompressFramework.Compress.quantize) == {"bits": 12, "finetune_steps": 2000}
    opt.CompressFramework.Compress.quantize.finetune_steps = STEPS              # (the whole shortened run is the fine-tune)
    logdir, cdir, res = _compress(opt, path)
    size = os.path.getsize(os.path.join(cdir, "module", quantize.FILE_NAME))
    assert size <= GIVEN and config.load(os.path.join(cdir, "sideinfos.yaml"))["quantize"]["bits"] == 12
