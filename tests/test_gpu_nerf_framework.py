"""NeRF against the reference's own fits (tests/golden/nerf.npz, written by tests/golden/make_golden_nerf.py) and through the
framework: NFGR SingleTask with rng: torch, the reference's artefact, DivideTask, Compress.half, a 2-D image, and main.py +
decompress.py --region with opt/SingleTask/nerf.yaml under both samplers (the reference's NeRF cannot run its skip layer under
randomcube, which it uses for volumes of at most 80^3 voxels; the per-sample net here does not depend on the sampler).

Bands, as in tests/test_gpu_nerf.py: the golden is the reference's CPU fp32 computation, itself ~e32 from float64, where e32 is the
distance of a float32 torch restatement of the same case from its float64 restatement (measured here)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config
from brief_pytorch_amd.framework import NFGR, MyLogger
from brief_pytorch_amd.networks import NeRF
from brief_pytorch_amd.tool import read_img, save_img
from tests.test_gpu_nerf import encoding, golden_band, torch_nerf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = {"adamax": ("Adamax", {"name": "MultiStepLR", "milestones": [10, 20], "gamma": 0.5}),
         "adam": ("Adam", {"name": "StepLR", "step_size": 7, "gamma": 0.7}),
         "sgd": ("SGD", {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 1e-2, "step_size_up": 5, "cycle_momentum": False})}
TRACE_F, TRACE_L, TRACE_FREQ = 24, 4, 10


def _opt(tmp_path, steps, given, layers):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "nerf.yaml"))
    cf = opt.CompressFramework
    cf.Compress.max_steps = steps
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = given
    cf.Compress.loss_log_freq = 50
    cf.Module.phi.layers = layers
    opt.Log.outputs_dir = str(tmp_path / "outputs")
    opt.Log.time = False
    return opt


def _replay(g, tag, dtype, data, dims):
    """the golden's fit in torch at `dtype` on the golden's recorded index stream (same init, torch optimizer and scheduler)"""
    optname, sched = TRACE[tag]
    lin = [torch.linspace(-1, 1, d, dtype=torch.float32) for d in dims]
    coords = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3)
    enc_all = encoding(coords, TRACE_FREQ, dtype)
    ws = []
    for l in range(TRACE_L):
        ws += [torch.from_numpy(g["tr_%s_init_w%d" % (tag, l)]).to(dtype).requires_grad_(True),
               torch.from_numpy(g["tr_%s_init_b%d" % (tag, l)]).to(dtype).requires_grad_(True)]
    o = {"Adamax": torch.optim.Adamax, "Adam": torch.optim.Adam, "SGD": torch.optim.SGD}[optname](ws, lr=1e-3)
    s = dict(sched)
    sc = getattr(torch.optim.lr_scheduler, s.pop("name"))(o, **s)
    y = data.to(dtype)
    losses, sl = [], (TRACE_L - 1) // 2
    for idx in g["tr_%s_idx" % tag]:
        i = torch.from_numpy(idx)
        enc = enc_all[i]
        o.zero_grad()
        h = enc
        for l in range(TRACE_L):
            if l == sl:
                h = torch.cat([enc, h], 1)
            h = h @ ws[2 * l].T + ws[2 * l + 1]
            if l < TRACE_L - 1:
                h = torch.relu(h)
        lt = ((h - y[i]) ** 2).mean()
        lt.backward()
        o.step()
        sc.step()
        losses.append(lt.item())
    return np.array(losses), [w.detach().double().numpy() for w in ws]


@pytest.mark.parametrize("tag", list(TRACE))
def test_fit_trace_matches_reference_golden(golden, tmp_path, tag):
    """NFGR with Compress.sampler.rng: torch, from the reference's seed alone: the NeRF init equals the reference's bit for bit, the
    sampler then draws the reference's voxel indices (checked for every step), and the 30-step loss trace and final weights are within
    band of the reference's run"""
    g = golden("nerf")
    vol = g["tr_vol"]
    dims = vol.shape[:-1]
    optname, sched = TRACE[tag]
    opt = _opt(tmp_path, 30, 4.0 * NeRF.calc_param_count(3, 1, TRACE_F, frequencies=TRACE_FREQ, layers=TRACE_L, skip=True), TRACE_L)
    cf = opt.CompressFramework
    cf.Compress.sampler.name = "randompoint"
    cf.Compress.sampler.sample_size = 1000
    cf.Compress.sampler.rng = "torch"
    cf.Compress.optimizer_name_phi = optname
    cf.Compress.lr_phi = 1e-3
    cf.Compress.lr_scheduler_phi = config.to_opt(copy.deepcopy(sched)) if hasattr(config, "to_opt") else copy.deepcopy(sched)
    torch.manual_seed(42)                                   # reproduc(seed 42), as in the golden run
    ctx = NFGR(cf, Log=None).prepare_fit(str(tmp_path / "vol.tif"), data=vol, logdir=str(tmp_path))
    phi, fit = ctx["phi"], ctx["fit"]
    assert isinstance(phi, NeRF) and phi.features == TRACE_F and phi.skip_layer == 1
    for l in range(TRACE_L):
        assert np.array_equal(phi.net[l][0].weight.data.cpu().numpy(), g["tr_%s_init_w%d" % (tag, l)])
        assert np.array_equal(phi.net[l][0].bias.data.cpu().numpy(), g["tr_%s_init_b%d" % (tag, l)])
    gen = torch.Generator()
    gen.set_state(fit.index_stream.gen.get_state())
    for t, want in enumerate(g["tr_%s_idx" % tag]):
        assert np.array_equal(torch.randint(0, fit.pop, (fit.n,), generator=gen).numpy(), want), "indices of step %d" % (t + 1)
    losses = fit.run(30, log=True).cpu().numpy().astype(np.float64)
    data = fit.targets.detach().cpu().reshape(-1)[:, None]
    l64, w64 = _replay(g, tag, torch.float64, data, dims)
    l32, w32 = _replay(g, tag, torch.float32, data, dims)
    golden_band(losses, g["tr_%s_losses" % tag], float(np.max(np.abs(l32 - l64))), float(np.max(g["tr_%s_losses" % tag])), "losses")
    for l in range(TRACE_L):
        for j, what in ((0, "w"), (1, "b")):
            got = (phi.net[l][0].weight if j == 0 else phi.net[l][0].bias).data.cpu().numpy()
            gold = g["tr_%s_final_%s%d" % (tag, what, l)]
            e32 = float(np.max(np.abs(w32[2 * l + j] - w64[2 * l + j])))
            golden_band(got, gold, e32, float(np.max(np.abs(gold))), "final %s%d" % (what, l))


def test_reference_artefact_decodes_like_the_reference(golden, tmp_path):
    """the weight files the reference wrote decode here (NFGR.decompress path: load_model + decode_grid) to the reference's own
    forward on the grid"""
    from brief_pytorch_amd.modelsave import load_model
    g = golden("nerf")
    src = tmp_path / "module"
    src.mkdir()
    for n in g["art_names"]:
        (src / str(n)).write_bytes(g["art_file_" + str(n)].tobytes())
    m = NeRF(coords_channel=3, data_channel=1, frequencies=TRACE_FREQ, features=TRACE_F, layers=TRACE_L, skip=True)
    load_model(m, str(src))
    m.to("cuda")
    dims = g["tr_vol"].shape[:-1]
    dec = m.decode_grid(dims).cpu().numpy()
    lin = [torch.linspace(-1, 1, d) for d in dims]
    x = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3)
    y64, _ = torch_nerf(m, x, torch.float64)
    y32, _ = torch_nerf(m, x, torch.float32)
    e32 = float(torch.max(torch.abs(y32.detach().double() - y64.detach())))
    golden_band(dec, g["art_decode"], e32, float(np.max(np.abs(g["art_decode"]))), "decode of the reference artefact")


def test_dividetask_nerf_blocks_fit_decode_and_region(tmp_path):
    """a DivideTask of NeRF blocks (fitted one after another: brief_multi_fit co-trains SIREN only) runs, decodes from its artefact
    tree bit for bit, and its region decode equals the slice of the merged volume"""
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume((16, 32, 32), seed=3)
    path = str(tmp_path / "blk.tif")
    save_img(path, vol)
    opt = _opt(tmp_path, 2000, 4 * 4.0 * NeRF.calc_param_count(3, 1, 48, frequencies=10, layers=5, skip=True), 5)
    cf = opt.CompressFramework
    cf.Compress.divide.divide_type = "total_1_2_2"
    cf.Compress.divide.param_alloc = "by_size"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    res = fw.compress_divide(path, opt)
    assert list(res) == [2000] and np.isfinite(res[2000]["psnr"])
    cdir = os.path.join(Log.logdir, "steps2000", "compressed")
    for n in os.listdir(os.path.join(cdir, "sideinfos")):
        assert config.load(os.path.join(cdir, "sideinfos", n, "sideinfos.yaml"))["phi_name"] == "NeRF"
    merged = read_img(os.path.join(Log.logdir, "steps2000", "decompressed", "blk_decompressed.tif"))
    again = fw.decompress_divide(os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    assert np.array_equal(again, merged)
    d0 = vol.astype(np.float64) - vol.astype(np.float64).mean()
    assert res[2000]["psnr"] > -10 * np.log10((d0 * d0).mean() / 65535.0 ** 2) + 3      # clearly better than the constant volume
    reg = fw.decompress_divide_region(os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"),
                                      "3:13,5:30,10:20", opt=opt)
    assert np.array_equal(reg, merged[3:13, 5:30, 10:20])


def test_half_with_nerf_runs_fp32_and_records_it(tmp_path, caplog):
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume((16, 24, 32), seed=10)
    path = str(tmp_path / "h.tif")
    save_img(path, vol)
    given = 4.0 * NeRF.calc_param_count(3, 1, 20, frequencies=10, layers=4, skip=True)
    opt = _opt(tmp_path, 100, given, 4)
    opt.CompressFramework.Compress.half = True
    opt.CompressFramework.Compress.checkpoints = "100"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(opt.CompressFramework, Log=Log)
    with caplog.at_level("WARNING"):
        res = fw.compress(path)
    assert any("NeRF has fp32 kernels only" in r.getMessage() for r in caplog.records)
    side = config.load(os.path.join(Log.logdir, "steps100", "compressed", "sideinfos.yaml"))
    assert side["phi_precision"] == "fp32" and side["phi_name"] == "NeRF"
    assert side["phi_features"] == NeRF.calc_features(given / 2.0, 3, 1, frequencies=10, layers=4, skip=True) > 20      # 2 bytes/param
    assert fw.module["phi"].precision == "fp32" and np.isfinite(res[100]["psnr"])


def test_2d_rgb_image(tmp_path):
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, 48), np.linspace(0, 1, 64), indexing="ij")
    img = np.stack([120 + 100 * np.sin(6 * xx + 2 * yy), 128 + 90 * np.cos(5 * yy), 100 + 80 * np.sin(4 * (xx + yy))], -1)
    img = np.clip(img + rng.normal(0, 2, img.shape), 0, 255).astype(np.uint8)
    path = str(tmp_path / "rgb.png")
    save_img(path, img)
    opt = _opt(tmp_path, 1500, 4.0 * NeRF.calc_param_count(2, 3, 40, frequencies=10, layers=4, skip=True), 4)
    cf = opt.CompressFramework
    cf.Module.phi.coords_channel, cf.Module.phi.data_channel = 2, 3
    cf.Compress.preprocess.clip = [0, 255]
    cf.Decompress.postprocess.clip = [0, 255]
    cf.Compress.loss.weight = ["value_255_255_1"]
    cf.Compress.loss.weight_thres = 255
    cf.Decompress.mip = False
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    res = fw.compress(path)
    assert res[1500]["psnr"] > 20
    sdir = os.path.join(Log.logdir, "steps1500")
    side = config.load(os.path.join(sdir, "compressed", "sideinfos.yaml"))
    assert side["phi_name"] == "NeRF" and side["phi_features"] == 40
    assert os.path.exists(os.path.join(sdir, "compressed", "module", "weight-0-40-42"))
    assert os.path.exists(os.path.join(sdir, "compressed", "module", "weight-1-40-82"))       # the skip layer: [F, d + F]
    dec = read_img(os.path.join(sdir, "decompressed", "rgb_decompressed.png"))
    again = NFGR.decompress(config.to_opt({"CompressFramework": cf}), os.path.join(sdir, "compressed", "module"), dict(side))
    assert np.array_equal(again, dec)


@pytest.mark.parametrize("shape,steps", [((24, 28, 32), 2000), ((64, 96, 96), 300)])
def test_main_nerf_yaml_and_region_cli(tmp_path, shape, steps):
    """python main.py -p opt/SingleTask/nerf.yaml: a volume of at most 80^3 voxels (the randomcube sampler, which the reference's NeRF
    cannot run) and a larger one (randompoint); decompress.py --region of the artefact equals the slice of the decoded volume"""
    import yaml
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume(shape, seed=3)
    data = str(tmp_path / "vol.tif")
    save_img(data, vol)
    with open(os.path.join(ROOT, "opt", "SingleTask", "nerf.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["Dataset"]["data_path"] = data
    cfg["Log"]["outputs_dir"] = str(tmp_path / "out")
    cfg["CompressFramework"]["Compress"]["max_steps"] = steps
    cfg["CompressFramework"]["Compress"]["checkpoints"] = str(steps)
    cfg["CompressFramework"]["Compress"]["param"]["filesize_ratio"] = 0
    cfg["CompressFramework"]["Compress"]["param"]["given_size"] = 4.0 * NeRF.calc_param_count(3, 1, 64, frequencies=10, layers=5, skip=True)
    p = str(tmp_path / "nerf.yaml")
    with open(p, "w") as f:
        yaml.safe_dump(cfg, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "-p", p], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    comp = [dp for dp, _, fs in os.walk(str(tmp_path / "out")) if "sideinfos.yaml" in fs and os.path.basename(dp) == "compressed"]
    assert len(comp) == 1
    with open(os.path.join(comp[0], "sideinfos.yaml")) as f:
        assert yaml.safe_load(f)["phi_name"] == "NeRF"
    decf = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "out")) for f in fs if f == "vol_decompressed.tif"]
    dec = read_img(decf[0])
    d = dec.astype(np.float64) - vol.astype(np.float64)
    psnr = -10 * np.log10((d * d).mean() / 65535.0 ** 2)
    d0 = vol.astype(np.float64) - vol.astype(np.float64).mean()
    psnr0 = -10 * np.log10((d0 * d0).mean() / 65535.0 ** 2)
    assert np.isfinite(psnr) and psnr > psnr0 + (3 if steps >= 2000 else 0), (psnr, psnr0)
    out = str(tmp_path / "roi.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", p, "-c", comp[0], "--region", "2:20,3:27,4:30", "-o", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert np.array_equal(np.load(out), dec[2:20, 3:27, 4:30])
