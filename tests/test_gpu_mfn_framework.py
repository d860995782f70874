"""MFNFourier / MFNGabor against the reference's own fits (tests/golden/mfn.npz, written by tests/golden/make_golden_mfn.py) and
through the framework: NFGR SingleTask with rng: torch, the reference's artefact (one torch.save file), DivideTask, Compress.half, a 2-D
image, and main.py + decompress.py --region with opt/SingleTask/mfn_gabor.yaml.

Bands, as in tests/test_gpu_mfn.py: the golden is the reference's CPU fp32 computation, itself ~e32 from float64, where e32 is the
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
from brief_pytorch_amd.modelsave import load_model
from brief_pytorch_amd.networks import MFNFourier, MFNGabor
from brief_pytorch_amd.tool import read_img, save_img
from tests.test_gpu_mfn import golden_band, torch_mfn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"fourier": MFNFourier, "gabor": MFNGabor}
TRACE = {"adamax": ("Adamax", {"name": "MultiStepLR", "milestones": [10, 20], "gamma": 0.5}),
         "adam": ("Adam", {"name": "StepLR", "step_size": 7, "gamma": 0.7}),
         "sgd": ("SGD", {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 1e-2, "step_size_up": 5, "cycle_momentum": False})}
TRACE_F, TRACE_L = 24, 4


def _opt(tmp_path, kind, steps, given, layers):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "mfn_%s.yaml" % kind))
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


def _replay(g, kind, tag, dtype, data, dims):
    """the golden's fit in torch at `dtype` on the golden's recorded index stream (same init, torch optimizer and scheduler)"""
    optname, sched = TRACE[tag]
    lin = [torch.linspace(-1, 1, d, dtype=torch.float32) for d in dims]
    coords = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3)
    m = KINDS[kind](coords_channel=3, features=TRACE_F, data_channel=1, layers=TRACE_L)
    pre = "%s_tr_%s_init_" % (kind, tag)
    m.load_state_dict({str(k): torch.from_numpy(g[pre + "s%d" % j]) for j, k in enumerate(g[pre + "keys"])})
    _, t = torch_mfn(m, coords[:1], dtype)
    leaves = list(t.values())
    o = {"Adamax": torch.optim.Adamax, "Adam": torch.optim.Adam, "SGD": torch.optim.SGD}[optname](leaves, lr=1e-3)
    s = dict(sched)
    sc = getattr(torch.optim.lr_scheduler, s.pop("name"))(o, **s)
    y = data.to(dtype)
    losses = []
    for idx in g["%s_tr_%s_idx" % (kind, tag)]:
        i = torch.from_numpy(idx)
        x = coords[i].to(dtype)
        o.zero_grad()

        def filt(j):
            h = torch.sin(x @ t["filters.%d.linear.weight" % j].T + t["filters.%d.linear.bias" % j])
            if m.GABOR:
                mu, gam = t["filters.%d.mu" % j], t["filters.%d.gamma" % j]
                D = (x ** 2).sum(-1)[..., None] + (mu ** 2).sum(-1)[None, :] - 2 * x @ mu.T
                h = h * torch.exp(-0.5 * D * gam[None, :])
            return h
        z = filt(0)
        for j in range(1, TRACE_L - 1):
            z = filt(j) * (z @ t["linear.%d.weight" % (j - 1)].T + t["linear.%d.bias" % (j - 1)])
        h = z @ t["output_linear.weight"].T + t["output_linear.bias"]
        lt = ((h - y[i]) ** 2).mean()
        lt.backward()
        o.step()
        sc.step()
        losses.append(lt.item())
    return np.array(losses), {k: v.detach().double().numpy() for k, v in t.items()}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("tag", list(TRACE))
def test_fit_trace_matches_reference_golden(golden, tmp_path, kind, tag):
    """NFGR with Compress.sampler.rng: torch, from the reference's seed alone: the init equals the reference's bit for bit, the sampler
    draws the reference's voxel indices (checked for every step), and the 30-step loss trace and final weights are within band of the
    reference's run"""
    g = golden("mfn")
    cls = KINDS[kind]
    vol = g["tr_vol"]
    dims = vol.shape[:-1]
    optname, sched = TRACE[tag]
    opt = _opt(tmp_path, kind, 30, 4.0 * cls.calc_param_count(3, 1, TRACE_F, TRACE_L), TRACE_L)
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
    assert isinstance(phi, cls) and phi.features == TRACE_F
    pre = "%s_tr_%s_" % (kind, tag)
    sd = phi.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[pre + "init_keys"]]
    for j, k in enumerate(sd):
        if kind == "gabor" and k.endswith("linear.weight") and k.startswith("filters."):
            # weight *= scale * torch.sqrt(gamma): torch's CPU sqrt is not correctly rounded on every host, so the reference's own
            # init differs by an ulp between machines; tests/test_mfn_host.py checks these bits on the machine the golden came from
            np.testing.assert_allclose(sd[k].numpy(), g[pre + "init_s%d" % j], rtol=1e-6, atol=0, err_msg=k)
        else:
            assert np.array_equal(sd[k].numpy(), g[pre + "init_s%d" % j]), k
    gen = torch.Generator()
    gen.set_state(fit.index_stream.gen.get_state())
    for t, want in enumerate(g[pre + "idx"]):
        assert np.array_equal(torch.randint(0, fit.pop, (fit.n,), generator=gen).numpy(), want), "indices of step %d" % (t + 1)
    losses = fit.run(30, log=True).cpu().numpy().astype(np.float64)
    data = fit.targets.detach().cpu().reshape(-1)[:, None]
    l64, w64 = _replay(g, kind, tag, torch.float64, data, dims)
    l32, w32 = _replay(g, kind, tag, torch.float32, data, dims)
    golden_band(losses, g[pre + "losses"], float(np.max(np.abs(l32 - l64))), float(np.max(g[pre + "losses"])), "losses")
    sd = phi.state_dict()
    for j, k in enumerate(sd):
        gold = g[pre + "final_s%d" % j]
        golden_band(sd[k].numpy(), gold, float(np.max(np.abs(w32[k] - w64[k]))), float(np.max(np.abs(gold))), "final %s" % k)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reference_artefact_decodes_like_the_reference(golden, tmp_path, kind):
    """the single torch.save file the reference's save_model wrote loads here (weights_only) and decodes (NFGR.decompress path:
    load_model + decode_grid) to the reference's own forward on the grid"""
    g = golden("mfn")
    src = tmp_path / "module"
    src.write_bytes(g["%s_art_bytes" % kind].tobytes())
    m = KINDS[kind](coords_channel=3, features=TRACE_F, data_channel=1, layers=TRACE_L)
    load_model(m, str(src))
    m.to("cuda")
    dims = g["tr_vol"].shape[:-1]
    dec = m.decode_grid(dims).cpu().numpy()
    lin = [torch.linspace(-1, 1, d) for d in dims]
    x = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1).reshape(-1, 3)
    y64, _ = torch_mfn(m, x, torch.float64)
    y32, _ = torch_mfn(m, x, torch.float32)
    e32 = float(torch.max(torch.abs(y32.detach().double() - y64.detach())))
    golden_band(dec, g["%s_art_decode" % kind], e32, float(np.max(np.abs(g["%s_art_decode" % kind]))), "decode of the reference artefact")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_dividetask_mfn_blocks_fit_decode_and_region(tmp_path, kind):
    """a DivideTask of MFN blocks (fitted one after another: brief_multi_fit co-trains SIREN only) runs, every block's artefact is one
    file, the tree decodes bit for bit, and its region decode equals the slice of the merged volume"""
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume((16, 32, 32), seed=3)
    path = str(tmp_path / "blk.tif")
    save_img(path, vol)
    opt = _opt(tmp_path, kind, 300, 4 * 4.0 * KINDS[kind].calc_param_count(3, 1, 32, 5), 5)
    cf = opt.CompressFramework
    cf.Compress.divide.divide_type = "total_1_2_2"
    cf.Compress.divide.param_alloc = "by_size"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    res = fw.compress_divide(path, opt)
    assert list(res) == [300] and np.isfinite(res[300]["psnr"])
    cdir = os.path.join(Log.logdir, "steps300", "compressed")
    names = os.listdir(os.path.join(cdir, "sideinfos"))
    assert len(names) == 4
    for n in names:
        assert config.load(os.path.join(cdir, "sideinfos", n, "sideinfos.yaml"))["phi_name"] == KINDS[kind].kind
        assert os.path.isfile(os.path.join(cdir, "module", n, "module"))
    merged = read_img(os.path.join(Log.logdir, "steps300", "decompressed", "blk_decompressed.tif"))
    again = fw.decompress_divide(os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    assert np.array_equal(again, merged)
    reg = fw.decompress_divide_region(os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"),
                                      "3:13,5:30,10:20", opt=opt)
    assert np.array_equal(reg, merged[3:13, 5:30, 10:20])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_half_with_mfn_runs_fp32_and_records_it(tmp_path, caplog, kind):
    from brief_pytorch_amd.synthetic import make_volume
    cls = KINDS[kind]
    vol = make_volume((16, 24, 32), seed=10)
    path = str(tmp_path / "h.tif")
    save_img(path, vol)
    given = 4.0 * cls.calc_param_count(3, 1, 20, 4)
    opt = _opt(tmp_path, kind, 100, given, 4)
    opt.CompressFramework.Compress.half = True
    opt.CompressFramework.Compress.checkpoints = "100"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(opt.CompressFramework, Log=Log)
    with caplog.at_level("WARNING"):
        res = fw.compress(path)
    assert any("%s has fp32 kernels only" % cls.kind in r.getMessage() for r in caplog.records)
    side = config.load(os.path.join(Log.logdir, "steps100", "compressed", "sideinfos.yaml"))
    assert side["phi_precision"] == "fp32" and side["phi_name"] == cls.kind
    assert side["phi_features"] == cls.calc_features(given / 2.0, 3, 1, 4) > 20      # 2 bytes/param
    assert fw.module["phi"].precision == "fp32" and np.isfinite(res[100]["psnr"])
    assert os.path.isfile(os.path.join(Log.logdir, "steps100", "compressed", "module"))


def test_2d_rgb_image(tmp_path):
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, 48), np.linspace(0, 1, 64), indexing="ij")
    img = np.stack([120 + 100 * np.sin(6 * xx + 2 * yy), 128 + 90 * np.cos(5 * yy), 100 + 80 * np.sin(4 * (xx + yy))], -1)
    img = np.clip(img + rng.normal(0, 2, img.shape), 0, 255).astype(np.uint8)
    path = str(tmp_path / "rgb.png")
    save_img(path, img)
    opt = _opt(tmp_path, "fourier", 1000, 4.0 * MFNFourier.calc_param_count(2, 3, 40, 4), 4)
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
    assert np.isfinite(res[1000]["psnr"])
    sdir = os.path.join(Log.logdir, "steps1000")
    side = config.load(os.path.join(sdir, "compressed", "sideinfos.yaml"))
    assert side["phi_name"] == "MFNFourier" and side["phi_features"] == 40
    sd = torch.load(os.path.join(sdir, "compressed", "module"), weights_only=True)
    assert tuple(sd["filters.0.linear.weight"].shape) == (40, 2) and tuple(sd["output_linear.weight"].shape) == (3, 40)
    dec = read_img(os.path.join(sdir, "decompressed", "rgb_decompressed.png"))
    again = NFGR.decompress(config.to_opt({"CompressFramework": cf}), os.path.join(sdir, "compressed", "module"), dict(side))
    assert np.array_equal(again, dec)


def test_main_mfn_gabor_yaml_and_region_cli(tmp_path):
    """python main.py -p opt/SingleTask/mfn_gabor.yaml, then decompress.py --region of the artefact equals the slice of the decoded
    volume"""
    import yaml
    from brief_pytorch_amd.synthetic import make_volume
    shape, steps = (24, 28, 32), 500
    vol = make_volume(shape, seed=3)
    data = str(tmp_path / "vol.tif")
    save_img(data, vol)
    with open(os.path.join(ROOT, "opt", "SingleTask", "mfn_gabor.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["Dataset"]["data_path"] = data
    cfg["Log"]["outputs_dir"] = str(tmp_path / "out")
    cfg["CompressFramework"]["Compress"]["max_steps"] = steps
    cfg["CompressFramework"]["Compress"]["checkpoints"] = str(steps)
    p = str(tmp_path / "mfn_gabor.yaml")
    with open(p, "w") as f:
        yaml.safe_dump(cfg, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "-p", p], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    comp = [dp for dp, _, fs in os.walk(str(tmp_path / "out")) if "sideinfos.yaml" in fs and os.path.basename(dp) == "compressed"]
    assert len(comp) == 1
    with open(os.path.join(comp[0], "sideinfos.yaml")) as f:
        assert yaml.safe_load(f)["phi_name"] == "MFNGabor"
    assert os.path.isfile(os.path.join(comp[0], "module"))
    decf = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "out")) for f in fs if f == "vol_decompressed.tif"]
    dec = read_img(decf[0])
    out = str(tmp_path / "roi.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", p, "-c", comp[0], "--region", "2:20,3:27,4:30", "-o", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert np.array_equal(np.load(out), dec[2:20, 3:27, 4:30])
