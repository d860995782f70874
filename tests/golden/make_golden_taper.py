#!/usr/bin/env python3
"""Generate tests/golden/taper.npz by RUNNING the reference's SIREN_Pyramid / SIRENFT / SIRENPS (utils/Networks.py:316-552) and its
NFGR.estimate_module_size (main.py:214-246).

Runs only where the reference tree is present (CPU torch), like make_golden.py, whose stubs and helpers it imports unchanged: the
reference modules are imported in place and driven on small seeded inputs; inputs and outputs are stored as a .npz fixture.  Tests
only read the .npz.

    python tests/golden/make_golden_taper.py

Contents (<k> one of "pyramid" / "ft" / "ps"; *_cfg entries are JSON strings of constructor keywords):
  <k>_init<i>_*   nets after different prior seeds: every state_dict entry (s<j>, in key order), the keys, the constructor keywords
                  (float `features` included), then torch.rand(5) drawn right after construction
  bud_rows        JSON list: NFGR.estimate_module_size of the reference over specs and budgets: {"phi", "bytes", "half"} and either
                  {"name", "features", "count", "theory"} (the name the reference left in the options) or {"raises": exception type}
  <k>_fwd<i>_*    reference forward (CPU fp32) on 256 random coordinates; the net is the reference's init right after
                  torch.manual_seed(<k>_fwd<i>_seed) (seeds, not weights: the init replay is exact)
  <k>_tr_<o>_*    a 30-step fit per optimizer / scheduler through the reference's NFGR (reproduc(42), prepare_module,
                  RandompointSampler, loss_func, optimizer + scheduler): init, final weights, losses, the phi spec and byte budget;
                  <k>_tr_idx is the recorded index stream (uint16; the same for the three optimizers: it follows the init's draws);
                  for adamax also the files the reference's save_model wrote and its decode of the final net; tr_normalize is the
                  Normalize.name of these fits (see TRACE_NORMALIZE)
"""
import copy
import importlib.util
import json
import os
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)          # stubs, sys.path and the reference imports of make_golden.py (its __main__ block does not run)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from utils.Networks import SIREN_Pyramid as RefPyramid, SIRENFT as RefFT, SIRENPS as RefPS  # noqa: E402
from utils import ModelSave as refsave  # noqa: E402
from utils import dataset as refdataset  # noqa: E402

KINDS = {"pyramid": ("SIREN_Pyramid", RefPyramid), "ft": ("SIRENFT", RefFT), "ps": ("SIRENPS", RefPS)}
BASE = {"coords_channel": 3, "data_channel": 1, "layers": 5, "w0": 20, "output_act": False, "res": False}


def kw(**over):
    return {**BASE, **over}


INIT_CASES = {
    "pyramid": [(42, kw(features=38, features_dis=10)), (7, kw(features=20, features_dis=-3, layers=4, coords_channel=2, data_channel=3)),
                (12345, kw(features=9, features_dis=0, layers=3, w0=30)), (99, kw(features=67, features_dis=10, output_act=True))],
    "ft": [(42, kw(features=43.936769251345325, ratio=2)), (7, kw(features=12.7, ratio=0.5, layers=4, coords_channel=2, data_channel=3)),
           (12345, kw(features=9, ratio=1, layers=3, w0=30)), (99, kw(features=7.4, ratio=1.5, output_act=True))],
    "ps": [(42, kw(features=24.960730560465638, ratio=1.5)), (7, kw(features=20.3, ratio=0.7, layers=4, coords_channel=2, data_channel=3)),
           (12345, kw(features=10, ratio=1.6, layers=3, w0=30)), (99, kw(features=5.5, ratio=1.3, layers=7, output_act=True))],
}
FWD_CASES = {   # every structural case: widths below 32, across a 32 boundary, output_act, cout 1..4, growing, ratio < 1 and > 1, near 1024
    "pyramid": [kw(features=38, features_dis=10), kw(features=67, features_dis=10), kw(features=271, features_dis=10),
                kw(features=39, features_dis=-8, coords_channel=2, data_channel=3), kw(features=1024, features_dis=300, layers=4),
                kw(features=130, features_dis=20, layers=7, data_channel=2, output_act=True)],
    "ft": [kw(features=43.936769251345325, ratio=2), kw(features=56, ratio=0.5, data_channel=4), kw(features=221.35926052107416, ratio=2),
           kw(features=510.8494900944081, ratio=2, layers=3), kw(features=7.4, ratio=1.5, coords_channel=2, output_act=True)],
    "ps": [kw(features=24.960730560465638, ratio=1.5), kw(features=80.66882526678584, ratio=0.7), kw(features=125.45368822738716, ratio=1.5),
           kw(features=289.41945872951385, ratio=1.5), kw(features=64, ratio=2, layers=6, coords_channel=2, data_channel=2),
           kw(features=10, ratio=1.6, layers=3, data_channel=3, output_act=True)],
}
TRACE_CASES = {  # optimizer, scheduler (the YAML keys utils/misc.py:184-197 passes through)
    "adamax": ("Adamax", {"name": "MultiStepLR", "milestones": [10, 20], "gamma": 0.5}),
    "adam": ("Adam", {"name": "StepLR", "step_size": 7, "gamma": 0.7}),
    "sgd": ("SGD", {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 1e-2, "step_size_up": 5, "cycle_momentum": False}),
}
TRACE_PHI = {"pyramid": kw(layers=4, features_dis=4), "ft": kw(layers=4, ratio=2), "ps": kw(layers=4, ratio=1.5)}
TRACE_BYTES = 4.0 * 1500
# targets in [0, 1]: with the shipped minmaxany_0_100 the SGD + CyclicLR (max_lr 1e-2) fits of these nets are chaotic in the reference
# itself (a torch fp32 and a torch float64 replay of its run on the recorded indices part by 4e-3 in the loss and by more than the
# weights' size within 30 steps, measured on the CPU), so no band on a 30-step trace would say anything about a third implementation
TRACE_NORMALIZE = "minmaxany_0_1"
TRACE_DIMS, TRACE_N, TRACE_STEPS = (12, 20, 28), 1000, 30


def sd_arrays(m, prefix):
    out = {}
    sd = m.state_dict()
    for j, (k, v) in enumerate(sd.items()):
        out[prefix + "s%d" % j] = v.detach().numpy().copy()
    out[prefix + "keys"] = np.array(list(sd.keys()))
    return out


def g_init(arrs):
    for kind, (_, Ref) in KINDS.items():
        for i, (seed, cfg) in enumerate(INIT_CASES[kind]):
            torch.manual_seed(seed)
            m = Ref(**cfg)
            arrs.update(sd_arrays(m, "%s_init%d_" % (kind, i)))
            arrs["%s_init%d_rand" % (kind, i)] = torch.rand(5).numpy()
            arrs["%s_init%d_cfg" % (kind, i)] = np.array(json.dumps(cfg))
            arrs["%s_init%d_seed" % (kind, i)] = np.array(seed, np.int64)


def g_budget(arrs):
    specs = []
    pyr = dict(name="SIREN_Pyramid", features_dis=10)
    for b in (6516, 33000, 794628, 4.2e6, 1.3e7):
        specs.append((kw(**pyr), b))
    for b in (400, 1200):
        specs.append((kw(ratio=1.5, **pyr), b))
    specs.append((kw(**pyr), 400))                                   # no ratio: the reference dies with TypeError
    specs.append((kw(ratio=2, **pyr), 60))                           # falls through SIRENFT to SIREN
    specs.append((kw(name="SIREN_Pyramid", features_dis=-8), 33000))
    for b in (60, 68, 33000, 794628, 4.2e6, 1.3e7):
        specs.append((kw(name="SIRENFT", ratio=2), b))
    specs.append((kw(name="SIRENFT", ratio=0.5), 33000))
    for b in (33000, 794628, 4.2e6, 1.3e7, 120, 20):
        specs.append((kw(name="SIRENPS", ratio=1.5), b))
    for b in (33000, 794628):
        specs.append((kw(name="SIRENPS", ratio=0.7), b))
    specs.append((kw(name="SIRENPS", ratio=1), 33000))               # ZeroDivisionError in the reference
    specs.append((kw(name="SIRENPS", ratio=1.5, data_channel=3), 33000))
    for name, extra in (("SIREN_Pyramid", {"features_dis": 10, "ratio": 1.5}), ("SIRENFT", {"ratio": 2}), ("SIRENPS", {"ratio": 1.5})):
        for L in (2, 3, 4, 5, 6, 7):
            for cin in (2, 3):
                for b in (33000, 794628):
                    specs.append((kw(name=name, layers=L, coords_channel=cin, **extra), b))
    specs.append((kw(name="SIRENPS", ratio=1.5), 33000, True))       # Compress.half: 2 bytes per parameter
    rows = []
    for sp in specs:
        phi, b = sp[0], sp[1]
        half = len(sp) > 2
        opt = mg.load_opt().CompressFramework
        opt.Compress.half = half
        opt.Module.phi = mg.to_attr(copy.deepcopy(phi))
        row = {"phi": phi, "bytes": b, "half": half}
        try:
            feats, count, theory = mg.refmain.NFGR.estimate_module_size(float(b), opt)
            row.update(name=opt.Module.phi.name, features=feats, count=count, theory=theory,
                       features_plus=opt.Module.phi.get("features_plus"))
        except Exception as e:      # noqa: BLE001 (the type is the datum)
            row["raises"] = type(e).__name__
        rows.append(row)
    arrs["bud_rows"] = np.array(json.dumps(rows))


def g_forward(arrs):
    for kind, (_, Ref) in KINDS.items():
        for i, cfg in enumerate(FWD_CASES[kind]):
            seed = 2000 + i
            torch.manual_seed(seed)
            m = Ref(**cfg)
            g = torch.Generator().manual_seed(300 + i)
            x = torch.rand(256, cfg["coords_channel"], generator=g) * 2 - 1
            with torch.no_grad():
                y = m(x)
            arrs["%s_fwd%d_cfg" % (kind, i)] = np.array(json.dumps(cfg))
            arrs["%s_fwd%d_widths" % (kind, i)] = np.array([m.net[l][0].out_features for l in range(len(m.net) - 1)], np.int64)
            arrs["%s_fwd%d_seed" % (kind, i)] = np.array(seed, np.int64)
            arrs["%s_fwd%d_x" % (kind, i)] = x.numpy()
            arrs["%s_fwd%d_y" % (kind, i)] = y.numpy()


def g_trace(arrs):
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume(TRACE_DIMS, seed=43)
    arrs["tr_vol"] = vol
    arrs["tr_bytes"] = np.array(TRACE_BYTES)
    arrs["tr_normalize"] = np.array(TRACE_NORMALIZE)
    for kind, (name, Ref) in KINDS.items():
        arrs["%s_tr_phi" % kind] = np.array(json.dumps({"name": name, **TRACE_PHI[kind]}))
        for tag, (optname, sched) in TRACE_CASES.items():
            opt = mg.load_opt()
            cf = opt.CompressFramework
            cf.Compress.gpu = False
            cf.Decompress.gpu = False
            cf.Module.phi = mg.to_attr({"name": name, **copy.deepcopy(TRACE_PHI[kind])})
            cf.Normalize.name = TRACE_NORMALIZE
            cf.Compress.sampler.name = "randompoint"
            cf.Compress.sampler.sample_size = TRACE_N
            cf.Compress.optimizer_name_phi = optname
            cf.Compress.lr_phi = 1e-3
            cf.Compress.lr_scheduler_phi = mg.to_attr(copy.deepcopy(sched))
            mg.refmain.reproduc(opt.Reproduc)
            nf = mg.refmain.NFGR(cf)
            nf.device = "cpu"
            weight = mg.refmisc.parse_weight(vol, cf.Compress.loss.weight)
            data, sideinfos = mg.refio.normalize_data(vol, **cf.Normalize)
            feats, _ = nf.prepare_module(TRACE_BYTES)
            assert cf.Module.phi.name == name
            phi = nf.module["phi"]
            init = sd_arrays(phi, "")
            sampler = mg.refmain.RandompointSampler(data, weight, cf.Compress.coords_mode, TRACE_N, TRACE_STEPS, "cpu")
            optim = mg.refmisc.configure_optimizer(phi.parameters(), optname, cf.Compress.lr_phi)
            sch = mg.refmisc.configure_lr_scheduler(optim, cf.Compress.lr_scheduler_phi)
            thr, _ = mg.refio.normalize_data(np.array(cf.Compress.loss.weight_thres), **cf.Normalize, max=sideinfos["max"], min=sideinfos["min"])
            idxs, losses = [], []
            orig = torch.randint

            def rec(*a, **k):
                r = orig(*a, **k)
                idxs.append(r.numpy().copy())
                return r
            torch.randint = rec
            try:
                for c, d, w in sampler:
                    optim.zero_grad()
                    loss = nf.loss_func(d, phi.forward(c), w, float(thr))
                    loss.backward()
                    optim.step()
                    sch.step()
                    losses.append(loss.item())
            finally:
                torch.randint = orig
            pre = "%s_tr_%s_" % (kind, tag)
            arrs[pre + "features"] = np.array(float(feats), np.float64)
            arrs.update({pre + "init_" + k: v for k, v in init.items()})
            arrs.update(sd_arrays(phi, pre + "final_"))
            arrs[pre + "losses"] = np.array(losses, np.float64)
            idx = np.stack(idxs)
            assert idx.max() < 65536
            if "%s_tr_idx" % kind in arrs:      # the draws follow the init's: one stream per net kind, whatever the optimizer
                assert np.array_equal(arrs["%s_tr_idx" % kind], idx)
            arrs["%s_tr_idx" % kind] = idx.astype(np.uint16)
            if tag == "adamax":
                with tempfile.TemporaryDirectory() as td:
                    p = os.path.join(td, "module")
                    refsave.save_model(phi, p)
                    names = sorted(os.listdir(p))
                    arrs["%s_art_names" % kind] = np.array(names)
                    for j, fn in enumerate(names):
                        arrs["%s_art_f%d" % (kind, j)] = np.fromfile(os.path.join(p, fn), np.uint8)
                coords = refdataset.create_flattened_coords(TRACE_DIMS, cf.Compress.coords_mode)
                with torch.no_grad():
                    arrs["%s_art_decode" % kind] = phi.forward(coords.reshape(-1, 3)).numpy()


if __name__ == "__main__":
    torch.set_num_threads(1)
    arrs = {}
    g_init(arrs)
    g_budget(arrs)
    g_forward(arrs)
    g_trace(arrs)
    mg.save("taper", **arrs)
