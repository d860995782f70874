#!/usr/bin/env python3
"""Generate tests/golden/mfn.npz by RUNNING the reference's MFNFourier / MFNGabor (utils/Networks.py:648-799).

Runs only where the reference tree is present (CPU torch), like make_golden.py, whose stubs and helpers it imports unchanged: the
reference modules are imported in place and driven on small seeded inputs; inputs and outputs are stored as a .npz fixture.  Tests
only read the .npz.

    python tests/golden/make_golden_mfn.py

Contents (<k> one of "fourier" / "gabor"):
  <k>_init<i>_*   nets after different prior seeds: every state_dict entry (s<j>, in key order), the keys, the constructor arguments,
                  then torch.rand(5) drawn right after construction (the generator state the init leaves; MFN does not reseed)
  <k>_bud_rows    the reference's calc_features / calc_param_count over budgets, cin, cout and layers >= 3 (it divides by zero at 2)
  <k>_fwd<i>_*    reference forward (CPU fp32) on 256 random coordinates; the net is the reference's init right after
                  torch.manual_seed(<k>_fwd<i>_seed) (seeds, not weights: the init replay is exact)
  <k>_tr_<o>_*    a 30-step fit per optimizer / scheduler through the reference's NFGR (main.py: reproduc(42), prepare_module,
                  RandompointSampler, loss_func, optimizer + scheduler): final weights, losses and the recorded index stream (torch.randint
                  as the sampler draws it); the init is the reference's after reproduc(42); for adamax also the artefact the reference's
                  save_model writes (one torch.save file, raw bytes) and the reference's decode of the final net on the volume's grid
"""
import copy
import importlib.util
import os
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)          # stubs, sys.path and the reference imports of make_golden.py (its __main__ block does not run)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from utils.Networks import MFNFourier as RefFourier, MFNGabor as RefGabor  # noqa: E402
from utils import ModelSave as refsave  # noqa: E402
from utils import dataset as refdataset  # noqa: E402

KINDS = {"fourier": ("MFNFourier", RefFourier), "gabor": ("MFNGabor", RefGabor)}
INIT_CASES = [  # (cin, cout, features, layers, prior seed, input_scale, weight_scale, alpha, beta, output_act)
    (3, 1, 20, 5, 42, 256.0, 1.0, 6.0, 1.0, 0), (2, 3, 9, 3, 7, 64.0, 2.0, 3.0, 2.0, 1), (3, 2, 5, 2, 12345, 256.0, 1.0, 6.0, 1.0, 0),
    (3, 4, 33, 4, 99, 10.0, 0.5, 1.0, 0.5, 0)]
BUDGETS = [2e3, 3.3e4, 7.7e5, 3.3e6, 2.1e7, 6.7e7]
FWD_CASES = [   # (cin, cout, layers, features, output_act)
    (3, 1, 5, 1, 0), (3, 1, 5, 31, 0), (3, 1, 5, 33, 1), (2, 3, 4, 31, 0), (3, 4, 3, 33, 1), (3, 1, 5, 184, 0), (3, 1, 5, 525, 0),
    (3, 2, 3, 1024, 0), (2, 1, 2, 97, 1), (3, 1, 6, 65, 0)]
TRACE_CASES = {  # optimizer, scheduler (the YAML keys utils/misc.py:184-197 passes through)
    "adamax": ("Adamax", {"name": "MultiStepLR", "milestones": [10, 20], "gamma": 0.5}),
    "adam": ("Adam", {"name": "StepLR", "step_size": 7, "gamma": 0.7}),
    "sgd": ("SGD", {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 1e-2, "step_size_up": 5, "cycle_momentum": False}),
}
TRACE_DIMS, TRACE_F, TRACE_L, TRACE_N, TRACE_STEPS = (12, 20, 28), 24, 4, 1000, 30


def sd_arrays(m, prefix):
    out = {}
    sd = m.state_dict()
    for j, (k, v) in enumerate(sd.items()):
        out[prefix + "s%d" % j] = v.detach().numpy().copy()
    out[prefix + "keys"] = np.array(list(sd.keys()))
    return out


def g_init(arrs):
    for kind, (_, Ref) in KINDS.items():
        for i, (cin, cout, F, L, seed, isc, wsc, al, be, oa) in enumerate(INIT_CASES):
            torch.manual_seed(seed)
            m = Ref(coords_channel=cin, features=F, data_channel=cout, layers=L, input_scale=isc, weight_scale=wsc, alpha=al, beta=be,
                    output_act=bool(oa))
            arrs.update(sd_arrays(m, "%s_init%d_" % (kind, i)))
            arrs["%s_init%d_rand" % (kind, i)] = torch.rand(5).numpy()
            arrs["%s_init%d_cfg" % (kind, i)] = np.array([cin, cout, F, L, seed, isc, wsc, al, be, oa], np.float64)


def g_budget(arrs):
    for kind, (_, Ref) in KINDS.items():
        rows = []
        for P in BUDGETS:
            for cin, cout in ((2, 1), (3, 1), (3, 3), (2, 4)):
                for L in (3, 4, 5, 7):
                    F = Ref.calc_features(P, cin, cout, L)
                    if F < 1:
                        continue
                    rows.append([P, cin, cout, L, F, Ref.calc_param_count(cin, cout, F, L)])
        arrs["%s_bud_rows" % kind] = np.array(rows, np.float64)


def g_forward(arrs):
    for kind, (_, Ref) in KINDS.items():
        for i, (cin, cout, L, F, oa) in enumerate(FWD_CASES):
            seed = 1000 + i
            torch.manual_seed(seed)
            m = Ref(coords_channel=cin, features=F, data_channel=cout, layers=L, output_act=bool(oa))
            g = torch.Generator().manual_seed(100 + i)
            x = torch.rand(256, cin, generator=g) * 2 - 1
            with torch.no_grad():
                y = m(x)
            arrs["%s_fwd%d_cfg" % (kind, i)] = np.array([cin, cout, L, F, oa], np.int64)
            arrs["%s_fwd%d_seed" % (kind, i)] = np.array(seed, np.int64)
            arrs["%s_fwd%d_x" % (kind, i)] = x.numpy()
            arrs["%s_fwd%d_y" % (kind, i)] = y.numpy()


def g_trace(arrs):
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume(TRACE_DIMS, seed=43)
    arrs["tr_vol"] = vol
    for kind, (name, Ref) in KINDS.items():
        for tag, (optname, sched) in TRACE_CASES.items():
            opt = mg.load_opt()
            cf = opt.CompressFramework
            cf.Compress.gpu = False
            cf.Decompress.gpu = False
            cf.Module.phi = mg.to_attr({"name": name, "layers": TRACE_L, "coords_channel": 3, "data_channel": 1})
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
            pcount = Ref.calc_param_count(3, 1, TRACE_F, TRACE_L)
            feats, _ = nf.prepare_module(4.0 * pcount)
            assert feats == TRACE_F, feats
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
            arrs.update({pre + "init_" + k: v for k, v in init.items()})
            arrs.update(sd_arrays(phi, pre + "final_"))
            arrs[pre + "losses"] = np.array(losses, np.float64)
            arrs[pre + "idx"] = np.stack(idxs).astype(np.int64)
            if tag == "adamax":
                with tempfile.TemporaryDirectory() as td:
                    p = os.path.join(td, "module")
                    refsave.save_model(phi, p)
                    assert os.path.isfile(p)
                    with open(p, "rb") as f:
                        arrs["%s_art_bytes" % kind] = np.frombuffer(f.read(), np.uint8).copy()
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
    mg.save("mfn", **arrs)
