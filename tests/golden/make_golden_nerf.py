#!/usr/bin/env python3
"""Generate tests/golden/nerf.npz by RUNNING the reference's NeRF (utils/Networks.py:64-136).

Runs only where the reference tree is present (CPU torch), like make_golden.py, whose stubs and helpers it imports unchanged: the
reference modules are imported in place and driven on small seeded inputs; inputs and outputs are stored as a .npz fixture.  Tests
only read the .npz.

    python tests/golden/make_golden_nerf.py

Contents:
  init<k>_*       shapes after different prior seeds: every weight / bias, then torch.rand(5) drawn right after construction (the
                  global generator state the init leaves behind; NeRF does not reseed)
  bud_*           the reference's calc_features / calc_param_count over budgets, cin, cout, layers, skip and frequencies
  enc<k>_*        PosEncodingNeRF on 256 coordinates (x = +-1, 0 and linspace grid points among them), fp32
  fwd<k>_*        reference forward (CPU fp32) at the listed shapes on 256 random coordinates; the net is the reference's init right
                  after torch.manual_seed(fwd<k>_seed)
  tr_<o>_*        a 30-step fit per optimizer / scheduler through the reference's NFGR (main.py: reproduc(42), prepare_module,
                  RandompointSampler, loss_func, optimizer + scheduler): init and final weights, losses, the recorded index stream
                  (torch.randint as the sampler draws it), and for the first one the artefact files the reference's save_model writes
                  (raw bytes) and the reference's decode of the final net on the volume's grid
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

from utils.Networks import NeRF as RefNeRF, PosEncodingNeRF  # noqa: E402
from utils import ModelSave as refsave  # noqa: E402
from utils import dataset as refdataset  # noqa: E402

INIT_CASES = [  # (cin, cout, frequencies, features, layers, skip, prior seed)
    (3, 1, 10, 48, 5, 1, 42), (2, 3, 4, 70, 3, 1, 7), (3, 2, 16, 9, 4, 0, 12345), (3, 1, 0, 5, 2, 0, 3), (2, 1, 10, 20, 6, 1, 99)]
BUDGETS = [2e3, 3.3e4, 7.7e5, 3.3e6, 2.1e7]
ENC_CASES = [(3, 10), (2, 16), (3, 4)]   # (cin, frequencies)
FWD_CASES = [   # (cin, cout, layers, features, frequencies, skip)
    (3, 1, 5, 10, 10, 1), (3, 1, 5, 48, 10, 1), (3, 1, 5, 167, 10, 1), (3, 1, 5, 507, 10, 1), (2, 3, 3, 1, 4, 1), (3, 2, 3, 1024, 16, 1),
    (3, 1, 4, 33, 0, 0), (2, 1, 3, 100, 10, 0), (3, 3, 6, 65, 4, 1), (3, 1, 2, 97, 10, 0)]
TRACE_CASES = {  # optimizer, scheduler (the YAML keys utils/misc.py:184-197 passes through)
    "adamax": ("Adamax", {"name": "MultiStepLR", "milestones": [10, 20], "gamma": 0.5}),
    "adam": ("Adam", {"name": "StepLR", "step_size": 7, "gamma": 0.7}),
    "sgd": ("SGD", {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 1e-2, "step_size_up": 5, "cycle_momentum": False}),
}
TRACE_DIMS, TRACE_F, TRACE_L, TRACE_FREQ, TRACE_N, TRACE_STEPS = (12, 20, 28), 24, 4, 10, 1000, 30


def nerf_arrays(m, prefix):
    out = {}
    for l in range(len(m.net)):
        out[prefix + "w%d" % l] = m.net[l][0].weight.detach().numpy().copy()
        out[prefix + "b%d" % l] = m.net[l][0].bias.detach().numpy().copy()
    return out


def g_init(arrs):
    for k, (cin, cout, Lf, F, L, skip, seed) in enumerate(INIT_CASES):
        torch.manual_seed(seed)
        m = RefNeRF(coords_channel=cin, data_channel=cout, frequencies=Lf, features=F, layers=L, skip=bool(skip))
        arrs.update(nerf_arrays(m, "init%d_" % k))
        arrs["init%d_rand" % k] = torch.rand(5).numpy()
        arrs["init%d_cfg" % k] = np.array([cin, cout, Lf, F, L, skip, seed], np.int64)
        arrs["init%d_keys" % k] = np.array(list(m.state_dict().keys()))


def g_budget(arrs):
    rows = []
    for P in BUDGETS:
        for cin, cout in ((2, 1), (3, 1), (3, 3)):
            for L in (3, 4, 5, 7):
                for skip in (0, 1):
                    for Lf in (0, 4, 10, 16):
                        F = RefNeRF.calc_features(P, cin, cout, Lf, L, bool(skip))
                        if F < 1:
                            continue
                        rows.append([P, cin, cout, L, skip, Lf, F, RefNeRF.calc_param_count(cin, cout, F, Lf, L, bool(skip))])
    arrs["bud_rows"] = np.array(rows, np.float64)


def g_encoding(arrs):
    for k, (cin, Lf) in enumerate(ENC_CASES):
        g = torch.Generator().manual_seed(200 + k)
        x = torch.rand(256, cin, generator=g) * 2 - 1
        lin = torch.linspace(-1, 1, 97)
        x[:97, 0] = lin                  # grid points of a 97-long axis, -1 and +1 included
        x[97:110, cin - 1] = torch.linspace(-1, 1, 13)
        x[110] = 1.0
        x[111] = -1.0
        x[112] = 0.0
        with torch.no_grad():
            e = PosEncodingNeRF(cin, Lf)(x.clone())
        arrs["enc%d_cfg" % k] = np.array([cin, Lf], np.int64)
        arrs["enc%d_x" % k] = x.numpy()
        arrs["enc%d_y" % k] = e.numpy()


def g_forward(arrs):
    for k, (cin, cout, L, F, Lf, skip) in enumerate(FWD_CASES):
        torch.manual_seed(1000 + k)
        m = RefNeRF(coords_channel=cin, data_channel=cout, frequencies=Lf, features=F, layers=L, skip=bool(skip))
        g = torch.Generator().manual_seed(100 + k)
        x = torch.rand(256, cin, generator=g) * 2 - 1
        with torch.no_grad():
            y = m(x)
        arrs["fwd%d_cfg" % k] = np.array([cin, cout, L, F, Lf, skip], np.int64)
        arrs["fwd%d_seed" % k] = np.array(1000 + k, np.int64)
        arrs["fwd%d_x" % k] = x.numpy()
        arrs["fwd%d_y" % k] = y.numpy()


def g_trace(arrs):
    from brief_pytorch_amd.synthetic import make_volume
    vol = make_volume(TRACE_DIMS, seed=43)
    arrs["tr_vol"] = vol
    for tag, (optname, sched) in TRACE_CASES.items():
        opt = mg.load_opt()
        cf = opt.CompressFramework
        cf.Compress.gpu = False
        cf.Decompress.gpu = False
        cf.Module.phi = mg.to_attr({"name": "NeRF", "layers": TRACE_L, "coords_channel": 3, "data_channel": 1, "frequencies": TRACE_FREQ,
                                    "skip": True})
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
        pcount = RefNeRF.calc_param_count(3, 1, TRACE_F, TRACE_FREQ, TRACE_L, True)
        feats, _ = nf.prepare_module(4.0 * pcount)
        assert feats == TRACE_F, feats
        phi = nf.module["phi"]
        arrs.update(nerf_arrays(phi, "tr_%s_init_" % tag))
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
        arrs.update(nerf_arrays(phi, "tr_%s_final_" % tag))
        arrs["tr_%s_losses" % tag] = np.array(losses, np.float64)
        arrs["tr_%s_idx" % tag] = np.stack(idxs).astype(np.int64)
        if tag == "adamax":
            with tempfile.TemporaryDirectory() as td:
                p = os.path.join(td, "module")
                refsave.save_model(phi, p)
                names = sorted(os.listdir(p))
                arrs["art_names"] = np.array(names)
                for n in names:
                    with open(os.path.join(p, n), "rb") as f:
                        arrs["art_file_" + n] = np.frombuffer(f.read(), np.uint8).copy()
            coords = refdataset.create_flattened_coords(TRACE_DIMS, cf.Compress.coords_mode)
            with torch.no_grad():
                arrs["art_decode"] = phi.forward(coords.reshape(-1, 3)).numpy()


if __name__ == "__main__":
    torch.set_num_threads(1)
    arrs = {}
    g_init(arrs)
    g_budget(arrs)
    g_encoding(arrs)
    g_forward(arrs)
    g_trace(arrs)
    mg.save("nerf", **arrs)
