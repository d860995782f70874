"""NeRF (positional-encoding net) host-side logic: budget rule, init replay, module surface, artefact files and the C-ABI structs.

The reference module (utils/Networks.py:64-136) is restated here with torch.nn, in the reference's construction order: every
nn.Linear in layer order on the caller's global generator (no reseed), the skip layer (layers - 1) // 2 taking d + F inputs."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.fit import _is_siren
from brief_pytorch_amd.modelsave import load_model, save_model
from brief_pytorch_amd.networks import (ALL_CALC_PHI_FEATURES, ALL_CALC_PHI_PARAM_COUNT, ALLPHI, FFN, NeRF, SIREN,
                                        get_nnmodule_param_count, init_phi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_nerf(cin, cout, frequencies, features, layers, skip):
    """torch.nn construction of the reference's NeRF: returns its state_dict"""
    d = cin * (1 + 2 * frequencies)
    sl = (layers - 1) // 2 if skip else -1
    net = [torch.nn.Linear(d, features)] + [torch.nn.Linear(d + features if l == sl else features, features) for l in range(1, layers - 1)] \
        + [torch.nn.Linear(features, cout)]
    sd = {}
    for l, lin in enumerate(net):
        sd["net.%d.0.weight" % l] = lin.weight.detach()
        sd["net.%d.0.bias" % l] = lin.bias.detach()
    return sd


@pytest.mark.parametrize("side,F", [(64, 10), (128, 48), (256, 166), (512, 507), (1024, 1474)])
def test_default_yaml_widths(side, F):
    """opt/SingleTask/nerf.yaml: 5 layers, 10 frequencies, skip, uint16 volume, filesize_ratio 80, 4 bytes per parameter"""
    P = side ** 3 * 2 / 80 / 4
    assert ALL_CALC_PHI_FEATURES["NeRF"](param_count=P, coords_channel=3, data_channel=1, layers=5, frequencies=10, skip=True) == F


def test_budget_matches_the_reference_golden(golden):
    g = golden("nerf")
    rows = g["bud_rows"]
    assert len(rows) > 100
    for P, cin, cout, L, skip, Lf, F, count in rows:
        kw = dict(coords_channel=int(cin), data_channel=int(cout), layers=int(L), skip=bool(skip), frequencies=int(Lf))
        assert NeRF.calc_features(P, **kw) == int(F)
        assert ALL_CALC_PHI_PARAM_COUNT["NeRF"](features=int(F), **kw) == int(count)


def test_budget_linear_case():
    """layers = 2 without skip: the reference divides by zero; the port solves the linear equation"""
    F = NeRF.calc_features(1000, 3, 1, frequencies=10, layers=2, skip=False)
    assert F == round((1000 - 1) / (63 + 1 + 1))
    assert abs(NeRF.calc_param_count(3, 1, F, frequencies=10, layers=2, skip=False) - 1000) <= 63 + 2


def test_init_matches_the_reference_golden(golden):
    g = golden("nerf")
    k = 0
    while "init%d_cfg" % k in g:
        cin, cout, Lf, F, L, skip, seed = (int(v) for v in g["init%d_cfg" % k])
        torch.manual_seed(seed)
        m = NeRF(coords_channel=cin, data_channel=cout, frequencies=Lf, features=F, layers=L, skip=bool(skip))
        after = torch.rand(5).numpy()
        sd = m.state_dict()
        assert list(sd.keys()) == [str(v) for v in g["init%d_keys" % k]]
        for l in range(L):
            assert np.array_equal(m.net[l][0].weight.data.numpy(), g["init%d_w%d" % (k, l)]), (k, l)
            assert np.array_equal(m.net[l][0].bias.data.numpy(), g["init%d_b%d" % (k, l)]), (k, l)
        assert np.array_equal(after, g["init%d_rand" % k]), "torch.rand right after construction"
        k += 1
    assert k == 5


@pytest.mark.parametrize("shape,prior_seed", [((3, 1, 10, 48, 5, True), 42), ((2, 3, 4, 70, 3, True), 7), ((3, 2, 16, 9, 4, False), 5)])
def test_init_bit_identical_and_rng_state(shape, prior_seed):
    cin, cout, Lf, F, L, skip = shape
    torch.manual_seed(prior_seed)
    m = NeRF(coords_channel=cin, data_channel=cout, frequencies=Lf, features=F, layers=L, skip=skip)
    after = torch.rand(5)
    torch.manual_seed(prior_seed)
    ref = reference_nerf(cin, cout, Lf, F, L, skip)
    ref_after = torch.rand(5)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert sd[k].shape == ref[k].shape, k
        assert torch.equal(sd[k], ref[k]), k
    assert torch.equal(after, ref_after), "the global generator continues from the same state after the init"


def test_surface_and_param_count():
    m = init_phi({"name": "NeRF", "coords_channel": 3, "data_channel": 1, "features": 48, "layers": 5, "frequencies": 10, "skip": True,
                  "w0": 20, "output_act": False, "res": False, "embsize": 256})
    assert isinstance(m, NeRF) and ALLPHI["NeRF"] is NeRF and m.kind == "NeRF" and not _is_siren(m)
    assert get_nnmodule_param_count(m) == NeRF.calc_param_count(3, 1, 48, frequencies=10, layers=5, skip=True) == m.param_count
    assert m.positional_encoding.out_channel == 63 and m.skip_layer == 2
    assert [tuple(m.net[l][0].weight.shape) for l in range(5)] == [(48, 63), (48, 48), (48, 111), (48, 48), (1, 48)]
    assert list(m.state_dict().keys()) == ["net.%d.0.%s" % (l, w) for l in range(5) for w in ("weight", "bias")]
    assert m.parameters()[0].numel() == m.param_count
    d = NeRF()                               # the reference constructor's defaults
    assert (d.coords_channel, d.data_channel, d.frequencies, d.features, d.layers, d.skip) == (3, 1, 10, 256, 5, True)
    # a Module.phi spec names frequencies and skip (the reference's budget rule has no default for them)
    for spec in ({"name": "NeRF"}, {"name": "NeRF", "features": 48, "skip": True}, {"name": "NeRF", "features": 48, "frequencies": 10}):
        with pytest.raises(NotImplementedError, match="without"):
            init_phi(spec)
    with pytest.raises(TypeError):
        NeRF.calc_features(1e5, 3, 1)
    assert _is_siren(SIREN(features=4)) and not _is_siren(FFN(features=4, embsize=4))


def test_refusals_name_the_limit():
    with pytest.raises(NotImplementedError, match="layers must be >= 2, and >= 3 with skip"):
        NeRF(layers=2, skip=True)
    with pytest.raises(NotImplementedError, match="1..1024"):
        NeRF(features=1474)
    with pytest.raises(NotImplementedError, match="0..16"):
        NeRF(frequencies=17)
    with pytest.raises(NotImplementedError, match="coords_channel"):
        NeRF(coords_channel=4)
    with pytest.raises(NotImplementedError, match="data_channel"):
        NeRF(data_channel=5)
    with pytest.raises(NotImplementedError, match="MFNFourier"):
        init_phi({"name": "MFNFourier"})
    assert NeRF(layers=2, skip=False, features=3).param_count == 3 * 63 + 3 + 3 + 1
    assert NeRF(features=4, precision="bf16").precision == "fp32"      # no low-precision NeRF kernels: fp32, with a warning
    assert NeRF(features=4).half().precision == "fp32"


def test_artefact_files_are_the_reference_layout(tmp_path):
    torch.manual_seed(1)
    m = NeRF(coords_channel=3, data_channel=1, frequencies=4, features=9, layers=3, skip=True)
    d = str(tmp_path / "module")
    save_model(m, d)
    names = sorted(os.listdir(d))
    assert names == sorted(["weight-0-9-27", "bias-0-9", "weight-1-9-36", "bias-1-9", "weight-2-1-9", "bias-2-1"])
    w1 = np.fromfile(os.path.join(d, "weight-1-9-36"), dtype=np.float32)
    assert np.array_equal(w1, m.net[1][0].weight.data.numpy().reshape(-1))
    torch.manual_seed(99)
    m2 = NeRF(coords_channel=3, data_channel=1, frequencies=4, features=9, layers=3, skip=True)
    load_model(m2, d)
    assert torch.equal(m2.params, m.params)


def test_reference_artefact_loads_and_round_trips_byte_for_byte(golden, tmp_path):
    """the weight files the reference's save_model wrote for its fitted NeRF load here, and save_model writes them back identically"""
    g = golden("nerf")
    src = tmp_path / "ref"
    src.mkdir()
    names = [str(n) for n in g["art_names"]]
    assert "weight-1-24-87" in names        # the skip layer of a 4-layer net is net[1] ((4 - 1) // 2), [F, d + F]
    for n in names:
        (src / n).write_bytes(g["art_file_" + n].tobytes())
    m = NeRF(coords_channel=3, data_channel=1, frequencies=10, features=24, layers=4, skip=True)
    load_model(m, str(src))
    for l in range(4):
        assert np.array_equal(m.net[l][0].weight.data.numpy(), g["tr_adamax_final_w%d" % l])
        assert np.array_equal(m.net[l][0].bias.data.numpy(), g["tr_adamax_final_b%d" % l])
    out = str(tmp_path / "ours")
    save_model(m, out)
    assert sorted(os.listdir(out)) == sorted(names)
    for n in names:
        with open(os.path.join(out, n), "rb") as f:
            assert f.read() == g["art_file_" + n].tobytes(), n


def test_c_abi_sizes_and_refusals():
    L = _lib.lib()
    for (cin, cout, layers, F, Lf, skip) in ((3, 1, 5, 167, 10, 1), (2, 3, 3, 1, 0, 0), (3, 2, 6, 1024, 16, 1), (3, 1, 2, 5, 4, 0)):
        d = _lib.NerfDesc(cin, cout, layers, F, Lf, skip)
        assert L.brief_nerf_param_count(C.byref(d)) == NeRF.calc_param_count(cin, cout, F, frequencies=Lf, layers=layers, skip=bool(skip))
        assert L.brief_nerf_packed_count(C.byref(d)) > 0
        assert L.brief_nerf_train_workspace_bytes(C.byref(d), 100000) > 0
    for bad, msg in ((_lib.NerfDesc(3, 1, 5, 1474, 10, 1), b"features must be 1..1024"), (_lib.NerfDesc(3, 1, 5, 100, 17, 1), b"frequencies must be 0..16"),
                     (_lib.NerfDesc(3, 1, 2, 100, 10, 1), b">= 3 with skip"), (_lib.NerfDesc(4, 1, 5, 100, 10, 1), b"coords_channel"),
                     (_lib.NerfDesc(3, 5, 5, 100, 10, 1), b"data_channel"), (_lib.NerfDesc(3, 1, 1, 100, 10, 0), b"layers"),
                     (_lib.NerfDesc(3, 1, 5, 100, 10, 2), b"skip must be 0 or 1")):
        assert L.brief_nerf_param_count(C.byref(bad)) == -1
        assert msg in L.brief_last_error()
        assert L.brief_nerf_repack(C.byref(bad), None, None, None) == -1


def test_struct_offsets_match_the_header(tmp_path):
    """a compiled C probe of brief_nerf_desc / brief_nerf_fit_job offsets against ctypes"""
    fields = [f for f, _ in _lib.NerfFitJob._fields_]
    src = tmp_path / "probe.c"
    body = "".join('printf("%%zu\\n", offsetof(brief_nerf_fit_job, %s));' % f for f in fields)
    body += "".join('printf("%%zu\\n", offsetof(brief_nerf_desc, %s));' % f for f, _ in _lib.NerfDesc._fields_)
    body += 'printf("%zu\\n%zu\\n", sizeof(brief_nerf_fit_job), sizeof(brief_nerf_desc));'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "brief_hip.h"\nint main(void){%s return 0;}\n' % body)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [getattr(_lib.NerfFitJob, f).offset for f in fields] + [getattr(_lib.NerfDesc, f).offset for f, _ in _lib.NerfDesc._fields_] \
        + [C.sizeof(_lib.NerfFitJob), C.sizeof(_lib.NerfDesc)]
    assert got == want


def test_nerf_yaml():
    import yaml
    with open(os.path.join(ROOT, "opt", "SingleTask", "nerf.yaml")) as f:
        y = yaml.safe_load(f)
    with open(os.path.join(ROOT, "opt", "SingleTask", "default.yaml")) as f:
        base = yaml.safe_load(f)
    assert y["CompressFramework"]["Module"]["phi"] == {"name": "NeRF", "layers": 5, "frequencies": 10, "skip": True, "coords_channel": 3,
                                                      "data_channel": 1}
    y["CompressFramework"]["Module"] = base["CompressFramework"]["Module"]
    assert y == base
