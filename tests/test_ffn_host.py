"""FFN (Fourier-feature net) host-side logic: budget rule, init replay, module surface, artefact files and the C-ABI structs.

The reference module (utils/Networks.py:138-207) is restated here with torch.nn, in the reference's construction order:
FourierFeatureEmbedding reseeds the global generator with 0 and draws bvals = normal(0, 1) * scale, then every nn.Linear of the
MLP is built in layer order."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.modelsave import load_model, save_model
from brief_pytorch_amd.networks import ALL_CALC_PHI_FEATURES, ALL_CALC_PHI_PARAM_COUNT, FFN, get_nnmodule_param_count, init_phi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_ffn(cin, cout, embsize, scale, features, layers):
    """torch.nn construction of the reference's FFN(skip=False): returns its state_dict"""
    torch.manual_seed(0)
    bvals = torch.normal(0, 1, size=(embsize, cin)) * scale
    net = [torch.nn.Linear(2 * embsize, features)] + [torch.nn.Linear(features, features) for _ in range(layers - 2)] \
        + [torch.nn.Linear(features, cout)]
    sd = {"fourierfeature_embedding.bvals": bvals}
    for l, lin in enumerate(net):
        sd["net.%d.0.weight" % l] = lin.weight.detach()
        sd["net.%d.0.bias" % l] = lin.bias.detach()
    return sd


def ref_param_count(cin, cout, features, embsize, layers):
    d = 2 * embsize
    return int(d * features + features + (layers - 2) * (features ** 2 + features) + features * cout + cout + cin * embsize)


def ref_features(P, cin, cout, embsize, layers):
    d = 2 * embsize
    a, b, c = layers - 2, d + 1 + layers - 2 + cout, -P + cout + cin * embsize
    return round((-b + math.sqrt(b ** 2 - 4 * a * c)) / (2 * a))


@pytest.mark.parametrize("side,F", [(64, 2), (128, 21), (256, 119), (512, 449), (1024, 1412)])
def test_default_yaml_widths(side, F):
    """opt/SingleTask/default.yaml: 5 layers, E = 256, uint16 volume, filesize_ratio 80, 4 bytes per parameter"""
    P = side ** 3 * 2 / 80 / 4
    assert ALL_CALC_PHI_FEATURES["FFN"](param_count=P, coords_channel=3, data_channel=1, layers=5, embsize=256) == F


def test_budget_sweep():
    for P in (3e3, 5e4, 7.7e5, 3.3e6, 2.1e7):
        for E in (16, 64, 256, 512):
            for L in (3, 4, 5, 7):
                for cin, cout in ((2, 1), (3, 1), (3, 3)):
                    if P < cin * E + 8 * E:
                        continue
                    F = FFN.calc_features(P, cin, cout, embsize=E, layers=L)
                    assert F == ref_features(P, cin, cout, E, L)
                    assert ALL_CALC_PHI_PARAM_COUNT["FFN"](coords_channel=cin, data_channel=cout, features=F, embsize=E, layers=L) \
                        == ref_param_count(cin, cout, F, E, L)


@pytest.mark.parametrize("shape,prior_seed", [((3, 1, 256, 10, 21, 5), 42), ((2, 3, 16, 3.5, 70, 3), 7), ((3, 2, 100, 10, 9, 2), 12345)])
def test_init_bit_identical_and_rng_state(shape, prior_seed):
    cin, cout, E, scale, F, L = shape
    torch.manual_seed(prior_seed)
    m = FFN(coords_channel=cin, data_channel=cout, embsize=E, scale=scale, features=F, layers=L)
    after = torch.rand(5)
    torch.manual_seed(prior_seed + 1)
    ref = reference_ffn(cin, cout, E, scale, F, L)
    ref_after = torch.rand(5)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert sd[k].shape == ref[k].shape, k
        assert torch.equal(sd[k], ref[k]), k
    assert torch.equal(after, ref_after), "the global generator continues from the same state after the init"


def test_surface_and_param_count():
    m = init_phi({"name": "FFN", "coords_channel": 3, "data_channel": 1, "features": 21, "layers": 5, "w0": 20, "output_act": False,
                  "res": False})
    assert isinstance(m, FFN)
    assert get_nnmodule_param_count(m) == FFN.calc_param_count(3, 1, 21, embsize=256, layers=5) == m.param_count
    assert m.fourierfeature_embedding.bvals.shape == (256, 3)
    assert m.fourierfeature_embedding.requires_grad is False
    assert [tuple(m.net[l][0].weight.shape) for l in range(5)] == [(21, 512), (21, 21), (21, 21), (21, 21), (1, 21)]
    assert m.parameters()[0].numel() == m.param_count


def test_nerf_and_limits_refused():
    with pytest.raises(NotImplementedError):
        init_phi({"name": "NeRF"})
    with pytest.raises(NotImplementedError, match="skip"):
        FFN(skip=True)
    with pytest.raises(NotImplementedError, match="1..1024"):
        FFN(features=1412)
    with pytest.raises(NotImplementedError, match="1..512"):
        FFN(embsize=600)
    assert FFN(features=4, embsize=4, precision="bf16").precision == "fp32"      # no low-precision FFN kernels: fp32, with a warning


def test_artefact_files_are_the_reference_layout(tmp_path):
    torch.manual_seed(1)
    m = FFN(coords_channel=3, data_channel=1, embsize=32, features=9, layers=3)
    d = str(tmp_path / "module")
    save_model(m, d)
    names = sorted(os.listdir(d))
    assert names == sorted(["weight-0-9-64", "bias-0-9", "weight-1-9-9", "bias-1-9", "weight-2-1-9", "bias-2-1"])
    # raw native float32, row-major [out, in] (utils/ModelSave.py:32-50)
    w0 = np.fromfile(os.path.join(d, "weight-0-9-64"), dtype=np.float32)
    assert np.array_equal(w0, m.net[0][0].weight.data.numpy().reshape(-1))
    # round trip into a fresh net of another seed: MLP from the files, bvals from the init
    torch.manual_seed(99)
    m2 = FFN(coords_channel=3, data_channel=1, embsize=32, features=9, layers=3)
    for l in range(3):
        m2.net[l][0].weight.data = torch.zeros_like(m2.net[l][0].weight.data)
    load_model(m2, d)
    assert torch.equal(m2.params, m.params)


def test_c_abi_sizes_and_refusals():
    L = _lib.lib()
    d = _lib.FfnDesc(3, 1, 5, 119, 256, 0)
    assert L.brief_ffn_param_count(C.byref(d)) == FFN.calc_param_count(3, 1, 119, embsize=256, layers=5)
    assert L.brief_ffn_packed_count(C.byref(d)) > 0
    assert L.brief_ffn_train_workspace_bytes(C.byref(d), 100000) > 0
    for bad, msg in ((_lib.FfnDesc(3, 1, 5, 1412, 256, 0), b"features must be 1..1024"), (_lib.FfnDesc(3, 1, 5, 100, 513, 0), b"embsize must be 1..512"),
                     (_lib.FfnDesc(3, 1, 5, 100, 256, 1), b"skip connections"), (_lib.FfnDesc(4, 1, 5, 100, 256, 0), b"coords_channel"),
                     (_lib.FfnDesc(3, 5, 5, 100, 256, 0), b"data_channel"), (_lib.FfnDesc(3, 1, 1, 100, 256, 0), b"layers")):
        assert L.brief_ffn_param_count(C.byref(bad)) == -1
        assert msg in L.brief_last_error()
        assert L.brief_ffn_repack(C.byref(bad), None, None, None) == -1


def test_struct_offsets_match_the_header(tmp_path):
    """a compiled C probe of brief_ffn_desc / brief_ffn_fit_job offsets against ctypes"""
    fields = [f for f, _ in _lib.FfnFitJob._fields_]
    src = tmp_path / "probe.c"
    body = "".join('printf("%%zu\\n", offsetof(brief_ffn_fit_job, %s));' % f for f in fields)
    body += "".join('printf("%%zu\\n", offsetof(brief_ffn_desc, %s));' % f for f, _ in _lib.FfnDesc._fields_)
    body += 'printf("%zu\\n%zu\\n", sizeof(brief_ffn_fit_job), sizeof(brief_ffn_desc));'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "brief_hip.h"\nint main(void){%s return 0;}\n' % body)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [getattr(_lib.FfnFitJob, f).offset for f in fields] + [getattr(_lib.FfnDesc, f).offset for f, _ in _lib.FfnDesc._fields_] \
        + [C.sizeof(_lib.FfnFitJob), C.sizeof(_lib.FfnDesc)]
    assert got == want


# ---- against the reference's own code: tests/golden/ffn.npz (tests/golden/make_golden_ffn.py runs the reference's FFN)
def test_init_matches_the_reference_golden(golden):
    g = golden("ffn")
    k = 0
    while "init%d_cfg" % k in g:
        cin, cout, E, scale, F, L, seed = g["init%d_cfg" % k]
        torch.manual_seed(int(seed))
        m = FFN(coords_channel=int(cin), data_channel=int(cout), embsize=int(E), scale=float(scale), features=int(F), layers=int(L))
        after = torch.rand(5).numpy()
        assert np.array_equal(m.fourierfeature_embedding.bvals.data.numpy(), g["init%d_bvals" % k])
        for l in range(int(L)):
            assert np.array_equal(m.net[l][0].weight.data.numpy(), g["init%d_w%d" % (k, l)]), (k, l)
            assert np.array_equal(m.net[l][0].bias.data.numpy(), g["init%d_b%d" % (k, l)]), (k, l)
        assert np.array_equal(after, g["init%d_rand" % k]), "torch.rand right after construction"
        k += 1
    assert k == 3


def test_reference_artefact_loads_and_round_trips_byte_for_byte(golden, tmp_path):
    """the weight files the reference's save_model wrote for its fitted FFN load here, and save_model writes them back identically"""
    g = golden("ffn")
    src = tmp_path / "ref"
    src.mkdir()
    names = [str(n) for n in g["art_names"]]
    for n in names:
        (src / n).write_bytes(g["art_file_" + n].tobytes())
    m = FFN(coords_channel=3, data_channel=1, embsize=256, features=24, layers=4)
    load_model(m, str(src))
    assert np.array_equal(m.fourierfeature_embedding.bvals.data.numpy(), g["tr_adamax_final_bvals"])
    for l in range(4):
        assert np.array_equal(m.net[l][0].weight.data.numpy(), g["tr_adamax_final_w%d" % l])
        assert np.array_equal(m.net[l][0].bias.data.numpy(), g["tr_adamax_final_b%d" % l])
    out = str(tmp_path / "ours")
    save_model(m, out)
    assert sorted(os.listdir(out)) == sorted(names)
    for n in names:
        with open(os.path.join(out, n), "rb") as f:
            assert f.read() == g["art_file_" + n].tobytes(), n
