"""MFNFourier / MFNGabor host-side logic: budget rule, init replay, module surface, state_dict artefact, refusals, the C-ABI structs,
the YAMLs and get_folder_size on a single-file artefact.  Goldens: tests/golden/mfn.npz (tests/golden/make_golden_mfn.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd import io as bio
from brief_pytorch_amd.fit import _is_siren
from brief_pytorch_amd.modelsave import load_model, save_model
from brief_pytorch_amd.networks import ALL_CALC_PHI_FEATURES, ALL_CALC_PHI_PARAM_COUNT, ALLPHI, MFNFourier, MFNGabor, init_phi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"fourier": MFNFourier, "gabor": MFNGabor}
WIDTHS = {"MFNFourier": [20, 63, 184, 525, 1492], "MFNGabor": [18, 60, 181, 523, 1490]}


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_default_yaml_widths(name):
    """default.yaml's budget (ratio 80, uint16, 4 bytes / parameter, 5 layers, 3 -> 1) with phi.name changed"""
    for side, F in zip((64, 128, 256, 512, 1024), WIDTHS[name]):
        P = side ** 3 * 2 / 80 / 4
        assert ALL_CALC_PHI_FEATURES[name](param_count=P, coords_channel=3, data_channel=1, layers=5) == F
    with pytest.raises(NotImplementedError, match="1..1024"):
        ALLPHI[name](coords_channel=3, data_channel=1, layers=5, features=WIDTHS[name][-1])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_budget_matches_the_reference_golden(golden, kind):
    rows = golden("mfn")["%s_bud_rows" % kind]
    assert len(rows) > 50
    cls = KINDS[kind]
    for P, cin, cout, L, F, count in rows:
        kw = dict(coords_channel=int(cin), data_channel=int(cout), layers=int(L))
        assert cls.calc_features(P, **kw) == int(F)
        assert ALL_CALC_PHI_PARAM_COUNT[cls.kind](features=int(F), **kw) == int(count)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_budget_linear_case(kind):
    """layers = 2: the reference divides by zero; the port solves the linear equation"""
    cls = KINDS[kind]
    k = 1 if kind == "fourier" else 2
    F = cls.calc_features(1000, 3, 1, layers=2)
    assert F == round((1000 - 1) / (1 + k * 4))
    assert cls.calc_param_count(3, 1, F, 2) == F + 1 + k * (3 * F + F) == cls(coords_channel=3, data_channel=1, features=F, layers=2).param_count


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_init_matches_the_reference_golden(golden, kind):
    g = golden("mfn")
    cls = KINDS[kind]
    for i in range(4):
        cin, cout, F, L, seed, isc, wsc, al, be, oa = g["%s_init%d_cfg" % (kind, i)]
        torch.manual_seed(int(seed))
        m = cls(coords_channel=int(cin), features=int(F), data_channel=int(cout), layers=int(L), input_scale=isc, weight_scale=wsc,
                alpha=al, beta=be, output_act=bool(oa))
        after = torch.rand(5).numpy()
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in g["%s_init%d_keys" % (kind, i)]]
        for j, k in enumerate(sd):
            assert np.array_equal(sd[k].numpy(), g["%s_init%d_s%d" % (kind, i, j)]), (i, k)
        assert np.array_equal(after, g["%s_init%d_rand" % (kind, i)]), "torch.rand right after construction"


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_state_dict_keys_shapes_storages_and_surface(kind):
    cls = KINDS[kind]
    m = init_phi({"name": cls.kind, "coords_channel": 3, "data_channel": 2, "features": 7, "layers": 4, "w0": 20, "res": False,
                  "output_act": False})
    assert isinstance(m, cls) and m.kind == cls.kind and not _is_siren(m) and not hasattr(m, "net")
    sd = m.state_dict()
    want = ["linear.0.weight", "linear.0.bias", "linear.1.weight", "linear.1.bias", "output_linear.weight", "output_linear.bias"]
    for i in range(3):
        want += (["filters.%d.mu" % i, "filters.%d.gamma" % i] if kind == "gabor" else []) + ["filters.%d.linear.weight" % i,
                                                                                               "filters.%d.linear.bias" % i]
    assert list(sd.keys()) == want
    shapes = {"linear.0.weight": (7, 7), "output_linear.weight": (2, 7), "filters.2.linear.weight": (7, 3), "filters.1.linear.bias": (7,)}
    if kind == "gabor":
        shapes.update({"filters.0.mu": (7, 3), "filters.2.gamma": (7,)})
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    for k, v in sd.items():
        assert v.dtype == torch.float32 and v.device.type == "cpu" and v.is_contiguous()
        assert v.untyped_storage().nbytes() == 4 * v.numel(), "%s: own storage of exactly its size" % k
    assert sum(v.numel() for v in sd.values()) == m.param_count == cls.calc_param_count(3, 2, 7, 4)
    # windows into the canonical buffer: readable and assignable
    assert torch.equal(m.linear[1].weight.data, sd["linear.1.weight"]) and torch.equal(m.output_linear.bias.data, sd["output_linear.bias"])
    m.filters[2].linear.weight.data = torch.ones(7, 3)
    assert torch.equal(m.state_dict()["filters.2.linear.weight"], torch.ones(7, 3))
    if kind == "gabor":
        m.filters[0].gamma.data = torch.full((7,), 2.5)
        assert torch.equal(m.state_dict()["filters.0.gamma"], torch.full((7,), 2.5))
        assert torch.equal(m.filters[1].mu.data, sd["filters.1.mu"])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_save_model_writes_one_file_that_loads_weights_only(kind, tmp_path):
    cls = KINDS[kind]
    torch.manual_seed(1)
    m = cls(coords_channel=3, data_channel=1, features=9, layers=3)
    p = str(tmp_path / "module")
    save_model(m, p)
    assert os.path.isfile(p)
    sd = torch.load(p, weights_only=True)
    assert list(sd.keys()) == list(m.state_dict().keys())
    assert bio.get_folder_size(p) == os.path.getsize(p) > 4 * m.param_count
    torch.manual_seed(99)
    m2 = cls(coords_channel=3, data_channel=1, features=9, layers=3)
    load_model(m2, p)
    assert torch.equal(m2.params, m.params)
    with pytest.raises(KeyError, match="missing keys"):
        m2.load_state_dict({k: v for k, v in sd.items() if k != "output_linear.bias"})


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reference_artefact_loads(golden, kind, tmp_path):
    """the single torch.save file the reference's save_model wrote loads through load_model; keys, shapes and values equal the
    reference's final weights"""
    g = golden("mfn")
    p = tmp_path / "module"
    p.write_bytes(g["%s_art_bytes" % kind].tobytes())
    ref = torch.load(str(p), weights_only=True)
    m = KINDS[kind](coords_channel=3, features=24, data_channel=1, layers=4)
    load_model(m, str(p))
    sd = m.state_dict()
    pre = "%s_tr_adamax_final_" % kind
    assert list(sd.keys()) == list(ref.keys()) == [str(k) for k in g[pre + "keys"]]
    for j, k in enumerate(sd):
        assert sd[k].shape == ref[k].shape and torch.equal(sd[k], ref[k])
        assert np.array_equal(sd[k].numpy(), g[pre + "s%d" % j])


def test_refusals_name_the_limit():
    with pytest.raises(NotImplementedError, match="bias=False"):
        MFNFourier(bias=False)
    with pytest.raises(NotImplementedError, match="bias=False"):
        MFNGabor(bias=False)
    with pytest.raises(NotImplementedError, match="1..1024"):
        MFNGabor(features=1025)
    with pytest.raises(NotImplementedError, match="layers must be >= 2"):
        MFNFourier(layers=1)
    with pytest.raises(NotImplementedError, match="coords_channel"):
        MFNFourier(coords_channel=4)
    with pytest.raises(NotImplementedError, match="data_channel"):
        MFNGabor(data_channel=5)
    with pytest.raises(NotImplementedError, match="without coords_channel"):
        init_phi({"name": "MFNGabor", "features": 8})
    assert MFNGabor(features=4, precision="bf16").precision == "fp32"      # no low-precision MFN kernels: fp32, with a warning
    assert MFNFourier(features=4).half().precision == "fp32"
    d = MFNFourier()                                                         # the reference constructor's defaults
    assert (d.coords_channel, d.features, d.data_channel, d.layers, d.input_scale, d.weight_scale, d.output_act) == (3, 256, 1, 5, 256.0, 1.0, False)
    e = MFNGabor(features=4)
    assert (e.alpha, e.beta) == (6.0, 1.0)


def test_c_abi_sizes_and_refusals():
    L = _lib.lib()
    for (cin, cout, layers, F, flt, oa) in ((3, 1, 5, 184, 0, 0), (2, 3, 3, 1, 1, 1), (3, 2, 6, 1024, 1, 0), (3, 4, 2, 5, 0, 1)):
        d = _lib.MfnDesc(cin, cout, layers, F, flt, oa)
        cls = MFNGabor if flt else MFNFourier
        assert L.brief_mfn_param_count(C.byref(d)) == cls.calc_param_count(cin, cout, F, layers)
        assert L.brief_mfn_packed_count(C.byref(d)) > 0
        assert L.brief_mfn_train_workspace_bytes(C.byref(d), 100000) > 0
    for bad, msg in ((_lib.MfnDesc(3, 1, 5, 1025, 0, 0), b"features must be 1..1024"), (_lib.MfnDesc(4, 1, 5, 100, 0, 0), b"coords_channel"),
                     (_lib.MfnDesc(3, 5, 5, 100, 0, 0), b"data_channel"), (_lib.MfnDesc(3, 1, 1, 100, 0, 0), b"layers must be >= 2"),
                     (_lib.MfnDesc(3, 1, 5, 100, 2, 0), b"filter must be 0"), (_lib.MfnDesc(3, 1, 5, 100, 1, 2), b"output_act must be 0 or 1")):
        assert L.brief_mfn_param_count(C.byref(bad)) == -1
        assert msg in L.brief_last_error()
        assert L.brief_mfn_repack(C.byref(bad), None, None, None) == -1


def test_struct_offsets_match_the_header(tmp_path):
    """a compiled C probe of brief_mfn_desc / brief_mfn_fit_job offsets against ctypes"""
    fields = [f for f, _ in _lib.MfnFitJob._fields_]
    src = tmp_path / "probe.c"
    body = "".join('printf("%%zu\\n", offsetof(brief_mfn_fit_job, %s));' % f for f in fields)
    body += "".join('printf("%%zu\\n", offsetof(brief_mfn_desc, %s));' % f for f, _ in _lib.MfnDesc._fields_)
    body += 'printf("%zu\\n%zu\\n", sizeof(brief_mfn_fit_job), sizeof(brief_mfn_desc));'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "brief_hip.h"\nint main(void){%s return 0;}\n' % body)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [getattr(_lib.MfnFitJob, f).offset for f in fields] + [getattr(_lib.MfnDesc, f).offset for f, _ in _lib.MfnDesc._fields_] \
        + [C.sizeof(_lib.MfnFitJob), C.sizeof(_lib.MfnDesc)]
    assert got == want


@pytest.mark.parametrize("name,fname", [("MFNFourier", "mfn_fourier.yaml"), ("MFNGabor", "mfn_gabor.yaml")])
def test_mfn_yamls(name, fname):
    import yaml
    with open(os.path.join(ROOT, "opt", "SingleTask", fname)) as f:
        y = yaml.safe_load(f)
    with open(os.path.join(ROOT, "opt", "SingleTask", "default.yaml")) as f:
        base = yaml.safe_load(f)
    assert y["CompressFramework"]["Module"]["phi"]["name"] == name
    y["CompressFramework"]["Module"]["phi"]["name"] = "SIREN"
    assert y == base, "default.yaml with phi.name changed"
    phi = {k: v for k, v in base["CompressFramework"]["Module"]["phi"].items() if k != "name"}
    assert [ALL_CALC_PHI_FEATURES[name](param_count=s ** 3 * 2 / 80 / 4, **phi) for s in (64, 128, 256, 512)] == WIDTHS[name][:4]


def test_get_folder_size_on_a_file(tmp_path):
    p = tmp_path / "module"
    p.write_bytes(b"x" * 1234)
    assert bio.get_folder_size(str(p)) == 1234
    d = tmp_path / "dir"
    d.mkdir()
    (d / "a").write_bytes(b"y" * 10)
    (d / "b").write_bytes(b"z" * 7)
    assert bio.get_folder_size(str(d)) == 17


def test_brief_sincosf_at_filter_phases(tmp_path):
    """the filters' sine (brief_sincosf, csrc/brief_math.h) against float64 over the phases the default init reaches (|a| <= 400)"""
    src, so = str(tmp_path / "p.cpp"), str(tmp_path / "p.so")
    with open(src, "w") as f:
        f.write('#include <math.h>\n#include "brief_math.h"\nextern "C" void probe(const float *x, float *s, float *c, long n) '
                '{ for (long i = 0; i < n; ++i) brief_sincosf(x[i], s + i, c + i); }\n')
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "brief_pytorch_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    x = np.random.default_rng(1).uniform(-400, 400, 400000).astype(np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    fp = C.POINTER(C.c_float)
    lib.probe(x.ctypes.data_as(fp), s.ctypes.data_as(fp), c.ctypes.data_as(fp), C.c_long(x.size))
    xd = x.astype(np.float64)
    assert np.max(np.abs(s - np.sin(xd))) <= 1.5e-7 and np.max(np.abs(c - np.cos(xd))) <= 1.5e-7
