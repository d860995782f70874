"""Quantised artefacts without a GPU: the quantiser's properties (brief_pytorch_amd/quantize.py, csrc/brief_quant.h), the bit packing, the
file format and its refusals, load_model on quantized.bin, the budget rule of Compress.quantize and the framework's refusals."""
import copy
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from brief_pytorch_amd import config, quantize
from brief_pytorch_amd.framework import NFGR, quantize_of
from brief_pytorch_amd.modelsave import load_model, save_model
from brief_pytorch_amd.networks import SIREN, SIREN_Pyramid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = (2, 3, 8, 11, 16)


def _tensors():
    """name -> float32 tensor: seeded tensors of 1, 7, 8, 9 and 4097 elements at several magnitudes, a constant one, one with offset >> spread"""
    rng = np.random.default_rng(7)
    out = {}
    for n in (1, 7, 8, 9, 4097):
        for mag in (1e-4, 0.3, 1e2):
            out["n%d_mag%g" % (n, mag)] = (rng.standard_normal(n) * mag).astype(np.float32)
    out["constant"] = np.full(33, 0.37, dtype=np.float32)
    out["offset"] = (1000.0 + rng.uniform(-1, 1, 513) * 0.01).astype(np.float32)       # offset 5 orders above the spread
    out["negative_offset"] = (-37.5 + rng.uniform(-1, 1, 100)).astype(np.float32)
    return out


TENSORS = _tensors()


@pytest.mark.parametrize("bits", BITS)
def test_error_bound_idempotence_and_code_range(bits):
    top = (1 << bits) - 1
    for name, w in TENSORS.items():
        lo, step = quantize.ranges(w, bits)
        hi = np.float32(w.max())
        assert lo.dtype == np.float32 and step.dtype == np.float32
        codes = quantize.quantise(w, lo, step, bits)
        assert codes.dtype == np.uint16 and codes.shape == w.shape
        assert int(codes.max()) <= top, name
        deq = quantize.dequantise(codes, lo, step)
        assert deq.dtype == np.float32
        # |w - deq| <= step / 2 + the four fp32 roundings (subtract, divide, multiply, add), each 2^-24 relative to a value below
        # max(|lo|, |hi|, hi - lo) in magnitude: 2^-21 of it covers them with a margin of two
        bound = 0.5 * float(step) + 2.0 ** -21 * max(abs(float(lo)), abs(float(hi)), float(hi) - float(lo))
        err = np.abs(w.astype(np.float64) - deq.astype(np.float64)).max()
        assert err <= bound, (name, err, bound)
        assert np.array_equal(quantize.quantise(deq, lo, step, bits), codes), name      # a loaded artefact re-saves to the same codes
        if name == "constant":
            assert step == 0 and not codes.any() and np.array_equal(deq, w)
        if w.size > 1 and step > 0:
            assert codes.min() == 0 and w[codes == 0].min() == lo
        assert np.array_equal(quantize.fake_quantise(w, bits), deq)


SRC = r'''
#include <math.h>
#include "brief_quant.h"
extern "C" {
float probe_step(float lo, float hi, int bits) { return brief_quant_step(lo, hi, bits); }
void probe(const float *w, long n, float lo, float step, int bits, float *code, float *deq)
{
    const float top = (float)((1 << bits) - 1);
    for (long i = 0; i < n; ++i) { code[i] = brief_quant_code(w[i], lo, step, top); deq[i] = brief_quant_deq(code[i], lo, step); }
}
}
'''


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("quant")
    src, so = str(d / "probe.cpp"), str(d / "probe.so")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "brief_pytorch_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.probe_step.restype = C.c_float
    L.probe_step.argtypes = [C.c_float, C.c_float, C.c_int]
    L.probe.argtypes = [C.c_void_p, C.c_long, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("bits", BITS)
def test_the_header_compiled_on_the_host_matches_numpy_bit_for_bit(hostlib, bits):
    for name, w in TENSORS.items():
        lo, step = quantize.ranges(w, bits)
        got_step = np.float32(hostlib.probe_step(float(lo), float(w.max()), bits))
        assert got_step.tobytes() == step.tobytes(), name
        code, deq = np.empty(w.size, np.float32), np.empty(w.size, np.float32)
        hostlib.probe(w.ctypes.data, w.size, float(lo), float(step), bits, code.ctypes.data, deq.ctypes.data)
        want = quantize.quantise(w, lo, step, bits)
        assert np.array_equal(code, want.astype(np.float32)), name
        assert deq.tobytes() == quantize.dequantise(want, lo, step).tobytes(), name


@pytest.mark.parametrize("bits", range(2, 17))
def test_bit_packing_round_trips(bits):
    rng = np.random.default_rng(bits)
    for n in (1, 7, 8, 9, 4097):
        codes = rng.integers(0, 1 << bits, n).astype(np.uint16)
        codes[0] = (1 << bits) - 1
        buf = quantize.pack_bits(codes, bits)
        assert len(buf) == (n * bits + 7) // 8 == quantize.code_bytes(n, bits)
        assert np.array_equal(quantize.unpack_bits(buf, n, bits), codes)
    # little-endian bit order: code i occupies stream bits [i bits, (i + 1) bits), least significant bit first
    codes = np.array([1, (1 << bits) - 1, 2], dtype=np.uint16)
    stream = int.from_bytes(quantize.pack_bits(codes, bits), "little")
    assert [(stream >> (i * bits)) & ((1 << bits) - 1) for i in range(3)] == [int(c) for c in codes]
    assert stream >> (3 * bits) == 0      # zero padding


def test_bit_packing_across_rounds(monkeypatch):
    monkeypatch.setattr(quantize, "_PACK_BLOCK", 16)
    rng = np.random.default_rng(0)
    for bits in (3, 11, 16):
        codes = rng.integers(0, 1 << bits, 53).astype(np.uint16)
        buf = quantize.pack_bits(codes, bits)
        assert len(buf) == quantize.code_bytes(53, bits)
        stream = int.from_bytes(buf, "little")
        assert [(stream >> (i * bits)) & ((1 << bits) - 1) for i in range(53)] == [int(c) for c in codes]
        assert np.array_equal(quantize.unpack_bits(buf, 53, bits), codes)


def _nets():
    torch.manual_seed(3)
    a = SIREN(coords_channel=2, data_channel=3, features=5, layers=3, w0=20)
    b = SIREN_Pyramid(coords_channel=3, data_channel=1, features=20, layers=4, w0=20, features_dis=3)
    fresh = (lambda: SIREN(coords_channel=2, data_channel=3, features=5, layers=3, w0=20),
             lambda: SIREN_Pyramid(coords_channel=3, data_channel=1, features=20, layers=4, w0=20, features_dis=3))
    return (a, fresh[0]), (b, fresh[1])


@pytest.mark.parametrize("bits", (2, 7, 12, 16))
def test_write_read_load_model(tmp_path, bits):
    for k, (net, fresh) in enumerate(_nets()):
        d = str(tmp_path / ("m%d" % k))
        save_model(net, d, quantize_bits=bits)
        assert os.listdir(d) == [quantize.FILE_NAME]
        path = os.path.join(d, quantize.FILE_NAME)
        assert os.path.getsize(path) == quantize.overhead_bytes(len(net.net)) + math.ceil(net.param_count * bits / 8)
        art = quantize.read(path)
        assert art["bits"] == bits and len(art["tensors"]) == 2 * len(net.net)
        other = fresh()
        assert load_model(other, d) is other
        for l in range(len(net.net)):
            for t, view in ((art["tensors"][2 * l], "weight"), (art["tensors"][2 * l + 1], "bias")):
                w = getattr(net.net[l][0], view).data.numpy()
                lo, step = quantize.ranges(w, bits)
                assert t["layer"] == l and t["kind"] == (quantize.KIND_WEIGHT if view == "weight" else quantize.KIND_BIAS)
                assert t["lo"].tobytes() == lo.tobytes() and t["step"].tobytes() == step.tobytes()
                assert np.array_equal(t["codes"], quantize.quantise(w, lo, step, bits))
                got = getattr(other.net[l][0], view).data.numpy()
                assert got.tobytes() == quantize.fake_quantise(w, bits).tobytes(), (l, view)
        # saving the loaded net again gives the same file
        d2 = str(tmp_path / ("again%d" % k))
        save_model(other, d2, quantize_bits=bits)
        assert open(os.path.join(d2, quantize.FILE_NAME), "rb").read() == open(path, "rb").read()
    # without quantize_bits nothing changes: the float32 weight files
    net = _nets()[0][0]
    save_model(net, str(tmp_path / "plain"))
    assert sorted(os.listdir(str(tmp_path / "plain"))) == sorted(["weight-0-5-2", "bias-0-5", "weight-1-5-5", "bias-1-5", "weight-2-3-5", "bias-2-3"])


def test_reader_and_writer_refusals(tmp_path):
    net, fresh = _nets()[0]
    path = str(tmp_path / quantize.FILE_NAME)
    size = quantize.write(path, net, 8)
    good = open(path, "rb").read()
    assert size == len(good)

    def put(b):
        with open(path, "wb") as f:
            f.write(b)
    put(b"XXXX" + good[4:])
    with pytest.raises(quantize.BadMagic, match="bad magic"):
        quantize.read(path)
    put(good[:4] + (99).to_bytes(4, "little") + good[8:])
    with pytest.raises(quantize.UnknownVersion, match="unknown format version 99"):
        quantize.read(path)
    for cut in (3, 15, 16 + 24 * 3 + 5, len(good) - 1):      # inside the header, the table, and one byte short of the codes
        put(good[:cut])
        with pytest.raises(quantize.TruncatedFile, match="truncated"):
            quantize.read(path)
    put(good)
    other = SIREN(coords_channel=2, data_channel=3, features=6, layers=3, w0=20)
    with pytest.raises(quantize.TensorTableMismatch, match="tensor table mismatch"):
        quantize.load_into(other, path)
    with pytest.raises(quantize.TensorTableMismatch):
        quantize.load_into(SIREN(coords_channel=2, data_channel=3, features=5, layers=4, w0=20), path)
    assert issubclass(quantize.TensorTableMismatch, quantize.QuantizedFileError) and issubclass(quantize.QuantizedFileError, ValueError)
    # the writer: a non-finite tensor, bits outside 2..16
    bad = fresh()
    bad.net[1][0].bias.data = torch.tensor([0.0, 1.0, float("nan"), 0.0, 0.0])
    with pytest.raises(quantize.NonFiniteTensor, match="bias of layer 1"):
        quantize.write(path, bad, 8)
    bad.net[1][0].bias.data = torch.zeros(5)
    bad.net[0][0].weight.data = torch.full((5, 2), float("inf"))
    with pytest.raises(quantize.NonFiniteTensor, match="weight of layer 0"):
        quantize.write(path, bad, 8)
    for bits in (1, 17, 0, -3, 8.0, True):
        with pytest.raises(ValueError, match="2..16"):
            quantize.write(path, net, bits)
        with pytest.raises(ValueError, match="2..16"):
            save_model(net, str(tmp_path / "m"), quantize_bits=bits)


# ---- framework: the key, the budget rule, the refusals
PHIS = {
    "SIREN": {"name": "SIREN", "layers": 5, "w0": 20, "coords_channel": 3, "data_channel": 1, "output_act": False, "res": False},
    "SIREN_Pyramid": {"name": "SIREN_Pyramid", "layers": 5, "w0": 20, "coords_channel": 3, "data_channel": 1, "output_act": False, "res": False,
                      "features_dis": 10, "ratio": 1},
    "SIRENFT": {"name": "SIRENFT", "layers": 5, "w0": 20, "coords_channel": 3, "data_channel": 1, "output_act": False, "res": False, "ratio": 2},
    "SIRENPS": {"name": "SIRENPS", "layers": 5, "w0": 20, "coords_channel": 3, "data_channel": 1, "output_act": False, "res": False, "ratio": 1.5},
}


def _opt(phi, quant="absent", **compress):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml")).CompressFramework
    opt.Module.phi = config.to_opt(copy.deepcopy(phi))
    if quant != "absent":
        opt.Compress.quantize = config.to_opt(quant)
    for k, v in compress.items():
        opt.Compress[k] = v
    return opt


def test_budget_rule():
    checked = 0
    for name, phi in PHIS.items():
        for budget in (3000.0, 6687.5, 17924.0, 33000.0, 65536.0, 262144.0, 794628.0, 3.3e6):
            try:
                pf, pa, pt = NFGR.estimate_module_size(budget, _opt(phi))
            except (ValueError, NotImplementedError):
                continue                                        # the parent's rule builds no net at this budget
            parent_ok = abs(pt - budget) <= 0.05 * budget
            for bits in (2, 5, 8, 12, 16):
                opt = _opt(phi, {"bits": bits, "finetune_steps": 0})
                feats, actual, theory = NFGR.estimate_module_size(budget, opt)
                over = quantize.overhead_bytes(opt.Module.phi.layers)
                assert theory == math.ceil(actual * bits / 8) + over, (name, budget, bits)
                if parent_ok:
                    assert theory <= 1.05 * budget, (name, budget, bits, theory)
                    checked += 1
    assert checked >= 60
    # at the same budget a 12-bit net has about 2.7 times the parameters
    p32 = NFGR.estimate_module_size(794628.0, _opt(PHIS["SIREN"]))[1]
    p12 = NFGR.estimate_module_size(794628.0, _opt(PHIS["SIREN"], {"bits": 12}))[1]
    assert 2.5 < p12 / p32 < 2.8


def test_key_absent_or_none_changes_nothing():
    for name, phi in PHIS.items():
        for half in (False, True):
            for budget in (6687.5, 33000.0, 794628.0):
                base = _opt(phi, half=half)
                want = NFGR.estimate_module_size(budget, base)
                assert want[2] == want[1] * (2.0 if half else 4.0)
                for off in (None, "none", "None"):
                    opt = _opt(phi, off, half=half)
                    assert quantize_of(opt) is None
                    assert NFGR.estimate_module_size(budget, opt) == want and opt.Module.phi.name == base.Module.phi.name
    assert quantize_of(_opt(PHIS["SIREN"])) is None
    assert quantize_of(_opt(PHIS["SIREN"], {"bits": 12})) == (12, 0)
    assert quantize_of(_opt(PHIS["SIREN"], {"bits": 2, "finetune_steps": 20000})) == (2, 20000)
    y = config.load(os.path.join(ROOT, "opt", "SingleTask", "quantize.yaml"))
    assert quantize_of(y.CompressFramework) == (12, 2000)
    d = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    del y.CompressFramework.Compress["quantize"]
    assert config.to_plain(y) == config.to_plain(d)            # default.yaml plus the key


def test_framework_refusals_need_no_gpu():
    """raised by NFGR's constructor in front of its GPU requirement (and by quantize_of itself)"""
    def both(opt, exc, match):
        with pytest.raises(exc, match=match):
            quantize_of(opt)
        with pytest.raises(exc, match=match):
            NFGR(opt)
    q = {"bits": 8, "finetune_steps": 0}
    for name, extra in (("FFN", {"embsize": 256, "skip": False}), ("NeRF", {"frequencies": 10, "skip": True}), ("MFNFourier", {}), ("MFNGabor", {})):
        phi = {"name": name, "layers": 5, "coords_channel": 3, "data_channel": 1, **extra}
        both(_opt(phi, q), NotImplementedError, "Compress.quantize supports SIREN, SIREN_Pyramid, SIRENFT, SIRENPS.*%s" % name)
    both(_opt(PHIS["SIREN"], q, half=True), ValueError, "Compress.quantize needs an fp32 fit")
    both(_opt(PHIS["SIREN"], q, precision="bf16"), ValueError, "Compress.quantize needs an fp32 fit")
    both(_opt(PHIS["SIRENFT"], q, precision="bf16x3"), ValueError, "Compress.quantize needs an fp32 fit")
    for bits in (1, 17, 0, 8.5, "8"):
        both(_opt(PHIS["SIREN"], {"bits": bits}), ValueError, "bits must be an integer in 2..16")
    both(_opt(PHIS["SIREN"], {"bits": 8, "finetune_steps": -1}), ValueError, "finetune_steps must be an integer >= 0")
    both(_opt(PHIS["SIREN"], {"bits": 8, "finetune_steps": 20001}), ValueError, "finetune_steps=20001 exceeds Compress.max_steps=20000")
    both(_opt(PHIS["SIREN"], {"finetune_steps": 5}), ValueError, "Compress.quantize must be")
    both(_opt(PHIS["SIREN"], 8), ValueError, "Compress.quantize must be")
