"""Host side of the spatial-gradient decode (brief_pytorch_amd/gradient.py, decompress.py --gradient): the voxel scaling, the refusals,
the C-ABI's declarations, and the yardstick of the GPU tests itself (tests/_jacobian.py).  Nothing here needs a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, gradient
from brief_pytorch_amd.networks import ALLPHI, SIREN

from ._jacobian import relerr, siren, value_and_jacobian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("brief_siren_jac_packed_count", "brief_siren_jac_repack", "brief_siren_jac_forward", "brief_siren_jac_forward_box")


def test_voxel_scale_is_its_formula_in_float64():
    for dims, lo, hi, rng, vmin, vmax in (((20, 24, 28), -1.0, 1.0, (0.0, 100.0), 3.0, 60000.0),
                                          ((7, 1, 9), -1.0, 1.0, (-0.5, 0.5), 0.0, 255.0),          # an axis of length 1
                                          ((13, 17), 0.0, 1.0, (0.0, 1.0), 100.0, 65535.0),        # a 0,1 coords mode, 2-D
                                          ((2, 3, 4), -3.5, 2.25, (10.0, 20.0), 17.0, 17.0)):       # a constant volume
        got = gradient.voxel_scale(dims, lo, hi, rng, vmin, vmax)
        assert got.dtype == np.float64 and got.shape == (len(dims),)
        for a, n in enumerate(dims):
            want = 0.0 if n == 1 else ((np.float64(hi) - np.float64(lo)) / np.float64(n - 1)) * (
                (np.float64(vmax) - np.float64(vmin)) / (np.float64(rng[1]) - np.float64(rng[0])))      # (a voxel step) x (grey levels per unit of output)
            assert got[a] == want, (dims, a)
    # what it is: the finite difference of the unclipped de-normalisation along one voxel step of a linear net output y = k x
    dims, lo, hi, (a, b), vmin, vmax, k = (11, 5, 3), -1.0, 1.0, (0.0, 100.0), 10.0, 4000.0, 7.0
    xs = np.linspace(lo, hi, dims[0])
    grey = (k * xs - a) / (b - a) * (vmax - vmin) + vmin
    assert np.allclose(np.diff(grey), k * gradient.voxel_scale(dims, lo, hi, (a, b), vmin, vmax)[0], rtol=1e-12)


def test_supported_refuses_by_name():
    families = [k for k in ALLPHI if k != "SIREN"]
    assert {"FFN", "NeRF", "MFNFourier", "MFNGabor", "SIREN_Pyramid", "SIRENFT", "SIRENPS"} <= set(families)
    for name in families:
        assert not gradient.supported(name, "fp32", 64)
        assert "spatial gradients exist for fp32 SIREN up to 1024 features (this net is %s" % name in gradient.refusal(name, "fp32", 64)
    for prec in ("bf16", "bf16x3"):
        assert not gradient.supported("SIREN", prec, 64)
        assert prec in gradient.refusal("SIREN", prec, 64)
    assert not gradient.supported("SIREN", "fp32", 1025) and "1025" in gradient.refusal("SIREN", "fp32", 1025)
    assert not gradient.supported("SIREN", "fp32", 0)
    assert gradient.supported("SIREN", "fp32", 1) and gradient.supported("SIREN", "fp32", 1024)
    assert gradient.refusal("SIREN", "fp32", 527) is None


def test_entries_are_exported_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brief_hip.h")).read(), flags=re.S)
    assert "#define BRIEF_VERSION 130" in text
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(\s*const brief_siren_desc \*d" % name, text), "%s is not declared in include/brief_hip.h" % name
    proto = re.search(r"int\s+brief_siren_jac_forward_box\s*\((.*?)\)\s*;", text, flags=re.S)
    assert [" ".join(p.split()) for p in proto.group(1).split(",")] == [
        "const brief_siren_desc *d", "const float *packed", "const brief_grid_box *box", "int64_t offset", "int64_t n", "float *value", "float *jac",
        "void *stream"]


def _cli(tmp_path, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"),
                           "-c", str(tmp_path), "--region", ":,:,:", *extra], capture_output=True, text=True, timeout=120)


def test_cli_refuses_by_name_before_the_gpu_path(tmp_path):
    """the artefact directory is empty and there may be no GPU: reaching the decode would fail differently"""
    r = _cli(tmp_path, "--gradient", "components", "--mip", "-o", str(tmp_path / "g.npy"))
    assert r.returncode != 0 and "--gradient" in r.stderr and "--mip" in r.stderr
    r = _cli(tmp_path, "--gradient", "magnitude", "-o", str(tmp_path / "g.tif"))
    assert r.returncode != 0 and ".npy" in r.stderr and ".tif" in r.stderr
    r = _cli(tmp_path, "--gradient", "laplacian", "-o", str(tmp_path / "g.npy"))
    assert r.returncode != 0 and "laplacian" in r.stderr
    os.makedirs(str(tmp_path / "div" / "sideinfos"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"),
                        "-c", str(tmp_path / "div"), "--region", ":,:,:", "--gradient", "components", "--shape", "8,8,8", "-o", str(tmp_path / "g.npy")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--shape" in r.stderr and "DivideTask" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["div"]


def test_autograd_jacobian_agrees_with_central_differences():
    """the yardstick itself: at 4x32 the float64 autograd Jacobian of the restatement equals float64 central differences (h = 1e-6)
    to 1e-6 relative"""
    for cin, cout, act in ((3, 1, False), (2, 3, True)):
        torch.manual_seed(5)
        m = SIREN(coords_channel=cin, data_channel=cout, features=32, layers=5, w0=30, output_act=act)
        x = torch.rand(64, cin, dtype=torch.float64) * 2 - 1
        _, jac = value_and_jacobian(m, x, torch.float64)
        assert jac.shape == (64, cout, cin) and jac.dtype == np.float64
        h = 1e-6
        fd = np.empty_like(jac)
        for a in range(cin):
            e = torch.zeros(cin, dtype=torch.float64)
            e[a] = h
            fd[:, :, a] = ((siren(m, x + e, torch.float64) - siren(m, x - e, torch.float64)) / (2 * h)).detach().numpy()
        assert relerr(jac, fd) < 1e-6, relerr(jac, fd)
