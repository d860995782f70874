"""Host side of the Hessian decode (brief_pytorch_amd/hessian.py, decompress.py --hessian): the voxel scaling, the derived maps
(laplacian, eigenvalues, vesselness), the refusals, the C-ABI's declarations, the yardstick of the GPU tests itself (tests/_hessian.py)
and the cap on how far its bands may widen.  Nothing here needs a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

from brief_pytorch_amd import _lib, hessian
from brief_pytorch_amd.networks import ALLPHI, SIREN

from . import _bands
from ._hessian import CASES, HESS_TOL, PAIRS, reference, value_jacobian_hessian
from ._jacobian import value_and_jacobian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("brief_siren_hess_forward", "brief_siren_hess_forward_box")


def test_voxel_scale_is_its_formula_in_float64():
    for dims, lo, hi, rng, vmin, vmax in (((20, 24, 28), -1.0, 1.0, (0.0, 100.0), 3.0, 60000.0),
                                          ((7, 1, 9), -1.0, 1.0, (-0.5, 0.5), 0.0, 255.0),          # an axis of length 1
                                          ((13, 17), 0.0, 1.0, (0.0, 1.0), 100.0, 65535.0),        # a 0,1 coords mode, 2-D
                                          ((2, 3, 4), -3.5, 2.25, (10.0, 20.0), 17.0, 17.0)):       # a constant volume
        got = hessian.voxel_scale(dims, lo, hi, rng, vmin, vmax)
        nd = len(dims)
        assert got.dtype == np.float64 and got.shape == (nd * (nd + 1) // 2,)
        step = [0.0 if n == 1 else (np.float64(hi) - np.float64(lo)) / np.float64(n - 1) for n in dims]
        grey = (np.float64(vmax) - np.float64(vmin)) / (np.float64(rng[1]) - np.float64(rng[0]))
        for k, (a, b) in enumerate(PAIRS[nd]):
            assert got[k] == step[a] * step[b] * grey, (dims, a, b)
    # what it is: the second difference of the unclipped de-normalisation of a quadratic net output y = k x0^2 along one axis, and the
    # mixed difference of y = k x0 x1 across two
    dims, lo, hi, (a, b), vmin, vmax, k = (11, 5, 3), -1.0, 1.0, (0.0, 100.0), 10.0, 4000.0, 7.0
    xs = np.linspace(lo, hi, dims[0])
    grey = (k * xs * xs - a) / (b - a) * (vmax - vmin) + vmin
    s = hessian.voxel_scale(dims, lo, hi, (a, b), vmin, vmax)
    assert np.allclose(np.diff(grey, 2), 2 * k * s[0], rtol=1e-9)
    ys = np.linspace(lo, hi, dims[1])
    grey = (k * xs[:, None] * ys[None, :] - a) / (b - a) * (vmax - vmin) + vmin
    assert np.allclose(np.diff(np.diff(grey, axis=0), axis=1), k * s[1], rtol=1e-9)


def _random_symmetric(n, count, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((count, n, n)) * np.exp(rng.uniform(-3, 3, (count, 1, 1)))
    return (a + a.transpose(0, 2, 1)) / 2


def _pack(mats):
    n = mats.shape[-1]
    return torch.from_numpy(np.stack([mats[:, i, j] for i, j in PAIRS[n]], axis=-1).astype(np.float32))


def _degenerate(n):
    eye = np.eye(n)
    out = [np.zeros((n, n)), eye, -3.0 * eye, np.diag(np.arange(1.0, n + 1)), np.diag([2.0] * (n - 1) + [-5.0]), np.diag([0.0] * (n - 1) + [4.0])]
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((n, n)))
    for d in ([1.0] * (n - 1) + [7.0], [-2.0] + [6.0] * (n - 1), [0.0] * (n - 1) + [1.0], [1e-3] * n):      # repeated roots, rotated
        out.append(q @ np.diag(d) @ q.T)
    return np.stack(out)


def test_eigenvalues_against_eigvalsh():
    """the tolerance is that of the float32 result type: 1e-5 of the largest |eigenvalue| of the matrix"""
    for n in (3, 2):
        mats = np.concatenate([_random_symmetric(n, 1000, seed=n), _degenerate(n)])
        h = _pack(mats)
        got = hessian.eigenvalues(h)
        assert got.dtype == torch.float32 and got.shape == (len(mats), n)
        got = got.numpy().astype(np.float64)
        assert np.all(np.diff(np.abs(got), axis=-1) >= 0), "not sorted by increasing absolute value"
        want = np.linalg.eigvalsh(hessian.full(h).numpy().astype(np.float64))      # of the float32 matrices the function was given
        scale = np.abs(want).max(axis=-1, keepdims=True)
        err = np.abs(np.sort(got, axis=-1) - want)
        assert np.all(err <= 1e-5 * scale), float((err / np.maximum(scale, 1e-300)).max())
        # the trace is the sum of the eigenvalues
        lap = hessian.laplacian(h).numpy().astype(np.float64)
        assert np.all(np.abs(lap - got.sum(-1)) <= 1e-5 * np.maximum(scale[:, 0], 1e-300) + 0.0)
    assert not hessian.eigenvalues(torch.zeros(4, 6)).any() and not hessian.eigenvalues(torch.zeros(4, 3)).any()


def test_full_expands_the_upper_triangle():
    h = torch.arange(12, dtype=torch.float32).reshape(2, 6)
    f = hessian.full(h)
    assert f.shape == (2, 3, 3) and torch.equal(f, f.transpose(-1, -2))
    assert f[1].tolist() == [[6, 7, 8], [7, 9, 10], [8, 10, 11]]
    assert hessian.full(torch.tensor([[1.0, 2.0, 3.0]]))[0].tolist() == [[1, 2], [2, 3]]


def test_vesselness_prefers_tubes_and_respects_the_sign():
    def diag3(a, b, c):
        return [a, 0.0, 0.0, b, 0.0, c]
    # bright structures on a dark ground have negative curvature across them
    tube, sheet, blob, flat = diag3(0.0, -10.0, -10.0), diag3(0.0, 0.0, -10.0), diag3(-10.0, -10.0, -10.0), diag3(0.0, 0.0, 0.0)
    h = torch.tensor([tube, sheet, blob, flat, diag3(0.0, 10.0, 10.0), diag3(0.0, -10.0, 10.0)])
    v = hessian.vesselness(h, c=5.0)
    assert v.dtype == torch.float32 and v.shape == (6,)
    assert v[0] > v[1] and v[0] > v[2] and v[0] > 0.5
    assert v[3] == 0 and v[4] == 0 and v[5] == 0, "a dark tube and a saddle fail the sign test of bright=True"
    d = hessian.vesselness(h, c=5.0, bright=False)
    assert d[4] == v[0] and d[0] == 0
    # a rotated tube scores what the axis-aligned one does
    q, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((3, 3)))
    rot = _pack((q @ np.diag([0.0, -10.0, -10.0]) @ q.T)[None])
    assert abs(float(hessian.vesselness(rot, c=5.0)[0]) - float(v[0])) < 1e-5
    # c=None: half the largest Frobenius norm of the map (here sqrt(300) / 2)
    assert torch.allclose(hessian.vesselness(h), hessian.vesselness(h, c=0.5 * 300.0 ** 0.5))
    assert not hessian.vesselness(torch.zeros(3, 6)).any()
    # two axes: a line (one strong negative curvature) against a blob
    h2 = torch.tensor([[0.0, 0.0, -10.0], [-10.0, 0.0, -10.0], [0.0, 0.0, 10.0]])
    v2 = hessian.vesselness(h2, c=5.0)
    assert v2[0] > v2[1] > 0 and v2[2] == 0 and hessian.vesselness(h2, c=5.0, bright=False)[2] == v2[0]
    # derive() in chunks is derive() at once
    big = _pack(_random_symmetric(3, 50, seed=9)).reshape(5, 10, 1, 6)
    for mode in ("eigenvalues", "vesselness", "laplacian"):
        assert torch.equal(hessian.derive(big, mode, chunk=7), hessian.derive(big, mode))
    assert hessian.derive(big, "eigenvalues").shape == (5, 10, 1, 3) and hessian.derive(big, "vesselness").shape == (5, 10, 1)
    assert hessian.derive(big, "components") is big


def test_supported_refuses_by_name():
    families = [k for k in ALLPHI if k != "SIREN"]
    assert {"FFN", "NeRF", "MFNFourier", "MFNGabor", "SIREN_Pyramid", "SIRENFT", "SIRENPS"} <= set(families)
    for name in families:
        assert not hessian.supported(name, "fp32", 64)
        assert "spatial Hessians exist for fp32 SIREN up to 1024 features (this net is %s" % name in hessian.refusal(name, "fp32", 64)
    for prec in ("bf16", "bf16x3"):
        assert not hessian.supported("SIREN", prec, 64)
        assert prec in hessian.refusal("SIREN", prec, 64)
    assert not hessian.supported("SIREN", "fp32", 1025) and "1025" in hessian.refusal("SIREN", "fp32", 1025)
    assert not hessian.supported("SIREN", "fp32", 0)
    assert hessian.supported("SIREN", "fp32", 1) and hessian.supported("SIREN", "fp32", 1024)
    assert hessian.refusal("SIREN", "fp32", 527) is None
    for bad in ("magnitude", "", None):
        try:
            hessian.check_mode(bad)
        except ValueError as e:
            assert "laplacian" in str(e)
        else:
            raise AssertionError(bad)


def test_entries_are_exported_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brief_hip.h")).read(), flags=re.S)
    assert "#define BRIEF_VERSION 130" in text
    for name in ENTRIES:
        assert name in _lib.EXPORTS
    protos = {name: [" ".join(p.split()) for p in re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(",")] for name in ENTRIES}
    assert protos["brief_siren_hess_forward"] == [
        "const brief_siren_desc *d", "const float *packed", "const brief_grid_desc *grid", "const brief_batch_desc *batch", "float *value", "float *jac",
        "float *hess", "void *stream"]
    assert protos["brief_siren_hess_forward_box"] == [
        "const brief_siren_desc *d", "const float *packed", "const brief_grid_box *box", "int64_t offset", "int64_t n", "float *value", "float *jac",
        "float *hess", "void *stream"]


def _cli(cdir, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", os.path.join(ROOT, "opt", "SingleTask", "default.yaml"),
                           "-c", str(cdir), "--region", ":,:,:", *extra], capture_output=True, text=True, timeout=120)


def test_cli_refuses_by_name_before_the_gpu_path(tmp_path):
    """the artefact directory is empty and there may be no GPU: reaching the decode would fail differently"""
    out = str(tmp_path / "h.npy")
    for flag in (("--mip",), ("--gradient", "components"), ("--view", "0,0,1"), ("--view", "0,0,1", "--view-surface", "100")):
        r = _cli(tmp_path, "--hessian", "components", *flag, "-o", out)
        assert r.returncode != 0 and "--hessian with %s" % flag[-2 if len(flag) > 1 else 0] in r.stderr, r.stderr[-500:]
    r = _cli(tmp_path, "--hessian", "laplacian", "-o", str(tmp_path / "h.tif"))
    assert r.returncode != 0 and ".npy" in r.stderr and ".tif" in r.stderr
    r = _cli(tmp_path, "--hessian", "magnitude", "-o", out)
    assert r.returncode != 0 and "magnitude" in r.stderr and "vesselness" in r.stderr
    os.makedirs(str(tmp_path / "div" / "sideinfos"))
    r = _cli(tmp_path / "div", "--hessian", "eigenvalues", "--shape", "8,8,8", "-o", out)
    assert r.returncode != 0 and "--shape" in r.stderr and "DivideTask" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["div"]


def test_autograd_hessian_agrees_with_central_differences_of_the_jacobian():
    """the yardstick itself: at 4x32 the float64 double-autograd Hessian of the restatement equals float64 central differences (h = 1e-6)
    of the float64 autograd Jacobian to 1e-6 relative, in the documented component order"""
    for cin, cout, act in ((3, 1, False), (2, 3, True)):
        torch.manual_seed(5)
        m = SIREN(coords_channel=cin, data_channel=cout, features=32, layers=5, w0=30, output_act=act)
        x = torch.rand(64, cin, dtype=torch.float64) * 2 - 1
        v, jac, hess = value_jacobian_hessian(m, x, torch.float64)
        v1, j1 = value_and_jacobian(m, x, torch.float64)
        assert hess.shape == (64, cout, len(PAIRS[cin])) and hess.dtype == np.float64
        assert np.array_equal(v, v1) and np.allclose(jac, j1, rtol=1e-13, atol=0)
        h = 1e-6
        for k, (a, b) in enumerate(PAIRS[cin]):
            e = torch.zeros(cin, dtype=torch.float64)
            e[b] = h
            fd = (value_and_jacobian(m, x + e, torch.float64)[1][:, :, a] - value_and_jacobian(m, x - e, torch.float64)[1][:, :, a]) / (2 * h)
            assert np.max(np.abs(hess[:, :, k] - fd)) / np.max(np.abs(hess)) < 1e-6, (cin, a, b)


def test_band_cap_of_the_parity_cases():
    """tests/_bands.py's cap on the Hessian bands of tests/test_gpu_hessian.py: at most 0.15 of the comparisons may need 3 x own > 1e-4, and
    none a band above 1e-3.  The fourteen initialised cases are computed here and must widen nothing; the fitted case needs a fit on the
    GPU and asserts its own band below 1e-3 where it is measured (tests/test_gpu_hessian.py): at most 1 widened comparison of 15."""
    owns = []
    for case in CASES:
        own = reference(case)[6]
        print("case %s: torch fp32 against float64 hessian %.3e" % (case, own))
        owns.append(own)
    bands = [max(HESS_TOL, 3 * o) for o in owns]
    widened = sum(b > HESS_TOL for b in bands)
    assert max(bands) <= _bands.MAX_BAND["grad"], max(bands)
    assert widened == 0 and widened + 1 <= _bands.MAX_WIDENED_FRACTION["grad"] * (len(bands) + 1), (widened, owns)
