"""The yardstick of the spatial-gradient tests: a plain-torch restatement of SIREN built from a module's canonical `params` /
`_shapes`, at a given dtype, and its Jacobian with respect to the coordinates by torch.autograd.grad, one output channel at a time.
No GPU and no library call."""
import numpy as np
import torch

VALUE_TOL, JAC_TOL = 2e-5, 1e-4      # the bands of the sine nets on the project's phase rule (tests/test_gpu_taper.py)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def layers_of(m, dtype, params=None):
    """[(W [out, in], b [out])] of the module's Linear layers in order, as `dtype` CPU tensors (params: another canonical buffer)"""
    p = (m.params if params is None else params).detach().cpu().to(dtype)
    out, off = [], 0
    for (o, i) in m._shapes:
        out.append((p[off:off + o * i].view(o, i), p[off + o * i:off + o * i + o]))
        off += o * i + o
    return out


def siren(m, x, dtype, params=None):
    """SIREN.forward (first sine w0 = m.w0, hidden sines and the output activation 30) on coordinates x [n, cin]"""
    lay = layers_of(m, dtype, params)
    h = x.to(dtype)
    for l, (W, b) in enumerate(lay[:-1]):
        h = torch.sin((m.w0 if l == 0 else 30.0) * (h @ W.t() + b))
    W, b = lay[-1]
    y = h @ W.t() + b
    return torch.sin(30.0 * y) if m.output_act else y


def value_and_jacobian(m, x, dtype, params=None):
    """(value [n, cout], jac [n, cout, cin]) as numpy arrays of `dtype`: autograd of the restatement, per output channel"""
    x = torch.as_tensor(np.asarray(x)).detach().cpu().to(dtype).reshape(-1, m.coords_channel).clone().requires_grad_(True)
    y = siren(m, x, dtype, params)
    jac = torch.stack([torch.autograd.grad(y[:, c].sum(), x, retain_graph=True)[0] for c in range(y.shape[1])], dim=1)
    return y.detach().numpy(), jac.detach().numpy()


def check_bands(m, x, value, jac, what="", params=None):
    """the issue's bands: value relerr < 2e-5 against float64; Jacobian relerr < max(1e-4, 3 x relerr(torch fp32, float64)); both
    Jacobian distances are printed"""
    v64, j64 = value_and_jacobian(m, x, torch.float64, params)
    _, j32 = value_and_jacobian(m, x, torch.float32, params)
    own, got = relerr(j32, j64), relerr(jac, j64)
    band = max(JAC_TOL, 3 * own)
    print("%s: jacobian relerr %.3e (band %.3e; torch fp32 against float64 %.3e)" % (what, got, band, own), end="")
    if value is not None:
        ev = relerr(value, v64)
        print(", value relerr %.3e" % ev)
        assert ev < VALUE_TOL, (what, ev)
    else:
        print()
    assert got < band, (what, got, band, own)
    return v64, j64
