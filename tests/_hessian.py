"""The yardstick of the Hessian tests: tests/_jacobian.py's plain-torch restatement of SIREN and its Hessian with respect to the
coordinates by torch.autograd.grad applied twice, one output channel and one axis at a time.  No GPU and no library call."""
import numpy as np
import torch

from ._jacobian import JAC_TOL, VALUE_TOL, relerr, siren

HESS_TOL = 1e-4                     # the project's Jacobian floor for sine nets
PAIRS = {2: ((0, 0), (0, 1), (1, 1)), 3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}

# (cin, cout, layers, features, n, output_act): the fourteen initialised parity cases
CASES = [(3, 1, 5, 256, 200, False), (3, 1, 5, 22, 501, False), (3, 1, 5, 1, 9, False), (3, 1, 5, 32, 8, False), (2, 3, 3, 33, 7, False),
         (2, 1, 3, 65, 255, False), (3, 4, 9, 300, 61, False), (3, 1, 2, 33, 203, False), (3, 2, 5, 1024, 13, False), (3, 1, 4, 527, 40, False),
         (2, 3, 3, 33, 7, True), (3, 1, 5, 256, 200, True), (3, 1, 5, 22, 1, False), (3, 2, 5, 1024, 1, False)]


def case_id(c):
    return "%dto%d_%dx%d_n%d%s" % (c[0], c[1], c[2], c[3], c[4], "_act" if c[5] else "")


def case_net(case, seed=0):
    from brief_pytorch_amd.networks import SIREN
    cin, cout, layers, features, _, act = case
    torch.manual_seed(seed)
    return SIREN(coords_channel=cin, data_channel=cout, features=features, layers=layers, w0=30, output_act=act)


def case_coords(n, cin, seed=1):
    return torch.rand(n, cin, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def value_jacobian_hessian(m, x, dtype, params=None):
    """(value [n, cout], jac [n, cout, cin], hess [n, cout, nh]) as numpy arrays of `dtype`; hess holds the upper triangle row by row
    ((00, 01, 02, 11, 12, 22) / (00, 01, 11)): the derivative along axis b >= a of the Jacobian's column a"""
    cin = m.coords_channel
    x = torch.as_tensor(np.asarray(x)).detach().cpu().to(dtype).reshape(-1, cin).clone().requires_grad_(True)
    y = siren(m, x, dtype, params)
    jac, hess = [], []
    for c in range(y.shape[1]):
        g = torch.autograd.grad(y[:, c].sum(), x, create_graph=True)[0]                     # [n, cin]
        rows = [torch.autograd.grad(g[:, a].sum(), x, retain_graph=True)[0] for a in range(cin)]      # rows[a][:, b] = d2 y_c / dx_a dx_b
        jac.append(g.detach())
        hess.append(torch.stack([rows[a][:, b] for a, b in PAIRS[cin]], dim=1))
    return y.detach().numpy(), torch.stack(jac, dim=1).numpy(), torch.stack(hess, dim=1).detach().numpy()


_REFS = {}


def reference(case):
    """(m, x, v64, j64, h64, own_jac, own_hess) of an initialised parity case, computed once per session and never changed: `own` is the
    distance between the torch fp32 and the torch float64 result of the same case"""
    if case not in _REFS:
        m = case_net(case)
        x = case_coords(case[4], case[0])
        v64, j64, h64 = value_jacobian_hessian(m, x, torch.float64)
        _, j32, h32 = value_jacobian_hessian(m, x, torch.float32)
        for a in (v64, j64, h64):
            a.setflags(write=False)
        _REFS[case] = (m, x, v64, j64, h64, relerr(j32, j64), relerr(h32, h64))
    return _REFS[case]


def check_bands(what, value, jac, hess, v64, j64, h64, own_j, own_h):
    """value relerr < 2e-5 and Jacobian relerr < max(1e-4, 3 x own) (tests/_jacobian.py's bands), Hessian relerr < max(1e-4, 3 x own); the
    distances are printed before anything is asserted"""
    got_h, band_h = relerr(hess, h64), max(HESS_TOL, 3 * own_h)
    print("%s: hessian relerr %.3e (band %.3e; torch fp32 against float64 %.3e)" % (what, got_h, band_h, own_h), end="")
    got_j = band_j = ev = None
    if jac is not None:
        got_j, band_j = relerr(jac, j64), max(JAC_TOL, 3 * own_j)
        print(", jacobian relerr %.3e (band %.3e; own %.3e)" % (got_j, band_j, own_j), end="")
    if value is not None:
        ev = relerr(value, v64)
        print(", value relerr %.3e" % ev, end="")
    print()
    if value is not None:
        assert ev < VALUE_TOL, (what, ev)
    if jac is not None:
        assert got_j < band_j, (what, got_j, band_j, own_j)
    assert got_h < band_h, (what, got_h, band_h, own_h)
    return got_h
