"""Hessian decode on the GPU (csrc/brief_hess.inc) through networks.SIREN and the C-ABI: value, Jacobian and Hessian against the float64
restatement of tests/_hessian.py (value 2e-5; Jacobian and Hessian max(1e-4, 3 x torch's own fp32 distance), every distance printed),
and the contracts of decode_box: a box is the slice of the whole, and neither the chunking, a repeat nor a sample's slot in its tile
changes a bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.modelsave import load_model, save_model
from brief_pytorch_amd.networks import FFN, SIREN, SIREN_Pyramid
from brief_pytorch_amd.synthetic import make_volume

from . import _bands
from ._hessian import CASES, HESS_TOL, case_coords, case_id, check_bands, reference, value_jacobian_hessian
from ._jacobian import JAC_TOL, VALUE_TOL, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _net(cin, cout, layers, features, act=False, seed=0):
    torch.manual_seed(seed)
    return SIREN(coords_channel=cin, data_channel=cout, features=features, layers=layers, w0=30, output_act=act)


def _full_check(m, x, what, ref=None):
    """the three outputs of m.spatial_hessian at x against the float64 restatement of `ref` (default: of m itself), inside the bands;
    returns them and torch's own fp32 distance of the Hessian"""
    ref = m if ref is None else ref
    v64, j64, h64 = value_jacobian_hessian(ref, x, torch.float64)
    _, j32, h32 = value_jacobian_hessian(ref, x, torch.float32)
    value, jac, hess = m.spatial_hessian(x.to(DEV))
    check_bands(what, value.cpu().numpy(), jac.cpu().numpy(), hess.cpu().numpy(), v64, j64, h64, relerr(j32, j64), relerr(h32, h64))
    return value, jac, hess, relerr(h32, h64)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_at_random_coordinates(case):
    cin, cout, layers, features, n, act = case
    ref_m, x, v64, j64, h64, own_j, own_h = reference(case)
    m = _net(cin, cout, layers, features, act)
    assert torch.equal(m.params, ref_m.params)
    m.to(DEV)
    value, jac, hess = m.spatial_hessian(x.to(DEV))
    nh = cin * (cin + 1) // 2
    assert value.shape == (n, cout) and jac.shape == (n, cout, cin) and hess.shape == (n, cout, nh)
    assert value.dtype == jac.dtype == hess.dtype == torch.float32
    check_bands("case %s" % (case,), value.cpu().numpy(), jac.cpu().numpy(), hess.cpu().numpy(), v64, j64, h64, own_j, own_h)
    # the value and the Jacobian of the Hessian kernel lie within those bands of spatial_gradient's
    gv, gj = m.spatial_gradient(x.to(DEV))
    ev, ej = relerr(value.cpu().numpy(), gv.cpu().numpy()), relerr(jac.cpu().numpy(), gj.cpu().numpy())
    print("case %s: against spatial_gradient value %.3e, jacobian %.3e" % (case, ev, ej))
    assert ev < VALUE_TOL and ej < max(JAC_TOL, 3 * own_j)


def _grid_coords(dims, lo=-1.0, hi=1.0):
    axes = [torch.linspace(lo, hi, n) for n in dims]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(dims))


@pytest.mark.parametrize("dims", [(9, 10, 11), (13, 17)])
def test_grid_and_box(dims):
    nd = len(dims)
    nh = nd * (nd + 1) // 2
    cout = 2 if nd == 3 else 1
    m = _net(nd, cout, 4, 40, seed=3).to(DEV)
    total = int(np.prod(dims))
    hess, value, jac = m.decode_hessian_box(dims, want_value=True, want_jac=True)
    assert hess.shape == (*dims, cout, nh) and value.shape == (*dims, cout) and jac.shape == (*dims, cout, nd)
    x = _grid_coords(dims)
    v64, j64, h64 = value_jacobian_hessian(m, x, torch.float64)
    _, j32, h32 = value_jacobian_hessian(m, x, torch.float32)
    check_bands("grid %s" % (dims,), value.cpu().numpy().reshape(total, cout), jac.cpu().numpy().reshape(total, cout, nd),
                hess.cpu().numpy().reshape(total, cout, nh), v64, j64, h64, relerr(j32, j64), relerr(h32, h64))
    only = m.decode_hessian_box(dims)
    assert torch.is_tensor(only) and torch.equal(only, hess)
    # a strided box is the slice of the whole, bit for bit
    step = [2, 3, 2][:nd]
    sl = tuple(slice(1, None, s) for s in step)
    bh, bv, bj = m.decode_hessian_box(dims, start=1, stop=None, step=step, want_value=True, want_jac=True)
    assert bh.shape[:nd] == hess[sl].shape[:nd] and min(bh.shape[:nd]) > 1
    assert torch.equal(bh, hess[sl]) and torch.equal(bv, value[sl]) and torch.equal(bj, jac[sl])
    # neither the chunking nor a repeat changes a bit
    for chunk in (1, 3, 5, 8, 13, total, total):
        ch, cv, cj = m.decode_hessian_box(dims, chunk=chunk, want_value=True, want_jac=True)
        assert torch.equal(ch, hess) and torch.equal(cv, value) and torch.equal(cj, jac), chunk
    assert torch.equal(m.decode_hessian_box(dims, start=1, stop=None, step=step, chunk=13), bh)
    # the other sample sources of the C-ABI: grid voxels from an offset, and through an index list
    L = _lib.lib()
    pk = m._sync_jac()
    g = m._grid(dims, -1.0, 1.0)
    off, cnt = 5, total - 9
    ov, oj, oh = torch.empty((cnt, cout), device=DEV), torch.empty((cnt, cout, nd), device=DEV), torch.empty((cnt, cout, nh), device=DEV)
    b = _lib.BatchDesc(None, None, None, None, off, cnt, 0, 0, 0)
    _lib.check(L.brief_siren_hess_forward(C.byref(m.desc), _lib.ptr(pk), C.byref(g), C.byref(b), _lib.ptr(ov), _lib.ptr(oj), _lib.ptr(oh), _lib.stream_ptr()))
    assert torch.equal(oh, hess.view(total, cout, nh)[off:off + cnt]) and torch.equal(oj, jac.view(total, cout, nd)[off:off + cnt])
    assert torch.equal(ov, value.view(total, cout)[off:off + cnt])
    idx = torch.randperm(total, generator=torch.Generator().manual_seed(2))[:37].to(DEV)
    iv, ij, ih = torch.empty((37, cout), device=DEV), torch.empty((37, cout, nd), device=DEV), torch.empty((37, cout, nh), device=DEV)
    b = _lib.BatchDesc(None, None, None, idx.data_ptr(), 0, 37, 0, 0, 0)
    _lib.check(L.brief_siren_hess_forward(C.byref(m.desc), _lib.ptr(pk), C.byref(g), C.byref(b), _lib.ptr(iv), _lib.ptr(ij), _lib.ptr(ih), _lib.stream_ptr()))
    assert torch.equal(ih, hess.view(total, cout, nh)[idx]) and torch.equal(ij, jac.view(total, cout, nd)[idx]) and torch.equal(iv, value.view(total, cout)[idx])


@pytest.mark.parametrize("cin", [3, 2])
def test_repeat_and_permutation_are_bitwise(cin):
    """two identical calls give identical bits, and a permutation of the coordinates permutes the rows bit for bit: a sample's result
    does not depend on its slot in the tile or on its neighbours; NULL value / jac leave hess unchanged"""
    m = _net(cin, 2, 5, 70, seed=4).to(DEV)
    x = case_coords(203, cin, seed=6).to(DEV)
    v0, j0, h0 = m.spatial_hessian(x)
    v1, j1, h1 = m.spatial_hessian(x)
    assert torch.equal(v0, v1) and torch.equal(j0, j1) and torch.equal(h0, h1)
    perm = torch.randperm(203, generator=torch.Generator().manual_seed(8)).to(DEV)
    vp, jp, hp = m.spatial_hessian(x[perm])
    assert torch.equal(vp, v0[perm]) and torch.equal(jp, j0[perm]) and torch.equal(hp, h0[perm])
    for wv, wj in ((False, True), (True, False), (False, False)):
        v, j, h = m.spatial_hessian(x, want_value=wv, want_jac=wj)
        assert (v is None) == (not wv) and (j is None) == (not wj) and torch.equal(h, h0)
        assert (v is None or torch.equal(v, v0)) and (j is None or torch.equal(j, j0))
    dims = (5, 6, 7)[:cin]
    hb, vb, jb = m.decode_hessian_box(dims, want_value=True, want_jac=True)
    assert torch.equal(m.decode_hessian_box(dims), hb)
    hb2, vb2, none = m.decode_hessian_box(dims, want_value=True)
    assert none is None and torch.equal(hb2, hb) and torch.equal(vb2, vb)


def _volume_targets(dims, seed=3):
    vol = make_volume(dims, seed=seed).astype(np.float32).reshape(-1, 1)
    vol = (vol - vol.min()) / (vol.max() - vol.min()) * 100.0
    return torch.from_numpy(vol).to(DEV)


def test_fitted_net_and_fresh_fragment_copy(tmp_path):
    """the fifteenth parity case, a net after a 200-step fit on a make_volume block, and the freshness of the derived fragment copy: after
    a fit and after load_state_dict the result is the NEW parameters'.  The fitted case's band may not leave 1e-3: with the fourteen
    initialised cases unwidened (tests/test_hessian_host.py::test_band_cap_of_the_parity_cases) it is then at most 1 widened comparison
    of 15, inside the cap of tests/_bands.py."""
    dims = (12, 20, 28)
    m = _net(3, 1, 5, 48, seed=2).to(DEV)
    x = case_coords(300, 3, seed=9)
    _, _, h0, _ = _full_check(m, x, "before the fit")
    before = m.params.detach().cpu().clone()
    fit = Fitter(m, _volume_targets(dims), dims, sampler="randompoint", sample_size=2000, optimizer="Adamax", lr=1e-3, seed=1)
    fit.run(200)
    assert not torch.equal(m.params.detach().cpu(), before)
    _, _, h1, own = _full_check(m, x, "after a 200-step fit")
    assert not torch.equal(h1, h0)
    assert max(HESS_TOL, 3 * own) <= _bands.MAX_BAND["grad"], "the fitted case's band leaves the cap: own %.3e" % own
    # load_state_dict: another net's weights
    other = _net(3, 1, 5, 48, seed=77)
    m.load_state_dict(other.state_dict())
    _, _, h2, _ = _full_check(m, x, "after load_state_dict", ref=other)
    assert torch.equal(m.params.detach().cpu(), other.params)
    _, _, h3 = m.spatial_hessian(x.to(DEV))
    assert torch.equal(h3, h2)
    # load_model: a third net's stored weights, read into the module where it lives
    third = _net(3, 1, 5, 48, seed=78)
    save_model(third, str(tmp_path / "module"))
    load_model(m, str(tmp_path / "module"), DEV)
    assert m.params.device.type == "cuda" and torch.equal(m.params.detach().cpu(), third.params)
    _, _, h4, _ = _full_check(m, x, "after load_model", ref=third)
    assert not torch.equal(h4, h2)
    h2 = h4
    # to(): a round trip through the CPU allocates the copy anew on the device it lands on
    m.to("cpu").to(DEV)
    assert torch.equal(m.spatial_hessian(x.to(DEV))[2], h2)


def test_python_refusals():
    x = case_coords(8, 3).to(DEV)
    torch.manual_seed(0)
    for net, what in ((FFN(coords_channel=3, data_channel=1, features=32, layers=3, embsize=16), "FFN"),
                      (SIREN_Pyramid(coords_channel=3, data_channel=1, features=40, layers=4, features_dis=5), "SIREN_Pyramid"),
                      (SIREN(coords_channel=3, data_channel=1, features=64, layers=3, precision="bf16"), "bf16"),
                      (SIREN(coords_channel=3, data_channel=1, features=64, layers=3, precision="bf16x3"), "bf16x3"),
                      (SIREN(coords_channel=3, data_channel=1, features=1025, layers=3), "1025")):
        net.to(DEV)
        with pytest.raises(_lib.BriefError, match=r"spatial Hessians exist for fp32 SIREN up to 1024 features \(this net is .*%s" % what):
            net.spatial_hessian(x)
        with pytest.raises(_lib.BriefError, match="spatial Hessians exist for fp32 SIREN"):
            net.decode_hessian_box((4, 4, 4))


SENTINEL = 12345.0


def test_entry_contract_refusals_write_nothing():
    """a null hess, a bad desc and more than 1024 features return the Jacobian entries' error code (BRIEF_ERR_INVALID = -1) with a
    message naming the limit, before any launch: the sentinel-filled outputs stay as they are"""
    L = _lib.lib()
    m = _net(3, 1, 3, 40).to(DEV)
    pk = m._sync_jac()
    n = 16
    x = case_coords(n, 3).to(DEV)
    value, jac, hess = (torch.full(s, SENTINEL, device=DEV) for s in ((n, 1), (n, 1, 3), (n, 1, 6)))
    st = _lib.stream_ptr()

    def desc(**kw):
        d = _lib.SirenDesc(3, 1, 3, 40, 30.0, 30.0, 0, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def batch(**kw):
        b = _lib.BatchDesc(x.data_ptr(), None, None, None, 0, n, 0, 0, 0)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def box(**kw):
        bx = _lib.GridBox()
        bx.grid = m._grid((4, 4, 4), -1.0, 1.0)
        for a in range(3):
            bx.start[a], bx.step[a], bx.extent[a] = 0, 1, 4
        for k, (a, v) in kw.items():
            getattr(bx, k)[a] = v
        return bx

    def fwd(d, packed=pk, b=None, v=value, j=jac, h=hess):
        return L.brief_siren_hess_forward(C.byref(d) if d is not None else None, _lib.ptr(packed), None, C.byref(b or batch()), _lib.ptr(v), _lib.ptr(j),
                                          _lib.ptr(h), st)

    def fbox(d, packed=pk, bx=None, off=0, cnt=n, v=value, j=jac, h=hess, nobox=False):
        return L.brief_siren_hess_forward_box(C.byref(d) if d is not None else None, _lib.ptr(packed), None if nobox else C.byref(bx or box()), off, cnt,
                                              _lib.ptr(v), _lib.ptr(j), _lib.ptr(h), st)

    bad_descs = [(dict(precision=1), "BRIEF_PREC_F32"), (dict(precision=2), "BRIEF_PREC_F32"), (dict(features=0), "1..1024"),
                 (dict(features=1025), "1..1024"), (dict(layers=1), "layers must be >= 2"), (dict(cin=1), "2 or 3"), (dict(cin=4), "2 or 3"),
                 (dict(cout=0), "1..4"), (dict(cout=5), "1..4")]
    for kw, what in bad_descs:
        d = desc(**kw)
        jac_rc = L.brief_siren_jac_forward(C.byref(d), _lib.ptr(pk), None, C.byref(batch()), _lib.ptr(value), _lib.ptr(jac), st)
        for rc in (fwd(d), fbox(d)):
            assert rc == jac_rc == -1 and what in L.brief_last_error().decode(), (kw, L.brief_last_error())
    good = desc()
    calls = [(lambda: fwd(None), "null desc"), (lambda: fbox(None), "null desc"),
             (lambda: fwd(good, packed=None), "null"), (lambda: fwd(good, h=None), "null"), (lambda: fwd(good, b=batch(n=0)), "empty batch"),
             (lambda: fwd(good, b=batch(coords=None)), "grid.ndim"),
             (lambda: fbox(good, packed=None), "null"), (lambda: fbox(good, h=None), "null"), (lambda: fbox(good, nobox=True), "null box"),
             (lambda: fbox(good, cnt=0), "empty batch"), (lambda: fbox(good, off=60), "offset"), (lambda: fbox(good, off=-1), "offset"),
             (lambda: fbox(good, bx=box(extent=(1, 5))), "exceeds"), (lambda: fbox(good, bx=box(step=(2, 0))), "step"),
             (lambda: fbox(good, bx=box(start=(0, -1))), "exceeds")]
    for i, (call, what) in enumerate(calls):
        assert call() == -1 and what in L.brief_last_error().decode(), (i, L.brief_last_error())
    torch.cuda.synchronize()
    assert bool((value == SENTINEL).all()) and bool((jac == SENTINEL).all()) and bool((hess == SENTINEL).all())
    # the accepted call with value and jac NULL writes every element of hess and nothing else
    assert fwd(good, v=None, j=None) == 0
    torch.cuda.synchronize()
    assert not bool((hess == SENTINEL).any()) and bool((value == SENTINEL).all()) and bool((jac == SENTINEL).all())
    # ... and with all three every element of each
    assert fbox(good) == 0
    torch.cuda.synchronize()
    assert not bool((value == SENTINEL).any()) and not bool((jac == SENTINEL).any())
