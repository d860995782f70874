"""Spatial-gradient decode on the GPU (csrc/brief_jac.inc) through networks.SIREN and the C-ABI: value and Jacobian against the float64
restatement of tests/_jacobian.py inside the bands of the sine nets (value 2e-5; Jacobian max(1e-4, 3 x torch's own fp32 distance), both
distances printed), and the contracts of decode_box: a box is the slice of the whole, and neither the chunking, a repeat nor a sample's
slot in its tile changes a bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import FFN, SIREN, SIREN_Pyramid
from brief_pytorch_amd.synthetic import make_volume

from ._jacobian import check_bands

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (cin, cout, layers, features, n, output_act): the ten shapes of the feature's issue, then two of them with the output activation and
# two with a single sample
CASES = [(3, 1, 5, 256, 1000, False), (3, 1, 5, 22, 1000, False), (3, 1, 5, 1, 9, False), (3, 1, 5, 32, 8, False), (2, 3, 3, 33, 7, False),
         (2, 1, 3, 65, 255, False), (3, 4, 9, 300, 300, False), (3, 1, 2, 33, 500, False), (3, 2, 5, 1024, 64, False), (3, 1, 4, 527, 40, False),
         (2, 3, 3, 33, 7, True), (3, 1, 5, 256, 1000, True), (3, 1, 5, 22, 1, False), (3, 2, 5, 1024, 1, False)]


def _net(cin, cout, layers, features, act=False, seed=0):
    torch.manual_seed(seed)
    return SIREN(coords_channel=cin, data_channel=cout, features=features, layers=layers, w0=30, output_act=act)


def _coords(n, cin, seed=1):
    return torch.rand(n, cin, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dto%d_%dx%d_n%d%s" % (c[0], c[1], c[2], c[3], c[4], "_act" if c[5] else ""))
def test_parity_at_random_coordinates(case):
    cin, cout, layers, features, n, act = case
    m = _net(cin, cout, layers, features, act)
    x = _coords(n, cin)
    m.to(DEV)
    value, jac = m.spatial_gradient(x.to(DEV))
    assert value.shape == (n, cout) and jac.shape == (n, cout, cin) and value.dtype == jac.dtype == torch.float32
    check_bands(m, x, value.cpu().numpy(), jac.cpu().numpy(), "case %s" % (case,))


def _grid_coords(dims, lo=-1.0, hi=1.0):
    axes = [torch.linspace(lo, hi, n) for n in dims]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(dims))


@pytest.mark.parametrize("dims", [(9, 10, 11), (13, 17)])
def test_grid_and_box(dims):
    nd = len(dims)
    cout = 2 if nd == 3 else 1
    m = _net(nd, cout, 4, 40, seed=3).to(DEV)
    total = int(np.prod(dims))
    jac, value = m.decode_gradient_box(dims)
    assert jac.shape == (*dims, cout, nd) and value.shape == (*dims, cout)
    check_bands(m, _grid_coords(dims), value.cpu().numpy().reshape(total, cout), jac.cpu().numpy().reshape(total, cout, nd), "grid %s" % (dims,))
    # a strided box is the slice of the whole, bit for bit
    step = [2, 3, 2][:nd]
    sl = tuple(slice(1, None, s) for s in step)
    bj, bv = m.decode_gradient_box(dims, start=1, stop=None, step=step)
    assert bj.shape[:nd] == jac[sl].shape[:nd] and min(bj.shape[:nd]) > 1
    assert torch.equal(bj, jac[sl]) and torch.equal(bv, value[sl])
    # neither the chunking nor a repeat changes a bit
    for chunk in (1, 5, 8, 13, total):
        cj, cv = m.decode_gradient_box(dims, chunk=chunk)
        assert torch.equal(cj, jac) and torch.equal(cv, value), chunk
    cj, cv = m.decode_gradient_box(dims, start=1, stop=None, step=step, chunk=13)
    assert torch.equal(cj, bj) and torch.equal(cv, bv)
    # the other sample sources of the C-ABI: grid voxels from an offset, and through an index list
    L = _lib.lib()
    pk = m._sync_jac()
    g = m._grid(dims, -1.0, 1.0)
    off, cnt = 5, total - 9
    ov, oj = torch.empty((cnt, cout), device=DEV), torch.empty((cnt, cout, nd), device=DEV)
    b = _lib.BatchDesc(None, None, None, None, off, cnt, 0, 0, 0)
    _lib.check(L.brief_siren_jac_forward(C.byref(m.desc), _lib.ptr(pk), C.byref(g), C.byref(b), _lib.ptr(ov), _lib.ptr(oj), _lib.stream_ptr()))
    assert torch.equal(oj, jac.view(total, cout, nd)[off:off + cnt]) and torch.equal(ov, value.view(total, cout)[off:off + cnt])
    idx = torch.randperm(total, generator=torch.Generator().manual_seed(2))[:37].to(DEV)
    iv, ij = torch.empty((37, cout), device=DEV), torch.empty((37, cout, nd), device=DEV)
    b = _lib.BatchDesc(None, None, None, idx.data_ptr(), 0, 37, 0, 0, 0)
    _lib.check(L.brief_siren_jac_forward(C.byref(m.desc), _lib.ptr(pk), C.byref(g), C.byref(b), _lib.ptr(iv), _lib.ptr(ij), _lib.stream_ptr()))
    assert torch.equal(ij, jac.view(total, cout, nd)[idx]) and torch.equal(iv, value.view(total, cout)[idx])


def test_repeat_and_permutation_are_bitwise():
    """two identical calls give identical bits, and a permutation of the coordinates permutes the rows bit for bit: a sample's result
    does not depend on its slot in the tile or on its neighbours"""
    m = _net(3, 2, 5, 70, seed=4).to(DEV)
    x = _coords(203, 3, seed=6).to(DEV)
    v0, j0 = m.spatial_gradient(x)
    v1, j1 = m.spatial_gradient(x)
    assert torch.equal(v0, v1) and torch.equal(j0, j1)
    perm = torch.randperm(203, generator=torch.Generator().manual_seed(8)).to(DEV)
    vp, jp = m.spatial_gradient(x[perm])
    assert torch.equal(vp, v0[perm]) and torch.equal(jp, j0[perm])
    # want_value=False / value == NULL leaves the Jacobian unchanged
    none, jn = m.spatial_gradient(x, want_value=False)
    assert none is None and torch.equal(jn, j0)
    jb, vb = m.decode_gradient_box((5, 6, 7))
    jb2, none = m.decode_gradient_box((5, 6, 7), want_value=False)
    assert none is None and torch.equal(jb2, jb)


def _volume_targets(dims, seed=3):
    vol = make_volume(dims, seed=seed).astype(np.float32).reshape(-1, 1)
    vol = (vol - vol.min()) / (vol.max() - vol.min()) * 100.0
    return torch.from_numpy(vol).to(DEV)


def test_fragment_copy_is_fresh_after_a_fit_and_a_load():
    """the Jacobian kernel reads a derived copy of the parameters of its own; after they change it must be the NEW parameters'"""
    dims = (12, 20, 28)
    m = _net(3, 1, 5, 48, seed=2).to(DEV)
    x = _coords(300, 3, seed=9)
    v0, j0 = m.spatial_gradient(x.to(DEV))
    check_bands(m, x, v0.cpu().numpy(), j0.cpu().numpy(), "before the fit")
    before = m.params.detach().cpu().clone()
    fit = Fitter(m, _volume_targets(dims), dims, sampler="randompoint", sample_size=2000, optimizer="Adamax", lr=1e-3, seed=1)
    fit.run(10)
    assert not torch.equal(m.params.detach().cpu(), before)
    v1, j1 = m.spatial_gradient(x.to(DEV))
    assert not torch.equal(j1, j0)
    check_bands(m, x, v1.cpu().numpy(), j1.cpu().numpy(), "after 10 steps")
    # load_state_dict: another net's weights
    other = _net(3, 1, 5, 48, seed=77)
    m.load_state_dict(other.state_dict())
    v2, j2 = m.spatial_gradient(x.to(DEV))
    check_bands(other, x, v2.cpu().numpy(), j2.cpu().numpy(), "after load_state_dict")
    assert torch.equal(m.params.detach().cpu(), other.params)
    # moved weights: after 200 steps they are no longer at their initial scale
    fit = Fitter(m, _volume_targets(dims), dims, sampler="randompoint", sample_size=2000, optimizer="Adamax", lr=1e-3, seed=1)
    fit.run(200)
    v3, j3 = m.spatial_gradient(x.to(DEV))
    check_bands(m, x, v3.cpu().numpy(), j3.cpu().numpy(), "after 200 steps")
    # to(): a round trip through the CPU allocates the copy anew on the device it lands on
    m.to("cpu").to(DEV)
    v4, j4 = m.spatial_gradient(x.to(DEV))
    assert torch.equal(v4, v3) and torch.equal(j4, j3)


def test_python_refusals():
    x = _coords(8, 3).to(DEV)
    torch.manual_seed(0)
    for net, what in ((FFN(coords_channel=3, data_channel=1, features=32, layers=3, embsize=16), "FFN"),
                      (SIREN_Pyramid(coords_channel=3, data_channel=1, features=40, layers=4, features_dis=5), "SIREN_Pyramid"),
                      (SIREN(coords_channel=3, data_channel=1, features=64, layers=3, precision="bf16"), "bf16"),
                      (SIREN(coords_channel=3, data_channel=1, features=64, layers=3, precision="bf16x3"), "bf16x3"),
                      (SIREN(coords_channel=3, data_channel=1, features=1025, layers=3), "1025")):
        net.to(DEV)
        with pytest.raises(_lib.BriefError, match=r"spatial gradients exist for fp32 SIREN up to 1024 features \(this net is .*%s" % what):
            net.spatial_gradient(x)
        with pytest.raises(_lib.BriefError, match="spatial gradients exist for fp32 SIREN"):
            net.decode_gradient_box((4, 4, 4))


SENTINEL = 12345.0


def test_c_abi_refusals_write_nothing():
    """every refusal returns BRIEF_ERR_INVALID with its message before any launch: the sentinel-filled outputs stay as they are"""
    L = _lib.lib()
    m = _net(3, 1, 3, 40).to(DEV)
    pk = m._sync_jac()
    n = 16
    x = _coords(n, 3).to(DEV)
    value = torch.full((n, 1), SENTINEL, device=DEV)
    jac = torch.full((n, 1, 3), SENTINEL, device=DEV)
    packed = torch.full_like(pk, SENTINEL)
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

    bad_descs = [(dict(precision=1), "BRIEF_PREC_F32"), (dict(precision=2), "BRIEF_PREC_F32"), (dict(features=0), "1..1024"),
                 (dict(features=1025), "1..1024"), (dict(layers=1), "layers must be >= 2"), (dict(cin=1), "2 or 3"), (dict(cin=4), "2 or 3"),
                 (dict(cout=0), "1..4"), (dict(cout=5), "1..4")]
    for kw, what in bad_descs:
        d = desc(**kw)
        assert L.brief_siren_jac_packed_count(C.byref(d)) == -1 and what in L.brief_last_error().decode(), kw
        for rc in (L.brief_siren_jac_repack(C.byref(d), _lib.ptr(m.params), _lib.ptr(packed), st),
                   L.brief_siren_jac_forward(C.byref(d), _lib.ptr(pk), None, C.byref(batch()), _lib.ptr(value), _lib.ptr(jac), st),
                   L.brief_siren_jac_forward_box(C.byref(d), _lib.ptr(pk), C.byref(box()), 0, n, _lib.ptr(value), _lib.ptr(jac), st)):
            assert rc == -1 and what in L.brief_last_error().decode(), (kw, L.brief_last_error())
    good = desc()
    calls = [
        (lambda: L.brief_siren_jac_repack(C.byref(good), None, _lib.ptr(packed), st), "null"),
        (lambda: L.brief_siren_jac_repack(C.byref(good), _lib.ptr(m.params), None, st), "null"),
        (lambda: L.brief_siren_jac_forward(C.byref(good), None, None, C.byref(batch()), _lib.ptr(value), _lib.ptr(jac), st), "null"),
        (lambda: L.brief_siren_jac_forward(C.byref(good), _lib.ptr(pk), None, C.byref(batch()), _lib.ptr(value), None, st), "null"),
        (lambda: L.brief_siren_jac_forward(C.byref(good), _lib.ptr(pk), None, C.byref(batch(n=0)), _lib.ptr(value), _lib.ptr(jac), st), "empty batch"),
        (lambda: L.brief_siren_jac_forward(C.byref(good), _lib.ptr(pk), None, C.byref(batch(coords=None)), _lib.ptr(value), _lib.ptr(jac), st), "grid.ndim"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), None, C.byref(box()), 0, n, _lib.ptr(value), _lib.ptr(jac), st), "null"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box()), 0, n, _lib.ptr(value), None, st), "null"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), None, 0, n, _lib.ptr(value), _lib.ptr(jac), st), "null box"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box()), 0, 0, _lib.ptr(value), _lib.ptr(jac), st), "empty batch"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box()), 60, n, _lib.ptr(value), _lib.ptr(jac), st), "offset"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box()), -1, n, _lib.ptr(value), _lib.ptr(jac), st), "offset"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box(extent=(1, 5))), 0, n, _lib.ptr(value), _lib.ptr(jac), st), "exceeds"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box(step=(2, 0))), 0, n, _lib.ptr(value), _lib.ptr(jac), st), "step"),
        (lambda: L.brief_siren_jac_forward_box(C.byref(good), _lib.ptr(pk), C.byref(box(start=(0, -1))), 0, n, _lib.ptr(value), _lib.ptr(jac), st), "exceeds"),
    ]
    for i, (call, what) in enumerate(calls):
        assert call() == -1 and what in L.brief_last_error().decode(), (i, L.brief_last_error())
    torch.cuda.synchronize()
    assert bool((value == SENTINEL).all()) and bool((jac == SENTINEL).all()) and bool((packed == SENTINEL).all())
    # and the accepted call writes every element
    _lib.check(L.brief_siren_jac_forward(C.byref(good), _lib.ptr(pk), None, C.byref(batch()), _lib.ptr(value), _lib.ptr(jac), st))
    torch.cuda.synchronize()
    assert not bool((value == SENTINEL).any()) and not bool((jac == SENTINEL).any())
