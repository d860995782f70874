"""The family kernels over their whole launch space against float64: every row of tests/_family_shapes.py runs a forward, a train step
and a box decode on the fused HIP path.

    forward     m.forward against the float64 restatement, under the family's forward band
    train step  m.train_step against the restatement, under the family's bands: the loss, and every parameter tensor on its own
    box decode  a small decode_box equals the slice of decode_grid bit for bit (the BOX instantiation of the same MTW)

The bands are the per-family files': FFN, NeRF and MFN use band_check (fused against float64 <= 4 x (torch fp32 against float64) +
1e-5 of the largest reference entry, per tensor); the tapered SIRENs use forward < 2e-5, loss < 1e-4 and every tensor < max(1e-4,
3 x own) against torch fp32 (tests/test_gpu_taper.py; tests/test_family_shapes_host.py shows that no tapered row widens a band).

A row states what it reaches in the driver (the MTW instantiation, ragged wave ownership, the split-K edges, a second tile of the
persistent loop, a second weight-gradient launch, ...).  The test takes the CU count of the device, restates the driver's arithmetic for
it and fails, never skips, when the row does not reach what it claims there.  Every figure is printed before it is asserted
(profiles/r25_family_shapes.md holds them)."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from tests import _family_ref as R
from tests import _family_shapes as S

pytestmark = pytest.mark.gpu


def _band(got, r64, r32):
    """(error against float64, bound) of band_check"""
    got, r64, r32 = (np.asarray(v, dtype=np.float64) for v in (got, r64, r32))
    return float(np.max(np.abs(got - r64))), R.BAND_FACTOR * float(np.max(np.abs(r32 - r64))) + R.FLOOR * max(float(np.max(np.abs(r64))), 1e-30)


class _Report:
    """prints every figure, collects the failed ones: a row runs all three parts before it fails"""

    def __init__(self, rid):
        self.rid, self.failed = rid, []

    def check(self, what, err, bound, strict=False):
        ok = err < bound if strict else err <= bound
        print("  %s %-28s %.3e  band %.3e%s" % (self.rid, what, err, bound, "" if ok else "  FAILED"))
        if not ok:
            self.failed.append("%s: %.3e, band %.3e" % (what, err, bound))

    def banded(self, what, got, r64, r32):
        """tests/_family_ref.py band_check, its figures printed first"""
        self.check(what, *_band(got, r64, r32))
        try:
            R.band_check(got, r64, r32, what)
        except AssertionError as e:
            if not any(f.startswith(what + ":") for f in self.failed):
                self.failed.append(str(e))


@pytest.mark.parametrize("row", S.ROWS, ids=lambda r: r.id)
def test_forward_train_step_and_box_decode(row):
    cus = int(_lib.lib().brief_cu_count())
    m = row.make("cuda")
    n = row.batch_n(m, cus)
    facts = S.reach(m, n, cus)
    print("%s on %d CUs: n %d, %s" % (row.id, cus, n, " ".join("%s=%s" % kv for kv in sorted(facts.items()))))
    assert not S.unmet(row.claims, facts), "%s does not reach %s on %d CUs: %s" % (row.id, S.unmet(row.claims, facts), cus, facts)
    taper = S.family_of(m) == "taper"
    res, comps = S.reference(row, n)
    (y64, l64, g64), (y32, l32, g32) = res[torch.float64], res[torch.float32]
    x, y, w = row.batch(m, n)
    loss, weighted, thr = S.LOSSES[row.li]
    rep = _Report(row.id)

    # ---- forward (the decode instantiation)
    yh = m.forward(x.cuda()).cpu().numpy()
    assert yh.shape == (n, m.data_channel)
    if taper:
        rep.check("forward", R.relerr(yh, y64), S.TAPER_FWD_TOL, strict=True)
    else:
        rep.banded("forward", yh, y64, y32)

    # ---- train step (the TRAIN instantiation, the weight-gradient launches, the reduction)
    bv0 = m.params[:m.bv_count].clone()
    lo, _ = m.train_step(n, y.cuda().contiguous(), coords=x.cuda().contiguous(), weights=w.cuda().contiguous() if weighted else None,
                         loss=loss, thr=thr, beta=S.BETA)
    got_loss, got = lo.item(), m.grads.cpu().numpy()
    assert got.shape == (m.param_count,)
    if taper:
        rep.check("loss", abs(got_loss - l32) / abs(l32), S.TAPER_LOSS_TOL, strict=True)
    else:
        rep.banded("loss", [got_loss], [l64], [l32])
    for name, k, off, shp, sl in comps:      # every tensor in its own band: a small layer cannot hide behind a large one
        g = got[off:off + int(np.prod(shp))].reshape(shp)[..., sl]
        if taper:
            own = R.relerr(g32[k][..., sl], g64[k][..., sl])
            rep.check("grad " + name, R.relerr(g, g32[k][..., sl]), max(S.TAPER_GRAD_TOL, 3.0 * own), strict=True)
        else:
            rep.banded("grad " + name, g, g64[k][..., sl], g32[k][..., sl])
    if m.bv_count:
        assert np.all(got[:m.bv_count] == 0.0) and torch.equal(m.params[:m.bv_count], bv0), "bvals gets no gradient and does not move"

    # ---- box decode (the BOX instantiation) equals the slice of the grid decode, bit for bit
    dims, start, stop, step = S.box_plan(m.coords_channel)
    full = m.decode_grid(dims).view(*dims, m.data_channel)
    box = m.decode_box(dims, start=start, stop=stop, step=step)
    sl = tuple(slice(a, b, c) for a, b, c in zip(start, stop, step))
    same = torch.equal(box.cpu(), full[sl].cpu())
    print("  %s box %s of %s: %s" % (row.id, (start, stop, step), dims, "equal" if same else "DIFFERS"))
    if not same:
        rep.failed.append("decode_box differs from the slice of decode_grid")
    assert torch.isfinite(full).all()
    assert not rep.failed, "%s (%s): %s" % (row.id, row.claims, "; ".join(rep.failed))
