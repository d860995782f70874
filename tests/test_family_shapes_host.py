"""What the case table of tests/_family_shapes.py reaches in the family driver, proved from the restated launch arithmetic for devices of
32, 64, 128 and 256 CUs, and the two conditions the GPU file (tests/test_gpu_family_shapes.py) relies on that involve the float64
reference alone.  No GPU, no HIP library."""
import numpy as np
import pytest
import torch

from tests import _family_shapes as S

KERNELS = ("ffn", "nerf", "mfnf", "mfng", "taper")


def test_the_arithmetic_restates_the_drivers_figures():
    """the figures csrc/brief_family_host.inc, brief_nerf.inc and brief_taper.inc state themselves"""
    assert [S.mtw(nt) for nt in (1, 4, 5, 29, 32)] == [1, 1, 2, 8, 8]
    wide = S.BY_ID["c-ffn-lds"].make()
    assert S.lds_bytes(wide) == 131584 and S.by_lds(131584) == 1                            # FFN(embsize=512, features=40): K0 = 1024 rows
    assert S.lds_bytes(S.N.NeRF(features=1024, frequencies=10)) == 139776                   # brief_nerf.inc: (64 + 1024) * 128 + 512
    assert S.lds_bytes(S.N.NeRF(features=507, frequencies=10)) == 74240
    assert S.lds_bytes(S.N.SIREN_Pyramid(features=1024, features_dis=0)) == 131584          # brief_taper.inc: 1024 rows
    # family_ksplit with 3 wave jobs on 256 CUs
    narrow = S.BY_ID["b-ffn-n513"].make()
    assert S.wave_jobs(narrow) == 3
    assert S.family_ksplit(544, 3, 256) == (2, 288, 2) and 544 - 288 == 256                 # n = 513: 2 splits of 288, the last of 256
    assert S.family_ksplit(2592, 3, 256) == (10, 288, 9)                                    # n = 2561: ns = 10 but nsplit = 9
    assert S.family_ksplit(20032, 3, 256) == (64, 320, 63) and 20032 - 62 * 320 == 192      # n = 20001: 63 splits of 320, the last of 192
    assert S.family_grid(S.lds_bytes(narrow), 20001, 256) == 512 and (20001 + 31) // 32 == 626
    assert S.family_grid(131584, 32 * 256 + 33, 256) == 256
    # wgrad_count of the deep nets
    assert [S.wgrad_count(r.make()) for r in S.DEEP] == [34, 34, 33, 34]


@pytest.mark.parametrize("cus", S.CU_COUNTS)
def test_every_row_reaches_what_it_claims(cus):
    for row in S.ROWS:
        m = row.make()
        n = row.batch_n(m, cus)
        facts = S.reach(m, n, cus)
        assert not S.unmet(row.claims, facts), (row.id, n, S.unmet(row.claims, facts), facts)
        assert 1 <= facts["mtw"] <= 8 and facts["lds"] <= S.LDS_BUDGET and facts["grid"] <= 4096      # kFfnLossParts


def test_rows_keep_the_literal_batch_sizes_on_the_four_cu_counts():
    """no search is needed on the CU counts the table was written for: batch_n() returns the row's own n"""
    for cus in S.CU_COUNTS:
        for row in S.ROWS:
            want = row.n(cus) if callable(row.n) else row.n
            assert row.batch_n(row.make(), cus) == want, (row.id, cus)


@pytest.mark.parametrize("cus", S.CU_COUNTS)
def test_the_table_covers_the_launch_space(cus):
    got = {}
    for row in S.ROWS:
        m = row.make()
        got[row.id] = (S.kernel_family(row), S.family_of(m), S.reach(m, row.batch_n(m, cus), cus))
    where = lambda pred: sorted(rid for rid, (k, fam, f) in got.items() if pred(k, fam, f))
    for kern in KERNELS:
        # every MTW for TRAIN, decode and BOX (a row runs all three), at nt % 4 = 1 and with a partial last K step
        for M in range(1, 9):
            assert where(lambda k, fam, f: k == kern and f["mtw"] == M and f["nt"] == 4 * M - 3 and f["widest"] % 8), (kern, M)
        assert where(lambda k, fam, f: k == kern and f["nt"] == 32), kern
        # the batch edges and the split edges, per family (the MFN rows run the Gabor kernel)
        if kern != "mfnf":
            for lanes, tiles in ((1, 1), (31, 1), (32, 1), (1, 2)):
                assert where(lambda k, fam, f: k == kern and f["last_lanes"] == lanes and f["tiles"] == tiles), (kern, lanes, tiles)
            assert where(lambda k, fam, f: k == kern and f["ns"] == 1 and f["npad"] >= 256), kern
            assert where(lambda k, fam, f: k == kern and f["ns"] > 1 and f["last_chunk"] < f["chunk"] and f["nsplit"] == f["ns"]), kern
            assert where(lambda k, fam, f: k == kern and f["nsplit"] < f["ns"]), kern
        # a second tile at two workgroups per CU, ns at the 64 cap
        assert where(lambda k, fam, f: k == kern and f["tiles"] > f["grid"] and f["tiles"] % f["grid"] and f["by_lds"] >= 2 and f["ns"] == 64), kern
        assert where(lambda k, fam, f: k == kern and (f["cin"], f["cout"]) == (2, 4)), kern
    assert where(lambda k, fam, f: f["nsplit"] == 64)
    assert where(lambda k, fam, f: f["by_lds"] == 1 and f["tiles"] > f["grid"] and f["tiles"] % f["grid"])
    for kern in ("ffn", "nerf", "mfnf", "mfng"):
        assert where(lambda k, fam, f: k == kern and f["launches"] == 2), kern
    for cls in (S.N.SIREN_Pyramid, S.N.SIRENFT, S.N.SIRENPS):
        assert [r.id for r in S.ROWS if r.cls is cls and r.kwargs["layers"] == 16], cls.__name__
    assert where(lambda k, fam, f: fam == "taper" and f["layers"] == 3)
    if cus == 256:      # on the device the table was written for, the two-tile walk is exactly that: 626 tiles over 512 workgroups
        f = got["c-ffn-walk"][2]
        assert (f["tiles"], f["grid"], f["nsplit"], f["chunk"], f["last_chunk"]) == (626, 512, 63, 320, 192)


def test_the_three_loss_settings_rotate_over_every_kernel():
    for kern in KERNELS:
        assert {r.li for r in S.ROWS if S.kernel_family(r) == kern and r.id.startswith("a-")} == {0, 1, 2}, kern


@pytest.mark.parametrize("row", S.DEEP, ids=lambda r: r.id)
def test_no_deep_net_leaves_a_tensor_without_a_gradient(row):
    """a tensor whose float64 gradient is all zero (dead ReLUs) would pass any band: every tensor of the deep nets has a non-zero one"""
    res, comps = S.reference(row, row.n)
    smallest = min(S.np_max(res[torch.float64][2][k][..., sl]) for _, k, _, _, sl in comps)
    print("%s: smallest per-tensor max |gradient| %.2e over %d tensors" % (row.id, smallest, len(comps)))
    assert smallest > 0.0
    assert all(np.isfinite(res[torch.float64][2][k]).all() for _, k, _, _, _ in comps)


def test_the_tapered_rows_need_no_widened_band():
    """`own` involves no GPU: over the gradient comparisons of the tapered rows none needs a band above 1e-4 (so the cap of
    tests/_bands.py, at most 0.15 widened and none above 1e-3, holds over the new cases alone)"""
    total = widened = 0
    worst = ("", 0.0)
    for row in S.TAPER:
        n = row.n(256) if callable(row.n) else row.n
        for v in S.taper_owns(row, n):
            total += 1
            widened += v > S.TAPER_GRAD_TOL
            worst = max(worst, (row.id, v), key=lambda t: t[1])
    print("tapered gradient comparisons %d, widened %d, worst 3 x own %.2e (%s)" % (total, widened, worst[1], worst[0]))
    assert widened == 0 and total > 0
    assert widened <= S.MAX_WIDENED_FRACTION * total and worst[1] <= S.MAX_BAND


def test_no_row_sits_on_a_discontinuity_of_its_reference():
    """a ReLU argument or a thresholded output within the forward band of its switching point makes the gradient of that sample a
    matter of rounding (either side is right in fp32): the batches of the table hold no such sample, so a gradient band can hold"""
    redrawn = 0
    for row in S.ROWS:
        m = row.make()
        n = row.n(256) if callable(row.n) else row.n
        x, y, w = row.batch(m, n)
        assert x.shape == (n, m.coords_channel) and float(x.abs().max()) <= 1.0
        assert not S.close_calls(row, m, x).any(), row.id
        redrawn += int((x != S.R.rand_coords(n, m.coords_channel, 11)).any(1).sum())
    print("samples drawn again over the table: %d" % redrawn)


def test_the_plain_draw_has_such_a_sample():
    """the 20 001 plain draws of the narrow FFN hold one: sample 499 puts a unit of the last hidden layer at 2.5e-7, inside the fp32
    error of its argument (torch fp32 keeps the sign there, a kernel need not), worth 0.1 / n in two layers' gradients"""
    row = S.BY_ID["c-ffn-walk"]
    m = row.make()
    x = S.R.rand_coords(20001, 3, 11)
    bad = S.close_calls(row, m, x)
    taps = []
    S.R.torch_ffn(m, x, torch.float64, taps)
    assert bad[499] and float(taps[1][499].abs().min()) < 1e-6
    assert 0 < int(bad.sum()) < 0.05 * len(bad)
