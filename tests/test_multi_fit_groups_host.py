"""What tests/test_gpu_multi_fit_groups.py relies on, proved without a GPU: the case lists of tests/_groups.py form the groups, singles and
stream slots their GPU tests are about (plan() restates brief_multi_fit's assignment), the jobs that host a group's device table are the ones
meant, the unlike jobs of case C really differ in every field the table and the per-slot kernel arguments carry, and the nets of case D are
shallow enough for the plain gradient band."""
import ctypes as C

import numpy as np
import pytest

from brief_pytorch_amd import _lib

from . import _groups as G


def _ws_bytes(s):
    """brief_train_workspace_bytes of the job (a host function of the library: no device needed)"""
    d = _lib.SirenDesc(s.cin, s.cout, s.L, s.F, G.W0, 30.0, int(s.output_act), _lib.PRECISION["fp32"])
    n = int(_lib.lib().brief_train_workspace_bytes(C.byref(d), s.batch))
    assert n > 0, str(s)
    return n


def test_plan_restates_the_rule_on_small_examples():
    """the rule itself, on lists short enough to read: newest group only, demotion, slots"""
    a, b, wide = G.spec(4, 22, (4, 4, 4)), G.spec(4, 40, (4, 4, 4)), G.spec(4, 96, (4, 4, 4))
    assert G.variant(a) == (1, 3) and G.variant(b) == (2, 3) and G.variant(wide) is None
    assert G.variant(G.spec(9, 64, (4, 4, 4))) == (2, 7) and G.variant(G.spec(10, 24, (4, 4, 4))) is None      # eight hidden layers
    assert G.variant(G.spec(2, 1, (4, 4, 4))) == (1, 1) and G.variant(G.spec(3, 32, (4, 4, 4))) == (1, 1) and G.variant(G.spec(3, 33, (4, 4, 4))) == (2, 1)
    groups, singles, units = G.plan([a, wide, b, a, b, a])
    assert groups == [(1, 3, [0, 3, 5]), (2, 3, [2, 4])] and singles == [1]
    assert units == [("group", 0), ("group", 1), ("single", 1)]
    groups, singles, units = G.plan([a, b, wide])                      # two groups of one: both dissolved, job order kept
    assert groups == [] and singles == [0, 1, 2] and units == [("single", 0), ("single", 1), ("single", 2)]
    # a full group: the next job of the variant opens a new one behind the groups opened meanwhile; the lone (2, 3) job is joined later
    groups, singles, _ = G.plan([a] * 64 + [b] + [a] * 2 + [b])
    assert [len(j) for _, _, j in groups] == [64, 2, 2] and [(nt, hb) for nt, hb, _ in groups] == [(1, 3), (2, 3), (1, 3)] and singles == []
    assert G.stream_of([0] * 10, 9) == 1 and G.stream_of([0] * 3, 2) == 2


def test_workgroups_restates_small_grid():
    one, two = G.spec(4, 22, (4, 4, 4), "randompoint", 1), G.spec(4, 40, (4, 4, 4), "randompoint", 1)
    for n, w1, w2 in ((1, 1, 1), (64, 1, 1), (65, 1, 1), (128, 1, 1), (129, 1, 2), (256, 1, 2), (257, 2, 3), (321, 2, 3), (700, 3, 6), (768, 3, 6)):
        assert G.workgroups(one._replace(n=n)) == w1 and G.workgroups(two._replace(n=n)) == w2, n
    # more tiles than two rounds of resident workgroups hold: three rounds (2 x 256 workgroups resident up to hb = 3, 256 above)
    assert G.workgroups(one._replace(n=128 * 1025)) == 342 and G.workgroups(G.spec(8, 22, (4, 4, 4), "randompoint", 128 * 513)) == 171


def test_case_a_has_every_variant_in_groups_of_five_that_interleave():
    groups, singles, units = G.plan(G.A)
    assert len(G.A) == 42
    assert sorted((nt, hb) for nt, hb, _ in groups) == sorted(G.A_VARIANTS) and len(groups) == 8
    assert all(len(jobs) == 5 for _, _, jobs in groups)
    assert singles == [13, 27] and G.variant(G.A[13]) is None and G.variant(G.A[27]) is None
    assert (G.A[13].L, G.A[13].F) == (4, 96) and (G.A[27].L, G.A[27].F) == (10, 24)
    assert len(units) == 10 > G.POOL_STREAMS                             # two units share a stream with a group
    assert [G.stream_of(units, u) for u in (8, 9)] == [0, 1] and units[8] == ("single", 13) and units[9] == ("single", 27)
    for nt, hb, jobs in groups:
        assert all(b - a > 1 for a, b in zip(jobs, jobs[1:])), (nt, hb, jobs)      # never contiguous in the job array
        assert {G.A[j].L for j in jobs} == set(G._A_L[hb]), (nt, hb)               # both depths of the bucket
        assert {G.A[j].F for j in jobs} == set(G._A_F[nt]), (nt, hb)               # one, partial and full tiles
        assert len({G.A[j].sampler for j in jobs}) == 2, (nt, hb)
        assert len({G.workgroups(G.A[j]) for j in jobs}) > 1, (nt, hb)
    narrow = [s for s in G.A if G.variant(s) is not None]
    assert {s.n for s in narrow if s.sampler == "randompoint"} == {1, 33, 300, 700}
    assert {s.dims for s in narrow} >= {(4, 4, 4), (8, 8, 12)} and max(s.pop for s in G.A) == 8 * 8 * 12
    assert len({s.seed for s in G.A}) == len(G.A)
    for _, _, jobs in groups:                                            # a job's rate differs from that of the job whose INDEX equals its slot
        assert any(G.base_lr(G.A[j]) != G.base_lr(G.A[slot]) for slot, j in enumerate(jobs)), jobs


@pytest.mark.parametrize("N,nt,hb", G.B_CASES)
def test_case_b_fills_and_overflows_groups_of_one_variant(N, nt, hb):
    specs = G.case_b(N, nt, hb)
    groups, singles, units = G.plan(specs)
    assert len(specs) == N and all(G.variant(s) == (nt, hb) for s in specs)
    assert [len(jobs) for _, _, jobs in groups] == G.B_EXPECT[N]
    assert all((g[0], g[1]) == (nt, hb) for g in groups)
    assert singles == ([64] if N == 65 else [])                          # the 65th job: a second group of one, dissolved
    assert [j for _, _, jobs in groups for j in jobs] + singles == list(range(N))
    assert len(units) == len(groups) + len(singles)
    # inside the variant widths, depths, volumes and samplers vary, every seed is its own
    assert len({s.L for s in specs}) == 2 and len({s.F for s in specs}) == 4 and len({s.dims for s in specs}) == 5
    assert {s.sampler for s in specs} == {"full", "randompoint"} and len({s.seed for s in specs}) == N
    assert min(s.pop for s in specs) == 64 and max(s.pop for s in specs) == 512
    s0 = specs[0]
    assert (s0.sampler, s0.batch, s0.dims) == ("randompoint", 1, (4, 4, 4))
    # the table host (slot 0 of the first group) has the smallest workspace of its group
    ws = [_ws_bytes(specs[j]) for j in groups[0][2]]
    assert groups[0][2][0] == 0 and ws[0] == min(ws) and ws[0] < max(ws)
    wg = [G.workgroups(s) for s in specs]
    assert min(wg) == 1 and max(wg) >= 2
    for _, _, jobs in groups[1:]:                                        # later groups: slot and job index differ, and so do the rates found there
        assert any(G.base_lr(specs[j]) != G.base_lr(specs[slot]) for slot, j in enumerate(jobs)), jobs
    assert specs[63].log and (N < 65 or specs[64].log)                   # the jobs either side of the group boundary keep a loss log


def test_case_c_is_one_group_of_twelve_jobs_that_differ_in_everything_the_tables_carry():
    groups, singles, units = G.plan(G.C)
    assert groups == [(2, 3, list(range(12)))] and singles == [] and units == [("group", 0)]
    ws = [_ws_bytes(s) for s in G.C]
    assert ws[0] == max(ws) and ws.count(ws[0]) == 1                     # the table host is the LARGEST job (in B: the smallest)
    rev = G.C[::-1]
    assert G.plan(rev)[0] == [(2, 3, list(range(12)))] and _ws_bytes(rev[0]) < ws[0]      # reversed: another host
    fields = {"cin": lambda s: s.cin, "cout": lambda s: s.cout, "output_act": lambda s: s.output_act, "loss": lambda s: s.loss,
              "thr": lambda s: s.thr, "weighted": lambda s: s.weighted, "optimizer": lambda s: s.optimizer, "scheduler": lambda s: s.sched_name,
              "sampler": lambda s: s.sampler, "log": lambda s: s.log, "t0": lambda s: s.pre_steps}
    for name, get in fields.items():
        assert len({get(s) for s in G.C}) >= 2, name
        assert sum(get(a) != get(b) for a, b in zip(G.C, G.C[1:])) >= 6, name          # ... and between most neighbours
    assert {s.cout for s in G.C} == {1, 2, 3, 4} and {s.cin for s in G.C} == {2, 3}
    assert {s.optimizer for s in G.C} == {"Adamax", "Adam", "SGD"}
    assert {s.sched_name for s in G.C} == {"none", "MultiStepLR", "StepLR", "CyclicLR"}
    assert {s.sampler for s in G.C} == {"full", "randompoint", "replay"}
    assert {np.sign(s.thr) for s in G.C} == {-1.0, 0.0, 1.0} and set(range(5)) == {s.pre_steps for s in G.C}
    assert any(s.weighted and s.thr != 0 for s in G.C)                   # (thr acts on the weight map only)
    assert any(s.sched_name == "CyclicLR" and s.optimizer == "Adam" for s in G.C)      # beta1_table
    # the doubled milestone falls inside the run, at another call-local step (and in another call) for jobs with another t0
    steps = sum(G.C_STEPS)
    multi = [s for s in G.C if s.sched_name == "MultiStepLR"]
    ms = multi[0].scheduler["milestones"]
    assert ms.count(6) == 2
    local = {6 + 1 - s.pre_steps - 1 for s in multi}                      # optimizer step 7 is the first at the reduced rate
    assert len(local) >= 2 and all(0 < k < steps for k in local)
    assert any(k < G.C_STEPS[0] for k in local) and any(k >= G.C_STEPS[0] for k in local)
    # batches from one sample to five workgroup tiles plus one; workgroup counts differ and include 1 and 3
    wg = [G.workgroups(s) for s in G.C]
    assert min(s.batch for s in G.C) == 1 and max(s.batch for s in G.C) == 5 * 64 + 1
    assert len(set(wg)) > 1 and 1 in wg and max(wg) >= 3
    assert max(s.pop for s in G.C) <= 8 * 8 * 12 and len({s.seed for s in G.C}) == 12
    assert len({G.base_lr(s) for s in G.C}) == 3 and all(G.base_lr(a) != G.base_lr(b) for a, b in zip(G.C, G.C[1:]))


def test_case_d_is_one_group_whose_oracle_gradients_need_no_widened_band():
    groups, singles, _ = G.plan(G.D)
    assert groups == [(1, 3, list(range(8)))] and singles == []
    assert all(s.log and s.L <= 5 and s.pre_steps == 0 for s in G.D)
    assert {s.sampler for s in G.D} == {"full", "randompoint"} and {s.optimizer for s in G.D} == {"Adamax", "Adam", "SGD"}
    assert {s.loss for s in G.D} == {"datal2", "datasmoothl1"} and {s.weighted for s in G.D} == {False, True} and {s.cin for s in G.D} == {2, 3}
    wg = [G.workgroups(s) for s in G.D]
    assert 1 in wg and max(wg) >= 3
    for k, s in enumerate(G.D):
        # (randompoint: any fixed index set serves for this bound; the GPU test takes the batch the kernel draws)
        idx = None if s.sampler == "full" else np.random.default_rng(s.seed).integers(0, s.pop, size=s.batch)
        d, p, lo, g32, own = G.oracle_step1(s, idx)
        assert np.isfinite(lo) and lo > 0 and np.all(np.isfinite(g32)), str(s)
        print("D[%d] %s: oracle f32 <-> f64 gradient distance %.2e" % (k, s, own))
        assert 3.0 * own <= 1e-4, (str(s), own)


def test_case_e_is_one_group_of_three():
    groups, singles, _ = G.plan(G.E)
    assert groups == [(1, 3, [0, 1, 2])] and singles == []
