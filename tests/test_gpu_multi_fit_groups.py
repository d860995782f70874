"""brief_multi_fit's GROUPS of narrow nets (k_small_group + k_reduce_group: one launch pair per step for up to 64 jobs of one kernel variant),
at the sizes and mixtures a DivideTask partition produces: every variant at once, full and overflowing groups, jobs that differ in everything
the device table and the per-slot kernel arguments carry, a second call of a run (the tables are uploaded again while t0 > 0).

The reference of A, B, C and E is the SOLO fit of the same spec (Fitter.run, held to the oracle and the goldens by tests/test_gpu_parity.py):
every buffer of every job is compared bit for bit.  D is independent of the solo path: one grouped step against the CPU oracle, in the
project's plain bands (loss 1e-5 relative, every gradient tensor 1e-4 of its max-abs, neither widened) and with the optimizer update bit-exact.
The case lists live in tests/_groups.py; tests/test_multi_fit_groups_host.py proves that they form the groups each test is about."""
import ctypes as C

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib
from brief_pytorch_amd.fit import MultiFitter
from oracle import oracle as O

from . import _bands
from . import _groups as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUFFERS = ("params", "packed", "s1", "s2", "grads", "loss")


def _snap(f):
    """every buffer a fit step writes, copied"""
    m = f.m
    return {"params": m.params.clone(), "packed": m.packed.clone(), "s1": f.s1.clone(), "s2": f.s2.clone(), "grads": m.grads.clone(),
            "loss": m._loss.clone()}


def _cotrain(fitters, specs, k):
    """MultiFitter.run's one C-ABI call, with a loss log for the jobs whose spec asks for one only (MultiFitter.run logs all jobs or none: a
    group then never mixes loss_log and loss_out slots).  Returns the logs (None where none was kept)."""
    jobs, logs = zip(*(f.job(k, s.log) for f, s in zip(fitters, specs)))
    arr = (_lib.FitJob * len(jobs))(*jobs)
    _lib.check(_lib.lib().brief_multi_fit(arr, len(jobs), k, _lib.stream_ptr()))
    for f in fitters:
        f.t += k
    return [None if l is None else l[:k] for l in logs]


def _solo(specs, calls):
    """the reference: every spec fitted on its own, call by call.  Returns [(initial parameters, buffers after the run, loss logs per call)]"""
    out = []
    for s in specs:
        f = G.make(s, DEV)
        init = f.m.params.clone()
        logs = []
        for k in calls:
            r = f.run(k, log=s.log)
            logs.append(r.clone() if s.log else None)
        assert f.t == s.pre_steps + sum(calls)
        out.append((init, _snap(f), logs))
    torch.cuda.synchronize()
    return out


def _grouped(specs, calls):
    fitters = [G.make(s, DEV) for s in specs]
    logs = [_cotrain(fitters, specs, k) for k in calls]
    torch.cuda.synchronize()
    return fitters, [[None if call[i] is None else call[i].clone() for call in logs] for i in range(len(specs))]


def _assert_job(what, s, ref, f, logs):
    """one co-trained job against its solo fit: every buffer and the loss log bit for bit, finite, and moved from the initial parameters"""
    init, want, want_logs = ref
    got = _snap(f)
    for name in BUFFERS:
        assert torch.equal(got[name], want[name]), "%s: %s differs from the solo fit (%d of %d values; %s)" % (
            what, name, int((got[name] != want[name]).sum()), got[name].numel(), s)
    for c, (a, b) in enumerate(zip(logs, want_logs)):
        assert (a is None) == (b is None) == (not s.log), (what, str(s))
        if a is not None:
            assert torch.equal(a, b), "%s: loss log of call %d differs from the solo fit: %s against %s (%s)" % (what, c, a.tolist(), b.tolist(), s)
            assert bool(torch.isfinite(a).all()), (what, str(s))
    if s.log:
        assert torch.equal(got["loss"], logs[-1][-1:]), (what, str(s))          # the device loss is the last logged one
    assert all(bool(torch.isfinite(got[n]).all()) for n in BUFFERS), "%s: not finite (%s)" % (what, s)
    assert not torch.equal(got["params"], init), "%s: the parameters did not move (%s)" % (what, s)


# ---- A
def test_every_variant_interleaved_through_multifitter_equals_solo():
    """eight groups of five (one per kernel variant, dealt round-robin: no group is contiguous in the job array) and two single jobs between
    them on 10 units > 8 pool streams, through MultiFitter.run itself; 6 steps as 4 (logged) + 2: the second call uploads the tables again"""
    groups, singles, _ = G.plan(G.A)
    assert len(groups) == 8 and len(singles) == 2
    solo = []
    for s in G.A:
        f = G.make(s, DEV)
        init = f.m.params.clone()
        log = f.run(G.A_STEPS[0], log=True).clone()
        f.run(G.A_STEPS[1])
        solo.append((init, _snap(f), log))
    fitters = [G.make(s, DEV) for s in G.A]
    mf = MultiFitter(fitters)
    logs = [l.clone() for l in mf.run(G.A_STEPS[0], log=True)]
    mf.run(G.A_STEPS[1])
    torch.cuda.synchronize()
    for j, (s, f) in enumerate(zip(G.A, fitters)):
        what = "A job %d (%s)" % (j, "single" if j in singles else "variant nt=%d hb=%d" % G.variant(s))
        init, want, want_log = solo[j]
        got = _snap(f)
        assert f.t == sum(G.A_STEPS)
        for name in BUFFERS:
            assert torch.equal(got[name], want[name]), "%s: %s differs from the solo fit (%d of %d values; %s)" % (
                what, name, int((got[name] != want[name]).sum()), got[name].numel(), s)
        assert torch.equal(logs[j], want_log), "%s: loss log %s against %s (%s)" % (what, logs[j].tolist(), want_log.tolist(), s)
        assert all(bool(torch.isfinite(got[n]).all()) for n in BUFFERS) and bool(torch.isfinite(logs[j]).all()), "%s: not finite (%s)" % (what, s)
        assert not torch.equal(got["params"], init), "%s: the parameters did not move (%s)" % (what, s)


# ---- B
@pytest.mark.parametrize("N,nt,hb", G.B_CASES)
def test_full_and_overflowing_groups_equal_solo(N, nt, hb):
    """N = 64: one full group; 65: the 65th job opens a group of one, which is dissolved; 66: [64, 2]; 130: [64, 64, 2].  The table of the
    first group sits in the smallest workspace of the group (job 0: one sample).  4 steps as 3 + 1."""
    specs = G.case_b(N, nt, hb)
    groups, singles, _ = G.plan(specs)
    assert [len(g[2]) for g in groups] == G.B_EXPECT[N]
    solo = _solo(specs, G.B_STEPS)
    fitters, logs = _grouped(specs, G.B_STEPS)
    # the two sides of the first group's boundary first: the last slot of a full table, and what follows it
    _assert_job("B N=%d job 63 (slot 63 of the first group)" % N, specs[63], solo[63], fitters[63], logs[63])
    if N > 64:
        where = "a single job on a stream of its own" if 64 in singles else "slot 0 of the second group: it hosts that group's table"
        _assert_job("B N=%d job 64 (%s)" % (N, where), specs[64], solo[64], fitters[64], logs[64])
    for j in range(N):
        _assert_job("B N=%d job %d" % (N, j), specs[j], solo[j], fitters[j], logs[j])


# ---- C
@pytest.fixture(scope="module")
def solo_c():
    """the solo fits of case C, computed once and left unchanged"""
    return _solo(G.C, G.C_STEPS)


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_unlike_jobs_in_one_group_equal_solo(solo_c, order):
    """twelve jobs of one variant that differ in grid rank, channels, head sine, loss, thr, weight map, optimizer, schedule (milestones that
    fall at another call-local step per job, lr_table, beta1_table), sample source (idx_stride), batch (1 .. 321), t0 and loss log; 9 steps
    as 4 + 5.  Reversed, every job sits in another slot and another job's workspace hosts the table: nothing may change."""
    perm = list(range(len(G.C)))
    if order == "reversed":
        perm.reverse()
    specs = [G.C[j] for j in perm]
    assert [len(g[2]) for g in G.plan(specs)[0]] == [12]
    fitters, logs = _grouped(specs, G.C_STEPS)
    for slot, j in enumerate(perm):
        assert fitters[slot].t == G.C[j].pre_steps + sum(G.C_STEPS)
        _assert_job("C (%s) job %d in slot %d" % (order, j, slot), G.C[j], solo_c[j], fitters[slot], logs[slot])


# ---- D
def test_one_grouped_step_against_the_oracle():
    """an 8-job group, one step: loss within 1e-5 of the oracle's, every gradient tensor within 1e-4 of its max-abs (the plain band: the host
    file proves 3 x the oracle's own f32 <-> f64 distance stays below it for these nets), parameters and optimizer state equal to the
    oracle's optimizer applied to the GPU's gradients, bit for bit.  A randompoint job's batch is brief_sample_indices(pop, seed, 1)."""
    assert [len(g[2]) for g in G.plan(G.D)[0]] == [8]
    fitters = [G.make(s, DEV) for s in G.D]
    init = [f.m.params.cpu().numpy().copy() for f in fitters]
    logs = _cotrain(fitters, G.D, 1)
    torch.cuda.synchronize()
    for k, (s, f) in enumerate(zip(G.D, fitters)):
        what = "D job %d (%s)" % (k, s)
        idx = None
        if s.sampler == "randompoint":
            it = torch.empty(s.batch, dtype=torch.int64, device=DEV)
            _lib.check(_lib.lib().brief_sample_indices(_lib.ptr(it), s.batch, s.pop, s.seed, 1, _lib.stream_ptr()))
            idx = it.cpu().numpy()
            assert 0 <= idx.min() and idx.max() < s.pop
        d, p, lo, g32, own = G.oracle_step1(s, idx)
        assert np.array_equal(p, init[k]), what
        loss = float(logs[k][0])
        print("%s: loss %.6f (oracle %.6f)" % (what, loss, lo))
        assert abs(loss - lo) / abs(lo) < 1e-5, (what, loss, lo)
        assert float(f.m._loss) == loss, what
        grads = f.m.grads.cpu().numpy()
        dist = G.tensor_distances(d, grads, g32)
        print("%s: gradient distance %.2e (oracle f32 <-> f64: %.2e)" % (what, max(dist), own))
        _bands.record("grad", "grouped step L=%d F=%d cin=%d cout=%d" % (s.L, s.F, s.cin, s.cout), 1e-4, 1e-4, own, max(dist))
        assert max(dist) < 1e-4, (what, dist)
        lr, b1 = G.first_step_lr(s)
        s1, s2 = np.zeros_like(p), np.zeros_like(p)
        O.optim_step(s.optimizer, p, grads, s1, s2, lr, 1, b1=b1)
        assert np.array_equal(f.m.params.cpu().numpy(), p), what + ": parameters after the update"
        assert np.array_equal(f.s1.cpu().numpy(), s1) and np.array_equal(f.s2.cpu().numpy(), s2), what + ": optimizer state"
        assert not np.array_equal(p, init[k]), what


# ---- E
def test_a_refusal_inside_a_group_leaves_every_job_untouched():
    """the middle job of a 3-job group arrives with a workspace four bytes short: brief_multi_fit returns BRIEF_ERR_WORKSPACE before any step
    is launched, no job's buffers change, and the same three fitters then train as they would alone; 4097 jobs are refused by name"""
    assert [len(g[2]) for g in G.plan(G.E)[0]] == [3]
    solo = _solo(G.E, (G.E_STEPS,))
    fitters = [G.make(s, DEV) for s in G.E]
    jobs = [f.job(G.E_STEPS)[0] for f in fitters]
    arr = (_lib.FitJob * 3)(*jobs)
    for j, f in zip(jobs, fitters):
        need = _lib.lib().brief_train_workspace_bytes(C.byref(f.m.desc), f.n)
        assert j.workspace_bytes == need                                   # (the modules allocate exactly what the library asks for)
    arr[1].workspace_bytes -= 4
    torch.cuda.synchronize()
    before = [_snap(f) for f in fitters]
    rc = _lib.lib().brief_multi_fit(arr, 3, G.E_STEPS, _lib.stream_ptr())
    msg = _lib.lib().brief_last_error()
    torch.cuda.synchronize()
    assert rc == -3 and msg == b"workspace too small", (rc, msg)           # BRIEF_ERR_WORKSPACE (include/brief_hip.h)
    for k, (f, b) in enumerate(zip(fitters, before)):
        now = _snap(f)
        for name in BUFFERS:
            assert torch.equal(now[name], b[name]), "job %d: %s changed by a refused call" % (k, name)
    many = (_lib.FitJob * 4097)(*([jobs[0]] * 4097))
    rc = _lib.lib().brief_multi_fit(many, 4097, 1, _lib.stream_ptr())
    assert rc == -1 and b"too many jobs" in _lib.lib().brief_last_error()
    MultiFitter(fitters).run(G.E_STEPS)
    torch.cuda.synchronize()
    for k, (s, f) in enumerate(zip(G.E, fitters)):
        _assert_job("E job %d" % k, s, solo[k], f, [None])
