"""Job specs for the tests of brief_multi_fit's GROUPS (tests/test_multi_fit_groups_host.py without a GPU, tests/test_gpu_multi_fit_groups.py
on one), and the grouping rule itself, restated.

A narrow net (fp32, at most 64 features, at most 7 hidden layers: use_small) has no launches of its own inside brief_multi_fit: the jobs of one
kernel variant (nt, hb) are packed into groups of up to BRIEF_GROUP_MAX = 64 and a group is trained by one k_small_group + one k_reduce_group
launch per step.  plan() restates how csrc/brief_hip.hip assigns jobs to groups, single launches and pool streams, workgroups() restates
small_grid; the host file asserts with them that every case list below has the structure its GPU test is about, so that no case goes vacuous
when a rule changes.

The case lists are module-level data: both files see the same specs.
    A   every variant, interleaved: 40 narrow jobs round-robin over the eight variants + two nets that are not narrow
    B   full and overflowing groups of one variant: case_b(N, nt, hb)
    C   twelve unlike jobs in one group: everything the device table and the per-slot kernel arguments carry differs between neighbours
    D   eight jobs, one step: checked against the CPU oracle, independent of the solo path
    E   three jobs: the middle one is handed over with a workspace that is too small"""
import collections

import numpy as np
import torch

from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.networks import SIREN

GROUP_MAX = 64           # BRIEF_GROUP_MAX (csrc/brief_small.inc)
POOL_STREAMS = 8         # kPoolStreams (csrc/brief_hip.hip)
CUS = 256                # kCUs
LR = 1e-3
W0 = 20.0


def base_lr(s):
    """the job's learning rate: three values dealt by the seed, so that neighbours in a job array and in a group differ (a rate looked up
    under another job's index must not go unnoticed)"""
    return LR * (1.0, 0.5, 2.0)[s.seed % 3]

_FIELDS = ("L", "F", "cin", "cout", "output_act", "dims", "sampler", "n", "optimizer", "scheduler", "loss", "thr", "beta", "weighted", "seed",
           "pre_steps", "log")


class Spec(collections.namedtuple("Spec", _FIELDS)):
    """one fit job.  sampler: "full" | "randompoint" | "replay"; n: the batch (ignored for "full": the whole volume); scheduler: None or the
    dict Fitter takes; pre_steps: optimizer steps the fitter has behind it when it is handed out (its t0)"""
    __slots__ = ()

    @property
    def pop(self):
        return int(np.prod(self.dims))

    @property
    def batch(self):
        return self.pop if self.sampler == "full" else int(self.n)

    @property
    def sched_name(self):
        return (self.scheduler or {}).get("name", "none")

    def __str__(self):
        return "%dx%d cin=%d cout=%d oa=%d dims=%s %s n=%d %s %s %s thr=%g w=%d seed=%d t0=%d log=%d" % (
            self.L, self.F, self.cin, self.cout, self.output_act, "x".join(str(v) for v in self.dims), self.sampler, self.batch, self.optimizer,
            self.sched_name, self.loss, self.thr, self.weighted, self.seed, self.pre_steps, self.log)


def spec(L, F, dims, sampler="full", n=0, seed=0, cout=1, output_act=False, optimizer="Adamax", scheduler=None, loss="datal2", thr=0.0,
         beta=0.01, weighted=False, pre_steps=0, log=False):
    return Spec(L, F, len(dims), cout, bool(output_act), tuple(dims), sampler, int(n), optimizer, scheduler, loss, float(thr), float(beta),
                bool(weighted), int(seed), int(pre_steps), bool(log))


# ---- building a job
def host_parts(s):
    """(net on the CPU, targets [pop, cout], weight map [pop, cout] in {0.25, 1} or None): seeded by the spec alone"""
    torch.manual_seed(s.seed)
    m = SIREN(coords_channel=s.cin, data_channel=s.cout, features=s.F, layers=s.L, w0=W0, output_act=s.output_act)
    tv = torch.rand(s.pop, s.cout, generator=torch.Generator().manual_seed(s.seed + 1)) * 100
    w = None
    if s.weighted:
        u = torch.rand(s.pop, s.cout, generator=torch.Generator().manual_seed(s.seed + 2))
        w = torch.where(u < 0.5, torch.tensor(0.25), torch.tensor(1.0)).contiguous()
    return m, tv.contiguous(), w


def make(s, device):
    """the spec's Fitter on `device`, its pre_steps behind it.  Two builds of one spec are the same job, bit for bit: a "replay" job draws
    its index sets from a generator of its own, seeded by the spec."""
    m, tv, w = host_parts(s)
    m.to(device)
    stream = None
    if s.sampler == "replay":
        gen = torch.Generator().manual_seed(s.seed + 3)
        stream = lambda t: torch.randint(0, s.pop, (s.batch,), generator=gen).to(device)      # noqa: E731 (one draw per step, in step order)
    f = Fitter(m, tv.to(device), s.dims, weights=None if w is None else w.to(device), sampler="full" if s.sampler == "full" else "randompoint",
               sample_size=s.batch, optimizer=s.optimizer, lr=base_lr(s), scheduler=s.scheduler, loss=s.loss, thr=s.thr, beta=s.beta, seed=s.seed,
               index_stream=stream)
    if s.pre_steps:
        f.run(s.pre_steps)
    return f


def first_step_lr(s):
    """(lr, beta1) of optimizer step 1, from the schedule's definition (torch: CyclicLR starts at base_lr with the momentum at its maximum)"""
    if s.sched_name == "CyclicLR":
        return float(s.scheduler["base_lr"]), float(s.scheduler.get("max_momentum", 0.9)) if s.optimizer != "SGD" else 0.9
    return base_lr(s), 0.9


# ---- the dispatch and the grouping rule, restated
def variant(s):
    """(nt, hb) of a narrow net, None for every other one.
    csrc/brief_layout.h brief_nt: 32-feature tiles; csrc/brief_hip.hip use_small: fp32, nt <= 2, layers - 2 <= 7; small_hb: hidden layers in buckets
    of 1, 3, 5, 7"""
    nt, h = (s.F + 31) // 32, s.L - 2
    if nt > 2 or h > 7:
        return None
    return nt, (1 if h <= 1 else (3 if h <= 3 else (5 if h <= 5 else 7)))


def workgroups(s):
    """small_grid (csrc/brief_hip.hip): workgroups (= gradient slabs) of a narrow job's k_small launch, and its share of a k_small_group launch.
    brief_wg_samples (csrc/brief_layout.h): 32 x (4 / nt) samples per workgroup tile; small_wpe (csrc/brief_small.inc): 2 resident workgroups
    per CU up to hb = 3, else 1; at least two rounds"""
    nt, hb = variant(s)
    wg_samples = 32 * (4 // nt)
    tiles = max(1, -(-s.batch // wg_samples))
    cap = CUS * (2 if hb <= 3 else 1)
    rounds = max(2, -(-tiles // cap))
    return -(-tiles // rounds)


def plan(specs):
    """brief_multi_fit's unit assignment (csrc/brief_hip.hip, the loop `for (int j = 0; j < njobs; ++j)` over use_small / brief_nt / small_hb
    and the two loops behind it):
      * a narrow job joins the NEWEST group of its variant, or opens a new one when that group is full (the search stops at the newest);
      * a group left with one job is dissolved: the job gets plain launches;
      * stream slots: the live groups in the order they were opened, then the single jobs in job order; unit u runs on pool stream
        u mod min(units, 8).
    Returns (groups: [(nt, hb, [job indices])], singles: [job indices], units: [("group", position in groups) | ("single", job)] in slot order)"""
    opened = []
    for j, s in enumerate(specs):
        v = variant(s)
        if v is None:
            continue
        gi = None
        for q in range(len(opened) - 1, -1, -1):
            if opened[q][0] == v:
                if len(opened[q][1]) < GROUP_MAX:
                    gi = q
                break
        if gi is None:
            opened.append((v, []))
            gi = len(opened) - 1
        opened[gi][1].append(j)
    groups = [(v[0], v[1], jobs) for v, jobs in opened if len(jobs) > 1]
    grouped = {j for _, _, jobs in groups for j in jobs}
    singles = [j for j in range(len(specs)) if j not in grouped]
    units = [("group", q) for q in range(len(groups))] + [("single", j) for j in singles]
    return groups, singles, units


def stream_of(units, u):
    return u % min(len(units), POOL_STREAMS)


# ---- A: every variant, interleaved
A_STEPS = (4, 2)
_A_L = {1: (2, 3), 3: (4, 5), 5: (6, 7), 7: (8, 9)}
_A_F = {1: (1, 22, 32), 2: (33, 50, 64)}
_A_DIMS = [(4, 4, 4), (5, 7, 9), (8, 8, 8), (4, 6, 8), (8, 8, 12)]
_A_N = [1, 33, 300, 700]
A_VARIANTS = [(nt, hb) for nt in (1, 2) for hb in (1, 3, 5, 7)]


def _case_a():
    out = []
    for k in range(40):
        nt, hb = A_VARIANTS[k % 8]
        r = k // 8                                                   # the variant's r-th job
        rand = (k + r) % 2 == 1
        out.append(spec(_A_L[hb][(r + nt) % 2], _A_F[nt][(r + hb // 2) % 3], _A_DIMS[(k + 2 * r) % 5], "randompoint" if rand else "full",
                        _A_N[(k // 2 + r) % 4] if rand else 0, seed=1000 + k))
    # two nets that are not narrow, in between: three feature tiles, and one tile but eight hidden layers (the general path: k_fused<1> + k_wgrad<1>)
    out.insert(13, spec(4, 96, (8, 8, 8), "full", seed=1100))
    out.insert(27, spec(10, 24, (4, 6, 8), "randompoint", 300, seed=1101))
    return out


A = _case_a()


# ---- B: full and overflowing groups of one variant
B_STEPS = (3, 1)
B_CASES = [(64, 1, 3), (65, 1, 3), (66, 1, 3), (130, 1, 3), (64, 2, 7)]      # (N, nt, hb)
B_EXPECT = {64: [64], 65: [64], 66: [64, 2], 130: [64, 64, 2]}               # group sizes; N = 65 leaves one demoted single
_B_DIMS = [(4, 4, 4), (8, 8, 8), (4, 6, 8), (5, 7, 9), (6, 6, 6)]


def case_b(N, nt, hb):
    """N jobs of variant (nt, hb); widths and depths vary inside the variant; job 0 is a one-sample randompoint fit on a 4^3 volume (the smallest
    workspace of its group hosts the group's table)"""
    Ls, Fs = _A_L[hb], {1: (5, 16, 22, 32), 2: (33, 40, 56, 64)}[nt]
    out = [spec(Ls[0], Fs[1], (4, 4, 4), "randompoint", 1, seed=2000 + 1000 * nt)]
    for k in range(1, N):
        rand = k % 3 == 1
        out.append(spec(Ls[k % 2], Fs[(k // 2) % 4], _B_DIMS[k % 5], "randompoint" if rand else "full", (1, 33, 130, 300, 64)[(k // 3) % 5] if rand else 0,
                        seed=2000 + 1000 * nt + k, log=k % 16 == 0 or k in (63, 64)))
    return out


# ---- C: unlike jobs in one group (variant nt = 2, hb = 3: two feature tiles, 64 samples per workgroup tile)
C_STEPS = (4, 5)
_CYC = {"name": "CyclicLR", "base_lr": 1e-4, "max_lr": 2e-3, "step_size_up": 3, "step_size_down": 2, "mode": "triangular2"}
_MULTI = {"name": "MultiStepLR", "milestones": [6, 6, 9], "gamma": 0.5}      # step 7 runs with a quarter of the rate: call-local step 7 - t0 - 1
_STEP = {"name": "StepLR", "step_size": 4, "gamma": 0.5}
C = [
    spec(5, 64, (8, 8, 12), "randompoint", 321, 3000, log=True),                                                              # five tiles + one sample, the deepest: the largest workspace
    spec(4, 33, (8, 8), "full", 0, 3001, cout=3, output_act=True, optimizer="Adam", scheduler=_CYC, loss="datasmoothl1", thr=0.01, weighted=True, pre_steps=2),
    spec(5, 50, (4, 4, 4), "replay", 1, 3002, cout=2, optimizer="SGD", scheduler=_MULTI, thr=-0.01, pre_steps=1, log=True),
    spec(4, 64, (6, 10), "randompoint", 33, 3003, cout=4, scheduler=_STEP, loss="datasmoothl1", beta=0.5, weighted=True, pre_steps=3),
    spec(4, 40, (5, 7, 9), "full", 0, 3004, output_act=True, optimizer="Adam", thr=0.01, weighted=True, pre_steps=4, log=True),
    spec(5, 57, (8, 8, 8), "randompoint", 129, 3005, cout=2, scheduler=_MULTI, loss="datasmoothl1", thr=-0.01, pre_steps=4),
    spec(4, 48, (16, 12), "replay", 200, 3006, cout=3, output_act=True, optimizer="SGD", scheduler=_STEP, weighted=True, log=True),
    spec(5, 35, (4, 6, 8), "full", 0, 3007, cout=4, optimizer="Adam", scheduler=_CYC, loss="datasmoothl1", thr=0.01, pre_steps=2),
    spec(4, 64, (8, 8, 12), "replay", 321, 3008, scheduler=_MULTI, thr=-0.01, weighted=True, pre_steps=1, log=True),
    spec(5, 44, (7, 9), "full", 0, 3009, cout=2, output_act=True, optimizer="Adam", scheduler=_STEP, loss="datasmoothl1", beta=0.5, pre_steps=3),
    spec(4, 52, (8, 8, 8), "randompoint", 64, 3010, cout=3, optimizer="SGD", thr=0.01, weighted=True, log=True),
    spec(5, 61, (6, 6, 6), "randompoint", 250, 3011, cout=4, output_act=True, scheduler=_CYC, loss="datasmoothl1", thr=-0.01, weighted=True),
]


# ---- D: one grouped step against the oracle (variant nt = 1, hb = 3; shallow: the oracle's own f32 <-> f64 distance stays a third of the band)
D = [
    spec(4, 22, (8, 8, 8), "full", 0, 4000, log=True),
    spec(5, 32, (6, 10), "full", 0, 4001, cout=3, optimizer="Adam", loss="datasmoothl1", weighted=True, log=True),
    spec(4, 16, (8, 8, 12), "randompoint", 300, 4002, cout=2, output_act=True, optimizer="SGD", thr=0.01, weighted=True, log=True),
    spec(4, 5, (4, 4, 4), "randompoint", 1, 4003, log=True),
    spec(5, 27, (5, 7, 9), "full", 0, 4004, cout=4, optimizer="Adam", scheduler=_CYC, thr=-0.01, weighted=True, log=True),
    spec(4, 32, (16, 12), "randompoint", 129, 4005, loss="datasmoothl1", beta=0.5, log=True),
    spec(5, 11, (4, 6, 8), "full", 0, 4006, cout=2, optimizer="SGD", log=True),
    spec(4, 30, (8, 8, 8), "randompoint", 700, 4007, cout=3, weighted=True, thr=0.01, log=True),
]


def oracle_step1(s, idx=None):
    """the oracle's answer for the job's first batch on the spec's initial parameters: (desc, params, loss, grads f32, own) with own = the
    largest distance, over the net's tensors and relative to a tensor's max-abs, between the oracle's f32 and f64 gradients.
    idx: the batch's indices (None: the whole volume in order)"""
    from oracle import oracle as O
    m, tv, w = host_parts(s)
    d = O.make_desc(s.cin, s.cout, s.L, s.F, W0, 30.0, s.output_act)
    p = m.params.numpy().copy()
    x = O.grid_coords(s.dims, idx=idx)
    sel = slice(None) if idx is None else np.asarray(idx)
    y = tv.numpy()[sel]
    ww = None if w is None else w.numpy()[sel]
    kind = {"datal2": 0, "datasmoothl1": 1}[s.loss]
    lo, g32, _, _ = O.loss_grad(d, p, x, y, ww, kind, s.thr, s.beta)
    _, g64, _, _ = O.loss_grad(d, p, x, y, ww, kind, s.thr, s.beta, f64=True)
    own = max(tensor_distances(d, g32, g64))
    return d, p, lo, g32, own


def tensor_distances(d, got, ref):
    """max |got - ref| / max |ref| of every weight and bias tensor of the net, in buffer order"""
    from oracle import oracle as O
    gw, gb = O.unpack_params(d, np.asarray(got))
    rw, rb = O.unpack_params(d, np.asarray(ref))
    out = []
    for l in range(d.layers):
        for a, b in ((gw[l], rw[l]), (gb[l], rb[l])):
            a, b = a.astype(np.float64), b.astype(np.float64)
            out.append(float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30)))
    return out


# ---- E: a refusal inside a group
E_STEPS = 3
E = [spec(4, 22, (8, 8, 8), "full", 0, 5000), spec(5, 30, (4, 6, 8), "randompoint", 130, 5001, cout=2, weighted=True),
     spec(4, 9, (5, 7, 9), "full", 0, 5002, optimizer="Adam")]
