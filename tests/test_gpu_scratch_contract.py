"""No result of a train, fit or decode entry depends on what its caller-owned scratch held on entry (include/brief_hip.h, "Scratch").

There is no device memset on the training path: every kernel has to write every byte a later kernel reads — the stash columns of the
samples between n and npad, the zero rows between F and FP, the slabs of every K split, the records of every workgroup, the bvals span
of a family's gradients.  The Python layer allocates all of that with torch.empty and reuses it, and in a test process torch.empty
returns fresh pages or finite floats, so a kernel that reads stale scratch passes every oracle parity.  Here every such buffer is a
window of exactly the size the library asks for between two guards (tests/_scratch.py), filled with zeros (the baseline), with 0xFF
bytes (NaN) and with seeded floats in [-1, 1] (a stale batch).

The assertion is the same everywhere: the results under NAN and under STALE equal those under ZERO bit for bit (every kernel is
bit-reproducible: tests/test_gpu_parity.py, tests/test_gpu_wgrad_feed.py), the baseline is finite, and every guard still holds its
pattern, which pins the size functions against what the kernels really write.  No band, no new number.

    a  a train step of every row of tests/_variants.py                       e  a big batch, then a small one, on one module
    b  the k_wgrad layouts and the LDS-DMA feed of k_wgrad<8>                f  fit loops, and one brief_multi_fit group
    c  the tail plans (side stream)                                          g  repack, decode, derivative decode, fake quantisation
    d  the ragged tiles of the bf16 step
The table of cases and what they found: profiles/r24_scratch_contract.md."""
import numpy as np
import pytest
import torch

from brief_pytorch_amd.fit import Fitter, MultiFitter
from brief_pytorch_amd.networks import SIREN

from . import _groups as G
from . import _scratch as S
from . import _variants as V

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _siren(L, F, cout=1, precision="fp32", seed=None):
    """make(): the seeded net on the device, the same one at every call"""
    def make():
        torch.manual_seed(L * 1000 + F if seed is None else seed)
        return SIREN(coords_channel=3, data_channel=cout, features=F, layers=L, w0=20, precision=precision).to(DEV)
    return make


def _step_under(make, n, fill, batch, thr):
    """one train step of a fresh net with workspace, gradients, loss and fragment copy seated under `fill`"""
    m = make()
    x, y, w = batch
    seated = S.seat_train(m, n, fill)
    # train_step allocates yhat itself: the entry is handed a guarded, filled one in its place (n * cout floats, no more)
    yhat = seated.new("yhat", 4 * n * m.data_channel).view(n, m.data_channel)
    entry = m._abi_train_step
    m._abi_train_step = lambda g, b, kind, thr_, beta, _yhat: entry(g, b, kind, thr_, beta, yhat)
    loss, own = m.train_step(n, y, coords=x, weights=w, thr=thr, want_yhat=True)
    assert own.shape == yhat.shape
    seated.check("train step, n = %d, %s" % (n, fill))
    assert loss.data_ptr() == seated.parts["loss"].f32.data_ptr() and m.grads.data_ptr() == seated.parts["grads"].f32.data_ptr()
    assert m._ws.data_ptr() == seated.parts["workspace"].f32.data_ptr() and m.packed.data_ptr() == seated.parts["packed"].f32.data_ptr()
    return {"loss": loss.clone(), "grads": m.grads.clone(), "yhat": yhat.clone(), "packed": m.packed.clone()}


def _train_step_case(make, n, cin, cout, output_act, what):
    """the step under the three fills: explicit coordinates, a weight map, thr = 30 (0.3 with a sine head), yhat wanted"""
    rng = np.random.default_rng(n * 31 + cin + cout)
    batch = tuple(_dev(a) for a in S.rand_batch(rng, n, cin, cout, 1.0 if output_act else 100.0))
    thr = 0.3 if output_act else 30.0
    base = S.assert_fills_agree(lambda fill: _step_under(make, n, fill, batch, thr), "%s, n = %d" % (what, n))
    assert base["yhat"].shape == (n, cout) and float(base["grads"].abs().max()) > 0
    return base


# ---- a: every kernel row
@pytest.mark.parametrize("n", [1, 33, 700])
@pytest.mark.parametrize("v", V.VARIANTS, ids=[v.label for v in V.VARIANTS])
def test_train_step_of_every_kernel_row(v, n):
    """k_small, k_fused<4 / 8>, k_lean, k_wide, k16, k_fused_x3 and the families; for FFN the bvals span of the gradient buffer is
    part of the compared buffer and is written as zeros"""
    base = _train_step_case(lambda: v.make(DEV), n, v.cin, v.cout, v.output_act, v.id)
    if v.id == "ffn":
        m = v.make()
        assert m.bv_count > 0 and not base["grads"][:m.bv_count].any()


# ---- b: the k_wgrad layouts and the DMA feed
FEED_N = [1, 32, 33, 64, 96, 2720, 2752]      # tests/test_gpu_wgrad_feed.py: the prologue alone .. K splits of one and two chunks side by side
B_CASES = [(L, F, n) for F in (256, 225) for L in (3, 5) for n in FEED_N]
# 96: LIST 3, 160: LIST 5, 200: HET7, 300: two left-over tiles, 384: 12 tiles, 527: 6 per side and two k-slices, 1100: k_wide
B_CASES += [(L, F, n) for F in (96, 160, 200, 300, 384, 527, 1100) for L in (3, 5) for n in (33, 700)]
B_CASES += [(10, 24, 130), (11, 48, 130)]      # k_fused<1 / 2> TRAIN (eight and nine hidden layers: not k_small): 128- and 64-sample workgroups


@pytest.mark.parametrize("L,F,n", B_CASES, ids=["%dx%d-n%d" % c for c in B_CASES])
def test_train_step_of_the_wgrad_layouts(L, F, n):
    _train_step_case(_siren(L, F), n, 3, 1, False, "SIREN %dx%d" % (L, F))


# ---- c: the tail plans
C_CASES = [(1100, 9000, 1), (512, 19457, 2), (768, 12801, 2)]


@pytest.mark.parametrize("F,n,mode", C_CASES, ids=["F%d-n%d-mode%d" % c for c in C_CASES])
def test_train_step_under_the_tail_plans(F, n, mode):
    """fused_tail_plan (csrc/brief_hip.hip) on 256 CUs, three layers (one hidden layer), derived from the code (tests/_scratch.py tail_plan):
      F = 1100, n = 9000    mode 1: k_wide, 282 tiles = one round of 256 + 26; the body's chunks in 30 K splits on the side stream, the
                            tail's 26 chunks as split 31 behind the tail launch
      F = 512               n = 18000 (563 tiles = 512 + 51, two workgroups per CU) takes NO plan: the uneven form needs short splits of
                            at least 4 chunks and gets (563 + 14 x 9.2) / 64 - 9.2 = 1.6; mode 1 is k_wide's alone.  The nearest batch
                            that takes one is n = 19457: 609 tiles = 512 + 97, the last with one sample; 38 normal splits of 13.25 chunks on
                            the side stream, 26 short ones of 4.05 behind the tail: mode 2
      F = 768               n = 9000 (282 tiles = 256 + 26, one workgroup per CU) takes none either (k_short < 0); the nearest that does is
                            n = 12801: 401 tiles = 256 + 145, the last with one sample; 8 normal splits of 27.8 chunks, 20 short ones of 8.9: mode 2
    (four layers change the numbers, not the outcome: neither n = 18000 at 512 nor n = 9000 at 768 takes a plan.)"""
    assert S.tail_plan(F, 3, n, S.cu_count()) == mode, "the device has %d CUs: this shape takes another plan there" % S.cu_count()
    _train_step_case(_siren(3, F), n, 3, 1, False, "SIREN 3x%d" % F)


def test_the_tail_plan_restatement_on_256_cus():
    """(needs no scratch: what the docstring above says, on the restated rule)"""
    assert [S.tail_plan(F, 3, n) for F, n, _ in C_CASES] == [1, 2, 2]
    assert S.tail_plan(512, 3, 18000) == 0 and S.tail_plan(768, 3, 9000) == 0 and S.tail_plan(512, 4, 18000) == 0 and S.tail_plan(768, 4, 9000) == 0
    assert S.tail_plan(512, 3, 19456) == 0 and S.tail_plan(768, 3, 12800) == 0      # (one tile fewer: no plan)


# ---- d: bf16 ragged tiles
@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("F,cout", [(96, 1), (96, 3), (300, 1)])
def test_train_step_of_the_bf16_ragged_tiles(F, cout, n):
    """128-sample tiles and the quarter / half-tile tails of split16 (cout = 1), the NS = 4 kernels (cout = 3), 8 and 16 padded tiles"""
    _train_step_case(_siren(4, F, cout, "bf16"), n, 3, cout, False, "bf16 SIREN 4x%d cout %d" % (F, cout))


# ---- e: a big batch, then a small one, on one module
E_NETS = {"k_fused_8": _siren(5, 256), "k_lean": _siren(4, 300), "k_small": _siren(4, 22), "bf16": _siren(4, 96, 1, "bf16"),
          "ffn": lambda: V.BY_ID["ffn"].make(DEV)}


@pytest.mark.parametrize("name", list(E_NETS))
def test_small_batch_behind_a_big_one(name):
    """the production form: a workspace larger than the step needs and full of the earlier batch.  n = 2752 and then n = 33 on one module, no
    attribute touched in between, against the n = 33 step of a freshly built identical module on zeroed scratch"""
    make = E_NETS[name]
    m = make()
    cin, cout = m.coords_channel, m.data_channel
    rng = np.random.default_rng(5)
    big, small = (tuple(_dev(a) for a in S.rand_batch(rng, n, cin, cout)) for n in (2752, 33))
    m.train_step(2752, big[1], coords=big[0], weights=big[2], thr=30.0, want_yhat=True)
    ws = m._ws
    loss, yhat = m.train_step(33, small[1], coords=small[0], weights=small[2], thr=30.0, want_yhat=True)
    assert m._ws is ws and ws.numel() * 4 > m._abi_train_ws_bytes(33)
    got = {"loss": loss.clone(), "grads": m.grads.clone(), "yhat": yhat.clone(), "packed": m.packed.clone()}
    want = _step_under(make, 33, "ZERO", small, 30.0)
    S.assert_finite(want, name)
    S.assert_same(got, want, "%s: n = 33 behind n = 2752" % name)


# ---- f: fit loops
def _fit_under(make, dims, sample_size, fill):
    m = make()
    pop = int(np.prod(dims))
    gen = torch.Generator().manual_seed(pop)
    tv = (torch.rand(pop, m.data_channel, generator=gen) * 100).to(DEV)
    f = Fitter(m, tv, dims, sampler="randompoint", sample_size=sample_size, seed=9)
    seated = S.seat_train(m, sample_size, fill)
    log = f.run(3, log=True)
    seated.check("fit, %s" % fill)
    assert m._ws.data_ptr() == seated.parts["workspace"].f32.data_ptr() and m.packed.data_ptr() == seated.parts["packed"].f32.data_ptr()
    return {"params": m.params.clone(), "packed": m.packed.clone(), "state1": f.s1.clone(), "state2": f.s2.clone(), "loss log": log.clone(),
            "loss": m._loss.clone(), "grads": m.grads.clone()}


F_CASES = {"5x256": (_siren(5, 256), (16, 16, 16), 2752), "4x22": (_siren(4, 22), (8, 8, 12), 321),
           "ffn": (lambda: V.BY_ID["ffn"].make(DEV), (31, 37), 700), "bf16": (_siren(4, 96, 1, "bf16"), (8, 8, 12), 300)}


@pytest.mark.parametrize("name", list(F_CASES))
def test_fit_loop(name):
    """Fitter.run(3) with in-kernel sampling: the fused update and the repack behind every step read the same scratch"""
    make, dims, n = F_CASES[name]
    init = make().params.clone()
    base = S.assert_fills_agree(lambda fill: _fit_under(make, dims, n, fill), "fit %s" % name)
    assert base["loss log"].shape == (3,) and not torch.equal(base["params"], init)


def _group_under(fill):
    fitters = [G.make(s, DEV) for s in G.E]
    seated = [S.seat_train(f.m, f.n, fill) for f in fitters]
    logs = MultiFitter(fitters).run(3, log=True)
    for j, sd in enumerate(seated):
        sd.check("group job %d, %s" % (j, fill))
    out = {}
    for j, (f, log) in enumerate(zip(fitters, logs)):
        for name, t in (("params", f.m.params), ("packed", f.m.packed), ("state1", f.s1), ("state2", f.s2), ("loss log", log), ("loss", f.m._loss),
                        ("grads", f.m.grads)):
            out["job %d %s" % (j, name)] = t.clone()
    return out


def test_multi_fit_group():
    """three narrow jobs of one variant are one k_small_group: every job's workspace is filled, and the first one's also hosts the group's
    device table (behind its slabs, inside brief_train_workspace_bytes: its guard holds)"""
    groups, singles, _ = G.plan(G.E)
    assert [len(g[2]) for g in groups] == [3] and not singles
    S.assert_fills_agree(_group_under, "brief_multi_fit group")


# ---- g: repack and decode
@pytest.mark.parametrize("v", V.VARIANTS, ids=[v.label for v in V.VARIANTS])
def test_repack_writes_all_of_packed(v):
    """the fragment copy filled before the module's first repack: the whole copy, padding included, and a forward pass over 257 coordinates"""
    x = _dev(np.random.default_rng(v.seed).uniform(-1, 1, size=(257, v.cin)).astype(np.float32))

    def run(fill):
        m = v.make(DEV)
        seated = S.seat_packed(m, fill)
        y = m.forward(x)
        seated.check("%s repack, %s" % (v.id, fill))
        assert not m._stale and m.packed.data_ptr() == seated.parts["packed"].f32.data_ptr()
        return {"packed": m.packed.clone(), "forward": y.clone()}

    S.assert_fills_agree(run, "%s repack + forward" % v.id)


def test_wide_decode_scratch():
    """above 1024 features the activations of a decode travel through caller scratch: two ping-pong planes per workgroup"""
    dims = (9, 13, 17)

    def run(fill):
        m = _siren(3, 1100)()
        seated = S.seat_forward(m, int(np.prod(dims)), fill, S.seat_packed(m, fill))
        y = m.decode_grid(dims)
        seated.check("k_wide decode, %s" % fill)
        assert m._fws.data_ptr() == seated.parts["forward scratch"].f32.data_ptr()
        return {"decode": y.clone()}

    S.assert_fills_agree(run, "decode_grid of a 3x1100 net")


@pytest.mark.parametrize("L,F", [(4, 40), (3, 527)])
def test_derivative_decode_fragment_copy(L, F):
    """the Jacobian / Hessian kernels' own fragment copy, written anew at the head of every call"""
    x = _dev(np.random.default_rng(F).uniform(-1, 1, size=(257, 3)).astype(np.float32))

    def run(fill):
        m = _siren(L, F)()
        seated = S.seat_jac(m, fill)
        value, jac = m.spatial_gradient(x)
        first = m._jac_packed.clone()
        v2, j2, hess = m.spatial_hessian(x)
        seated.check("derivative decode, %s" % fill)
        assert m._jac_packed.data_ptr() == seated.parts["jac packed"].f32.data_ptr()
        return {"value": value.clone(), "jac": jac.clone(), "jac packed": first, "hessian value": v2.clone(), "hessian jac": j2.clone(),
                "hess": hess.clone()}

    S.assert_fills_agree(run, "spatial_gradient + spatial_hessian of a %dx%d net" % (L, F))


def test_fake_quantise_scratch():
    """brief_quant_ranges + brief_quant_apply of the F = 67 net: the range kernel's workspace, the ranges and the result filled"""
    def run(fill):
        m = _siren(5, 67)()
        seated = S.seat_quant(m, fill)
        q = m.fake_quantise(8)
        seated.check("fake_quantise, %s" % fill)
        assert q.data_ptr() == seated.parts["qparams"].f32.data_ptr() and m._qws.data_ptr() == seated.parts["quant workspace"].f32.data_ptr()
        return {"qparams": q.clone(), "lo_step": m._qlo_step.clone()}

    base = S.assert_fills_agree(run, "fake_quantise(8)")
    assert not torch.equal(base["qparams"], _siren(5, 67)().params)
