"""The quantiser's kernels (csrc/brief_quant.inc) against numpy bit for bit, the C-ABI refusals, and the quantised training step
(Fitter.run_quantised): its gradients are those of a net holding the fake-quantised weights, its update is brief_optim_step on the
masters, and what it leaves is what the written artefact decodes to."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, quantize
from brief_pytorch_amd.fit import Fitter
from brief_pytorch_amd.modelsave import load_model, save_model
from brief_pytorch_amd.networks import SIREN, SIRENFT

pytestmark = pytest.mark.gpu
BITS = (2, 8, 11, 16)
K16 = 16384


def _net_spans(shapes):
    spans, off = [], 0
    for o, i in shapes:
        spans += [(off, o * i), (off + o * i, o)]
        off += o * i + o
    return spans


def _tables():
    """name -> (buffer as float32 numpy, spans, elements in front of the buffer inside its 16-byte aligned allocation)"""
    rng = np.random.default_rng(11)
    out = {}
    f5 = _net_spans([(5, 2), (5, 5), (3, 5)])                                  # spans of 10, 5, 25, 5, 15, 3
    assert [c for _, c in f5] == [10, 5, 25, 5, 15, 3]
    for shift in (0, 1, 3):
        out["f5_shift%d" % shift] = (rng.standard_normal(63).astype(np.float32), f5, shift)
    f67 = _net_spans([(67, 3)] + [(67, 67)] * 3 + [(1, 67)])
    n67 = f67[-1][0] + f67[-1][1]
    out["f67"] = ((rng.standard_normal(n67) * 0.05).astype(np.float32), f67, 0)
    out["f67_shift2"] = ((rng.standard_normal(n67) * 0.05 + 3.0).astype(np.float32), f67, 2)
    out["ones64"] = (rng.standard_normal(64).astype(np.float32), [(i, 1) for i in range(64)], 1)
    big = rng.standard_normal(K16 + 1 + (1 << 20) + 3).astype(np.float32)
    for a, b in ((0, K16 + 1), (K16 + 1, big.size)):                           # the minimum at element 0, the maximum at the last element
        big[a], big[b - 1] = -7.5, 9.25
    out["big"] = (big, [(0, K16 + 1), (K16 + 1, (1 << 20) + 3)], 0)
    out["big_shift3_reversed"] = (big, [(K16 + 1, (1 << 20) + 3), (0, K16 + 1)], 3)
    out["constant"] = (np.concatenate([np.full(301, -0.125, np.float32), rng.standard_normal(40).astype(np.float32)]), [(0, 301), (301, 40)], 0)
    # gaps between the spans (copied through to qparams), spans given out of order, unused elements in front and behind
    out["gaps"] = (rng.standard_normal(5000).astype(np.float32), [(2100, 2500), (3, 7), (17, 2050), (4700, 1)], 1)
    return out


TABLES = _tables()


def _spans(spans):
    return (_lib.QuantSpan * len(spans))(*spans)


def _shifted(arr, shift, dtype, fill):
    """a device tensor holding `arr` that starts `shift` elements behind a 16-byte aligned address, and the allocation around it"""
    whole = torch.full((arr.size + shift + 8,), fill, dtype=dtype, device="cuda")
    view = whole[shift:shift + arr.size]
    view.copy_(torch.from_numpy(arr).to(dtype))
    return whole, view


def _run(name, bits):
    buf, spans, shift = TABLES[name]
    L, n, st = _lib.lib(), len(spans), _lib.stream_ptr()
    keep, params = _shifted(buf, shift, torch.float32, 0.0)
    lo_step = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
    total = sum(c for _, c in spans)
    ws = torch.empty(L.brief_quant_workspace_bytes(total, n) // 4, dtype=torch.float32, device="cuda")
    sp = _spans(spans)
    _lib.check(L.brief_quant_ranges(_lib.ptr(params), sp, n, bits, _lib.ptr(lo_step), _lib.ptr(ws), ws.numel() * 4, st))
    QS, CS = -12345.0, 0xABCD                                                  # sentinels: what the kernels must leave alone
    qkeep, qparams = _shifted(np.full(buf.size, QS, np.float32), shift, torch.float32, QS)
    ckeep, codes = _shifted(np.full(buf.size, CS, np.uint16).view(np.int16), shift, torch.int16, -1)
    _lib.check(L.brief_quant_apply(_lib.ptr(params), sp, n, bits, _lib.ptr(lo_step), _lib.ptr(qparams), _lib.ptr(codes), st))
    dkeep, decoded = _shifted(np.full(buf.size, QS, np.float32), shift, torch.float32, QS)
    _lib.check(L.brief_quant_decode(_lib.ptr(codes), sp, n, _lib.ptr(lo_step), _lib.ptr(decoded), st))
    # each output alone (the other NULL) gives the same
    q_only = torch.full_like(qparams, QS)
    c_only = torch.full_like(codes, -1)
    _lib.check(L.brief_quant_apply(_lib.ptr(params), sp, n, bits, _lib.ptr(lo_step), _lib.ptr(q_only), None, st))
    _lib.check(L.brief_quant_apply(_lib.ptr(params), sp, n, bits, _lib.ptr(lo_step), None, _lib.ptr(c_only), st))
    d_only = torch.full_like(decoded, QS)                                      # (aligned differently from the codes it is decoded from)
    _lib.check(L.brief_quant_decode(_lib.ptr(codes), sp, n, _lib.ptr(lo_step), _lib.ptr(d_only), st))
    torch.cuda.synchronize()
    assert torch.equal(d_only, decoded)
    got_ls, got_q, got_d = lo_step.cpu().numpy(), qparams.cpu().numpy(), decoded.cpu().numpy()
    got_c = codes.cpu().numpy().view(np.uint16)
    want_q, want_d, want_c = np.full(buf.size, QS, np.float32), np.full(buf.size, QS, np.float32), np.full(buf.size, CS, np.uint16)
    first, last = min(o for o, _ in spans), max(o + c for o, c in spans)
    want_q[first:last] = buf[first:last]                                       # gaps: copied through
    for k, (o, c) in enumerate(spans):
        w = buf[o:o + c]
        lo, step = quantize.ranges(w, bits)
        assert got_ls[k, 0].tobytes() == lo.tobytes() and got_ls[k, 1].tobytes() == step.tobytes(), (name, bits, k, got_ls[k], lo, step)
        want_c[o:o + c] = quantize.quantise(w, lo, step, bits)
        want_q[o:o + c] = want_d[o:o + c] = quantize.dequantise(want_c[o:o + c], lo, step)
    assert np.array_equal(got_c, want_c), (name, bits)
    assert got_q.tobytes() == want_q.tobytes(), (name, bits)
    assert got_d.tobytes() == want_d.tobytes(), (name, bits)
    assert torch.equal(q_only, qparams) and np.array_equal(c_only.cpu().numpy().view(np.uint16)[want_c != CS], want_c[want_c != CS])
    # nothing around the buffers was written
    for whole, fill in ((qkeep, QS), (dkeep, QS), (ckeep, -1)):
        w = whole.cpu().numpy()
        assert (w[:shift] == fill).all() and (w[shift + buf.size:] == fill).all(), (name, bits)
    del keep


@pytest.mark.parametrize("bits", BITS)
def test_kernels_equal_numpy_bit_for_bit(bits):
    for name in TABLES:
        _run(name, bits)


def test_constant_tensor_and_extremes_at_the_ends():
    L, st = _lib.lib(), _lib.stream_ptr()
    buf, spans, _ = TABLES["constant"]
    p = torch.from_numpy(buf).cuda()
    ls = torch.empty((2, 2), dtype=torch.float32, device="cuda")
    ws = torch.empty(L.brief_quant_workspace_bytes(buf.size, 2) // 4, dtype=torch.float32, device="cuda")
    q = torch.empty_like(p)
    c = torch.full((buf.size,), 7, dtype=torch.int16, device="cuda")
    _lib.check(L.brief_quant_ranges(_lib.ptr(p), _spans(spans), 2, 8, _lib.ptr(ls), _lib.ptr(ws), ws.numel() * 4, st))
    _lib.check(L.brief_quant_apply(_lib.ptr(p), _spans(spans), 2, 8, _lib.ptr(ls), _lib.ptr(q), _lib.ptr(c), st))
    assert ls[0].tolist() == [-0.125, 0.0] and not c[:301].any() and torch.equal(q[:301], p[:301])
    buf, spans, _ = TABLES["big"]
    p = torch.from_numpy(buf).cuda()
    ws = torch.empty(L.brief_quant_workspace_bytes(buf.size, 2) // 4, dtype=torch.float32, device="cuda")
    _lib.check(L.brief_quant_ranges(_lib.ptr(p), _spans(spans), 2, 16, _lib.ptr(ls), _lib.ptr(ws), ws.numel() * 4, st))
    assert ls[:, 0].tolist() == [-7.5, -7.5] and ls[0, 1].item() == ls[1, 1].item() == float(np.float32(16.75) / np.float32(65535))


def test_c_abi_refusals_name_the_limit():
    L, st = _lib.lib(), _lib.stream_ptr()
    p = torch.zeros(100, dtype=torch.float32, device="cuda")
    q = torch.zeros(100, dtype=torch.float32, device="cuda")
    c = torch.zeros(100, dtype=torch.int16, device="cuda")
    ls = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    ws = torch.zeros(1024, dtype=torch.float32, device="cuda")
    ok = [(0, 50), (50, 50)]

    def ranges(params=p, spans=ok, n=None, bits=8, lo_step=ls, work=ws, nbytes=None):
        return L.brief_quant_ranges(_lib.ptr(params), _spans(spans) if spans else None, len(spans) if n is None else n, bits, _lib.ptr(lo_step),
                                    _lib.ptr(work), (work.numel() * 4 if work is not None else 0) if nbytes is None else nbytes, st)

    def apply(params=p, spans=ok, n=None, bits=8, lo_step=ls, qp=q, codes=c):
        return L.brief_quant_apply(_lib.ptr(params), _spans(spans) if spans else None, len(spans) if n is None else n, bits, _lib.ptr(lo_step),
                                   _lib.ptr(qp), _lib.ptr(codes), st)

    def decode(codes=c, spans=ok, n=None, lo_step=ls, out=q):
        return L.brief_quant_decode(_lib.ptr(codes), _spans(spans) if spans else None, len(spans) if n is None else n, _lib.ptr(lo_step), _lib.ptr(out), st)

    def refused(rc, code, text):
        assert rc == code and text in L.brief_last_error().decode(), (rc, L.brief_last_error())

    INVALID, WORKSPACE = -1, -3
    assert ranges() == 0 and apply() == 0 and decode() == 0
    for call in (ranges, apply):
        for bits in (1, 17, 0, -8):
            refused(call(bits=bits), INVALID, "bits must be 2..16")
    for call in (ranges, apply, decode):
        refused(call(spans=[(i, 1) for i in range(65)]), INVALID, "ntensors must be 1..64")
        refused(call(n=0), INVALID, "ntensors must be 1..64")
        refused(call(spans=None, n=2), INVALID, "null buffer")
        refused(call(spans=[(0, 50), (60, 0)]), INVALID, "count >= 1")
        refused(call(spans=[(0, 50), (60, -4)]), INVALID, "count >= 1")
        refused(call(spans=[(-1, 50), (60, 4)]), INVALID, "negative offset")
        refused(call(spans=[(0, 50), (49, 10)]), INVALID, "overlapping spans")
        refused(call(spans=[(40, 30), (0, 41)]), INVALID, "overlapping spans")
        refused(call(spans=[(0, 50), (0, 50)]), INVALID, "overlapping spans")
        refused(call(spans=[(0, (1 << 40) + 1)]), INVALID, "2^40")
        refused(call(lo_step=None), INVALID, "null buffer")
    refused(ranges(params=None), INVALID, "null buffer")
    refused(ranges(work=None), INVALID, "null buffer")
    refused(apply(params=None), INVALID, "null buffer")
    refused(apply(qp=None, codes=None), INVALID, "null buffer")
    refused(decode(codes=None), INVALID, "null buffer")
    refused(decode(out=None), INVALID, "null buffer")
    refused(ranges(nbytes=15), WORKSPACE, "workspace too small")
    refused(ranges(spans=[(0, K16 + 1)], nbytes=8), WORKSPACE, "workspace too small")      # (refused before anything is read)
    assert ranges(nbytes=16) == 0
    assert L.brief_quant_workspace_bytes(100, 2) == 16 and L.brief_quant_workspace_bytes(K16 + 1 + (1 << 20) + 3, 2) == (65 + 2) * 8
    assert L.brief_quant_workspace_bytes(0, 2) == -1 and L.brief_quant_workspace_bytes(100, 65) == -1 and L.brief_quant_workspace_bytes(100, 0) == -1
    torch.cuda.synchronize()


# ---- the quantised step
DIMS = (13, 17, 19)
N = 2000


def _siren():
    return SIREN(coords_channel=3, data_channel=1, features=67, layers=5, w0=20)


def _sirenft():
    return SIRENFT(coords_channel=3, data_channel=1, features=20, layers=4, w0=20, ratio=2)


def _targets():
    g = torch.Generator().manual_seed(5)
    return (torch.rand(int(np.prod(DIMS)), 1, generator=g) * 100.0).cuda()


def _fake_quantised_params(net, bits):
    """numpy's fake-quantisation of every tensor of the net, in the canonical order of net.params"""
    p = net.params.cpu().numpy()
    out = p.copy()
    for o, c in [(s.offset, s.count) for s in net.quant_spans()]:
        out[o:o + c] = quantize.fake_quantise(p[o:o + c], bits)
    return out


@pytest.mark.parametrize("make", [_siren, _sirenft], ids=["SIREN_F67", "SIRENFT"])
@pytest.mark.parametrize("optimizer", ["Adamax", "Adam"])
def test_one_quantised_step_is_a_plain_step_on_the_fake_quantised_weights(make, optimizer):
    bits, seed, lr = 6, 42, 2e-3
    torch.manual_seed(2)
    net = make().to("cuda")
    tv = _targets()
    masters = net.params.clone()
    fit = Fitter(net, tv, DIMS, sampler="randompoint", sample_size=N, optimizer=optimizer, lr=lr, seed=seed)
    loss = fit.run_quantised(1, bits)
    assert fit.t == 1
    # a second net holding numpy's fake-quantisation of the first one's parameters, on the index set the step drew
    torch.manual_seed(2)
    other = make().to("cuda")
    other.params.copy_(torch.from_numpy(_fake_quantised_params(other, bits)))
    other.mark_packed_stale()
    assert torch.equal(net.qparams, other.params)
    pop = int(np.prod(DIMS))
    idx = torch.empty(N, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().brief_sample_indices(_lib.ptr(idx), N, pop, seed, 1, _lib.stream_ptr()))
    loss2, _ = other.train_step(N, tv, idx=idx, grid=(DIMS, -1.0, 1.0))
    assert torch.equal(net.grads, other.grads) and bool(net.grads.abs().max() > 0)
    assert torch.equal(loss, loss2)
    # the masters: brief_optim_step on the UNQUANTISED parameters with those gradients
    s1, s2 = torch.zeros_like(masters), torch.zeros_like(masters)
    _lib.check(_lib.lib().brief_optim_step(_lib.OPT_KIND[optimizer], _lib.ptr(masters), _lib.ptr(other.grads), _lib.ptr(s1), _lib.ptr(s2),
                                           masters.numel(), lr, 0.9, 0.999, 1e-8, 1, _lib.stream_ptr()))
    assert torch.equal(net.params, masters) and torch.equal(fit.s1, s1) and torch.equal(fit.s2, s2)
    assert not torch.equal(net.params, net.qparams)


def test_run_switches_to_the_quantised_phase_without_a_seam():
    """Fitter(quantize=(bits, first)): run() over the boundary == plain steps up to it, then run_quantised; counter, schedule, state and
    sample stream continue (a second fitter that is driven by hand gives the same bits)"""
    sched = {"name": "MultiStepLR", "milestones": [4], "gamma": 0.5}
    nets, fits = [], []
    for quant in ((7, 3), None):
        torch.manual_seed(4)
        nets.append(_sirenft().to("cuda"))
        fits.append(Fitter(nets[-1], _targets(), DIMS, sampler="randompoint", sample_size=N, lr=1e-3, scheduler=sched, seed=9, quantize=quant))
    log = fits[0].run(6, log=True)
    a = fits[1].run(3, log=True)
    b = fits[1].run_quantised(3, 7, log=True)
    assert fits[0].t == fits[1].t == 6
    assert torch.equal(log, torch.cat([a, b])) and torch.equal(nets[0].params, nets[1].params) and torch.equal(fits[0].s2, fits[1].s2)
    # afterwards the in-memory net decodes its masters again
    torch.manual_seed(4)
    ref = _sirenft().to("cuda")
    ref.params.copy_(nets[0].params)
    ref.mark_packed_stale()
    assert torch.equal(nets[0].decode_grid((5, 6, 7)), ref.decode_grid((5, 6, 7)))


@pytest.mark.parametrize("make", [_siren, _sirenft], ids=["SIREN_F67", "SIRENFT"])
def test_the_written_artefact_decodes_to_the_in_memory_quantised_weights(tmp_path, make):
    bits, dims = 8, (9, 13, 17)
    torch.manual_seed(6)
    net = make().to("cuda")
    fit = Fitter(net, _targets(), DIMS, sampler="randompoint", sample_size=N, lr=1e-3, seed=1)
    fit.run_quantised(5, bits)
    d = str(tmp_path / "module")
    save_model(net, d, quantize_bits=bits)
    assert os.listdir(d) == [quantize.FILE_NAME]
    loaded = load_model(make(), d).to("cuda")
    held = make().to("cuda")
    held.params.copy_(net.fake_quantise(bits))                                 # the quantisation of the masters as they are now
    held.mark_packed_stale()
    assert torch.equal(loaded.params, held.params)
    assert np.array_equal(loaded.params.cpu().numpy(), _fake_quantised_params(net, bits))
    for kind, kw in (("f32", {}), ("u16", {"scale": (0.0, 100.0), "vrange": (0.0, 60000.0)})):
        got, want = loaded.decode_grid(dims, out_kind=kind, **kw), held.decode_grid(dims, out_kind=kind, **kw)
        assert torch.equal(got, want), kind
    assert not torch.equal(loaded.decode_grid(dims), net.decode_grid(dims))     # (the masters are another net)


def test_unsupported_nets_are_refused_by_name():
    from brief_pytorch_amd.networks import FFN
    with pytest.raises(_lib.BriefError, match="quantised weights exist for SIREN"):
        FFN(coords_channel=3, data_channel=1, embsize=8, features=16, layers=3).to("cuda").fake_quantise(8)
    with pytest.raises(_lib.BriefError, match="fp32 net"):
        SIREN(coords_channel=3, data_channel=1, features=32, layers=3, precision="bf16").to("cuda").fake_quantise(8)
