"""Caller-owned scratch between guards, filled three ways, for tests/test_gpu_scratch_contract.py.

include/brief_hip.h: what a workspace, a fragment copy or an output holds on entry is irrelevant, and nothing outside the buffer is touched.
Python allocates all of them with torch.empty, which in a test process returns fresh pages or recycled blocks of finite floats; here
every one of them is a window of exactly the size the library asks for into a larger allocation:

    [ GUARD bytes of a pattern | the buffer, filled | GUARD bytes of the pattern ]

GUARD = 4096 is a multiple of 256, so the window keeps the alignment a fresh torch.empty has (the 16-byte LDS-DMA and buffer loads of the
kernels assume it; a misaligned workspace is another subject).

The fills:
    ZERO    every byte 0: the baseline
    NAN     every byte 0xFF: a NaN as f32 and as a bf16 pair, -1 as an integer
    STALE   seeded uniform floats in [-1, 1], what an earlier batch's activations look like (v_max / v_min, the clip of the integer epilogue
            and the `yhat <= thr` select all drop a NaN operand silently: a stale finite value is not dropped)

seat_*() put such windows where the modules look for their buffers (brief_pytorch_amd/networks.py honours a seated buffer that is large
enough), and tail_plan() restates fused_tail_plan of csrc/brief_hip.hip for the shapes whose test is about a plan."""
import ctypes as C

import numpy as np
import torch

from brief_pytorch_amd import _lib

GUARD = 4096
FILLS = ("ZERO", "NAN", "STALE")
OTHER_FILLS = FILLS[1:]


def _guard_pattern(count, device):
    """bytes that no fill consists of, and not one value repeated"""
    i = torch.arange(count, dtype=torch.int64, device=device)
    return ((i * 7 + 13) % 251 + 1).to(torch.uint8)


class Scratch:
    """`nbytes` bytes (a multiple of 4) of `fill` between two guards; `.f32` is the window as float32"""

    def __init__(self, nbytes, fill, device, seed=0):
        nbytes = int(nbytes)
        assert nbytes >= 0 and nbytes % 4 == 0 and fill in FILLS, (nbytes, fill)
        self.nbytes, self.fill = nbytes, fill
        self.buf = torch.empty(2 * GUARD + nbytes, dtype=torch.uint8, device=device)
        self.pat = _guard_pattern(GUARD, self.buf.device)
        self.buf[:GUARD] = self.pat
        self.buf[GUARD + nbytes:] = self.pat
        self.f32 = self.buf[GUARD:GUARD + nbytes].view(torch.float32)
        if fill == "ZERO":
            self.f32.zero_()
        elif fill == "NAN":
            self.buf[GUARD:GUARD + nbytes] = 0xFF
        else:
            g = torch.Generator(device=self.buf.device).manual_seed(1234 + seed)
            self.f32.uniform_(-1.0, 1.0, generator=g)
        assert self.f32.numel() * 4 == nbytes
        assert self.f32.data_ptr() % 256 == 0 or self.buf.device.type != "cuda"      # (the device allocator's granularity)

    def intact(self):
        return bool(torch.equal(self.buf[:GUARD], self.pat)), bool(torch.equal(self.buf[GUARD + self.nbytes:], self.pat))


class Seated:
    """the Scratch objects behind one module's buffers, by name"""

    def __init__(self, fill, device):
        self.fill, self.device, self.parts = fill, device, {}

    def new(self, name, nbytes):
        assert nbytes >= 0, (name, nbytes, _lib.lib().brief_last_error().decode())
        s = self.parts[name] = Scratch(nbytes, self.fill, self.device, seed=len(self.parts))
        return s.f32

    def check(self, what=""):
        """after the calls: both guards of every buffer still hold the pattern (synchronises)"""
        torch.cuda.synchronize()
        for name, s in self.parts.items():
            front, back = s.intact()
            assert front, "%s: the guard in front of %s (%d bytes, %s) was written" % (what, name, s.nbytes, s.fill)
            assert back, "%s: the guard behind %s (%d bytes, %s) was written" % (what, name, s.nbytes, s.fill)


def seat_packed(m, fill, seated=None):
    """the fragment copy, filled, before the module's first repack"""
    seated = seated or Seated(fill, m.params.device)
    m.packed = seated.new("packed", 4 * m._abi_packed_count())
    m._stale = True
    return seated


def seat_train(m, n, fill):
    """workspace, gradient buffer, loss and fragment copy of a train / fit step of n samples, each of exactly the size asked for"""
    seated = seat_packed(m, fill)
    m._ws = seated.new("workspace", m._abi_train_ws_bytes(n))
    m.grads = seated.new("grads", 4 * m.params.numel())
    m._loss = seated.new("loss", 4)
    return seated


def seat_forward(m, n, fill, seated=None):
    """the inference scratch of a net above 1024 features for calls of n samples"""
    seated = seated or Seated(fill, m.params.device)
    need = _lib.lib().brief_forward_workspace_bytes(C.byref(m.desc), int(n))
    assert need > 0 and need % 4 == 0, need
    m._fws = seated.new("forward scratch", need)
    return seated


def seat_jac(m, fill):
    """the derivative decode's own fragment copy"""
    seated = Seated(fill, m.params.device)
    m._jac_packed = seated.new("jac packed", 4 * _lib.lib().brief_siren_jac_packed_count(C.byref(m.desc)))
    return seated


def seat_quant(m, fill):
    """what fake_quantise allocates on first use: the result, the ranges and the range kernel's workspace"""
    seated = Seated(fill, m.params.device)
    m._qspans = m.quant_spans()
    n = len(m._qspans)
    m.qparams = seated.new("qparams", 4 * m.params.numel())
    m._qlo_step = seated.new("lo_step", 4 * 2 * n).view(n, 2)
    m._qws = seated.new("quant workspace", _lib.lib().brief_quant_workspace_bytes(m.params.numel(), n))
    return seated


def bits(t):
    """a float32 tensor as its bit patterns: -0.0 is not 0.0 and a NaN equals itself"""
    return t.contiguous().view(torch.int32)


def assert_same(got, want, what):
    """two {name: float32 tensor} results, bit for bit"""
    assert got.keys() == want.keys()
    for name in want:
        a, b = got[name], want[name]
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        if not torch.equal(bits(a), bits(b)):
            bad = bits(a) != bits(b)
            raise AssertionError("%s: %s differs in %d of %d elements (%d of them not finite), first at %d" % (
                what, name, int(bad.sum()), a.numel(), int((~torch.isfinite(a))[bad].sum()), int(bad.reshape(-1).nonzero()[0])))


def assert_finite(res, what):
    for name, t in res.items():
        assert bool(torch.isfinite(t).all()), "%s: %s of the baseline is not finite" % (what, name)


def assert_fills_agree(run, what):
    """run(fill) -> {name: tensor}: finite under ZERO, and the same bits under NAN and under STALE (both are run before either is
    reported: which fills a defect shows under says what kind of read it is).  Returns the baseline."""
    base = run("ZERO")
    assert_finite(base, what)
    errors = []
    for fill in OTHER_FILLS:
        try:
            assert_same(run(fill), base, "%s, scratch filled with %s" % (what, fill))
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, "\n".join(errors)
    return base


# ---- fused_tail_plan (csrc/brief_hip.hip), restated for fp32 SIRENs of 9 tiles and more
def _lean_wpe(mtw):
    """lean_wpe(1, MTW), csrc/brief_lean.inc (BRIEF_LEAN_WPE2 = 3)"""
    return 3 if mtw <= 2 else (2 if mtw <= 4 else 1)


def _lean_lds_floats(mtw, nt):
    """lean_lds(1, MTW, nt).total"""
    return max(nt * 1024, 4 * 32 * mtw * 33) + 4 * 256 + 4 * 32 * nt + 4 * 32 * 4


def _train_grid(nt, n, cus):
    """fused_grid(d, n, true) of k_lean (9 .. 32 tiles) and k_wide"""
    cap = cus
    if nt <= 32:
        mtw = (nt + 3) // 4
        by_lds, by_regs = (160 * 1024) // (4 * _lean_lds_floats(mtw, nt)), _lean_wpe(mtw)
        cap = cus * (max(by_lds, 1) if by_lds < by_regs else by_regs)
    return min(max((n + 31) // 32, 1), cap)


def _split_rule(nt, hidden, nchunks, min_rounds, cus):
    """wgrad_split_rule"""
    nq = (nt + 7) // 8
    B = hidden * nq * nq
    s = max(cus // B, 1)
    rounds = lambda c: (c * B + cus - 1) // cus      # noqa: E731
    if min_rounds > 1:
        best = 1e30
        for c in range(1, 65):
            if rounds(c) < min_rounds and c < 64:
                continue
            cost = rounds(c) / c + 0.0001 * c
            if cost < best - 1e-9:
                best, s = cost, c
    elif nt > 32:
        best = 1e30
        for c in range(1, 17):
            cost = rounds(c) / c + 0.001 * c
            if cost < best - 1e-9:
                best, s = cost, c
    elif nq >= 2:
        base = 1.0 / s + 0.0001 * s
        best = base
        for c in range(s + 1, min(max(4 * s, 16), 64) + 1):
            cost = rounds(c) / c + 0.0001 * c
            if cost < best - 1e-9 and cost < 0.985 * base:
                best, s = cost, c
    return min(s, nchunks)


def tail_plan(features, layers, n, cus=256):
    """the mode fused_tail_plan gives an fp32 SIREN of 9 tiles and more on `cus` compute units: 0 none, 1 the extra K split behind the body
    (k_wide), 2 uneven K splits (k_lean, 9 .. 32 tiles)"""
    nt, hidden = (features + 31) // 32, layers - 2
    assert nt >= 9 and hidden >= 1
    tiles = (n + 31) // 32
    G = _train_grid(nt, n, cus)
    full = tiles // G * G
    rem = tiles - full
    if full == 0 or rem == 0:
        return 0
    if nt <= 32 and rem * 4 <= 3 * cus:
        nq = (nt + 7) // 8
        qt, B = (nt + nq - 1) // nq, hidden * nq * nq
        ns = _split_rule(nt, hidden, tiles, 1, cus)
        if ns * B > cus:
            ns = cus // B
        n_norm = 0
        if ns * B <= cus:
            for c in range(ns - 1, 0, -1):
                a_, s_ = (c * B + 7) // 8, ((ns - c) * B + 7) // 8
                if a_ + (rem + 7) // 8 <= cus // 8 and a_ + s_ <= cus // 8 and (ns - c) * B >= rem:
                    n_norm = c
                    break
        rho = (1.15 if nt <= 16 else 1.05) * 2.0 * hidden * nt * nt / (qt * qt)
        k_norm = (tiles + (ns - n_norm) * rho) / ns
        if n_norm > 0 and k_norm - rho >= 4.0 and rho < 0.8 * k_norm and 0 < (n_norm * int(k_norm * 65536.0)) >> 16 <= full:
            return 2
    if nt <= 32 or rem * 4 > 3 * G or _split_rule(nt, hidden, full, 3, cus) < 6:
        return 0
    return 1


def cu_count():
    return int(_lib.lib().brief_cu_count())


def rand_batch(rng, n, cin, cout, scale=100.0):
    """coordinates in [-1, 1], targets in [0, scale] and a weight map in {0.25, 1}, as float32 numpy"""
    x = rng.uniform(-1, 1, size=(n, cin)).astype(np.float32)
    y = rng.uniform(0, scale, size=(n, cout)).astype(np.float32)
    w = np.where(rng.uniform(size=(n, cout)) < 0.5, 0.25, 1.0).astype(np.float32)
    return x, y, w
