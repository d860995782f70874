"""The composite view's arithmetic (csrc/brief_composite.h) restated in Python integers, for tests/test_composite_host.py and
tests/test_gpu_composite.py: the constants from `decimal`, the transmittance W, one ray's fold and a pixel's finish."""
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

TAU_SAT = 32 * 65536


def exact_tables():
    """A[i] = round(2^31 * 2^(-i / 256)), B[j] = round(2^31 * 2^(-j / 65536)), 256 entries each, from decimal at 60 digits"""
    getcontext().prec = 60
    ln2 = Decimal(2).ln()
    r = lambda x: int(x.to_integral_value(rounding=ROUND_HALF_EVEN))
    return ([r((ln2 * (Decimal(31) - Decimal(i) / 256)).exp()) for i in range(256)],
            [r((ln2 * (Decimal(31) - Decimal(j) / 65536)).exp()) for j in range(256)])


A, B = exact_tables()


def W(tau):
    q, f = tau >> 16, tau & 0xFFFF
    return 0 if q >= 32 else ((A[f >> 8] * B[f & 255]) >> 30) >> q


def random_table(rng, bits):
    """int32 [2^bits, 4], in range: empty, faint, dense and opaque rows in a random order (the first two kinds of the list even in a
    table of two rows), and emissions that are consistent with nothing: the fold must not care"""
    import numpy as np
    kinds = np.array([700, TAU_SAT // 5, 0, 65536, 1, 700, 0, 20000, 700, 65536, 0, TAU_SAT])
    n = 1 << bits
    tf = np.empty((n, 4), np.int32)
    tf[:, 0] = np.minimum(kinds[rng.permutation(n) % len(kinds)] + rng.integers(0, 3, n), TAU_SAT)
    tf[:, 1:] = rng.integers(0, 65281, (n, 3))
    return tf


def fold_ray(rows):
    """(tau_run, [accR, accG, accB]) of one ray from the table rows (tau, eR, eG, eB) of its inside samples, front to back"""
    run, acc = 0, [0, 0, 0]
    for e in rows:
        w = W(run)
        acc = [a + w * int(x) for a, x in zip(acc, e[1:])]
        run = min(run + int(e[0]), TAU_SAT)
    return run, acc


def finish(run, acc, bg):
    """[R, G, B, A] of a pixel"""
    w = W(run)
    return [min(255, (a + int(b) * 256 * w + (1 << 39)) >> 40) for a, b in zip(acc, bg)] + [min(255, (((1 << 32) - w) * 255 + (1 << 31)) >> 32)]
