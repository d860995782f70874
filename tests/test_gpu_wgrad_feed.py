"""The operand feed of the 8-tile k_wgrad (the headline's weight-gradient GEMM): both panels of a 32-sample chunk reach LDS
by LDS-DMA, the sine and the bias sums are taken in place.  Train steps against the CPU oracle at the shapes where that feed
can go wrong — eight tiles exact (F = 256) and eight tiles with 31 zero padding rows (F = 225: the bias sums and the DMA of
padded rows), one and three hidden layers, and chunk counts that cover the prologue alone (n = 1, 32), a mostly empty last
chunk (33), buffer parity at the loop's exit (64, 96: two and three chunks), one chunk per K split at the headline's split
count (2720 = 85 chunks) and K splits of one and two chunks side by side (2752 = 86) — and bit-reproducibility of a step.
The check is that of test_train_step_shapes_vs_oracle (loss 1e-5 relative, every gradient tensor 1e-4 of its max-abs)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

from .test_gpu_parity import DEV, _check_grads, make_net

pytestmark = pytest.mark.gpu


def _batch(F, n):
    rng = np.random.default_rng(F + n)
    x = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    y = rng.uniform(0, 100, size=(n, 1)).astype(np.float32)
    w = np.where(rng.uniform(size=(n, 1)) < 0.5, 0.25, 1.0).astype(np.float32)
    return x, y, w


@pytest.mark.parametrize("n", [1, 32, 33, 64, 96, 2720, 2752])
@pytest.mark.parametrize("L", [3, 5])
@pytest.mark.parametrize("F", [256, 225])
def test_wgrad_feed_train_step_vs_oracle(F, L, n):
    m, d, p = make_net(L, F, 20.0, seed=L * 10 + F)
    x, y, w = _batch(F, n)
    loss, _ = m.train_step(n, torch.from_numpy(y).to(DEV), coords=torch.from_numpy(x).to(DEV),
                           weights=torch.from_numpy(w).to(DEV), thr=30.0)
    lo, go, _, _ = O.loss_grad(d, p, x, y, w, 0, 30.0, 0.01)
    assert abs(loss.item() - lo) / abs(lo) < 1e-5
    _check_grads(m, d, go)


def test_wgrad_feed_step_is_bit_reproducible():
    m, d, p = make_net(5, 256, 20.0, seed=7)
    n = 2752
    x, y, w = _batch(256, n)
    args = dict(coords=torch.from_numpy(x).to(DEV), weights=torch.from_numpy(w).to(DEV), thr=30.0)
    l1, _ = m.train_step(n, torch.from_numpy(y).to(DEV), **args)
    g1 = m.grads.clone()
    l2, _ = m.train_step(n, torch.from_numpy(y).to(DEV), **args)
    assert torch.equal(g1, m.grads) and l1.item() == l2.item()
