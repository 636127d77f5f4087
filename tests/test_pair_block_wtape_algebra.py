"""The algebra behind "w on the tape" (pair_launch.hpp: pair_wtape), on dense matrices, no GPU.  A block of two
factors of one exponential shares H = D + c P with P the sum of all single-qubit flips.  For ANY split of the qubits into the bits X
of the layout that started the block and the rest Y', P = P_X + P_Y', and the mid-block state the adjoint needs,
x_a = (gamma_1 + beta_1 H) v, is rebuilt from v and the taped w = P_X v with one partner-sum round over the Y' bits only:
x_a = gamma_1 v + beta_1 (D v + c (w + P_Y' v))."""
import numpy as np
import pytest


def _flip_sum(n, bits):
    """Dense sum of the flips of the qubits in `bits` on 2^n amplitudes."""
    dim = 1 << n
    p = np.zeros((dim, dim))
    idx = np.arange(dim)
    for b in bits:
        p[idx, idx ^ (1 << b)] += 1.0
    return p


@pytest.mark.parametrize("n,seed", [(3, 0), (5, 1), (6, 2), (7, 3), (7, 4)])
def test_mid_block_state_from_the_taped_partial_sum(n, seed):
    rng = np.random.default_rng(seed)
    dim = 1 << n
    perm = rng.permutation(n)
    k = int(rng.integers(0, n + 1))  # an arbitrary split, the empty and the full one included over the seeds
    xbits, ybits = perm[:k], perm[k:]
    d = rng.normal(size=dim)
    c = rng.normal()
    gamma, beta = complex(*rng.normal(size=2)), complex(*rng.normal(size=2))
    v = rng.normal(size=dim) + 1j * rng.normal(size=dim)
    h = np.diag(d) + c * _flip_sum(n, range(n))
    assert np.array_equal(_flip_sum(n, xbits) + _flip_sum(n, ybits), _flip_sum(n, range(n)))
    w = _flip_sum(n, xbits) @ v   # what the forward chain tapes
    s = _flip_sum(n, ybits) @ v   # the adjoint's extra round
    x_a = gamma * v + beta * (d * v + c * (w + s))
    ref = gamma * v + beta * (h @ v)
    assert np.abs(x_a - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("n_blocks", [1, 2, 5, 15, 20])
def test_adjoint_launch_layouts_follow_the_forward_blocks(n_blocks):
    """Forward launch j runs in layout j & 1, starts block j and finishes block j - 1.  The adjoint chain that ends in block g_hi runs
    its launch i in layout (i + g_hi) & 1 and finishes block g_hi - (i - 1) there: the layout in which the forward pass finished it."""
    finished_in = {g: (g + 1) & 1 for g in range(n_blocks)}
    for g_hi in range(n_blocks):
        for i in range(1, g_hi + 2):
            assert (i + g_hi) & 1 == finished_in[g_hi - (i - 1)]
