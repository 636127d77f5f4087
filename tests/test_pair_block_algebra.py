"""CPU model of the block-of-two chained pass (pair_kernels.hpp) against dense linear algebra.

Two layouts X, Y of tile bits (X u Y = every bit), P = P_X + P_Y' with Y' = Y \\ X.  The launch that starts a block in X hands
over v, w = P_X v, t = P_X (D v + c w); the launch that finishes it in Y forms, with partner sums over Y' only,
y = q(H) v = (g1 + b1 H)(g2 + b2 H) v and v_mid = (g1 + b1 H) v.  Run on a cotangent with conjugated scalars (H real symmetric
for a phase-free drive), the same quantities give P mu_y and P mu_mid exactly, hence both factors' drive contractions."""
import numpy as np
import pytest

N = 8
DIM = 1 << N


def flips(v, bits):
    x = np.arange(DIM)
    out = np.zeros_like(v)
    for b in bits:
        out += v[x ^ (1 << b)]
    return out


def dense_p(bits):
    m = np.zeros((DIM, DIM))
    x = np.arange(DIM)
    for b in bits:
        m[x, x ^ (1 << b)] += 1.0
    return m


def block(v, d, c, X, Yp, s1, s2):
    """The two launches on one vector: (y, v_mid, w + s, t + P_Y' e) as the kernel forms them."""
    g1, b1 = s1
    g2, b2 = s2
    a, bq, k = g1 * g2, g1 * b2 + b1 * g2, b1 * b2
    w = flips(v, X)                      # start, layout X
    t = flips(d * v + c * w, X)
    s = flips(v, Yp)                     # finish, layout Y: round A
    h1 = d * v + c * (w + s)
    e = h1 + c * w
    pe = flips(e, Yp) if k != 0 else np.zeros_like(v)  # round B (skipped for a one-factor block)
    y = a * v + bq * h1 + k * (d * h1 + c * (t + pe))
    return y, g1 * v + b1 * h1, w + s, t + pe


@pytest.mark.parametrize("seed,c,kappa_zero", [(0, 0.83, False), (1, -2.1, False), (2, 0.0, False), (3, 1.4, True), (4, 0.0, True)])
@pytest.mark.parametrize("layouts", [((0, 1, 2, 3, 4), (0, 1, 5, 6, 7)), ((1, 3, 4, 6, 7), (0, 2, 5, 4, 1))])
def test_block_of_two_equals_dense_product_and_gives_exact_flip_sums(seed, c, kappa_zero, layouts):
    X, Y = layouts
    assert set(X) | set(Y) == set(range(N))
    Yp = tuple(b for b in Y if b not in X)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=DIM) * 3.0
    P = dense_p(range(N))
    H = np.diag(d) + c * P
    g1, b1, g2, b2 = rng.normal(size=4) + 1j * rng.normal(size=4)
    if kappa_zero:
        g2, b2 = 1.0, 0.0
    v = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)
    y, v_mid, pv, ph = block(v, d, c, X, Yp, (g1, b1), (g2, b2))
    I = np.eye(DIM)
    F1, F2 = g1 * I + b1 * H, g2 * I + b2 * H
    np.testing.assert_allclose(v_mid, F1 @ v, rtol=0, atol=1e-12 * np.abs(v_mid).max())
    np.testing.assert_allclose(y, F2 @ F1 @ v, rtol=0, atol=1e-12 * np.abs(y).max())
    np.testing.assert_allclose(pv, P @ v, atol=1e-12 * np.abs(pv).max())
    if not kappa_zero:
        np.testing.assert_allclose(ph, P @ (H @ v), atol=1e-12 * max(np.abs(ph).max(), 1.0))

    # adjoint: the same block on the cotangent mu_y with conjugated scalars
    x = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)   # input of the block (forward)
    x_mid = F1 @ x
    mu_y = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)
    mu_x, mu_mid, p_mu_y, p_h = block(mu_y, d, c, X, Yp, (np.conj(g2), np.conj(b2)), (np.conj(g1), np.conj(b1)))
    np.testing.assert_allclose(mu_x, F1.conj().T @ F2.conj().T @ mu_y, atol=1e-12 * np.abs(mu_x).max())
    np.testing.assert_allclose(mu_mid, F2.conj().T @ mu_y, atol=1e-12 * np.abs(mu_mid).max())
    np.testing.assert_allclose(p_mu_y, P @ mu_y, atol=1e-12 * np.abs(p_mu_y).max())
    p_mu_mid = np.conj(g2) * p_mu_y + np.conj(b2) * p_h
    np.testing.assert_allclose(p_mu_mid, P @ mu_mid, atol=1e-12 * np.abs(p_mu_mid).max())
    # drive contractions of both factors, elementwise against the tape vectors: dRe<mu_y, F2 F1 x>/dc
    # = Re(b2 <P mu_y, x_mid>) + Re(b1 <P mu_mid, x>)
    h = 1e-6
    def loss(cc):
        Hc = np.diag(d) + cc * P
        return np.real(np.vdot(mu_y, (g2 * I + b2 * Hc) @ (g1 * I + b1 * Hc) @ x))
    fd = (loss(c + h) - loss(c - h)) / (2 * h)
    z2 = np.real(b2 * np.vdot(p_mu_y, x_mid))
    z1 = np.real(b1 * np.vdot(p_mu_mid, x))
    assert abs((z1 + z2) - fd) < 1e-6 * max(1.0, abs(fd))
    # detuning / U_ij weights: Re(b conj(mu) x) per factor, elementwise
    wd = np.real(b2 * np.conj(mu_y) * x_mid) + np.real(b1 * np.conj(mu_mid) * x)
    dd = rng.normal(size=DIM)
    def loss_d(eps):
        Hd = np.diag(d + eps * dd) + c * P
        return np.real(np.vdot(mu_y, (g2 * I + b2 * Hd) @ (g1 * I + b1 * Hd) @ x))
    fdd = (loss_d(h) - loss_d(-h)) / (2 * h)
    assert abs(float(wd @ dd) - fdd) < 1e-6 * max(1.0, abs(fdd))
