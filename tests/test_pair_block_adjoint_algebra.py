"""CPU model of the adjoint block pass (k_chain2_bwd, pair_kernels.hpp) against the dense discrete adjoint.

A block holds the factors b then a of one exponential (forward order): x_a = (g_b + b_b H) x_b, out = (g_a + b_a H) x_a, with
H = D + c P real symmetric.  The launch that starts it in layout X hands over mu, w = P_X mu, t = P_X (D mu + c w); the launch
that finishes it in Y forms, with partner sums over Y' = Y \\ X only (round A on mu, round B on e = H mu + c w), the cotangent at
the block's input and both factors' exact gradient contractions, in the order the kernel uses."""
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


def adjoint_block(mu, xa, xb, d, c, X, Yp, sa, sb):
    """The two launches as the kernel runs them: (mu_out, P mu_mid, dL/dc, weight of d(x) per amplitude)."""
    ga, ba = np.conj(sa[0]), np.conj(sa[1])   # conjugated scalars of the adjoint
    gb, bb = np.conj(sb[0]), np.conj(sb[1])
    k = ba * bb
    w = flips(mu, X)                           # start, layout X
    t = flips(d * mu + c * w, X)
    s = flips(mu, Yp)                          # finish, layout Y: round A
    pm = w + s                                 # P mu
    h1 = d * mu + c * pm                       # H mu
    e = h1 + c * w
    mid = ga * mu + ba * h1                    # mu_mid: never written
    wx = np.real(sa[1] * np.conj(mu) * xa)     # factor a's weight of d(x)
    zc = np.real(sa[1] * np.vdot(pm, xa))      # factor a's drive contraction
    wx = wx + np.real(sb[1] * np.conj(mid) * xb)
    zc += np.real(sb[1] * np.vdot(ga * pm, xb))
    y = (gb + bb * d) * mid + bb * c * ga * pm  # mu_out but its tp part
    tp = t + (flips(e, Yp) if k != 0 else 0.0)  # round B (skipped for a one-factor block)
    y = y + k * c * tp
    zc += np.real(sb[1] * np.vdot(ba * tp, xb))
    return y, ga * pm + ba * tp, zc, wx


CASES = [(0, 0.83, False), (1, -2.1, False), (2, 0.0, False), (3, 1.4, True), (4, 0.0, True)]


@pytest.mark.parametrize("seed,c,one_factor", CASES)
@pytest.mark.parametrize("layouts", [((0, 1, 2, 3, 4), (0, 1, 5, 6, 7)), ((1, 3, 4, 6, 7), (0, 2, 5, 4, 1))])
def test_adjoint_block_equals_dense_discrete_adjoint(seed, c, one_factor, layouts):
    X, Y = layouts
    assert set(X) | set(Y) == set(range(N))
    Yp = tuple(b for b in Y if b not in X)
    rng = np.random.default_rng(100 + seed)
    d = rng.normal(size=DIM) * 3.0
    P = dense_p(range(N))
    I = np.eye(DIM)
    ga_, ba_, gb_, bb_ = rng.normal(size=4) + 1j * rng.normal(size=4)
    if one_factor:  # a one-factor block: b alone, a = identity (k = 0)
        ga_, ba_ = 1.0, 0.0
    H = np.diag(d) + c * P
    Fa, Fb = ga_ * I + ba_ * H, gb_ * I + bb_ * H
    xb = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)  # input of b (forward)
    xa = Fb @ xb                                           # input of a
    mu = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)  # cotangent at a's output
    y, p_mid, zc, wx = adjoint_block(mu, xa, xb, d, c, X, Yp, (ga_, ba_), (gb_, bb_))

    mu_mid = Fa.conj().T @ mu
    np.testing.assert_allclose(y, Fb.conj().T @ mu_mid, rtol=0, atol=1e-12 * np.abs(y).max())
    np.testing.assert_allclose(p_mid, P @ mu_mid, rtol=0, atol=1e-12 * np.abs(p_mid).max())

    # L = Re <mu, Fa Fb x_b>: the exact drive and diagonal derivatives
    def loss(cc, dd):
        Hc = np.diag(d + dd) + cc * P
        return np.real(np.vdot(mu, (ga_ * I + ba_ * Hc) @ (gb_ * I + bb_ * Hc) @ xb))

    # dL/dc, per factor against the dense matrices, and in sum against a central difference
    za = np.real(ba_ * np.vdot(P @ mu, xa))
    zb = np.real(bb_ * np.vdot(P @ mu_mid, xb))
    assert abs(zc - (za + zb)) < 1e-10 * max(1.0, abs(za) + abs(zb))
    h = 1e-6
    fd = (loss(c + h, 0.0) - loss(c - h, 0.0)) / (2 * h)
    assert abs(zc - fd) < 1e-6 * max(1.0, abs(fd))
    # weights of d(x): detuning and U_ij gradients are their contractions with dD/dtheta
    wref = np.real(ba_ * np.conj(mu) * xa) + np.real(bb_ * np.conj(mu_mid) * xb)
    np.testing.assert_allclose(wx, wref, rtol=0, atol=1e-12 * max(np.abs(wref).max(), 1.0))
    dd = rng.normal(size=DIM)
    fdd = (loss(c, h * dd) - loss(c, -h * dd)) / (2 * h)
    assert abs(float(wx @ dd) - fdd) < 1e-6 * max(1.0, abs(fdd))
    # a detuning group: D += delta * (count - popcount(x & mask)) — its gradient is the weight times that count
    x = np.arange(DIM)
    cnt = 5 - np.array([bin(int(v) & 0b11111).count("1") for v in x], dtype=float)
    fdg = (loss(c, h * cnt) - loss(c, -h * cnt)) / (2 * h)
    assert abs(float(wx @ cnt) - fdg) < 1e-6 * max(1.0, abs(fdg))


def test_adjoint_block_with_zero_amplitude_factor_needs_no_special_case():
    """c = 0 (the padded last sample): exact contractions, nothing divided by c."""
    rng = np.random.default_rng(7)
    X, Y = (0, 1, 2, 3, 4), (0, 1, 5, 6, 7)
    Yp = (5, 6, 7)
    d = rng.normal(size=DIM)
    I = np.eye(DIM)
    P = dense_p(range(N))
    sa, sb = (0.9 + 0.1j, -0.02 + 0.3j), (1.1 - 0.2j, 0.05 - 0.25j)
    H = np.diag(d)
    Fa, Fb = sa[0] * I + sa[1] * H, sb[0] * I + sb[1] * H
    xb = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)
    xa = Fb @ xb
    mu = rng.normal(size=DIM) + 1j * rng.normal(size=DIM)
    y, _, zc, _ = adjoint_block(mu, xa, xb, d, 0.0, X, Yp, sa, sb)
    np.testing.assert_allclose(y, Fb.conj().T @ Fa.conj().T @ mu, rtol=0, atol=1e-12 * np.abs(y).max())
    mu_mid = Fa.conj().T @ mu
    ref = np.real(sa[1] * np.vdot(P @ mu, xa)) + np.real(sb[1] * np.vdot(P @ mu_mid, xb))
    assert np.isfinite(zc) and abs(zc - ref) < 1e-10 * max(1.0, abs(ref))
