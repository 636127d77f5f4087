"""Dense numpy references for the occupation correlations of a density-matrix register (RydProblem.dm_moments): the rows as sums over
the axes of the real diagonal reshaped to n two-level axes — no index arithmetic shared with the library or with
observables.dm_occupation_moments — the sum of the absolute terms of every row, the dense cotangent rydiff.h writes down, and the
explicit number operators of the host test."""
import itertools

import numpy as np


def moment_row_count(n: int) -> int:
    return 1 + n + n * (n - 1) // 2


def _rows_of_diagonal(p: np.ndarray, n: int) -> np.ndarray:
    """p (2^n,) -> S, the singles in ascending atom, the pairs in lexicographic order; atom q is axis q of p.reshape((2,) * n)."""
    t = p.reshape((2,) * n)
    rows = [t.sum()]
    rows += [np.take(t, 1, axis=q).sum() for q in range(n)]
    rows += [np.take(np.take(t, 1, axis=r), 1, axis=q).sum() for q, r in itertools.combinations(range(n), 2)]  # (axis r first: r > q)
    return np.asarray(rows, dtype=np.float64)


def dm_moment_rows_reference(v: np.ndarray, n: int):
    """The DmMoments rows of one vector v = vec(rho) (4^n,): (values, sums of absolute terms), float64 (1 + n + n(n-1)/2,).  Only the
    real part of the diagonal counts, as it is (no clamp)."""
    p = np.real(np.diagonal(v.reshape(2 ** n, 2 ** n))).astype(np.float64)
    return _rows_of_diagonal(p, n), _rows_of_diagonal(np.abs(p), n)


def dm_moment_cotangent_reference(n: int, g):
    """The dense cotangent of the rows with weights g (row order): q(x) = g_S + sum_q g_q x_q + sum_{q<r} g_qr x_q x_r on the real
    part of entry (x, x), nothing elsewhere.  Returns (cotangent (4^n,) complex, sum of the absolute contributions per entry (4^n,))."""
    dim = 2 ** n
    g = np.asarray(g, dtype=np.float64)
    assert g.shape == (moment_row_count(n),)
    grid = np.indices((2,) * n).reshape(n, dim).astype(np.float64)  # grid[q][x]: atom q of index x (axis 0 most significant)
    q = np.full(dim, g[0])
    tot = np.full(dim, abs(g[0]))
    r = 1
    for a in range(n):
        q += g[r] * grid[a]
        tot += abs(g[r]) * grid[a]
        r += 1
    for a, b in itertools.combinations(range(n), 2):
        q += g[r] * grid[a] * grid[b]
        tot += abs(g[r]) * grid[a] * grid[b]
        r += 1
    cot = np.zeros((dim, dim), dtype=np.complex128)
    full = np.zeros((dim, dim), dtype=np.float64)
    cot[np.arange(dim), np.arange(dim)] = q
    full[np.arange(dim), np.arange(dim)] = tot
    return cot.reshape(-1), full.reshape(-1)


def number_operator(n: int, q: int) -> np.ndarray:
    """n_q as a dense (2^n, 2^n) matrix: 1 (x) ... (x) diag(0, 1) (x) ... (x) 1 with atom 0 the leftmost factor."""
    op = np.ones((1, 1))
    for j in range(n):
        op = np.kron(op, np.diag([0.0, 1.0]) if j == q else np.eye(2))
    return op


def dense_moment_rows(rho: np.ndarray, n: int) -> np.ndarray:
    """Re Tr(rho), Re Tr(rho n_q), Re Tr(rho n_q n_r) with explicit dense operators, in the row order."""
    ops = [number_operator(n, q) for q in range(n)]
    rows = [np.trace(rho).real]
    rows += [np.trace(rho @ ops[q]).real for q in range(n)]
    rows += [np.trace(rho @ ops[q] @ ops[r]).real for q, r in itertools.combinations(range(n), 2)]
    return np.asarray(rows)


# ---- the forward-mode oracle of the tangent tests ------------------------------------------------------------------------------
# The moment rows and their directional derivatives from R.lindblad_magnus_dense on terms + s * direction and
# torch.autograd.functional.jacobian w.r.t. s at s = 0, exactly as tests/dm_tangent_reference.py forms the other rows: its terms, its
# recorded inputs (psi0 and the first TANGENT_DIRS directions: all three tables, d_amp only, zero), its TSAVE and h_max, with dephasing.
# The oracle takes minutes, so the suite reads the record tests/golden/dm_moments_tangent_oracle.npz;
# `python -m tests.dm_moments_reference` regenerates it, and tests/test_dm_moments_host.py recomputes the values of the smallest case.
TANGENT_SIZES = (2, 3)
TANGENT_NOISE = "dephasing"
TANGENT_DIRS = 3


def _golden():
    from pathlib import Path

    return Path(__file__).resolve().parent / "golden" / "dm_moments_tangent_oracle.npz"


def tangent_oracle_case(n: int, derivatives: bool = True):
    """(values (rows, n_t, B), derivatives (TANGENT_DIRS, rows, n_t, B) or None) of the oracle at n atoms."""
    import torch

    from oracle import restatement as R
    from pulser_diff_amd.observables import dm_occupation_moments
    from tests import dm_tangent_reference as T
    from tests.helpers import shifted_terms

    inp = T.load_case(n, TANGENT_NOISE)
    terms = T.case_terms(n)
    tsave = torch.tensor(T.TSAVE, dtype=torch.float64)
    collapse = R.collapse_operators(n, T.NOISE[TANGENT_NOISE])
    d_amp, d_det, d_u = (inp[k][:TANGENT_DIRS] for k in ("d_amp", "d_det", "d_u"))
    vals, jacs = [], []
    for b in range(T.BATCH[n]):
        rho0 = torch.outer(inp["psi0"][:, b], inp["psi0"][:, b].conj())

        def rows(s):
            rho = R.lindblad_magnus_dense(shifted_terms(terms, d_amp[:, 0], d_det[:, 0], d_u, s), collapse, rho0, tsave, h_max=T.h_max(n))
            return dm_occupation_moments(rho[..., None])[..., 0]  # (rows, n_t)

        s0 = torch.zeros(TANGENT_DIRS, dtype=torch.float64)
        vals.append(rows(s0).detach())
        if derivatives:
            jacs.append(torch.autograd.functional.jacobian(rows, s0))  # (rows, n_t, TANGENT_DIRS)
    return torch.stack(vals, dim=-1), (torch.stack(jacs, dim=-1).permute(2, 0, 1, 3).contiguous() if derivatives else None)


def load_tangent_case(n: int) -> dict:
    """The recorded oracle outputs of one size as CPU tensors: val (rows, n_t, B), der (TANGENT_DIRS, rows, n_t, B)."""
    import torch

    with np.load(_golden()) as z:
        return {name: torch.from_numpy(z[f"n{n}/{name}"]) for name in ("val", "der")}


if __name__ == "__main__":
    import torch

    torch.set_num_threads(1)
    merged = {}
    for size in TANGENT_SIZES:
        val, der = tangent_oracle_case(size)
        merged[f"n{size}/val"], merged[f"n{size}/der"] = val.numpy(), der.numpy()
    np.savez_compressed(_golden(), **merged)
    print("wrote", _golden(), _golden().stat().st_size, "bytes")
