"""References for the native XY exchange term (RydProblem.xy_mode): a dense one (small registers) and a matrix-free one with
autograd (past the dense limit), both on the oracle's structured terms (``R.HamTerms``) plus the couplings ``J``:

    mode 1:  (X v)[x] = sum_{i<j, b_i(x) != b_j(x)} J_ij v[x ^ m_i ^ m_j]
    mode 2:  only the rows with b_i(x) = 0, b_j(x) = 1 (the reference's one-directional 2 * int_mat)

b_q = index bit N-1-q, m_q = 1 << (N-1-q), J in itertools.combinations order.  The discrete map is the oracle's (``exponentials``: KRYLOV_SE: one per save interval at the right endpoint; DP5_SE: the CF4 pieces of
``helpers.magnus_cf4_dense``).  Everything is differentiable in J, the tables, u_pairs, tsave and psi0.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

from oracle import restatement as R

CD = torch.complex128


def pair_list(n: int) -> list:
    return list(itertools.combinations(range(n), 2))


def exchange_indices(n: int, mode: int):
    """Per pair: (rows of the stencil, their partner columns) as index tensors."""
    x = np.arange(2**n)
    out = []
    for i, j in pair_list(n):
        mi, mj = 1 << (n - 1 - i), 1 << (n - 1 - j)
        bi, bj = (x & mi) != 0, (x & mj) != 0
        rows = x[(~bi) & bj] if mode == 2 else x[bi != bj]
        out.append((torch.as_tensor(rows), torch.as_tensor(rows ^ mi ^ mj)))
    return out


def exchange_dense(n: int, J: torch.Tensor, mode: int) -> torch.Tensor:
    dim = 2**n
    X = torch.zeros(dim, dim, dtype=CD)
    for p, (rows, cols) in enumerate(exchange_indices(n, mode)):
        E = torch.zeros(dim, dim, dtype=CD)
        E[rows, cols] = 1.0
        X = X + J[p] * E
    return X


def exponentials(terms, tsave: torch.Tensor, solver) -> list:
    """Per save interval the (t, tau) of its exponentials exp(-i tau H(t)), in order, as tensors that keep tsave in the graph.
    KRYLOV_SE: one at the right endpoint.  DP5_SE: the CF4 scheme of ``helpers.magnus_cf4_dense`` at the native default sub-step."""
    from tests.helpers import DP5_DEFAULT_H_MAX

    name = getattr(solver, "name", str(solver))
    out = []
    dt, n = terms.dt, terms.n_samples
    for k in range(len(tsave) - 1):
        a, b = tsave[k], tsave[k + 1]
        if name == "KRYLOV_SE":
            out.append([(b, b - a)])
            continue
        fa, fb = float(a.detach()), float(b.detach())
        pts = [a]
        i = math.floor(fa / dt) + 1
        while i <= n - 2 and i * dt < fb - 1e-13:
            if i * dt > fa + 1e-13:
                pts.append(torch.tensor(i * dt, dtype=torch.float64))
            i += 1
        pts.append(b)
        steps = []
        for p0, p1 in zip(pts[:-1], pts[1:]):
            hf = p1 - p0
            S = max(1, math.ceil(float(hf.detach()) / DP5_DEFAULT_H_MAX - 1e-9))
            for sub in range(S):
                for theta in (1.0 / 6.0, 5.0 / 6.0):
                    steps.append((p0 + ((sub + theta) / S) * hf, hf / (2.0 * S)))
        out.append(steps)
    return out


def dense_map(terms: R.HamTerms, J: torch.Tensor, mode: int, psi0: torch.Tensor, tsave: torch.Tensor, solver) -> torch.Tensor:
    """States (n_t, dim, B) of the discrete map with dense matrix exponentials."""
    from tests.helpers import accurate_matrix_exp

    xmat = exchange_dense(terms.n_qubits, J, mode)
    psi, out = psi0, [psi0]
    for interval in exponentials(terms, tsave, solver):
        for t, tau in interval:
            psi = accurate_matrix_exp(-1j * (R.dense_hamiltonian(terms, t) + xmat) * tau) @ psi
        out.append(psi)
    return torch.stack(out)


class _Exchange(torch.autograd.Function):
    """X(J) v by gathers, pair by pair, with a hand-written backward (X^dagger g and dL/dJ_p = Re <g, E_p v>) so that autograd
    keeps one vector per application instead of one per pair.  stencil: per pair (rows, partner rows) of the forward stencil."""

    @staticmethod
    def forward(ctx, J, v, stencil):
        ctx.stencil = stencil
        ctx.save_for_backward(J, v)
        out = torch.zeros_like(v)
        for p, (rows, cols) in enumerate(stencil):
            out[rows] += J[p] * v[cols]
        return out

    @staticmethod
    def backward(ctx, g):
        J, v = ctx.saved_tensors
        gv = torch.zeros_like(v)
        gJ = torch.zeros_like(J)
        for p, (rows, cols) in enumerate(ctx.stencil):
            gr = g[rows]
            gv[cols] += J[p] * gr  # (J real: X^dagger moves the cotangent of a row to its partner)
            gJ[p] = (gr.conj() * v[cols]).sum().real
        return gJ, gv, None


class MatrixFree:
    """H(t) v without a matrix: diagonal, single-qubit flips, exchange gathers.  v: (dim, B)."""

    def __init__(self, terms: R.HamTerms, J: torch.Tensor, mode: int):
        self.terms, self.J, self.mode, self.n = terms, J, mode, terms.n_qubits
        n = self.n
        x = torch.arange(2**n)
        self.x = x
        self.occ = R.occupation_table(n)
        self.udiag = R.interaction_diagonal(n, terms.u_pairs)
        self.bits = [((x >> (n - 1 - q)) & 1).bool() for q in range(n)]
        self.stencil = exchange_indices(n, mode)

    def apply(self, t, v: torch.Tensor) -> torch.Tensor:
        tr, n = self.terms, self.n
        diag = self.udiag
        for coeff, targets in tr.det_terms():
            d = R.interp_coeff(coeff, t, tr.dt, tr.n_samples)
            for q in targets:
                diag = diag + 2.0 * d * self.occ[q]
        out = diag.to(CD)[:, None] * v
        for coeff, targets in tr.amp_terms():
            c = R.interp_coeff(coeff, t, tr.dt, tr.n_samples)
            for q in targets:
                part = v[self.x ^ (1 << (n - 1 - q))]
                out = out + torch.where(self.bits[q][:, None], c * part, torch.conj(c) * part)
        if self.stencil:
            out = out + _Exchange.apply(self.J, v, self.stencil)
        return out

    def bound(self) -> float:
        """A bound of ||H(t)|| over the run (Gershgorin rows, every table at its largest)."""
        from tests.helpers import gershgorin_half_width

        u = self.terms.u_pairs.detach().abs().sum()
        return float(2.0 * gershgorin_half_width(self.terms) + u + self.J.detach().abs().sum())

    def expm(self, t, tau, v: torch.Tensor) -> torch.Tensor:
        """exp(-i tau H(t)) v: Taylor series to 1e-14 of the vector's norm, in pieces of tau ||H|| <= 1 (no cancellation)."""
        pieces = max(1, int(math.ceil(abs(float(tau)) * self.bound())))
        h = tau / pieces
        for _ in range(pieces):
            term, acc = v, v
            for k in range(1, 60):
                term = self.apply(t, term) * (-1j * h / k)
                acc = acc + term
                if float(term.detach().abs().max()) < 1e-15 * float(acc.detach().abs().max()):
                    break
            v = acc
        return v


def matrix_free_map(terms: R.HamTerms, J: torch.Tensor, mode: int, psi0: torch.Tensor, tsave: torch.Tensor, solver) -> torch.Tensor:
    """``dense_map`` without matrices: states (n_t, dim, B)."""
    mf = MatrixFree(terms, J, mode)
    psi, out = psi0, [psi0]
    for interval in exponentials(terms, tsave, solver):
        for t, tau in interval:
            psi = mf.expm(t, tau, psi)
        out.append(psi)
    return torch.stack(out)


def couplings_from_dense(H_int: torch.Tensor, n: int) -> torch.Tensor:
    """J_ij read off the oracle's dense one-directional interaction matrix: the entry <u_i d_j ...| H |d_i u_j ...> (others u)."""
    return torch.stack([H_int[1 << (n - 1 - j), 1 << (n - 1 - i)].real for i, j in pair_list(n)]) if n > 1 else torch.zeros(0, dtype=torch.float64)
