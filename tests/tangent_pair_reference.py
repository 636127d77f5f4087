"""Dense forward-mode reference of the tangent sweep on kets WITH dense pair terms: tests.helpers.tangent_dense_reference with
sum_p embed(T_p) added to R.dense_hamiltonian inside the block-exponential identity
    exp([[A, dA], [0, A]]) = [[e^A, L], [0, e^A]],   psi' = e^A psi,   dpsi' = e^A dpsi + L psi,      A = -i tau (H(t) + P),
with dA = -i tau dH_d(t) unchanged: the pair blocks are constants in every direction.  No autograd.

Up to 2^6 amplitudes the block matrix is exponentiated densely (tests.helpers.accurate_matrix_exp, as in the helper this is a variant
of).  Beyond, exp([[A, dA], [0, A]]) is APPLIED to the stacked vector [dpsi; psi] — the same identity, read column by column — by
scaling and a Taylor sum on vectors (`expm_action`): at 8 and 10 qubits the dense route would exponentiate 512 x 512 and 2048 x 2048 matrices per
direction and exponential.  tests/test_dm_tangent_host.py checks the two routes against each other."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import restatement as R
from tests.helpers import DP5_DEFAULT_H_MAX, _direction_terms, accurate_matrix_exp, map_exponentials

DENSE_EXP_MAX_DIM = 64


def embed_pair(n_qubits: int, qa: int, qb: int, block) -> torch.Tensor:
    """The 2^n x 2^n matrix of a dense pair term (include/rydiff.h): qubit q is bit n - 1 - q of the amplitude index, the block's
    index is 2 * bit_a + bit_b, and (P v)[x] = sum_s T[own(x)][s] v[x with the pair's bits set to s]."""
    dim = 2 ** n_qubits
    t = np.asarray(block, dtype=complex).reshape(4, 4)
    ma, mb = 1 << (n_qubits - 1 - qa), 1 << (n_qubits - 1 - qb)
    x = np.arange(dim)
    own = 2 * ((x & ma) != 0) + ((x & mb) != 0)
    out = np.zeros((dim, dim), dtype=complex)
    for s in range(4):
        xs = (x & ~(ma | mb)) | (ma if s & 2 else 0) | (mb if s & 1 else 0)
        out[x, xs] += t[own, s]
    return torch.from_numpy(out)


def pair_matrix(n_qubits: int, pair_terms) -> torch.Tensor:
    out = torch.zeros(2 ** n_qubits, 2 ** n_qubits, dtype=torch.complex128)
    for qa, qb, block in pair_terms:
        out += embed_pair(n_qubits, qa, qb, block)
    return out


def expm_action(a: torch.Tensor, da: torch.Tensor, psi: torch.Tensor, dpsi: torch.Tensor):
    """exp([[a, da_d], [0, a]]) applied to [dpsi_d; psi]: returns (e^a psi, e^a dpsi_d + L_d psi).  a (dim, dim), da (n_dir, dim, dim),
    psi (dim, B), dpsi (n_dir, dim, B).  Scaling by 1 / reps to a 1-norm of at most 2, then a Taylor sum of 40 terms on the vectors
    (largest term 2, remainder below 2^41 / 41! ~ 7e-38: no cancellation to speak of), repeated reps times."""
    n_dir, dim, batch = dpsi.shape
    norm = float(torch.linalg.matrix_norm(a, 1)) + float(torch.linalg.matrix_norm(da, 1).max())
    reps = max(1, math.ceil(norm / 2.0))
    a_s, da_s = a / reps, da / reps
    for _ in range(reps):
        tp, td = psi, dpsi  # the Taylor term of the lower / upper half
        out_p, out_d = psi.clone(), dpsi.clone()
        for k in range(1, 41):
            flat = td.permute(1, 0, 2).reshape(dim, n_dir * batch)  # one product with a for all directions
            td = ((a_s @ flat).reshape(dim, n_dir, batch).permute(1, 0, 2) + da_s @ tp) / k
            tp = (a_s @ tp) / k
            out_p = out_p + tp
            out_d = out_d + td
        psi, dpsi = out_p, out_d
    return psi, dpsi


def tangent_pair_reference(terms, pair_terms, d_amp, d_det, d_u, psi0, d_psi0, tsave, solver, h_max=DP5_DEFAULT_H_MAX, dense=None):
    """States (n_t, dim, B) and tangent states (n_t, n_dir, dim, B) of the oracle's discrete map (tests.helpers.map_exponentials) of
    H(t) + sum_p embed(T_p), shared tables.  d_amp (n_dir, Ka, n) | None, d_det (n_dir, Kd, n) | None, d_u (n_dir, n_pairs) | None,
    psi0 (dim, B), d_psi0 (n_dir, dim, B) | None.  `dense`: force the dense block exponential (True) or the vector action (False)."""
    psi = psi0.to(torch.complex128)
    dim, batch = psi.shape
    given = [t for t in (d_amp, d_det, d_u, d_psi0) if t is not None]
    n_dir = int(given[0].shape[0])
    if dense is None:
        dense = dim <= DENSE_EXP_MAX_DIM
    pmat = pair_matrix(terms.n_qubits, pair_terms)
    dirs = [_direction_terms(terms, None if d_amp is None else d_amp[d], None if d_det is None else d_det[d],
                             None if d_u is None else d_u[d]) for d in range(n_dir)]
    dpsi = d_psi0.to(torch.complex128) if d_psi0 is not None else torch.zeros(n_dir, dim, batch, dtype=torch.complex128)
    states, tangents = [psi], [dpsi]
    for steps in map_exponentials(terms, tsave, solver, h_max):
        for t, tau in steps:
            a = -1j * tau * (R.dense_hamiltonian(terms, t) + pmat)
            da = torch.stack([-1j * tau * R.dense_hamiltonian(dirs[d], t) for d in range(n_dir)])
            if dense:
                blk = torch.zeros(n_dir, 2 * dim, 2 * dim, dtype=torch.complex128)
                blk[:, :dim, :dim] = a
                blk[:, dim:, dim:] = a
                blk[:, :dim, dim:] = da
                e = accurate_matrix_exp(blk)
                ea, el = e[0, :dim, :dim], e[:, :dim, dim:]
                dpsi = ea @ dpsi + el @ psi
                psi = ea @ psi
            else:
                psi, dpsi = expm_action(a, da, psi, dpsi)
        states.append(psi)
        tangents.append(dpsi)
    return torch.stack(states), torch.stack(tangents)
