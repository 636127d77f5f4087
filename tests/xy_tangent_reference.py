"""Dense forward-mode reference of the tangent sweep on kets WITH the native XY exchange (RydProblem.xy_mode, RYDIFF_TANGENT_XY): the
block identity of tests/tangent_pair_reference.py,
    exp([[a, da], [0, a]]) = [[e^a, L], [0, e^a]],   psi' = e^a psi,   dpsi' = e^a dpsi + L psi,
with  a = -i tau (H(t) + X(J))  and  da_d = -i tau (dH_d(t) + X(dJ_d)):  unlike dense pair blocks, which are constants in every
direction, the couplings have tangents of their own.  X(.) is tests.xy_exchange_reference.exchange_dense (mode 1 or 2), the
exponentials those of the oracle's discrete map (tests.helpers.map_exponentials).  No autograd.

Up to 2^6 amplitudes the block matrix is exponentiated densely (tests.helpers.accurate_matrix_exp); beyond, it is applied to the
stacked vector by tests.tangent_pair_reference.expm_action.  tests/test_xy_tangent_host.py checks the reference against
tangent_pair_reference (dJ = 0) and against reverse-mode autograd through xy_exchange_reference.dense_map."""
from __future__ import annotations

import itertools

import numpy as np
import torch

from oracle import restatement as R
from tests.helpers import DP5_DEFAULT_H_MAX, _direction_terms, accurate_matrix_exp, map_exponentials
from tests.tangent_pair_reference import DENSE_EXP_MAX_DIM, expm_action
from tests.xy_exchange_reference import exchange_dense


def xy_tangent_reference(terms, J, mode, d_amp, d_det, d_u, d_xy, psi0, d_psi0, tsave, solver, h_max=DP5_DEFAULT_H_MAX, dense=None):
    """States (n_t, dim, B) and tangent states (n_t, n_dir, dim, B) of the discrete map of H(t) + X(J).
      terms   HamTerms shared by the trajectories, or a list of B HamTerms (per-trajectory tables)
      J       (n_pairs,) real, itertools.combinations order;  mode 1 (Hermitian) or 2 (one-directional)
      d_amp   (n_dir, Ka, n) complex | (n_dir, B, Ka, n) per trajectory | None;  d_det likewise, real
      d_u     (n_dir, n_pairs) | None;  d_xy (n_dir, n_pairs) | None: the tangents of J
      psi0    (dim, B);  d_psi0 (n_dir, dim, B) | None
    `dense`: force the dense block exponential (True) or the vector action (False)."""
    per_traj = isinstance(terms, (list, tuple))
    psi0 = psi0.to(torch.complex128)
    dim, batch = psi0.shape
    given = [t for t in (d_amp, d_det, d_u, d_xy, d_psi0) if t is not None]
    n_dir = int(given[0].shape[0])
    first = terms[0] if per_traj else terms
    n = first.n_qubits
    if dense is None:
        dense = dim <= DENSE_EXP_MAX_DIM
    xmat = exchange_dense(n, J.to(torch.float64), mode)
    dxmat = [exchange_dense(n, d_xy[d].to(torch.float64), mode) if d_xy is not None else torch.zeros(dim, dim, dtype=torch.complex128)
             for d in range(n_dir)]
    groups = [(terms[b], [b]) for b in range(batch)] if per_traj else [(terms, list(range(batch)))]
    n_t = len(tsave)
    states = torch.zeros(n_t, dim, batch, dtype=torch.complex128)
    tangents = torch.zeros(n_t, n_dir, dim, batch, dtype=torch.complex128)

    def table(t, d, b):  # direction d of a table tangent, for trajectory b
        if t is None:
            return None
        return t[d, b] if t.ndim == 4 else t[d]

    for g_terms, cols in groups:
        dirs = [_direction_terms(g_terms, table(d_amp, d, cols[0]), table(d_det, d, cols[0]), None if d_u is None else d_u[d])
                for d in range(n_dir)]
        psi = psi0[:, cols]
        dpsi = (d_psi0[:, :, cols].to(torch.complex128) if d_psi0 is not None
                else torch.zeros(n_dir, dim, len(cols), dtype=torch.complex128))
        states[0][:, cols] = psi
        tangents[0][:, :, cols] = dpsi
        for k, steps in enumerate(map_exponentials(g_terms, tsave, solver, h_max)):
            for t, tau in steps:
                a = -1j * tau * (R.dense_hamiltonian(g_terms, t) + xmat)
                da = torch.stack([-1j * tau * (R.dense_hamiltonian(dirs[d], t) + dxmat[d]) for d in range(n_dir)])
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
            states[k + 1][:, cols] = psi
            tangents[k + 1][:, :, cols] = dpsi
    return states, tangents


def pair_blocks(n: int, J, mode: int) -> tuple:
    """J as dense pair blocks (include/rydiff.h): block [1][2] = J, plus [2][1] = J in mode 1."""
    out = []
    for p, (a, b) in enumerate(itertools.combinations(range(n), 2)):
        blk = np.zeros((4, 4), dtype=np.complex128)
        blk[1, 2] = float(J[p])
        if mode == 1:
            blk[2, 1] = float(J[p])
        out.append((a, b, blk))
    return tuple(out)
