"""Quantum geometry from the Gram matrices of the tangent sweep (``solver.evolve_geometry``, ``rydiff_forward_geometry``).

``gram[..., i, j] = <v_i|v_j>`` with ``v_0 = psi`` and ``v_{1+d} = d psi / d theta_d`` (conjugate on the left index).  The helpers
below are plain torch on the small matrices — they take CPU and GPU tensors alike and any leading axes — and hold for unnormalised
states (``N = <psi|psi> = gram[..., 0, 0]``):

    quantum geometric tensor     Q_de = <d_d psi|d_e psi> / N - <d_d psi|psi><psi|d_e psi> / N^2
    quantum Fisher information   F = 4 Re Q      (the Cramer-Rao bound of a pulse sequence used as a sensor; the natural-gradient metric)
    Berry curvature              -2 Im Q
"""
from __future__ import annotations

from dataclasses import dataclass

from torch import Tensor

SWEEP_DIRECTIONS = 8  # directions of one native sweep (RYDIFF_MAX_TANGENTS)
GROUP_DIRECTIONS = 4  # more than one sweep: groups of this many directions, one sweep per unordered pair of groups


def geometry_sweeps(n_dir: int) -> list[list[int]]:
    """The direction indices of every native sweep that ``evolve_geometry`` runs for ``n_dir`` directions.  Up to 8 directions are
    one sweep.  Beyond that the Gram matrix needs every PAIR of directions in some sweep: the directions are split into groups of at
    most 4 and every unordered pair of groups (a, b) is one sweep of at most 8 directions, which fills the blocks (a, a), (a, b) and
    (b, b)."""
    if n_dir < 1:
        raise ValueError(f"n_dir must be at least 1, got {n_dir}")
    if n_dir <= SWEEP_DIRECTIONS:
        return [list(range(n_dir))]
    groups = [list(range(d0, min(n_dir, d0 + GROUP_DIRECTIONS))) for d0 in range(0, n_dir, GROUP_DIRECTIONS)]
    return [groups[a] + groups[b] for a in range(len(groups)) for b in range(a + 1, len(groups))]


def quantum_geometric_tensor(gram: Tensor) -> Tensor:
    """``(..., 1 + D, 1 + D)`` Gram matrices -> the complex ``(..., D, D)`` quantum geometric tensor."""
    if gram.ndim < 2 or gram.shape[-1] != gram.shape[-2] or gram.shape[-1] < 2:
        raise ValueError(f"gram must be (..., 1 + D, 1 + D) with D >= 1, got {tuple(gram.shape)}")
    norm = gram[..., 0, 0].real[..., None, None]
    return gram[..., 1:, 1:] / norm - gram[..., 1:, :1] * gram[..., :1, 1:] / norm ** 2


def quantum_fisher_information(gram: Tensor) -> Tensor:
    """``F = 4 Re Q``: real ``(..., D, D)``."""
    return 4.0 * quantum_geometric_tensor(gram).real


def berry_curvature(gram: Tensor) -> Tensor:
    """``-2 Im Q``: real antisymmetric ``(..., D, D)``."""
    return -2.0 * quantum_geometric_tensor(gram).imag


@dataclass
class QuantumGeometry:
    """What ``TorchEmulator.run_quantum_fisher`` returns.  With D scalar entries in the request ``x`` (in the order of ``x``, each
    tensor flattened): ``gram`` (n_t, 1 + D, 1 + D) complex, ``qgt`` (n_t, D, D) complex, ``qfi`` and ``berry`` (n_t, D, D) real — with
    several columns in the initial state every one of them carries a batch axis behind the time axis, (n_t, B, ...): the geometry of
    a batch is per state.  ``values`` (n_obs, n_t) and ``grads[i]`` (n_obs, n_t, *x[i].shape) are shaped as in ``Sensitivities``
    (empty when no observables were given; a ``StateOverlap`` contributes two rows, Re and Im).  ``route`` is "tangent"."""

    gram: Tensor
    qgt: Tensor
    qfi: Tensor
    berry: Tensor
    values: Tensor
    grads: list
    route: str
    times: Tensor
