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
from typing import Optional

import torch
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


def place_sweep_block(full: Tensor, idx: list, block: Tensor) -> None:
    """Write the (..., 1 + len(idx), 1 + len(idx)) matrix `block` of the sweep over the directions `idx` into the
    (..., 1 + n_dir, 1 + n_dir) matrix `full`: row / column 0 is the state, 1 + d direction d.  The assembly of ``evolve_geometry``
    and ``evolve_fisher`` for more than one sweep (``geometry_sweeps``)."""
    sel = torch.tensor([0] + [1 + i for i in idx], device=full.device)
    full[..., sel[:, None], sel[None, :]] = block


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


def classical_fisher_information(cgram: Tensor) -> Tensor:
    """``(..., 1 + D, 1 + D)`` classical Gram matrices (``solver.evolve_fisher``, ``observables.classical_gram``) -> the real
    ``(..., D, D)`` classical Fisher information of the occupation-basis measurement, ``F_C,de = sum_y d_d p(y) d_e p(y) / p(y)`` with
    ``p(y) = |psi[y]|^2 / S``:  ``F_C = C[1:, 1:] / S - C[1:, 0] C[0, 1:] / S^2``, ``S = C_00`` (valid for unnormalised states)."""
    if cgram.ndim < 2 or cgram.shape[-1] != cgram.shape[-2] or cgram.shape[-1] < 2:
        raise ValueError(f"cgram must be (..., 1 + D, 1 + D) with D >= 1, got {tuple(cgram.shape)}")
    if cgram.is_complex():
        raise TypeError("cgram is the real classical Gram matrix; the complex Gram matrix goes to quantum_fisher_information")
    norm = cgram[..., 0, 0][..., None, None]
    return cgram[..., 1:, 1:] / norm - cgram[..., 1:, :1] * cgram[..., :1, 1:] / norm ** 2


def fisher_efficiency(cgram: Tensor, gram: Tensor, direction: Optional[Tensor] = None) -> Tensor:
    """``F_C / F_Q``, the share of the quantum Cramer-Rao bound the occupation-basis measurement reaches: per diagonal entry
    ``(..., D)``, or with ``direction`` (a real vector of D entries) along it, ``n.F_C.n / n.F_Q.n`` of shape ``(...)``.  Where both
    are zero (the state does not depend on the parameter) the ratio is NaN."""
    fc, fq = classical_fisher_information(cgram), quantum_fisher_information(gram)
    if direction is None:
        num, den = torch.diagonal(fc, dim1=-2, dim2=-1), torch.diagonal(fq, dim1=-2, dim2=-1)
    else:
        n = torch.as_tensor(direction, dtype=fc.dtype, device=fc.device)
        if n.ndim != 1 or n.shape[0] != fc.shape[-1]:
            raise ValueError(f"direction must be a vector of {fc.shape[-1]} entries, got {tuple(n.shape)}")
        num, den = torch.einsum("d,...de,e->...", n, fc, n), torch.einsum("d,...de,e->...", n, fq, n)
    return num / den  # 0 / 0 = NaN


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


@dataclass
class MeasurementFisher:
    """What ``TorchEmulator.run_classical_fisher`` returns.  With D scalar entries in the request ``x`` (in the order of ``x``, each
    tensor flattened): ``cgram`` (n_t, 1 + D, 1 + D) real, the classical Gram matrix of the occupation-basis measurement, ``cfi``
    (n_t, D, D) its classical Fisher information, ``gram`` (n_t, 1 + D, 1 + D) complex and ``qfi`` (n_t, D, D) the quantum ones of
    the same sweep (``cfi <= qfi`` as matrices) — with several columns in the initial state every one of them carries a batch axis
    behind the time axis, (n_t, B, ...).  ``values``, ``grads``, ``route`` and ``times`` as in ``QuantumGeometry``."""

    cgram: Tensor
    cfi: Tensor
    gram: Tensor
    qfi: Tensor
    values: Tensor
    grads: list
    route: str
    times: Tensor
