"""Observables that are real-weighted sums of Pauli strings, ``O = sum_s w_s P_s`` — what the native solver evaluates and
differentiates next to diagonal tables (``include/rydiff.h``: ``RydProblem.pauli_*``; ``csrc/pauli_kernels.hpp``).

Conventions (the header's): a string is two qubit masks, bit j = qubit j (qubit 0 = first atom = most significant bit of the
amplitude index): ``x`` = the qubits carrying X or Y, ``z`` = the qubits carrying Z or Y.  The 2x2 matrices are the ones of
``utils.py`` (``XMAT / YMAT / ZMAT``) in the index order of the basis.  With ``xm``, ``zm`` the masks moved to index bits and
``ny = popcount(x & z)``::

    (P psi)[y] = i^ny * (-1)^popcount((y ^ xm) & zm) * psi[y ^ xm]
"""
from __future__ import annotations

import math
from typing import Iterable, Mapping, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

MAX_PAULI_STRINGS = 1024  # RYDIFF_MAX_PAULI_STRINGS
MAX_OVERLAPS = 16  # RYDIFF_MAX_OVERLAPS
MAX_RDMS = 8  # RYDIFF_MAX_RDMS
MAX_RDM_QUBITS = 6  # RYDIFF_MAX_RDM_QUBITS
MAX_DENSE_QUBITS = 14
_I_POW = (1.0, 1j, -1.0, -1j)


def _term_masks(n_qubits: int, paulis: Union[str, Mapping[int, str]]) -> tuple[int, int]:
    if isinstance(paulis, str):
        if len(paulis) != n_qubits:
            raise ValueError(f"Pauli string {paulis!r} must name one of I, X, Y, Z for each of the {n_qubits} qubits")
        paulis = {j: c for j, c in enumerate(paulis)}
    x = z = 0
    for j, c in paulis.items():
        j = int(j)
        if not 0 <= j < n_qubits:
            raise ValueError(f"qubit {j} is outside the register of {n_qubits} qubits")
        c = str(c).upper()
        if c not in "IXYZ" or len(c) != 1:
            raise ValueError(f"{c!r} is not one of I, X, Y, Z")
        if c in "XY":
            x |= 1 << j
        if c in "ZY":
            z |= 1 << j
    return x, z


class PauliObservable:
    """``PauliObservable(n_qubits, [(weight, {qubit: "X" | "Y" | "Z"}), (weight, "XIZY"), ...])``; equal strings are merged."""

    def __init__(self, n_qubits: int, terms: Iterable = ()):
        self.n_qubits = int(n_qubits)
        if self.n_qubits < 1:
            raise ValueError("n_qubits must be positive")
        self._terms: dict[tuple[int, int], float] = {}
        for weight, paulis in terms:
            if isinstance(weight, complex) and abs(weight.imag) > 0.0:
                raise ValueError("Pauli observables take real weights")
            key = _term_masks(self.n_qubits, paulis)
            self._terms[key] = self._terms.get(key, 0.0) + float(weight.real if isinstance(weight, complex) else weight)

    @classmethod
    def _from_masks(cls, n_qubits: int, terms: Mapping[tuple[int, int], float]) -> "PauliObservable":
        out = cls(n_qubits)
        out._terms = {k: float(v) for k, v in terms.items() if v != 0.0}
        return out

    # ---- algebra ------------------------------------------------------------------------------------------------------
    def __add__(self, other: "PauliObservable") -> "PauliObservable":
        if not isinstance(other, PauliObservable):
            return NotImplemented
        if other.n_qubits != self.n_qubits:
            raise ValueError("Pauli observables on registers of different size")
        terms = dict(self._terms)
        for k, v in other._terms.items():
            terms[k] = terms.get(k, 0.0) + v
        return PauliObservable._from_masks(self.n_qubits, terms)

    def __mul__(self, scalar) -> "PauliObservable":
        if isinstance(scalar, PauliObservable) or (isinstance(scalar, complex) and scalar.imag != 0.0):
            return NotImplemented
        s = float(scalar.real if isinstance(scalar, complex) else scalar)
        return PauliObservable._from_masks(self.n_qubits, {k: s * v for k, v in self._terms.items()})

    __rmul__ = __mul__

    def __neg__(self) -> "PauliObservable":
        return self * -1.0

    def __sub__(self, other: "PauliObservable") -> "PauliObservable":
        return self + (-other)

    def __len__(self) -> int:
        return len(self._terms)

    @property
    def terms(self) -> list[tuple[float, int, int]]:
        """``[(weight, x_mask, z_mask), ...]`` in a fixed order."""
        return [(w, x, z) for (x, z), w in sorted(self._terms.items())]

    # ---- what a dense tensor offers (simresults.expect validates ``shape``) --------------------------------------------------
    @property
    def shape(self) -> tuple:
        return (2**self.n_qubits, 2**self.n_qubits)

    @property
    def is_sparse(self) -> bool:
        return False

    def index_masks(self) -> list[tuple[float, int, int, complex]]:
        """``[(weight, xm, zm, i^ny), ...]`` with the masks on amplitude-index bits (qubit j -> bit N-1-j)."""
        n = self.n_qubits
        flip = lambda m: sum(1 << (n - 1 - j) for j in range(n) if m >> j & 1)  # noqa: E731
        return [(w, flip(x), flip(z), _I_POW[bin(x & z).count("1") & 3]) for w, x, z in self.terms]

    def to_dense(self) -> Tensor:
        if self.n_qubits > MAX_DENSE_QUBITS:
            raise ValueError(f"dense operators are limited to {MAX_DENSE_QUBITS} qubits")
        dim = 2**self.n_qubits
        y = torch.arange(dim)
        mat = torch.zeros(dim, dim, dtype=torch.complex128)
        for w, xm, zm, ph in self.index_masks():
            yp = y ^ xm
            mat[y, yp] += w * ph * _parity_sign(yp & zm)
        return mat

    def masks(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``(pauli_first, pauli_x, pauli_z, pauli_w)`` of this one observable as the C ABI takes them."""
        return pack_pauli([self], self.n_qubits)

    def rotated(self, phi: float) -> "PauliObservable":
        """``V O V^dagger`` for ``V = exp(i phi #ones)`` (the frame ``sesolve`` evolves in under one constant drive phase): per
        flipped qubit ``X -> cos X + sin Y``, ``Y -> cos Y - sin X``; Z and I unchanged."""
        c, s = math.cos(float(phi)), math.sin(float(phi))
        out: dict[tuple[int, int], float] = {}
        for (x, z), w in self._terms.items():
            parts = {(x, z): w}
            for j in range(self.n_qubits):
                if not x >> j & 1:
                    continue
                nxt: dict[tuple[int, int], float] = {}
                for (px, pz), pw in parts.items():
                    nxt[(px, pz)] = nxt.get((px, pz), 0.0) + c * pw
                    other = (px, pz ^ (1 << j))
                    nxt[other] = nxt.get(other, 0.0) + (-s if pz >> j & 1 else s) * pw
                parts = nxt
            for k, v in parts.items():
                out[k] = out.get(k, 0.0) + v
        return PauliObservable._from_masks(self.n_qubits, {k: v for k, v in out.items() if abs(v) > 0.0})

    def rotated_count(self) -> int:
        """Strings of ``rotated(phi)`` for a generic phi: 2^k for a string with k flipped qubits (before merging)."""
        return sum(2 ** bin(x).count("1") for (x, _z) in self._terms)


def _parity_sign(v: Tensor) -> Tensor:
    """(-1)^popcount(v) for an integer tensor, as float64."""
    p = torch.zeros_like(v)
    for j in range(32):
        p ^= (v >> j) & 1
    return 1.0 - 2.0 * p.to(torch.float64)


def pack_pauli(observables: Sequence[PauliObservable], n_qubits: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The host arrays of ``RydProblem.pauli_first / pauli_x / pauli_z / pauli_w`` for a list of observables."""
    first, xs, zs, ws = [0], [], [], []
    for obs in observables:
        if obs.n_qubits != n_qubits:
            raise ValueError(f"Pauli observable on {obs.n_qubits} qubits handed to a register of {n_qubits}")
        for w, x, z in obs.terms:
            xs.append(x)
            zs.append(z)
            ws.append(w)
        first.append(len(xs))
    packed = (np.asarray(first, dtype=np.int32), np.asarray(xs, dtype=np.uint32), np.asarray(zs, dtype=np.uint32),
              np.asarray(ws, dtype=np.float64))
    check_pauli(packed, n_qubits)
    return packed


def check_pauli(packed, n_qubits: int) -> None:
    """The C ABI sees raw pointers: counts, mask bits and the string cap are checked here (ValueError, never a bad device read)."""
    first, x, z, w = (np.asarray(a) for a in packed)
    if first.ndim != 1 or len(first) < 2 or first[0] != 0 or np.any(np.diff(first) < 0):
        raise ValueError("pauli_first must be a non-decreasing array starting at 0 with one entry per observable plus one")
    if not (len(x) == len(z) == len(w) == int(first[-1])):
        raise ValueError(f"pauli_x / pauli_z / pauli_w must hold pauli_first[-1] = {int(first[-1])} strings each")
    if len(x) > MAX_PAULI_STRINGS:
        raise ValueError(f"too many Pauli strings: {len(x)} (at most {MAX_PAULI_STRINGS} per call)")
    if len(x) and (int(np.max(x.astype(np.uint64) | z.astype(np.uint64))) >> n_qubits) != 0:
        raise ValueError(f"a Pauli string addresses a qubit at or above n_qubits = {n_qubits}")
    if len(w) and not np.all(np.isfinite(w)):
        raise ValueError("Pauli weights must be finite")


def expect_pauli(obs: PauliObservable, states: Tensor) -> Tensor:
    """``<O>`` by index arithmetic in torch (no 2^N x 2^N operator): kets ``(n_t, dim, B)`` or density matrices
    ``(n_t, dim, dim, B)``, on any device.  One gather per distinct flip mask."""
    dim = 2**obs.n_qubits
    if states.ndim not in (3, 4) or states.shape[1] != dim:
        raise ValueError(f"PauliObservable on {obs.n_qubits} qubits expects kets (n_t, {dim}, B) or density matrices (n_t, {dim}, {dim}, B)")
    dev = states.device
    y = torch.arange(dim, device=dev)
    by_flip: dict[int, Tensor] = {}
    for w, xm, zm, ph in obs.index_masks():
        coef = (w * ph) * _parity_sign((y ^ xm) & zm).to(torch.complex128)
        by_flip[xm] = by_flip[xm] + coef if xm in by_flip else coef
    cdt = states.dtype if states.is_complex() else torch.complex128
    out = torch.zeros(states.shape[0], dtype=cdt, device=dev)
    for xm, coef in by_flip.items():
        yp = y ^ xm
        coef = coef.to(cdt)
        if states.ndim == 3:  # sum_y conj(psi[y]) coef[y] psi[y ^ xm]
            out = out + (states.conj() * coef[None, :, None] * states[:, yp, :]).sum(dim=(1, 2))
        else:  # tr(O rho) = sum_y O[y, y ^ xm] rho[y ^ xm, y]
            out = out + (coef[None, :, None] * states[:, yp, y, :]).sum(dim=(1, 2))
    return out


class StateOverlap:
    """The complex overlap ``c[k][b] = <phi_b | psi_b(t_k)>`` with a target state — what fidelities are made of (state fidelity
    ``|c|^2``, gate fidelity ``|sum_b c_b| / dim``); evaluated and differentiated natively at every evaluation time
    (``include/rydiff.h``: ``RydProblem.overlap_*``; ``csrc/overlap_kernels.hpp``), no stored trajectory.

    ``targets``: ``(dim,)`` — one target shared by every trajectory of the batch — or ``(dim, B)``, one target per trajectory, in
    the reference's layout of kets (basis index first).  Targets are constants (no gradient) and need not be normalised.
    As an operator the observable is the projector ``|phi><phi|``: ``shape`` is ``(dim, dim)`` and ``results.expect`` gives
    ``sum_b |c_b|^2``; the overlaps themselves come from ``results.overlap``."""

    def __init__(self, targets):
        t = torch.as_tensor(targets)
        if not (t.is_complex() or t.is_floating_point()):
            raise TypeError(f"StateOverlap targets must be complex (or real floating point) amplitudes, got {t.dtype}")
        if t.ndim == 1:
            t = t.unsqueeze(1)
        if t.ndim != 2 or t.shape[0] < 2 or t.shape[1] < 1:
            raise ValueError(f"StateOverlap targets must have shape (dim,) or (dim, B) with dim >= 2, got {tuple(t.shape)}")
        self.targets = t.detach().to(torch.complex128)  # (dim, 1 | B)

    @property
    def shape(self) -> tuple:
        return (self.targets.shape[0], self.targets.shape[0])

    @property
    def batch(self) -> int:
        return int(self.targets.shape[1])

    @property
    def is_sparse(self) -> bool:
        return False

    def to(self, device) -> "StateOverlap":
        """Moves the targets (in place: the object keeps its identity, which is how results find its native values)."""
        self.targets = self.targets.to(device)
        return self


def overlap_states(obs: StateOverlap, states: Tensor) -> Tensor:
    """``c[k][b] = sum_y conj(phi_b[y]) psi[k][y][b]`` in torch on stored kets ``(n_t, dim, B)``; complex ``(n_t, B)``."""
    if states.is_sparse:
        states = states.to_dense()
    if states.ndim == 4:
        raise NotImplementedError("StateOverlap is defined on kets; density matrices (master-equation runs) are not supported")
    dim = obs.targets.shape[0]
    if states.ndim != 3 or states.shape[1] != dim:
        raise ValueError(f"StateOverlap with targets of dimension {dim} expects kets (n_t, {dim}, B), got {tuple(states.shape)}")
    if obs.batch not in (1, states.shape[2]):
        raise ValueError(f"StateOverlap holds {obs.batch} targets but the states have batch {states.shape[2]}")
    phi = obs.targets.to(states.device)
    return (phi.conj()[None, :, :] * states.to(torch.complex128)).sum(dim=1)


def pack_overlaps(observables: Sequence[StateOverlap], dim: int, batch: int, device=None) -> Tensor:
    """The ``(n_ov, 1 | B, dim)`` complex128 tensor of ``RydProblem.overlap_targets`` (``ProblemSpec.overlaps``): batch 1 when every
    observable shares its target over the trajectories, else ``B`` (shared targets repeated)."""
    observables = list(observables)
    if not observables:
        raise ValueError("no StateOverlap observable to pack")
    if len(observables) > MAX_OVERLAPS:
        raise ValueError(f"too many StateOverlap observables: {len(observables)} (at most {MAX_OVERLAPS} per call)")
    for o in observables:
        if not isinstance(o, StateOverlap):
            raise TypeError(f"expected StateOverlap objects, got {type(o)}")
        if o.targets.shape[0] != dim:
            raise ValueError(f"StateOverlap targets of dimension {o.targets.shape[0]} handed to states of dimension {dim}")
        if o.batch not in (1, batch):
            raise ValueError(f"StateOverlap holds {o.batch} targets: must be 1 or the batch size {batch}")
    bt = max(o.batch for o in observables)
    rows = [o.targets.to(device).transpose(0, 1).expand(bt, dim) for o in observables]
    return torch.stack(rows).contiguous()


class ReducedDensityMatrix:
    """The state of a subsystem, ``rho_A[a][a'] = sum_e psi[idx(a, e)] conj(psi[idx(a', e)])`` (``Tr_E |psi><psi|``, not normalised),
    for ``A`` = ``qubits``: 1 to 6 distinct qubit indices in any order; evaluated and differentiated natively at every evaluation time
    (``include/rydiff.h``: ``RydProblem.n_rdms / rdm_masks``; ``csrc/rdm_kernels.hpp``), no stored trajectory.

    The matrix index ``a`` enumerates the settings of ``qubits`` with the FIRST listed qubit most significant, in the basis order of
    the register (r = 0, g = 1).  The library works in ascending qubit order; other orders are a permutation of the small matrix,
    applied in torch.  Read the values with ``results.reduced_density_matrix`` / ``SolveResult.rdms``: complex ``(n_t, B, 2^m, 2^m)``.

    In a master-equation run the same object asks for the partial trace of the register's density matrix,
    ``rho_A[a][a'] = sum_e rho[idx(a, e)][idx(a', e)]`` (``RydProblem.n_dm_rdms / dm_rdm_masks``; ``csrc/dm_kernels.hpp``), with
    ``store_states=False``; ``MasterEquationResult.rdms`` holds the values."""

    def __init__(self, qubits):
        qs = tuple(int(q) for q in qubits)
        if not 1 <= len(qs) <= MAX_RDM_QUBITS:
            raise ValueError(f"a reduced density matrix takes 1 to {MAX_RDM_QUBITS} qubits, got {len(qs)}")
        if len(set(qs)) != len(qs):
            raise ValueError(f"the qubits of a reduced density matrix must be distinct, got {qs}")
        if min(qs) < 0:
            raise ValueError(f"negative qubit index in {qs}")
        self.qubits = qs

    @property
    def n_sub(self) -> int:
        return len(self.qubits)

    @property
    def shape(self) -> tuple:
        return (2 ** self.n_sub, 2 ** self.n_sub)

    @property
    def is_sparse(self) -> bool:
        return False

    @property
    def mask(self) -> int:
        """Bit j = qubit j, the convention of ``amp_masks``."""
        return sum(1 << q for q in self.qubits)

    def check(self, n_qubits: int) -> None:
        if max(self.qubits) >= n_qubits:
            raise ValueError(f"qubit {max(self.qubits)} is outside the register of {n_qubits} qubits")

    def native_index(self) -> Tensor:
        """``perm`` with ``rho_user = rho_native[perm][:, perm]``: for every index in the order of ``qubits`` the index in ascending
        qubit order (lowest-numbered qubit most significant), which is how the library lays the matrix out."""
        m = self.n_sub
        rank = {q: i for i, q in enumerate(sorted(self.qubits))}  # position in ascending order, 0 = most significant
        perm = torch.zeros(2 ** m, dtype=torch.long)
        for au in range(2 ** m):
            an = 0
            for i, q in enumerate(self.qubits):
                if au >> (m - 1 - i) & 1:
                    an |= 1 << (m - 1 - rank[q])
            perm[au] = an
        return perm


def reduced_density_matrix(obs: ReducedDensityMatrix, states: Tensor) -> Tensor:
    """The torch route on stored kets ``(n_t, dim, B)`` or stored density matrices ``(n_t, dim, dim, B)`` (the partial trace
    ``Tr_E rho``; no Hermiticity assumed): complex ``(n_t, B, 2^m, 2^m)``, differentiable, in the order of ``obs.qubits``."""
    if not isinstance(obs, ReducedDensityMatrix):
        raise TypeError(f"expected a ReducedDensityMatrix, got {type(obs)}")
    if states.is_sparse:
        states = states.to_dense()
    if states.ndim == 4:
        return _reduced_density_matrix_dm(obs, states)
    if states.ndim != 3:
        raise ValueError(f"expected kets (n_t, dim, B) or density matrices (n_t, dim, dim, B), got {tuple(states.shape)}")
    n_t, dim, batch = states.shape
    n = dim.bit_length() - 1
    if dim != 1 << n:
        raise ValueError(f"ReducedDensityMatrix needs a register of qubits (dim a power of two), got dim {dim}")
    obs.check(n)
    m = obs.n_sub
    rest = [q for q in range(n) if q not in obs.qubits]
    st = states.to(torch.complex128).reshape((n_t,) + (2,) * n + (batch,))
    st = st.permute([0] + [1 + q for q in obs.qubits] + [1 + q for q in rest] + [n + 1]).reshape(n_t, 2 ** m, 2 ** (n - m), batch)
    return torch.einsum("taeb,tceb->tbac", st, st.conj())


def _reduced_density_matrix_dm(obs: ReducedDensityMatrix, states: Tensor) -> Tensor:
    """``rho_A[a][a'] = sum_e rho[idx(a, e)][idx(a', e)]`` of stored density matrices ``(n_t, dim, dim, B)``."""
    n_t, dim, dim2, batch = states.shape
    n = dim.bit_length() - 1
    if dim != 1 << n or dim2 != dim:
        raise ValueError(f"ReducedDensityMatrix needs density matrices (n_t, 2^n, 2^n, B), got {tuple(states.shape)}")
    obs.check(n)
    m = obs.n_sub
    rest = [q for q in range(n) if q not in obs.qubits]
    order = list(obs.qubits) + rest
    st = states.to(torch.complex128).reshape((n_t,) + (2,) * (2 * n) + (batch,))
    st = st.permute([0] + [1 + q for q in order] + [1 + n + q for q in order] + [2 * n + 1])
    st = st.reshape(n_t, 2 ** m, 2 ** (n - m), 2 ** m, 2 ** (n - m), batch)
    return torch.einsum("taeceb->tbac", st)


def pack_rdms(observables: Sequence[ReducedDensityMatrix], n_qubits: int) -> np.ndarray:
    """The uint32 masks of ``RydProblem.rdm_masks`` (``ProblemSpec.rdms``)."""
    observables = list(observables)
    if not observables:
        raise ValueError("no ReducedDensityMatrix to pack")
    if len(observables) > MAX_RDMS:
        raise ValueError(f"too many reduced density matrices: {len(observables)} (at most {MAX_RDMS} per call)")
    for o in observables:
        if not isinstance(o, ReducedDensityMatrix):
            raise TypeError(f"expected ReducedDensityMatrix objects, got {type(o)}")
        o.check(n_qubits)
    return np.asarray([o.mask for o in observables], dtype=np.uint32)


class Purity:
    """``Tr rho^2`` of the register state at every evaluation time — handed to ``run(observables=[...])`` of a master-equation run
    it is evaluated (as ``sum |rho_xy|^2``) and differentiated natively (``include/rydiff.h``: ``RydProblem.dm_purity``); read it
    with ``results.purity()``.  Not an operator: ``results.expect`` does not take it."""


class OccupationCorrelations:
    """Every ``<n_i>`` and every ``<n_i n_j>`` of the register at every evaluation time, from one read of the state — handed to
    ``run(observables=[...])`` of a ket run it is evaluated and differentiated natively (``include/rydiff.h``:
    ``RydProblem.bit_moments``; ``csrc/moments_kernels.hpp``), no stored trajectory and no ``2^N`` table.  Read it with
    ``results.occupations()``, ``results.occupation_correlations(connected=...)`` and ``results.structure_factor(signs)``.  Not an
    operator: ``results.expect`` does not take it.  All qubits, or off: there is no subset.  A master-equation run with
    ``store_states=False`` serves it from the diagonal of rho (``RydProblem.dm_moments``; ``csrc/dm_kernels.hpp``: ``k_dm_moments``)."""


class Energy:
    """The energy of the state under the sequence's own Hamiltonian, ``E(t_k) = <psi(t_k)| H(t_k) |psi(t_k)>``, and (with
    ``second_moment=True``, the default) ``<H(t_k)^2> = |H(t_k) psi(t_k)|^2`` at every evaluation time — the score of a
    state-preparation or annealing sequence that needs no target state, and through the variance the distance from any eigenstate.
    Handed to ``run(observables=[...])`` of a ket run it is evaluated and differentiated natively (``include/rydiff.h``:
    ``RydProblem.energy_rows``; ``csrc/energy_kernels.hpp``): no stored trajectory, and ``H(t_k)`` is ``get_hamiltonian(t_k)`` — the
    tables interpolated at the evaluation times (``Hamiltonian.energy_tables``), so that gradients w.r.t. pulse parameters, the
    register and (``time_grad``) the evaluation times include the explicit dependence of ``H``.  Read it with ``results.energy()``,
    ``results.energy_second_moment()`` and ``results.energy_variance()``.  Not an operator: ``results.expect`` does not take it."""

    def __init__(self, second_moment: bool = True):
        self.second_moment = bool(second_moment)

    @property
    def rows(self) -> int:
        """Rows of the energy block: 1 (E) or 2 (E, then the second moment)."""
        return 2 if self.second_moment else 1


def moment_rows(n_qubits: int) -> int:
    """Rows of the moments block: ``1 + N + N(N-1)/2``."""
    return 1 + n_qubits + n_qubits * (n_qubits - 1) // 2


def moment_pair_row(n_qubits: int, q: int, r: int) -> int:
    """The row of ``B_qr`` (``q < r``) in the moments block: ``S``, the ``B_q``, then the pairs in lexicographic order."""
    if not 0 <= q < r < n_qubits:
        raise ValueError(f"a pair row needs 0 <= q < r < {n_qubits}, got ({q}, {r})")
    return 1 + n_qubits + q * (2 * n_qubits - q - 1) // 2 + (r - q - 1)


def occupation_moments(states: Tensor) -> Tensor:
    """The rows of ``RydProblem.bit_moments`` in torch on stored kets ``(n_t, dim, B)``: real ``(1 + N + N(N-1)/2, n_t, B)``,
    differentiable.  With ``p[y] = |psi[y]|^2`` and ``y_q`` the index bit of qubit ``q`` (index bit ``N-1-q``): ``S = sum p``, then
    ``B_q = sum p y_q`` in ascending ``q``, then ``B_qr = sum p y_q y_r`` in lexicographic ``(q, r)``."""
    if states.is_sparse:
        states = states.to_dense()
    if states.ndim == 4:
        raise NotImplementedError("OccupationCorrelations is defined on kets; density matrices (master-equation runs) are not supported")
    if states.ndim != 3:
        raise ValueError(f"expected kets (n_t, dim, B), got {tuple(states.shape)}")
    n_t, dim, batch = states.shape
    n = dim.bit_length() - 1
    if dim != 1 << n:
        raise ValueError(f"OccupationCorrelations needs a register of qubits (dim a power of two), got dim {dim}")
    p = states.real.to(torch.float64) ** 2 + states.imag.to(torch.float64) ** 2 if states.is_complex() else states.to(torch.float64) ** 2
    y = torch.arange(dim, device=states.device)
    bits = torch.stack([((y >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]) if n else torch.zeros(0, dim, dtype=torch.float64)
    rows = [p.sum(dim=1)[None]]
    if n:
        rows.append(torch.einsum("qy,tyb->qtb", bits, p))
    if n > 1:
        iq, ir = torch.triu_indices(n, n, offset=1, device=states.device)  # lexicographic (q, r), q < r
        rows.append(torch.einsum("ey,tyb->etb", bits[iq] * bits[ir], p))
    return torch.cat(rows, dim=0)


def dm_occupation_moments(rho: Tensor) -> Tensor:
    """The rows of ``RydProblem.dm_moments`` in torch on stored density matrices ``(n_t, dim, dim, B)``: real
    ``(1 + n + n(n-1)/2, n_t, B)``, differentiable.  With ``p[x] = Re rho[x][x]`` — as it is: no clamp, no Hermitian part, nothing
    but the real diagonal counts — and ``x_q`` the index bit of atom ``q`` (index bit ``n-1-q``): ``S = sum p``, then
    ``B_q = sum p x_q`` in ascending ``q``, then ``B_qr = sum p x_q x_r`` in lexicographic ``(q, r)``: the order of
    ``occupation_moments`` on kets, and equal to it on ``rho = |psi><psi|``."""
    if rho.is_sparse:
        rho = rho.to_dense()
    if rho.ndim != 4 or rho.shape[1] != rho.shape[2]:
        raise ValueError(f"expected density matrices (n_t, dim, dim, B), got {tuple(rho.shape)}")
    dim = rho.shape[1]
    n = dim.bit_length() - 1
    if dim != 1 << n:
        raise ValueError(f"OccupationCorrelations needs a register of qubits (dim a power of two), got dim {dim}")
    diag = torch.diagonal(rho, dim1=1, dim2=2)  # (n_t, B, dim)
    p = (diag.real if diag.is_complex() else diag).to(torch.float64).permute(0, 2, 1)  # (n_t, dim, B)
    x = torch.arange(dim, device=rho.device)
    bits = torch.stack([((x >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]) if n else torch.zeros(0, dim, dtype=torch.float64)
    rows = [p.sum(dim=1)[None]]
    if n:
        rows.append(torch.einsum("qy,tyb->qtb", bits, p))
    if n > 1:
        iq, ir = torch.triu_indices(n, n, offset=1, device=rho.device)  # lexicographic (q, r), q < r
        rows.append(torch.einsum("ey,tyb->etb", bits[iq] * bits[ir], p))
    return torch.cat(rows, dim=0)


def classical_gram(states: Tensor, tangents: Tensor) -> Tensor:
    """The "classical Gram matrix" of ``rydiff_forward_fisher`` in plain torch on stored vectors: ``states`` complex ``(..., dim)``,
    ``tangents`` complex ``(..., D, dim)`` (the same leading axes) -> real ``(..., 1 + D, 1 + D)``.  With ``u = psi / |psi|`` the
    phase of every amplitude, ``w_0 = |psi|`` and ``w_{1+d} = 2 Re(conj(u) dpsi_d)``, ``C_ij = sum_y w_i[y] w_j[y]`` — what
    ``geometry.classical_fisher_information`` takes.  The modulus is ``torch.abs`` on the complex amplitude (no ``|psi|^2`` that
    could underflow); an amplitude that is exactly zero contributes nothing (``w_i[y] = 0`` for every ``i``: the sum over the
    support).  The reference of the native route, and the route for users who hold states on the CPU."""
    if not states.is_complex() or not tangents.is_complex():
        raise TypeError("classical_gram takes complex states and tangents")
    if tangents.ndim != states.ndim + 1 or tangents.shape[:-2] != states.shape[:-1] or tangents.shape[-1] != states.shape[-1]:
        raise ValueError(f"expected states (..., dim) and tangents (..., D, dim), got {tuple(states.shape)} and {tuple(tangents.shape)}")
    mod = torch.abs(states)
    support = mod > 0
    phase = torch.where(support, states / torch.where(support, mod, torch.ones_like(mod)), torch.zeros_like(states))
    w = torch.cat([mod[..., None, :], 2.0 * (phase.conj()[..., None, :] * tangents).real], dim=-2)  # (..., 1 + D, dim)
    return torch.einsum("...iy,...jy->...ij", w, w)


def fidelity_states(obs: StateOverlap, states: Tensor) -> Tensor:
    """``<phi_b| rho_b(t_k) |phi_b>`` in torch, real ``(n_t, B)``: stored density matrices ``(n_t, dim, dim, B)``, or kets
    ``(n_t, dim, B)`` (``|<phi|psi>|^2``).  The real part of the bilinear form, as the library takes it (no Hermiticity assumed)."""
    if states.is_sparse:
        states = states.to_dense()
    if states.ndim == 3:
        return overlap_states(obs, states).abs() ** 2
    dim = obs.targets.shape[0]
    if states.ndim != 4 or states.shape[1] != dim or states.shape[2] != dim:
        raise ValueError(f"StateOverlap with targets of dimension {dim} expects density matrices (n_t, {dim}, {dim}, B), got {tuple(states.shape)}")
    if obs.batch not in (1, states.shape[3]):
        raise ValueError(f"StateOverlap holds {obs.batch} targets but the states have batch {states.shape[3]}")
    phi = obs.targets.to(states.device).expand(dim, states.shape[3])
    return torch.einsum("xb,txyb,yb->tb", phi.conj(), states.to(torch.complex128), phi).real


def purity_states(states: Tensor) -> Tensor:
    """``Tr rho^2`` in torch, real ``(n_t, B)``: ``sum |rho_xy|^2`` of stored density matrices ``(n_t, dim, dim, B)`` (the library's
    row: equal to the trace for Hermitian rho), ``<psi|psi>^2`` of kets ``(n_t, dim, B)``."""
    if states.is_sparse:
        states = states.to_dense()
    if states.ndim == 4:
        return (states.real ** 2 + states.imag ** 2).sum(dim=(1, 2))
    if states.ndim != 3:
        raise ValueError(f"expected kets (n_t, dim, B) or density matrices (n_t, dim, dim, B), got {tuple(states.shape)}")
    return (states.real ** 2 + states.imag ** 2).sum(dim=1) ** 2


MAX_DM_ATOMS = 12  # RYDIFF_MAX_DM_ATOMS
MAX_DM_DIAG = 64  # RYDIFF_MAX_DM_DIAG


class DensityMatrixObservables:
    """The density-matrix block of ``RydProblem`` (``include/rydiff.h``: ``dm_*``) as ``ProblemSpec.dm`` carries it: the register
    is the doubled register of ``n_atoms`` atoms, ``vec(rho)[x * 2^n + y] = rho[x][y]``, and these functionals of rho are evaluated
    (and differentiated) natively at every evaluation time.  Their rows follow all other rows of ``expect``, in this order:

    ``diag``     float64 DEVICE tensor ``(n_diag, 2^n)``: ``sum_x o[x] Re rho[x][x]``
    ``pauli``    list of ``PauliObservable`` on ``n_atoms`` qubits (or the four packed host arrays): ``Re Tr(O rho)``
    ``targets``  complex128 DEVICE tensor ``(n_fid, 1 | B, 2^n)`` (``pack_overlaps``): ``Re <phi|rho|phi>``; constants
    ``purity``   one row ``sum |rho_xy|^2``
    ``rdms``     list of ``ReducedDensityMatrix`` over the ATOMS (or raw masks, bit j = atom j): ``2 * 4^m`` rows each, Re / Im of
                 every entry of ``Tr_E rho`` in ascending atom order (``solver.split_observables`` takes them out)
    ``shots``    the shots of ``ProblemSpec.shots`` are drawn from ``max(Re rho[x][x], 0)`` (atom indices ``x < 2^n``)
    ``moments``  the occupation correlations of the diagonal (``RydProblem.dm_moments``): ``1 + n + n(n-1)/2`` rows ``S``, ``B_q``,
                 ``B_qr`` of ``Re rho[x][x]``, the last rows of all (``solver.split_dm_moments`` takes them off the end)"""

    def __init__(self, n_atoms: int, diag=None, pauli=None, targets=None, purity: bool = False, shots: bool = False, rdms=None,
                 moments: bool = False):
        self.n_atoms = int(n_atoms)
        self.moments = bool(moments)
        self.rdms = None if rdms is None or len(rdms) == 0 else list(rdms)
        self.diag = diag
        self.pauli = pauli
        self.targets = targets
        self.purity = bool(purity)
        self.shots = bool(shots)

    @property
    def n_diag(self) -> int:
        return 0 if self.diag is None else int(self.diag.shape[0])

    @property
    def n_fid(self) -> int:
        return 0 if self.targets is None else int(self.targets.shape[0])

    def packed_pauli(self):
        """The four host arrays of ``RydProblem.dm_pauli_*`` (None: no Pauli rows); validated like the library does."""
        if self.pauli is None or len(self.pauli) == 0:
            return None
        if all(isinstance(o, PauliObservable) for o in self.pauli):
            return pack_pauli(list(self.pauli), self.n_atoms)
        if len(self.pauli) != 4:
            raise ValueError("DensityMatrixObservables.pauli: a list of PauliObservable or (pauli_first, pauli_x, pauli_z, pauli_w)")
        packed = (np.ascontiguousarray(self.pauli[0], dtype=np.int32), np.ascontiguousarray(self.pauli[1], dtype=np.uint32),
                  np.ascontiguousarray(self.pauli[2], dtype=np.uint32), np.ascontiguousarray(self.pauli[3], dtype=np.float64))
        check_pauli(packed, self.n_atoms)
        return packed

    @property
    def n_pauli(self) -> int:
        packed = self.packed_pauli()
        return 0 if packed is None else len(packed[0]) - 1

    def packed_rdms(self) -> Optional[np.ndarray]:
        """The host array of ``RydProblem.dm_rdm_masks`` (None: no reduced density matrices); validated like the library does."""
        if self.rdms is None:
            return None
        if not 1 <= len(self.rdms) <= MAX_RDMS:
            raise ValueError(f"DensityMatrixObservables.rdms: 1 to {MAX_RDMS} reduced density matrices per call, got {len(self.rdms)}")
        masks = []
        for o in self.rdms:
            if isinstance(o, ReducedDensityMatrix):
                o.check(self.n_atoms)
                masks.append(o.mask)
                continue
            try:
                v = int(o)
            except (TypeError, ValueError):
                raise TypeError(f"DensityMatrixObservables.rdms: ReducedDensityMatrix objects or integer masks, got {type(o)}") from None
            if v <= 0 or v >> self.n_atoms or bin(v).count("1") > MAX_RDM_QUBITS:
                raise ValueError(f"DensityMatrixObservables.rdms: mask {v:#x} must name 1 to {MAX_RDM_QUBITS} atoms below {self.n_atoms}")
            masks.append(v)
        return np.asarray(masks, dtype=np.uint32)

    def rdm_rows(self) -> int:
        """Rows the reduced density matrices take: 2 * sum_o 4^{m_o}."""
        masks = self.packed_rdms()
        return 0 if masks is None else sum(2 * 4 ** bin(int(v)).count("1") for v in masks)

    def rows(self) -> int:
        return self.n_diag + self.n_pauli + self.n_fid + int(self.purity) + self.rdm_rows() + self.moment_rows()

    def moment_rows(self) -> int:
        """Rows of the occupation correlations of the diagonal: ``1 + n + n(n-1)/2``, or 0."""
        return moment_rows(self.n_atoms) if self.moments else 0

    def check(self, n_qubits: int, batch: int, device=None) -> None:
        """Every buffer against the register (the C ABI sees raw pointers): ValueError, never a bad device read."""
        n, dim = self.n_atoms, 2 ** self.n_atoms
        if not 1 <= n <= MAX_DM_ATOMS or n_qubits != 2 * n:
            raise ValueError(f"a density-matrix register of {n} atoms (1 to {MAX_DM_ATOMS}) needs n_qubits = {2 * n}, got {n_qubits}")
        for name, t, dtype, cap in (("diag", self.diag, torch.float64, MAX_DM_DIAG), ("targets", self.targets, torch.complex128, MAX_OVERLAPS)):
            if t is None:
                continue
            if not isinstance(t, Tensor) or t.dtype != dtype or t.shape[-1] != dim or t.ndim != (2 if name == "diag" else 3):
                raise ValueError(f"DensityMatrixObservables.{name}: a {dtype} tensor with last dimension {dim}, got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
            if not 1 <= t.shape[0] <= cap:
                raise ValueError(f"DensityMatrixObservables.{name}: 1 to {cap} entries, got {t.shape[0]}")
            if device is not None and t.device != torch.device(device):
                raise ValueError(f"DensityMatrixObservables.{name} must live on the device of the states ({device}), got {t.device}")
        if self.targets is not None and self.targets.shape[1] not in (1, batch):
            raise ValueError(f"DensityMatrixObservables.targets: the target batch must be 1 or the batch size {batch}, got {self.targets.shape[1]}")
        self.packed_pauli()
        self.packed_rdms()


def dm_trace_indices(obs: PauliObservable):
    """The index and phase arithmetic of the library's Pauli rows on a density matrix, as numpy arrays per string:
    ``[(weight, rows, cols, phase), ...]`` with ``Tr(P rho) = sum_x phase[x] * rho[rows[x], cols[x]]``, ``rows = x ^ xm``,
    ``cols = x``, ``phase[x] = i^ny (-1)^popcount((x ^ xm) & zm)``."""
    dim = 2 ** obs.n_qubits
    x = np.arange(dim)
    out = []
    for w, xm, zm, ph in obs.index_masks():
        xp = x ^ xm
        par = np.zeros(dim, dtype=np.int64)
        for j in range(obs.n_qubits):
            par ^= ((xp & zm) >> j) & 1
        out.append((w, xp, x, ph * (1.0 - 2.0 * par)))
    return out
