"""Master-equation path (``SolverType.DP5_ME``; ``pulser_diff/backend.py:495-509`` + the collapse operators of
``pulser_diff/hamiltonian.py:98-143``) on the native Schroedinger machinery.

The reference hands H(t) and a list of 2^N x 2^N collapse operators to ``pyqtorch.mesolve``.  Here the density matrix is the
state vector of a DOUBLED register — row qubits 0..N-1, column qubits N..2N-1, vec(rho)[x * 2^N + y] = rho[x, y] — and

    d vec(rho)/dt = -i M(t) vec(rho),      M = (H (x) 1  -  1 (x) H^T)  +  i * D

  * the commutator part is an ordinary structured Rydberg "Hamiltonian" on 2N qubits: every drive term appears twice, with
    coefficient c on the row qubits and -conj(c) on the column qubits; detunings +delta / -delta; pair interactions +U_ij
    among row qubits, -U_ij among column qubits, none across — built with torch ops, so gradients w.r.t. pulse parameters,
    distances and evaluation times flow through the same adjoint sweep as for kets;
  * the dissipator D = sum_k ( L_k (x) conj(L_k) - 1/2 L_k^dag L_k (x) 1 - 1/2 1 (x) (L_k^dag L_k)^T ) of single-qubit
    collapse operators is a constant 4x4 block on each (row qubit j, column qubit j) pair: the library's dense "pair terms".

DP5_ME's semantics — the continuous-time solution — are those of DP5_SE: H(t) is piecewise linear, so is M(t), and every
linear piece is advanced by commutator-free Magnus steps whose exponentials are product-form polynomials in M.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .observables import (DensityMatrixObservables, OccupationCorrelations, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap,
                          pack_overlaps)
from .shots import ShotRequest
from .simconfig import NoiseModel
from .solver import ProblemSpec, SolverType, evolve, split_dm_moments, split_observables, tolerance_from_options
from .utils import DiagonalObservable, real_diagonal

CD = torch.complex128
MAX_ME_QUBITS = 12  # 4^12 amplitudes = 256 MiB per density matrix
ME_DEFAULT_TOL = 1e-10

_Z = np.array([[1, 0], [0, -1]], dtype=complex)        # r = |0>, g = |1>; Z|r> = +|r> (utils.py ZMAT)
_X = np.array([[0, 1], [1, 0]], dtype=complex)
_Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
_SIGMA_GR = np.array([[0, 0], [1, 0]], dtype=complex)  # |g><r| (op_matrix["sigma_gr"], hamiltonian.py:108-115)


def local_collapse_operators(cfg: NoiseModel, basis_name: str = "ground-rydberg") -> list:
    """The single-qubit collapse operators of ``hamiltonian.py:98-143`` (each is applied to every qubit).  In the digital basis the
    dephasing rate is the hyperfine one (:106-111) and relaxation — built on sigma_gr — is refused (:113-120)."""
    ops = []
    if "dephasing" in cfg.noise_types:
        rate = cfg.hyperfine_dephasing_rate if basis_name == "digital" else cfg.dephasing_rate
        ops.append(np.sqrt(rate / 2) * _Z)
    if "relaxation" in cfg.noise_types:
        if basis_name != "ground-rydberg":
            raise ValueError("'relaxation' noise requires addressing of the 'ground-rydberg' basis.")
        ops.append(np.sqrt(cfg.relaxation_rate) * _SIGMA_GR)
    if "depolarizing" in cfg.noise_types:
        c = np.sqrt(cfg.depolarizing_rate / 4)
        ops += [c * _X, c * _Y, c * _Z]
    if "eff_noise" in cfg.noise_types:
        for rate, oper in zip(cfg.eff_noise_rates, cfg.eff_noise_opers):
            ops.append(np.sqrt(rate) * np.asarray(torch.as_tensor(oper).to(CD).numpy() if isinstance(oper, Tensor) else oper,
                                                  dtype=complex))
    return ops


def dissipator_block(local_ops: list) -> np.ndarray:
    """i * D restricted to one (row qubit, column qubit) pair: the 4x4 table of a pair term, index 2*bit_row + bit_col."""
    eye = np.eye(2, dtype=complex)
    d = np.zeros((4, 4), dtype=complex)
    for op in local_ops:
        m = op.conj().T @ op
        d += np.kron(op, op.conj()) - 0.5 * np.kron(m, eye) - 0.5 * np.kron(eye, m.T)
    return 1j * d


def _pair_index(n: int, i: int, j: int) -> int:
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def doubled_tables(amp: Tensor, det: Tensor, u_pairs: Tensor, amp_masks, det_masks, n: int):
    """Coefficient tables / masks / pair interactions of the commutator on the doubled register (differentiable)."""
    amp2 = torch.cat([amp, -amp.conj()], dim=1) if amp.shape[1] else amp
    det2 = torch.cat([det, -det], dim=1) if det.shape[1] else det
    am2 = tuple(amp_masks) + tuple(m << n for m in amp_masks)
    dm2 = tuple(det_masks) + tuple(m << n for m in det_masks)
    n2 = 2 * n
    rows, cols, sign = [], [], []
    for k, (i, j) in enumerate(itertools.combinations(range(n), 2)):
        rows += [_pair_index(n2, i, j), _pair_index(n2, n + i, n + j)]
        cols += [k, k]
        sign += [1.0, -1.0]
    u2 = torch.zeros(n2 * (n2 - 1) // 2, dtype=torch.float64, device=u_pairs.device)
    if rows:
        idx = torch.tensor(rows, device=u_pairs.device)
        u2 = u2.index_put((idx,), u_pairs[torch.tensor(cols, device=u_pairs.device)] *
                          torch.tensor(sign, dtype=torch.float64, device=u_pairs.device))
    return amp2, det2, u2, am2, dm2


MAX_PAIR_TERMS = 28  # RYDIFF_MAX_PAIR_TERMS (include/rydiff.h)


def doubled_pair_terms(pair_terms, n: int, dissipator: Optional[np.ndarray] = None) -> tuple:
    """Dense two-qubit terms of the generator on the doubled register: a Hamiltonian block B on qubits (a, b) — the XY exchange,
    ``hamiltonian.py:346-366`` — enters the commutator as B on the row qubits (a, b) and -B^T on the column qubits (n + a, n + b)
    ((1 (x) H^T) vec(rho) = vec(rho H)); the dissipator block sits on every (row qubit j, column qubit j) pair."""
    out = []
    if dissipator is not None and np.any(dissipator != 0):
        out += [(j, n + j, dissipator) for j in range(n)]
    for a, b, blk in pair_terms:
        blk = np.asarray(blk, dtype=complex).reshape(4, 4)
        out += [(a, b, blk), (n + a, n + b, -blk.T)]
    if len(out) > MAX_PAIR_TERMS:
        raise NotImplementedError(f"The master equation with pair interactions needs {len(out)} dense two-qubit terms; the library "
                                  f"takes {MAX_PAIR_TERMS} (XY mode: up to 5 atoms with collapse operators).")
    return tuple(out)


@dataclass
class MasterEquationResult:
    """What ``mesolve`` returns.  Unpacks like the pair it used to return: ``rho, stats = mesolve(...)``."""

    states: Tensor  # (n_t, dim, dim, B); empty (0, dim, dim, B) with store_states=False
    stats: dict
    expect: list = field(default_factory=list)  # one real (n_t, B) tensor per non-RDM entry of `observables`, evaluated natively (differentiable)
    shots: Optional[ShotRequest] = None  # the request, holding the native shots (.indices: basis-state indices of the ATOMS)
    rdms: list = field(default_factory=list)  # one complex (n_t, B, 2^m, 2^m) per ReducedDensityMatrix of `observables`, in order (native, differentiable)
    moments: Optional[Tensor] = None  # (1 + n + n(n-1)/2, n_t, B) with OccupationCorrelations in `observables`: S, B_q, B_qr of diag rho (native, differentiable)

    def __iter__(self):
        return iter((self.states, self.stats))


def pack_dm_observables(observables: Sequence, n: int, batch: int, device, shots: bool = False):
    """``observables`` of a master-equation run -> (``DensityMatrixObservables`` or None, the row of every observable).  Takes
    ``DiagonalObservable`` / diagonal ``(dim, dim)`` tensors / ``(dim,)`` diagonals, ``PauliObservable``, ``StateOverlap`` (the
    fidelity ``<phi|rho|phi>``), ``Purity`` and ``ReducedDensityMatrix`` (``Tr_E rho``: its ``2 * 4^m`` rows sit behind all the real
    rows; the row listed for it is the first of them, and ``DensityMatrixObservables.rdms`` keeps the objects in order) and
    ``OccupationCorrelations`` (the moments of the diagonal of rho: ``DensityMatrixObservables.moments``, the last block of all; the
    row listed for it is -1: it takes no slot of the real rows).  Strings go
    to the library as they are: the master equation runs in no rotating frame (``mesolve`` hands ``ham.amp_tables`` over, never
    ``amp_tables_frame``)."""
    dim = 2 ** n
    diags, paulis, overlaps, purity, kinds, rdms, moments = [], [], [], False, [], [], False
    for obs in observables:
        if isinstance(obs, OccupationCorrelations):
            moments = True
            kinds.append(("moments", 0))
        elif isinstance(obs, ReducedDensityMatrix):
            obs.check(n)
            kinds.append(("rdm", sum(2 * 4 ** o.n_sub for o in rdms)))
            rdms.append(obs)
        elif isinstance(obs, Purity):
            purity = True
            kinds.append(("purity", 0))
        elif isinstance(obs, StateOverlap):
            kinds.append(("fid", len(overlaps)))
            overlaps.append(obs)
        elif isinstance(obs, PauliObservable):
            if obs.n_qubits != n:
                raise ValueError(f"PauliObservable on {obs.n_qubits} qubits handed to a register of {n}")
            kinds.append(("pauli", len(paulis)))
            paulis.append(obs)
        else:
            if isinstance(obs, DiagonalObservable) or (isinstance(obs, Tensor) and obs.ndim == 2):
                d = real_diagonal(obs, "Only diagonal tensors can be evaluated natively; hand off-diagonal ones over as PauliObservable.")
            elif isinstance(obs, Tensor) and obs.ndim == 1:
                d = obs.real if obs.is_complex() else obs
            else:
                raise TypeError("observables of a master-equation run must be DiagonalObservable / PauliObservable / StateOverlap / "
                                f"Purity / ReducedDensityMatrix / OccupationCorrelations objects or diagonal tensors, got {type(obs)}")
            if d.shape[0] != dim:
                raise ValueError(f"diagonal observable of dimension {d.shape[0]} handed to a register of dimension {dim}")
            kinds.append(("diag", len(diags)))
            diags.append(d.to(device, torch.float64))
    if not kinds and not shots:
        return None, []
    dm = DensityMatrixObservables(n, diag=torch.stack(diags) if diags else None, pauli=paulis or None,
                                  targets=pack_overlaps(overlaps, dim, batch, device) if overlaps else None, purity=purity, shots=shots,
                                  rdms=rdms or None, moments=moments)
    n_real = len(diags) + len(paulis) + len(overlaps) + int(purity)
    first = {"diag": 0, "pauli": len(diags), "fid": len(diags) + len(paulis), "purity": n_real - 1, "rdm": n_real, "moments": -1}
    return dm, [first[kind] + i for kind, i in kinds]


def mesolve(ham, psi0: Tensor, tsave: Tensor, noise: NoiseModel, options: Optional[dict] = None,
            observables: Optional[Sequence] = None, shots: Union[None, int, ShotRequest] = None,
            store_states: bool = True) -> MasterEquationResult:
    """Density matrices rho(t_k) of shape (n_t, dim, dim, B) for the structured Hamiltonian ``ham`` and the collapse
    operators of ``noise``; psi0: (dim, B) kets (rho0 = |psi0><psi0|, ``backend.py:503``).

    ``observables`` (see ``pack_dm_observables``) are evaluated natively at every evaluation time while rho is on the device
    (``MasterEquationResult.expect``, differentiable); ``shots``: an int (that many at the final time) or a ``ShotRequest``, drawn
    natively from the diagonal of rho; ``ReducedDensityMatrix`` entries come back in ``MasterEquationResult.rdms`` (complex
    ``(n_t, B, 2^m, 2^m)``, in the order of their ``qubits``) and take no slot of ``expect``; ``OccupationCorrelations()`` comes back as
    ``MasterEquationResult.moments`` (``(1 + n + n(n-1)/2, n_t, B)``: ``S, B_q, B_qr`` of the diagonal of rho, differentiable) and takes
    no slot of ``expect`` either; ``store_states=False`` keeps the ``(n_t, 4^n)`` trajectory out of the result (``states``
    is then empty) — gradients of the native values need no stored state."""
    n = ham._size
    if n > MAX_ME_QUBITS:
        raise ValueError(f"The master-equation solver keeps 4^N amplitudes; limited to {MAX_ME_QUBITS} qubits.")
    options = dict(options or {})
    dev = ham.amp_tables.device
    amp2, det2, u2, am2, dm2 = doubled_tables(ham.amp_tables, ham.det_tables, ham.u_pairs, ham.amp_masks, ham.det_masks, n)
    block = dissipator_block(local_collapse_operators(noise, getattr(ham, "basis_name", "ground-rydberg")))
    pair_terms = doubled_pair_terms(getattr(ham, "pair_terms", ()), n, block)  # dissipators + the XY exchange (if any)
    # default accuracy target one decade below the ket solver's: the calibration of the Magnus step is a little optimistic
    # for non-normal (dissipative) generators
    psi = psi0.to(dev, CD)
    if psi.ndim == 1:
        psi = psi.unsqueeze(1)
    dim = psi.shape[0]
    if shots is not None and not isinstance(shots, ShotRequest):
        shots = ShotRequest(int(shots))
    dm, rows = pack_dm_observables(list(observables or []), n, psi.shape[1], dev, shots=shots is not None)
    spec = ProblemSpec(2 * n, ham.dt, ham.n_samples, am2, dm2, solver=SolverType.DP5_SE,
                       tol=tolerance_from_options(options) or ME_DEFAULT_TOL, store_states=bool(store_states), pair_terms=pair_terms,
                       piece_refine=getattr(ham, "piece_refine", None),  # same time structure on the doubled register
                       dm=dm, shots=shots)
    rho0 = torch.einsum("xb,yb->bxy", psi, psi.conj()).reshape(psi.shape[1], dim * dim).contiguous()
    states, expect = evolve(amp2, det2, u2, tsave, rho0, spec, None)  # (n_t, B, dim^2), (rows, n_t, B)
    rho = states.reshape(states.shape[0], states.shape[1], dim, dim).permute(0, 2, 3, 1)
    obs_list = list(observables or [])
    moments = None
    if dm is not None and dm.moments:
        expect, moments = split_dm_moments(expect, n)
    expect, _, rdms = split_observables(expect, 0, dm.rdms if dm is not None else None)
    real_rows = [r for r, o in zip(rows, obs_list) if not isinstance(o, (ReducedDensityMatrix, OccupationCorrelations))]
    return MasterEquationResult(rho, dict(spec.options.get("_last_stats", {})), [expect[r] for r in real_rows], shots, rdms or [], moments)


def doubled_table_tangents(d_amp: Optional[Tensor], d_det: Optional[Tensor], d_u: Optional[Tensor], n: int) -> tuple:
    """Tangents of ``doubled_tables`` in the directions ``d_amp`` / ``d_det`` / ``d_u`` (direction-major: one more leading axis than the
    tables; None stays None).  The map is REAL-linear (the column half conjugates the drive coefficient), so its directional
    derivative is the map itself applied per direction: ``cat[d_amp, -conj(d_amp)]``, ``cat[d_det, -d_det]``, and ``d_u`` through
    the same index map (+ among row qubits, - among column qubits)."""
    d_amp2 = None if d_amp is None else (torch.cat([d_amp, -d_amp.conj()], dim=2) if d_amp.shape[2] else d_amp)
    d_det2 = None if d_det is None else (torch.cat([d_det, -d_det], dim=2) if d_det.shape[2] else d_det)
    d_u2 = None
    if d_u is not None:
        n2 = 2 * n
        d_u2 = torch.zeros((d_u.shape[0], n2 * (n2 - 1) // 2), dtype=torch.float64, device=d_u.device)
        for k, (i, j) in enumerate(itertools.combinations(range(n), 2)):
            d_u2[:, _pair_index(n2, i, j)] = d_u[:, k]
            d_u2[:, _pair_index(n2, n + i, n + j)] = -d_u[:, k]
    return d_amp2, d_det2, d_u2


def mesolve_tangent(ham, psi0: Tensor, tsave: Tensor, noise: NoiseModel, options: Optional[dict] = None,
                    observables: Optional[Sequence] = None, d_amp: Optional[Tensor] = None, d_det: Optional[Tensor] = None,
                    d_u: Optional[Tensor] = None, d_psi0: Optional[Tensor] = None, moments: bool = False) -> tuple:
    """Forward-mode twin of ``mesolve(..., store_states=False)``: ONE tangent sweep (``solver.evolve_tangent``) on the doubled
    register carries vec(rho) and its tangents in up to 8 directions (more: chunks of 8) and returns ``(expect, dexpect)`` — the
    values (n_obs, n_t, B) of ``observables`` and their directional derivatives (n_dir, n_obs, n_t, B) at EVERY evaluation time,
    in the order of ``observables`` (diagonal / ``PauliObservable`` / ``StateOverlap`` = the fidelity ``<phi|rho|phi>`` /
    ``Purity``; a ``ReducedDensityMatrix`` raises ``NotImplementedError``).  ``moments=True``: the occupation correlations of the
    diagonal of rho join — the return is ``(expect, dexpect, moments, dmoments)`` with ``moments`` (1 + n + n(n-1)/2, n_t, B) and
    ``dmoments`` (n_dir, 1 + n + n(n-1)/2, n_t, B), the same rows of ``d rho_d`` (they are linear in rho); an
    ``OccupationCorrelations`` in ``observables`` is a ``TypeError`` here (ask with the keyword).

    A direction d is a tangent of the UNDOUBLED inputs: ``d_amp[d]`` shaped like ``ham.amp_tables``, ``d_det[d]`` like
    ``ham.det_tables``, ``d_u[d]`` like ``ham.u_pairs``, ``d_psi0[d]`` like ``psi0`` (dim, B) — the tangent of rho0 is then
    ``|dpsi><psi| + |psi><dpsi|``.  The collapse rates of ``noise`` and the XY blocks of ``ham`` are constants in every direction.
    Same tolerance default, time structure and pair terms as ``mesolve``."""
    from . import _native
    from .solver import evolve_tangent

    n = ham._size
    if n > MAX_ME_QUBITS:
        raise ValueError(f"The master-equation solver keeps 4^N amplitudes; limited to {MAX_ME_QUBITS} qubits.")
    obs_list = list(observables or [])
    if any(isinstance(o, ReducedDensityMatrix) for o in obs_list):
        raise NotImplementedError("mesolve_tangent evaluates no reduced density matrices (the tangent sweep has no tangents of them); "
                                  "differentiate mesolve(..., store_states=False).rdms instead")
    if any(isinstance(o, OccupationCorrelations) for o in obs_list):
        raise TypeError("mesolve_tangent takes the occupation correlations through moments=True, not as an entry of observables")
    options = dict(options or {})
    dev = ham.amp_tables.device
    amp2, det2, u2, am2, dm2 = doubled_tables(ham.amp_tables.detach(), ham.det_tables.detach(), ham.u_pairs.detach(), ham.amp_masks,
                                              ham.det_masks, n)
    block = dissipator_block(local_collapse_operators(noise, getattr(ham, "basis_name", "ground-rydberg")))
    pair_terms = doubled_pair_terms(getattr(ham, "pair_terms", ()), n, block)
    psi = psi0.detach().to(dev, CD)
    if psi.ndim == 1:
        psi = psi.unsqueeze(1)
    dim, batch = psi.shape
    dm, rows = pack_dm_observables(obs_list + ([OccupationCorrelations()] if moments else []), n, batch, dev)
    rows = rows[:len(obs_list)]
    spec = ProblemSpec(2 * n, ham.dt, ham.n_samples, am2, dm2, solver=SolverType.DP5_SE,
                       tol=tolerance_from_options(options) or ME_DEFAULT_TOL, store_states=False, pair_terms=pair_terms,
                       piece_refine=getattr(ham, "piece_refine", None), dm=dm)
    rho0 = torch.einsum("xb,yb->bxy", psi, psi.conj()).reshape(batch, dim * dim).contiguous()
    to_dev = lambda t, dt: None if t is None else t.detach().to(dev, dt)
    d_amp2, d_det2, d_u2 = doubled_table_tangents(to_dev(d_amp, CD), to_dev(d_det, torch.float64), to_dev(d_u, torch.float64), n)
    d_rho0 = None
    if d_psi0 is not None:
        dpsi = d_psi0.detach().to(dev, CD)
        if dpsi.ndim == 2:
            dpsi = dpsi.unsqueeze(2)
        d_rho0 = (torch.einsum("dxb,yb->dbxy", dpsi, psi.conj()) + torch.einsum("xb,dyb->dbxy", psi, dpsi.conj()))
        d_rho0 = d_rho0.reshape(dpsi.shape[0], batch, dim * dim).contiguous()
    expect, dexpect = evolve_tangent(amp2, det2, u2, tsave, rho0, spec, None, d_amp=d_amp2, d_det=d_det2, d_u=d_u2, d_psi0=d_rho0,
                                     flags=_native.TANGENT_PAIR_TERMS | _native.TANGENT_DENSITY_MATRIX)
    if not moments:
        return expect[rows], dexpect[:, rows]
    first = expect.shape[0] - dm.moment_rows()
    return expect[rows], dexpect[:, rows], expect[first:], dexpect[:, first:]
