"""Solver seam: the MI355X-native replacement of ``pyqtorch.sesolve`` as called at
``pulser_diff/backend.py:488-494``.

The reference passes an opaque callable ``H_t`` (``pulser_diff/hamiltonian.py:526-546``) that the third-party
solver evaluates on every sub-step, and lets torch autograd tape every one of those sub-steps.  Here the seam
takes the STRUCTURED problem (the coefficient arrays ``build_ham_tensor`` captures, the qubits they act on, the
pair interactions) and a ``torch.autograd.Function`` whose backward is the native adjoint sweep
(``rydiff_backward``), so ``torch.autograd.grad(f, x, v, retain_graph=True)`` (``pulser_diff/derivative.py:40,76``)
works unchanged on its outputs, any number of times.
"""
from __future__ import annotations

import ctypes
import enum
from dataclasses import dataclass, field, replace
from typing import Any, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _native
from .observables import (DensityMatrixObservables, PauliObservable, ReducedDensityMatrix, StateOverlap, check_pauli, moment_rows,
                          pack_overlaps, pack_pauli, pack_rdms)
from .shots import ShotRequest


class SolverType(enum.Enum):
    """Member names of ``pyqtorch.utils.SolverType`` used by the reference (``backend.py:434,483,487``)."""

    DP5_SE = "dp5_se"
    KRYLOV_SE = "krylov_se"
    DP5_ME = "dp5_me"


_SOLVER_CODE = {SolverType.KRYLOV_SE: _native.SOLVER_KRYLOV_SE, SolverType.DP5_SE: _native.SOLVER_DP5_SE}

# options the reference forwards verbatim to pyqtorch (backend.py:435,493); the ones that steer accuracy map
# onto the per-exponential truncation target, the others are accepted and ignored.
_KNOWN_OPTIONS = {"atol", "rtol", "max_krylov", "exp_tolerance", "norm_tolerance", "max_steps", "tol", "use_sparse"}


@dataclass
class ProblemSpec:
    """Static (non-tensor) description of one evolution problem."""

    n_qubits: int
    dt: float
    n_samples: int
    amp_masks: tuple[int, ...]  # bit j = term acts on qubit j
    det_masks: tuple[int, ...]
    solver: SolverType = SolverType.KRYLOV_SE
    tol: float = 0.0
    store_states: bool = True
    # gradients: "steps" (one state per save point + recompute) | "full" (every factor output kept) | "partial" (one state per save
    # point + every factor output of the trailing `tape_steps` intervals) | "auto" (full when it fits in HBM, else as much of the
    # run as fits, from 13 qubits on)
    tape: str = "auto"
    tape_steps: Optional[int] = None  # tape="partial": trailing save intervals kept on the tape (None: as many as fit)
    options: dict = field(default_factory=dict)
    # dense two-qubit terms of the generator (include/rydiff.h): ((qubit_a, qubit_b, 4x4 complex table), ...); constants
    pair_terms: tuple = ()
    # kernel family (RydProblem.kernel_variant): None = this thread's default (_native.set_kernel_variant, normally 0 = automatic)
    kernel_variant: Optional[int] = None
    # three-level registers as two qubits per atom (include/rydiff.h, amp_conditioned_terms / det_ones_terms): per-term flags
    amp_conditioned: tuple = ()   # () or one bool per amplitude term: the flip acts only where the sibling qubit (j ^ 1) is 1
    det_ones: tuple = ()          # () or one bool per detuning term: the term counts the ones of its mask with minus its coefficient
    # DP5_SE: optional uint8 array [n_samples - 1], multiplier of the Magnus sub-steps per sample interval (RydProblem.dp5_piece_refine)
    piece_refine: Optional[Any] = None
    # Pauli-string observables evaluated (and differentiated) natively next to obs_diag: a list of PauliObservable, or the packed
    # host arrays (pauli_first, pauli_x, pauli_z, pauli_w) of RydProblem; their values follow the diagonal ones in `expect`
    pauli: Optional[Any] = None
    # state-overlap observables (RydProblem.overlap_*): the packed targets, a complex128 DEVICE tensor (n_ov, 1 | B, 2^N)
    # (observables.pack_overlaps); Re / Im of every overlap follow the Pauli rows in `expect`.  Constants: no gradient.
    overlaps: Optional[Tensor] = None
    # reduced density matrices (RydProblem.n_rdms / rdm_masks): a list of ReducedDensityMatrix, or the packed uint32 qubit masks
    # (observables.pack_rdms); Re / Im of every entry follow the overlap rows in `expect` (split_observables takes them out)
    rdms: Optional[Any] = None
    # measurement shots drawn natively at chosen save points (RydProblem.n_shots / shot_*): the request object receives the amplitude
    # indices (shots.ShotRequest.indices); a non-differentiable by-product, allowed next to a gradient
    shots: Optional[ShotRequest] = None
    # density-matrix observables (RydProblem.dm_*): the register is the doubled register of a density matrix and these functionals of
    # rho — diagonal tables, Pauli strings over the atoms, fidelities with target states, the purity, reduced density matrices — are evaluated and differentiated
    # natively; their rows follow every other row of `expect` (observables.DensityMatrixObservables).  `dm.shots`: the shots of
    # `shots` are drawn from the diagonal of rho
    dm: Optional[DensityMatrixObservables] = None
    # occupation correlations (RydProblem.bit_moments): the moments S, B_q, B_qr of |psi|^2 over the index bits, 1 + N + N(N-1)/2 rows
    # behind the reduced-density-matrix rows of `expect` (split_moments takes them off the end); kets only
    moments: bool = False
    # XY exchange as a term of its own (RydProblem.xy_mode): 0 none | 1 Hermitian | 2 one-directional, as the reference writes it; the
    # couplings J_ij are the `xy_pairs` input of ``evolve`` (N(N-1)/2 values in the order of u_pairs; they take part in autograd)
    xy_mode: int = 0
    # energy observables (RydProblem.energy_rows): 0 off | 1 the row E(t_k) = <psi_k|H(t_k)|psi_k> | 2 E then M2 = |H(t_k) psi_k|^2, the last
    # rows of a ket's `expect` (split_energy takes them off the end); H(t_k) is built from the `energy_amp` / `energy_det` inputs of
    # ``evolve``: the coefficient tables AT the save points (Hamiltonian.energy_tables), which take part in autograd
    energy: int = 0
    energy_kernel: int = 0  # RydProblem.energy_kernel: 0 automatic | 1 the direct version | 2 the LDS-tile version (13 .. 24 qubits, no exchange)

    def moment_rows(self) -> int:
        """Rows of `expect` the occupation correlations take: 1 + N + N(N-1)/2, or 0."""
        return moment_rows(self.n_qubits) if self.moments else 0

    @property
    def n_overlaps(self) -> int:
        return 0 if self.overlaps is None else int(self.overlaps.shape[0])

    def packed_rdms(self) -> Optional[np.ndarray]:
        """The host array of RydProblem.rdm_masks (None: no reduced density matrices); validated like the library does."""
        if self.rdms is None:
            return None
        rdms = list(self.rdms)
        if rdms and all(isinstance(o, ReducedDensityMatrix) for o in rdms):
            return pack_rdms(rdms, self.n_qubits)
        masks = [int(v) for v in rdms]
        if not 1 <= len(masks) <= _native.MAX_RDMS:
            raise ValueError(f"ProblemSpec.rdms: 1 to {_native.MAX_RDMS} reduced density matrices per call, got {len(masks)}")
        for v in masks:
            if v <= 0 or v >> self.n_qubits or bin(v).count("1") > _native.MAX_RDM_QUBITS:
                raise ValueError(f"ProblemSpec.rdms: mask {v:#x} must name 1 to {_native.MAX_RDM_QUBITS} qubits below {self.n_qubits}")
        return np.asarray(masks, dtype=np.uint32)

    def rdm_rows(self) -> int:
        """Rows of `expect` the reduced density matrices take: 2 * sum_o 4^{m_o}."""
        masks = self.packed_rdms()
        return 0 if masks is None else sum(2 * 4 ** bin(int(v)).count("1") for v in masks)

    def packed_pauli(self):
        """The four host arrays of RydProblem.pauli_* (None: no Pauli observables)."""
        if self.pauli is None:
            return None
        pauli = self.pauli
        if len(pauli) and all(isinstance(o, PauliObservable) for o in pauli):
            return pack_pauli(list(pauli), self.n_qubits)
        if len(pauli) != 4:
            raise ValueError("ProblemSpec.pauli: a list of PauliObservable or (pauli_first, pauli_x, pauli_z, pauli_w)")
        packed = (np.ascontiguousarray(pauli[0], dtype=np.int32), np.ascontiguousarray(pauli[1], dtype=np.uint32),
                  np.ascontiguousarray(pauli[2], dtype=np.uint32), np.ascontiguousarray(pauli[3], dtype=np.float64))
        check_pauli(packed, self.n_qubits)
        return packed

    def solver_code(self) -> int:
        if self.solver not in _SOLVER_CODE:
            raise ValueError(f"Solver {self.solver} not available.")  # backend.py:511
        return _SOLVER_CODE[self.solver]


_SMALL_TAPE_BYTES = 64 << 20  # a full tape below this size is taken without consulting the allocator


def tolerance_from_options(options: dict[str, Any]) -> float:
    unknown = set(options) - _KNOWN_OPTIONS
    if unknown:
        raise TypeError(f"Unknown solver option(s): {sorted(unknown)}")
    for key in ("tol", "exp_tolerance"):
        if key in options:
            return float(options[key])
    if "atol" in options or "rtol" in options:
        # DP5-style local tolerances: aim two orders below the requested accuracy
        return max(min(float(options.get("atol", 1e-8)), float(options.get("rtol", 1e-6))) * 1e-2, 1e-14)
    return 0.0


def _require_cuda(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} must live on the GPU (got device {t.device}); the MI355X backend has no CPU path. "
            "Move the inputs with .to('cuda')."
        )


class _Call:
    """Keeps the ctypes structures and every buffer they point to alive for the duration of a native call."""

    def __init__(self, spec: ProblemSpec, amp: Tensor, det: Tensor, u_pairs: Tensor, tsave_host: np.ndarray,
                 batch: int, obs: Optional[Tensor], real_amp_grad: bool = False, xy_pairs: Optional[Tensor] = None,
                 energy_amp: Optional[Tensor] = None, energy_det: Optional[Tensor] = None):
        self.spec = spec
        self.amp_masks = np.asarray(spec.amp_masks, dtype=np.uint32)
        self.det_masks = np.asarray(spec.det_masks, dtype=np.uint32)
        self.tsave = np.ascontiguousarray(tsave_host, dtype=np.float64)
        self.tensors = (amp, det, u_pairs, obs, xy_pairs, energy_amp, energy_det)
        p = _native.RydProblem()
        p.n_qubits = spec.n_qubits
        p.batch = batch
        ka, kd = len(spec.amp_masks), len(spec.det_masks)
        cb = 1
        if ka:
            cb = amp.shape[0]
        elif kd:
            cb = det.shape[0]
        p.coeff_batch = cb
        p.n_samples = spec.n_samples
        p.dt = spec.dt
        p.n_amp_terms = ka
        p.n_det_terms = kd
        p.amp_masks = self.amp_masks.ctypes.data if ka else None
        p.det_masks = self.det_masks.ctypes.data if kd else None
        p.amp_tables = amp.data_ptr() if ka else None
        p.det_tables = det.data_ptr() if kd else None
        p.u_pairs = u_pairs.data_ptr() if u_pairs.numel() else None
        p.n_tsave = len(self.tsave)
        p.tsave = self.tsave.ctypes.data
        p.solver = spec.solver_code()
        p.tol = spec.tol
        p.n_obs = 0 if obs is None else obs.shape[0]
        p.obs_diag = None if obs is None or obs.shape[0] == 0 else obs.data_ptr()
        self.pair_qubits = np.ascontiguousarray([[a, b] for a, b, _ in spec.pair_terms], dtype=np.uint32).reshape(-1, 2)
        self.pair_tables = np.ascontiguousarray([np.asarray(t, dtype=np.complex128).reshape(16) for _, _, t in spec.pair_terms],
                                                dtype=np.complex128).reshape(-1, 16)
        p.n_pair_terms = len(spec.pair_terms)
        p.pair_qubits = self.pair_qubits.ctypes.data if spec.pair_terms else None
        p.pair_tables = self.pair_tables.ctypes.data if spec.pair_terms else None
        p.real_amp_grad = int(real_amp_grad)  # the caller's amplitude tables are a REAL tensor: only Re(g_amp) is used
        p.kernel_variant = _native.default_kernel_variant() if spec.kernel_variant is None else int(spec.kernel_variant)
        p.amp_conditioned_terms = sum(1 << k for k, f in enumerate(spec.amp_conditioned) if f)
        p.det_ones_terms = sum(1 << k for k, f in enumerate(spec.det_ones) if f)
        self.piece_refine = None
        if spec.piece_refine is not None and spec.n_samples >= 2:
            self.piece_refine = np.ascontiguousarray(np.clip(np.asarray(spec.piece_refine), 0, 255), dtype=np.uint8)
            if self.piece_refine.shape != (spec.n_samples - 1,):
                raise ValueError(f"piece_refine must have n_samples - 1 = {spec.n_samples - 1} entries, got {self.piece_refine.shape}")
            p.dp5_piece_refine = self.piece_refine.ctypes.data
        self.pauli = spec.packed_pauli()  # (validated: counts, mask bits, the string cap)
        if self.pauli is not None and len(self.pauli[0]) > 1:
            first, px, pz, pw = self.pauli
            p.n_pauli_obs = len(first) - 1
            p.n_pauli_strings = len(px)
            p.pauli_first = first.ctypes.data
            p.pauli_x = px.ctypes.data if len(px) else None
            p.pauli_z = pz.ctypes.data if len(px) else None
            p.pauli_w = pw.ctypes.data if len(px) else None
        self.overlaps = None
        if spec.overlaps is not None:
            _check_overlaps(spec, batch)
            self.overlaps = spec.overlaps.contiguous()
            p.n_overlaps = self.overlaps.shape[0]
            p.overlap_batch = self.overlaps.shape[1]
            p.overlap_targets = self.overlaps.data_ptr()
        self.rdm_masks = spec.packed_rdms()
        if self.rdm_masks is not None:
            p.n_rdms = len(self.rdm_masks)
            p.rdm_masks = self.rdm_masks.ctypes.data
        p.bit_moments = int(spec.moments)
        p.xy_mode = int(spec.xy_mode)
        p.xy_pairs = xy_pairs.data_ptr() if (spec.xy_mode and xy_pairs is not None and xy_pairs.numel()) else None
        p.energy_rows = int(spec.energy)
        p.energy_kernel = int(spec.energy_kernel) if spec.energy else 0
        if spec.energy:
            p.energy_amp = energy_amp.data_ptr() if (ka and energy_amp is not None) else None
            p.energy_det = energy_det.data_ptr() if (kd and energy_det is not None) else None
        self.dm_buffers = None
        if spec.dm is not None:
            dm = spec.dm
            dm.check(spec.n_qubits, batch)
            diag = None if dm.diag is None else dm.diag.contiguous()
            targets = None if dm.targets is None else dm.targets.contiguous()
            packed = dm.packed_pauli()
            rdm_masks = dm.packed_rdms()
            self.dm_buffers = (diag, targets, packed, rdm_masks)
            p.dm_atoms = dm.n_atoms
            if rdm_masks is not None:
                p.n_dm_rdms = len(rdm_masks)
                p.dm_rdm_masks = rdm_masks.ctypes.data
            if diag is not None:
                p.n_dm_diag = diag.shape[0]
                p.dm_diag = diag.data_ptr()
            if packed is not None:
                first, px, pz, pw = packed
                p.n_dm_pauli_obs = len(first) - 1
                p.n_dm_pauli_strings = len(px)
                p.dm_pauli_first = first.ctypes.data
                p.dm_pauli_x = px.ctypes.data if len(px) else None
                p.dm_pauli_z = pz.ctypes.data if len(px) else None
                p.dm_pauli_w = pw.ctypes.data if len(px) else None
            if targets is not None:
                p.n_dm_fid = targets.shape[0]
                p.dm_fid_batch = targets.shape[1]
                p.dm_fid_targets = targets.data_ptr()
            p.dm_purity = int(dm.purity)
            p.dm_shots = int(dm.shots)
            p.dm_moments = int(dm.moments)
        self.problem = p
        self.shot_buffers = None

    def expect_rows(self) -> int:
        """Rows of `expect` / `dexpect[d]`, in the order the library writes them (ExpectRows, csrc/plan.hpp): diagonal observables,
        then the Pauli ones, then Re / Im of every overlap, then Re / Im of every RDM entry, then the moments S, B_q, B_qr of the occupation correlations, then the energy rows E (and M2), then the density-matrix rows."""
        p = self.problem
        dm_rows = self.spec.dm.rows() if self.spec.dm is not None else 0
        return p.n_obs + p.n_pauli_obs + 2 * p.n_overlaps + self.spec.rdm_rows() + self.spec.moment_rows() + int(self.spec.energy) + dm_rows

    def set_shots(self, times: np.ndarray, uniforms: Tensor, out: Tensor) -> None:
        """RydProblem.n_shots / shot_*: sampled save points (host int32), uniforms (device float64) and the output (device, 32-bit),
        both (n_shot_times, batch, n_shots).  rydiff_backward is handed the same fields: the counts size the workspace."""
        self.shot_buffers = (np.ascontiguousarray(times, dtype=np.int32), uniforms, out)
        p = self.problem
        p.n_shots = uniforms.shape[2]
        p.n_shot_times = len(self.shot_buffers[0])
        p.shot_times = self.shot_buffers[0].ctypes.data
        p.shot_uniforms = uniforms.data_ptr()
        p.shots_out = out.data_ptr()


def _check_overlaps(spec: ProblemSpec, batch: int, device: Optional[torch.device] = None) -> None:
    """ProblemSpec.overlaps against the spec: shape (n_ov, 1 | batch, 2^N), complex128, count within the cap, on `device`."""
    ov = spec.overlaps
    if ov is None:
        return
    dim = 2 ** spec.n_qubits
    if not isinstance(ov, Tensor) or ov.dtype != torch.complex128:
        raise ValueError(f"overlaps must be a complex128 tensor, got {getattr(ov, 'dtype', type(ov))}")
    if ov.ndim != 3 or ov.shape[2] != dim or ov.shape[0] < 1:
        raise ValueError(f"overlaps must have shape (n_overlaps, 1 or batch, {dim}), got {tuple(ov.shape)}")
    if ov.shape[0] > _native.MAX_OVERLAPS:
        raise ValueError(f"too many overlap observables: {ov.shape[0]} (at most {_native.MAX_OVERLAPS} per call)")
    if ov.shape[1] not in (1, batch):
        raise ValueError(f"overlaps: the target batch must be 1 or the batch size {batch}, got {ov.shape[1]}")
    if device is not None and ov.device != torch.device(device):
        raise ValueError(f"overlaps must live on the device of the states ({device}), got {ov.device}")


def _check_shapes(spec: ProblemSpec, amp: Tensor, det: Tensor, u_pairs: Tensor, obs: Optional[Tensor], batch: int,
                  device: Optional[torch.device] = None, xy_pairs: Optional[Tensor] = None, energy_amp: Optional[Tensor] = None,
                  energy_det: Optional[Tensor] = None, n_t: int = 0) -> None:
    """The C ABI sees raw pointers only: every buffer is checked against the spec here, so that a mismatch is a ValueError and
    never an out-of-bounds device read."""
    ka, kd, n, nq = len(spec.amp_masks), len(spec.det_masks), spec.n_samples, spec.n_qubits
    if len(spec.amp_conditioned) not in (0, ka) or len(spec.det_ones) not in (0, kd):
        raise ValueError("amp_conditioned / det_ones: one flag per amplitude / detuning term (or empty)")
    cb = None
    for name, t, k in (("amp_tables", amp, ka), ("det_tables", det, kd)):
        if k == 0:
            continue
        if t.ndim != 3 or t.shape[1] != k or t.shape[2] != n:
            raise ValueError(f"{name} must have shape (coeff_batch, {k}, {n}), got {tuple(t.shape)}")
        if t.shape[0] not in (1, batch):
            raise ValueError(f"{name}: coeff_batch must be 1 or the batch size {batch}, got {t.shape[0]}")
        if cb is not None and t.shape[0] != cb:
            raise ValueError(f"amp_tables and det_tables disagree on coeff_batch ({cb} vs {t.shape[0]})")
        cb = t.shape[0]
    n_pairs = nq * (nq - 1) // 2
    if u_pairs.numel() != n_pairs:
        raise ValueError(f"u_pairs must hold N(N-1)/2 = {n_pairs} values, got {u_pairs.numel()}")
    if spec.xy_mode not in (0, 1, 2):
        raise ValueError(f"ProblemSpec.xy_mode must be 0 (none), 1 (Hermitian exchange) or 2 (one-directional), got {spec.xy_mode}")
    if spec.xy_mode and xy_pairs is None:
        raise ValueError("ProblemSpec.xy_mode is set: evolve needs the couplings xy_pairs")
    if not spec.xy_mode and xy_pairs is not None:
        raise ValueError("xy_pairs given without ProblemSpec.xy_mode")
    if xy_pairs is not None and xy_pairs.numel() != n_pairs:
        raise ValueError(f"xy_pairs must hold N(N-1)/2 = {n_pairs} values, got {xy_pairs.numel()}")
    if xy_pairs is not None and device is not None and xy_pairs.device != torch.device(device):
        raise ValueError(f"xy_pairs must live on the device of the states ({device}), got {xy_pairs.device}")
    if spec.energy not in (0, 1, 2):
        raise ValueError(f"ProblemSpec.energy must be 0 (off), 1 (E) or 2 (E and its second moment), got {spec.energy}")
    if not spec.energy and (energy_amp is not None or energy_det is not None):
        raise ValueError("energy_amp / energy_det given without ProblemSpec.energy")
    if spec.energy:
        for name, t, k in (("energy_amp", energy_amp, ka), ("energy_det", energy_det, kd)):
            if k == 0:
                continue
            if t is None:
                raise ValueError(f"ProblemSpec.energy is set: evolve needs {name}, the coefficients at the evaluation times "
                                 "(Hamiltonian.energy_tables)")
            if t.ndim != 3 or t.shape[1] != k or t.shape[2] != n_t or t.shape[0] != cb:
                raise ValueError(f"{name} must have shape ({cb}, {k}, {n_t}) = (coeff_batch, terms, evaluation times), got {tuple(t.shape)}")
            if device is not None and t.device != torch.device(device):
                raise ValueError(f"{name} must live on the device of the states ({device}), got {t.device}")
    if obs is not None and obs.numel() and (obs.ndim != 2 or obs.shape[1] != 2 ** nq):
        raise ValueError(f"obs_diag must have shape (n_obs, {2 ** nq}), got {tuple(obs.shape)}")
    spec.packed_pauli()  # raises ValueError on a mask bit at or above N, inconsistent counts, too many strings
    _check_overlaps(spec, batch, device)
    spec.packed_rdms()  # raises ValueError on an empty mask, too many qubits, a bit at or above N, too many matrices
    if spec.dm is not None:
        spec.dm.check(nq, batch, device)
        if spec.dm.shots and spec.shots is None:
            raise ValueError("DensityMatrixObservables.shots needs a ShotRequest in ProblemSpec.shots")
    if batch > 65535:
        raise ValueError("batch must be <= 65535 (split the columns / trajectories into several calls)")


def _partial_tape_steps(L, call, info, spec, dev, scratch, stream, n_t: int, state_bytes: int, forced: Optional[int]) -> int:
    """Plan a PARTIAL tape (rydiff.h: need_tape = 3): the trailing save intervals whose factor outputs all stay in HBM.  `forced`
    = the caller's number; None: as many as fit in 80 % of the free + reusable device memory next to the save-point states, the
    backward buffers and (for stored states) the states output.  Leaves the plan for need_tape = 3 in `info` and the count in
    call.problem.tape_steps and returns it; 0 (and an untouched tape_steps) when not even one interval fits or the library would
    not grant the mode."""
    n_steps = n_t - 1
    if forced is not None:
        steps = max(1, min(int(forced), n_steps))
    else:
        probe = _native.RydPlanInfo()
        call.problem.tape_steps = 0
        _native.check(L.rydiff_plan(ctypes.byref(call.problem), 1, 1, _ptr(scratch), stream, ctypes.byref(probe)))
        free_bytes, _total = torch.cuda.mem_get_info(dev)
        reusable = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        budget = 0.8 * (free_bytes + reusable) - probe.workspace_bytes - (n_t * state_bytes if spec.store_states else 0)
        per_step = max(probe.total_factors / max(n_steps, 1) - 1.0, 1.0) * state_bytes  # intermediate factor outputs of one interval
        steps = int(min(budget // per_step, n_steps)) if budget > 0 else 0
    if steps < 1:
        return 0
    call.problem.tape_steps = steps
    _native.check(L.rydiff_plan(ctypes.byref(call.problem), 3, 1, _ptr(scratch), stream, ctypes.byref(info)))
    if info.tape_mode != 3:
        call.problem.tape_steps = 0
        return 0
    return steps


def _stream_ptr(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _new_workspace(nbytes: int, dev) -> Tensor:
    """Every byte buffer the library is handed (workspaces, the plan scratch) comes from here: uninitialised device memory.  The
    library writes whatever it reads; tests/test_gpu_workspace_contents.py replaces this seam to hand it hostile contents."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


class _Prepared(NamedTuple):
    """The inputs of one native call as the C ABI reads them (``_prepare``)."""

    amp: Tensor
    det: Tensor
    u: Tensor
    psi: Tensor
    obs: Optional[Tensor]
    ts_host: np.ndarray
    batch: int
    dim: int
    n_t: int
    call: _Call
    xy: Optional[Tensor] = None
    energy_amp: Optional[Tensor] = None
    energy_det: Optional[Tensor] = None


def _prepare(amp: Tensor, det: Tensor, u_pairs: Tensor, tsave: Tensor, psi0: Tensor, spec: ProblemSpec, obs: Optional[Tensor],
             real_amp_grad: bool = False, xy_pairs: Optional[Tensor] = None, energy_amp: Optional[Tensor] = None,
             energy_det: Optional[Tensor] = None) -> _Prepared:
    """What every entry point does first: the inputs must be on the GPU; detached, contiguous copies in the library's dtypes; their
    shapes against the spec; the ctypes problem."""
    for t, name in ((amp, "amp_tables"), (det, "det_tables"), (u_pairs, "u_pairs"), (psi0, "psi0")):
        _require_cuda(t, name)
    amp_c = amp.detach().to(torch.complex128).contiguous()
    det_c = det.detach().to(torch.float64).contiguous()
    u_c = u_pairs.detach().to(torch.float64).contiguous()
    psi_c = psi0.detach().to(torch.complex128).contiguous()
    obs_c = None if obs is None else obs.detach().to(torch.float64).contiguous()
    xy_c = None if xy_pairs is None else xy_pairs.detach().to(torch.float64).contiguous()
    ea_c = None if energy_amp is None else energy_amp.detach().to(torch.complex128).contiguous()
    ed_c = None if energy_det is None else energy_det.detach().to(torch.float64).contiguous()
    ts_host = tsave.detach().to("cpu", torch.float64).numpy()
    if psi_c.ndim != 2:
        raise ValueError(f"psi0 must be (batch, 2^N), got shape {tuple(psi_c.shape)}")
    batch, dim = psi_c.shape
    if dim != 2 ** spec.n_qubits:
        raise ValueError(f"Incompatible shape of initial state.Expected {2 ** spec.n_qubits}, got {dim}.")
    _check_shapes(spec, amp_c, det_c, u_c, obs_c, batch, psi0.device, xy_c, ea_c, ed_c, len(ts_host))
    call = _Call(spec, amp_c, det_c, u_c, ts_host, batch, obs_c, real_amp_grad=real_amp_grad, xy_pairs=xy_c, energy_amp=ea_c,
                 energy_det=ed_c)
    return _Prepared(amp_c, det_c, u_c, psi_c, obs_c, ts_host, batch, dim, len(ts_host), call, xy_c, ea_c, ed_c)


class _RydbergEvolve(torch.autograd.Function):
    """states, expect = evolve(amp_tables, det_tables, u_pairs, tsave, psi0; obs_diag, spec; xy_pairs, energy_amp, energy_det)."""

    @staticmethod
    def forward(ctx, amp: Tensor, det: Tensor, u_pairs: Tensor, tsave: Tensor, psi0: Tensor,
                obs: Optional[Tensor], spec: ProblemSpec, xy_pairs: Optional[Tensor] = None, energy_amp: Optional[Tensor] = None,
                energy_det: Optional[Tensor] = None):
        L = _native.lib()
        dev = psi0.device
        # (real_amp_grad only matters to the adjoint launches; set here as well so that the plan's kernel_bwd names what will run)
        if xy_pairs is not None:
            _require_cuda(xy_pairs, "xy_pairs")
        for t, name in ((energy_amp, "energy_amp"), (energy_det, "energy_det")):
            if t is not None:
                _require_cuda(t, name)
        amp_c, det_c, u_c, psi_c, obs_c, ts_host, batch, dim, n_t, call, xy_c, ea_c, ed_c = _prepare(
            amp, det, u_pairs, tsave, psi0, spec, obs, real_amp_grad=not amp.is_complex(), xy_pairs=xy_pairs, energy_amp=energy_amp,
            energy_det=energy_det)
        # the kernel variant this call resolved to (spec field, else the CALLING thread's default): the backward pass runs on the
        # autograd engine's device thread, where that thread-local default is not visible
        ctx.kernel_variant = int(call.problem.kernel_variant)
        ctx.shot_buffers = None
        if spec.shots is not None:
            if not isinstance(spec.shots, ShotRequest):
                raise TypeError(f"ProblemSpec.shots must be a ShotRequest, got {type(spec.shots)}")
            shot_times = spec.shots.resolve_times(n_t)
            with torch.cuda.device(dev):
                shot_u = spec.shots.draw_uniforms(len(shot_times), batch, dev)
                shot_out = torch.empty(shot_u.shape, dtype=torch.int32, device=dev)
            call.set_shots(shot_times, shot_u, shot_out)
            ctx.shot_buffers = call.shot_buffers
        needs_grad = any(ctx.needs_input_grad[:5]) or any(ctx.needs_input_grad[7:10])
        need_tape = int(bool(needs_grad and not spec.store_states))
        with torch.cuda.device(dev):
            stream = _stream_ptr(dev)
            scratch = _new_workspace(_native.PLAN_SCRATCH_BYTES, dev)
            info = _native.RydPlanInfo()
            # with the trajectory kept in the workspace tape, size the workspace for the backward sweep right away
            # (every register size has a tape-mode adjoint: the launch-per-factor sweeps from 12 qubits on, the one-launch
            # sweeps below, which otherwise recompute the factor inputs on chip)
            if needs_grad and spec.tape in ("auto", "full"):
                # FULL tape (every factor output kept, no recompute in the adjoint sweep) when HBM has room for it — also next
                # to stored states (the states at the save points are then copied out of the tape), where it is granted
                _native.check(L.rydiff_plan(ctypes.byref(call.problem), 2, 1, _ptr(scratch), stream, ctypes.byref(info)))
                fits = spec.tape == "full" or info.workspace_bytes < _SMALL_TAPE_BYTES
                if not fits:  # the allocator queries cost ~0.3 ms of host time: only asked when the answer is not obvious
                    free_bytes, _total = torch.cuda.mem_get_info(dev)
                    reusable = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
                    fits = info.workspace_bytes < 0.8 * (free_bytes + reusable)
                if fits and (need_tape or info.tape_mode == 2):
                    need_tape = 2
                elif info.tape_mode == 2 and spec.n_qubits >= 13 and n_t > 2:
                    # the full tape does not fit: keep the factor outputs of as many TRAILING intervals as do (need_tape = 3) — the
                    # adjoint sweep then recomputes the earlier intervals only
                    steps = _partial_tape_steps(L, call, info, spec, dev, scratch, stream, n_t, batch * dim * 16, None)
                    if steps:
                        need_tape = 3
            if needs_grad and spec.tape == "partial":
                steps = _partial_tape_steps(L, call, info, spec, dev, scratch, stream, n_t, batch * dim * 16, spec.tape_steps)
                if steps:
                    need_tape = 3
            if need_tape < 2:
                # a differentiated run is planned WITH the backward-sweep buffers: the backward call then reuses this plan
                # (rydiff_plan holds the library's only stream synchronisation)
                _native.check(L.rydiff_plan(ctypes.byref(call.problem), need_tape, int(needs_grad), _ptr(scratch),
                                            stream, ctypes.byref(info)))
            workspace = None
            for attempt in range(3):
                try:
                    workspace = _new_workspace(info.workspace_bytes, dev)
                    break
                except torch.OutOfMemoryError:
                    # The fit test above counts the caching allocator's free blocks as reusable, but a cached block that is a little
                    # SMALLER than this request (the previous run's tape) cannot serve it.  First hand the cache back to the driver
                    # and ask again; if the full tape still does not come (memory the driver has not returned yet, a second tenant),
                    # fall back to one state per save point + recompute, which is what the solver does whenever the full tape
                    # does not fit.  An explicitly requested full tape is not downgraded.
                    if attempt == 0:
                        torch.cuda.synchronize(dev)
                        torch.cuda.empty_cache()
                    elif attempt == 1 and need_tape >= 2 and spec.tape != "full":
                        need_tape = int(bool(needs_grad and not spec.store_states))
                        call.problem.tape_steps = 0
                        _native.check(L.rydiff_plan(ctypes.byref(call.problem), need_tape, int(needs_grad), _ptr(scratch),
                                                    stream, ctypes.byref(info)))
                    else:
                        raise
            states = (torch.empty((n_t, batch, dim), dtype=torch.complex128, device=dev) if spec.store_states
                      else torch.empty((0, batch, dim), dtype=torch.complex128, device=dev))
            n_obs = call.expect_rows()
            expect = torch.empty((n_obs, n_t, batch), dtype=torch.float64, device=dev)
            _native.check(L.rydiff_forward(ctypes.byref(call.problem), ctypes.byref(info), _ptr(psi_c),
                                           _ptr(states) if spec.store_states else None,
                                           _ptr(expect) if n_obs else None, _ptr(workspace),
                                           workspace.numel(), need_tape, stream))
            if spec.shots is not None:
                spec.shots.indices = shot_out.to(torch.int64) & 0xFFFFFFFF  # (the library writes unsigned 32-bit indices)
                spec.shots.time_indices = tuple(int(k) for k in shot_times)
                spec.shots.last_uniforms = shot_u
        ctx.spec = spec
        ctx.info = info
        ctx.tsave_host = ts_host
        ctx.tsave_meta = (tsave.device, tsave.dtype)
        ctx.in_dtypes = (amp.dtype, det.dtype, u_pairs.dtype, psi0.dtype)
        ctx.xy = xy_c  # (a constant of the backward pass, like the masks: not an output, kept on the context)
        ctx.xy_dtype = None if xy_pairs is None else xy_pairs.dtype
        ctx.energy = (ea_c, ed_c)  # (inputs of the backward pass that are not saved outputs: kept on the context, like xy)
        ctx.energy_dtypes = (None if energy_amp is None else energy_amp.dtype, None if energy_det is None else energy_det.dtype)
        ctx.need_tape = need_tape
        ctx.tape_steps = int(call.problem.tape_steps)
        ctx.keep_tape = True  # retain_graph=True callers may run backward again
        ctx.tape_workspace = workspace if need_tape else None
        ctx.save_for_backward(amp_c, det_c, u_c, psi_c, obs_c if obs_c is not None else torch.empty(0, device=dev),
                              states)
        ctx.has_obs = obs_c is not None
        ctx.has_expect = n_obs > 0
        ctx.set_materialize_grads(False)
        ctx.stats = {"degree": info.degree, "total_factors": info.total_factors, "rho": info.rho_design,
                     "spectral": (info.spectral_lo, info.spectral_hi), "n_stages": info.n_stages,
                     "tape": ("none", "steps", "full", "partial")[(info.tape_mode if need_tape >= 2 else min(need_tape, info.tape_mode)) if need_tape else 0],
                     "tape_steps": int(call.problem.tape_steps) if need_tape == 3 and info.tape_mode == 3 else 0,
                     "kernel_family": _native.KERNEL_FAMILIES[info.kernel_family],
                     "kernel_fwd": info.kernel_fwd.decode(), "kernel_bwd": info.kernel_bwd.decode()}
        spec.options["_last_stats"] = ctx.stats
        return states, expect

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_states: Optional[Tensor], g_expect: Optional[Tensor]):
        L = _native.lib()
        amp_c, det_c, u_c, psi_c, obs_c, states = ctx.saved_tensors
        spec: ProblemSpec = ctx.spec
        dev = psi_c.device
        batch, dim = psi_c.shape
        obs = obs_c if ctx.has_obs else None
        ea_c, ed_c = ctx.energy
        call = _Call(spec, amp_c, det_c, u_c, ctx.tsave_host, batch, obs, real_amp_grad=not ctx.in_dtypes[0].is_complex,
                     xy_pairs=ctx.xy, energy_amp=ea_c, energy_det=ed_c)
        call.problem.kernel_variant = ctx.kernel_variant  # same kernel family as the forward pass (see forward)
        call.problem.tape_steps = ctx.tape_steps
        if ctx.shot_buffers is not None:  # ignored by the adjoint sweep, but the counts are part of the workspace layout
            call.set_shots(*ctx.shot_buffers)
        need = ctx.needs_input_grad
        if g_states is not None and g_states.numel() == 0:
            g_states = None
        if g_states is not None:
            g_states = g_states.to(torch.complex128).contiguous()
        if g_expect is not None:
            g_expect = g_expect.to(torch.float64).contiguous()
        with torch.cuda.device(dev):
            stream = _stream_ptr(dev)
            g_amp = torch.empty_like(amp_c) if need[0] and amp_c.numel() else None
            g_det = torch.empty_like(det_c) if need[1] and det_c.numel() else None
            g_u = torch.empty_like(u_c) if need[2] and u_c.numel() else None
            g_ts = torch.empty(len(ctx.tsave_host), dtype=torch.float64, device=dev) if need[3] else None
            g_psi = torch.empty_like(psi_c) if need[4] else None
            g_xy = torch.empty_like(ctx.xy) if (need[7] and ctx.xy is not None and ctx.xy.numel()) else None
            call.problem.g_xy = None if g_xy is None else g_xy.data_ptr()
            g_ea = torch.empty_like(ea_c) if (spec.energy and need[8] and ea_c is not None and ea_c.numel()) else None
            g_ed = torch.empty_like(ed_c) if (spec.energy and need[9] and ed_c is not None and ed_c.numel()) else None
            call.problem.g_energy_amp = None if g_ea is None else g_ea.data_ptr()
            call.problem.g_energy_det = None if g_ed is None else g_ed.data_ptr()
            info = ctx.info
            if ctx.need_tape:
                workspace = ctx.tape_workspace  # sized for forward + backward by the forward call
                states_ptr = None
            else:
                workspace = _new_workspace(info.workspace_bytes, dev)  # sized by the forward call's plan
                states_ptr = _ptr(states)
            _native.check(L.rydiff_backward(ctypes.byref(call.problem), ctypes.byref(info), states_ptr, _ptr(g_states),
                                            _ptr(g_expect) if (g_expect is not None and ctx.has_expect) else None,
                                            _ptr(g_amp), _ptr(g_det), _ptr(g_u), _ptr(g_ts), _ptr(g_psi),
                                            _ptr(workspace), workspace.numel(), int(ctx.need_tape), stream))
            if ctx.need_tape:
                ctx.tape_workspace = None if not ctx.keep_tape else ctx.tape_workspace
        a_dt, d_dt, u_dt, p_dt = ctx.in_dtypes
        if g_amp is not None:
            g_amp = g_amp.to(a_dt) if a_dt.is_complex else g_amp.real.to(a_dt)
        if g_det is not None:
            g_det = g_det.to(d_dt)
        if g_u is not None:
            g_u = g_u.to(u_dt)
        if g_ts is not None:
            ts_dev, ts_dt = ctx.tsave_meta
            g_ts = g_ts.to(ts_dev, ts_dt)
        if g_psi is not None:
            g_psi = g_psi.to(p_dt)
        if g_xy is not None:
            g_xy = g_xy.to(ctx.xy_dtype)
        if g_ea is not None:
            ea_dt = ctx.energy_dtypes[0]
            g_ea = g_ea.to(ea_dt) if ea_dt.is_complex else g_ea.real.to(ea_dt)
        if g_ed is not None:
            g_ed = g_ed.to(ctx.energy_dtypes[1])
        return g_amp, g_det, g_u, g_ts, g_psi, None, None, g_xy, g_ea, g_ed


@dataclass
class SolveResult:
    """What the reference reads from pyqtorch's result object: ``.states`` iterable over time (backend.py:513-521)."""

    states: Tensor  # (n_t, dim, B) view, like pyqtorch
    expect: Tensor  # (n_obs + n_pauli, n_t, B) observables evaluated natively, the diagonal ones first
    stats: dict
    overlaps: Optional[Tensor] = None  # complex (n_ov, n_t, B): <phi_o,b | psi_b(t_k)> evaluated natively (differentiable), or None
    shots: Optional[ShotRequest] = None  # the request handed to sesolve(shots=...), holding the native shots (.indices)
    rdms: Optional[list] = None  # per ReducedDensityMatrix: complex (n_t, B, 2^m, 2^m), evaluated natively (differentiable), or None
    moments: Optional[Tensor] = None  # (1 + N + N(N-1)/2, n_t, B): S, B_q, B_qr evaluated natively (differentiable), or None
    energy: Optional[Tensor] = None  # (1 | 2, n_t, B): E(t_k) = <psi_k|H(t_k)|psi_k>, then M2 = |H(t_k) psi_k|^2, evaluated natively (differentiable), or None


def split_expect(expect: Tensor, n_overlaps: int) -> tuple[Tensor, Optional[Tensor]]:
    """The `expect` output of ``evolve`` -> (diagonal and Pauli rows, complex overlaps (n_ov, n_t, B) or None)."""
    if not n_overlaps:
        return expect, None
    n_real = expect.shape[0] - 2 * n_overlaps
    pairs = expect[n_real:].reshape(n_overlaps, 2, *expect.shape[1:])
    return expect[:n_real], torch.complex(pairs[:, 0], pairs[:, 1])


def split_energy(expect: Tensor, energy: int) -> tuple[Tensor, Optional[Tensor]]:
    """Takes the energy rows (``ProblemSpec.energy`` = 1: E; 2: E, M2), the last block of a ket's rows — behind the moments — off the
    END of `expect`, before ``split_moments`` and ``split_observables`` take theirs: -> (the other rows, the energy rows
    (energy, n_t, B) or None).  ``energy = 0``: `expect` as it is."""
    energy = int(energy)
    if not energy:
        return expect, None
    if energy not in (1, 2) or expect.shape[0] < energy:
        raise ValueError(f"split_energy: energy must be 0, 1 or 2 and `expect` must hold that many rows, got {energy} and {expect.shape[0]} rows")
    return expect[:expect.shape[0] - energy], expect[expect.shape[0] - energy:]


def split_ket_tail(expect: Tensor, n_qubits: int, moments: bool = False, energy: int = 0) -> tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """The one splitter of the blocks at the END of a ket's `expect`, in the only order that is right (the energy rows sit behind the
    moments): -> (the rows ``split_observables`` takes, the moments (1 + N + N(N-1)/2, n_t, B) or None, the energy rows
    (energy, n_t, B) or None)."""
    expect, en = split_energy(expect, energy)
    mom = None
    if moments:
        expect, mom = split_moments(expect, n_qubits)
    return expect, mom, en


def split_observables(expect: Tensor, n_overlaps: int, rdms=None, energy: int = 0) -> tuple:
    """``split_expect`` that also takes the reduced-density-matrix rows out: `expect` of ``evolve`` -> (diagonal and Pauli rows,
    complex overlaps (n_ov, n_t, B) or None, one complex (n_t, B, 2^m, 2^m) per entry of ``rdms`` or None).  ``rdms``: what
    ``ProblemSpec.rdms`` held — ``ReducedDensityMatrix`` objects (the matrices come back in the order of their ``qubits``) or integer
    masks (ascending qubit order, the library's).  ``energy`` (``ProblemSpec.energy``) > 0: the energy rows, which sit behind every
    other row of a ket, are taken off the end first and returned as a fourth entry (a run that also asked for the moments takes
    both tail blocks off with ``split_ket_tail`` first); 0: the three entries as before."""
    if energy:
        expect, en = split_energy(expect, energy)
        return split_observables(expect, n_overlaps, rdms) + (en,)
    rdms = list(rdms or [])
    if not rdms:
        return split_expect(expect, n_overlaps) + (None,)
    ms = [o.n_sub if isinstance(o, ReducedDensityMatrix) else bin(int(o)).count("1") for o in rdms]
    first = expect.shape[0] - sum(2 * 4 ** m for m in ms)
    out = []
    for o, m in zip(rdms, ms):
        d = 2 ** m
        rows = expect[first:first + 2 * d * d].reshape(d, d, 2, *expect.shape[1:])  # (a, a', Re | Im, n_t, B)
        rho = torch.complex(rows[:, :, 0], rows[:, :, 1]).permute(2, 3, 0, 1)
        if isinstance(o, ReducedDensityMatrix):
            perm = o.native_index().to(rho.device)
            rho = rho.index_select(2, perm).index_select(3, perm)
        out.append(rho)
        first += 2 * d * d
    real, ov = split_expect(expect[:expect.shape[0] - sum(2 * 4 ** m for m in ms)], n_overlaps)
    return real, ov, out


def split_moments(expect: Tensor, n_qubits: int) -> tuple[Tensor, Tensor]:
    """Takes the moments block of the occupation correlations (``ProblemSpec.moments``) off the END of a ket's `expect`:
    -> (the other rows, as ``split_observables`` takes them; the moments (1 + N + N(N-1)/2, n_t, B): S, B_q, B_qr)."""
    n = moment_rows(n_qubits)
    if expect.shape[0] < n:
        raise ValueError(f"expect holds {expect.shape[0]} rows: fewer than the {n} moment rows of {n_qubits} qubits")
    return expect[:expect.shape[0] - n], expect[expect.shape[0] - n:]


def split_dm_moments(expect: Tensor, n_atoms: int) -> tuple[Tensor, Tensor]:
    """Takes the occupation correlations of a density-matrix register (``DensityMatrixObservables.moments``), the last block of
    all, off the END of `expect` — before ``split_observables`` takes the reduced density matrices in front of it:
    -> (the other rows; the moments (1 + n + n(n-1)/2, n_t, B): S, B_q, B_qr of the diagonal of rho)."""
    n = moment_rows(n_atoms)
    if expect.shape[0] < n:
        raise ValueError(f"expect holds {expect.shape[0]} rows: fewer than the {n} moment rows of {n_atoms} atoms")
    return expect[:expect.shape[0] - n], expect[expect.shape[0] - n:]


def frame_factor(n_sub: int, phi: float) -> Tensor:
    """``exp(-i phi (ones(a) - ones(a')))``, ``(2^m, 2^m)``: takes a reduced density matrix of the state ``V psi`` in the frame that
    rotates with a constant drive phase ``phi`` (``V = exp(i phi * number of ones)``) back to the lab frame."""
    ones = torch.tensor([bin(a).count("1") for a in range(2 ** n_sub)], dtype=torch.float64)
    return torch.exp(-1j * phi * (ones[:, None] - ones[None, :]))


def evolve(amp_tables: Tensor, det_tables: Tensor, u_pairs: Tensor, tsave: Tensor, psi0: Tensor,
           spec: ProblemSpec, obs_diag: Optional[Tensor] = None, xy_pairs: Optional[Tensor] = None,
           energy_amp: Optional[Tensor] = None, energy_det: Optional[Tensor] = None) -> tuple[Tensor, Tensor]:
    """Low-level entry: psi0 is (B, dim); returns states (n_t, B, dim) and expect (n_obs + n_pauli + 2 n_overlaps, n_t, B)
    (``split_expect`` takes the overlap rows of ``spec.overlaps`` out as complex numbers).  ``spec.shots`` (a ``ShotRequest``)
    receives its measurement shots as a by-product; the return value does not change.  ``xy_pairs`` (with ``spec.xy_mode``): the
    N(N-1)/2 exchange couplings J_ij in the order of ``u_pairs``, a device tensor that takes part in autograd (``g_xy``).
    ``energy_amp`` / ``energy_det`` (with ``spec.energy``): the coefficient tables at the evaluation times, (coeff_batch, terms, n_t)
    in the conventions of ``amp_tables`` / ``det_tables``; the energy rows E (and M2) are the last rows of ``expect``
    (``split_energy``), and the explicit dependence of H(t_k) on the two tables comes back as their gradients."""
    return _RydbergEvolve.apply(amp_tables, det_tables, u_pairs, tsave, psi0, obs_diag, spec, xy_pairs, energy_amp, energy_det)


def sesolve(problem, psi0: Tensor, tsave: Tensor, solver: SolverType = SolverType.DP5_SE,
            options: Optional[dict] = None, obs_diag: Optional[Tensor] = None, store_states: bool = True,
            pauli_obs: Optional[Sequence[PauliObservable]] = None,
            overlap_obs: Optional[Sequence[StateOverlap]] = None, shots: Union[None, int, ShotRequest] = None,
            rdm_obs: Optional[Sequence[ReducedDensityMatrix]] = None, moments: bool = False, energy: int = 0) -> SolveResult:
    """Drop-in for ``pyqtorch.sesolve(H=..., psi0, tsave, solver, options)`` at ``backend.py:488-494``.

    ``problem`` is the structured Hamiltonian (``pulser_diff_amd.hamiltonian.Hamiltonian``) instead of the opaque
    callable; ``psi0`` is ``(dim, B)`` as in the reference.  ``pauli_obs``: Pauli-string observables evaluated natively; their
    values follow the diagonal ones in ``SolveResult.expect``.  ``overlap_obs``: ``StateOverlap`` observables evaluated natively
    into ``SolveResult.overlaps``.  ``shots``: a ``ShotRequest`` (or an int: that many shots at the final time) filled natively and
    returned as ``SolveResult.shots``; its indices are in the basis order of the native register (three-level registers: two qubits
    per atom, see ``shots.indices_to_bitstrings``).  ``rdm_obs``: ``ReducedDensityMatrix`` observables evaluated natively into
    ``SolveResult.rdms`` (lab frame, the order of their ``qubits``).  ``moments``: the occupation correlations — the moments
    ``S, B_q, B_qr`` of ``|psi|^2`` over the index bits — evaluated natively into ``SolveResult.moments`` (diagonal: they do not see
    the rotating frame).  ``energy`` (1, or 2 for the second moment too): ``E(t_k) = <psi_k|H(t_k)|psi_k>`` and ``|H(t_k) psi_k|^2`` with
    the problem's own Hamiltonian at the evaluation times (``Hamiltonian.energy_tables``), evaluated natively into ``SolveResult.energy``.
    """
    options = dict(options or {})
    spec = problem.problem_spec(solver=solver, tol=tolerance_from_options(options), store_states=store_states)
    if shots is not None:
        spec.shots = shots if isinstance(shots, ShotRequest) else ShotRequest(int(shots))
    psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1)
    amp_tables = problem.amp_tables.real if getattr(problem, "amp_is_real", False) else problem.amp_tables
    embed = None
    if getattr(problem, "basis_name", None) == "all":
        # three levels per atom = two qubits per atom: scatter the 3^n amplitudes (and diagonal observables) into the 4^n
        # vector, gather the states back; the unused codes carry exact zeros (nothing couples to them)
        embed = problem.embedded_three_level().to(psi_bd.device)
        big = torch.zeros(psi_bd.shape[0], 1 << spec.n_qubits, dtype=psi_bd.dtype, device=psi_bd.device)
        psi_bd = big.index_copy(1, embed, psi_bd)
        if obs_diag is not None:
            obs_diag = torch.zeros(obs_diag.shape[0], 1 << spec.n_qubits, dtype=obs_diag.dtype,
                                   device=obs_diag.device).index_copy(1, embed, obs_diag)
    overlap_obs = list(overlap_obs or [])
    targets = None
    if overlap_obs:
        # (n_ov, 1 | B, dim) in the basis the states are stored in; three levels: scattered like psi0, zeros on the unused codes
        targets = pack_overlaps(overlap_obs, psi_bd.shape[1] if embed is None else embed.numel(), psi_bd.shape[0], psi_bd.device)
        if embed is not None:
            targets = torch.zeros(*targets.shape[:2], 1 << spec.n_qubits, dtype=targets.dtype,
                                  device=targets.device).index_copy(2, embed, targets)
    rdm_obs = list(rdm_obs or [])
    if rdm_obs:
        if embed is not None:
            raise NotImplementedError("ReducedDensityMatrix is not available in the three-level all-basis (an atom is two qubits "
                                      "there); trace the stored states instead.")
        spec.rdms = rdm_obs
    if moments:
        if embed is not None:
            raise NotImplementedError("OccupationCorrelations is not available in the three-level all-basis (an atom is two qubits "
                                      "there); reduce the stored states instead.")
        spec.moments = True
    energy = int(energy)
    if energy:
        if embed is not None:
            raise NotImplementedError("Energy is not available in the three-level all-basis (conditioned terms are not part of the "
                                      "native energy rows); apply get_hamiltonian to the stored states instead.")
        if spec.pair_terms:
            raise NotImplementedError("Energy is not available with dense pair terms (the XY mode on the dense route, master-equation "
                                      "runs); the XY mode takes it on the native exchange term: TorchEmulator(..., xy_native=True).")
        if spec.xy_mode == 2:
            raise NotImplementedError("Energy needs a Hermitian Hamiltonian: the XY exchange as the reference writes it is one-directional. "
                                      "Pass xy_hermitian=True to TorchEmulator (Hamiltonian.XY_HERMITIAN = True).")
        spec.energy = energy
    pauli_obs = list(pauli_obs or [])
    if pauli_obs and embed is not None:
        raise NotImplementedError("Pauli observables are not available in the three-level all-basis; use results.expect on stored states.")
    rot = None
    phi = getattr(problem, "frame_phase", None)
    if pauli_obs and phi is not None and not spec.pair_terms:
        # off-diagonal observables DO see the frame: the library gets V O V^dagger (a string with k flipped qubits becomes 2^k).
        # Where that would exceed the cap of strings per call the frame stays off for this call (complex tables: slower kernels,
        # same numbers).
        rotated = [o.rotated(float(phi)) for o in pauli_obs]
        if sum(len(o) for o in rotated) <= _native.MAX_PAULI_STRINGS:
            pauli_obs = rotated
        else:
            phi = None
    if pauli_obs:
        spec.pauli = pauli_obs
    if phi is not None and embed is None and not spec.pair_terms:
        # one constant drive phase: evolve in the frame that rotates with it (hamiltonian.py: frame_phase) — real tables, V psi0 in,
        # V^dagger psi(t) out; diagonal observables do not see the frame
        amp_tables = problem.amp_tables_frame
        x = torch.arange(1 << spec.n_qubits, device=psi_bd.device)
        ones = torch.zeros(1 << spec.n_qubits, dtype=torch.float64, device=psi_bd.device)
        for j in range(spec.n_qubits):
            ones += ((x >> j) & 1).to(torch.float64)
        rot = torch.exp(1j * float(phi) * ones)
        psi_bd = psi_bd * rot[None, :]
        if targets is not None:  # <phi|psi> = <V phi|V psi>: the targets go into the frame with psi0
            targets = targets * rot[None, None, :]
    if targets is not None:
        spec.overlaps = targets.contiguous()
    e_amp = e_det = None
    if spec.energy:
        # the tables at the evaluation times, in the frame the states are evolved in (<V psi|V H V^dagger|V psi> = <psi|H|psi>)
        e_amp, e_det = problem.energy_tables(tsave, frame=rot is not None)
        if getattr(problem, "amp_is_real", False):
            e_amp = e_amp.real
    states, expect = evolve(amp_tables, problem.det_tables, problem.u_pairs, tsave, psi_bd, spec, obs_diag,
                            xy_pairs=problem.xy_pairs if spec.xy_mode else None, energy_amp=e_amp, energy_det=e_det)
    if rot is not None and states.numel():
        states = states * rot.conj()[None, None, :]
    if embed is not None and states.numel():
        states = states.index_select(2, embed)
    expect, mom, en = split_ket_tail(expect, spec.n_qubits, spec.moments, spec.energy)
    expect, overlaps, rdms = split_observables(expect, len(overlap_obs), rdm_obs)
    if rdms is not None and rot is not None:
        # the library saw V psi: rho_lab[a][a'] = rho[a][a'] exp(-i phi (ones(a) - ones(a'))), on the small matrix (differentiable)
        rdms = [r * frame_factor(o.n_sub, float(phi)).to(r.device) for o, r in zip(rdm_obs, rdms)]
    return SolveResult(states.permute(0, 2, 1) if states.numel() else states, expect,
                       dict(spec.options.get("_last_stats", {})), overlaps, spec.shots, rdms, mom, en)


def _tangent_take(t: Optional[Tensor], sel, shape: tuple, dtype: torch.dtype, name: str, dev) -> Optional[Tensor]:
    """The directions ``sel`` (a slice or a list of indices) of one tangent input as the contiguous device buffer the C ABI reads
    (None stays None)."""
    if t is None:
        return None
    _require_cuda(t, name)
    if tuple(t.shape[1:]) != tuple(shape):
        raise ValueError(f"{name} must have shape (n_dir, {', '.join(str(s) for s in shape)}), got {tuple(t.shape)}")
    return t[sel].detach().to(dev, dtype).contiguous()


def _tangent_buffers(sel, pre: _Prepared, d_amp, d_det, d_u, d_psi0, dev, d_xy=None) -> tuple:
    """(d_amp, d_det, d_u, d_psi0, d_xy)[sel] for RydTangent; None: not given, or the tangent of an input this problem does not have."""
    return (_tangent_take(d_amp, sel, pre.amp.shape, torch.complex128, "d_amp", dev) if pre.amp.numel() else None,
            _tangent_take(d_det, sel, pre.det.shape, torch.float64, "d_det", dev) if pre.det.numel() else None,
            _tangent_take(d_u, sel, pre.u.shape, torch.float64, "d_u", dev) if pre.u.numel() else None,
            _tangent_take(d_psi0, sel, pre.psi.shape, torch.complex128, "d_psi0", dev),
            _tangent_take(d_xy, sel, pre.xy.shape, torch.float64, "d_xy", dev) if (pre.xy is not None and pre.xy.numel()) else None)


def _sweep_prepare(name: str, amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0,
                   xy_pairs=None, d_xy=None):
    """What ``evolve_tangent`` and ``evolve_geometry`` (`name`) share behind their refusals: the number of directions, the inputs of
    the call, its row count."""
    if d_xy is not None and xy_pairs is None:
        raise ValueError(f"{name}: d_xy given without xy_pairs (the tangent of couplings the problem does not have)")
    given = [t for t in (d_amp, d_det, d_u, d_psi0, d_xy) if t is not None]
    if not given:
        raise ValueError(f"{name} needs at least one of d_amp, d_det, d_u, d_psi0" + (", d_xy" if xy_pairs is not None else ""))
    n_dir = int(given[0].shape[0])
    if n_dir < 1 or any(int(t.shape[0]) != n_dir for t in given):
        raise ValueError("d_amp, d_det, d_u, d_psi0 must agree on the number of directions (their first axis), at least one")
    if xy_pairs is not None:
        _require_cuda(xy_pairs, "xy_pairs")
    pre = _prepare(amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag, xy_pairs=xy_pairs)
    pre.call.problem.kernel_variant = 0  # the tangent sweep has one kernel family
    return n_dir, pre, pre.call.expect_rows()


def _sweep_plan(L, p, dev) -> tuple:
    """(stream, plan, plan scratch) of the sweeps of one call; inside ``torch.cuda.device(dev)``."""
    stream = _stream_ptr(dev)
    scratch = _new_workspace(_native.PLAN_SCRATCH_BYTES, dev)
    info = _native.RydPlanInfo()
    _native.check(L.rydiff_plan(ctypes.byref(p), 0, 0, _ptr(scratch), stream, ctypes.byref(info)))
    return stream, info, scratch


def _sweep_tangent(n_dir: int, bufs: tuple, flags: int) -> "_native.RydTangent":
    tg = _native.RydTangent()
    tg.n_dir = n_dir
    tg.d_amp, tg.d_det, tg.d_u, tg.d_psi0, tg.d_xy = (None if b is None else b.data_ptr() for b in bufs)
    tg.flags = int(flags)
    return tg


def _sweep_workspace(size_fn, size_name: str, sweep, p, info, tg, workspace: Optional[Tensor], dev) -> Tensor:
    """The workspace of one sweep: `workspace` where it is large enough for what ``size_fn`` asks, else a new one.  ``sweep(ws)``
    makes the call on the workspace `ws`."""
    need = size_fn(ctypes.byref(p), ctypes.byref(info), tg.n_dir, tg.flags)
    if need == 0:  # refused: the sweep's own (host-only) validation reports why, with its error code
        _native.check(sweep(None))
        raise RuntimeError(f"{size_name} returned 0: " + _native.last_error())
    if workspace is None or workspace.numel() < need:
        workspace = _new_workspace(need, dev)
    return workspace


def evolve_tangent(amp_tables: Tensor, det_tables: Tensor, u_pairs: Tensor, tsave: Tensor, psi0: Tensor, spec: ProblemSpec,
                   obs_diag: Optional[Tensor] = None, d_amp: Optional[Tensor] = None, d_det: Optional[Tensor] = None,
                   d_u: Optional[Tensor] = None, d_psi0: Optional[Tensor] = None, flags: int = 0,
                   xy_pairs: Optional[Tensor] = None, d_xy: Optional[Tensor] = None) -> tuple[Tensor, Tensor]:
    """Forward-mode twin of ``evolve`` (``rydiff_forward_tangent``): ONE sweep carries the state and the tangent states of up to 8
    directions through every factor and returns the observable values ``expect`` (rows, n_t, B) and their directional derivatives
    ``dexpect`` (n_dir, rows, n_t, B) at EVERY evaluation time — rows = diagonal observables, then the Pauli observables and Re / Im
    of the overlaps of ``spec``, as in ``evolve``.  A direction d is the tangent of the inputs: ``d_amp[d]`` shaped like
    ``amp_tables``, ``d_det[d]`` like ``det_tables``, ``d_u[d]`` like ``u_pairs``, ``d_psi0[d]`` like ``psi0`` (B, dim); an
    input left out has tangent zero.  More than 8 directions run in chunks of 8.  No autograd graph hangs off the outputs.

    ``flags`` (``RydTangent.flags``) opts into what the sweep takes beyond plain Ising kets; without them such a problem is refused as
    it always was.  ``_native.TANGENT_PAIR_TERMS``: ``spec.pair_terms`` (the XY exchange; the dissipator of a master-equation run)
    ride in the same sweep, constants in every direction.  ``_native.TANGENT_DENSITY_MATRIX``: with ``spec.dm`` the register is the
    doubled register of a density matrix (``lindblad.mesolve_tangent`` builds the doubled tables and their tangents): ``psi0`` /
    ``d_psi0`` are ``vec(rho0)`` / ``vec(d rho0)``, and the density-matrix rows — diagonal, Pauli, fidelity, purity — and their
    tangents follow the other rows, as in ``evolve``.  ``_native.TANGENT_RDMS``: the reduced density matrices of ``spec.rdms`` (kets
    only) join the rows behind the overlaps, values in ``expect`` and ``d rho_A = Tr_E(|dpsi><psi| + |psi><dpsi|)`` in ``dexpect``;
    ``split_observables`` takes them out of ``expect`` and, direction by direction, out of ``dexpect[d]``.
    ``_native.TANGENT_MOMENTS``: the occupation correlations of ``spec.moments`` (kets only) join the rows behind the RDM block — the
    moments ``S, B_q, B_qr`` in ``expect``, the same moments of ``2 Re(conj psi . dpsi_d)`` in ``dexpect[d]``, formed in a fixed order
    (two calls return the same bits); ``split_moments`` takes the block off ``expect`` and off each ``dexpect[d]``.  The flag without
    ``spec.moments`` is a ``ValueError`` (``RYDIFF_EINVAL``: it asks for a block the problem does not have).

    ``xy_pairs`` (with ``spec.xy_mode``): the couplings of the native XY exchange, as in ``evolve``; handing them in is the opt-in
    (``_native.TANGENT_XY`` is set here) and the exchange stencil rides in the sweep at every register size.  ``d_xy[d]`` shaped like
    ``xy_pairs`` is direction d's tangent of the couplings — a tangent input like the others, valid on its own.  ``spec.xy_mode``
    without ``xy_pairs`` stays the ``NotImplementedError`` it was."""
    if (spec.rdms is not None and not (int(flags) & _native.TANGENT_RDMS)) or (spec.dm is not None and spec.dm.rdms is not None):
        raise NotImplementedError("evolve_tangent evaluates no reduced density matrices (rydiff_forward_tangent: RYDIFF_ENOTIMPL) unless "
                                  "flags has _native.TANGENT_RDMS (kets only); or request them from evolve")
    if spec.dm is not None and not (int(flags) & _native.TANGENT_DENSITY_MATRIX):
        raise NotImplementedError("evolve_tangent takes no density-matrix registers (rydiff_forward_tangent: RYDIFF_ENOTIMPL) unless "
                                  "flags has _native.TANGENT_DENSITY_MATRIX (lindblad.mesolve_tangent); or differentiate evolve")
    if spec.moments and (spec.dm is not None or not (int(flags) & _native.TANGENT_MOMENTS)):
        raise NotImplementedError("evolve_tangent evaluates no occupation correlations (rydiff_forward_tangent: RYDIFF_ENOTIMPL) unless "
                                  "flags has _native.TANGENT_MOMENTS (kets only); or request them from evolve")
    if spec.shots is not None or (spec.dm is not None and spec.dm.shots):
        raise NotImplementedError("evolve_tangent draws no measurement shots (rydiff_forward_tangent: RYDIFF_ENOTIMPL); request them from evolve")
    if spec.xy_mode and xy_pairs is None:
        raise NotImplementedError("evolve_tangent takes no XY exchange term (rydiff_forward_tangent: RYDIFF_ENOTIMPL with xy_mode != 0); "
                                  "differentiate evolve, or run the dense pair-term route with _native.TANGENT_PAIR_TERMS")
    L = _native.lib()
    dev = psi0.device
    if xy_pairs is not None:
        flags = int(flags) | _native.TANGENT_XY
    n_dir, pre, rows = _sweep_prepare("evolve_tangent", amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag,
                                      d_amp, d_det, d_u, d_psi0, xy_pairs, d_xy)
    p, n_t, batch = pre.call.problem, pre.n_t, pre.batch
    expect = torch.empty((rows, n_t, batch), dtype=torch.float64, device=dev)
    dexpect = torch.empty((n_dir, rows, n_t, batch), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream, info, _scratch = _sweep_plan(L, p, dev)
        workspace = None
        values_done = False
        for d0 in range(0, n_dir, _native.MAX_TANGENTS):
            d1 = min(n_dir, d0 + _native.MAX_TANGENTS)
            bufs = _tangent_buffers(slice(d0, d1), pre, d_amp, d_det, d_u, d_psi0, dev, d_xy)
            out = dexpect[d0:d1]
            if all(b is None for b in bufs):  # tangents of inputs this problem does not have: the derivative is zero
                out.zero_()
                continue
            tg = _sweep_tangent(d1 - d0, bufs, flags)
            want_values = rows > 0 and not values_done

            def sweep(ws):
                return L.rydiff_forward_tangent(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), _ptr(pre.psi),
                                                _ptr(expect) if want_values else None, _ptr(out), _ptr(ws),
                                                0 if ws is None else ws.numel(), stream)

            workspace = _sweep_workspace(L.rydiff_tangent_workspace_bytes_flags, "rydiff_tangent_workspace_bytes", sweep, p, info, tg,
                                         workspace, dev)
            values_done = True
            _native.check(sweep(workspace))
    if rows and not values_done:  # no chunk reached the library (tangents of inputs the problem does not have)
        with torch.no_grad():
            expect = evolve(pre.amp, pre.det, pre.u, tsave.detach(), pre.psi, replace(spec, store_states=False), pre.obs,
                            xy_pairs=pre.xy)[1]
    return expect, dexpect


def evolve_geometry(amp_tables: Tensor, det_tables: Tensor, u_pairs: Tensor, tsave: Tensor, psi0: Tensor, spec: ProblemSpec,
                    obs_diag: Optional[Tensor] = None, d_amp: Optional[Tensor] = None, d_det: Optional[Tensor] = None,
                    d_u: Optional[Tensor] = None, d_psi0: Optional[Tensor] = None, flags: int = 0,
                    xy_pairs: Optional[Tensor] = None, d_xy: Optional[Tensor] = None) -> tuple[Tensor, Tensor, Tensor]:
    """``evolve_tangent`` that also returns the Gram matrix of the state and its tangents at EVERY evaluation time
    (``rydiff_forward_geometry``): ``(expect, dexpect, gram)`` with ``gram`` complex128 of shape (n_t, B, 1 + n_dir, 1 + n_dir),
    ``gram[k, b, i, j] = <v_i|v_j>``, ``v_0 = psi_b(t_k)``, ``v_{1+d} = d psi_b(t_k) / d theta_d`` — what
    ``geometry.quantum_fisher_information`` and its neighbours take.  The sums are formed in a fixed order: two calls on the same
    inputs return bit-identical matrices.  Same arguments as ``evolve_tangent``; tangents of inputs the problem does not have give
    zero rows and columns.  More than 8 directions run one sweep per pair of groups of 4 (``geometry.geometry_sweeps``).
    ``flags=_native.TANGENT_PAIR_TERMS`` takes dense pair terms on kets, ``_native.TANGENT_RDMS`` the reduced density matrices of
    ``spec.rdms`` (rows as in ``evolve_tangent``; their sums use atomics and are not part of the fixed order),
    ``_native.TANGENT_MOMENTS`` the occupation correlations of ``spec.moments`` (fixed order, like the Gram matrix, which they leave
    as it is); density-matrix registers stay refused.  ``xy_pairs`` / ``d_xy``: the native XY exchange and the tangents of its
    couplings, as in ``evolve_tangent``."""
    return _evolve_gram(False, amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0, flags,
                        xy_pairs, d_xy)[:3]


def evolve_fisher(amp_tables: Tensor, det_tables: Tensor, u_pairs: Tensor, tsave: Tensor, psi0: Tensor, spec: ProblemSpec,
                  obs_diag: Optional[Tensor] = None, d_amp: Optional[Tensor] = None, d_det: Optional[Tensor] = None,
                  d_u: Optional[Tensor] = None, d_psi0: Optional[Tensor] = None, flags: int = 0,
                  xy_pairs: Optional[Tensor] = None, d_xy: Optional[Tensor] = None) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``evolve_geometry`` that also returns the classical Gram matrix of the occupation-basis measurement at EVERY evaluation time
    (``rydiff_forward_fisher``): ``(expect, dexpect, gram, cgram)`` with ``cgram`` float64 of shape (n_t, B, 1 + n_dir, 1 + n_dir),
    ``cgram[k, b, i, j] = sum_y w_i[y] w_j[y]``, ``w_0 = |psi_b(t_k)|``, ``w_{1+d} = 2 Re(conj(psi / |psi|) d psi_b(t_k) / d theta_d)``
    — what ``geometry.classical_fisher_information`` and ``geometry.fisher_efficiency`` take; ``observables.classical_gram`` is the
    same matrix in torch on stored vectors.  ``gram`` is ``evolve_geometry``'s, bit for bit: one sweep serves the quantum and the
    classical Fisher information.  Fixed order: two calls on the same inputs return bit-identical matrices.  Same arguments, flags and
    refusals as ``evolve_geometry``; tangents of inputs the problem does not have give zero rows and columns (``cgram[..., 0, 0]``
    stays ``<psi|psi>``).  More than 8 directions run one sweep per pair of groups of 4 (``geometry.geometry_sweeps``)."""
    return _evolve_gram(True, amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0, flags,
                        xy_pairs, d_xy)


def _evolve_gram(fisher: bool, amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0, flags,
                 xy_pairs=None, d_xy=None):
    """``evolve_geometry`` (``cgram`` None) and ``evolve_fisher``: the refusals, the sweeps over groups of directions, the assembly."""
    from .geometry import geometry_sweeps, place_sweep_block

    name, native = ("evolve_fisher", "rydiff_forward_fisher") if fisher else ("evolve_geometry", "rydiff_forward_geometry")
    if spec.rdms is not None and not (int(flags) & _native.TANGENT_RDMS):
        raise NotImplementedError(f"{name} evaluates no reduced density matrices ({native}: RYDIFF_ENOTIMPL) unless "
                                  "flags has _native.TANGENT_RDMS; or request them from evolve")
    if spec.dm is not None:
        raise NotImplementedError(f"{name} takes no density-matrix registers ({native}: RYDIFF_ENOTIMPL): the "
                                  "pure-state quantum Fisher information is not the mixed-state one")
    if spec.moments and not (int(flags) & _native.TANGENT_MOMENTS):
        raise NotImplementedError(f"{name} evaluates no occupation correlations ({native}: RYDIFF_ENOTIMPL) unless "
                                  "flags has _native.TANGENT_MOMENTS; or request them from evolve")
    if spec.shots is not None:
        raise NotImplementedError(f"{name} draws no measurement shots ({native}: RYDIFF_ENOTIMPL); request them from evolve")
    if spec.xy_mode and xy_pairs is None:
        raise NotImplementedError(f"{name} takes no XY exchange term ({native}: RYDIFF_ENOTIMPL with xy_mode != 0); "
                                  "run the dense pair-term route with _native.TANGENT_PAIR_TERMS")
    L = _native.lib()
    dev = psi0.device
    if xy_pairs is not None:
        flags = int(flags) | _native.TANGENT_XY
    n_dir, pre, rows = _sweep_prepare(name, amp_tables, det_tables, u_pairs, tsave, psi0, spec, obs_diag,
                                      d_amp, d_det, d_u, d_psi0, xy_pairs, d_xy)
    p, n_t, batch = pre.call.problem, pre.n_t, pre.batch
    expect = torch.empty((rows, n_t, batch), dtype=torch.float64, device=dev)
    dexpect = torch.empty((n_dir, rows, n_t, batch), dtype=torch.float64, device=dev)
    gram = torch.empty((n_t, batch, 1 + n_dir, 1 + n_dir), dtype=torch.complex128, device=dev)
    cgram = torch.empty((n_t, batch, 1 + n_dir, 1 + n_dir), dtype=torch.float64, device=dev) if fisher else None
    # tangents of inputs this problem does not have are zero: where nothing else is given the tangent states are identically zero,
    # and ONE sweep with a single zero direction delivers <psi|psi> and the values; every other entry is an exact zero
    live = ((d_amp is not None and pre.amp.numel() > 0) or (d_det is not None and pre.det.numel() > 0)
            or (d_u is not None and pre.u.numel() > 0) or d_psi0 is not None
            or (d_xy is not None and pre.xy is not None and pre.xy.numel() > 0))
    sweeps = geometry_sweeps(n_dir) if live else [[0]]
    size_fn = L.rydiff_fisher_workspace_bytes_flags if fisher else L.rydiff_geometry_workspace_bytes_flags
    size_name = "rydiff_fisher_workspace_bytes_flags" if fisher else "rydiff_geometry_workspace_bytes"
    with torch.cuda.device(dev):
        stream, info, _scratch = _sweep_plan(L, p, dev)
        workspace = None
        done = torch.zeros(n_dir, dtype=torch.bool)
        for s, idx in enumerate(sweeps):
            if live:
                bufs = _tangent_buffers(idx, pre, d_amp, d_det, d_u, d_psi0, dev, d_xy)
            else:
                bufs = (None, None, None, torch.zeros((1,) + tuple(pre.psi.shape), dtype=torch.complex128, device=dev), None)
            tg = _sweep_tangent(len(idx), bufs, flags)
            g = torch.empty((n_t, batch, 1 + len(idx), 1 + len(idx)), dtype=torch.complex128, device=dev)
            c = torch.empty((n_t, batch, 1 + len(idx), 1 + len(idx)), dtype=torch.float64, device=dev) if fisher else None
            want_rows = rows > 0 and not bool(done[idx].all())  # a later sweep of directions whose row tangents are all there skips them
            out = torch.empty((len(idx), rows, n_t, batch), dtype=torch.float64, device=dev) if want_rows else None

            def sweep(ws):
                head = (ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), _ptr(pre.psi),
                        _ptr(expect) if (rows > 0 and s == 0) else None, _ptr(out), _ptr(g))
                tail = (_ptr(ws), 0 if ws is None else ws.numel(), stream)
                return L.rydiff_forward_fisher(*head, _ptr(c), *tail) if fisher else L.rydiff_forward_geometry(*head, *tail)

            workspace = _sweep_workspace(size_fn, size_name, sweep, p, info, tg, workspace, dev)
            _native.check(sweep(workspace))
            if not live:
                gram.zero_()
                gram[:, :, 0, 0] = g[:, :, 0, 0]
                if fisher:
                    cgram.zero_()
                    cgram[:, :, 0, 0] = c[:, :, 0, 0]
                dexpect.zero_()
                break
            place_sweep_block(gram, idx, g)
            if fisher:
                place_sweep_block(cgram, idx, c)
            if out is not None:
                dexpect[idx] = out
            done[idx] = True
    return expect, dexpect, gram, cgram
