"""``TorchEmulator``: same constructor, properties and ``run`` signature as ``pulser_diff/backend.py:35-711``, with the
solver seam (``backend.py:488-494``) served by the MI355X-native library instead of ``pyqtorch.sesolve``.

What changes for a user switching over:
  * tensors handed to / returned by the solver live on the GPU (``compute_device``, default ``"cuda"``); leaf
    parameters may stay on the CPU — the (tiny) coefficient tables are moved, gradients flow back through the move;
  * ``run(..., observables=[DiagonalObservable(...)], store_states=False)`` evaluates diagonal observables natively
    and keeps the trajectory inside the solver workspace — the only way to run a 20-qubit sequence, where a dense
    observable (2^40 entries) or an autograd tape through every sub-step cannot exist;
  * stochastic noise (``SimConfig(noise=("doppler", "amplitude", "SPAM"))``) runs all realisations as ONE batch of
    trajectories and returns ``NoisyResults``; collapse-operator noise (dephasing, relaxation, depolarizing, eff_noise) and
    ``SolverType.DP5_ME`` run the master equation on a doubled register (``lindblad.py``) and return density matrices;
  * the digital basis, the XY mode (up to 8 qubits; its exchange exactly as the reference assembles it, see
    ``hamiltonian.Hamiltonian.XY_HERMITIAN``) and SLM masks run on the same kernels; the three-level "all" basis (a ground-rydberg
    and a digital channel in one sequence) runs as two qubits per atom with conditioned flips (noiseless runs);
  * a training loop keeps ONE emulator and calls ``refresh_from_sequence`` per epoch (``model.QuantumModel`` does).
"""
from __future__ import annotations

import functools
from bisect import bisect_left
from collections import Counter
from dataclasses import dataclass, replace
from typing import Any, Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import _native, pulser_adapter, pulses, utils
from .hamiltonian import COLLAPSE_NOISES, Hamiltonian
from .lindblad import (MAX_ME_QUBITS, ME_DEFAULT_TOL, dissipator_block, doubled_pair_terms, doubled_tables, local_collapse_operators,
                       mesolve, mesolve_tangent)
from .result import SampledResult
from .simconfig import SimConfig
from .simresults import CoherentResults, NoisyResults, SimulationResults
from .solver import (ProblemSpec, SolverType, evolve, evolve_fisher, evolve_geometry, evolve_tangent, sesolve, split_moments,
                     split_observables, tolerance_from_options)
from .observables import Energy, OccupationCorrelations, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap, pack_overlaps
from .geometry import (MeasurementFisher, QuantumGeometry, classical_fisher_information, quantum_fisher_information,
                       quantum_geometric_tensor)
from .shots import MAX_SHOTS, ShotRequest, indices_to_bitstrings
from .utils import DiagonalObservable, real_diagonal


def _same_field(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return bool(torch.equal(torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)))


@dataclass
class Sensitivities:
    """What ``TorchEmulator.run_sensitivities`` returns: ``values`` (n_obs, n_t), per tensor ``x_i`` of the request ``grads[i]`` of
    shape (n_obs, n_t, *x_i.shape) = d values / d x_i at every evaluation time (float64), the route that produced them —
    "tangent" (one native forward-mode sweep) or "adjoint-loop" (one reverse sweep per evaluation time) — and the times."""

    values: Tensor
    grads: list
    route: str
    times: Tensor


@dataclass
class SubsystemSensitivities:
    """What ``TorchEmulator.run_rdm_sensitivities`` returns: per subsystem ``o`` the reduced density matrix ``rho[o]`` complex
    (n_t, B, 2^m, 2^m) at every evaluation time (B: the columns of the initial state) and, per tensor ``x_i`` of the request,
    ``drho[o][i]`` complex (n_t, B, 2^m, 2^m, *x_i.shape) = d rho[o] / d x_i, on the device of ``x_i`` like the ``grads`` of
    ``Sensitivities``; and the times.  The scalar functionals below are
    formed from them in torch (``utils.purity_tangent``, ``utils.von_neumann_entropy_tangent``)."""

    rho: list
    drho: list
    times: Tensor

    def _along(self, o: int, tangent) -> list:
        out = []
        for dr in self.drho[o]:
            lead, shape = tuple(dr.shape[:2]), tuple(dr.shape[4:])
            flat = dr.reshape(dr.shape[:4] + (-1,)).permute(4, 0, 1, 2, 3)  # (numel, n_t, B, d, d)
            out.append(tangent(self.rho[o].to(flat.device), flat).permute(1, 2, 0).reshape(lead + shape))  # (drho sits with x_i)
        return out

    def purity(self, o: int) -> Tensor:
        """``tr rho[o]^2``, (n_t, B)."""
        return utils.purity(self.rho[o])

    def d_purity(self, o: int) -> list:
        """Per tensor ``x_i``: d purity(o) / d x_i, (n_t, B, *x_i.shape)."""
        return self._along(o, utils.purity_tangent)

    def entropy(self, o: int, base: float = 2) -> Tensor:
        """The von Neumann entropy of ``rho[o]``, (n_t, B)."""
        return utils.von_neumann_entropy(self.rho[o], base)

    def d_entropy(self, o: int, base: float = 2) -> list:
        """Per tensor ``x_i``: d entropy(o) / d x_i, (n_t, B, *x_i.shape); defined where ``rho[o]`` has full rank only
        (``utils.von_neumann_entropy_tangent``)."""
        return self._along(o, lambda rho, drho: utils.von_neumann_entropy_tangent(rho, drho, base))


@dataclass
class OccupationSensitivities:
    """What ``TorchEmulator.run_occupation_sensitivities`` returns: the moments ``S, B_q, B_qr`` of ``|psi|^2`` over the index bits
    (``RydProblem.bit_moments``) at every evaluation time, ``moments`` (1 + N + N(N-1)/2, n_t, B) (B: the columns of the initial
    state), per tensor ``x_i`` of the request ``dmoments[i]`` (rows, n_t, B, *x_i.shape) = d moments / d x_i on the device of
    ``x_i``, the times, and ``occupied_bit``: the index value of the level ``sample_state`` reports as "1" (r = 0 in the
    ground-rydberg basis, 1 in the digital and XY bases).  The accessors below convert them in torch (``utils``): values
    ``(n_t, B, ...)``, derivatives one ``(n_t, B, ..., *x_i.shape)`` per ``x_i``.  Nothing is normalised (``S`` enters as it is)."""

    moments: Tensor
    dmoments: list
    times: Tensor
    occupied_bit: int

    @property
    def n_qubits(self) -> int:
        rows = int(self.moments.shape[0])
        return next(n for n in range(1, _native.MAX_QUBITS + 1) if 1 + n + n * (n - 1) // 2 == rows)

    def _along(self, tangent, tail: int) -> list:
        """``tangent(rows (rows, P, n_t, B)) -> (P, n_t, B, <tail axes>)`` per ``x_i`` -> ``(n_t, B, <tail axes>, *x_i.shape)``."""
        out = []
        for dm in self.dmoments:
            shape = tuple(dm.shape[3:])
            flat = dm.reshape(tuple(dm.shape[:3]) + (-1,)).movedim(-1, 1)  # (rows, P, n_t, B)
            res = tangent(flat).movedim(0, -1)
            out.append(res.reshape(tuple(res.shape[:2 + tail]) + shape))
        return out

    def occupations(self) -> Tensor:
        """``<n_i>``, (n_t, B, N)."""
        return utils.occupations_from_moments(self.moments, self.n_qubits, self.occupied_bit)

    def d_occupations(self) -> list:
        """Per tensor ``x_i``: d<n_j> / d x_i, (n_t, B, N, *x_i.shape)."""
        return self._along(lambda dm: utils.occupations_from_moments(dm, self.n_qubits, self.occupied_bit), 1)

    def correlations(self, connected: bool = False) -> Tensor:
        """``<n_i n_j>`` (diagonal ``<n_i>``), (n_t, B, N, N); ``connected=True``: ``g_ij = <n_i n_j> - <n_i><n_j>``."""
        fn = utils.connected_correlations if connected else utils.occupation_correlations_from_moments
        return fn(self.moments, self.n_qubits, self.occupied_bit)

    def d_correlations(self, connected: bool = False) -> list:
        """Per tensor ``x_i``: d<n_j n_k> / d x_i (``connected=True``: d g_jk / d x_i, the product rule), (n_t, B, N, N, *x_i.shape)."""
        if connected:
            return self._along(lambda dm: utils.connected_correlations_tangent(self.moments.to(dm.device), dm, self.n_qubits,
                                                                              self.occupied_bit), 2)
        return self._along(lambda dm: utils.occupation_correlations_from_moments(dm, self.n_qubits, self.occupied_bit), 2)

    def structure_factor(self, signs) -> Tensor:
        """``sum_ij s_i s_j g_ij / N`` for a pattern ``signs`` of +-1 over the atoms (the Neel pattern: the antiferromagnetic
        order parameter), (n_t, B)."""
        return utils.structure_factor(self.correlations(connected=True), signs)

    def d_structure_factor(self, signs) -> list:
        """Per tensor ``x_i``: d structure_factor / d x_i, (n_t, B, *x_i.shape)."""
        return self._along(lambda dm: utils.structure_factor_tangent(self.moments.to(dm.device), dm, self.n_qubits, signs,
                                                                     self.occupied_bit), 0)


def _keeps_xy_route(method):
    """XY mode: a call that needs the dense pair terms (``Hamiltonian.require_dense_xy``) borrows them for its own duration.  When
    the outermost such call returns or raises, the Hamiltonian is back on the route ``Hamiltonian.xy_route()`` names, so a later
    ``run()`` on the native exchange term still delivers the gradient of the geometry."""

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        self._xy_route_depth = getattr(self, "_xy_route_depth", 0) + 1
        try:
            return method(self, *args, **kwargs)
        finally:
            self._xy_route_depth -= 1
            ham = self._hamiltonian
            if self._xy_route_depth == 0 and ham._interaction == "XY" and (ham.xy_mode != 0) != (ham.xy_route() == "native"):
                ham._select_xy_route()

    return wrapper


class TorchEmulator:
    r"""Emulator of a pulse sequence using the MI355X-native solver.

    Args:
        sampled_seq: A pulse sequence samples used in the emulation.
        register: The register associating coordinates to the qubits targeted by the pulses within the samples.
        device: The device specifications used in the emulation.
        sampling_rate: The fraction of samples that we wish to extract from the samples to simulate.
        config: Configuration to be used for this simulation.
        evaluation_times: "Full", "Minimal", an array of times in us, or a float fraction (``backend.py:47-58``).
        compute_device: torch device of the native solver (extension; default "cuda").
        xy_hermitian: XY mode only (extension): True = the physical exchange U (s+s- + s-s+); None / False = the exchange as the
            reference assembles it (one-directional, non-Hermitian generator; a warning is issued once).
        xy_native: XY mode only (extension): True = the exchange runs as the library's native exchange term (any register size,
            gradients of the geometry); False = as dense pair terms (at most 8 atoms); None = automatic: native past 8 atoms or when
            the coordinates or distances carry a gradient.  Only True also puts the all-times entry points (``run_sensitivities``,
            ``run_rdm_sensitivities``, ``run_occupation_sensitivities``, ``run_quantum_fisher``, ``run_classical_fisher``) on the
            native term: the tangent sweep with the exchange stencil, any register size, ``dist_grad=True`` and coordinates as
            directions.  With None / False they borrow the dense pair terms as before (8 atoms, no ``dist_grad``, no Fisher routes).
    """

    def __init__(self, sampled_seq, register, device, sampling_rate: float = 1.0, config: Optional[SimConfig] = None,
                 evaluation_times: Union[float, str, Any] = "Full", compute_device: Union[str, torch.device] = "cuda",
                 xy_hermitian: Optional[bool] = None, xy_native: Optional[bool] = None) -> None:
        # real Pulser objects are converted by attribute access (pulser_adapter.py); anything else is a TypeError
        sampled_seq = pulser_adapter.adapt_samples(sampled_seq)
        register = pulser_adapter.adapt_register(register)
        device = pulser_adapter.adapt_device(device)
        ids = set(register.qubit_ids)
        local_targets = {ch: set().union(*(slot.targets for slot in cs.slots))
                         for ch, cs in sampled_seq.channel_samples.items() if sampled_seq._ch_objs[ch].addressing == "Local"}
        # what must hold between samples, register and device (backend.py:72-101), each with the reference's message
        if sampled_seq.max_duration == 0:
            raise ValueError("SequenceSamples is empty.")
        device.validate_register(register)
        for broken, message in (
            (sampled_seq._slm_mask.end > 0 and not device.supports_slm_mask, "Samples use SLM mask but device does not have one."),
            (not sampled_seq.used_bases <= set(device.supported_bases), "Bases used in samples should be supported by device."),
            (not sampled_seq._slm_mask.targets <= ids, "The ids of qubits targeted in SLM mask should be defined in register."),
            (any(not t <= ids for t in local_targets.values()), "The ids of qubits targeted in Local channels should be defined in register."),
            (not (0 < sampling_rate <= 1.0), f"The sampling rate (`sampling_rate` = {sampling_rate}) must be greater than 0 and "
                                              "less than or equal to 1."),
            (int(sampled_seq.max_duration * sampling_rate) < 4, "`sampling_rate` is too small, less than 4 data points."),
        ):
            if broken:
                raise ValueError(message)
        self._register = register
        # a global channel drives the atoms of THIS register, whatever targets its slots were sampled with (backend.py:102-112);
        # the Hamiltonian reads one sample beyond the last instruction (backend.py:113-115)
        everyone = frozenset(register.qubit_ids)
        samples_list = [cs if ch in local_targets else replace(cs, slots=[replace(slot, targets=everyone) for slot in cs.slots])
                        for ch, cs in sampled_seq.channel_samples.items()]
        self._tot_duration = sampled_seq.max_duration
        self.samples_obj = replace(sampled_seq, samples_list=samples_list).extend_duration(self._tot_duration + 1)
        self._compute_device = torch.device(compute_device)
        self._noisy_state_budget = 8 * 2**30  # bytes of saved states per batch of noise realisations
        noise_model = config.to_noise_model() if config else SimConfig().to_noise_model()
        self._config = config if config else SimConfig()
        self._hamiltonian = Hamiltonian(self.samples_obj, self._register.qubits, device, sampling_rate, noise_model,
                                        compute_device=self._compute_device, xy_hermitian=xy_hermitian,
                                        xy_native=xy_native)
        self._eval_times_array: Tensor
        self.set_evaluation_times(evaluation_times)
        # backend.py:141-147: the sequence's measurement basis, else the Hamiltonian's ("digital" for the three-level basis)
        self._meas_basis = self.samples_obj._measurement or ("digital" if self._hamiltonian.basis_name == "all" else self._hamiltonian.basis_name)
        self.set_initial_state("all-ground")
        self.dist_dict: dict[str, Tensor] = {}

    # ---- properties (backend.py:153-181) ----------------------------------------------------------------
    @property
    def sampling_times(self) -> Tensor:
        return self._hamiltonian.sampling_times

    @property
    def _sampling_rate(self) -> float:
        return self._hamiltonian._sampling_rate

    @property
    def dim(self) -> int:
        return self._hamiltonian.dim

    @property
    def basis_name(self) -> str:
        return self._hamiltonian.basis_name

    @property
    def basis(self) -> dict:
        return self._hamiltonian.basis

    @property
    def config(self) -> SimConfig:
        return self._config

    def _require_simconfig(self, cfg, what: str, sep: str) -> None:
        """A SimConfig whose noise types the interaction mode knows (backend.py:185-196, :202-213)."""
        if not isinstance(cfg, SimConfig):
            raise ValueError(what)
        mode = self._hamiltonian._interaction
        foreign = set(cfg.noise) - cfg.supported_noises[mode]
        if foreign:
            raise NotImplementedError(f"Interaction mode '{mode}' does not support simulation of noise types:{sep}{', '.join(foreign)}.")

    def set_config(self, cfg: SimConfig) -> None:
        """Replace the noise configuration (backend.py:183-198)."""
        self._require_simconfig(cfg, f"Object {cfg} is not a valid `SimConfig`.", "")
        self._hamiltonian.set_config(cfg.to_noise_model())
        self._config = cfg

    def add_config(self, config: SimConfig) -> None:
        """backend.py:200-238: merge another configuration; noise types that are new bring their parameters along,
        noise types present in both keep the former parameters."""
        self._require_simconfig(config, f"Object {config} is not a valid `SimConfig`", " ")
        params_of = {"SPAM": ("eta", "epsilon", "epsilon_prime"), "doppler": ("temperature",),
                     "amplitude": ("laser_waist", "amp_sigma"), "relaxation": ("relaxation_rate",),
                     "dephasing": ("dephasing_rate", "hyperfine_dephasing_rate"), "depolarizing": ("depolarizing_rate",),
                     "eff_noise": ("eff_noise_rates", "eff_noise_opers")}
        old = self._config
        added = [n for n in config.noise if n not in old.noise]
        changes: dict = {"noise": tuple(old.noise) + tuple(added), "temperature": old.temperature * 1e6}  # stored in K
        for n in added:
            for name in params_of.get(n, ()):
                changes[name] = getattr(config, name) * 1e6 if name == "temperature" else getattr(config, name)
        self.set_config(replace(old, **changes))

    def show_config(self, solver_options: bool = False) -> None:
        print(self.config.__str__(solver_options))

    def reset_config(self) -> None:
        self.set_config(SimConfig())

    @property
    def initial_state(self) -> Tensor:
        return self._initial_state

    def set_initial_state(self, state: Union[str, Tensor]) -> None:
        """backend.py:253-280: "all-ground" or a (dim[, B]) tensor."""
        n = self._hamiltonian._size
        if isinstance(state, str) and state == "all-ground":
            # kron of N |g> kets: |g> is basis state 1 of the ground-rydberg basis (r, g) -> last vector; it is basis state 0
            # of the digital basis (g, h), like |u> of the XY basis (u, d) (backend.py:266-271) -> first vector
            dim = self._hamiltonian.dim
            psi = torch.zeros(dim**n, 1, dtype=torch.complex128)
            # position of |g> in the basis: 1 in (r, g) and in (r, g, h), 0 in (g, h); |u> of (u, d) is 0
            g = 0 if self._hamiltonian.basis_name in ("digital", "XY") else 1
            psi[sum(g * dim**k for k in range(n)), 0] = 1.0
            self._initial_state = psi
        else:
            shape = state.shape[0]
            legal_shape = self._hamiltonian.dim**n
            if shape != legal_shape:
                raise ValueError("Incompatible shape of initial state." + f"Expected {legal_shape}, got {shape}.")
            self._initial_state = state.to(torch.complex128)

    @property
    def evaluation_times(self) -> Tensor:
        return self._eval_times_array

    @property
    def qq_distances(self) -> dict:
        return self.dist_dict

    @property
    def endtimes(self) -> list:
        """backend.py:291-310."""
        end_ts = [0]
        remaining_indices = torch.linspace(0, self._tot_duration, int(self._sampling_rate * (self._tot_duration + 1)),
                                           dtype=torch.int)
        for samples in self.samples_obj.samples_list:
            end_ts += [bisect_left(remaining_indices.numpy(), sl.tf) - 1 for sl in samples.slots]
            end_ts += [bisect_left(remaining_indices.numpy(), sl.tf) for sl in samples.slots]
        return sorted(end_ts)

    def _requested_times(self, value) -> Tensor:
        """The times a caller asks for, before the two end points are added (backend.py:335-362): a label, a fraction of the
        sampling times, or explicit times in us."""
        st = self._hamiltonian.sampling_times
        wrong_label = "Wrong evaluation time label. It should be `Full`, `Minimal`, an array of times or a float between 0 and 1."
        if isinstance(value, str):
            if value not in ("Full", "Minimal"):
                raise ValueError(wrong_label)
            return torch.clone(st) if value == "Full" else torch.tensor([], dtype=st.dtype)
        if isinstance(value, float):
            if not 0 < value <= 1:
                raise ValueError("evaluation_times float must be between 0 and 1.")
            keep = torch.linspace(0, len(st) - 1, int(value * len(st)), dtype=torch.int)
            return st[keep.long()]
        if isinstance(value, (list, tuple, Tensor)):
            times = torch.as_tensor(value)
            if torch.max(times) > self._tot_duration / 1000:
                raise ValueError("Provided evaluation-time list extends further than sequence duration.")
            if torch.min(times) < 0:
                raise ValueError("Provided evaluation-time list contains negative values.")
            return times if times.is_floating_point() else times.to(torch.float64)  # (the union is taken in the caller's dtype)
        raise ValueError(wrong_label)

    def set_evaluation_times(self, value) -> None:
        """Times at which the results are returned (backend.py:312-375): what was asked for plus t = 0 and the end of the
        sequence, sorted, without duplicates."""
        asked = self._requested_times(value).detach().cpu()
        ends = torch.tensor([0.0, self._tot_duration / 1000], dtype=asked.dtype)
        self._eval_times_array = torch.cat([asked, ends]).unique().to(torch.float64).requires_grad_(False)
        self._eval_times_instruction = value

    def build_operator(self, operations) -> Tensor:
        return self._hamiltonian.build_operator(operations)

    def build_observable(self, operations) -> PauliObservable:
        """``build_operator`` as a sum of Pauli strings (no 2^N x 2^N tensor: any register size), for ``run(observables=[...])``,
        ``results.expect`` and ``QuantumModel.expectation``."""
        return self._hamiltonian.build_observable(operations)

    def build_reduced_density_matrix(self, atom_ids) -> ReducedDensityMatrix:
        """The ``ReducedDensityMatrix`` of the atoms ``atom_ids`` (register ids, in the order the matrix index should have), for
        ``run(observables=[...])`` and ``results.reduced_density_matrix`` / ``results.entanglement_entropy``."""
        index = self._hamiltonian._qid_index
        ids = list(atom_ids)
        missing = [q for q in ids if q not in index]
        if missing:
            raise ValueError(f"atom id(s) {missing} are not in the register ({list(index)})")
        return ReducedDensityMatrix([index[q] for q in ids])

    def get_hamiltonian(self, time: float) -> Tensor:
        """backend.py:401-427 (explicit matrix; small registers)."""
        if time > self._tot_duration:
            raise ValueError(
                f"Provided time (`time` = {time}) must be "
                "less than or equal to the sequence duration "
                f"({self._tot_duration})."
            )
        if time < 0:
            raise ValueError(f"Provided time (`time` = {time}) must be " "greater than or equal to 0.")
        return self._hamiltonian._hamiltonian(time / 1000)

    def _enable_dist_grad(self) -> None:
        """backend.py:456-460: the distances r_ij become differentiable inputs (``qq_distances``)."""
        for k, v in self._hamiltonian._dist_dict.items():
            if v.requires_grad:
                v.retain_grad()
            else:
                v.requires_grad_(True)  # constant register: make r_ij a leaf and reconnect U_ij to it
            self.dist_dict[k] = v
        self._hamiltonian._rebuild_u_pairs()
        if self._hamiltonian._interaction == "XY":
            # J_ij = C3 (1 - 3 cos^2 theta_ij) / r_ij^3 from the leaves, the angular factor a constant of the register; the couplings
            # now carry a gradient, which the native exchange term delivers (Hamiltonian.xy_route)
            self._hamiltonian._xy_dist_grad = True
            self._hamiltonian._rebuild_xy_pairs()

    def _xy_native_sweep(self) -> bool:
        """XY mode with ``xy_native=True``: the all-times entry points run the tangent sweep on the native exchange term (any
        register size, couplings with tangents of their own).  None / False: they borrow the dense pair terms as they always have."""
        ham = self._hamiltonian
        return ham._interaction == "XY" and ham._xy_native is True

    def _xy_sweep_inputs(self, spec, *d_xy) -> dict:
        """The exchange's keyword arguments of the solver's entry points on the native route (nothing off it): the couplings and,
        for the sweeps, which hand in `d_xy`, their tangents."""
        if not spec.xy_mode:
            return {}
        return dict(xy_pairs=self._hamiltonian.xy_pairs, **({"d_xy": d_xy[0]} if d_xy else {}))

    def _dense_xy_for(self, what: str, dist_grad: bool, native_ok: bool = False) -> None:
        """XY mode: `what` runs on the dense pair terms (constants, at most 8 atoms), not on the native exchange term — unless the
        emulator was built with ``xy_native=True`` and `what` has a native sweep (`native_ok`)."""
        if self._hamiltonian._interaction != "XY":
            return
        if native_ok and self._xy_native_sweep():
            return
        if dist_grad:
            raise NotImplementedError(f"dist_grad is not available in the XY mode for {what}: it runs on the dense pair terms, whose "
                                      "exchange blocks are constants (run(dist_grad=True) differentiates the native exchange term).")
        self._hamiltonian.require_dense_xy(what)

    # ---- run (backend.py:430-611) -------------------------------------------------------------------------
    @_keeps_xy_route
    def run(self, time_grad: bool = False, dist_grad: bool = False, solver: SolverType = SolverType.DP5_SE,
            observables: Optional[list] = None, store_states: bool = True, shots: Union[None, int, ShotRequest] = None,
            native_shots: bool = False, **options: Any) -> SimulationResults:
        """Simulates the sequence with the native solver and returns ``CoherentResults``.

        ``observables`` (extension): diagonal observables (``DiagonalObservable`` or dense diagonal tensors) and sums of Pauli
        strings (``PauliObservable``, e.g. from ``build_observable``) and overlaps with target states (``StateOverlap``; read with
        ``results.overlap``) and states of subsystems (``ReducedDensityMatrix``, e.g. from ``build_reduced_density_matrix``; read
        with ``results.reduced_density_matrix`` / ``results.entanglement_entropy`` / ``results.negativity``; master-equation runs
        serve them — ``Tr_E rho`` — with ``store_states=False``) and the occupation correlations (``OccupationCorrelations``; read
        with ``results.occupations`` / ``occupation_correlations`` / ``structure_factor``; master-equation runs serve them — the
        moments of the diagonal of rho — with ``store_states=False``) and the energy under the sequence's own Hamiltonian (``Energy``; read
        with ``results.energy`` / ``energy_second_moment`` / ``energy_variance``; ket runs only) to be evaluated natively at every evaluation time; ``store_states=False`` keeps the trajectory out of the results.

        ``shots`` (extension): measurement shots drawn natively while the state is on the device — an int (that many at the final
        evaluation time) or a ``ShotRequest`` (``times="all"``: every evaluation time).  ``results.sample_state`` /
        ``sample_final_state`` return them when asked for a sampled time and exactly that many samples, also with
        ``store_states=False``.  Coherent runs: Schroedinger, and master-equation runs without stored states (drawn from the
        diagonal of rho; with stored states ``sample_state`` draws from the stored density matrices and ``shots=`` is refused).  ``native_shots=True`` (extension, noisy runs that average over
        realisations): the per-run measurements are drawn natively as well and no run's states are stored.
        """
        if shots is not None and not isinstance(shots, ShotRequest):
            if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)):
                raise TypeError(f"shots must be an int or a ShotRequest, got {type(shots)}")
            shots = ShotRequest(int(shots))
        if time_grad:
            self._eval_times_array.requires_grad_(True)  # backend.py:453-455
        if dist_grad:
            # XY mode: the master equation and the averaged noisy runs stay on the dense pair terms, whose blocks are constants
            if solver == SolverType.DP5_ME or set(self.config.noise) & COLLAPSE_NOISES:
                self._dense_xy_for("the master-equation solver (DP5_ME)", True)
            if not (self._no_resampling() and ("SPAM" not in self.config.noise or self.config.eta == 0)):
                self._dense_xy_for("noisy runs that average over realisations", True)
            self._enable_dist_grad()
        if set(self.config.noise) & COLLAPSE_NOISES:  # backend.py:482-488: collapse operators force the master equation
            solver = SolverType.DP5_ME
        if solver not in (SolverType.DP5_SE, SolverType.KRYLOV_SE, SolverType.DP5_ME):
            raise ValueError(f"Solver {solver} not available.")
        if solver == SolverType.DP5_ME:
            self._hamiltonian.require_dense_xy("the master-equation solver (DP5_ME)")
        if solver == SolverType.DP5_ME and self._hamiltonian.basis_name == "all":
            raise NotImplementedError("The master-equation solver is not available in the three-level all-basis "
                                      "(the reference admits no collapse-operator noise there, hamiltonian.py:98-103).")

        dev = self._compute_device
        ham = self._hamiltonian
        obs_tensors, obs_objs, pauli_objs, overlap_objs, rdm_objs, purity_objs = [], [], [], [], [], []
        moments = False
        energy = 0
        for obs in observables or []:
            if isinstance(obs, Energy):
                if ham.basis_name == "all":
                    raise NotImplementedError("Energy is not available in the three-level all-basis (the native energy rows do not "
                                              "take conditioned terms); apply get_hamiltonian to the stored states instead.")
                if solver == SolverType.DP5_ME:
                    raise NotImplementedError("Energy is not available in master-equation runs (Tr(rho H) is not evaluated natively "
                                              "yet); apply get_hamiltonian to the stored density matrices instead.")
                if ham._interaction == "XY" and (ham.xy_mode != 1 or ham.pair_terms):
                    raise NotImplementedError("Energy in the XY mode runs on the native, Hermitian exchange term only: "
                                              "TorchEmulator(..., xy_native=True, xy_hermitian=True).")
                energy = max(energy, obs.rows)
                continue
            if isinstance(obs, OccupationCorrelations):
                if ham.basis_name == "all":
                    raise NotImplementedError("OccupationCorrelations is not available in the three-level all-basis (an atom is "
                                              "two qubits there); reduce the stored states instead.")
                moments = True
                continue
            if isinstance(obs, Purity):
                if solver != SolverType.DP5_ME:
                    raise NotImplementedError("Purity is evaluated natively in master-equation runs only (a ket has purity "
                                              "<psi|psi>^2: results.purity() computes it from the stored states).")
                purity_objs.append(obs)
                continue
            if isinstance(obs, ReducedDensityMatrix):
                if ham.basis_name == "all":
                    raise NotImplementedError("ReducedDensityMatrix is not available in the three-level all-basis; trace the "
                                              "stored states instead.")
                obs.check(ham._size)
                rdm_objs.append(obs)
                continue
            if isinstance(obs, StateOverlap):
                if tuple(obs.shape) != (ham.dim ** ham._size,) * 2:
                    raise ValueError(f"StateOverlap targets of dimension {obs.shape[0]} handed to states of dimension {ham.dim ** ham._size}")
                overlap_objs.append(obs)
                continue
            if isinstance(obs, PauliObservable):
                if ham.basis_name == "all":
                    raise NotImplementedError("Pauli observables are not available in the three-level all-basis; use "
                                              "results.expect on stored states.")
                if obs.n_qubits != ham._size:
                    raise ValueError(f"PauliObservable on {obs.n_qubits} qubits handed to a register of {ham._size}")
                pauli_objs.append(obs)
                continue
            if not isinstance(obs, DiagonalObservable) and not (isinstance(obs, Tensor) and obs.ndim == 2):
                raise TypeError("observables must be DiagonalObservable / PauliObservable / StateOverlap / ReducedDensityMatrix / Purity / "
                                "OccupationCorrelations / Energy objects or diagonal (dim, dim) tensors")
            diag = real_diagonal(obs, "Only diagonal observables can be evaluated natively; use results.expect on the states.")
            obs_tensors.append(diag.to(dev, torch.float64))
            obs_objs.append(obs)
        obs_diag = torch.stack(obs_tensors) if obs_tensors else None

        psi0 = self.initial_state
        if psi0.ndim == 1:
            psi0 = psi0.unsqueeze(1)

        # measurement errors of the SPAM model (backend.py:462-480)
        noise = set(self.config.noise)
        meas_errors = None
        if "SPAM" in noise:
            meas_errors = {k: self.config.spam_dict[k] for k in ("epsilon", "epsilon_prime")}
            ground = torch.zeros_like(self.initial_state)
            ground[-1 if self._hamiltonian.basis_name == "ground-rydberg" else 0] = 1.0  # |g..g>: last vector of (r, g), first of (g, h)
            if self.config.eta > 0 and not torch.equal(self.initial_state, ground):
                raise NotImplementedError("Can't combine state preparation errors with an initial "
                                          "state different from the ground.")

        def run_coherent() -> CoherentResults:
            if rdm_objs and solver == SolverType.DP5_ME and store_states:
                raise NotImplementedError("ReducedDensityMatrix observables of master-equation runs are evaluated natively (the partial "
                                          "trace Tr_E rho) with store_states=False only; with stored states "
                                          "results.reduced_density_matrix(obs) computes it from the density matrices without the "
                                          "observable being handed to run().")
            # A master-equation run that stores its density matrices already serves fidelities (results.fidelity) and samples
            # (sample_state) from them: the two requests that used to be refused there stay refused with stored states, and are
            # served natively where no trajectory is kept
            if overlap_objs and solver == SolverType.DP5_ME and store_states:
                raise NotImplementedError("StateOverlap observables of master-equation runs are evaluated natively (the fidelity "
                                          "<phi|rho|phi>) with store_states=False only; with stored states results.fidelity(obs) "
                                          "computes it from the density matrices without the observable being handed to run().")
            if moments and solver == SolverType.DP5_ME and store_states:
                raise NotImplementedError("OccupationCorrelations of master-equation runs is evaluated natively (the moments of the "
                                          "diagonal of rho) with store_states=False only; with stored states results.occupations() / "
                                          "occupation_correlations() / structure_factor() compute them from the density matrices "
                                          "without the observable being handed to run().")
            if shots is not None and solver == SolverType.DP5_ME and store_states:
                raise NotImplementedError("Native measurement shots of master-equation runs are drawn (from the diagonal of rho) with "
                                          "store_states=False only; with stored states sample_state draws from the stored density "
                                          "matrices.")
            if solver == SolverType.DP5_ME:  # density matrices (backend.py:495-509); without collapse noise L = 0
                # diagonal tables, Pauli strings (unrotated: this path runs in no rotating frame), fidelities, the purity, reduced
                # density matrices, the occupation correlations and the shots are taken from rho while it is on the device; store_states=False keeps the (n_t, 4^N) trajectory out
                res = mesolve(ham, psi0.to(dev), self._eval_times_array, ham.config, options,
                              observables=obs_objs + pauli_objs + overlap_objs + purity_objs + rdm_objs
                              + ([OccupationCorrelations()] if moments else []), shots=shots, store_states=store_states)
                n_ex, n_ov = len(obs_objs) + len(pauli_objs), len(overlap_objs)
                return CoherentResults(res.states, ham._size, ham.basis_name, self._eval_times_array, self._meas_basis, meas_errors,
                                       atom_order=tuple(ham._qdict), stats=res.stats, density=True,
                                       native_expect=torch.stack(res.expect[:n_ex]) if n_ex else None,
                                       native_observables=obs_objs + pauli_objs, overlap_observables=overlap_objs,
                                       native_fidelities=res.expect[n_ex:n_ex + n_ov] if n_ov else None,
                                       native_purity=res.expect[n_ex + n_ov] if purity_objs else None, native_shots=res.shots,
                                       native_rdms=res.rdms if rdm_objs else None, rdm_observables=rdm_objs,
                                       native_moments=res.moments)
            result = sesolve(ham, psi0.to(dev), self._eval_times_array, solver=solver, options=options, obs_diag=obs_diag,
                             store_states=store_states, pauli_obs=pauli_objs, overlap_obs=overlap_objs, shots=shots, rdm_obs=rdm_objs,
                             moments=moments, energy=energy)
            states_tbd = result.states.permute(0, 2, 1) if result.states.numel() else result.states
            return CoherentResults(states_tbd, ham._size, ham.basis_name, self._eval_times_array, self._meas_basis,
                                   meas_errors, atom_order=tuple(ham._qdict),
                                   native_expect=result.expect if (obs_diag is not None or pauli_objs) else None,
                                   native_observables=obs_objs + pauli_objs, stats=result.stats,
                                   native_overlaps=result.overlaps, overlap_observables=overlap_objs, native_shots=result.shots,
                                   native_rdms=result.rdms, rdm_observables=rdm_objs, native_moments=result.moments,
                                   native_energy=result.energy, hamiltonian_at=ham._hamiltonian)

        # does the noise ask for averaging over several runs?  (backend.py:531-569)
        bad_atom_configs = None
        if self._no_resampling():
            if "SPAM" not in noise or self.config.eta == 0:
                return run_coherent()
            # only the state preparation is random: one run per distinct configuration of badly prepared atoms
            n_atoms = len(ham._qid_index)
            drawn = Counter("".join(str(int(b)) for b in (torch.rand(size=(n_atoms,)) < self.config.eta).tolist())
                            for _ in range(self.config.runs)).most_common()
            bad_atom_configs = [tuple(c == "1" for c in cfg) for cfg, _ in drawn]
            reps = [r for _, r in drawn]
        else:
            reps = [1] * self.config.runs
        if overlap_objs:
            raise NotImplementedError("StateOverlap observables stay refused in noisy runs that average over realisations.")
        if rdm_objs:
            raise NotImplementedError("ReducedDensityMatrix observables stay refused in noisy runs that average over realisations.")
        if purity_objs:
            raise NotImplementedError("Purity observables stay refused in noisy runs that average over realisations.")
        if moments:
            raise NotImplementedError("OccupationCorrelations stays refused in noisy runs that average over realisations.")
        if energy:
            raise NotImplementedError("Energy stays refused in noisy runs that average over realisations.")
        if shots is not None:
            raise NotImplementedError("A ShotRequest belongs to one coherent run; noisy runs that average over realisations return "
                                      "their measurements as NoisyResults (native_shots=True draws them natively).")
        ham.require_dense_xy("noisy runs that average over realisations")
        return self._run_noisy(psi0, solver, options, reps, bad_atom_configs, meas_errors, native_shots=native_shots)

    # ---- sensitivities at every evaluation time (extension) ---------------------------------------------------
    def _table_tangents(self, x: list, with_xy: bool = False) -> tuple:
        """d(amp_tables, det_tables, u_pairs) / d(every scalar entry of every tensor in x) — with ``with_xy`` a fourth entry, the
        tangent of the couplings ``Hamiltonian.xy_pairs`` of the native XY exchange (None off that route) —, direction-major, through the host-side
        torch graph tables(x) by the double-backward trick: the VJP g(w) = J^T w with a dummy cotangent w under create_graph=True is
        linear in w, so the gradient of its entry j w.r.t. w is column j of J — the table tangent of that scalar.  Outputs that do
        not require grad are skipped (None: zero tangent); the complex table goes through view_as_real."""
        ham = self._hamiltonian
        outs = {"amp": torch.view_as_real(ham.amp_tables) if ham.amp_tables.numel() else ham.amp_tables.real,
                "det": ham.det_tables, "u": ham.u_pairs}
        if with_xy and getattr(ham, "xy_mode", 0):
            outs["xy"] = ham.xy_pairs  # (on the compute device like the tables, where the sweep reads its tangent)
        live = {k: v for k, v in outs.items() if v.requires_grad and v.numel()}
        n_dir = sum(int(t.numel()) for t in x)
        tangents = {k: None for k in outs}
        pick = lambda: (tangents["amp"], tangents["det"], tangents["u"]) + ((tangents.get("xy"),) if with_xy else ())  # noqa: E731
        if not live or n_dir == 0:
            return pick()
        dummies = {k: torch.zeros_like(v, requires_grad=True) for k, v in live.items()}
        vjp = torch.autograd.grad(list(live.values()), x, grad_outputs=list(dummies.values()), create_graph=True, allow_unused=True)
        cols = {k: [] for k in live}
        for g, t in zip(vjp, x):
            flat = None if g is None or not g.requires_grad else g.reshape(-1)
            for j in range(int(t.numel())):
                col = (None,) * len(live) if flat is None else torch.autograd.grad(flat[j], list(dummies.values()), retain_graph=True,
                                                                                    allow_unused=True)
                for k, c in zip(live, col):
                    cols[k].append(torch.zeros_like(live[k]) if c is None else c.detach())
        for k in live:
            stacked = torch.stack(cols[k])
            tangents[k] = torch.view_as_complex(stacked.contiguous()) if k == "amp" else stacked
        return pick()

    def _no_resampling(self) -> bool:
        """The noise asks for no averaging over several runs of resampled tables (backend.py:531-569; a random state preparation,
        SPAM with eta > 0, still does)."""
        noise = set(self.config.noise)
        return noise <= {"dephasing", "relaxation", "SPAM", "depolarizing", "eff_noise", "amplitude"} and (
            "amplitude" not in noise or self.config.amp_sigma == 0.0)

    def _check_sensitivity_request(self, name: str, x: list, solver: SolverType, averaging: str = "",
                                   master_equation: Optional[str] = None, all_basis: Optional[str] = None) -> tuple:
        """What the all-times methods (`name`) ask of a request before they look at the observables -> (x as a list, the solver that
        will run).  ``averaging``: the method's reason behind the refusal of averaging noise; ``master_equation`` / ``all_basis``: the
        method's refusal of master-equation runs / of the three-level basis (None: it takes them)."""
        x = list(x)
        if not x or not all(isinstance(t, Tensor) for t in x):
            raise TypeError("x must be a non-empty list of tensors")
        if any(t is self._eval_times_array for t in x):
            raise ValueError(f"{name} differentiates w.r.t. parameters; the evaluation times are not one of them: "
                             "run(time_grad=True) and deriv_time deliver d f(t_k) / d t_k for every k in one reverse sweep.")
        noise = set(self.config.noise)
        if not self._no_resampling() or ("SPAM" in noise and self.config.eta > 0):
            raise NotImplementedError(f"{name} is not available in noisy runs that average over realisations{averaging}.")
        if noise & COLLAPSE_NOISES:
            solver = SolverType.DP5_ME
        if solver == SolverType.DP5_ME and master_equation is not None:
            raise NotImplementedError(master_equation)
        if solver not in (SolverType.DP5_SE, SolverType.KRYLOV_SE, SolverType.DP5_ME):
            raise ValueError(f"Solver {solver} not available.")
        if self._hamiltonian.basis_name == "all" and all_basis is not None:
            raise NotImplementedError(all_basis)
        return x, solver

    def _pack_row_observables(self, observables: list, overlaps: bool = False) -> tuple:
        """Diagonal observables, ``PauliObservable`` and (``overlaps``) ``StateOverlap`` objects -> (obs_diag or None, the Pauli
        objects, the overlap objects, rows): ``rows`` lists the native rows of the observables in the order they were handed in —
        diagonal rows, then the Pauli rows, then two rows (Re, Im) per overlap, the order ``solver._Call.expect_rows`` counts."""
        ham, dev = self._hamiltonian, self._compute_device
        diag_rows, pauli_objs, overlap_objs, order = [], [], [], []  # order: where observable i sits among the native rows
        for obs in observables:
            if isinstance(obs, PauliObservable):
                if obs.n_qubits != ham._size:
                    raise ValueError(f"PauliObservable on {obs.n_qubits} qubits handed to a register of {ham._size}")
                order.append(("p", len(pauli_objs)))
                pauli_objs.append(obs)
                continue
            if overlaps and isinstance(obs, StateOverlap):
                order.append(("o", len(overlap_objs)))
                overlap_objs.append(obs)
                continue
            diag = real_diagonal(obs, "Only diagonal observables can be evaluated natively; build off-diagonal ones with build_observable.")
            order.append(("d", len(diag_rows)))
            diag_rows.append(diag.to(dev, torch.float64))
        n_real = len(diag_rows) + len(pauli_objs)
        rows = []
        for kind, r in order:
            rows += [r] if kind == "d" else ([len(diag_rows) + r] if kind == "p" else [n_real + 2 * r, n_real + 2 * r + 1])
        return torch.stack(diag_rows) if diag_rows else None, pauli_objs, overlap_objs, rows

    @staticmethod
    def _plain_run_with_zero_tangents(n_dir: int, run) -> tuple:
        """Nothing in x reaches the tables: (expect, dexpect) with the values of the plain run ``run()`` (under no_grad) and zero
        derivatives in every direction."""
        with torch.no_grad():
            expect = run()
        return expect, torch.zeros((n_dir,) + tuple(expect.shape), dtype=torch.float64, device=expect.device)

    @staticmethod
    def _per_tensor(dvals: Tensor, x: list) -> list:
        """Direction-major derivatives (n_dir, ...), one direction per scalar entry of the tensors in x -> one tensor per x_i on
        x_i's device, of shape (..., *x_i.shape)."""
        dvals = dvals.movedim(0, -1)
        out, d0 = [], 0
        for t in x:
            m = int(t.numel())
            out.append(dvals[..., d0:d0 + m].reshape(tuple(dvals.shape[:-1]) + tuple(t.shape)).to(t.device))
            d0 += m
        return out

    @_keeps_xy_route
    def run_sensitivities(self, x: list, observables: list, solver: SolverType = SolverType.DP5_SE, dist_grad: bool = False,
                          route: Optional[str] = None, **options: Any) -> "Sensitivities":
        """Values AND derivatives of observables at EVERY evaluation time w.r.t. the tensors in ``x`` — what a loop of
        ``deriv_param(f, x, times, t)`` over all ``t`` delivers, in one forward-mode sweep (``rydiff_forward_tangent``): the state
        and one tangent state per scalar entry of ``x`` advance together, ~(1 + D) forward passes instead of n_t reverse sweeps.

        ``x`` takes what ``deriv_param`` takes: leaf parameters of the pulses, register coordinates and — with ``dist_grad=True``,
        which has the side effects it has in ``run`` — distances from ``qq_distances``.  ``observables``: diagonal observables
        (``DiagonalObservable`` or diagonal dense tensors) and ``PauliObservable`` objects; master-equation runs (collapse-operator
        noise, ``DP5_ME``) additionally take ``StateOverlap`` (the fidelity ``<phi|rho|phi>``) and ``Purity``.

        ``route``: ``None`` — noiseless Ising runs take the tangent sweep; master-equation runs, the XY exchange and the three-level
        basis run the loop of one-hot reverse sweeps, as they always have.  ``"tangent"`` asks for the sweep: master-equation runs
        (``lindblad.mesolve_tangent``: vec(rho) and its tangents on the doubled register, the dissipator and the exchange as constant
        pair terms) and XY runs take it too; the three-level basis, which the sweep does not take, raises.  ``"adjoint-loop"`` forces
        the loop anywhere (the A/B partner of the sweep).  An XY emulator built with ``xy_native=True`` takes the sweep on the native
        exchange term by default (``RYDIFF_TANGENT_XY``: coordinates and distances reach the couplings' tangents ``d_xy``), and its
        ``"adjoint-loop"`` loops over native reverse sweeps.  ``Sensitivities.route`` says which ran.  Derivatives w.r.t. the evaluation
        times come from ``deriv_time``."""
        if route not in (None, "tangent", "adjoint-loop"):
            raise ValueError(f'route must be None, "tangent" or "adjoint-loop", got {route!r}')
        x, solver = self._check_sensitivity_request("run_sensitivities", x, solver)
        ham, dev = self._hamiltonian, self._compute_device
        observables = list(observables)
        full = ham.dim ** ham._size
        for obs in observables:
            if isinstance(obs, OccupationCorrelations):
                raise NotImplementedError("run_sensitivities does not take OccupationCorrelations (its rows are one scalar per "
                                          "observable); run_occupation_sensitivities returns every <n_i>, <n_i n_j> and their "
                                          "derivatives at every evaluation time from the same tangent sweep.")
            if isinstance(obs, ReducedDensityMatrix):
                if solver != SolverType.DP5_ME:
                    raise NotImplementedError("run_sensitivities does not take ReducedDensityMatrix observables (its rows are real "
                                              "scalars); run_rdm_sensitivities returns the matrices and their derivatives at every "
                                              "evaluation time from the same tangent sweep.")
                raise NotImplementedError("run_sensitivities does not take ReducedDensityMatrix observables (the tangent sweep "
                                          "evaluates none); differentiate results.reduced_density_matrix through run().")
            if isinstance(obs, Purity) and solver == SolverType.DP5_ME:
                continue
            kinds = (DiagonalObservable, PauliObservable) + ((StateOverlap,) if solver == SolverType.DP5_ME else ())
            if not isinstance(obs, kinds) and not (isinstance(obs, Tensor) and obs.ndim == 2):
                raise TypeError("observables must be DiagonalObservable / PauliObservable objects or diagonal (dim, dim) tensors "
                                "(master-equation runs: StateOverlap and Purity too)")
            if tuple(obs.shape) != (full, full):
                raise ValueError(f"Incompatible shape of observable.Expected {(full, full)}, got {tuple(obs.shape)}.")
        self._dense_xy_for("run_sensitivities", dist_grad, native_ok=solver != SolverType.DP5_ME)
        if dist_grad:
            self._enable_dist_grad()
        times = self._eval_times_array.detach()
        n_t = int(times.shape[0])
        sweepable = ham.basis_name != "all"  # what the tangent sweep takes at all
        if route == "tangent" and not sweepable:
            raise NotImplementedError("run_sensitivities: the tangent sweep is not available in the three-level all-basis (no "
                                      "conditioned flips / ones-counting terms); route=None runs the adjoint loop there.")
        # route=None keeps the choice callers have relied on: master-equation and XY runs loop unless the sweep is asked for
        native = sweepable and route != "adjoint-loop" and (
            route == "tangent" or (solver != SolverType.DP5_ME and not getattr(ham, "pair_terms", ())))
        if not native:
            # the loop the tangent sweep replaces: one reverse sweep per evaluation time and observable
            results = self.run(dist_grad=False, solver=solver, **options)
            plain = [o for o in observables if not isinstance(o, Purity)]
            plain_fs = iter(results.expect(plain))
            fs = [results.purity().sum(dim=-1) if isinstance(o, Purity) else next(plain_fs).real for o in observables]
            grads = [torch.zeros((len(fs), n_t) + tuple(t.shape), dtype=torch.float64, device=t.device) for t in x]
            for o, f in enumerate(fs):
                for k in range(n_t):
                    cot = torch.zeros(n_t, dtype=f.dtype, device=f.device)
                    cot[k] = 1.0
                    for g_out, g in zip(grads, torch.autograd.grad(f, x, grad_outputs=cot, retain_graph=True, allow_unused=True)):
                        if g is not None:
                            g_out[o, k] = g.detach().to(torch.float64)
            return Sensitivities(torch.stack([f.detach() for f in fs]).to(torch.float64), grads, "adjoint-loop", times)

        n_dir = sum(int(t.numel()) for t in x)
        if solver == SolverType.DP5_ME:
            # vec(rho) and its tangents on the doubled register; the rows come back in the order of `observables`
            d_amp, d_det, d_u = self._table_tangents(x)
            psi0 = self.initial_state
            psi_db = (psi0.unsqueeze(1) if psi0.ndim == 1 else psi0).to(dev)
            if d_amp is None and d_det is None and d_u is None:  # nothing in x reaches the tables
                expect, dexpect = self._plain_run_with_zero_tangents(n_dir, lambda: torch.stack(
                    mesolve(ham, psi_db, times, ham.config, dict(options), observables=observables, store_states=False).expect))
            else:
                expect, dexpect = mesolve_tangent(ham, psi_db, times, ham.config, dict(options), observables,
                                                  d_amp=d_amp, d_det=d_det, d_u=d_u)
            return Sensitivities(expect.sum(dim=-1), self._per_tensor(dexpect.sum(dim=-1), x), "tangent", times)

        obs_diag, pauli_objs, _, rows = self._pack_row_observables(observables)
        d_amp, d_det, d_u, d_xy = self._table_tangents(x, with_xy=True)
        n_dir = sum(int(t.numel()) for t in x)
        psi0 = self.initial_state
        psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1).to(dev)
        spec = ham.problem_spec(solver=solver, tol=tolerance_from_options(dict(options)), store_states=False)
        if pauli_objs:
            spec.pauli = pauli_objs
        xy_in = self._xy_sweep_inputs(spec, d_xy)
        if d_amp is None and d_det is None and d_u is None and d_xy is None:  # nothing in x reaches the tables: zero derivatives, values from a plain run
            expect, dexpect = self._plain_run_with_zero_tangents(
                n_dir, lambda: evolve(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, obs_diag,
                                      **self._xy_sweep_inputs(spec))[1])
        else:
            # the complex tables and the unrotated psi0: the rotating frame is a per-call device of sesolve, not of this path
            expect, dexpect = evolve_tangent(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, obs_diag,
                                             d_amp=d_amp, d_det=d_det, d_u=d_u,
                                             flags=_native.TANGENT_PAIR_TERMS if spec.pair_terms else 0,  # (the dense XY exchange)
                                             **xy_in)
        values = expect.sum(dim=-1)[rows]            # (n_obs, n_t): summed over the columns of psi0 like results.expect
        dvals = dexpect.sum(dim=-1)[:, rows]         # (n_dir, n_obs, n_t)
        return Sensitivities(values, self._per_tensor(dvals, x), "tangent", times)

    @_keeps_xy_route
    def run_rdm_sensitivities(self, x: list, subsystems: list, solver: SolverType = SolverType.DP5_SE, dist_grad: bool = False,
                              **options: Any) -> "SubsystemSensitivities":
        """Reduced density matrices of up to 8 subsystems AND their derivatives w.r.t. the tensors in ``x`` at EVERY evaluation time,
        from one forward-mode sweep (``rydiff_forward_tangent`` with ``RYDIFF_TANGENT_RDMS``): at every save point the sweep holds the
        state and one tangent state per scalar entry of ``x``, and ``d rho_A = Tr_E(|dpsi><psi| + |psi><dpsi|)`` is formed natively
        beside ``rho_A``.  What the loop of one reverse sweep per evaluation time and per scalar functional of ``rho_A`` (purity,
        entropy, mutual information ...) through ``run(observables=[ReducedDensityMatrix(...)])`` delivers.

        ``x`` is what ``run_sensitivities`` takes.  ``subsystems``: ``ReducedDensityMatrix`` objects (e.g. from
        ``build_reduced_density_matrix``) or tuples of qubit indices, 1 to 6 qubits each.  Noiseless Ising and XY runs (the exchange
        rides in the sweep as constant pair terms).  Returns ``SubsystemSensitivities``."""
        x, solver = self._check_sensitivity_request(
            "run_rdm_sensitivities", x, solver,
            master_equation="run_rdm_sensitivities is not available for master-equation runs (collapse-operator noise, "
                            "DP5_ME): the tangent sweep forms no tangents of the partial trace of a density matrix; "
                            "differentiate results.reduced_density_matrix through run().",
            all_basis="run_rdm_sensitivities is not available in the three-level all-basis: the native tangent sweep "
                      "takes no conditioned flips / ones-counting terms, and ReducedDensityMatrix is a qubit observable.")
        ham, dev = self._hamiltonian, self._compute_device
        if any(isinstance(o, OccupationCorrelations) for o in subsystems):
            raise NotImplementedError("run_rdm_sensitivities does not take OccupationCorrelations (they are no subsystem); "
                                      "run_occupation_sensitivities returns them and their derivatives at every evaluation time.")
        rdm_objs = [o if isinstance(o, ReducedDensityMatrix) else ReducedDensityMatrix(o) for o in subsystems]
        if not 1 <= len(rdm_objs) <= _native.MAX_RDMS:
            raise ValueError(f"run_rdm_sensitivities takes 1 to {_native.MAX_RDMS} subsystems per call, got {len(rdm_objs)}")
        for obs in rdm_objs:
            obs.check(ham._size)
        self._dense_xy_for("run_rdm_sensitivities", dist_grad, native_ok=True)
        if dist_grad:
            self._enable_dist_grad()
        times = self._eval_times_array.detach()
        d_amp, d_det, d_u, d_xy = self._table_tangents(x, with_xy=True)
        n_dir = sum(int(t.numel()) for t in x)
        psi0 = self.initial_state
        psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1).to(dev)
        spec = ham.problem_spec(solver=solver, tol=tolerance_from_options(dict(options)), store_states=False)
        spec.rdms = rdm_objs
        xy_in = self._xy_sweep_inputs(spec, d_xy)
        if d_amp is None and d_det is None and d_u is None and d_xy is None:  # nothing in x reaches the tables: zero derivatives, values from a plain run
            expect, dexpect = self._plain_run_with_zero_tangents(
                n_dir, lambda: evolve(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, None,
                                      **self._xy_sweep_inputs(spec))[1])
        else:
            # the complex tables and the unrotated psi0, as in run_sensitivities: the matrices are lab-frame ones
            expect, dexpect = evolve_tangent(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, None,
                                             d_amp=d_amp, d_det=d_det, d_u=d_u,
                                             flags=_native.TANGENT_RDMS | (_native.TANGENT_PAIR_TERMS if spec.pair_terms else 0),
                                             **xy_in)
        rho = split_observables(expect, 0, rdm_objs)[2]
        per_dir = [split_observables(dexpect[d], 0, rdm_objs)[2] for d in range(n_dir)]
        # per subsystem: (n_dir, n_t, B, 2^m, 2^m) -> one (n_t, B, 2^m, 2^m, *x_i.shape) per x_i
        drho = [self._per_tensor(torch.stack([per_dir[d][o] for d in range(n_dir)]), x) for o in range(len(rdm_objs))]
        return SubsystemSensitivities(rho, drho, times)

    @_keeps_xy_route
    def run_occupation_sensitivities(self, x: list, solver: SolverType = SolverType.DP5_SE, dist_grad: bool = False,
                                     **options: Any) -> "OccupationSensitivities":
        """The occupation correlations — the moments behind every ``<n_i>`` and ``<n_i n_j>`` — AND their derivatives w.r.t. the
        tensors in ``x`` at EVERY evaluation time, from one forward-mode sweep (``rydiff_forward_tangent`` with
        ``RYDIFF_TANGENT_MOMENTS``): at every save point the sweep holds the state and one tangent state per scalar entry of ``x``,
        and the moments of ``2 Re(conj psi . dpsi)`` are formed natively beside those of ``|psi|^2``, one read of each vector.
        What the loop of one reverse sweep per evaluation time and per scalar functional (a structure factor, one ``g_ij``)
        through ``run(observables=[OccupationCorrelations()])`` delivers.

        ``x`` is what ``run_sensitivities`` takes.  Noiseless Ising and XY runs (the exchange rides in the sweep as constant pair
        terms).  Returns ``OccupationSensitivities``."""
        x, solver = self._check_sensitivity_request(
            "run_occupation_sensitivities", x, solver,
            averaging=": OccupationCorrelations stays refused there",
            master_equation="run_occupation_sensitivities is not available for master-equation runs (collapse-operator noise, "
                            "DP5_ME): occupation correlations are evaluated natively on kets only; hand run_sensitivities "
                            "DiagonalObservable projectors instead.",
            all_basis="run_occupation_sensitivities is not available in the three-level all-basis: an atom is two qubits "
                      "there, and the native tangent sweep takes no conditioned flips / ones-counting terms.")
        ham, dev = self._hamiltonian, self._compute_device
        self._dense_xy_for("run_occupation_sensitivities", dist_grad, native_ok=True)
        if dist_grad:
            self._enable_dist_grad()
        times = self._eval_times_array.detach()
        d_amp, d_det, d_u, d_xy = self._table_tangents(x, with_xy=True)
        n_dir = sum(int(t.numel()) for t in x)
        psi0 = self.initial_state
        psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1).to(dev)
        spec = ham.problem_spec(solver=solver, tol=tolerance_from_options(dict(options)), store_states=False)
        spec.moments = True
        xy_in = self._xy_sweep_inputs(spec, d_xy)
        if d_amp is None and d_det is None and d_u is None and d_xy is None:  # nothing in x reaches the tables: zero derivatives, values from a plain run
            expect, dexpect = self._plain_run_with_zero_tangents(
                n_dir, lambda: evolve(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, None,
                                      **self._xy_sweep_inputs(spec))[1])
        else:
            # the complex tables and the unrotated psi0, as in run_sensitivities (the moments are diagonal: they see no frame)
            expect, dexpect = evolve_tangent(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, None,
                                             d_amp=d_amp, d_det=d_det, d_u=d_u,
                                             flags=_native.TANGENT_MOMENTS | (_native.TANGENT_PAIR_TERMS if spec.pair_terms else 0),
                                             **xy_in)
        moments = split_moments(expect, ham._size)[1]
        dmom = torch.stack([split_moments(dexpect[d], ham._size)[1] for d in range(n_dir)])  # (n_dir, rows, n_t, B)
        return OccupationSensitivities(moments, self._per_tensor(dmom, x), times, 0 if ham.basis_name == "ground-rydberg" else 1)

    def run_quantum_fisher(self, x: list, observables: list = (), solver: SolverType = SolverType.DP5_SE, dist_grad: bool = False,
                           **options: Any) -> "QuantumGeometry":
        """The quantum Fisher information matrix of the state w.r.t. the scalar entries of the tensors in ``x`` at EVERY evaluation
        time, with the quantum geometric tensor, the Berry curvature and the Gram matrix they are formed from — one native
        forward-mode sweep that carries the state and one tangent state per scalar and reduces their inner products at every save
        point (``rydiff_forward_geometry``); no state is stored.  ``x`` is what ``run_sensitivities`` takes.  ``observables``
        (optional): diagonal observables, ``PauliObservable`` and ``StateOverlap`` objects, whose ``values`` / ``grads`` come out as
        in ``Sensitivities`` — a ``StateOverlap`` as two rows, Re and Im of ``c = <phi|psi>`` and of its derivatives, so that the
        Gauss-Newton term ``2 Re(conj(dc_i) dc_j)`` of a fidelity loss can be formed from the same call.  One initial state gives
        (n_t, D, D) matrices, several columns of it (n_t, B, D, D): the geometry of a batch is per state.  This is the PURE-state
        quantity: runs whose state is a density matrix or an average are refused, there is no fallback loop."""
        x, solver = self._check_sensitivity_request(
            "run_quantum_fisher", x, solver,
            averaging=": the average of pure states is a mixed state, and this is the pure-state quantum Fisher information",
            master_equation="run_quantum_fisher is not available for master-equation runs (collapse-operator noise, DP5_ME): "
                            "the state is a density matrix, and the pure-state quantum Fisher information is not the "
                            "mixed-state one.",
            all_basis="run_quantum_fisher is not available in the three-level all-basis: the native tangent sweep takes "
                      "no conditioned flips / ones-counting terms.")
        gram, _, values, grads, times = self._run_gram_sweep("run_quantum_fisher", False, x, observables, solver, dist_grad, options)
        qgt = quantum_geometric_tensor(gram)
        return QuantumGeometry(gram, qgt, 4.0 * qgt.real, -2.0 * qgt.imag, values, grads, "tangent", times)

    def run_classical_fisher(self, x: list, observables: list = (), solver: SolverType = SolverType.DP5_SE, dist_grad: bool = False,
                             **options: Any) -> "MeasurementFisher":
        """The classical Fisher information matrix of the device's one measurement — bitstrings in the occupation basis,
        ``p(y) = |psi[y]|^2`` — w.r.t. the scalar entries of the tensors in ``x`` at EVERY evaluation time, next to the quantum
        Fisher information of the same sweep: ``F_C <= F_Q`` as matrices, with equality where the native measurement saturates the
        quantum Cramer-Rao bound (``geometry.fisher_efficiency``).  One native forward-mode sweep as in ``run_quantum_fisher``,
        which at every save point also reduces the classical Gram matrix of the state and its tangents
        (``rydiff_forward_fisher``); no state is stored.  ``x`` and ``observables`` are what ``run_quantum_fisher`` takes.  One
        initial state gives (n_t, D, D) matrices, several columns of it (n_t, B, D, D).  Pure states only: runs whose state is a
        density matrix or an average are refused, there is no fallback loop.  Returns ``MeasurementFisher``."""
        x, solver = self._check_sensitivity_request(
            "run_classical_fisher", x, solver,
            averaging=": the bitstring distribution of an average of runs is that of a mixed state, and run_classical_fisher forms "
                      "the classical Fisher information of a pure state's distribution",
            master_equation="run_classical_fisher is not available for master-equation runs (collapse-operator noise, DP5_ME): "
                            "the state is a density matrix, and the classical Fisher information of diag rho is not formed "
                            "by the tangent sweep.",
            all_basis="run_classical_fisher is not available in the three-level all-basis: the native tangent sweep takes "
                      "no conditioned flips / ones-counting terms, and a bitstring there is not one index bit per atom.")
        gram, cgram, values, grads, times = self._run_gram_sweep("run_classical_fisher", True, x, observables, solver, dist_grad, options)
        return MeasurementFisher(cgram, classical_fisher_information(cgram), gram, quantum_fisher_information(gram), values, grads,
                                 "tangent", times)

    def _run_gram_sweep(self, name: str, fisher: bool, x: list, observables: list, solver: SolverType, dist_grad: bool, options: dict):
        """What ``run_quantum_fisher`` and ``run_classical_fisher`` (`name`) share behind their request checks: the observables, the
        table tangents, the sweep.  ``(gram, cgram or None, values, grads, times)``."""
        ham, dev = self._hamiltonian, self._compute_device
        sweep = evolve_fisher if fisher else (lambda *a, **k: evolve_geometry(*a, **k) + (None,))
        if (getattr(ham, "pair_terms", ()) or getattr(ham, "xy_mode", 0)) and not self._xy_native_sweep():
            if ham._size > ham.MAX_XY_QUBITS:
                raise NotImplementedError(ham.dense_xy_limit(name))
            raise NotImplementedError(f"{name} is not available with the XY exchange: this route hands no dense pair terms "
                                      "to the tangent sweep (solver.evolve_geometry takes them on request).")
        observables = list(observables)
        full = ham.dim ** ham._size
        for obs in observables:
            if isinstance(obs, OccupationCorrelations):
                raise NotImplementedError(f"{name} does not take OccupationCorrelations (its rows are one scalar per "
                                          "observable); run_occupation_sensitivities returns them and their derivatives at every "
                                          "evaluation time (solver.evolve_geometry takes them with _native.TANGENT_MOMENTS).")
            if not isinstance(obs, (DiagonalObservable, PauliObservable, StateOverlap)) and not (isinstance(obs, Tensor) and obs.ndim == 2):
                raise TypeError("observables must be DiagonalObservable / PauliObservable / StateOverlap objects or diagonal (dim, dim) tensors")
            if tuple(obs.shape) != (full, full):
                raise ValueError(f"Incompatible shape of observable.Expected {(full, full)}, got {tuple(obs.shape)}.")
        if dist_grad:
            self._enable_dist_grad()
        times = self._eval_times_array.detach()
        n_t = int(times.shape[0])
        obs_diag, pauli_objs, overlap_objs, rows = self._pack_row_observables(observables, overlaps=True)
        d_amp, d_det, d_u, d_xy = self._table_tangents(x, with_xy=True)
        n_dir = sum(int(t.numel()) for t in x)
        psi0 = self.initial_state
        psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1).to(dev)
        batch = int(psi_bd.shape[0])
        spec = ham.problem_spec(solver=solver, tol=tolerance_from_options(dict(options)), store_states=False)
        if pauli_objs:
            spec.pauli = pauli_objs
        if overlap_objs:  # the complex tables and the unrotated psi0 (as in run_sensitivities): the targets stay in the lab frame too
            spec.overlaps = pack_overlaps(overlap_objs, int(psi_bd.shape[1]), batch, dev)
        xy_in = self._xy_sweep_inputs(spec, d_xy)  # (the native exchange of an xy_native=True emulator: the couplings and their tangents)
        if d_amp is None and d_det is None and d_u is None and d_xy is None:
            # nothing in x reaches the tables: every tangent state is zero — <psi|psi> and the values from one sweep with one zero direction
            expect, _, g1, c1 = sweep(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, obs_diag,
                                      d_psi0=torch.zeros((1,) + tuple(psi_bd.shape), dtype=torch.complex128, device=dev), **xy_in)
            dexpect = torch.zeros((n_dir,) + tuple(expect.shape), dtype=torch.float64, device=expect.device)
            gram = torch.zeros((n_t, batch, 1 + n_dir, 1 + n_dir), dtype=torch.complex128, device=g1.device)
            gram[:, :, 0, 0] = g1[:, :, 0, 0]
            cgram = None
            if fisher:
                cgram = torch.zeros((n_t, batch, 1 + n_dir, 1 + n_dir), dtype=torch.float64, device=c1.device)
                cgram[:, :, 0, 0] = c1[:, :, 0, 0]
        else:
            expect, dexpect, gram, cgram = sweep(ham.amp_tables, ham.det_tables, ham.u_pairs, times, psi_bd, spec, obs_diag,
                                                 d_amp=d_amp, d_det=d_det, d_u=d_u, **xy_in)
        if batch == 1:
            gram = gram[:, 0]
            cgram = cgram[:, 0] if fisher else None
        values = expect.sum(dim=-1)[rows]            # (n_rows, n_t): summed over the columns of psi0 like results.expect
        dvals = dexpect.sum(dim=-1)[:, rows]         # (n_dir, n_rows, n_t)
        return gram, cgram, values, self._per_tensor(dvals, x), times

    def _run_noisy(self, psi0: Tensor, solver: SolverType, options: dict, reps: list, bad_atom_configs,
                   meas_errors, native_shots: bool = False) -> NoisyResults:
        """backend.py:571-611 with the stochastic runs as the BATCH axis of the native solver: every run is one more
        trajectory with its own coefficient tables, all advanced by the same launches; the per-run measurements
        (``samples_per_run`` x repetitions, then detection errors) are drawn on the GPU from |psi(t)|^2.  ``native_shots``
        (Schroedinger runs): the solver draws them itself at every evaluation time and stores no states, so the runs of one
        batch are bounded by its workspace instead of the saved trajectories."""
        ham, dev = self._hamiltonian, self._compute_device
        if psi0.shape[1] != 1:
            raise NotImplementedError("Noisy runs start from a single initial state.")
        loop_runs = len(reps)
        amp, det, amp_masks, det_masks = ham.noisy_batch_tables(loop_runs, bad_atom_configs)
        n, n_t = ham._size, int(self._eval_times_array.shape[0])
        dim = 2**n
        master = solver == SolverType.DP5_ME  # collapse operators on top: every realisation is a density matrix
        native_shots = bool(native_shots) and not master  # (density matrices keep the route through stored states)
        u_pairs = ham.u_pairs.detach()
        # the XY exchange lives in dense pair terms (they used to be dropped here, i.e. noisy XY runs evolved without
        # any interaction).  A badly prepared atom takes no part in it (hamiltonian.py:393-397 skips its pairs), so the pair terms
        # depend on the realisation: such runs go one configuration per solver call (the configurations are distinct and few).
        xy_terms = tuple(getattr(ham, "pair_terms", ()))
        per_run_pairs = bool(xy_terms) and bad_atom_configs is not None and any(any(cfg) for cfg in bad_atom_configs)

        def xy_terms_of(run: int) -> tuple:
            if not per_run_pairs:
                return xy_terms
            bad = bad_atom_configs[run]
            return tuple(t for t in xy_terms if not (bad[t[0]] or bad[t[1]]))

        if master:
            if n > MAX_ME_QUBITS:
                raise ValueError(f"The master-equation solver keeps 4^N amplitudes; limited to {MAX_ME_QUBITS} qubits.")
            amp, det, u_pairs, amp_masks, det_masks = doubled_tables(amp, det, u_pairs, amp_masks, det_masks, n)
            block = dissipator_block(local_collapse_operators(ham.config, ham.basis_name))

            def spec_of(run: int) -> ProblemSpec:
                return ProblemSpec(2 * n, ham.dt, ham.n_samples, amp_masks, det_masks, solver=SolverType.DP5_SE,
                                   tol=tolerance_from_options(options) or ME_DEFAULT_TOL, store_states=True,
                                   pair_terms=doubled_pair_terms(xy_terms_of(run), n, block))
            ket = psi0.to(dev)[:, 0]
            start = torch.outer(ket, ket.conj()).reshape(1, dim * dim)
        else:
            def spec_of(run: int) -> ProblemSpec:
                return ProblemSpec(n, ham.dt, ham.n_samples, amp_masks, det_masks, solver=solver,
                                   tol=tolerance_from_options(options), store_states=not native_shots, pair_terms=xy_terms_of(run))
            start = psi0.to(dev).T.contiguous()
        # bound the saved states of one batch (n_t x runs x 2^N, or 4^N, amplitudes)
        chunk = 1 if per_run_pairs else max(1, min(loop_runs, int(self._noisy_state_budget // max(n_t * start.shape[1] * 16, 1))))
        max_shots = self.config.samples_per_run * max(reps)
        if native_shots:
            if max_shots > MAX_SHOTS:
                raise ValueError(f"native_shots: samples_per_run x repetitions = {max_shots} exceeds {MAX_SHOTS} shots per run and time; "
                                 "use the default route")
            # no stored states: one trajectory costs its share of the workspace — a handful of state vectors, up to 12 qubits the
            # trajectory the one-launch sweep is sampled from — plus its uniforms and shots
            per_run = (8 + (n_t if n <= 12 else 0)) * dim * 16 + n_t * max_shots * 12
            chunk = 1 if per_run_pairs else max(1, min(loop_runs, 65535, int(self._noisy_state_budget // per_run)))
        eps = meas_errors["epsilon"] if meas_errors else 0.0
        eps_p = meas_errors["epsilon_prime"] if meas_errors else 0.0
        bit_weights = (1 << torch.arange(n, device=dev, dtype=torch.int64))
        total_count = [Counter() for _ in range(n_t)]
        # outcome histogram per evaluation time, accumulated ON the device over all runs (one bitstring conversion per distinct outcome
        # at the end instead of one per run, time and outcome: that loop was half of a 100-run call); huge registers keep the host path
        hist = torch.zeros(n_t * dim, dtype=torch.int64, device=dev) if n_t * dim <= (1 << 26) else None
        t_offset = (torch.arange(n_t, device=dev) * dim)[:, None]
        tsave = self._eval_times_array.detach()
        for r0 in range(0, loop_runs, chunk):
            r1 = min(loop_runs, r0 + chunk)
            with torch.no_grad():
                spec = spec_of(r0)
                if native_shots:
                    spec.shots = ShotRequest(max_shots, times="all")
                states, _ = evolve(amp[r0:r1], det[r0:r1], u_pairs, tsave, start.repeat(r1 - r0, 1), spec, None)
                if native_shots:
                    probs = None
                elif master:  # populations = diagonal of rho
                    probs = states.reshape(n_t, r1 - r0, dim, dim).diagonal(dim1=2, dim2=3).real.clamp_min(0.0)
                else:
                    probs = states.real**2 + states.imag**2  # (n_t, runs, dim), basis order r = 0, g = 1
                del states
                for b in range(r1 - r0):
                    n_shots = self.config.samples_per_run * reps[r0 + b]
                    # measured bitstring (result.py:70-120): ground-rydberg '1' = r = index bit 0, i.e. the complement of the index;
                    # digital / XY '1' = h / d = index bit 1: the index itself
                    if native_shots:  # (n_t, shots): the first n_shots of the run's native shots (shot s belongs to uniform s)
                        shots = indices_to_bitstrings(spec.shots.indices[:, b, :n_shots], ham.basis_name, self._meas_basis, n)
                    else:
                        idx = torch.multinomial(probs[:, b, :], n_shots, replacement=True)  # (n_t, shots)
                        shots = (dim - 1) - idx if ham.basis_name == "ground-rydberg" else idx
                    if eps > 0 or eps_p > 0:
                        bits = (shots.unsqueeze(-1) >> torch.arange(n, device=dev)) & 1
                        flip = torch.rand(bits.shape, device=dev) < torch.where(bits == 1, eps_p, eps)
                        shots = ((bits ^ flip.to(bits.dtype)) * bit_weights).sum(-1)
                    if hist is not None:
                        flat = (shots + t_offset).reshape(-1)
                        hist.scatter_add_(0, flat, torch.ones_like(flat))
                        continue
                    shots = shots.cpu().numpy()
                    for t in range(n_t):
                        vals, cnt = np.unique(shots[t], return_counts=True)
                        total_count[t].update({np.binary_repr(int(v), n): int(c) for v, c in zip(vals, cnt)})
                del probs
        if hist is not None:
            counts = hist.reshape(n_t, dim).cpu().numpy()
            for t in range(n_t):
                hit = np.flatnonzero(counts[t])
                total_count[t].update({format(int(v), f"0{n}b"): int(counts[t, v]) for v in hit})
        n_measures = self.config.runs * self.config.samples_per_run
        results = [SampledResult(tuple(ham._qdict), self._meas_basis, total_count[t]) for t in range(n_t)]
        return NoisyResults(results, ham._size, ham.basis_name, self._eval_times_array, n_measures)

    def refresh_from_sequence(self, sequence, with_modulation: bool = False) -> bool:
        """Persistent problem object for training loops: the reference builds a NEW emulator — and
        with it every sparse operator — on each epoch (``pulser_diff/model.py:405-414``).  Here a built sequence with the SAME
        structure as the one this emulator was made from (same channels, same total duration, same register ids) only
        re-samples the pulses and rebuilds the coefficient tables / pair interactions in place (torch ops, so the autograd
        history to the new parameter values is kept); evaluation times, initial state, configuration and the basis objects
        stay.  Returns False — and changes nothing — when the structure differs; the caller then builds a new emulator."""
        native = isinstance(sequence, pulses.Sequence)
        sampler = pulses.sample if native else pulser_adapter.sample_pulser_sequence
        if sequence.is_parametrized() or sequence.is_register_mappable():
            raise ValueError("The provided sequence needs to be built to be simulated.")
        sampled = pulser_adapter.adapt_samples(sampler(sequence, modulation=with_modulation,
                                                       extended_duration=sequence.get_duration(include_fall_time=with_modulation)))
        register = pulser_adapter.adapt_register(sequence.register)
        old = self.samples_obj
        if (sampled.max_duration != self._tot_duration or tuple(register.qubit_ids) != tuple(self._register.qubit_ids)
                or list(sampled.channels) != list(old.channels) or sampled.used_bases != old.used_bases
                or sampled._slm_mask != old._slm_mask
                or sampled._measurement != old._measurement
                or not _same_field(sampled._magnetic_field, old._magnetic_field)
                or any(sampled._ch_objs[c] != old._ch_objs[c] for c in sampled.channels)):
            return False
        # what the constructor checks about targets and the register holds for a refreshed sequence as well
        self._hamiltonian._device.validate_register(register)
        ids = set(register.qubit_ids)
        for ch, ch_samples in sampled.channel_samples.items():
            if sampled._ch_objs[ch].addressing == "Local" and not set().union(*(slot.targets for slot in ch_samples.slots)) <= ids:
                raise ValueError("The ids of qubits targeted in Local channels should be defined in register.")
        samples_list = []
        for ch, ch_samples in sampled.channel_samples.items():
            if sampled._ch_objs[ch].addressing == "Local":
                samples_list.append(ch_samples)
            else:  # backend.py:102-112
                samples_list.append(replace(ch_samples, slots=[replace(slot, targets=frozenset(register.qubit_ids))
                                                               for slot in ch_samples.slots]))
        self._register = register
        self.samples_obj = replace(sampled, samples_list=samples_list).extend_duration(self._tot_duration + 1)
        ham = self._hamiltonian
        ham.samples_obj = self.samples_obj
        ham._qdict = {k: (v if isinstance(v, Tensor) else torch.as_tensor(v)).to(torch.float64) for k, v in register.qubits.items()}
        ham._dist_dict = {}
        ham._xy_dist_grad = False  # the new distances are functions of the coordinates again, and so is the angular factor
        ham._construct_hamiltonian()
        self.dist_dict = {}
        # a fresh leaf for the evaluation times: with time_grad the old one has requires_grad set and would ACCUMULATE its
        # gradient from epoch to epoch (the reference makes a new emulator, hence a new tensor, per epoch: model.py:405-414)
        self._eval_times_array = self._eval_times_array.detach().clone()
        return True

    @classmethod
    def from_sequence(cls, sequence, sampling_rate: float = 1.0, config: Optional[SimConfig] = None,
                      evaluation_times: Union[float, str, Any] = "Full", with_modulation: bool = False,
                      compute_device: Union[str, torch.device] = "cuda", xy_hermitian: Optional[bool] = None,
                      xy_native: Optional[bool] = None) -> "TorchEmulator":
        r"""backend.py:651-711."""
        native = isinstance(sequence, pulses.Sequence)
        if not native and not all(hasattr(sequence, a) for a in ("is_parametrized", "is_register_mappable", "_schedule",
                                                                   "declared_channels", "get_duration", "register", "device")):
            raise TypeError("The provided sequence has to be a valid pulser.Sequence instance.")
        if sequence.is_parametrized() or sequence.is_register_mappable():
            raise ValueError(
                "The provided sequence needs to be built to be simulated. Call"
                " `Sequence.build()` with the necessary parameters."
            )
        if not sequence._schedule:
            raise ValueError("The provided sequence has no declared channels.")
        if all(sequence.get_duration(ch) == 0 for ch in sequence.declared_channels):
            raise ValueError("No instructions given for the channels in the sequence.")
        if with_modulation and sequence._slm_mask_targets:
            raise NotImplementedError(
                "Simulation of sequences combining an SLM mask and output " "modulation is not supported."
            )
        sampler = pulses.sample if native else pulser_adapter.sample_pulser_sequence  # the latter needs Pulser installed
        return cls(
            sampler(sequence, modulation=with_modulation,
                    extended_duration=sequence.get_duration(include_fall_time=with_modulation)),
            sequence.register, sequence.device, sampling_rate, config, evaluation_times, compute_device=compute_device,
            xy_hermitian=xy_hermitian, xy_native=xy_native)
