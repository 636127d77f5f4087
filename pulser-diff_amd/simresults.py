"""Results containers with the reference's semantics (``pulser_diff/simresults.py``): ``.states`` is a tensor of
shape (n_t, dim, B) (``simresults.py:398-401``), ``.expect(obs_list)`` returns one (n_t,) tensor per observable
(``simresults.py:81-129``), indexing / iteration yields per-time ``TorchResult`` objects.

States live on the GPU as ONE (n_t, B, dim) buffer written by the native solver; ``.states`` is its permuted view
and the per-time results are views into it (the reference stacks a Python list of per-time tensors).
Diagonal observables that were handed to ``TorchEmulator.run(observables=...)`` are evaluated by the native
``k_expect_diag`` kernel and returned from ``expect`` without touching the states.
"""
from __future__ import annotations

import collections.abc
from abc import ABC, abstractmethod
from collections import Counter
from typing import Callable, Mapping, Optional

import numpy as np
import torch
from torch import Tensor

from .result import SampledResult, TorchResult
from .observables import (PauliObservable, ReducedDensityMatrix, StateOverlap, dm_occupation_moments, fidelity_states,
                          occupation_moments, overlap_states, purity_states, reduced_density_matrix)
from .shots import ShotRequest, bitstring_counts, indices_to_bitstrings
from .utils import (DiagonalObservable, connected_correlations, energy_variance, expect, negativity, occupation_correlations_from_moments,
                    occupations_from_moments, structure_factor, von_neumann_entropy)


class SimulationResults(ABC):
    """Results of a simulation run of a pulse sequence (parent of CoherentResults)."""

    _use_pseudo_dens: bool = False

    def __init__(self, size: int, basis_name: str, sim_times: Tensor) -> None:
        self._dim = 3 if basis_name == "all" else 2
        self._size = size
        if basis_name not in {"ground-rydberg", "digital", "all", "XY"}:
            raise ValueError("`basis_name` must be 'ground-rydberg', 'digital', 'all' or 'XY'.")
        self._basis_name = basis_name
        self._sim_times = sim_times

    @property
    @abstractmethod
    def states(self) -> Tensor:
        ...

    def _get_index_from_time(self, t_float: float, tol: float = 1.0e-3) -> int:
        """simresults.py:167-181."""
        try:
            return int(torch.where(abs(t_float - self._sim_times.detach().cpu()) < tol)[0][0])
        except IndexError:
            raise IndexError(f"Given time {t_float} is absent from Simulation times within" + f" tolerance {tol}.")


class CoherentResults(SimulationResults, collections.abc.Sequence):
    """Results of a coherent simulation run (``simresults.py:347-396``)."""

    def __init__(self, states_tbd: Tensor, size: int, basis_name: str, sim_times: Tensor, meas_basis: str,
                 meas_errors: Optional[Mapping[str, float]] = None, atom_order: tuple = (),
                 native_expect: Optional[Tensor] = None, native_observables: Optional[list] = None,
                 stats: Optional[dict] = None, density: bool = False, native_overlaps: Optional[Tensor] = None,
                 overlap_observables: Optional[list] = None, native_shots: Optional[ShotRequest] = None,
                 native_rdms: Optional[list] = None, rdm_observables: Optional[list] = None,
                 native_fidelities: Optional[list] = None, native_purity: Optional[Tensor] = None,
                 native_moments: Optional[Tensor] = None, native_energy: Optional[Tensor] = None,
                 hamiltonian_at: Optional[Callable] = None) -> None:
        super().__init__(size, basis_name, sim_times)
        if self._basis_name == "all":  # simresults.py:381-383
            if meas_basis not in {"ground-rydberg", "digital"}:
                raise ValueError("`meas_basis` must be 'ground-rydberg' or 'digital'.")
        elif meas_basis != self._basis_name:
            raise ValueError("`meas_basis` and `basis_name` must have the same value.")
        if meas_errors is not None and not {"epsilon", "epsilon_prime"} <= set(meas_errors.keys()):
            raise ValueError("Measurement error probabilities must be given in the form `{'epsilon':0.01, 'epsilon_prime':0.05}`")
        self._meas_basis = meas_basis
        self._meas_errors = meas_errors
        self._density = density  # master-equation run: `states_tbd` holds density matrices (n_t, dim, dim, B) instead
        self._states_tbd = states_tbd  # (n_t, B, dim), possibly empty when states were not stored
        self._atom_order = atom_order
        self._native_expect = native_expect  # (n_obs, n_t, B)
        self._native_observables = list(native_observables or [])
        self._native_overlaps = native_overlaps  # complex (n_ov, n_t, B)
        self._overlap_observables = list(overlap_observables or [])
        self._native_rdms = native_rdms  # per observable: complex (n_t, B, 2^m, 2^m)
        self._rdm_observables = list(rdm_observables or [])
        self._native_fidelities = native_fidelities  # master-equation runs, per StateOverlap: real (n_t, B) = <phi|rho|phi>
        self._native_purity = native_purity  # master-equation runs with a Purity observable: real (n_t, B)
        self._native_moments = native_moments  # run with OccupationCorrelations: real (1 + N + N(N-1)/2, n_t, B): S, B_q, B_qr
        self._native_energy = native_energy  # run with Energy: real (1 | 2, n_t, B): E, then the second moment
        self._hamiltonian_at = hamiltonian_at  # t (us) -> explicit H(t): energies of stored states where no native rows were asked for
        self._native_shots = native_shots  # filled by the solver: amplitude indices (n_shot_times, B, n_shots)
        self.solver_stats = dict(stats or {})

    # ---- sequence protocol over per-time results (pulser.result.Results)
    def __len__(self) -> int:
        return int(self._sim_times.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if self._states_tbd.numel() == 0:
            raise RuntimeError("States were not stored for this run (store_states=False).")
        if self._density:
            return TorchResult(self._atom_order, self._meas_basis, self._states_tbd[i], True)  # (dim, dim, B)
        return TorchResult(self._atom_order, self._meas_basis, self._states_tbd[i].transpose(0, 1), True)

    @property
    def states(self) -> Tensor:
        """(n_t, dim, B) like ``torch.stack([res.state for res in self])`` (``simresults.py:398-401``)."""
        if self._states_tbd.numel() == 0:
            raise RuntimeError("States were not stored for this run (store_states=False).")
        if self._density:
            return self._states_tbd  # (n_t, dim, dim, B): what mesolve's states stack to (backend.py:513-521)
        return self._states_tbd.permute(0, 2, 1)

    def get_state(self, t: float, reduce_to_basis=None, ignore_global_phase: bool = True, tol: float = 1e-6,
                  normalize: bool = True, t_tol: float = 1.0e-3) -> Tensor:
        return self[self._get_index_from_time(t, t_tol)].get_state(reduce_to_basis, ignore_global_phase, tol, normalize)

    def get_final_state(self, *args, **kwargs) -> Tensor:
        return self.get_state(float(self._sim_times[-1]), *args, **kwargs)

    def expect(self, obs_list) -> list:
        """simresults.py:81-129."""
        if not isinstance(obs_list, (list, Tensor)):
            raise TypeError("`obs_list` must be a list of operators.")
        legal_shape = (self._dim**self._size, self._dim**self._size)
        out = []
        for obs in obs_list:
            if not isinstance(obs, (Tensor, DiagonalObservable, PauliObservable, StateOverlap)):
                raise TypeError(f"Incompatible type {type(obs)} of observable. Type must be ArrayLike or qutip.Qobj.")
            if tuple(obs.shape) != legal_shape:
                raise ValueError("Incompatible shape of observable." + f"Expected {legal_shape}, got {tuple(obs.shape)}.")
            hit = [k for k, o in enumerate(self._native_observables) if o is obs]
            if hit and self._native_expect is not None:
                out.append(self._native_expect[hit[0]].sum(dim=-1).to(torch.complex128))
                continue
            if isinstance(obs, StateOverlap):  # the projector |phi><phi|: sum_b |c_b|^2 (kets), sum_b <phi_b|rho_b|phi_b>
                out.append(self.fidelity(obs).sum(dim=-1).to(torch.complex128))
                continue
            out.append(expect(obs, self.states))
        return out

    def overlap(self, obs: StateOverlap) -> Tensor:
        """``<phi_b | psi_b(t_k)>``, complex ``(n_t, B)``: the native values when ``obs`` was handed to ``run(observables=...)``,
        else computed from the stored states."""
        if not isinstance(obs, StateOverlap):
            raise TypeError(f"overlap takes a StateOverlap, got {type(obs)}")
        if self._density:
            raise NotImplementedError("The complex overlap is defined on kets; this is a master-equation run: results.fidelity(obs) "
                                      "gives <phi|rho|phi>.")
        hit = [k for k, o in enumerate(self._overlap_observables) if o is obs]
        if hit and self._native_overlaps is not None:
            return self._native_overlaps[hit[0]]
        return overlap_states(obs, self.states)

    def fidelity(self, obs: StateOverlap) -> Tensor:
        """The fidelity with the target of ``obs``, real ``(n_t, B)``: ``<phi_b| rho_b(t_k) |phi_b>`` in a master-equation run,
        ``|<phi_b|psi_b(t_k)>|^2`` for kets.  The native values when ``obs`` was handed to ``run(observables=...)``, else computed
        from the stored states."""
        if not isinstance(obs, StateOverlap):
            raise TypeError(f"fidelity takes a StateOverlap, got {type(obs)}")
        if not self._density:
            return self.overlap(obs).abs() ** 2
        hit = [k for k, o in enumerate(self._overlap_observables) if o is obs]
        if hit and self._native_fidelities is not None:
            return self._native_fidelities[hit[0]]
        return fidelity_states(obs, self.states)

    def purity(self) -> Tensor:
        """``Tr rho^2`` at every evaluation time, real ``(n_t, B)``: the native values of a master-equation run that was handed a
        ``Purity`` observable, else computed from the stored states (kets: ``<psi|psi>^2``, 1 for a normalised state)."""
        if self._density and self._native_purity is not None:
            return self._native_purity
        return purity_states(self.states)

    def reduced_density_matrix(self, obs: ReducedDensityMatrix) -> Tensor:
        """``Tr_E |psi_b(t_k)><psi_b(t_k)|`` on the qubits of ``obs`` — in a master-equation run ``Tr_E rho_b(t_k)`` — complex
        ``(n_t, B, 2^m, 2^m)``: the native values when ``obs`` was handed to ``run(observables=...)``, else computed from the stored
        states (kets or density matrices)."""
        if not isinstance(obs, ReducedDensityMatrix):
            raise TypeError(f"reduced_density_matrix takes a ReducedDensityMatrix, got {type(obs)}")
        if self._basis_name == "all":
            raise NotImplementedError("ReducedDensityMatrix is not available in the three-level all-basis.")
        hit = [k for k, o in enumerate(self._rdm_observables) if o is obs]
        if hit and self._native_rdms is not None:
            return self._native_rdms[hit[0]]
        return reduced_density_matrix(obs, self.states)

    def entanglement_entropy(self, obs: ReducedDensityMatrix, base: float = 2) -> Tensor:
        """Von Neumann entropy of the subsystem of ``obs`` at every evaluation time, real ``(n_t, B)`` (``base=2``: bits); for a pure
        register state the entanglement entropy between the subsystem and the rest.  For a MIXED register state (master-equation
        runs) it is the entropy of the subsystem, not an entanglement measure: use ``negativity`` for that."""
        return von_neumann_entropy(self.reduced_density_matrix(obs), base)

    def negativity(self, obs: ReducedDensityMatrix, n_first: int) -> Tensor:
        """Negativity of the state of the subsystem of ``obs`` across the cut between its first ``n_first`` listed qubits and the
        others, real ``(n_t, B)`` (``utils.negativity``); an entanglement measure for mixed states too."""
        return negativity(self.reduced_density_matrix(obs), n_first)

    def _occupation_moments(self) -> tuple[Tensor, int]:
        """(the moments S, B_q, B_qr summed over the columns of the initial state like ``expect``: (rows, n_t); the index value of
        the level ``sample_state`` reports as "1": r = 0 in the ground-rydberg basis, 1 in the digital and XY bases)."""
        if self._basis_name == "all":
            raise NotImplementedError("Occupation correlations are not available in the three-level all-basis.")
        if self._native_moments is not None:
            rows = self._native_moments
        else:  # a master-equation run: the moments of the diagonal of rho, the same rows
            rows = dm_occupation_moments(self.states) if self._density else occupation_moments(self.states)
        return rows.sum(dim=-1), 0 if self._basis_name == "ground-rydberg" else 1

    def occupations(self) -> Tensor:
        """``<n_i>`` of every atom (in ``atom_order``) at every evaluation time, real ``(n_t, N)``; "occupied" is the level
        ``sample_state`` reports as "1".  The native values when the run was handed ``OccupationCorrelations()``, else computed
        from the stored states (kets, or the density matrices of a master-equation run: ``Tr(rho n_i)``).  Not normalised by the library (``S = <psi|psi>`` enters as it is)."""
        rows, bit = self._occupation_moments()
        return occupations_from_moments(rows, self._size, bit)

    def occupation_correlations(self, connected: bool = False) -> Tensor:
        """``<n_i n_j>``, real symmetric ``(n_t, N, N)`` with ``<n_i>`` on the diagonal (``n^2 = n``); ``connected=True``:
        ``g_ij = <n_i n_j> - <n_i><n_j>``.  Native when the run was handed ``OccupationCorrelations()``, else from the stored states."""
        rows, bit = self._occupation_moments()
        return connected_correlations(rows, self._size, bit) if connected else occupation_correlations_from_moments(rows, self._size, bit)

    def structure_factor(self, signs) -> Tensor:
        """``sum_ij s_i s_j g_ij / N`` at every evaluation time, real ``(n_t,)``, for a pattern ``signs`` of +-1 over the atoms in
        ``atom_order``; the Neel pattern gives the antiferromagnetic order parameter."""
        return structure_factor(self.occupation_correlations(connected=True), signs)

    def _energy_rows(self, second_moment: bool) -> Tensor:
        """(2, n_t, B) (or (1, n_t, B) where only E was asked for natively and only E is wanted): the native rows of a run that was
        handed ``Energy``, else ``<psi_k|H(t_k)|psi_k>`` and ``|H(t_k) psi_k|^2`` of the stored kets with the explicit matrix of
        ``get_hamiltonian`` (small registers)."""
        if self._density:
            raise NotImplementedError("Energy is not available in master-equation runs; apply get_hamiltonian to the stored density matrices.")
        if self._basis_name == "all":
            raise NotImplementedError("Energy is not available in the three-level all-basis.")
        if self._native_energy is not None and (self._native_energy.shape[0] == 2 or not second_moment):
            return self._native_energy
        if self._states_tbd.numel() == 0:
            raise RuntimeError("States were not stored for this run (store_states=False) and it evaluated no native energy rows"
                               + (" with the second moment" if self._native_energy is not None else "")
                               + ": hand run(observables=[Energy()]) the observable.")
        if self._hamiltonian_at is None:
            raise RuntimeError("These results do not know the sequence's Hamiltonian: hand run(observables=[Energy()]) the observable.")
        states = self.states  # (n_t, dim, B)
        e, m2 = [], []
        for k in range(states.shape[0]):
            h = self._hamiltonian_at(self._sim_times[k].to("cpu")).to_dense().to(states.device) @ states[k]
            e.append((states[k].conj() * h).sum(dim=0).real)
            m2.append((h.conj() * h).sum(dim=0).real)
        return torch.stack([torch.stack(e), torch.stack(m2)])

    def energy(self) -> Tensor:
        """``E(t_k) = <psi(t_k)| H(t_k) |psi(t_k)>`` with the sequence's own Hamiltonian (``get_hamiltonian(t_k)``) at every
        evaluation time, real ``(n_t,)``, summed over the columns of the initial state like ``expect``; not normalised (the state is
        taken as it is).  The native rows when the run was handed ``Energy()``, else computed from the stored states."""
        return self._energy_rows(False)[0].sum(dim=-1)

    def energy_second_moment(self) -> Tensor:
        """``<psi(t_k)| H(t_k)^2 |psi(t_k)> = |H(t_k) psi(t_k)|^2``, real ``(n_t,)``; native with ``Energy(second_moment=True)``."""
        return self._energy_rows(True)[1].sum(dim=-1)

    def energy_variance(self) -> Tensor:
        """``<H^2> - <H>^2`` per column of the initial state, summed over the columns, real ``(n_t,)``; clamped at 0 in the value
        only.  An eigenstate gives rounding noise of about ``1e-12 R^2`` (``R``: the spectral bound of ``H``), not an exact 0:
        ``utils.energy_variance`` states the floor."""
        rows = self._energy_rows(True)
        return energy_variance(rows[0], rows[1]).sum(dim=-1)

    def sample_state(self, t: float, n_samples: int = 1000, t_tol: float = 1.0e-3) -> Counter:
        """simresults.py:497-540: ideal samples, then the detection errors of the SPAM model (a measured 0 flips with
        probability epsilon, a measured 1 with probability epsilon_prime), independently per shot and per atom."""
        t_index = self._get_index_from_time(t, t_tol)
        sampled_state = self._native_sample(t_index, n_samples)
        if sampled_state is None:
            if self._states_tbd.numel() == 0:
                raise RuntimeError(
                    "States were not stored for this run (store_states=False) and it drew no native shots for this time and count: "
                    f"request them with run(..., shots=ShotRequest({n_samples}, times=[{t_index}])) — an int samples the final time, "
                    'times="all" every evaluation time — and ask sample_state for exactly that many samples.')
            sampled_state = self[t_index].get_samples(n_samples)
        if self._meas_errors is None or (self._meas_errors["epsilon"] == 0.0 and self._meas_errors["epsilon_prime"] == 0):
            return sampled_state
        return apply_detection_errors(sampled_state, self._meas_errors["epsilon"], self._meas_errors["epsilon_prime"])

    def sample_final_state(self, N_samples: int = 1000) -> Counter:
        return self.sample_state(float(self._sim_times[-1]), N_samples)

    @property
    def native_shots(self) -> Optional[ShotRequest]:
        """The ``ShotRequest`` of ``run(..., shots=...)`` with the shots the solver drew (``.indices``), or None."""
        return self._native_shots

    def _native_sample(self, t_index: int, n_samples: int) -> Optional[Counter]:
        """The native shots of evaluation time ``t_index`` as bitstring counts, when that time was sampled with exactly
        ``n_samples`` shots (first column of the initial state, like ``TorchResult.get_samples``); else None."""
        req = self._native_shots
        if req is None or req.n_shots != n_samples:  # (master-equation runs: drawn from the diagonal of rho, atom indices as well)
            return None
        pos = req.position_of(t_index)
        if pos is None:
            return None
        outcomes = indices_to_bitstrings(req.indices[pos, 0], self._basis_name, self._meas_basis, self._size)
        return bitstring_counts(outcomes, self._size)


def apply_detection_errors(counts: Counter, eps: float, eps_p: float) -> Counter:
    """Flip every measured bit independently: 0 -> 1 with probability ``eps`` (false positive), 1 -> 0 with probability
    ``eps_p`` (false negative); ``simresults.py:514-540``."""
    shots = list(counts.keys())
    n_detects = np.fromiter(counts.values(), dtype=np.int64, count=len(shots))
    shot_arr = np.array([[int(c) for c in shot] for shot in shots], dtype=np.int64)
    rep = np.repeat(shot_arr, n_detects, axis=0)
    flips = np.random.random_sample(rep.shape) < np.where(rep == 1, eps_p, eps)
    new_shots = rep ^ flips
    weights = 1 << np.arange(rep.shape[1] - 1, -1, -1, dtype=np.int64)
    values, cnt = np.unique(new_shots @ weights, return_counts=True)
    return Counter({np.binary_repr(int(v), rep.shape[1]): int(c) for v, c in zip(values, cnt)})


class NoisyResults(SimulationResults, collections.abc.Sequence):
    """Results of a noisy simulation run (``simresults.py:225-345``): one bitstring distribution per evaluation time,
    aggregated over the stochastic runs."""

    _use_pseudo_dens: bool = True

    def __init__(self, run_output, size: int, basis_name: str, sim_times: Tensor, n_measures: int) -> None:
        basis_name_ = "digital" if basis_name == "all" else basis_name
        super().__init__(size, basis_name_, sim_times)
        self.n_measures = n_measures
        self._results = tuple(run_output)

    def __len__(self) -> int:
        return len(self._results)

    def __getitem__(self, i):
        return self._results[i]

    @property
    def results(self) -> list:
        """Probability distribution of the bitstrings at every evaluation time."""
        return [Counter(res.sampling_dist) for res in self]

    def _pseudo_density_diag(self, t_index: int) -> Tensor:
        """Diagonal of ``_calc_pseudo_density`` (``simresults.py:188-210``): sum_b p(b) |b><b| with '1' -> |r> (index
        bit 0) and '0' -> |g> (index bit 1) in the ground-rydberg basis, canonical order otherwise."""
        diag = torch.zeros(2**self._size, dtype=torch.float64)
        full = 2**self._size - 1
        for bitstr, p in self._results[t_index].sampling_dist.items():
            idx = int(bitstr, 2)
            diag[full - idx if self._basis_name == "ground-rydberg" else idx] = p
        return diag

    def get_state(self, t: float, t_tol: float = 1.0e-3) -> Tensor:
        """The state at time t as a diagonal density matrix (a device for expectation values, not the system's rho)."""
        return torch.diag(self._pseudo_density_diag(self._get_index_from_time(t, t_tol))).to(torch.complex128)

    def get_final_state(self) -> Tensor:
        return self.get_state(float(self._sim_times[-1]))

    @property
    def states(self) -> Tensor:
        return torch.stack([self.get_state(float(t)) for t in self._sim_times])

    def expect(self, obs_list) -> list:
        """simresults.py:81-129 on the pseudo-density: <O>(t) = sum_x p_t(x) O[x, x]."""
        if not isinstance(obs_list, (list, Tensor)):
            raise TypeError("`obs_list` must be a list of operators.")
        legal_shape = (2**self._size, 2**self._size)
        diags = torch.stack([self._pseudo_density_diag(k) for k in range(len(self))])
        out = []
        for obs in obs_list:
            if not isinstance(obs, (Tensor, DiagonalObservable)):
                raise TypeError(f"Incompatible type {type(obs)} of observable. Type must be ArrayLike or qutip.Qobj.")
            if tuple(obs.shape) != legal_shape:
                raise ValueError("Incompatible shape of observable." + f"Expected {legal_shape}, got {tuple(obs.shape)}.")
            if isinstance(obs, DiagonalObservable):
                od = obs.diag.detach().cpu().to(torch.float64)
            else:
                od = torch.diagonal(obs.to_dense() if obs.is_sparse else obs).detach().cpu()
            out.append(diags.to(od.dtype) @ od)
        return out

    def sample_state(self, t: float, n_samples: int = 1000, t_tol: float = 1.0e-3) -> Counter:
        return self[self._get_index_from_time(t, t_tol)].get_samples(n_samples)

    def sample_final_state(self, N_samples: int = 1000) -> Counter:
        return self.sample_state(float(self._sim_times[-1]), N_samples)
