"""User-facing derivative helpers with the contract of ``pulser_diff/derivative.py``: ``deriv_time(f, times, endtimes)`` and
``deriv_param(f, params, times, t_ns)``.

Both are vector-Jacobian products of the run's autograd graph.  On this backend the node behind ``results.expect`` /
``results.states`` is the native adjoint sweep (``rydiff_backward``), which is re-entrant: ``retain_graph=True`` and any
number of VJPs with different one-hot-in-time cotangents are supported (``derivative.py:74-76`` calls it once per time).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor


def _extrapolate(deriv: Tensor, target: int, near: int, far: int) -> None:
    """deriv[target] <- straight line through deriv[near], deriv[far] (equally spaced samples, target two steps past near's
    neighbour): the reference's `a +/- ((a - b) / dt) * 2 * dt`, i.e. a + 2 (a' - b') with the step cancelling out."""
    deriv[target] = deriv[far] + 2.0 * (deriv[near] - deriv[far])


def _fix_border_vals(deriv: Tensor, border_indices: Sequence[int], dt: Tensor) -> Tensor:
    """Piecewise-defined pulses make d f / d t jump at pulse borders; the samples next to a border are replaced by a linear
    continuation of their neighbours (``derivative.py:7-23``).  A border at index 0, or one that directly follows the
    previous border and has room to its right, is continued from the RIGHT (samples idx+1, idx+2); any other border is
    continued from the LEFT, for the sample before it and for the border sample itself."""
    del dt  # the step cancels in the two-point extrapolation
    n = len(deriv)
    previous = 0
    with torch.no_grad():
        for idx in border_indices:
            from_right = idx == 0 or ((idx - previous) == 1 and idx + 3 < n)
            if from_right:
                _extrapolate(deriv, idx, near=idx + 1, far=idx + 2)
            else:
                _extrapolate(deriv, idx - 1, near=idx - 2, far=idx - 3)
                _extrapolate(deriv, idx, near=idx - 1, far=idx - 2)
            previous = idx
    return deriv


def deriv_time(f: Tensor, times: Tensor, pulse_endtimes: Optional[Sequence[int]] = None) -> Tensor:
    """d f(t_k) / d t_k for every evaluation time (the run must have been made with ``time_grad=True``); with
    ``pulse_endtimes`` (``TorchEmulator.endtimes``) the artefacts at pulse borders are smoothed (``derivative.py:26-46``)."""
    (grad,) = torch.autograd.grad(f, times, grad_outputs=torch.ones_like(f), retain_graph=True)
    if pulse_endtimes is None:
        return grad
    return _fix_border_vals(grad, pulse_endtimes, times[1] - times[0])


def deriv_param(f: Tensor, x: list, times: Optional[Tensor] = None, t=None):
    """Gradient of f at ONE evaluation time w.r.t. the tensors in ``x`` (``derivative.py:49-78``): the final time when
    ``times`` is not given, else the evaluation time closest to ``t`` (in ns; default: the last one)."""
    if times is None:
        index = len(f) - 1
    else:
        t_us = float(times[-1]) if t is None else float(t) / 1000.0
        index = int(torch.argmin(torch.abs(times.detach() - t_us)))
    cotangent = torch.zeros(len(f), dtype=torch.float64, device=f.device)
    cotangent[index] = 1.0
    return torch.autograd.grad(f, x, grad_outputs=cotangent, retain_graph=True)


def deriv_param_all_times(sim, x: list, observables: list, **kw):
    """``deriv_param`` at EVERY evaluation time in one call: ``sim.run_sensitivities(x, observables, **kw)`` — one native
    forward-mode sweep that carries a tangent state per scalar entry of ``x`` instead of one reverse sweep per evaluation time
    (``basic_usage.ipynb``: ``for t in times: deriv_param(f=exp_val, x=diff_params, times=eval_times, t=t)``).  With
    ``route="tangent"`` noisy runs with collapse operators (the master equation: vec(rho) and its tangents on the doubled register)
    and the XY exchange take the sweep too (without it they run the loop of reverse sweeps, as does the three-level basis always);
    master-equation runs also accept ``StateOverlap`` (the fidelity) and ``Purity`` observables.  ``route="adjoint-loop"`` forces the
    loop (the A/B partner).  Returns
    ``Sensitivities``: ``values`` (n_obs, n_t), ``grads[i]`` (n_obs, n_t, *x[i].shape), ``route``."""
    return sim.run_sensitivities(x, observables, **kw)


def deriv_rdm_all_times(sim, x: list, subsystems: list, **kw):
    """Reduced density matrices of ``subsystems`` AND their derivatives w.r.t. the scalar entries of ``x`` at EVERY evaluation time
    in one call: ``sim.run_rdm_sensitivities(x, subsystems, **kw)`` — the tangent sweep of ``deriv_param_all_times`` with
    ``d rho_A = Tr_E(|dpsi><psi| + |psi><dpsi|)`` formed natively at every save point, instead of one reverse sweep per evaluation
    time and scalar functional of ``rho_A``.  Returns ``SubsystemSensitivities``: ``rho[o]`` (n_t, B, 2^m, 2^m), ``drho[o][i]``
    (n_t, B, 2^m, 2^m, *x[i].shape), ``times`` and ``purity`` / ``d_purity`` / ``entropy`` / ``d_entropy``."""
    return sim.run_rdm_sensitivities(x, subsystems, **kw)


def deriv_occupations_all_times(sim, x: list, **kw):
    """The occupation correlations — every ``<n_i>`` and ``<n_i n_j>`` — AND their derivatives w.r.t. the scalar entries of ``x`` at
    EVERY evaluation time in one call: ``sim.run_occupation_sensitivities(x, **kw)`` — the tangent sweep of
    ``deriv_param_all_times`` with the moments of ``2 Re(conj psi . dpsi)`` formed natively at every save point, instead of one
    reverse sweep per evaluation time and scalar functional through ``run(observables=[OccupationCorrelations()])``.  Returns
    ``OccupationSensitivities``: ``moments`` (rows, n_t, B), ``dmoments[i]`` (rows, n_t, B, *x[i].shape), ``times`` and
    ``occupations`` / ``correlations`` / ``structure_factor`` with their ``d_`` twins."""
    return sim.run_occupation_sensitivities(x, **kw)


def quantum_fisher_information_all_times(sim, x: list, **kw):
    """The quantum Fisher information matrix w.r.t. the scalar entries of ``x`` at EVERY evaluation time in one call:
    ``sim.run_quantum_fisher(x, **kw)`` — the tangent sweep of ``deriv_param_all_times`` with the inner products of the tangent states
    reduced at every save point.  Returns ``QuantumGeometry``: ``qfi`` (n_t, D, D), ``qgt``, ``berry``, ``gram``, ``times`` and the
    ``values`` / ``grads`` of the optional ``observables``."""
    return sim.run_quantum_fisher(x, **kw)


def classical_fisher_information_all_times(sim, x: list, **kw):
    """The classical Fisher information matrix of the occupation-basis measurement (bitstrings) w.r.t. the scalar entries of ``x`` at
    EVERY evaluation time in one call: ``sim.run_classical_fisher(x, **kw)`` — the tangent sweep of
    ``quantum_fisher_information_all_times`` with the classical Gram matrix reduced beside the Gram matrix at every save point.
    Returns ``MeasurementFisher``: ``cfi`` and ``qfi`` (n_t, D, D), ``cgram``, ``gram``, ``times`` and the ``values`` / ``grads`` of
    the optional ``observables``."""
    return sim.run_classical_fisher(x, **kw)
