"""Measurement shots drawn by the native solver while the state is on the device (``include/rydiff.h``: ``RydProblem.n_shots`` /
``shot_*``): a ``ShotRequest`` rides along with a run (``ProblemSpec.shots``, ``sesolve(..., shots=...)``,
``TorchEmulator.run(..., shots=...)``) and receives amplitude indices; ``indices_to_bitstrings`` turns them into measured
bitstrings in the order of ``TorchResult.sampling_dist``.  No stored trajectory, no 2^N probabilities on the host.

The sampling rule is deterministic given the uniforms (which come from ``torch.rand``, so ``torch.manual_seed`` / a generator
governs them): with p[y] = |psi[y]|^2, C[x] = sum_{y <= x} p[y] and S = C[-1], uniform u gives the smallest x with C[x] > u * S;
u is clamped into [0, 1) and anything not > 0 (NaN included) counts as 0; where rounding leaves no such x the largest x with
p[x] > 0 is taken; an x with p[x] == 0 is never returned; S == 0 gives ``SHOT_NONE``.  ``sample_indices_reference`` is that rule
on the host with a ``longdouble`` cumulative sum.
"""
from __future__ import annotations

from collections import Counter
from typing import Any, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from ._native import MAX_SHOTS, SHOT_NONE

__all__ = ["MAX_SHOTS", "SHOT_NONE", "ShotRequest", "sample_indices_reference", "indices_to_bitstrings", "bitstring_counts"]


class ShotRequest:
    """``n_shots`` measurement shots per sampled evaluation time and trajectory.

    ``times``: ``None`` = the final evaluation time only; ``"all"`` = every evaluation time; or save-point indices (strictly
    increasing after sorting, negative values count from the end).  ``generator``: the ``torch.Generator`` the uniforms are drawn
    with (``None``: the device's default generator, i.e. ``torch.manual_seed``).  ``uniforms``: a float64 tensor
    ``(n_shot_times, B, n_shots)`` to use instead of drawing any.

    After the run: ``indices`` holds an ``int64`` tensor ``(n_shot_times, B, n_shots)`` of amplitude indices in the basis order of
    the solver (qubit 0 = most significant bit; three-level registers: two qubits per atom), ``time_indices`` the sampled save
    points and ``last_uniforms`` the uniforms that were used (shot s belongs to uniform s).  A request may serve several runs: every run
    draws fresh uniforms (unless ``uniforms`` was given) and replaces the results.
    """

    def __init__(self, n_shots: int, times: Union[None, str, Sequence[int]] = None, generator: Optional[torch.Generator] = None,
                 uniforms: Optional[Tensor] = None) -> None:
        n_shots = int(n_shots)
        if not 1 <= n_shots <= MAX_SHOTS:
            raise ValueError(f"n_shots must be in [1, {MAX_SHOTS}], got {n_shots}")
        if isinstance(times, str) and times != "all":
            raise ValueError('times must be None (the final evaluation time), "all" or a sequence of save-point indices')
        self.n_shots = n_shots
        self.times = times
        self.generator = generator
        self.uniforms = uniforms
        self.indices: Optional[Tensor] = None
        self.time_indices: Optional[tuple] = None
        self.last_uniforms: Optional[Tensor] = None

    def resolve_times(self, n_tsave: int) -> np.ndarray:
        """The sampled save points of a run with ``n_tsave`` evaluation times: int32, strictly increasing."""
        if self.times is None:
            idx = [n_tsave - 1]
        elif isinstance(self.times, str):
            idx = list(range(n_tsave))
        else:
            idx = [int(k) for k in (self.times.tolist() if isinstance(self.times, (Tensor, np.ndarray)) else self.times)]
            if not idx:
                raise ValueError("ShotRequest.times is empty")
            if any(k < -n_tsave or k >= n_tsave for k in idx):
                raise ValueError(f"ShotRequest.times: save-point indices must lie in [{-n_tsave}, {n_tsave}), got {idx}")
            idx = sorted(k % n_tsave for k in idx)
            if any(a == b for a, b in zip(idx[:-1], idx[1:])):
                raise ValueError(f"ShotRequest.times names a save point twice: {idx}")
        return np.asarray(idx, dtype=np.int32)

    def draw_uniforms(self, n_times: int, batch: int, device) -> Tensor:
        """The uniforms of one run, float64 ``(n_times, batch, n_shots)`` on ``device``: the ones handed in, else ``torch.rand``."""
        shape = (n_times, batch, self.n_shots)
        if self.uniforms is not None:
            u = torch.as_tensor(self.uniforms)
            if tuple(u.shape) != shape:
                raise ValueError(f"ShotRequest.uniforms must have shape {shape}, got {tuple(u.shape)}")
            return u.detach().to(device, torch.float64).contiguous()
        return torch.rand(shape, dtype=torch.float64, device=device, generator=self.generator)

    def position_of(self, k: int) -> Optional[int]:
        """Where save point ``k`` sits among the sampled ones of the finished run (None: not sampled, or no run yet)."""
        if self.indices is None or self.time_indices is None or int(k) not in self.time_indices:
            return None
        return self.time_indices.index(int(k))

    def __repr__(self) -> str:
        done = "pending" if self.indices is None else f"indices {tuple(self.indices.shape)}"
        return f"ShotRequest(n_shots={self.n_shots}, times={self.times!r}, {done})"


def sample_indices_reference(probs: Any, uniforms: Any) -> Any:
    """The sampling rule on the host: ``probs`` (..., dim) non-negative weights (need not be normalised), ``uniforms`` (..., n) —
    leading axes equal — gives int64 indices (..., n).  The cumulative sum is taken in ``longdouble``.  Tensors in, a tensor (on
    the CPU) out; anything else gives a numpy array."""
    as_tensor = isinstance(probs, Tensor) or isinstance(uniforms, Tensor)
    p = np.asarray(probs.detach().cpu() if isinstance(probs, Tensor) else probs, dtype=np.float64)
    u = np.asarray(uniforms.detach().cpu() if isinstance(uniforms, Tensor) else uniforms, dtype=np.float64)
    if p.ndim < 1 or u.ndim != p.ndim or p.shape[:-1] != u.shape[:-1]:
        raise ValueError(f"probs (..., dim) and uniforms (..., n) must agree on the leading axes, got {p.shape} and {u.shape}")
    if (p < 0).any():
        raise ValueError("probs must be non-negative")
    lead, dim = p.shape[:-1], p.shape[-1]
    p2, u2 = p.reshape(-1, dim), u.reshape(-1, u.shape[-1])
    out = np.empty(u2.shape, dtype=np.int64)
    one_below = 1.0 - 2.0 ** -53
    for r in range(p2.shape[0]):
        cum = np.cumsum(p2[r].astype(np.longdouble))
        total = cum[-1]
        if not total > 0:
            out[r] = SHOT_NONE
            continue
        populated = np.flatnonzero(p2[r] > 0)
        # searched among the populated amplitudes alone, so the result never lands on p == 0
        cum_pop = cum[populated]
        ur = np.where(u2[r] > 0, np.minimum(u2[r], one_below), 0.0).astype(np.longdouble)  # NaN > 0 is False -> 0
        pos = np.searchsorted(cum_pop, ur * total, side="right")  # first populated x with C[x] > u * S
        out[r] = populated[np.minimum(pos, len(populated) - 1)]   # none left: the largest x with p[x] > 0
    out = out.reshape(lead + (u.shape[-1],))
    return torch.from_numpy(out) if as_tensor else out


def indices_to_bitstrings(indices: Any, basis_name: str, meas_basis: str, n_atoms: int) -> Any:
    """Amplitude indices -> measured bitstrings as integers (atom 0 = most significant bit; ``format(v, f"0{n_atoms}b")`` is the
    key of ``TorchResult.sampling_dist``).  ground-rydberg: '1' = r = index bit 0, the complement of the index; digital and XY:
    '1' = h / d = index bit 1, the index itself; "all": two qubits per atom, r = (0, 1), g = (1, 1), h = (1, 0) — the bit reads 1
    for r under a ground-rydberg measurement and 1 for h under a digital one, and the unpopulated code (0, 0) reads 0.  Works on
    tensors (any device) and numpy arrays; ``SHOT_NONE`` entries are refused."""
    is_tensor = isinstance(indices, Tensor)
    idx = indices.to(torch.int64) if is_tensor else np.asarray(indices, dtype=np.int64)
    if bool((idx == SHOT_NONE).any()):
        raise ValueError("the sampled state was identically zero (SHOT_NONE): no bitstring to report")
    n = int(n_atoms)
    if basis_name == "ground-rydberg":
        return ((1 << n) - 1) - idx
    if basis_name in ("digital", "XY"):
        return idx
    if basis_name != "all":
        raise ValueError("`basis_name` must be 'ground-rydberg', 'digital', 'all' or 'XY'.")
    if meas_basis not in ("ground-rydberg", "digital"):
        raise ValueError("`meas_basis` must be 'ground-rydberg' or 'digital'.")
    out = idx * 0
    for i in range(n):
        a = (idx >> (2 * n - 1 - 2 * i)) & 1
        b = (idx >> (2 * n - 2 - 2 * i)) & 1
        one = (1 - a) * b if meas_basis == "ground-rydberg" else a * (1 - b)
        out = out | (one << (n - 1 - i))
    return out


def bitstring_counts(outcomes: Any, n_atoms: int) -> Counter:
    """Counter of bitstrings (``'0110'`` -> count) from integer outcomes (``indices_to_bitstrings``)."""
    arr = outcomes.detach().cpu().numpy() if isinstance(outcomes, Tensor) else np.asarray(outcomes)
    values, cnt = np.unique(arr.reshape(-1), return_counts=True)
    return Counter({np.binary_repr(int(v), int(n_atoms)): int(c) for v, c in zip(values, cnt)})
