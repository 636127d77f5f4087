"""Host-side helpers mirroring ``pulser_diff/utils.py`` (same names and argument meaning).

``expect`` (``utils.py:68-86``) keeps the reference's dense-observable semantics for small registers and adds the
matrix-free forms the hot path needs: a diagonal observable is a length-2^N real vector (``DiagonalObservable``),
which is what the native ``k_expect_diag`` kernel consumes — a dense 2^N x 2^N observable is impossible beyond
N ~ 14.
"""
from __future__ import annotations

from functools import lru_cache, reduce
import math
from math import pi, prod, sin

import torch
from torch import Tensor

from .observables import PauliObservable, StateOverlap, expect_pauli, overlap_states

# pyqtorch.matrices restated (imported by the reference at utils.py:7, hamiltonian.py:17)
IMAT = torch.eye(2, dtype=torch.complex128)
XMAT = torch.tensor([[0, 1], [1, 0]], dtype=torch.complex128)
YMAT = torch.tensor([[0, -1j], [1j, 0]], dtype=torch.complex128)
ZMAT = torch.tensor([[1, 0], [0, -1]], dtype=torch.complex128)


class DiagonalObservable:
    """A diagonal observable stored as its diagonal (real, length 2^N).  ``shape`` reports the operator shape so
    it passes the same validation as a dense tensor (``simresults.py:104-109``)."""

    def __init__(self, diag: Tensor):
        self.diag = diag.real.to(torch.float64) if diag.is_complex() else diag.to(torch.float64)

    @property
    def shape(self) -> tuple:
        return (self.diag.shape[0], self.diag.shape[0])

    @property
    def is_sparse(self) -> bool:
        return False

    def to_dense(self) -> Tensor:
        return torch.diag(self.diag.to(torch.complex128))


def real_diagonal(obs, message: str) -> Tensor:
    """The real diagonal of a ``DiagonalObservable`` or of a diagonal (dim, dim) tensor, dense or sparse; ``ValueError(message)``
    where the tensor has an off-diagonal entry."""
    if isinstance(obs, DiagonalObservable):
        return obs.diag
    dense = obs.to_dense() if obs.is_sparse else obs
    if not torch.equal(torch.diag(torch.diagonal(dense)), dense):
        raise ValueError(message)
    return torch.diagonal(dense).real


def kron(*args: Tensor) -> Tensor:
    """utils.py:12-44: Kronecker product; sparse in -> sparse COO out (index arithmetic, no Python loops)."""
    if not all(t.is_sparse for t in args):
        return reduce(torch.kron, tuple(t.to_dense() if t.is_sparse else t for t in args))
    out = args[0].coalesce()
    for m in args[1:]:
        m = m.coalesce()
        ia, va, ib, vb = out.indices(), out.values(), m.indices(), m.values()
        rows = (ia[0][:, None] * m.shape[0] + ib[0][None, :]).reshape(-1)
        cols = (ia[1][:, None] * m.shape[1] + ib[1][None, :]).reshape(-1)
        vals = (va[:, None] * vb[None, :]).reshape(-1)
        out = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals,
                                      (out.shape[0] * m.shape[0], out.shape[1] * m.shape[1])).coalesce()
    return out


def total_magnetization_diag(n_qubits: int, device=None) -> Tensor:
    """Diagonal of sum_j Z_j (Z = diag(+1 for r, -1 for g)); qubit 0 is the most significant bit."""
    x = torch.arange(2**n_qubits, device=device)
    diag = torch.zeros(2**n_qubits, dtype=torch.float64, device=device)
    for j in range(n_qubits):
        diag += 1.0 - 2.0 * ((x >> (n_qubits - 1 - j)) & 1).to(torch.float64)
    return diag


@lru_cache
def total_magnetization(n_qubits: int, use_sparse: bool = False) -> Tensor:
    """utils.py:47-65 (dense or sparse 2^N x 2^N operator)."""
    diag = total_magnetization_diag(n_qubits).to(torch.complex128)
    if use_sparse:
        idx = torch.arange(2**n_qubits)
        return torch.sparse_coo_tensor(torch.stack([idx, idx]), diag, (2**n_qubits, 2**n_qubits)).coalesce()
    return torch.diag(diag)


def expect(obs, states: Tensor) -> Tensor:
    """utils.py:68-86.  states: (n_t, dim, B) kets or (n_t, dim, dim, B) density matrices."""
    if isinstance(obs, PauliObservable):  # matrix-free: index arithmetic, no 2^N x 2^N operator
        if states.is_sparse:
            states = states.to_dense()
        return expect_pauli(obs, states)
    if isinstance(obs, StateOverlap):  # the projector |phi><phi|: sum_b |<phi_b|psi_b>|^2
        return (overlap_states(obs, states).abs() ** 2).sum(dim=-1).to(torch.complex128)
    if isinstance(obs, DiagonalObservable):
        d = obs.diag.to(states.device)
        if states.ndim == 4:  # density matrices: tr(O rho) = sum_x O[x] rho[x, x]
            return (torch.diagonal(states, dim1=1, dim2=2) * d[None, None, :]).sum(dim=(1, 2)).to(states.dtype)
        if states.ndim != 3:
            raise ValueError("DiagonalObservable expects kets (n_t, dim, B) or density matrices (n_t, dim, dim, B).")
        return (states.abs() ** 2 * d[None, :, None]).sum(dim=(1, 2)).to(states.dtype)
    if states.is_sparse:  # a sparse density matrix (tests/test_noise.py:121-125): small, densify
        states = states.to_dense()
    if obs.is_sparse:
        if states.ndim == 3:
            st = states.squeeze(-1)
            return torch.matmul(st.conj(), torch.matmul(obs, st.T)).to_dense().diag()
        return trace(torch.matmul(obs, states.squeeze(-1)))
    if states.ndim == 3:
        return torch.einsum("...ij,jk,...kl->...", states.mH, obs.to(states.device), states)  # <x|O|x>
    if states.ndim == 4:
        return torch.einsum("ij,...jik->...", obs.to(states.device), states)  # tr(Ox)
    raise ValueError("states must have 3 (kets) or 4 (density matrices) dimensions")


def trace(mat: Tensor) -> Tensor:
    """utils.py:89-94: trace of a 2D (sparse or dense) tensor."""
    if mat.is_sparse:
        m = mat.coalesce()
        i = m.indices()
        return m.values()[i[0] == i[1]].sum()
    return torch.diagonal(mat, dim1=-2, dim2=-1).sum(-1)


def vn_entropy(rho: Tensor) -> Tensor:
    """utils.py:97-105."""
    ev = torch.linalg.eigvalsh(rho)
    ev = ev[ev > 0]
    return -(ev * torch.log2(ev)).sum()


def basis_state(dim, number) -> Tensor:
    """utils.py:108-133."""
    dim = (dim,) if isinstance(dim, int) else dim
    number = (number,) if isinstance(number, int) else number
    if len(dim) != len(number):
        raise ValueError(
            "Arguments `number` must have the same length as `dim` of length"
            f" {len(dim)}, but has length {len(number)}."
        )
    n = 0
    for d, s in zip(dim, number):
        n = d * n + s
    ket = torch.zeros(prod(dim), 1)
    ket[n] = 1.0
    return ket


def s(t: float) -> float:
    """utils.py:136-148."""
    return (1 + sin((pi * t - (pi / 2)))) / 2


def interpolate_sine(num_values: int, duration: int) -> Tensor:
    """utils.py:151-180."""
    step_size = duration / (num_values + 1)
    mat = torch.zeros((duration, num_values))
    for k in range(duration):
        idx, r = divmod(k, step_size)
        idx = int(idx)
        h = r / step_size
        if idx > 0:
            mat[k, idx - 1] = 1 - s(h)
        if idx < num_values:
            mat[k, idx] = s(h)
    return mat


def freeze_gc() -> None:
    """Move every object that is alive NOW (torch's ~1e5 module-level objects, the built model) into the garbage collector's
    permanent generation (``gc.freeze()``), after one full collection.  A training loop on a small register runs an epoch in a
    few milliseconds; a generation-2 pass of CPython's collector over torch's object graph takes ~35 ms and comes every few
    dozen epochs — on the 9-qubit timing of round 2 exactly such a pause looked like a 1.8 x slower kernel
    (profiles/r03_small_register_tape_walk.txt).  Call once after the model is built; nothing is leaked (frozen objects stay
    referenced as before, they are only no longer traversed), and ``gc.unfreeze()`` undoes it."""
    import gc

    gc.collect()
    gc.freeze()



def purity(rho: Tensor) -> Tensor:
    """``Re tr rho^2`` of density matrices ``(..., d, d)``: 1 for a pure state, 1/d for the maximally mixed one.  Smooth everywhere —
    the entanglement loss to recommend for gradient-based optimisation."""
    return torch.einsum("...ij,...ji->...", rho, rho).real


def von_neumann_entropy(rho: Tensor, base: float = 2) -> Tensor:
    """``-tr rho log rho`` of Hermitian density matrices ``(..., d, d)`` from ``eigvalsh``, eigenvalues clamped at 0 before ``x log x``
    (``base=2``: bits).  Differentiable, but the gradient is undefined at degenerate spectra (``eigvalsh``) and unbounded at zero
    eigenvalues (pure states, product states); optimise ``purity`` instead."""
    ev = torch.linalg.eigvalsh(0.5 * (rho + rho.mH)).clamp_min(0.0)
    return -torch.special.xlogy(ev, ev).sum(dim=-1) / math.log(base)


def purity_tangent(rho: Tensor, drho: Tensor) -> Tensor:
    """The directional derivative ``2 Re tr(rho drho)`` of ``purity`` at ``rho`` along ``drho`` (both ``(..., d, d)``, broadcast
    against each other)."""
    return 2.0 * torch.einsum("...ij,...ji->...", rho, drho).real


def von_neumann_entropy_tangent(rho: Tensor, drho: Tensor, base: float = 2) -> Tensor:
    """The directional derivative ``-tr(drho (log rho + 1)) / ln(base)`` of ``von_neumann_entropy`` at ``rho`` along the Hermitian
    direction ``drho`` (both ``(..., d, d)``, broadcast against each other), ``log rho`` from ``eigh`` of the Hermitian part.  Defined
    for FULL-RANK ``rho`` only: at a zero eigenvalue (pure states, product states) ``log rho`` does not exist and the result is
    infinite or NaN.  Unlike autograd through ``eigvalsh`` it needs no distinct eigenvalues."""
    ev, vec = torch.linalg.eigh(0.5 * (rho + rho.mH))
    rotated = torch.einsum("...ji,...jk,...ki->...i", vec.conj(), drho.to(vec.dtype), vec).real  # diagonal of V^H drho V
    return -(rotated * (torch.log(ev) + 1.0)).sum(dim=-1) / math.log(base)


def partial_transpose(rho: Tensor, n_first: int) -> Tensor:
    """Matrices ``(..., 2^m, 2^m)`` transposed on the first party: the ``n_first`` LEADING qubits of the matrix ordering
    (``0 < n_first < m``), ``rho^{T_1}[(a1, a2), (b1, b2)] = rho[(b1, a2), (a1, b2)]``."""
    d = rho.shape[-1]
    m = d.bit_length() - 1
    if rho.ndim < 2 or rho.shape[-2] != d or d != 1 << m:
        raise ValueError(f"expected matrices (..., 2^m, 2^m), got {tuple(rho.shape)}")
    if not 0 < int(n_first) < m:
        raise ValueError(f"n_first must split the {m} qubits into two non-empty parties, got {n_first}")
    d1, d2 = 2 ** int(n_first), 2 ** (m - int(n_first))
    return rho.reshape(rho.shape[:-2] + (d1, d2, d1, d2)).transpose(-4, -2).reshape(rho.shape)


def negativity(rho: Tensor, n_first: int) -> Tensor:
    """``(||rho^{T_1}||_1 - tr rho) / 2`` = minus the sum of the negative eigenvalues of the partial transpose (``eigvalsh`` of its
    Hermitian part) of density matrices ``(..., 2^m, 2^m)``; ``n_first`` as in ``partial_transpose``.  Zero for separable states,
    1/2 for a Bell pair.  Differentiable; the gradient is undefined at degenerate spectra (``eigvalsh``)."""
    pt = partial_transpose(rho, n_first)
    ev = torch.linalg.eigvalsh(0.5 * (pt + pt.mH))
    return (-ev).clamp_min(0.0).sum(dim=-1)


def logarithmic_negativity(rho: Tensor, n_first: int, base: float = 2) -> Tensor:
    """``log ||rho^{T_1}||_1`` from the same eigenvalues (``base=2``: 1 for a Bell pair); an upper bound on the distillable
    entanglement.  Differentiable like ``negativity``."""
    pt = partial_transpose(rho, n_first)
    ev = torch.linalg.eigvalsh(0.5 * (pt + pt.mH))
    return torch.log(ev.abs().sum(dim=-1)) / math.log(base)


# ---- occupation correlations from the moments block (observables.occupation_moments / RydProblem.bit_moments) --------------------
def energy_variance(energy: Tensor, second_moment: Tensor, norm=1.0) -> Tensor:
    """``<H^2> - <H>^2`` from the two native energy rows (``observables.Energy``), clamped at 0 — in the value only: where the clamp
    acts the gradient is that of the unclamped difference.  For a state of squared norm ``norm`` (a number, or a tensor of the rows'
    shape) the rows are taken as ``E / norm`` and ``M2 / norm``.  Cancellation floor: both terms are of the size of the squared
    spectral bound ``R^2`` of ``H`` and each carries a relative rounding error of about 1e-13 from the float64 sums over ``2^N``
    amplitudes, so a variance below about ``1e-12 R^2`` — that of an eigenstate — comes back as rounding noise of that size (or 0
    after the clamp), not as the true value; compare it with ``R^2``, never with 0."""
    e, m2 = energy / norm, second_moment / norm
    var = m2 - e * e
    return var + (var.clamp(min=0.0) - var).detach()


def _moment_parts(moments: Tensor, n_qubits: int) -> tuple[Tensor, Tensor, Tensor]:
    """(S (...), B_q (N, ...), B_qr as a symmetric (N, N, ...) with zeros on the diagonal) of rows ``(1 + N + N(N-1)/2, ...)``."""
    n = int(n_qubits)
    if moments.shape[0] != 1 + n + n * (n - 1) // 2:
        raise ValueError(f"the moments of {n} qubits are 1 + N + N(N-1)/2 = {1 + n + n * (n - 1) // 2} rows, got {moments.shape[0]}")
    pairs = torch.zeros((n, n) + tuple(moments.shape[1:]), dtype=moments.dtype, device=moments.device)
    if n > 1:
        iq, ir = torch.triu_indices(n, n, offset=1, device=moments.device)  # lexicographic (q, r): the order of the rows
        pairs = pairs.index_put((iq, ir), moments[1 + n:]).index_put((ir, iq), moments[1 + n:])
    return moments[0], moments[1:1 + n], pairs


def occupations_from_moments(moments: Tensor, n_qubits: int, occupied_bit: int = 0) -> Tensor:
    """``<n_i>`` from the rows ``S, B_q, B_qr`` (``(rows, ...)`` -> ``(..., N)``).  ``occupied_bit``: the index value of the occupied
    level — 0 in the ground-rydberg basis (r is index value 0: ``<n_i> = S - B_i``), 1 in the digital and XY bases (``B_i``)."""
    s, b1, _ = _moment_parts(moments, n_qubits)
    occ = b1 if occupied_bit else s[None] - b1
    return torch.movedim(occ, 0, -1)


def occupation_correlations_from_moments(moments: Tensor, n_qubits: int, occupied_bit: int = 0) -> Tensor:
    """``<n_i n_j>`` from the rows (``(rows, ...)`` -> ``(..., N, N)``): symmetric, diagonal ``<n_i>`` (``n^2 = n``).  With r as index
    value 0, ``<n_i n_j> = S - B_i - B_j + B_ij``."""
    s, b1, b2 = _moment_parts(moments, n_qubits)
    n = int(n_qubits)
    occ = b1 if occupied_bit else s[None] - b1
    nn = b2 if occupied_bit else (s[None, None] + b2) - (b1[:, None] + b1[None, :])  # (a + b == b + a: symmetric bit for bit)
    eye = torch.eye(n, dtype=torch.bool, device=moments.device).reshape((n, n) + (1,) * (moments.ndim - 1))
    nn = torch.where(eye, occ[:, None].expand_as(nn), nn)
    return torch.movedim(torch.movedim(nn, 0, -1), 0, -1)


def connected_correlations(moments: Tensor, n_qubits: int, occupied_bit: int = 0) -> Tensor:
    """``g_ij = <n_i n_j> - <n_i><n_j>`` from the rows (``(rows, ...)`` -> ``(..., N, N)``); diagonal ``<n_i> - <n_i>^2``."""
    occ = occupations_from_moments(moments, n_qubits, occupied_bit)
    return occupation_correlations_from_moments(moments, n_qubits, occupied_bit) - occ[..., :, None] * occ[..., None, :]


def structure_factor(g: Tensor, signs) -> Tensor:
    """``sum_ij s_i s_j g_ij / N`` of connected correlations ``(..., N, N)`` for a pattern of +-1 (the Neel pattern +1, -1, +1, ...
    gives the antiferromagnetic order parameter)."""
    s = torch.as_tensor(signs, dtype=g.dtype, device=g.device)
    if s.ndim != 1 or s.shape[0] != g.shape[-1] or g.shape[-2] != g.shape[-1]:
        raise ValueError(f"signs must hold one entry per atom ({g.shape[-1]}), got {tuple(s.shape)}")
    if not bool(torch.all(s.abs() == 1)):
        raise ValueError("signs must be a pattern of +1 and -1")
    return torch.einsum("i,...ij,j->...", s, g, s) / g.shape[-1]


# ---- their tangents (the Moments block of the tangent sweep: solver.evolve_tangent with _native.TANGENT_MOMENTS) ----------------
# ``occupations_from_moments`` and ``occupation_correlations_from_moments`` are linear in the rows, and ``structure_factor`` is
# linear in g: applied to tangent rows ``dmoments`` as they are they return the tangents.  The connected correlations are not:
def connected_correlations_tangent(moments: Tensor, dmoments: Tensor, n_qubits: int, occupied_bit: int = 0) -> Tensor:
    """``d g_ij = d<n_i n_j> - d<n_i> <n_j> - <n_i> d<n_j>`` (the product rule on ``connected_correlations``) from the rows
    ``moments`` ``(rows, *shape)`` and their tangents ``dmoments`` ``(rows, *lead, *shape)`` — any number of leading direction axes
    in front of the shape of the values — -> ``(*lead, *shape, N, N)``."""
    occ = occupations_from_moments(moments, n_qubits, occupied_bit)
    docc = occupations_from_moments(dmoments, n_qubits, occupied_bit)
    dnn = occupation_correlations_from_moments(dmoments, n_qubits, occupied_bit)
    return dnn - (docc[..., :, None] * occ[..., None, :] + occ[..., :, None] * docc[..., None, :])


def structure_factor_tangent(moments: Tensor, dmoments: Tensor, n_qubits: int, signs, occupied_bit: int = 0) -> Tensor:
    """The tangent of ``structure_factor(connected_correlations(moments, ...), signs)`` along ``dmoments`` (shapes as in
    ``connected_correlations_tangent``) -> ``(*lead, *shape)``."""
    return structure_factor(connected_correlations_tangent(moments, dmoments, n_qubits, occupied_bit), signs)
