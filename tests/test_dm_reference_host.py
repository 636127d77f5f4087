"""The references of tests/test_gpu_dm_observables_wide.py (tests/helpers.py: dm_rows_reference, dm_cotangent_reference, the ket-style
cotangents, the shaped shot inputs), checked on the CPU against definitions that share nothing with them: PauliObservable.to_dense()
and torch.autograd through dense matrices.  A reference that was wrong in the same way as a kernel would fail here first."""
import numpy as np
import pytest
import torch

from pulser_diff_amd.observables import PauliObservable
from pulser_diff_amd.shots import sample_indices_reference
from tests.helpers import (DM_SHOTS, dm_cotangent_reference, dm_pauli_row, dm_pauli_row_torch, dm_rows_reference, dm_shot_inputs,
                           ket_pauli_cotangent, ket_pauli_row, sample_with_prefix, segmented_prefix, shot_band)


def _paulis(n):
    """As _paulis of tests/test_gpu_dm_observables.py, plus (from 3 atoms) strings on a middle atom: Y on several atoms."""
    a, z = 0, n - 1
    first = [(0.7, {a: "Y", z: "Y"}), (-1.1, {a: "X", z: "Y"}), (0.4, {a: "Z"}), (0.9, {z: "Y"}), (-0.6, {a: "Y"}), (0.3, {a: "Y", z: "Z"})]
    second = [(1.3, {a: "Z", z: "Z"}), (-0.8, {a: "X"}), (0.5, {a: "Y", z: "X"})]
    if n >= 3:
        first.append((0.45, {a: "Y", 1: "Y", z: "Y"}))
        second.append((-0.35, {1: "Y", z: "Z"}))
    return [PauliObservable(n, first), PauliObservable(n, second)]


def _letters(x, z, n):
    return {j: "Y" if (x >> j & 1 and z >> j & 1) else ("X" if x >> j & 1 else "Z") for j in range(n) if (x | z) >> j & 1}


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("n", [3, 4, 5])
def test_tensor_form_pauli_rows_match_the_dense_operators(n):
    rng = np.random.default_rng(40 + n)
    dim = 2 ** n
    rho = _rand(rng, dim, dim)  # deliberately non-Hermitian
    for obs in _paulis(n):
        dense = obs.to_dense().numpy()
        want = float(np.trace(dense @ rho).real)
        want_abs = sum(abs(w) * float(np.abs(PauliObservable(n, [(1.0, _letters(x, z, n))]).to_dense().numpy() * rho.T).sum())
                       for w, x, z in obs.terms)
        got, got_abs = dm_pauli_row(rho, obs.terms, n)
        assert abs(got - want) <= 1e-13 * want_abs, (got, want)
        assert abs(got_abs - want_abs) <= 1e-13 * want_abs
        got_t = float(dm_pauli_row_torch(torch.from_numpy(rho), obs.terms, n))
        assert abs(got_t - want) <= 1e-13 * want_abs


def _dense_rows_torch(v, n, diag, paulis, targets, purity):
    """The definitions through dense matrices, differentiable."""
    dim = 2 ** n
    rho = v.reshape(dim, dim)
    rows = [(torch.from_numpy(o) * rho.diagonal().real).sum() for o in diag]
    rows += [torch.trace(p.to_dense() @ rho).real for p in paulis]
    rows += [(torch.from_numpy(t).conj() @ rho @ torch.from_numpy(t)).real for t in targets]
    if purity:
        rows.append((v.real ** 2 + v.imag ** 2).sum())
    return torch.stack(rows)


def test_row_and_cotangent_references_match_autograd_through_the_dense_definitions():
    n = 3
    dim = 2 ** n
    rng = np.random.default_rng(7)
    v = _rand(rng, dim * dim)
    diag = rng.standard_normal((2, dim))
    targets = _rand(rng, 3, dim)
    paulis = _paulis(n)
    g = rng.standard_normal(2 + 2 + 3 + 1)
    g[1] = g[5] = 0.0
    leaf = torch.from_numpy(v.copy()).requires_grad_(True)
    rows = _dense_rows_torch(leaf, n, diag, paulis, targets, True)
    val, tot = dm_rows_reference(v, n, diag, paulis, targets, True)
    assert np.all(np.abs(val - rows.detach().numpy()) <= 1e-13 * tot)
    assert np.all(tot >= np.abs(val) * (1 - 1e-12))
    (torch.from_numpy(g) * rows).sum().backward()
    cot, ctot = dm_cotangent_reference(v, n, g, diag, paulis, targets, True)
    assert np.all(np.abs(cot - leaf.grad.numpy()) <= 8 * 2.0 ** -52 * ctot)
    assert np.all(ctot >= np.abs(cot) * (1 - 1e-12))
    # every composition the GPU cases use is a subset of these rows: the diagonal and Z-type strings alone stay on the diagonal
    zonly = [PauliObservable(n, [(0.8, {0: "Z"}), (-0.3, {0: "Z", 2: "Z"})])]
    cot, ctot = dm_cotangent_reference(v, n, [0.5, 1.5], diag[:1], zonly)
    off = ~np.eye(dim, dtype=bool).reshape(-1)
    assert not cot[off].any() and not ctot[off].any() and cot[~off].all()


def test_ket_style_references_match_the_dense_operators():
    nq = 6  # the doubled register of 3 atoms
    rng = np.random.default_rng(11)
    v = _rand(rng, 2 ** nq)
    obs = PauliObservable(nq, [(0.6, {0: "Y", 5: "Y", 2: "X"}), (-0.9, {3: "Z", 0: "Y"}), (0.4, {1: "X"})])
    dense = obs.to_dense()
    leaf = torch.from_numpy(v.copy()).requires_grad_(True)
    row = (leaf.conj() @ dense @ leaf).real
    val, tot = ket_pauli_row(v.reshape((2,) * nq), nq, obs.terms)
    assert abs(val - float(row.detach())) <= 1e-13 * tot
    (1.7 * row).backward()
    cot, ctot = ket_pauli_cotangent(v, nq, obs.terms, 1.7)
    assert np.all(np.abs(cot - leaf.grad.numpy()) <= 8 * 2.0 ** -52 * ctot)


@pytest.mark.parametrize("n,batch", [(9, 2), (10, 2), (12, 1)])
def test_shaped_shot_inputs_leave_no_random_shot_in_the_band(n, batch):
    """The inputs of the GPU shot cases at save point 0 (the one state known here).  sample_indices_reference (longdouble prefix) against
    the rule on a second float64 prefix sum in the kernel's order: equal outside the band |u S - C[x]| <= 4 D 2^-53 S, and the band
    holds no randomly drawn uniform.  The two planted uniforms are in it by construction: u = 0 meets C[x] = 0 of the leading zero
    segments, u = 1 - 2^-53 is 2^-53 S below C[D - 1]."""
    dim = 2 ** n
    seg = (dim + 255) // 256
    v0, uniforms = dm_shot_inputs(n, batch, 1100 + n)
    p_all = np.maximum(v0.numpy().reshape(batch, dim, dim)[:, np.arange(dim), np.arange(dim)].real, 0.0)
    for b in range(batch):
        p, u = p_all[b], uniforms[0, b].numpy()
        pop = np.flatnonzero(p > 0)
        assert pop[0] >= 2 * seg and pop[-1] < dim - 3 * seg  # dead segments at both ends: last_pos is not D - 1
        mid = 128 * seg
        assert not p[mid:mid + 4 * seg].any() and 0.2 * dim < len(pop) < 0.45 * dim
        band = shot_band(p, u)
        assert band[:2].all() and not band[2:].any(), np.flatnonzero(band)
        want = sample_indices_reference(p, u)
        got = sample_with_prefix(p, segmented_prefix(p), u)
        assert np.array_equal(got[~band], want[~band])
        assert want[0] == pop[0] and got[0] == pop[0] and (p[got] > 0).all() and len(u) == DM_SHOTS
