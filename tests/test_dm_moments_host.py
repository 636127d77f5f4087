"""Occupation correlations of master-equation runs (RydProblem.dm_moments), the host side: where the field sits in the struct and the
field-order pins of the other blocks, the validation of plan.hpp: build_dm — answered without a device — the row bookkeeping, the torch
reference observables.dm_occupation_moments against explicit dense operators (tests/dm_moments_reference.py) and against the ket
reference, split_dm_moments next to split_observables, pack_dm_observables, CoherentResults on a density run, and what the backend
keeps refusing."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.lindblad import MasterEquationResult, pack_dm_observables
from pulser_diff_amd.observables import (DensityMatrixObservables, OccupationCorrelations, Purity, ReducedDensityMatrix, dm_occupation_moments,
                                         moment_pair_row, moment_rows, occupation_moments)
from pulser_diff_amd.simresults import CoherentResults
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, split_dm_moments, split_observables
from pulser_diff_amd.utils import DiagonalObservable, connected_correlations, occupations_from_moments, structure_factor
from tests.dm_moments_reference import (dense_moment_rows, dm_moment_cotangent_reference, dm_moment_rows_reference, moment_row_count)
from tests.test_dm_observables_host import N, _dm_call, _plan
from tests.test_dm_rdm_host import _passes_the_field_checks


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_field_sits_in_front_of_the_shot_block_and_every_pinned_block_keeps_its_place():
    names = [f[0] for f in _native.RydProblem._fields_]
    at = names.index
    assert at("dp5_piece_refine") + 1 == at("dm_moments") and at("dm_moments") + 1 == at("n_shots")
    assert dict(_native.RydProblem._fields_)["dm_moments"] is ctypes.c_int32
    assert ctypes.sizeof(_native.RydProblem) == _native.lib().rydiff_sizeof_problem()
    # the pins of the other blocks
    assert names[at("shots_out"):at("shots_out") + 7] == ["shots_out", "bit_moments", "n_rdms", "rdm_masks", "n_dm_rdms", "dm_rdm_masks", "dm_atoms"]
    assert at("dm_shots") - at("dm_atoms") == 13 and at("dm_shots") + 1 == at("tape_steps")
    assert names[at("tape_steps") + 1:at("tape_steps") + 4] == ["n_overlaps", "overlap_batch", "overlap_targets"]
    assert names[-6:] == ["n_pauli_obs", "n_pauli_strings", "pauli_first", "pauli_x", "pauli_z", "pauli_w"]
    assert at("overlap_targets") + 1 == at("n_pauli_obs")
    assert names[at("n_shots"):at("n_shots") + 5] == ["n_shots", "n_shot_times", "shot_times", "shot_uniforms", "shots_out"]
    # the header lists the fields in the order of the mirror
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    assert "int32_t dm_moments;" in header
    assert header.index("const uint8_t* dp5_piece_refine;") < header.index("int32_t dm_moments;") < header.index("int32_t n_shots;")


def _moments_call(n=N, moments=True, rdms=None, purity=True):
    nq = 2 * n
    dm = DensityMatrixObservables(n, purity=purity, rdms=rdms, moments=moments)
    spec = ProblemSpec(nq, 0.004, 5, (2 ** nq - 1,), (2 ** nq - 1,), solver=SolverType.DP5_SE, dm=dm)
    return _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(nq * (nq - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, 3), 1, None)


@pytest.mark.parametrize("bad", [2, -1])
def test_rydiff_plan_rejects_a_bad_flag_without_a_device(bad):
    call = _dm_call(shots=False)
    call.problem.dm_moments = bad
    rc = _plan(call)
    assert rc == _native.RYDIFF_EINVAL, (rc, _native.last_error())
    with pytest.raises(ValueError, match="dm_moments"):
        _native.check(rc)


def test_the_flag_passes_is_ignored_without_a_density_register_and_bit_moments_stays_refused():
    for value in (0, 1):
        call = _dm_call(shots=False)
        call.problem.dm_moments = value
        assert _passes_the_field_checks(call), _native.last_error()
    assert _passes_the_field_checks(_moments_call()), _native.last_error()
    # dm_atoms = 0: ignored like the other dm_* fields, garbage included
    for garbage in (1, 2, -1, 77):
        call = _dm_call(shots=False)
        call.problem.dm_atoms = 0
        call.problem.dm_moments = garbage
        assert _passes_the_field_checks(call), _native.last_error()
    # bit_moments keeps its meaning: with a density-matrix register it is still not implemented, with or without dm_moments
    for value in (0, 1):
        call = _moments_call(moments=bool(value))
        call.problem.bit_moments = 1
        rc = _plan(call)
        assert rc == _native.RYDIFF_ENOTIMPL, (rc, _native.last_error())
        with pytest.raises(NotImplementedError, match="dm_atoms"):
            _native.check(rc)
    sharded = _moments_call()
    sharded.problem.shard_bits = 1
    assert _plan(sharded) == _native.RYDIFF_ENOTIMPL and "shard" in _native.last_error()


def test_the_sweeps_that_refuse_density_registers_keep_refusing():
    L = _native.lib()
    info = _native.RydPlanInfo()
    info.spectral_lo, info.spectral_hi, info.flags = -1.0, 1.0, 0
    call = _moments_call()
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0
    assert "density-matrix" in _native.last_error()
    assert L.rydiff_geometry_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(info), 1,
                                                   _native.TANGENT_DENSITY_MATRIX | _native.TANGENT_PAIR_TERMS) == 0
    assert "dm_atoms" in _native.last_error()
    # evolve_tangent / evolve_geometry: spec.moments (the ket block) together with spec.dm stays refused
    spec = ProblemSpec(4, 0.004, 5, (15,), (15,), moments=True, dm=DensityMatrixObservables(2, moments=True))
    z = torch.zeros(1)
    for fn in (S.evolve_tangent, S.evolve_geometry):
        with pytest.raises(NotImplementedError):
            fn(z, z, z, z, z, spec, d_det=z, flags=_native.TANGENT_DENSITY_MATRIX | _native.TANGENT_MOMENTS)


def test_the_call_carries_the_flag_and_counts_the_block_behind_the_rdm_rows():
    assert _moments_call().problem.dm_moments == 1 and _moments_call(moments=False).problem.dm_moments == 0
    assert _moments_call().problem.bit_moments == 0
    assert _moments_call(moments=False).expect_rows() == 1
    assert _moments_call().expect_rows() == 1 + (1 + 2 + 1)
    assert _moments_call(n=1, purity=False).expect_rows() == 2  # one atom: S and B_0, no pair row
    rdms = [ReducedDensityMatrix([0]), ReducedDensityMatrix([1, 2])]
    assert _moments_call(n=3, moments=False, rdms=rdms).expect_rows() == 1 + 8 + 32
    assert _moments_call(n=3, rdms=rdms).expect_rows() == 1 + 8 + 32 + 7
    dm = DensityMatrixObservables(12, moments=True)
    assert dm.rows() == dm.moment_rows() == 79 == moment_rows(12) == moment_row_count(12)
    assert DensityMatrixObservables(12).moment_rows() == 0


# ---- the torch reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_reference_equals_explicit_traces_with_dense_number_operators(n):
    """Tr(rho n_i n_j) with dense operators, on a random Hermitian rho and on a random non-Hermitian matrix with a complex diagonal:
    only the real diagonal counts.  1e-14: at most 2^4 terms of size ~1."""
    dim, n_t, batch = 2 ** n, 2, 3
    gen = torch.Generator().manual_seed(40 + n)
    m = torch.randn(n_t, dim, dim, batch, generator=gen, dtype=torch.complex128)
    herm = m + m.conj().transpose(1, 2)
    for name, rho in (("hermitian", herm), ("non-hermitian", m)):
        got = dm_occupation_moments(rho)
        assert got.shape == (moment_rows(n), n_t, batch) and got.dtype == torch.float64
        for k in range(n_t):
            for b in range(batch):
                mat = rho[k, :, :, b].numpy()
                assert np.abs(got[:, k, b].numpy() - dense_moment_rows(mat, n)).max() <= 1e-14, (name, k, b)
                want, tot = dm_moment_rows_reference(mat.reshape(-1), n)
                assert np.abs(got[:, k, b].numpy() - want).max() <= 1e-14 and (tot >= np.abs(want) - 1e-14).all()
    # nothing but the real diagonal: a different imaginary diagonal and different off-diagonal entries give the same rows, bit for bit
    other = torch.randn_like(m)
    idx = torch.arange(dim)
    other[:, idx, idx, :] = torch.complex(m[:, idx, idx, :].real, other[:, idx, idx, :].imag)
    assert torch.equal(dm_occupation_moments(other), dm_occupation_moments(m))
    # no clamp: the rows are linear in rho
    assert torch.allclose(dm_occupation_moments(-m), -dm_occupation_moments(m), rtol=0, atol=0)
    if n >= 2:
        assert moment_pair_row(n, 0, 1) == 1 + n and moment_pair_row(n, n - 2, n - 1) == moment_rows(n) - 1


@pytest.mark.parametrize("n", [1, 3, 5])
def test_reference_on_a_pure_state_equals_the_ket_reference(n):
    gen = torch.Generator().manual_seed(60 + n)
    psi = torch.randn(2, 2 ** n, 3, generator=gen, dtype=torch.complex128)  # (n_t, dim, B)
    rho = torch.einsum("txb,tyb->txyb", psi, psi.conj())
    got, want = dm_occupation_moments(rho), occupation_moments(psi)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


def test_reference_is_differentiable_and_checks_its_input():
    n = 2
    rho = torch.randn(1, 4, 4, 1, dtype=torch.complex128, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    g = torch.randn(moment_rows(n), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (dm_occupation_moments(rho)[:, 0, 0] * g).sum().backward()
    want, _ = dm_moment_cotangent_reference(n, g.numpy())
    assert np.abs(rho.grad[0, :, :, 0].numpy().reshape(-1) - want).max() <= 1e-15
    with pytest.raises(ValueError):
        dm_occupation_moments(torch.zeros(1, 4, 1, dtype=torch.complex128))
    with pytest.raises(ValueError):
        dm_occupation_moments(torch.zeros(1, 4, 2, 1, dtype=torch.complex128))
    with pytest.raises(ValueError):
        dm_occupation_moments(torch.zeros(1, 3, 3, 1, dtype=torch.complex128))
    with pytest.raises(NotImplementedError):  # occupation_moments stays as it is
        occupation_moments(torch.zeros(1, 4, 4, 1, dtype=torch.complex128))


def test_reference_rows_and_cotangent_are_adjoint_to_each_other():
    """<g, rows(v)> = Re <cot(g), v> for random v and g: each dense reference of the GPU tests is checked by the other."""
    n = 4
    rng = np.random.default_rng(7)
    v = rng.normal(size=4 ** n) + 1j * rng.normal(size=4 ** n)
    g = rng.normal(size=moment_row_count(n))
    rows, tot = dm_moment_rows_reference(v, n)
    cot, ctot = dm_moment_cotangent_reference(n, g)
    assert abs(np.dot(g, rows) - np.sum(cot.real * v.real + cot.imag * v.imag)) <= 1e-12
    assert (cot.imag == 0).all() and np.count_nonzero(ctot) <= 2 ** n
    # atom 0 is the most significant bit of x: B_0 sums the upper half of the diagonal, B_{n-1} the odd entries
    p = np.real(np.diagonal(v.reshape(16, 16)))
    assert abs(rows[1] - p[8:].sum()) <= 1e-14 and abs(rows[n] - p[1::2].sum()) <= 1e-14
    assert abs(rows[moment_pair_row(n, 0, n - 1)] - p[9::2].sum()) <= 1e-14


# ---- splitting and packing ----------------------------------------------------------------------------------------------------
def test_split_dm_moments_takes_the_block_off_the_end_in_front_of_split_observables():
    rdms = [ReducedDensityMatrix([0])]
    n = 3
    total = 2 + 8 + moment_rows(n)
    expect = torch.arange(total * 2.0, dtype=torch.float64).reshape(total, 2, 1)
    rest, mom = split_dm_moments(expect, n)
    assert torch.equal(mom, expect[10:]) and torch.equal(rest, expect[:10])
    real, ov, rho = split_observables(rest, 0, rdms)
    assert torch.equal(real, expect[:2]) and ov is None and rho[0].shape == (2, 1, 2, 2)
    assert torch.equal(rho[0][:, :, 0, 0].real, expect[2]) and torch.equal(rho[0][:, :, 1, 1].imag, expect[9])
    with pytest.raises(ValueError):
        split_dm_moments(expect[:3], n)


def test_pack_dm_observables_takes_the_request_and_gives_it_no_real_row():
    n = 2
    diag = DiagonalObservable(torch.arange(4.0, dtype=torch.float64))
    rdm = ReducedDensityMatrix([1])
    dm, rows = pack_dm_observables([diag, OccupationCorrelations(), Purity(), rdm], n, 1, "cpu")
    assert dm.moments and dm.rows() == 1 + 1 + 8 + 4 and dm.moment_rows() == 4
    assert rows == [0, -1, 1, 2]
    dm, rows = pack_dm_observables([OccupationCorrelations()], n, 1, "cpu")
    assert dm.moments and dm.rows() == 4 and rows == [-1]
    dm, rows = pack_dm_observables([diag], n, 1, "cpu")
    assert not dm.moments and dm.rows() == 1
    assert MasterEquationResult(torch.zeros(0), {}).moments is None


# ---- results ------------------------------------------------------------------------------------------------------------------
def test_results_of_a_density_run_serve_the_accessors_from_stored_rho_and_from_native_rows():
    gen = torch.Generator().manual_seed(8)
    n, n_t = 3, 2
    m = torch.randn(n_t, 2 ** n, 2 ** n, 1, generator=gen, dtype=torch.complex128)
    rho = m + m.conj().transpose(1, 2)
    times = torch.linspace(0, 1, n_t, dtype=torch.float64)
    rows = dm_occupation_moments(rho)
    signs = [1, -1, 1]
    for basis, bit in (("ground-rydberg", 0), ("digital", 1)):
        stored = CoherentResults(rho, n, basis, times, basis, atom_order=("a", "b", "c"), density=True)
        native = CoherentResults(rho[:0], n, basis, times, basis, atom_order=("a", "b", "c"), density=True, native_moments=rows)
        want = occupations_from_moments(rows.sum(dim=-1), n, bit)
        assert stored.occupations().shape == (n_t, n)
        assert torch.equal(stored.occupations(), want) and torch.equal(native.occupations(), want)
        for connected in (False, True):
            a, b = stored.occupation_correlations(connected), native.occupation_correlations(connected)
            assert a.shape == (n_t, n, n) and torch.equal(a, b)
        assert torch.equal(stored.structure_factor(signs), native.structure_factor(signs))
        assert torch.equal(native.structure_factor(signs), structure_factor(connected_correlations(rows.sum(dim=-1), n, bit), signs))
        with pytest.raises(RuntimeError, match="not stored"):
            native.states
    # the digital basis counts index bit 1, the ground-rydberg basis index bit 0: <n_i> of one is S - <n_i> of the other
    gr = CoherentResults(rho, n, "ground-rydberg", times, "ground-rydberg", density=True).occupations()
    dg = CoherentResults(rho, n, "digital", times, "digital", density=True).occupations()
    assert float((gr + dg - rows[0].sum(dim=-1)[:, None]).abs().max()) <= 1e-13
    assert float((dg - rows[1:1 + n].sum(dim=-1).T).abs().max()) <= 1e-13
    with pytest.raises(RuntimeError, match="not stored"):
        CoherentResults(rho[:0], n, "ground-rydberg", times, "ground-rydberg", density=True).occupations()


# ---- the backend ---------------------------------------------------------------------------------------------------------------
def test_the_backend_keeps_refusing_what_it_does_not_serve():
    from tests.test_pauli_observables_host import _emulator

    obs = OccupationCorrelations()
    plain = _emulator(3)
    dephasing = _emulator(3)
    dephasing.set_config(P.SimConfig(noise="dephasing"))
    for emu, kwargs in ((plain, dict(solver=P.SolverType.DP5_ME)), (dephasing, {})):
        for stored in (dict(), dict(store_states=True)):
            with pytest.raises(NotImplementedError, match="master-equation") as info:
                emu.run(observables=[obs], **kwargs, **stored)
            assert "store_states=False" in str(info.value) and "results.occupations()" in str(info.value)
    averaging = _emulator(3)
    averaging.set_config(P.SimConfig(noise="doppler", runs=2))
    for kwargs in (dict(), dict(solver=P.SolverType.DP5_ME, store_states=False)):
        with pytest.raises(NotImplementedError, match="average"):
            averaging.run(observables=[obs], **kwargs)
    both = _emulator(3)
    both.set_config(P.SimConfig(noise=("doppler", "dephasing"), runs=2))
    with pytest.raises(NotImplementedError, match="average"):
        both.run(observables=[obs], store_states=False)
    for kwargs in (dict(), dict(solver=P.SolverType.DP5_ME, store_states=False)):
        with pytest.raises(NotImplementedError, match="three-level"):
            _emulator(2, basis="all").run(observables=[obs], **kwargs)
