"""Density-matrix observables (RydProblem.dm_*), the host side: the struct handshake, every validation rule of plan.hpp: build_dm —
which must answer without a device — the Python statement of the index and phase arithmetic against dense traces, and the shot
rule on the clamped diagonal."""
import ctypes

import numpy as np
import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd.observables import (DensityMatrixObservables, PauliObservable, Purity, StateOverlap, dm_trace_indices, fidelity_states,
                                         purity_states)
from pulser_diff_amd.shots import SHOT_NONE, ShotRequest, sample_indices_reference
from pulser_diff_amd.simresults import CoherentResults
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call


def test_ctypes_mirror_carries_the_dm_fields():
    names = [f[0] for f in _native.RydProblem._fields_]
    first = names.index("dm_atoms")
    assert names[first:first + 14] == ["dm_atoms", "n_dm_diag", "dm_diag", "n_dm_pauli_obs", "n_dm_pauli_strings", "dm_pauli_first",
                                       "dm_pauli_x", "dm_pauli_z", "dm_pauli_w", "n_dm_fid", "dm_fid_batch", "dm_fid_targets",
                                       "dm_purity", "dm_shots"]
    # behind the RDM and shots blocks, in front of tape_steps; the Pauli block stays the tail
    assert names.index("rdm_masks") < first and names[first + 14] == "tape_steps" and names[-1] == "pauli_w"
    assert ctypes.sizeof(_native.RydProblem) == _native.lib().rydiff_sizeof_problem()
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    assert f"#define RYDIFF_MAX_DM_ATOMS {_native.MAX_DM_ATOMS}" in header and f"#define RYDIFF_MAX_DM_DIAG {_native.MAX_DM_DIAG}" in header


N, B, N_T = 2, 2, 3


def _dm_call(shots=True):
    """A _Call on the doubled register of two atoms with every density-matrix field set.  HOST tensors: the validation never follows
    the device pointers."""
    dim = 2 ** N
    dm = DensityMatrixObservables(N, diag=torch.zeros(2, dim, dtype=torch.float64),
                                  pauli=[PauliObservable(N, [(1.0, "XY"), (0.5, "ZI")]), PauliObservable(N, [(2.0, "YY")])],
                                  targets=torch.zeros(3, B, dim, dtype=torch.complex128), purity=True, shots=shots)
    nq = 2 * N
    spec = ProblemSpec(nq, 0.004, 5, (2 ** nq - 1,), (2 ** nq - 1,), solver=SolverType.DP5_SE, dm=dm)
    call = _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(nq * (nq - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, N_T), B, None)
    if shots:
        call.set_shots(np.asarray([2], dtype=np.int32), torch.zeros(1, B, 5, dtype=torch.float64), torch.zeros(1, B, 5, dtype=torch.int32))
    return call


def _plan(call):
    scratch = (ctypes.c_char * _native.PLAN_SCRATCH_BYTES)()
    return _native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.cast(scratch, ctypes.c_void_p), None,
                                    ctypes.byref(_native.RydPlanInfo()))


def test_the_call_carries_the_block():
    p = _dm_call().problem
    assert (p.dm_atoms, p.n_dm_diag, p.n_dm_pauli_obs, p.n_dm_pauli_strings, p.n_dm_fid, p.dm_fid_batch, p.dm_purity, p.dm_shots) == (
        N, 2, 2, 3, 3, B, 1, 1)
    assert p.dm_diag and p.dm_pauli_first and p.dm_pauli_x and p.dm_pauli_z and p.dm_pauli_w and p.dm_fid_targets


BAD = [
    ("n_qubits", lambda p: setattr(p, "dm_atoms", 3), "2 \\* dm_atoms"),
    ("atoms-range", lambda p: setattr(p, "dm_atoms", -1), "dm_atoms"),
    ("atoms-cap", lambda p: setattr(p, "dm_atoms", _native.MAX_DM_ATOMS + 1), "dm_atoms"),
    ("diag-count", lambda p: setattr(p, "n_dm_diag", _native.MAX_DM_DIAG + 1), "n_dm_diag"),
    ("diag-negative", lambda p: setattr(p, "n_dm_diag", -1), "n_dm_diag"),
    ("diag-null", lambda p: setattr(p, "dm_diag", None), "dm_diag"),
    ("pauli-count", lambda p: setattr(p, "n_dm_pauli_strings", _native.MAX_PAULI_STRINGS + 1), "n_dm_pauli"),
    ("pauli-negative", lambda p: setattr(p, "n_dm_pauli_obs", -1), "n_dm_pauli"),
    ("pauli-end", lambda p: setattr(p, "n_dm_pauli_strings", 2), "dm_pauli_first"),
    ("pauli-first-null", lambda p: setattr(p, "dm_pauli_first", None), "Pauli arrays"),
    ("pauli-x-null", lambda p: setattr(p, "dm_pauli_x", None), "Pauli arrays"),
    ("pauli-z-null", lambda p: setattr(p, "dm_pauli_z", None), "Pauli arrays"),
    ("pauli-w-null", lambda p: setattr(p, "dm_pauli_w", None), "Pauli arrays"),
    ("fid-count", lambda p: setattr(p, "n_dm_fid", _native.MAX_OVERLAPS + 1), "n_dm_fid"),
    ("fid-negative", lambda p: setattr(p, "n_dm_fid", -1), "n_dm_fid"),
    ("fid-batch", lambda p: setattr(p, "dm_fid_batch", 3), "dm_fid_batch"),
    ("fid-null", lambda p: setattr(p, "dm_fid_targets", None), "dm_fid_targets"),
    ("purity-range", lambda p: setattr(p, "dm_purity", 2), "dm_purity"),
    ("shots-range", lambda p: setattr(p, "dm_shots", -1), "dm_shots"),
    ("shots-without-n_shots", lambda p: setattr(p, "n_shots", 0), "n_shots"),
]


@pytest.mark.parametrize("mutate,match", [b[1:] for b in BAD], ids=[b[0] for b in BAD])
def test_rydiff_plan_rejects_bad_dm_fields_without_a_device(mutate, match):
    """Every rule is RYDIFF_EINVAL and is answered before anything touches a device (this test runs without one)."""
    call = _dm_call()
    mutate(call.problem)
    rc = _plan(call)
    assert rc == _native.RYDIFF_EINVAL, (rc, _native.last_error())
    with pytest.raises(ValueError, match=match):
        _native.check(rc)


def test_mask_bits_at_or_above_the_atom_count_are_rejected():
    for which in (1, 2):  # the x mask, the z mask
        call = _dm_call()
        arr = call.dm_buffers[2][which]
        arr[1] |= 1 << N  # atom 2 of a 2-atom register (a legal qubit of the DOUBLED register: the ket block would take it)
        assert _plan(call) == _native.RYDIFF_EINVAL and "atom" in _native.last_error()


def test_sharded_and_tangent_calls_are_refused():
    call = _dm_call()
    call.problem.shard_bits = 1
    rc = _plan(call)
    assert rc == _native.RYDIFF_ENOTIMPL and "shard" in _native.last_error()
    L = _native.lib()
    call = _dm_call(shots=False)
    info = _native.RydPlanInfo()
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0
    tg = _native.RydTangent()
    tg.n_dir = 1
    rc = L.rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), None, None, None, None, 0, None)
    assert rc == _native.RYDIFF_ENOTIMPL and "density-matrix" in _native.last_error()


def test_dm_atoms_zero_ignores_the_block():
    """dm_atoms = 0: nothing changes — a well-formed problem then gets as far as the first device touch would (here: an n_qubits that
    no longer has to be even, and garbage in the other dm fields, pass the field checks)."""
    call = _dm_call(shots=False)
    p = call.problem
    p.dm_atoms = 0
    p.n_dm_diag = -5
    p.n_dm_fid = 99
    scratch = None
    rc = _native.lib().rydiff_plan(ctypes.byref(p), 0, 0, scratch, None, ctypes.byref(_native.RydPlanInfo()))
    assert rc == _native.RYDIFF_EINVAL and "null info or scratch" in _native.last_error()


def test_python_side_checks():
    dim = 2 ** N
    with pytest.raises(ValueError, match="n_qubits"):
        DensityMatrixObservables(N).check(2 * N + 1, 1)
    with pytest.raises(ValueError, match="diag"):
        DensityMatrixObservables(N, diag=torch.zeros(1, dim + 1, dtype=torch.float64)).check(2 * N, 1)
    with pytest.raises(ValueError, match="targets"):
        DensityMatrixObservables(N, targets=torch.zeros(1, 3, dim, dtype=torch.complex128)).check(2 * N, 2)
    with pytest.raises(ValueError):
        DensityMatrixObservables(N, pauli=[PauliObservable(N + 1, [(1.0, "XXX")])]).check(2 * N, 1)
    dm = DensityMatrixObservables(N, diag=torch.zeros(2, dim, dtype=torch.float64), pauli=[PauliObservable(N, [(1.0, "XY")])], purity=True)
    assert dm.rows() == 4


# ---- the index and phase arithmetic --------------------------------------------------------------------------------------------
def _random_rho(n, seed):
    g = np.random.default_rng(seed)
    dim = 2 ** n
    return g.normal(size=(dim, dim)) + 1j * g.normal(size=(dim, dim))  # deliberately NOT Hermitian


@pytest.mark.parametrize("n", [1, 2, 3])
def test_trace_indices_match_dense_traces_for_non_hermitian_rho(n):
    g = np.random.default_rng(5 + n)
    for trial in range(12):
        string = "".join(g.choice(list("IXYZ"), size=n))
        obs = PauliObservable(n, [(float(g.normal()), string)])
        if len(obs) == 0:
            continue
        rho = _random_rho(n, 100 * n + trial)
        dense = obs.to_dense().numpy()
        want = np.trace(dense @ rho)
        got = sum(w * (phase * rho[rows, cols]).sum() for w, rows, cols, phase in dm_trace_indices(obs))
        assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (string, got, want)
        # the library's row is the real part of the same sum over v = vec(rho): v[(x ^ xm) 2^n + x]
        v = rho.reshape(-1)
        row = sum(w * (phase * v[rows * 2 ** n + cols]).sum() for w, rows, cols, phase in dm_trace_indices(obs)).real
        assert abs(row - want.real) <= 1e-13 * max(1.0, abs(want))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_torch_fallbacks_state_the_definitions(n):
    dim = 2 ** n
    rho = np.stack([_random_rho(n, 7 * n + b) for b in range(2)], axis=-1)[None]  # (1, dim, dim, 2)
    phi = np.random.default_rng(n).normal(size=(dim, 2)) + 1j * np.random.default_rng(n + 9).normal(size=(dim, 2))
    fid = fidelity_states(StateOverlap(torch.from_numpy(phi)), torch.from_numpy(rho)).numpy()
    pur = purity_states(torch.from_numpy(rho)).numpy()
    for b in range(2):
        assert abs(fid[0, b] - (phi[:, b].conj() @ rho[0, :, :, b] @ phi[:, b]).real) < 1e-12
        assert abs(pur[0, b] - (np.abs(rho[0, :, :, b]) ** 2).sum()) < 1e-12
    ket = torch.from_numpy(phi)[None]  # (1, dim, 2)
    assert np.allclose(purity_states(ket).numpy(), (np.abs(phi) ** 2).sum(0) ** 2)
    assert np.allclose(fidelity_states(StateOverlap(torch.from_numpy(phi)), ket).numpy(), (np.abs(phi) ** 2).sum(0) ** 2)


# ---- the shot rule on the clamped diagonal ----------------------------------------------------------------------------------------
def dm_shot_reference(rho, uniforms):
    """numpy statement of the rule: p[x] = max(Re rho[x][x], 0), then the rule of the ket shots (shots.sample_indices_reference)."""
    p = np.maximum(np.real(np.diagonal(rho, axis1=-2, axis2=-1)), 0.0)
    return sample_indices_reference(p, uniforms)


def test_shot_rule_on_a_hand_made_density_matrix():
    rho = np.zeros((1, 4, 4), dtype=complex)
    rho[0] = np.diag([0.5 + 3j, -0.25, 0.0, 0.25])  # a negative entry clamps to 0; the imaginary part is ignored
    rho[0, 0, 3] = 9.0  # off-diagonal entries play no part
    u = np.array([[0.0, 0.3, 0.666, 0.667, 0.9999, 1.0 - 2.0 ** -53, float("nan"), -1.0, 2.0]])
    got = dm_shot_reference(rho, u)
    assert got.tolist() == [[0, 0, 0, 3, 3, 3, 0, 0, 3]]
    assert not np.isin(got, [1, 2]).any()  # p = 0 there: never returned
    assert (dm_shot_reference(np.zeros((1, 4, 4), dtype=complex), u) == SHOT_NONE).all()
    assert (dm_shot_reference(-np.eye(4)[None] + 0j, u) == SHOT_NONE).all()  # everything clamps to zero


@pytest.mark.parametrize("n", [2, 4, 7])
def test_few_shots_sit_on_a_cumulative_boundary(n):
    """The GPU test may leave out shots whose u * S lies within 1e-12 * S of a cumulative boundary (another summation order may
    decide them differently), but for at most 1 % of the shots: with the seeds it uses, the reference alone leaves out far fewer."""
    dim = 2 ** n
    g = torch.Generator().manual_seed(1000 + n)
    p = torch.rand(2, dim, generator=g, dtype=torch.float64).numpy()
    u = torch.rand(2, 4096, generator=g, dtype=torch.float64).numpy()
    for b in range(2):
        cum = np.cumsum(p[b])
        near = np.abs(u[b][:, None] * cum[-1] - cum[None, :]).min(axis=1) <= 1e-12 * cum[-1]
        assert near.mean() < 1e-3


# ---- results -----------------------------------------------------------------------------------------------------------------------
def _density_results(**kw):
    n_t, dim = 3, 4
    rho = torch.zeros(n_t, dim, dim, 1, dtype=torch.complex128)
    rho[:, 3, 3, 0] = 1.0
    return CoherentResults(rho if kw.pop("stored", True) else rho[:0], 2, "ground-rydberg", torch.linspace(0, 1, n_t), "ground-rydberg",
                           density=True, **kw)


def test_results_serve_native_values_and_fall_back_to_stored_rho():
    obs = StateOverlap(torch.tensor([0, 0, 0, 1.0], dtype=torch.complex128))
    other = StateOverlap(torch.tensor([1.0, 0, 0, 0], dtype=torch.complex128))
    fid = torch.full((3, 1), 0.25, dtype=torch.float64)
    pur = torch.full((3, 1), 0.5, dtype=torch.float64)
    res = _density_results(overlap_observables=[obs], native_fidelities=[fid], native_purity=pur)
    assert res.fidelity(obs) is fid and res.purity() is pur
    assert torch.equal(res.fidelity(other), torch.zeros(3, 1, dtype=torch.float64))  # not handed to run: from the stored rho
    assert torch.equal(res.expect([obs])[0], fid.sum(-1).to(torch.complex128))
    plain = _density_results()
    assert torch.equal(plain.fidelity(obs), torch.ones(3, 1, dtype=torch.float64)) and torch.equal(plain.purity(), torch.ones(3, 1, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="fidelity"):
        plain.overlap(obs)
    empty = _density_results(stored=False, overlap_observables=[obs], native_fidelities=[fid], native_purity=pur)
    assert empty.fidelity(obs) is fid and empty.purity() is pur
    with pytest.raises(RuntimeError, match="not stored"):
        empty.fidelity(other)


def test_ket_results_have_fidelity_and_purity_too():
    psi = torch.zeros(2, 1, 4, dtype=torch.complex128)  # (n_t, B, dim)
    psi[:, 0, 3] = 1.0
    res = CoherentResults(psi, 2, "ground-rydberg", torch.linspace(0, 1, 2), "ground-rydberg")
    obs = StateOverlap(torch.tensor([0, 0, 0.6, 0.8j], dtype=torch.complex128))
    assert torch.allclose(res.fidelity(obs), torch.full((2, 1), 0.64, dtype=torch.float64))
    assert torch.allclose(res.purity(), torch.ones(2, 1, dtype=torch.float64))


def test_native_shots_of_a_density_run_are_served_as_bitstrings():
    req = ShotRequest(4)
    req.indices = torch.tensor([[[3, 3, 0, 3]]])
    req.time_indices = (2,)
    res = _density_results(stored=False, native_shots=req)
    counts = res.sample_final_state(4)
    assert sum(counts.values()) == 4 and counts["00"] == 3 and counts["11"] == 1  # index 3 = |gg> -> "00" in the ground-rydberg basis


def test_purity_is_exported():
    import pulser_diff_amd as P

    assert P.Purity is Purity
