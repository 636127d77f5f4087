"""Measurement shots, host side (no GPU): the sampling rule restated on the host (shots.sample_indices_reference), the index ->
bitstring conversion against TorchResult.sampling_dist, the struct mirror, the library's own validation of the shot fields (all of
it runs before anything touches a device) and the routing of CoherentResults.sample_state."""
import ctypes
import itertools
from collections import Counter

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd.result import TorchResult
from pulser_diff_amd.shots import (MAX_SHOTS, SHOT_NONE, ShotRequest, bitstring_counts, indices_to_bitstrings,
                                   sample_indices_reference)
from pulser_diff_amd.simresults import CoherentResults
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call

ONE_BELOW = 1.0 - 2.0 ** -53


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_rule_on_a_hand_made_distribution():
    p = np.array([[0.25, 0.5, 0.25]])
    u = np.array([[0.0, 0.2, 0.25, 0.25 + 1e-12, 0.74, 0.75, ONE_BELOW]])
    # C = (0.25, 0.75, 1): smallest x with C[x] > u — a uniform ON a cumulative value belongs to the next amplitude
    assert sample_indices_reference(p, u).tolist() == [[0, 0, 1, 1, 1, 2, 2]]


def test_clamping_of_the_uniforms():
    p = np.array([[1.0, 1.0, 1.0, 1.0]])
    u = np.array([[-0.5, -0.0, float("nan"), 1.0, 7.0, float("inf"), -float("inf")]])
    # not > 0 (NaN included) counts as 0; 1 and above are clamped to 1 - 2^-53
    assert sample_indices_reference(p, u).tolist() == [[0, 0, 0, 3, 3, 3, 0]]


def test_zero_probability_heads_tails_and_interior_runs_are_never_returned():
    p = np.array([[0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]])  # unnormalised as well: S = 4
    u = np.concatenate([[0.0, ONE_BELOW, 0.75, np.nextafter(0.75, 0.0)], np.linspace(0, 1, 1001)[:-1]])[None]
    x = sample_indices_reference(p, u)[0]
    assert set(x.tolist()) == {2, 6}
    assert x[0] == 2 and x[1] == 6          # u = 0 skips the empty head; u = 1 - 2^-53 stops before the empty tail
    assert x[2] == 6 and x[3] == 2          # u * S = 3 = C[2] exactly: the next POPULATED amplitude, across the interior run
    assert (x[4:] == np.where(u[0, 4:] * 4.0 < 3.0, 2, 6)).all()


def test_an_unnormalised_distribution_gives_what_its_normalised_twin_gives():
    g = np.random.default_rng(5)
    p = np.ldexp(g.integers(0, 64, size=(3, 40)).astype(np.float64), -10)  # dyadic: scaling by 2^k is exact
    p[:, ::7] = 0.0
    u = np.ldexp(g.integers(0, 2 ** 20, size=(3, 500)).astype(np.float64), -20)
    ref = sample_indices_reference(p, u)
    assert (sample_indices_reference(p * 1024.0, u) == ref).all() and (sample_indices_reference(p / 4096.0, u) == ref).all()
    assert (np.take_along_axis(p, ref, axis=1) > 0).all()
    # against the definition, exactly (integers): smallest x with C[x] > u * S
    ci = np.cumsum(np.ldexp(p, 10).astype(np.int64), axis=1)
    ui = np.ldexp(u, 20).astype(np.int64)
    for r in range(3):
        want = [int(np.argmax(ci[r] * 2 ** 20 > ui[r, s] * ci[r, -1])) for s in range(u.shape[1])]
        assert ref[r].tolist() == want


def test_rounding_that_leaves_no_amplitude_takes_the_last_populated_one():
    # S = 1 + 2^-60 in longdouble; u * S for u = 1 - 2^-53 stays below S there, but whatever the arithmetic, the answer is populated
    p = np.array([[1.0, 2.0 ** -60, 0.0]])
    assert sample_indices_reference(p, np.array([[ONE_BELOW, 0.0]])).tolist()[0][1] == 0
    assert sample_indices_reference(p, np.array([[ONE_BELOW]]))[0, 0] in (0, 1)


def test_a_state_that_is_identically_zero_gives_shot_none():
    out = sample_indices_reference(np.zeros((2, 8)), np.array([[0.0, 0.5], [0.3, ONE_BELOW]]))
    assert (out == SHOT_NONE).all() and SHOT_NONE == _native.SHOT_NONE == 0xFFFFFFFF
    mixed = sample_indices_reference(np.array([[0.0, 0.0], [0.0, 1.0]]), np.array([[0.5], [0.5]]))
    assert mixed.tolist() == [[SHOT_NONE], [1]]
    with pytest.raises(ValueError, match="identically zero"):
        indices_to_bitstrings(out, "digital", "digital", 3)


def test_tensors_in_tensors_out_and_shape_checks():
    p = torch.tensor([[[1.0, 0.0, 1.0]], [[0.0, 2.0, 0.0]]], dtype=torch.float64)  # (2, 1, 3)
    u = torch.tensor([[[0.1, 0.6]], [[0.1, 0.6]]], dtype=torch.float64)
    out = sample_indices_reference(p, u)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.int64 and out.tolist() == [[[0, 2]], [[1, 1]]]
    with pytest.raises(ValueError, match="leading axes"):
        sample_indices_reference(np.ones((2, 4)), np.ones((3, 5)))
    with pytest.raises(ValueError, match="non-negative"):
        sample_indices_reference(np.array([[1.0, -1.0]]), np.array([[0.5]]))


# ---- the request object ------------------------------------------------------------------------------------------------------
def test_shot_request_times_and_uniforms():
    assert ShotRequest(5).resolve_times(7).tolist() == [6]
    assert ShotRequest(5, times="all").resolve_times(4).tolist() == [0, 1, 2, 3]
    assert ShotRequest(5, times=[-1, 0, 2]).resolve_times(4).tolist() == [0, 2, 3]
    assert ShotRequest(5, times=torch.tensor([3, 1])).resolve_times(4).dtype == np.int32
    for bad in ([4], [-5], [], [1, 1], [3, -1]):
        with pytest.raises(ValueError):
            ShotRequest(5, times=bad).resolve_times(4)
    for bad in (0, -3, MAX_SHOTS + 1):
        with pytest.raises(ValueError, match="n_shots"):
            ShotRequest(bad)
    with pytest.raises(ValueError, match="times"):
        ShotRequest(5, times="final")
    # torch.manual_seed governs the uniforms; a generator of the caller's does as well
    torch.manual_seed(7)
    a = ShotRequest(6).draw_uniforms(2, 3, "cpu")
    torch.manual_seed(7)
    b = ShotRequest(6).draw_uniforms(2, 3, "cpu")
    assert a.shape == (2, 3, 6) and a.dtype == torch.float64 and torch.equal(a, b) and bool(((a >= 0) & (a < 1)).all())
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert torch.equal(ShotRequest(6, generator=g1).draw_uniforms(1, 1, "cpu"), ShotRequest(6, generator=g2).draw_uniforms(1, 1, "cpu"))
    given = torch.rand(2, 3, 6, dtype=torch.float64)
    assert torch.equal(ShotRequest(6, uniforms=given).draw_uniforms(2, 3, "cpu"), given)
    with pytest.raises(ValueError, match="shape"):
        ShotRequest(6, uniforms=given).draw_uniforms(2, 2, "cpu")
    assert _native.MAX_SHOTS == MAX_SHOTS == 1 << 20 and "ShotRequest" in repr(ShotRequest(3))


# ---- indices -> bitstrings ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["ground-rydberg", "digital", "XY"])
def test_bitstrings_of_one_hot_states_match_sampling_dist_two_levels(basis):
    n = 3
    for x in range(2 ** n):
        ket = torch.zeros(2 ** n, 1, dtype=torch.complex128)
        ket[x, 0] = 1.0
        keys = list(TorchResult(tuple(f"q{i}" for i in range(n)), basis, ket, True).sampling_dist)
        assert len(keys) == 1
        got = indices_to_bitstrings(np.array([x]), basis, basis, n)
        assert format(int(got[0]), f"0{n}b") == keys[0], (basis, x)
        assert bitstring_counts(indices_to_bitstrings(torch.tensor([x, x]), basis, basis, n), n) == Counter({keys[0]: 2})


@pytest.mark.parametrize("meas_basis", ["ground-rydberg", "digital"])
def test_bitstrings_of_one_hot_states_match_sampling_dist_three_levels(meas_basis):
    """Basis "all": the 3^n ket of TorchResult against the index of the same state in the two-qubit-per-atom register
    (r = 01, g = 11, h = 10, atom 0 most significant — Hamiltonian.embedded_three_level)."""
    n = 2
    code = (1, 3, 2)
    for levels in itertools.product(range(3), repeat=n):
        ket = torch.zeros(3 ** n, 1, dtype=torch.complex128)
        ket[sum(lv * 3 ** (n - 1 - i) for i, lv in enumerate(levels)), 0] = 1.0
        keys = list(TorchResult(("q0", "q1"), meas_basis, ket, True).sampling_dist)
        assert len(keys) == 1
        x = 0
        for lv in levels:
            x = 4 * x + code[lv]
        got = indices_to_bitstrings(torch.tensor([x]), "all", meas_basis, n)
        assert format(int(got[0]), f"0{n}b") == keys[0], (meas_basis, levels)
    # the unpopulated code (0, 0) reads 0 under either measurement
    assert indices_to_bitstrings(np.array([0b0001, 0b0100, 0b0000]), "all", meas_basis, 2).tolist() == (
        [1, 2, 0] if meas_basis == "ground-rydberg" else [0, 0, 0])
    with pytest.raises(ValueError):
        indices_to_bitstrings(np.array([1]), "all", "XY", 2)
    with pytest.raises(ValueError):
        indices_to_bitstrings(np.array([1]), "xy", "xy", 2)


def test_three_level_embedding_agrees_with_the_hamiltonian():
    from tests.test_host_logic import _three_level_emulator

    sim, _ = _three_level_emulator(n=2)
    embed = sim._hamiltonian.embedded_three_level()
    code = (1, 3, 2)
    assert embed.tolist() == [4 * code[a] + code[b] for a in range(3) for b in range(3)]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_carries_the_shot_fields():
    names = [f[0] for f in _native.RydProblem._fields_]
    first = names.index("n_shots")
    assert names[first:first + 5] == ["n_shots", "n_shot_times", "shot_times", "shot_uniforms", "shots_out"]
    assert first < names.index("n_overlaps") < names.index("n_pauli_obs")  # in front of the overlap block; the Pauli block stays the tail
    assert ctypes.sizeof(_native.RydProblem) == _native.lib().rydiff_sizeof_problem()
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    assert "#define RYDIFF_MAX_SHOTS (1 << 20)" in header and "#define RYDIFF_SHOT_NONE 0xFFFFFFFFu" in header


def _spec(n=3):
    return ProblemSpec(n, 0.004, 5, (2 ** n - 1,), (2 ** n - 1,), solver=SolverType.KRYLOV_SE)


def _tables(n=3):
    return (torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
            torch.zeros(n * (n - 1) // 2, dtype=torch.float64))


def _shot_call(n=3, batch=2, n_t=4, n_shots=6, times=(1, 3)):
    """A _Call with valid shot fields.  The buffers are HOST tensors: the validation never follows the device pointers."""
    amp, det, u = _tables(n)
    call = _Call(_spec(n), amp, det, u, np.linspace(0, 0.016, n_t), batch, None)
    call.set_shots(np.asarray(times, dtype=np.int32), torch.zeros(len(times), batch, n_shots, dtype=torch.float64),
                   torch.zeros(len(times), batch, n_shots, dtype=torch.int32))
    return call


def test_rydiff_plan_rejects_bad_shot_fields():
    """plan.hpp: build_shots runs with the other field checks, before anything touches a device; with valid fields the call gets as
    far as the plan scratch (NULL here: 'null info or scratch' is the first complaint of a well-formed problem)."""
    L = _native.lib()
    scratch = (ctypes.c_char * _native.PLAN_SCRATCH_BYTES)()

    def plan(mutate, times=(1, 3)):
        call = _shot_call(times=times)
        p = call.problem
        assert (p.n_shots, p.n_shot_times) == (6, len(times)) and p.shot_uniforms and p.shots_out and p.shot_times
        mutate(p)
        _native.check(L.rydiff_plan(ctypes.byref(p), 0, 0, ctypes.cast(scratch, ctypes.c_void_p), None, ctypes.byref(_native.RydPlanInfo())))

    with pytest.raises(ValueError, match="n_shots"):
        plan(lambda p: setattr(p, "n_shots", MAX_SHOTS + 1))
    with pytest.raises(ValueError, match="n_shots"):
        plan(lambda p: setattr(p, "n_shots", -1))
    with pytest.raises(ValueError, match="n_shot_times"):
        plan(lambda p: setattr(p, "n_shot_times", 0))
    with pytest.raises(ValueError, match="n_shot_times"):
        plan(lambda p: setattr(p, "n_shot_times", 5))  # more than n_tsave = 4
    for field in ("shot_times", "shot_uniforms", "shots_out"):
        with pytest.raises(ValueError, match="shot arrays"):
            plan(lambda p, f=field: setattr(p, f, None))
    for bad in ((3, 1), (1, 1), (0, 4), (-1, 2)):  # unsorted, repeated, beyond the last save point, negative
        with pytest.raises(ValueError, match="strictly increasing"):
            plan(lambda p: None, times=bad)
    with pytest.raises(NotImplementedError, match="shard"):
        plan(lambda p: setattr(p, "shard_bits", 1))


def test_tangent_entry_points_refuse_shots():
    L = _native.lib()
    call = _shot_call()
    info = _native.RydPlanInfo()
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0
    assert "shots" in _native.last_error()
    tg = _native.RydTangent()
    tg.n_dir = 1
    rc = L.rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), None, None, None, None, 0, None)
    assert rc == _native.RYDIFF_ENOTIMPL and "shots" in _native.last_error()
    with pytest.raises(NotImplementedError, match="shots"):
        _native.check(rc)
    call.problem.n_shots = 0  # without shots the same call gets past that refusal (and stops at the missing tangents)
    rc = L.rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), None, None, None, None, 0, None)
    assert rc == _native.RYDIFF_EINVAL and "shots" not in _native.last_error()


def test_evolve_tangent_refuses_a_shot_request():
    from pulser_diff_amd.solver import evolve_tangent

    amp, det, u = _tables()
    spec = _spec()
    spec.shots = ShotRequest(4)
    with pytest.raises(NotImplementedError, match="shots"):  # (refused before the inputs are looked at)
        evolve_tangent(amp, det, u, torch.linspace(0, 0.016, 3, dtype=torch.float64), torch.ones(1, 8, dtype=torch.complex128), spec,
                       d_det=torch.zeros(1, 1, 1, 5, dtype=torch.float64))


# ---- sample_state routing ------------------------------------------------------------------------------------------------------
def _filled_request(n_shots, time_indices, indices):
    req = ShotRequest(n_shots, times=list(time_indices))
    req.indices = torch.as_tensor(indices, dtype=torch.int64)
    req.time_indices = tuple(time_indices)
    return req


def _results(states, req, basis="ground-rydberg", meas_errors=None, n=2):
    times = torch.tensor([0.0, 0.1, 0.2], dtype=torch.float64)
    return CoherentResults(states, n, basis, times, basis, meas_errors, atom_order=("q0", "q1")[:n], native_shots=req)


def test_sample_state_returns_the_native_shots_of_a_sampled_time():
    # two sampled times (k = 0 and 2), one trajectory, 5 shots; ground-rydberg reads the complement of the index
    req = _filled_request(5, (0, 2), [[[3, 3, 3, 3, 3]], [[0, 0, 1, 3, 0]]])
    res = _results(torch.empty(0, 1, 4, dtype=torch.complex128), req)
    assert res.native_shots is req
    assert res.sample_state(0.0, 5) == Counter({"00": 5})
    assert res.sample_final_state(5) == Counter({"11": 3, "10": 1, "00": 1})
    assert _results(torch.empty(0, 1, 4, dtype=torch.complex128), req, basis="digital").sample_final_state(5) == Counter({"00": 3, "01": 1, "11": 1})
    # detection errors still act on top: every measured 1 is lost, every measured 0 stays
    lossy = _results(torch.empty(0, 1, 4, dtype=torch.complex128), req, meas_errors={"epsilon": 0.0, "epsilon_prime": 1.0})
    assert lossy.sample_final_state(5) == Counter({"00": 5})


def test_sample_state_falls_back_to_the_stored_states():
    states = torch.zeros(3, 1, 4, dtype=torch.complex128)
    states[:, 0, 3] = 1.0  # |gg> at every time: '00'
    req = _filled_request(5, (2,), [[[0, 0, 0, 0, 0]]])  # native shots that say '11', so the route taken is visible
    res = _results(states, req)
    assert res.sample_final_state(5) == Counter({"11": 5})       # native
    assert res.sample_final_state(7) == Counter({"00": 7})       # n_samples mismatch: the stored state
    assert res.sample_state(0.1, 5) == Counter({"00": 5})        # a time that was not sampled: the stored state
    assert _results(states, None).sample_final_state(5) == Counter({"00": 5})
    pending = ShotRequest(5)                                        # a request that no run has filled
    assert _results(states, pending).sample_final_state(5) == Counter({"00": 5})


def test_sample_state_without_shots_or_states_says_how_to_request_them():
    empty = torch.empty(0, 1, 4, dtype=torch.complex128)
    req = _filled_request(5, (2,), [[[0, 0, 0, 0, 0]]])
    for res, t, n_samples in ((_results(empty, None), 0.2, 5), (_results(empty, req), 0.2, 6), (_results(empty, req), 0.1, 5)):
        with pytest.raises(RuntimeError, match=r"shots=ShotRequest\(") as err:
            res.sample_state(t, n_samples)
        assert "store_states=False" in str(err.value)
    with pytest.raises(RuntimeError, match="States were not stored"):  # the other accessors keep their message
        _results(empty, req).states


def test_run_validates_the_shots_argument_before_anything_runs():
    from pulser_diff_amd import pulses as pl

    seq = pl.Sequence(pl.Register.from_coordinates([[0.0, 0.0], [8.0, 0.0]]), pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(100, 2.0, 0.0, 0.0), "g")
    sim = P.TorchEmulator.from_sequence(seq, compute_device="cpu")
    for bad in (2.5, "10", True, [3]):
        with pytest.raises(TypeError, match="shots"):
            sim.run(shots=bad)
    with pytest.raises(ValueError, match="n_shots"):
        sim.run(shots=0)
    with pytest.raises(NotImplementedError, match="master-equation"):
        sim.run(solver=SolverType.DP5_ME, shots=10)
    noisy = P.TorchEmulator.from_sequence(seq, compute_device="cpu", config=P.SimConfig(noise="doppler", temperature=10.0, runs=2))
    with pytest.raises(NotImplementedError, match="native_shots=True"):
        noisy.run(shots=10)
