"""State-overlap observables without a GPU: the StateOverlap object, its torch fallback, the identities the solver layer relies on
(rotating frame, three-level embedding), the ABI mirror and the validation in front of the device."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd.observables import MAX_OVERLAPS, StateOverlap, overlap_states, pack_overlaps
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, _check_shapes, split_expect
from pulser_diff_amd.utils import expect


def _kets(dim, batch, seed, n_t=None):
    g = torch.Generator().manual_seed(seed)
    shape = (dim, batch) if n_t is None else (n_t, dim, batch)
    v = torch.randn(*shape, generator=g, dtype=torch.complex128)
    return v / v.norm(dim=-2, keepdim=True)


def test_state_overlap_validates_shape_and_dtype():
    o = StateOverlap(_kets(8, 1, 0)[:, 0])
    assert o.shape == (8, 8) and o.batch == 1 and o.targets.shape == (8, 1) and o.targets.dtype == torch.complex128
    o = StateOverlap(_kets(8, 3, 0))
    assert o.shape == (8, 8) and o.batch == 3
    assert StateOverlap(torch.ones(4, dtype=torch.float64)).targets.dtype == torch.complex128  # real amplitudes are fine
    assert StateOverlap(np.ones(4, dtype=np.complex64)).targets.dtype == torch.complex128
    assert o.to("cpu") is o  # moved in place: results look native values up by identity
    with pytest.raises(TypeError):
        StateOverlap(torch.ones(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        StateOverlap(torch.ones(2, 2, 2, dtype=torch.complex128))
    with pytest.raises(ValueError):
        StateOverlap(torch.ones(1, dtype=torch.complex128))
    assert "StateOverlap" in P.__all__


def test_packing_batch_one_against_batch_b_and_the_cap():
    dim, batch = 8, 3
    shared, per_traj = StateOverlap(_kets(dim, 1, 1)), StateOverlap(_kets(dim, batch, 2))
    packed = pack_overlaps([shared, shared], dim, batch)
    assert packed.shape == (2, 1, dim) and packed.dtype == torch.complex128 and packed.is_contiguous()
    packed = pack_overlaps([shared, per_traj], dim, batch)  # one per-trajectory target: every row is repeated over the batch
    assert packed.shape == (2, batch, dim)
    assert torch.equal(packed[0], shared.targets.T.expand(batch, dim)) and torch.equal(packed[1], per_traj.targets.T)
    with pytest.raises(ValueError):  # 2 targets for a batch of 3
        pack_overlaps([StateOverlap(_kets(dim, 2, 3))], dim, batch)
    with pytest.raises(ValueError):  # wrong dimension
        pack_overlaps([StateOverlap(_kets(4, 1, 3))], dim, batch)
    pack_overlaps([shared] * MAX_OVERLAPS, dim, batch)
    with pytest.raises(ValueError):
        pack_overlaps([shared] * (MAX_OVERLAPS + 1), dim, batch)
    assert MAX_OVERLAPS == _native.MAX_OVERLAPS == 16


@pytest.mark.parametrize("target_batch", [1, 3])
def test_overlap_states_is_numpy_vdot(target_batch):
    n_t, dim, batch = 4, 16, 3
    states = _kets(dim, batch, 5, n_t=n_t)
    obs = StateOverlap(_kets(dim, target_batch, 6))
    got = overlap_states(obs, states)
    assert got.shape == (n_t, batch) and got.dtype == torch.complex128
    for k in range(n_t):
        for b in range(batch):
            want = np.vdot(obs.targets[:, b if target_batch > 1 else 0].numpy(), states[k, :, b].numpy())
            assert abs(got[k, b].item() - want) < 1e-14
    # as an operator it is the projector: expect sums |c|^2 over the batch like the other observables
    assert torch.allclose(expect(obs, states), (got.abs() ** 2).sum(-1).to(torch.complex128), atol=1e-15)
    with pytest.raises(NotImplementedError):
        overlap_states(obs, torch.zeros(n_t, dim, dim, batch, dtype=torch.complex128))
    with pytest.raises(ValueError):
        overlap_states(obs, _kets(8, batch, 1, n_t=2))


def test_frame_rotation_leaves_the_overlap_alone():
    """What sesolve relies on in the rotating frame: V = exp(i phi #ones) is unitary, so <V phi|V psi> = <phi|psi>."""
    n, batch = 5, 2
    dim = 2**n
    x = torch.arange(dim)
    ones = sum(((x >> j) & 1).to(torch.float64) for j in range(n))
    rot = torch.exp(1j * 0.37 * ones)
    states, targets = _kets(dim, batch, 7, n_t=3), _kets(dim, batch, 8)
    plain = overlap_states(StateOverlap(targets), states)
    framed = overlap_states(StateOverlap(targets * rot[:, None]), states * rot[None, :, None])
    assert (plain - framed).abs().max().item() < 1e-14 and plain.abs().max().item() > 1e-3


def test_three_level_embedding_leaves_the_overlap_alone():
    """The 3^n amplitudes scattered into the 4^n vector of two qubits per atom (zeros on the unused codes), targets likewise."""
    from tests.test_host_logic import _three_level_emulator

    sim, _ = _three_level_emulator(n=2)
    embed = sim._hamiltonian.embedded_three_level()
    n_q = sim._hamiltonian.problem_spec(solver=SolverType.KRYLOV_SE, tol=0.0, store_states=True).n_qubits
    assert embed.numel() == 9 and n_q == 4
    states, targets = _kets(9, 1, 9, n_t=3), _kets(9, 1, 10)
    big_s = torch.zeros(3, 16, 1, dtype=torch.complex128).index_copy(1, embed, states)
    big_t = torch.zeros(16, 1, dtype=torch.complex128).index_copy(0, embed, targets)
    assert (overlap_states(StateOverlap(targets), states) - overlap_states(StateOverlap(big_t), big_s)).abs().max().item() < 1e-15


def test_ctypes_mirror_carries_the_overlap_fields():
    names = [f[0] for f in _native.RydProblem._fields_]
    first = names.index("n_overlaps")
    assert names[first:first + 3] == ["n_overlaps", "overlap_batch", "overlap_targets"] and first == names.index("tape_steps") + 1
    assert ctypes.sizeof(_native.RydProblem) == _native.lib().rydiff_sizeof_problem()


def _spec(n=3, overlaps=None):
    return ProblemSpec(n, 0.004, 5, (2**n - 1,), (2**n - 1,), solver=SolverType.KRYLOV_SE, overlaps=overlaps)


def _tables(n=3, batch=2):
    return (torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
            torch.zeros(n * (n - 1) // 2, dtype=torch.float64))


def test_check_shapes_rejects_bad_overlap_tensors():
    n, batch = 3, 2
    amp, det, u = _tables(n, batch)
    good = pack_overlaps([StateOverlap(_kets(8, 1, 0)), StateOverlap(_kets(8, batch, 1))], 8, batch)
    _check_shapes(_spec(n, good), amp, det, u, None, batch)
    _check_shapes(_spec(n, good[:, :1].contiguous()), amp, det, u, None, batch)
    for bad in (good[..., :4],                       # wrong dimension
                good[0],                             # not (n_ov, batch, dim)
                good.to(torch.complex64),            # wrong dtype
                good.real.contiguous(),
                good.repeat(1, 2, 1)[:, :3],         # target batch 3: neither 1 nor B
                good[:1].repeat(_native.MAX_OVERLAPS + 1, 1, 1)):  # above the cap
        with pytest.raises(ValueError):
            _check_shapes(_spec(n, bad), amp, det, u, None, batch)
    with pytest.raises(ValueError):  # targets on another device than the states
        _check_shapes(_spec(n, good), amp, det, u, None, batch, torch.device("cuda", 0))


def test_rydiff_plan_rejects_bad_overlap_fields():
    """The library's own validation (plan.hpp: build_overlaps) runs before anything touches a device."""
    n, batch = 3, 2
    amp, det, u = _tables(n, batch)
    targets = pack_overlaps([StateOverlap(_kets(8, batch, 1))], 8, batch)
    L = _native.lib()
    scratch = (ctypes.c_char * _native.PLAN_SCRATCH_BYTES)()

    def plan(mutate):
        call = _Call(_spec(n, targets), amp, det, u, np.linspace(0, 0.016, 3), batch, None)
        assert (call.problem.n_overlaps, call.problem.overlap_batch) == (1, batch) and call.problem.overlap_targets == targets.data_ptr()
        mutate(call.problem)
        _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.cast(scratch, ctypes.c_void_p), None,
                                    ctypes.byref(_native.RydPlanInfo())))

    with pytest.raises(ValueError, match="overlap_batch"):
        plan(lambda p: setattr(p, "overlap_batch", 3))
    with pytest.raises(ValueError, match="overlap_targets"):
        plan(lambda p: setattr(p, "overlap_targets", None))
    with pytest.raises(ValueError, match="n_overlaps"):
        plan(lambda p: setattr(p, "n_overlaps", _native.MAX_OVERLAPS + 1))
    with pytest.raises(ValueError, match="n_overlaps"):
        plan(lambda p: setattr(p, "n_overlaps", -1))
    with pytest.raises(NotImplementedError, match="shard"):
        plan(lambda p: setattr(p, "shard_bits", 1))


def test_split_expect_takes_the_overlap_rows_out_as_complex_numbers():
    expect_rows = torch.arange(5 * 3 * 2, dtype=torch.float64).reshape(5, 3, 2).requires_grad_(True)
    real, ov = split_expect(expect_rows, 2)
    assert real.shape == (1, 3, 2) and ov.shape == (2, 3, 2) and ov.dtype == torch.complex128
    assert torch.equal(ov[1].real, expect_rows[3].detach()) and torch.equal(ov[1].imag, expect_rows[4].detach())
    (ov.abs() ** 2).sum().backward()  # differentiable: d|c|^2 = 2 Re, 2 Im in the two rows
    assert torch.allclose(expect_rows.grad[1:], 2 * expect_rows.detach()[1:], rtol=1e-14, atol=0) and expect_rows.grad[0].abs().max() == 0
    assert split_expect(expect_rows, 0)[1] is None


def test_noisy_and_master_equation_runs_refuse_state_overlaps():
    from pulser_diff_amd import pulses as pl

    seq = pl.Sequence(pl.Register.from_coordinates([[0.0, 0.0], [8.0, 0.0]]), pl.MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(100, 3.0, 0.5, 0.0), "ch")
    obs = StateOverlap(_kets(4, 1, 0))
    emu = P.TorchEmulator.from_sequence(seq, sampling_rate=0.5, compute_device="cpu")
    with pytest.raises(NotImplementedError, match="master-equation"):
        emu.run(solver=SolverType.DP5_ME, observables=[obs])
    emu.set_config(P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="master-equation"):
        emu.run(observables=[obs])
    emu.set_config(P.SimConfig(noise="doppler", runs=2))
    with pytest.raises(NotImplementedError, match="noisy"):
        emu.run(observables=[obs])
    with pytest.raises(ValueError):  # wrong dimension for the register
        emu.run(observables=[StateOverlap(_kets(8, 1, 0))])
