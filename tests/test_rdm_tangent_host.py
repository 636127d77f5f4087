"""Reduced-density-matrix tangents from the tangent sweep, host side (no GPU): the C ABI's planning of a call with
RYDIFF_TANGENT_RDMS (every refusal happens before anything touches a device), the scalar tangent formulas of utils against autograd
and the refusals of the public route."""
import ctypes

import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native, utils
from pulser_diff_amd.derivative import deriv_rdm_all_times
from pulser_diff_amd.observables import ReducedDensityMatrix
from tests.test_dm_observables_host import _dm_call
from tests.test_dm_tangent_host import _with_pair
from tests.test_host_logic import _three_level_emulator
from tests.test_rdm_observables_host import _raw_call
from tests.test_tangent_host import _basic_usage_emulator, _info, _params

RDMS = _native.TANGENT_RDMS
ALL = _native.TANGENT_PAIR_TERMS | _native.TANGENT_DENSITY_MATRIX | RDMS


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_workspace_of_an_rdm_problem_with_the_flag():
    """8 qubits, B = 2, one RDM on qubits 0 and 2: with the flag the size is non-zero and grows by at least two state vectors (the
    ping-pong pair) per direction; without it the size is 0 with RYDIFF_ENOTIMPL, as it always was."""
    lib = _native.lib()
    call, info = _raw_call(), _info()
    assert RDMS == 4
    assert lib.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0
    assert "reduced density" in _native.last_error()
    state_bytes = 2 * 256 * 16
    for size_of in (lib.rydiff_tangent_workspace_bytes_flags, lib.rydiff_geometry_workspace_bytes_flags):
        sizes = [size_of(ctypes.byref(call.problem), ctypes.byref(info), d, RDMS) for d in (1, 2, 8)]
        assert sizes[0] > 0, _native.last_error()
        assert sizes[1] - sizes[0] >= 2 * state_bytes and sizes[2] - sizes[1] >= 12 * state_bytes
        assert size_of(ctypes.byref(call.problem), ctypes.byref(info), 1, 0) == 0


def _forward(mutate=None, flags=RDMS, geometry=False, call=None):
    """The sweep with host dummies for every device pointer: a call that gets past validation would touch them."""
    lib = _native.lib()
    c = call or _raw_call()
    if mutate:
        mutate(c.problem)
    tg = _native.RydTangent()
    tg.n_dir, tg.d_amp, tg.flags = 2, 0x1000, flags
    info = _info()
    if geometry:
        rc = lib.rydiff_forward_geometry(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None,
                                         ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
    else:
        rc = lib.rydiff_forward_tangent(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None,
                                        ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
    _native.check(rc)


def test_a_valid_call_with_the_flag_stops_at_the_workspace_test():
    with pytest.raises(MemoryError, match="tangent workspace too small"):
        _forward()
    with pytest.raises(MemoryError, match="geometry workspace too small"):
        _forward(geometry=True)
    with pytest.raises(MemoryError, match="tangent workspace too small"):  # with pair terms (XY kets)
        _forward(_with_pair, flags=RDMS | _native.TANGENT_PAIR_TERMS)


def test_without_the_flag_the_call_is_refused_as_before():
    with pytest.raises(NotImplementedError, match="reduced density"):
        _forward(flags=0)
    with pytest.raises(NotImplementedError, match="reduced density"):
        _forward(flags=0, geometry=True)
    with pytest.raises(NotImplementedError, match="RYDIFF_TANGENT_RDMS"):
        _forward(flags=_native.TANGENT_PAIR_TERMS)


def test_unknown_flag_bits_are_invalid():
    with pytest.raises(ValueError, match="flags"):
        _forward(flags=8)
    with pytest.raises(ValueError, match="flags"):
        _forward(flags=ALL | 8)


def test_partial_traces_of_a_density_matrix_stay_refused_with_every_flag():
    with pytest.raises(NotImplementedError, match="n_dm_rdms"):
        _forward(lambda p: setattr(p, "n_dm_rdms", 1), flags=ALL, call=_dm_call(shots=False))


def test_what_the_sweep_does_not_take_stays_refused_with_the_flag():
    with pytest.raises(NotImplementedError, match="shard"):
        _forward(lambda p: setattr(p, "shard_bits", 1))
    with pytest.raises(NotImplementedError, match="shots"):
        _forward(lambda p: setattr(p, "n_shots", 4))
    with pytest.raises(NotImplementedError, match="conditioned"):
        _forward(lambda p: setattr(p, "amp_conditioned_terms", 1))
    with pytest.raises(NotImplementedError, match="ones-counting"):
        _forward(lambda p: setattr(p, "det_ones_terms", 1))
    with pytest.raises(NotImplementedError, match="RYDIFF_TANGENT_PAIR_TERMS"):
        _forward(_with_pair)


# ---- scalar tangents -----------------------------------------------------------------------------------------------------------------
def _density_matrix(d, seed):
    """A seeded full-rank density matrix (a Wishart matrix of 4 d samples, normalised) and a Hermitian direction."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(d, 4 * d, generator=gen, dtype=torch.complex128)
    rho = a @ a.mH
    rho = rho / torch.einsum("ii->", rho).real
    h = torch.randn(d, d, generator=gen, dtype=torch.complex128)
    return rho, 0.5 * (h + h.mH)


@pytest.mark.parametrize("d, seed", [(2, 11), (8, 12), (64, 13)])
def test_scalar_tangents_match_autograd(d, seed):
    """d/ds f(rho + s drho) at s = 0 by autograd against the closed forms, 1e-10 relative.  The spectrum is kept away from zero
    (smallest eigenvalue > 1e-3, asserted): the entropy tangent exists for full-rank rho only."""
    rho, drho = _density_matrix(d, seed)
    assert float(torch.linalg.eigvalsh(rho).min()) > 1e-3
    for f, tangent in ((utils.purity, utils.purity_tangent), (utils.von_neumann_entropy, utils.von_neumann_entropy_tangent)):
        s = torch.zeros((), dtype=torch.float64, requires_grad=True)
        (want,) = torch.autograd.grad(f(rho + s * drho), s)
        got = tangent(rho, drho)
        assert got.dtype == torch.float64 and got.shape == ()
        assert abs(float(want)) > 1e-3
        assert abs(float(got - want)) <= 1e-10 * abs(float(want))
    # the base, and leading axes that broadcast
    e2, e = utils.von_neumann_entropy_tangent(rho, drho), utils.von_neumann_entropy_tangent(rho, drho, base=torch.e)
    assert abs(float(e2 * torch.log(torch.tensor(2.0, dtype=torch.float64)) - e)) <= 1e-13 * abs(float(e))
    stacked = torch.stack([drho, -2.0 * drho])
    for tangent in (utils.purity_tangent, utils.von_neumann_entropy_tangent):
        both = tangent(rho, stacked)
        assert both.shape == (2,) and abs(float(both[1] + 2.0 * both[0])) <= 1e-12 * abs(float(both[0]))


# ---- public refusals -----------------------------------------------------------------------------------------------------------------
def test_run_rdm_sensitivities_refusals():
    prm = _params()
    args = (prm["q0"], prm["omega"], prm["area"], prm["phase"])
    emu = _basic_usage_emulator(*args)
    with pytest.raises(ValueError, match="deriv_time"):
        emu.run_rdm_sensitivities([prm["omega"], emu.evaluation_times], [(0, 1)])
    with pytest.raises(TypeError):
        deriv_rdm_all_times(emu, [], [(0,)])
    with pytest.raises(NotImplementedError, match="master-equation"):
        emu.run_rdm_sensitivities([prm["omega"]], [(0,)], solver=P.SolverType.DP5_ME)
    with pytest.raises(ValueError, match="outside the register"):
        emu.run_rdm_sensitivities([prm["omega"]], [ReducedDensityMatrix((0, 4))])
    with pytest.raises(ValueError, match="subsystems"):
        emu.run_rdm_sensitivities([prm["omega"]], [(0,)] * 9)
    dephasing = _basic_usage_emulator(*args, config=P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="master-equation"):
        deriv_rdm_all_times(dephasing, [prm["omega"]], [(0,)])
    doppler = _basic_usage_emulator(*args, config=P.SimConfig(noise="doppler", runs=2, temperature=50.0))
    with pytest.raises(NotImplementedError, match="average"):
        doppler.run_rdm_sensitivities([prm["omega"]], [(0,)])
    three, _ = _three_level_emulator()
    leaf = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="three-level"):
        three.run_rdm_sensitivities([leaf], [(0,)])
    # run_sensitivities keeps refusing the observable, and in coherent runs points at the new route
    with pytest.raises(NotImplementedError, match="ReducedDensityMatrix.*run_rdm_sensitivities"):
        emu.run_sensitivities([prm["omega"]], [ReducedDensityMatrix((0,))])
