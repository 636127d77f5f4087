"""Occupation-correlation tangents from the tangent sweep, host side (no GPU): the C ABI's planning of a call with
RYDIFF_TANGENT_MOMENTS (every refusal happens before anything touches a device), the workspace the documented layout asks for, the
tangent helpers of utils against torch.func.jvp and the refusals of the public route."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native, utils
from pulser_diff_amd import solver as S
from pulser_diff_amd.backend import OccupationSensitivities
from pulser_diff_amd.derivative import deriv_occupations_all_times
from pulser_diff_amd.observables import OccupationCorrelations, moment_rows
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, split_moments
from tests.test_dm_tangent_host import _with_pair
from tests.test_host_logic import _three_level_emulator
from tests.test_tangent_host import _basic_usage_emulator, _info, _params

MOMENTS = _native.TANGENT_MOMENTS
KET_FLAGS = _native.TANGENT_PAIR_TERMS | _native.TANGENT_RDMS | MOMENTS
B, N_T = 2, 3


def _call(n=3, moments=True):
    """A _Call on n qubits, B = 2.  HOST tensors: the validation never follows the device pointers."""
    spec = ProblemSpec(n, 0.004, 5, (2 ** n - 1,), (2 ** n - 1,), solver=SolverType.DP5_SE, moments=moments)
    return _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(n * (n - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, N_T), B, None)


def _forward(mutate=None, flags=MOMENTS, geometry=False, call=None):
    """The sweep with host dummies for every device pointer: a call that gets past validation would touch them."""
    lib = _native.lib()
    c = call or _call()
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
    return rc


# ---- 1. the flag and the validation order ------------------------------------------------------------------------------------------
def test_the_flag_and_its_exports():
    assert MOMENTS == 8
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    assert "#define RYDIFF_TANGENT_MOMENTS 8" in header
    assert "OccupationSensitivities" in P.__all__ and P.OccupationSensitivities is OccupationSensitivities


def test_a_valid_call_with_the_flag_stops_at_the_workspace_test():
    for flags in (MOMENTS, MOMENTS | _native.TANGENT_RDMS, KET_FLAGS):
        with pytest.raises(MemoryError, match="tangent workspace too small"):
            _native.check(_forward(flags=flags))
        with pytest.raises(MemoryError, match="geometry workspace too small"):
            _native.check(_forward(flags=flags, geometry=True))
    with pytest.raises(MemoryError, match="tangent workspace too small"):  # with pair terms (XY kets)
        _native.check(_forward(_with_pair, flags=MOMENTS | _native.TANGENT_PAIR_TERMS))


def test_without_the_flag_the_refusal_names_it():
    for flags in (0, _native.TANGENT_RDMS | _native.TANGENT_PAIR_TERMS):
        for geometry in (False, True):
            rc = _forward(flags=flags, geometry=geometry)
            assert rc == _native.RYDIFF_ENOTIMPL
            with pytest.raises(NotImplementedError, match="tangent sweep: bit moments are not implemented.*unless RydTangent.flags has "
                                                          "RYDIFF_TANGENT_MOMENTS"):
                _native.check(rc)


def test_unknown_flag_bits_are_invalid():
    for flags in (16, KET_FLAGS | 16, MOMENTS | 32):
        rc = _forward(flags=flags)
        assert rc == _native.RYDIFF_EINVAL
        with pytest.raises(ValueError, match="flags"):
            _native.check(rc)


def test_the_flag_on_a_problem_without_moments_is_invalid():
    """Bit 8 was the first unknown bit before the flag existed; on a problem without bit moments it keeps that answer."""
    for flags in (MOMENTS, KET_FLAGS):
        for geometry in (False, True):
            rc = _forward(flags=flags, geometry=geometry, call=_call(moments=False))
            assert rc == _native.RYDIFF_EINVAL
            with pytest.raises(ValueError, match="flags: RYDIFF_TANGENT_MOMENTS"):
                _native.check(rc)


def test_what_the_sweep_does_not_take_stays_refused_with_the_flag():
    def doubled(p):
        p.n_qubits, p.dm_atoms = 4, 2

    every = KET_FLAGS | _native.TANGENT_DENSITY_MATRIX
    for mutate, word, flags in ((doubled, "dm_atoms", MOMENTS), (doubled, "bit moments", every),
                                (lambda p: setattr(p, "shard_bits", 1), "shard", MOMENTS),
                                (lambda p: setattr(p, "n_shots", 4), "shots", MOMENTS),
                                (lambda p: setattr(p, "amp_conditioned_terms", 1), "conditioned", MOMENTS),
                                (lambda p: setattr(p, "det_ones_terms", 1), "ones-counting", MOMENTS),
                                (_with_pair, "RYDIFF_TANGENT_PAIR_TERMS", MOMENTS)):
        rc = _forward(mutate, flags=flags)
        assert rc == _native.RYDIFF_ENOTIMPL, (word, rc, _native.last_error())
        with pytest.raises(NotImplementedError, match=word):
            _native.check(rc)


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("n_dir", [1, 3, 5, 8])
def test_workspace_at_13_qubits_holds_the_tile_records_of_the_real_directions(n_dir):
    """include/rydiff.h: beyond 12 qubits the forward plan holds B * 79 * 2^(N-12) doubles for the values' tile records and the
    tangent layout n_dir * B * 79 * 2^(N-12) doubles for the tangents' — n_dir, not the padded count — each rounded up to 256
    bytes; everything else is the size of the same problem without moments."""
    lib, info = _native.lib(), _info()
    with_m, without = _call(13), _call(13, moments=False)
    tiles = 2
    extra = _align(B * 79 * tiles * 8) + _align(n_dir * B * 79 * tiles * 8)
    for size_of in (lib.rydiff_tangent_workspace_bytes_flags, lib.rydiff_geometry_workspace_bytes_flags):
        plain = size_of(ctypes.byref(without.problem), ctypes.byref(info), n_dir, 0)
        got = size_of(ctypes.byref(with_m.problem), ctypes.byref(info), n_dir, MOMENTS)
        assert plain > 0 and got > 0, _native.last_error()
        assert got >= plain and got - plain == extra
        assert size_of(ctypes.byref(without.problem), ctypes.byref(info), n_dir, MOMENTS) == 0  # the flag without the block: invalid
        assert "RYDIFF_TANGENT_MOMENTS" in _native.last_error()
        assert size_of(ctypes.byref(with_m.problem), ctypes.byref(info), n_dir, 0) == 0  # refused without it


def test_the_python_entry_points_refuse_without_the_flag_and_density_matrices_with_it():
    spec = ProblemSpec(3, 0.004, 5, (7,), (7,), moments=True)
    z = torch.zeros(1)
    for fn in (S.evolve_tangent, S.evolve_geometry):
        for flags in (0, _native.TANGENT_RDMS):
            with pytest.raises(NotImplementedError, match="occupation correlations.*TANGENT_MOMENTS"):
                fn(z, z, z, z, z, spec, d_det=z, flags=flags)


# ---- 2. the tangent helpers of utils against torch.func.jvp -------------------------------------------------------------------------
def _moments_and_direction(n, seed, lead=()):
    """Seeded positive rows (rows, 3, 2) (values of order one, S the largest) and a direction (rows, *lead, 3, 2)."""
    gen = torch.Generator().manual_seed(seed)
    rows = moment_rows(n)
    m = torch.rand(rows, 3, 2, generator=gen, dtype=torch.float64) + 0.1
    m[0] += 1.0
    return m, torch.randn(rows, *lead, 3, 2, generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("occupied_bit", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_tangent_helpers_match_jvp(n, occupied_bit):
    m, dm = _moments_and_direction(n, 40 + n)
    signs = [(-1.0) ** i for i in range(n)]
    jvp = lambda f: torch.func.jvp(f, (m,), (dm,))[1]  # noqa: E731
    cases = {
        "occupations": (jvp(lambda r: utils.occupations_from_moments(r, n, occupied_bit)), utils.occupations_from_moments(dm, n, occupied_bit)),
        "correlations": (jvp(lambda r: utils.occupation_correlations_from_moments(r, n, occupied_bit)),
                         utils.occupation_correlations_from_moments(dm, n, occupied_bit)),
        "connected": (jvp(lambda r: utils.connected_correlations(r, n, occupied_bit)), utils.connected_correlations_tangent(m, dm, n, occupied_bit)),
        "structure factor": (jvp(lambda r: utils.structure_factor(utils.connected_correlations(r, n, occupied_bit), signs)),
                             utils.structure_factor_tangent(m, dm, n, signs, occupied_bit)),
    }
    for name, (want, got) in cases.items():
        assert tuple(got.shape) == tuple(want.shape), name
        scale = float(want.abs().max())
        assert scale > 1e-2, name
        assert float((got - want).abs().max()) <= 1e-12 * scale, name
    # the structure factor is linear in g: on the tangent of g as it is
    dg = utils.connected_correlations_tangent(m, dm, n, occupied_bit)
    assert torch.equal(utils.structure_factor(dg, signs), cases["structure factor"][1])


def test_tangent_helpers_take_leading_direction_axes():
    n = 4
    m, dm = _moments_and_direction(n, 77, lead=(3,))
    got = utils.connected_correlations_tangent(m, dm, n, 0)
    assert tuple(got.shape) == (3, 3, 2, n, n)
    for d in range(3):
        assert torch.equal(got[d], utils.connected_correlations_tangent(m, dm[:, d], n, 0))
    assert tuple(utils.structure_factor_tangent(m, dm, n, [1, -1, 1, -1], 1).shape) == (3, 3, 2)


def test_the_dataclass_reshapes_per_tensor_of_the_request():
    """moments (rows, n_t, B); dmoments[i] (rows, n_t, B, *x_i.shape): the accessors return (n_t, B, ..., *x_i.shape)."""
    n = 3
    m, _ = _moments_and_direction(n, 5)
    gen = torch.Generator().manual_seed(6)
    dms = [torch.randn(moment_rows(n), 3, 2, 2, 2, generator=gen, dtype=torch.float64), torch.randn(moment_rows(n), 3, 2, 1, generator=gen, dtype=torch.float64)]
    sens = OccupationSensitivities(m, dms, torch.linspace(0, 1, 3, dtype=torch.float64), 0)
    assert sens.n_qubits == n
    assert tuple(sens.occupations().shape) == (3, 2, n) and tuple(sens.correlations().shape) == (3, 2, n, n)
    assert tuple(sens.structure_factor([1, -1, 1]).shape) == (3, 2)
    assert [tuple(t.shape) for t in sens.d_occupations()] == [(3, 2, n, 2, 2), (3, 2, n, 1)]
    assert [tuple(t.shape) for t in sens.d_correlations(connected=True)] == [(3, 2, n, n, 2, 2), (3, 2, n, n, 1)]
    assert [tuple(t.shape) for t in sens.d_structure_factor([1, -1, 1])] == [(3, 2, 2, 2), (3, 2, 1)]
    want = utils.connected_correlations_tangent(m, dms[0][..., 1, 0], n, 0)
    assert torch.equal(sens.d_correlations(connected=True)[0][..., 1, 0], want)
    assert torch.equal(sens.d_correlations()[1][..., 0], utils.occupation_correlations_from_moments(dms[1][..., 0], n, 0))
    rest, mom = split_moments(torch.cat([torch.zeros(2, 3, 2, dtype=torch.float64), m]), n)  # off each dexpect[d] like off expect
    assert torch.equal(mom, m) and rest.shape[0] == 2


# ---- 3. public refusals --------------------------------------------------------------------------------------------------------------
def test_run_occupation_sensitivities_refusals():
    prm = _params()
    args = (prm["q0"], prm["omega"], prm["area"], prm["phase"])
    emu = _basic_usage_emulator(*args)
    with pytest.raises(ValueError, match="deriv_time"):
        emu.run_occupation_sensitivities([prm["omega"], emu.evaluation_times])
    with pytest.raises(TypeError):
        deriv_occupations_all_times(emu, [])
    with pytest.raises(NotImplementedError, match="run_occupation_sensitivities.*master-equation"):
        emu.run_occupation_sensitivities([prm["omega"]], solver=P.SolverType.DP5_ME)
    dephasing = _basic_usage_emulator(*args, config=P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="run_occupation_sensitivities.*master-equation"):
        deriv_occupations_all_times(dephasing, [prm["omega"]])
    doppler = _basic_usage_emulator(*args, config=P.SimConfig(noise="doppler", runs=2, temperature=50.0))
    with pytest.raises(NotImplementedError, match="run_occupation_sensitivities.*average"):
        doppler.run_occupation_sensitivities([prm["omega"]])
    three, _ = _three_level_emulator()
    leaf = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="run_occupation_sensitivities.*three-level"):
        three.run_occupation_sensitivities([leaf])


def test_the_other_all_times_methods_keep_refusing_and_point_at_the_new_one():
    prm = _params()
    emu = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"])
    obs = OccupationCorrelations()
    for call in (lambda: emu.run_sensitivities([prm["omega"]], [obs]), lambda: emu.run_rdm_sensitivities([prm["omega"]], [obs]),
                 lambda: emu.run_quantum_fisher([prm["omega"]], [obs])):
        with pytest.raises(NotImplementedError, match="OccupationCorrelations.*run_occupation_sensitivities"):
            call()
