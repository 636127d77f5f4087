"""Energy observables, host side (no GPU): the struct handshake, the C ABI's refusals (every one before anything touches a
device), the row layout, Hamiltonian.energy_tables against _interp entry by entry and under autograd, and the Python refusals."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native, pulses as pl, utils
from pulser_diff_amd import solver as S
from pulser_diff_amd.observables import Energy, OccupationCorrelations, ReducedDensityMatrix, moment_rows
from pulser_diff_amd.simconfig import SimConfig
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, split_energy, split_ket_tail, split_moments, split_observables
from tests.test_dm_tangent_host import _with_pair
from tests.test_host_logic import _three_level_emulator
from tests.test_tangent_host import _basic_usage_emulator, _info, _params
from tests.test_xy_exchange_host import emulator as xy_emulator, grid

B, N_T = 2, 3


def _call(n=3, energy=2, **kw):
    """A _Call on n qubits, B = 2.  HOST tensors: the validation never follows the device pointers."""
    spec = ProblemSpec(n, 0.004, 5, (2 ** n - 1,), (2 ** n - 1,), solver=SolverType.DP5_SE, energy=energy, **kw)
    ea = torch.zeros(1, 1, N_T, dtype=torch.complex128) if energy else None
    ed = torch.zeros(1, 1, N_T, dtype=torch.float64) if energy else None
    return _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(n * (n - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, N_T), B, None, energy_amp=ea, energy_det=ed,
                 xy_pairs=torch.zeros(n * (n - 1) // 2, dtype=torch.float64) if kw.get("xy_mode") else None)


def _plan(call, mutate=None):
    """rydiff_plan with a host scratch: a problem that is refused never reaches the one kernel of the call."""
    if mutate:
        mutate(call.problem)
    scratch = ctypes.create_string_buffer(_native.PLAN_SCRATCH_BYTES)
    return _native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.cast(scratch, ctypes.c_void_p), None,
                                    ctypes.byref(_native.RydPlanInfo()))


# ---- 1. the struct and the header ---------------------------------------------------------------------------------------------------
def test_struct_sizes_agree_and_the_fields_sit_in_front_of_the_exchange_block():
    L = _native.lib()  # (raises on a size mismatch)
    assert L.rydiff_sizeof_problem() == ctypes.sizeof(_native.RydProblem)
    names = [f[0] for f in _native.RydProblem._fields_]
    i = names.index("energy_rows")
    assert names[i:i + 6] == ["energy_rows", "energy_amp", "energy_det", "g_energy_amp", "g_energy_det", "energy_kernel"]
    assert names[i - 1] == "det_ones_terms" and names[i + 6] == "xy_mode" and names[-1] == "pauli_w"
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    order = [header.index(f" {f};") for f in ("det_ones_terms", "energy_rows", "g_energy_det", "xy_mode")]
    assert order == sorted(order)
    assert "Energy" in P.__all__ and P.Energy is Energy


def test_the_call_carries_the_block():
    p = _call().problem
    assert p.energy_rows == 2 and p.energy_amp and p.energy_det and not p.g_energy_amp and not p.g_energy_det
    off = _call(energy=0).problem
    assert off.energy_rows == 0 and not off.energy_amp and not off.energy_det


# ---- 2. refusals of the C ABI ------------------------------------------------------------------------------------------------------
def test_invalid_values_are_refused():
    for bad in (-1, 3):
        rc = _plan(_call(), lambda p: setattr(p, "energy_rows", bad))
        assert rc == _native.RYDIFF_EINVAL and "energy_rows" in _native.last_error()
    for bad in (-1, 3):
        rc = _plan(_call(), lambda p: setattr(p, "energy_kernel", bad))
        assert rc == _native.RYDIFF_EINVAL and "energy_kernel" in _native.last_error()
    rc = _plan(_call(), lambda p: setattr(p, "energy_kernel", 2))  # (3 qubits: the tile version starts at 13)
    assert rc == _native.RYDIFF_ENOTIMPL and "energy_kernel = 2" in _native.last_error()
    assert _plan(_call(energy=0), lambda p: setattr(p, "energy_kernel", 7)) != _native.RYDIFF_EINVAL  # ignored with the block off
    assert _call(energy_kernel=1).problem.energy_kernel == 1 and _call(energy=0, energy_kernel=1).problem.energy_kernel == 0
    for field in ("energy_amp", "energy_det"):
        rc = _plan(_call(), lambda p: setattr(p, field, None))
        assert rc == _native.RYDIFF_EINVAL and "energy_amp / energy_det" in _native.last_error()
    # a table is asked for only where the problem has such terms
    spec = ProblemSpec(3, 0.004, 5, (7,), (), solver=SolverType.KRYLOV_SE, energy=1)
    call = _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 0, 5, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                 np.linspace(0, 0.008, N_T), 1, None, energy_amp=torch.zeros(1, 1, N_T, dtype=torch.complex128))
    assert not call.problem.energy_det
    assert _plan(call, lambda p: setattr(p, "n_pair_terms", -1)) == _native.RYDIFF_EINVAL and "pair terms" in _native.last_error()  # (got past the block)


def _sharded(p):
    p.shard_bits, p.batch = 1, 2


def _density(p):
    p.dm_atoms, p.n_qubits = 1, 2


NOTIMPL = {"pair terms": (_with_pair, "dense pair terms"), "density matrix": (_density, "density-matrix registers"),
           "sharding": (_sharded, "state sharding"),
           "conditioned": (lambda p: setattr(p, "amp_conditioned_terms", 1), "conditioned flips"),
           "ones-counting": (lambda p: setattr(p, "det_ones_terms", 1), "conditioned flips / ones-counting"),
           "one-directional exchange": (lambda p: setattr(p, "xy_mode", 2), "xy_mode = 2")}


@pytest.mark.parametrize("name", sorted(NOTIMPL))
def test_combinations_that_are_not_implemented_are_refused_by_name(name):
    mutate, words = NOTIMPL[name]
    n = 2 if name in ("conditioned", "ones-counting", "density matrix") else 3
    call = _call(n, xy_mode=1) if name == "one-directional exchange" else _call(n)
    rc = _plan(call, mutate)
    assert rc == _native.RYDIFF_ENOTIMPL, _native.last_error()
    assert "energy observables (energy_rows > 0): not implemented together with" in _native.last_error() and words in _native.last_error()
    with pytest.raises(NotImplementedError):
        _native.check(rc)
    # the same problem with the block off is not refused for it
    off = _call(n, energy=0, xy_mode=1) if name == "one-directional exchange" else _call(n, energy=0)
    rc = _plan(off, mutate)
    assert "energy" not in (_native.last_error() if rc else "")


def test_the_hermitian_exchange_is_taken():
    """(refused only by what comes after the validation: the plan's one kernel — here the host scratch is enough to see it pass
    build_plan: with a NULL stream and no device the launch fails with a HIP error, never with a refusal)"""
    rc = _plan(_call(3, xy_mode=1))
    assert rc in (_native.RYDIFF_OK, _native.RYDIFF_EHIP), _native.last_error()


@pytest.mark.parametrize("sweep", ["tangent", "geometry", "fisher"])
def test_the_tangent_sweeps_refuse_the_block(sweep):
    lib = _native.lib()
    c = _call()
    tg = _native.RydTangent()
    tg.n_dir, tg.d_amp, tg.flags = 2, 0x1000, 0
    info = _info()
    vp = ctypes.c_void_p
    if sweep == "tangent":
        rc = lib.rydiff_forward_tangent(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), vp(0x1000), None, vp(0x1000), vp(0x1000), 0, None)
    elif sweep == "geometry":
        rc = lib.rydiff_forward_geometry(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), vp(0x1000), None, vp(0x1000), vp(0x1000),
                                         vp(0x1000), 0, None)
    else:
        rc = lib.rydiff_forward_fisher(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), vp(0x1000), None, vp(0x1000), vp(0x1000),
                                       vp(0x1000), vp(0x1000), 0, None)
    assert rc == _native.RYDIFF_ENOTIMPL
    assert "tangent sweep: energy observables are not implemented" in _native.last_error()
    assert lib.rydiff_tangent_workspace_bytes(ctypes.byref(c.problem), ctypes.byref(info), 2) == 0


# ---- 3. the row layout --------------------------------------------------------------------------------------------------------------
def test_expect_rows_and_the_splitters_place_the_block_behind_the_moments():
    n = 3
    assert _call(n, energy=0).expect_rows() == 0 and _call(n, energy=1).expect_rows() == 1 and _call(n, energy=2).expect_rows() == 2
    rdms = [ReducedDensityMatrix([0]), ReducedDensityMatrix([1, 2])]
    full = _call(n, energy=2, moments=True, rdms=rdms).expect_rows()
    assert full == 8 + 32 + moment_rows(n) + 2
    assert _call(n, energy=0, moments=True, rdms=rdms).expect_rows() == full - 2
    expect = torch.arange(full * N_T * B, dtype=torch.float64).reshape(full, N_T, B)
    rest, en = split_energy(expect, 2)
    assert torch.equal(en, expect[-2:]) and rest.shape[0] == full - 2
    rest, mom = split_moments(rest, n)
    assert torch.equal(mom, expect[-2 - moment_rows(n):-2])
    one = split_ket_tail(expect, n, moments=True, energy=2)  # the one splitter of both tail blocks
    assert torch.equal(one[0], rest) and torch.equal(one[1], mom) and torch.equal(one[2], en)
    assert split_ket_tail(rest, n)[0] is rest and split_ket_tail(rest, n)[1:] == (None, None)
    real, ov, mats = split_observables(rest, 0, rdms)
    assert real.shape[0] == 0 and ov is None and [tuple(m.shape) for m in mats] == [(N_T, B, 2, 2), (N_T, B, 4, 4)]
    # energy = 0: exactly what they returned before the block existed
    same, none = split_energy(expect, 0)
    assert same is expect and none is None
    plain = expect[:8 + 32]
    a, b = split_observables(plain, 0, rdms), split_observables(plain, 0, rdms, energy=0)
    assert len(a) == len(b) == 3 and torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    # energy > 0 without moments: split_observables takes the rows off itself and returns them fourth
    with_e = torch.cat([plain, expect[-2:]])
    c = split_observables(with_e, 0, rdms, energy=2)
    assert len(c) == 4 and torch.equal(c[3], expect[-2:]) and all(torch.equal(x, y) for x, y in zip(a[2], c[2]))
    with pytest.raises(ValueError, match="split_energy"):
        split_energy(expect[:1], 2)


def test_python_side_shape_checks():
    n = 3
    spec = ProblemSpec(n, 0.004, 5, (7,), (7,), energy=1)
    amp, det, u = torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    ea, ed = torch.zeros(1, 1, N_T, dtype=torch.complex128), torch.zeros(1, 1, N_T, dtype=torch.float64)
    S._check_shapes(spec, amp, det, u, None, 1, energy_amp=ea, energy_det=ed, n_t=N_T)
    with pytest.raises(ValueError, match="needs energy_amp"):
        S._check_shapes(spec, amp, det, u, None, 1, energy_det=ed, n_t=N_T)
    with pytest.raises(ValueError, match=r"energy_det must have shape \(1, 1, 3\)"):
        S._check_shapes(spec, amp, det, u, None, 1, energy_amp=ea, energy_det=torch.zeros(1, 1, 5, dtype=torch.float64), n_t=N_T)
    with pytest.raises(ValueError, match="without ProblemSpec.energy"):
        S._check_shapes(ProblemSpec(n, 0.004, 5, (7,), (7,)), amp, det, u, None, 1, energy_amp=ea, n_t=N_T)
    with pytest.raises(ValueError, match="ProblemSpec.energy must be 0"):
        S._check_shapes(ProblemSpec(n, 0.004, 5, (7,), (7,), energy=3), amp, det, u, None, 1, energy_amp=ea, energy_det=ed, n_t=N_T)


# ---- 4. Hamiltonian.energy_tables ---------------------------------------------------------------------------------------------------
def _emu(shift=None):
    prm = _params(shift)
    return _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"]), prm


def test_energy_tables_equal_interp_entry_by_entry():
    """An irregular grid with points on the sample grid, between samples, in the clamped last interval and at the end of the run."""
    emu, _ = _emu()
    ham = emu._hamiltonian
    n, dt = ham.n_samples, ham.dt
    ts = torch.tensor([0.0, 0.3 * dt, dt, 2.5 * dt, 17.25 * dt, (n - 2) * dt, (n - 1.5) * dt, (n - 1) * dt, (n - 0.1) * dt], dtype=torch.float64)
    e_amp, e_det = ham.energy_tables(ts)
    assert tuple(e_amp.shape) == (1, ham.amp_tables.shape[1], len(ts)) and tuple(e_det.shape) == (1, ham.det_tables.shape[1], len(ts))
    assert e_amp.dtype == torch.complex128 and e_det.dtype == torch.float64
    for k, t in enumerate(ts):
        for j, (coeff, _) in enumerate(ham._amp_terms):
            assert e_amp[0, j, k] == ham._interp(coeff, t), (j, k)
        for j, (coeff, _) in enumerate(ham._det_terms):
            assert e_det[0, j, k] == ham._interp(coeff, t), (j, k)
    assert float(e_amp.detach().abs().max()) > 0 and float(e_det.detach().abs().max()) > 0
    # the frame tables (one constant phase that carries no gradient): the real 0.5 * amp, interpolated by the same rule
    prm = _params()
    fham = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], 0.4)._hamiltonian
    assert fham.amp_tables_frame is not None
    f_amp, _ = fham.energy_tables(ts, frame=True)
    l_amp, _ = fham.energy_tables(ts)
    assert not f_amp.is_complex() and float(l_amp.detach().imag.abs().max()) > 0
    assert torch.allclose(f_amp.detach(), l_amp.detach().abs(), rtol=1e-13, atol=1e-15)


def test_autograd_through_energy_tables_matches_finite_differences_of_interp():
    """d/d(pulse parameters) and d/d(evaluation times) of sum w * tables against central differences of _interp (h = 1e-6, 1e-7
    relative to the largest finite-difference entry, as tests/test_tangent_host.py does for the table tangents)."""
    ts0 = [0.013, 0.207, 0.5551, 1.1003, 1.5902]
    gen = torch.Generator().manual_seed(5)

    def value(emu, ts, w):
        ham = emu._hamiltonian
        tot = 0.0
        for k, t in enumerate(ts):
            for j, (coeff, _) in enumerate(ham._amp_terms):
                c = ham._interp(coeff, t)
                tot = tot + w[0][j, k] * c.real + w[1][j, k] * c.imag
            for j, (coeff, _) in enumerate(ham._det_terms):
                tot = tot + w[2][j, k] * ham._interp(coeff, t)
        return tot

    emu, prm = _emu()
    ham = emu._hamiltonian
    ka, kd = ham.amp_tables.shape[1], ham.det_tables.shape[1]
    w = [torch.randn(ka, len(ts0), generator=gen, dtype=torch.float64) for _ in range(2)] + [torch.randn(kd, len(ts0), generator=gen, dtype=torch.float64)]
    ts = torch.tensor(ts0, dtype=torch.float64, requires_grad=True)
    e_amp, e_det = ham.energy_tables(ts)
    loss = (w[0] * e_amp[0].real).sum() + (w[1] * e_amp[0].imag).sum() + (w[2] * e_det[0]).sum()
    leaves = [prm["omega"], prm["area"], prm["phase"], ts]
    got = torch.autograd.grad(loss, leaves)
    h = 1e-6
    for name, g in zip(("omega", "area", "phase"), got[:3]):
        fd = (float(value(_emu((name, 0, h))[0], [torch.tensor(t, dtype=torch.float64) for t in ts0], w).detach())
              - float(value(_emu((name, 0, -h))[0], [torch.tensor(t, dtype=torch.float64) for t in ts0], w).detach())) / (2 * h)
        assert abs(fd) > 1e-3 and abs(float(g) - fd) <= 1e-7 * abs(fd), (name, float(g), fd)
    fd_t = []
    for k in range(len(ts0)):
        vals = []
        for s in (h, -h):
            tt = [torch.tensor(t + (s if i == k else 0.0), dtype=torch.float64) for i, t in enumerate(ts0)]
            vals.append(float(value(emu, tt, w).detach()))
        fd_t.append((vals[0] - vals[1]) / (2 * h))
    fd_t = torch.tensor(fd_t, dtype=torch.float64)
    assert float(fd_t.abs().max()) > 1e-3  # (the ramp's slope is not zero)
    assert float((got[3] - fd_t).abs().max()) <= 1e-7 * float(fd_t.abs().max())


# ---- 5. the public objects and their refusals ---------------------------------------------------------------------------------------
def test_energy_object_and_variance_helper():
    assert Energy().rows == 2 and Energy(second_moment=False).rows == 1
    e = torch.tensor([1.0, 2.0, -3.0], dtype=torch.float64, requires_grad=True)
    m2 = torch.tensor([1.5, 4.0 - 1e-13, 9.5], dtype=torch.float64, requires_grad=True)
    var = utils.energy_variance(e, m2)
    assert var.tolist() == [0.5, 0.0, 0.5]  # clamped at 0 in the value ...
    g_e, g_m = torch.autograd.grad(var.sum(), [e, m2])
    assert g_m.tolist() == [1.0, 1.0, 1.0] and g_e.tolist() == [-2.0, -4.0, 6.0]  # ... and only there
    assert "1e-12 R^2" in utils.energy_variance.__doc__


def test_results_fall_back_to_stored_states_and_say_what_is_missing():
    from pulser_diff_amd.simresults import CoherentResults

    emu, _ = _emu()
    ham = emu._hamiltonian
    n_t, dim = 3, 16
    gen = torch.Generator().manual_seed(3)
    states = torch.randn(n_t, 1, dim, generator=gen, dtype=torch.complex128)
    states = states / states.norm(dim=2, keepdim=True)
    times = torch.tensor([0.1, 0.7, 1.3], dtype=torch.float64)
    res = CoherentResults(states, 4, "ground-rydberg", times, "ground-rydberg", hamiltonian_at=ham._hamiltonian)
    e, m2 = res.energy().detach(), res.energy_second_moment().detach()
    for k in range(n_t):
        h = emu.get_hamiltonian(float(times[k]) * 1000).to_dense().detach() @ states[k, 0]
        assert abs(float(e[k]) - float((states[k, 0].conj() * h).sum().real)) < 1e-12 * float(m2[k]) ** 0.5
        assert abs(float(m2[k]) - float((h.conj() * h).sum().real)) < 1e-12 * float(m2[k])
    assert float((res.energy_variance() - (m2 - e ** 2)).detach().abs().max()) == 0.0 and float((m2 - e ** 2).min()) > 0
    native = torch.arange(6, dtype=torch.float64).reshape(1, n_t, 2)
    only_e = CoherentResults(torch.empty(0, 2, dim, dtype=torch.complex128), 4, "ground-rydberg", times, "ground-rydberg", native_energy=native)
    assert only_e.energy().tolist() == [1.0, 5.0, 9.0]
    with pytest.raises(RuntimeError, match="no native energy rows with the second moment"):
        only_e.energy_second_moment()
    with pytest.raises(RuntimeError, match=r"hand run\(observables=\[Energy\(\)\]\)"):
        CoherentResults(torch.empty(0, 2, dim, dtype=torch.complex128), 4, "ground-rydberg", times, "ground-rydberg").energy()


def test_python_refusals_fire():
    emu3, _ = _three_level_emulator()
    with pytest.raises(NotImplementedError, match="Energy is not available in the three-level all-basis"):
        emu3.run(observables=[Energy()], solver=SolverType.KRYLOV_SE)
    emu, _ = _emu()
    with pytest.raises(NotImplementedError, match="Energy is not available in master-equation runs"):
        emu.run(observables=[Energy()], solver=SolverType.DP5_ME)
    prm = _params()
    noisy = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"], config=SimConfig(noise="SPAM", eta=0.4, runs=3))
    with pytest.raises(NotImplementedError, match="Energy stays refused in noisy runs that average over realisations"):
        noisy.run(observables=[Energy()], solver=SolverType.KRYLOV_SE)
    collapse = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"], config=SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="Energy is not available in master-equation runs"):
        collapse.run(observables=[Energy()], solver=SolverType.KRYLOV_SE)
    for kw in (dict(), dict(xy_hermitian=True), dict(xy_native=True)):  # dense route / dense Hermitian / native but one-directional
        with pytest.raises(NotImplementedError, match="xy_native=True, xy_hermitian=True"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (the one-directional exchange warns once per process)
                xy_emulator(grid(4), **kw).run(observables=[Energy()], solver=SolverType.KRYLOV_SE)
    with pytest.raises(TypeError, match="OccupationCorrelations / Energy objects"):
        emu.run(observables=["energy"], solver=SolverType.KRYLOV_SE)

