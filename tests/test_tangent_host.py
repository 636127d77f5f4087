"""Forward-mode (tangent) sweep, host side (no GPU): the table tangents the public route feeds the sweep, the C ABI's argument
validation (every refusal happens before anything touches a device), the ctypes mirror, and the Python-side refusals."""
import ctypes
import re

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native, pulses as pl
from pulser_diff_amd.derivative import deriv_param_all_times
from oracle import restatement as R
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call
from tests.helpers import (DP5_DEFAULT_H_MAX, magnus_cf4_dense, map_exponentials, random_terms, shifted_terms, tangent_dense_reference,
                           tangent_rows_reference)


def _basic_usage_emulator(q0, omega, area, phase, config=None):
    """The sequence of examples/basic_usage.py (4 atoms, Blackman + constant pulse) with float64 parameters and a drive phase."""
    reg = pl.Register({"q0": q0, "q1": torch.tensor([0.0, 8.0], dtype=torch.float64), "q2": torch.tensor([8.0, 0.0], dtype=torch.float64),
                       "q3": torch.tensor([8.0, 8.0], dtype=torch.float64)})
    seq = pl.Sequence(reg, pl.MockDevice)
    seq.declare_channel("rydberg_global", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(800, area), pl.RampWaveform(800, -5.0, 0.0), phase), "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(800, omega, 0.0, phase), "rydberg_global")
    return P.TorchEmulator.from_sequence(seq, sampling_rate=0.1, config=config, compute_device="cpu")


_P0 = {"q0": [0.3, -0.2], "omega": [5.0], "area": [torch.pi], "phase": [0.4]}


def _params(shift=None):
    vals = {k: torch.tensor(v, dtype=torch.float64) for k, v in _P0.items()}
    if shift is not None:
        name, idx, h = shift
        vals[name][idx] += h
    return {k: v.requires_grad_(True) for k, v in vals.items()}


def _tables(emu):
    ham = emu._hamiltonian
    return ham.amp_tables.detach(), ham.det_tables.detach(), ham.u_pairs.detach()


def test_table_tangents_match_central_differences():
    """The double-backward table tangents against central differences (h = 1e-6, float64 parameters, 1e-7 relative to the largest
    entry of the finite-difference tangent): one coordinate, the amplitude, the area and a phase."""
    prm = _params()
    emu = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"])
    x = [prm["q0"], prm["omega"], prm["area"], prm["phase"]]
    d_amp, d_det, d_u = emu._table_tangents(x)
    assert d_amp.shape == (5,) + tuple(emu._hamiltonian.amp_tables.shape) and d_amp.dtype == torch.complex128
    assert d_u.shape == (5, 6)
    assert d_det is None  # the detuning ramp carries no parameter: skipped, not differentiated
    h = 1e-6
    seen = 0
    for d, (name, idx) in enumerate([("q0", 0), ("q0", 1), ("omega", 0), ("area", 0), ("phase", 0)]):
        tabs = []
        for sign in (+1, -1):
            q = _params((name, idx, sign * h))
            tabs.append(_tables(_basic_usage_emulator(q["q0"], q["omega"], q["area"], q["phase"])))
        fd_amp = (tabs[0][0] - tabs[1][0]) / (2 * h)
        fd_u = (tabs[0][2] - tabs[1][2]) / (2 * h)
        for got, fd in ((d_amp[d], fd_amp), (d_u[d], fd_u)):
            scale = float(fd.abs().max())
            err = float((got - fd).abs().max())
            print(f"{name}[{idx}]: max |fd| = {scale:.3e}, max |tangent - fd| = {err:.3e}")
            if scale == 0.0:
                assert float(got.abs().max()) == 0.0
            else:
                assert err <= 1e-7 * scale
                seen += 1
    assert seen == 5  # coordinates reach U, the three pulse parameters reach the amplitude table: none passed on zeros


def _spec(n=3):
    return ProblemSpec(n, 0.004, 5, (2**n - 1,), (2**n - 1,), solver=SolverType.KRYLOV_SE)


def _call(n=3, batch=2):
    amp = torch.zeros(1, 1, 5, dtype=torch.complex128)
    det = torch.zeros(1, 1, 5, dtype=torch.float64)
    u = torch.zeros(n * (n - 1) // 2, dtype=torch.float64)
    return _Call(_spec(n), amp, det, u, np.linspace(0, 0.016, 3), batch, None)


def _info():
    info = _native.RydPlanInfo()  # what rydiff_plan would report for the all-zero tables (no device here)
    info.spectral_lo, info.spectral_hi, info.flags = -1.0, 1.0, 0
    return info


def _tangent_call(mutate_problem=None, mutate_tangent=None, dexpect=0x1000, info=True):
    """rydiff_forward_tangent with host dummies for every device pointer: a call that gets past validation would touch them."""
    call = _call()
    tg = _native.RydTangent()
    tg.n_dir = 2
    tg.d_amp = 0x1000
    if mutate_problem:
        mutate_problem(call.problem)
    if mutate_tangent:
        mutate_tangent(tg)
    plan = _info()
    rc = _native.lib().rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(plan) if info else None, ctypes.byref(tg),
                                              ctypes.c_void_p(0x1000), None, ctypes.c_void_p(dexpect) if dexpect else None,
                                              ctypes.c_void_p(0x1000), 0, None)
    _native.check(rc)


def test_forward_tangent_validates_before_touching_a_device():
    for n_dir in (0, -1, _native.MAX_TANGENTS + 1):
        with pytest.raises(ValueError, match="n_dir"):
            _tangent_call(mutate_tangent=lambda t, n=n_dir: setattr(t, "n_dir", n))
    with pytest.raises(ValueError, match="d_amp, d_det, d_u, d_psi0 are NULL"):
        _tangent_call(mutate_tangent=lambda t: setattr(t, "d_amp", None))
    with pytest.raises(ValueError, match="dexpect_out"):
        _tangent_call(dexpect=0)
    with pytest.raises(ValueError, match="info"):
        _tangent_call(info=False)
    with pytest.raises(NotImplementedError, match="shard"):
        _tangent_call(lambda p: setattr(p, "shard_bits", 1))
    pair_q = np.array([[0, 1]], dtype=np.uint32)
    pair_t = np.zeros((1, 16), dtype=np.complex128)

    def with_pair(p):
        p.n_pair_terms, p.pair_qubits, p.pair_tables = 1, pair_q.ctypes.data, pair_t.ctypes.data

    with pytest.raises(NotImplementedError, match="pair terms"):
        _tangent_call(with_pair)
    with pytest.raises(NotImplementedError, match="conditioned"):
        _tangent_call(lambda p: setattr(p, "amp_conditioned_terms", 1))
    with pytest.raises(NotImplementedError, match="ones-counting"):
        _tangent_call(lambda p: setattr(p, "det_ones_terms", 1))
    # a call that passes every check is stopped by the (host-side) workspace test: still nothing launched
    with pytest.raises(MemoryError, match="tangent workspace too small"):
        _tangent_call()


def test_tangent_workspace_bytes_is_host_only_and_grows_with_the_directions():
    L = _native.lib()
    call, plan = _call(), _info()
    sizes = [L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), d) for d in (1, 2, 8)]
    state_bytes = 2 * 8 * 16  # B * 2^N * sizeof(complex128)
    assert sizes[0] > 0 and sizes[1] - sizes[0] >= 2 * state_bytes and sizes[2] - sizes[1] >= 12 * state_bytes
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), 9) == 0
    assert "n_dir" in _native.last_error()
    call.problem.shard_bits = 1
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), 1) == 0
    assert "not implemented" in _native.last_error()


def test_ctypes_mirror_of_rydtangent_matches_the_header(tmp_path):
    import subprocess
    from pathlib import Path

    header = Path(__file__).resolve().parent.parent / "include" / "rydiff.h"
    assert ctypes.sizeof(_native.RydTangent) == _native.lib().rydiff_sizeof_tangent()
    assert int(re.search(r"#define RYDIFF_MAX_TANGENTS (\d+)", header.read_text()).group(1)) == _native.MAX_TANGENTS
    fields = [f[0] for f in _native.RydTangent._fields_]
    nl = chr(92) + "n"
    src = tmp_path / "layout.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
                              f'printf("%zu{nl}", sizeof(RydTangent));']
                             + [f'printf("%zu{nl}", offsetof(RydTangent, {f}));' for f in fields] + ["return 0;}"]))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_native.RydTangent)
    assert out[1:] == [getattr(_native.RydTangent, f).offset for f in fields]


def test_python_side_refusals():
    prm = _params()
    emu = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"])
    obs = P.DiagonalObservable(torch.ones(16, dtype=torch.float64))
    with pytest.raises(ValueError, match="deriv_time"):
        deriv_param_all_times(emu, [prm["omega"], emu.evaluation_times], [obs])
    with pytest.raises(TypeError):
        deriv_param_all_times(emu, [], [obs])
    with pytest.raises(ValueError, match="shape"):
        deriv_param_all_times(emu, [prm["omega"]], [P.DiagonalObservable(torch.ones(8, dtype=torch.float64))])
    noisy = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"],
                                  config=P.SimConfig(noise="doppler", runs=2, temperature=50.0))
    with pytest.raises(NotImplementedError, match="noisy"):
        deriv_param_all_times(noisy, [prm["omega"]], [obs])
    spam = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"],
                                 config=P.SimConfig(noise="SPAM", runs=2, eta=0.1))
    with pytest.raises(NotImplementedError, match="noisy"):
        deriv_param_all_times(spam, [prm["omega"]], [obs])


STATE_ATOL = 1e-13  # the same exponentials applied in the same order: rounding only


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


@pytest.mark.parametrize("solver", [SolverType.KRYLOV_SE, SolverType.DP5_SE], ids=["KRYLOV_SE", "DP5_SE"])
def test_dense_tangent_reference_against_reverse_mode_autograd(solver):
    """tests.helpers.tangent_dense_reference (block-exponential forward mode, no autograd) against reverse-mode autograd through
    the oracle's map (R.krylov_map_dense / magnus_cf4_dense) on terms + s * direction: 4 qubits, B = 2, 3 directions, all four
    tangent inputs.  tsave is off the sample grid with every DP5 piece at least 2 ns long, on a register 6.5 um apart:
    torch.linalg.matrix_exp, which the reverse-mode side goes through, loses accuracy for arguments of 1-norm 5e-3 .. 4.99e-2
    (tests.helpers.accurate_matrix_exp; with pieces of 1.3 ns at 8 um the two sides differ by 4.5e-10, and it is the reverse-mode
    side that is off), so the test asserts that no exponential of the map falls there.  Measured: 5e-16 (KRYLOV_SE), 4e-15 (DP5_SE).
    For a seeded random cotangent w over the states, sum Re(conj(w) * tangent_d) must equal d/ds_d of
    sum Re(conj(w) * states(s)) at 1e-12 relative; the states themselves must be the oracle's.  A second run with one HamTerms
    per trajectory (tables that differ) must reproduce, column by column, the runs with each trajectory's tables shared."""
    n, n_dir, batch = 4, 3, 2
    terms = random_terms(n, 21, 0.005, seed=61, local=True, phase=True, spacing=6.5)
    tsave = torch.tensor([0.0, 0.022, 0.048, 0.092], dtype=torch.float64)
    for steps in map_exponentials(terms, tsave, solver):
        for t, tau in steps:  # the reverse-mode side's matrix_exp is exact to rounding on every exponential of this map
            assert tau * float(torch.linalg.matrix_norm(R.dense_hamiltonian(terms, t), 1)) > 5.5e-2
    gen = torch.Generator().manual_seed(1234)
    dim = 2**n
    psi0 = _randn(gen, dim, batch, cplx=True)
    psi0 = psi0 / psi0.norm(dim=0, keepdim=True)
    ka, kd = len(terms.amp_terms()), len(terms.det_terms())
    d_amp = 0.5 * _randn(gen, n_dir, ka, 21, cplx=True)
    d_det = 0.5 * _randn(gen, n_dir, kd, 21)
    d_u = 0.5 * _randn(gen, n_dir, n * (n - 1) // 2)
    d_psi = _randn(gen, n_dir, dim, batch, cplx=True) / np.sqrt(dim)
    w = _randn(gen, len(tsave), dim, batch, cplx=True)

    def oracle_states(s):
        shifted = shifted_terms(terms, d_amp, d_det, d_u, s)
        start = psi0 + sum(s[j] * d_psi[j] for j in range(n_dir))
        if solver == SolverType.KRYLOV_SE:
            return R.krylov_map_dense(shifted, start, tsave)
        return magnus_cf4_dense(shifted, start, tsave, h_max=DP5_DEFAULT_H_MAX)

    s0 = torch.zeros(n_dir, dtype=torch.float64, requires_grad=True)
    ref_states = oracle_states(s0)
    (want,) = torch.autograd.grad((w.conj() * ref_states).real.sum(), s0)
    states, tangents = tangent_dense_reference(terms, d_amp, d_det, d_u, psi0, d_psi, tsave, solver)
    assert tuple(states.shape) == (len(tsave), dim, batch) and tuple(tangents.shape) == (len(tsave), n_dir, dim, batch)
    state_err = float((states - ref_states.detach()).abs().max())
    print(f"max |states - oracle states| = {state_err:.2e}")
    assert state_err <= STATE_ATOL
    for d in range(n_dir):
        got = float((w.conj() * tangents[:, d]).real.sum())
        rel = abs(got - float(want[d])) / max(abs(got), abs(float(want[d])))
        print(f"direction {d}: forward {got:+.15e}  reverse {float(want[d]):+.15e}  rel {rel:.2e}")
        assert abs(float(want[d])) > 1e-2  # cannot pass on zeros
        assert rel <= 1e-12
    # per-trajectory tables: the list form against one shared run per trajectory
    other = random_terms(n, 21, 0.005, seed=62, local=True, phase=True, spacing=6.5)
    d_amp_b = torch.stack([d_amp, 0.5 * _randn(gen, n_dir, ka, 21, cplx=True)], dim=1)
    d_det_b = torch.stack([d_det, 0.5 * _randn(gen, n_dir, kd, 21)], dim=1)
    st2, tg2 = tangent_dense_reference([terms, other], d_amp_b, d_det_b, d_u, psi0, d_psi, tsave, solver)
    for b, tb in enumerate((terms, other)):
        st1, tg1 = tangent_dense_reference(tb, d_amp_b[:, b], d_det_b[:, b], d_u, psi0[:, b:b + 1], d_psi[:, :, b:b + 1], tsave, solver)
        assert torch.equal(st2[:, :, b:b + 1], st1) and torch.equal(tg2[:, :, :, b:b + 1], tg1)
    assert float((tg2[..., 1] - tangents[..., 1]).abs().max()) > 1e-3  # the second trajectory's tables really differ


def test_dense_tangent_rows_are_the_derivatives_of_the_values():
    """tests.helpers.tangent_rows_reference: its derivative rows against autograd through its own value rows on psi + s * dpsi
    (diagonal, dense Pauli and overlap rows, shared and per-trajectory targets), 1e-13 relative to the largest entry."""
    n, n_dir, batch, n_t = 3, 2, 2, 2
    dim = 2**n
    gen = torch.Generator().manual_seed(99)
    states = _randn(gen, n_t, dim, batch, cplx=True)
    tangents = _randn(gen, n_t, n_dir, dim, batch, cplx=True)
    diag = _randn(gen, 2, dim)
    paulis = [P.PauliObservable(n, [(0.7, {0: "X", 2: "Y"}), (-0.4, {1: "Z"})]), P.PauliObservable(n, [(1.0, {1: "Y"})])]
    targets = [_randn(gen, dim, cplx=True), _randn(gen, dim, batch, cplx=True)]
    val, der = tangent_rows_reference(states, tangents, diag, paulis, targets)
    assert tuple(val.shape) == (2 + 2 + 4, n_t, batch) and tuple(der.shape) == (n_dir, 8, n_t, batch)
    for d in range(n_dir):
        s = torch.zeros((), dtype=torch.float64, requires_grad=True)
        jac = torch.autograd.functional.jacobian(
            lambda s_: tangent_rows_reference(states + s_ * tangents[:, d], tangents, diag, paulis, targets)[0], s)
        assert float((jac - der[d]).abs().max()) <= 1e-13 * float(der[d].abs().max())
