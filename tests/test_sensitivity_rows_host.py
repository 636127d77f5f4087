"""Row order and gradient shapes of the three all-times methods of TorchEmulator (run_sensitivities, run_quantum_fisher,
run_rdm_sensitivities), host side (no GPU): the sweeps are replaced by recorders that number the native rows — expect[r] = r,
dexpect[d, r] = 100 (d + 1) + r — so that a row taken from a neighbour's block, or a direction unflattened into the wrong entry of
x, shows as a wrong number."""
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native, backend as B, pulses as pl
from pulser_diff_amd.observables import PauliObservable, ReducedDensityMatrix, StateOverlap
from pulser_diff_amd.solver import split_observables
from pulser_diff_amd.utils import DiagonalObservable

N, DIM = 3, 8


def _emulator(w, phase):
    """Three atoms, a Blackman and a constant pulse; w = [[amplitude], [area]] (2-D) and the drive phase carry the parameters."""
    reg = pl.Register({"q0": torch.tensor([0.0, 0.0], dtype=torch.float64), "q1": torch.tensor([0.0, 8.0], dtype=torch.float64),
                       "q2": torch.tensor([8.0, 0.0], dtype=torch.float64)})
    seq = pl.Sequence(reg, pl.MockDevice)
    seq.declare_channel("rydberg_global", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(400, w[1, 0]), pl.RampWaveform(400, -5.0, 0.0), phase[0]), "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(400, w[0, 0], 0.0, phase[0]), "rydberg_global")
    return P.TorchEmulator.from_sequence(seq, sampling_rate=0.1, compute_device="cpu")


def _parameters(requires_grad=True):
    w = torch.tensor([[5.0], [torch.pi]], dtype=torch.float64, requires_grad=requires_grad)
    phase = torch.tensor([0.4], dtype=torch.float64, requires_grad=requires_grad)
    return w, phase


def _native_rows(spec, obs_diag):
    return (0 if obs_diag is None else obs_diag.shape[0]) + len(spec.pauli or []) + 2 * spec.n_overlaps + spec.rdm_rows()


def _numbered(rows, n_t, batch, n_dir):
    expect = torch.arange(rows, dtype=torch.float64)[:, None, None].expand(rows, n_t, batch).clone()
    return expect, torch.stack([expect + 100.0 * (d + 1) for d in range(n_dir)]) if n_dir else expect.new_zeros((0,) + expect.shape)


@pytest.fixture
def recorders(monkeypatch):
    """backend.evolve_tangent / evolve_geometry / evolve replaced by recorders; seen[name] holds the arguments of the last call."""
    seen = {}

    def record(name, tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0, flags):
        given = [t for t in (d_amp, d_det, d_u, d_psi0) if t is not None]
        n_dir = int(given[0].shape[0]) if given else 0
        rows = _native_rows(spec, obs_diag)
        expect, dexpect = _numbered(rows, len(tsave), psi0.shape[0], n_dir)
        seen[name] = dict(spec=spec, obs_diag=obs_diag, flags=flags, n_dir=n_dir, expect=expect, dexpect=dexpect, d_psi0=d_psi0)
        return expect, dexpect

    def tangent(amp, det, u, tsave, psi0, spec, obs_diag=None, d_amp=None, d_det=None, d_u=None, d_psi0=None, flags=0):
        return record("tangent", tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0, flags)

    def geometry(amp, det, u, tsave, psi0, spec, obs_diag=None, d_amp=None, d_det=None, d_u=None, d_psi0=None, flags=0):
        expect, dexpect = record("geometry", tsave, psi0, spec, obs_diag, d_amp, d_det, d_u, d_psi0, flags)
        gram = torch.zeros((len(tsave), psi0.shape[0], 1 + dexpect.shape[0], 1 + dexpect.shape[0]), dtype=torch.complex128)
        gram[:, :, 0, 0] = 1.0
        return expect, dexpect, gram

    def plain(amp, det, u, tsave, psi0, spec, obs_diag=None):
        expect, _ = record("evolve", tsave, psi0, spec, obs_diag, None, None, None, None, None)
        return torch.empty((0, psi0.shape[0], psi0.shape[1]), dtype=torch.complex128), expect

    monkeypatch.setattr(B, "evolve_tangent", tangent)
    monkeypatch.setattr(B, "evolve_geometry", geometry)
    monkeypatch.setattr(B, "evolve", plain)
    return seen


def _check_grads(grads, x, native_row, n_t):
    """grads[i][o, k, idx] = 100 (d + 1) + native_row[o] with d the position of entry idx of x_i among all scalars of x."""
    d0 = 0
    for g, t in zip(grads, x):
        assert g.shape == (len(native_row), n_t) + tuple(t.shape) and g.dtype == torch.float64
        flat = g.reshape(len(native_row), n_t, -1)
        for j in range(t.numel()):
            for o, r in enumerate(native_row):
                assert flat[o, :, j].tolist() == [100.0 * (d0 + j + 1) + r] * n_t
        d0 += t.numel()


def test_run_sensitivities_maps_observables_to_native_rows(recorders):
    w, phase = _parameters()
    emu = _emulator(w, phase)
    n_t = int(emu.evaluation_times.shape[0])
    p0, p1 = PauliObservable(N, [(1.0, "XYZ")]), PauliObservable(N, [(0.5, "ZII"), (0.25, "IXI")])
    d0 = DiagonalObservable(torch.arange(DIM, dtype=torch.float64))
    dense = torch.diag(torch.linspace(-1.0, 1.0, DIM).to(torch.complex128))
    x = [w, phase]  # (2, 1) and (1,): three directions
    out = emu.run_sensitivities(x, [p0, d0, p1, dense], solver=P.SolverType.KRYLOV_SE)
    native_row = [2, 0, 3, 1]  # diagonal rows 0-1, Pauli rows 2-3
    assert out.route == "tangent" and "evolve" not in recorders
    assert out.values.shape == (4, n_t) and out.values[:, 0].tolist() == [float(r) for r in native_row]
    _check_grads(out.grads, x, native_row, n_t)
    seen = recorders["tangent"]
    assert seen["n_dir"] == 3 and seen["flags"] == 0
    assert list(seen["spec"].pauli) == [p0, p1] and seen["spec"].overlaps is None and seen["spec"].rdms is None
    assert not seen["spec"].store_states
    assert torch.equal(seen["obs_diag"], torch.stack([d0.diag, torch.diagonal(dense).real]))


def test_run_quantum_fisher_gives_every_overlap_two_rows(recorders):
    w, phase = _parameters()
    emu = _emulator(w, phase)
    n_t = int(emu.evaluation_times.shape[0])
    gen = torch.Generator().manual_seed(11)
    targets = [torch.randn(DIM, generator=gen, dtype=torch.complex128) for _ in range(2)]
    ov0, ov1 = (StateOverlap(t / t.norm()) for t in targets)
    d0 = DiagonalObservable(torch.arange(DIM, dtype=torch.float64))
    p0 = PauliObservable(N, [(1.0, "XXI")])
    x = [phase, w]
    out = emu.run_quantum_fisher(x, [ov0, d0, p0, ov1], solver=P.SolverType.KRYLOV_SE)
    native_row = [2, 3, 0, 1, 4, 5]  # n_real = 2: overlap r sits in rows n_real + 2 r (Re) and n_real + 2 r + 1 (Im)
    assert out.values.shape == (6, n_t) and out.values[:, 0].tolist() == [float(r) for r in native_row]
    _check_grads(out.grads, x, native_row, n_t)
    assert out.gram.shape == (n_t, 4, 4) and out.qfi.shape == (n_t, 3, 3)
    seen = recorders["geometry"]
    assert seen["n_dir"] == 3 and seen["flags"] == 0
    assert list(seen["spec"].pauli) == [p0] and seen["obs_diag"].shape == (1, DIM)
    assert seen["spec"].overlaps.shape == (2, 1, DIM) and seen["spec"].overlaps.dtype == torch.complex128


def test_run_rdm_sensitivities_returns_the_matrices_of_the_rdm_block(recorders):
    w, phase = _parameters()
    emu = _emulator(w, phase)
    n_t = int(emu.evaluation_times.shape[0])
    x = [w, phase]
    out = emu.run_rdm_sensitivities(x, [ReducedDensityMatrix([1]), (2, 0)], solver=P.SolverType.KRYLOV_SE)
    seen = recorders["tangent"]
    assert seen["flags"] == _native.TANGENT_RDMS and seen["n_dir"] == 3 and seen["obs_diag"] is None
    rdms = seen["spec"].rdms
    assert [tuple(o.qubits) for o in rdms] == [(1,), (2, 0)]
    assert seen["expect"].shape[0] == 2 * 4 + 2 * 16
    want = split_observables(seen["expect"], 0, rdms)[2]
    want_d = [split_observables(seen["dexpect"][d], 0, rdms)[2] for d in range(3)]
    for o, m in enumerate((1, 2)):
        assert out.rho[o].shape == (n_t, 1, 2 ** m, 2 ** m) and torch.equal(out.rho[o], want[o])
        d0 = 0
        for i, t in enumerate(x):
            got = out.drho[o][i]
            assert got.shape == (n_t, 1, 2 ** m, 2 ** m) + tuple(t.shape) and got.dtype == torch.complex128
            flat = got.reshape(n_t, 1, 2 ** m, 2 ** m, -1)
            for j in range(t.numel()):
                assert torch.equal(flat[..., j], want_d[d0 + j][o])
            d0 += t.numel()


def test_x_that_reaches_no_table_takes_the_plain_run_and_gives_zero_derivatives(recorders):
    emu = _emulator(*_parameters(requires_grad=False))
    n_t = int(emu.evaluation_times.shape[0])
    x = [torch.tensor([[1.0, 2.0]], dtype=torch.float64, requires_grad=True), torch.tensor([3.0], dtype=torch.float64, requires_grad=True)]
    p0 = PauliObservable(N, [(1.0, "XYZ")])
    d0 = DiagonalObservable(torch.arange(DIM, dtype=torch.float64))
    out = emu.run_sensitivities(x, [p0, d0], solver=P.SolverType.KRYLOV_SE)
    assert "tangent" not in recorders and recorders["evolve"]["n_dir"] == 0
    assert out.values[:, 0].tolist() == [1.0, 0.0]
    assert [tuple(g.shape) for g in out.grads] == [(2, n_t, 1, 2), (2, n_t, 1)]
    assert all(not g.any() for g in out.grads)
    recorders.clear()
    sub = emu.run_rdm_sensitivities(x, [(0,), (1, 2)], solver=P.SolverType.KRYLOV_SE)
    assert "tangent" not in recorders and recorders["evolve"]["expect"].shape[0] == 2 * 4 + 2 * 16
    assert torch.equal(sub.rho[1], split_observables(recorders["evolve"]["expect"], 0, recorders["evolve"]["spec"].rdms)[2][1])
    assert [tuple(g.shape) for g in sub.drho[1]] == [(n_t, 1, 4, 4, 1, 2), (n_t, 1, 4, 4, 1)]
    assert all(not g.any() for parts in sub.drho for g in parts)
    recorders.clear()
    # run_quantum_fisher's variant: one sweep with a single zero d_psi0 direction delivers <psi|psi> and the values
    geo = emu.run_quantum_fisher(x, [d0], solver=P.SolverType.KRYLOV_SE)
    assert "evolve" not in recorders and recorders["geometry"]["n_dir"] == 1 and not recorders["geometry"]["d_psi0"].any()
    assert geo.gram.shape == (n_t, 4, 4) and [tuple(g.shape) for g in geo.grads] == [(1, n_t, 1, 2), (1, n_t, 1)]
    assert all(not g.any() for g in geo.grads)
