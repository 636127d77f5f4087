"""Pauli-string observables on the GPU: values and gradients through the C ABI (pulser_diff_amd.solver.evolve) and through the
emulator, against the CPU oracle and against the route through stored states and grad_states.

Bars (tests/test_gpu_solver_parity.py): values vs the oracle 1e-9 absolute x sum_s |w_s|; gradients vs oracle autograd 1e-8 relative
to the largest entry; one native route against another 1e-10 (1e-9 from 21 qubits on)."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd import pulses as pl
from pulser_diff_amd.observables import PauliObservable, expect_pauli
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, evolve
from pulser_diff_amd.utils import XMAT, DiagonalObservable, total_magnetization_diag
from tests.helpers import random_terms, rel_err, to_native

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9
GRAD_RTOL = 1e-8


def observable_set(n, seed=5):
    """sum X_j, sum Y_j, X_0 X_{N-1}, Z_1 Z_2, X_a Y_b Z_c (a among the last qubits, b, c among the first) and, from 13 qubits,
    X_a X_b with the two flips in different tile layouts; weights seeded in [-1, 1]."""
    rng = np.random.default_rng(seed + n)
    w = lambda: float(rng.uniform(-1, 1))  # noqa: E731
    out = [PauliObservable(n, [(w(), {j: "X"}) for j in range(n)]), PauliObservable(n, [(w(), {j: "Y"}) for j in range(n)])]
    if n >= 2:
        out.append(PauliObservable(n, [(w(), {0: "X", n - 1: "X"})]))
    if n >= 3:
        out.append(PauliObservable(n, [(w(), {1: "Z", 2: "Z"})]))
        out.append(PauliObservable(n, [(w(), {n - 1: "X", 0: "Y", 1: "Z"})]))
    if n >= 13:
        out.append(PauliObservable(n, [(w(), {1: "X", n - 2: "X"}), (w(), {n - 1: "Z"})]))  # index bits N-2 and 1: straddles the layouts
    return out


def weight_sum(obs):
    return sum(abs(w) for w, _, _ in obs.terms)


def np_expect(obs, psi):
    """<psi|O|psi> by numpy index arithmetic; psi (..., dim)."""
    dim = psi.shape[-1]
    y = np.arange(dim)
    total = 0.0
    for w, xm, zm, ph in obs.index_masks():
        yp = y ^ xm
        par = np.zeros(dim, dtype=np.int64)
        for j in range(obs.n_qubits):
            par ^= ((yp & zm) >> j) & 1
        total = total + w * (ph * np.conj(psi) * (1.0 - 2.0 * par) * psi[..., yp]).sum(-1)
    assert np.abs(np.imag(total)).max() < 1e-10
    return np.real(total)


def native_values(terms, tsave, psi_bd, device, solver=SolverType.KRYLOV_SE, variant=0, store_states=True, with_diag=True, obs=None):
    amp, det, u, spec = to_native(terms, device, solver, store_states=store_states)
    spec.pauli = observable_set(terms.n_qubits) if obs is None else obs
    spec.kernel_variant = variant
    zd = R.total_magnetization_diag(terms.n_qubits)[None].to(device) if with_diag else None
    states, expect = evolve(amp, det, u, tsave, psi_bd.to(device), spec, zd)
    torch.cuda.synchronize()
    return states, expect, spec


def check_values(expect, ref_states_tdb, n, with_diag=True, atol=VALUE_ATOL):
    """expect (n_diag + n_pauli, n_t, B) against states (n_t, dim, B) of the oracle."""
    ref = np.moveaxis(np.asarray(ref_states_tdb), 1, 2)  # (n_t, B, dim)
    got = expect.cpu().numpy()
    row = 0
    if with_diag:
        zd = R.total_magnetization_diag(n).numpy()
        assert np.abs(got[0] - (np.abs(ref) ** 2 * zd).sum(-1)).max() < atol * n
        row = 1
    obs = observable_set(n)
    assert got.shape[0] == row + len(obs)
    for o, ob in enumerate(obs):
        err = np.abs(got[row + o] - np_expect(ob, ref)).max()
        print(f"N={n} observable {o}: |native - oracle| = {err:.3e} (bar {atol * weight_sum(ob):.3e})")
        assert err < atol * weight_sum(ob), (n, o, err)


@pytest.mark.parametrize("n_qubits,phase", [(3, True), (5, False), (8, True), (10, False)])
def test_values_match_dense_oracle(cuda_device, n_qubits, phase):
    """One wave (3, 5 qubits) and one workgroup (8, 10): the one-launch sweeps, observables evaluated on the stored trajectory."""
    terms = random_terms(n_qubits, 41, 0.004, seed=500 + n_qubits, local=True, phase=phase)
    tsave = torch.linspace(0, 0.16, 11, dtype=torch.float64)
    gen = torch.Generator().manual_seed(n_qubits)
    psi0 = torch.randn(2**n_qubits, 2, generator=gen, dtype=torch.complex128)
    psi0 = psi0 / psi0.norm(dim=0, keepdim=True)
    ref = R.krylov_map_dense(terms, psi0, tsave).numpy()
    for store in (True, False):
        _, expect, _ = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, store_states=store)
        check_values(expect, ref, n_qubits)
    _, expect, _ = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, variant=1)  # launch per factor
    check_values(expect, ref, n_qubits)


def test_values_match_continuous_oracle_dp5(cuda_device):
    n = 5
    terms = random_terms(n, 61, 0.002, seed=505, local=True)
    tsave = torch.linspace(0, 0.12, 7, dtype=torch.float64)
    psi0 = R.all_ground_state(n)
    cont = R.continuous_solution(terms, psi0.numpy(), tsave.numpy())
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.DP5_SE, store_states=False)
    spec.pauli = observable_set(n)
    spec.tol = 1e-12
    _, expect = evolve(amp, det, u, tsave, psi0.T.contiguous().to(cuda_device), spec, R.total_magnetization_diag(n)[None].to(cuda_device))
    check_values(expect, cont, n)


@pytest.mark.parametrize("n_qubits,variants", [(12, (0, 1)), (14, (0, 2)), (16, (2, 14))])
def test_values_match_matrix_free_oracle(cuda_device, n_qubits, variants):
    terms = random_terms(n_qubits, 13, 0.002, seed=600 + n_qubits, local=True, phase=n_qubits != 14)
    tsave = torch.linspace(0, 0.022, 5, dtype=torch.float64)
    psi0 = R.all_ground_state(n_qubits)
    ref = R.krylov_map_matrix_free(terms, psi0.numpy(), tsave.numpy(), save_all=True, tol=1e-14)
    for v in variants:
        for store in (True, False):
            _, expect, _ = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, variant=v, store_states=store)
            check_values(expect, ref, n_qubits)


def _raw_final_state_only(terms, tsave, psi_bd, device, obs):
    """rydiff_forward with final_state_only through ctypes: expectation values at every save point, one state out."""
    amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE)
    spec.pauli = obs
    call = _Call(spec, amp, det, u, tsave.numpy(), psi_bd.shape[0], None)
    call.problem.final_state_only = 1
    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=device)
    info = _native.RydPlanInfo()
    _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()), stream, ctypes.byref(info)))
    ws = torch.empty(info.workspace_bytes, dtype=torch.uint8, device=device)
    last = torch.empty((1,) + tuple(psi_bd.shape), dtype=torch.complex128, device=device)
    expect = torch.empty((len(obs), len(tsave), psi_bd.shape[0]), dtype=torch.float64, device=device)
    _native.check(L.rydiff_forward(ctypes.byref(call.problem), ctypes.byref(info), ctypes.c_void_p(psi_bd.data_ptr()),
                                   ctypes.c_void_p(last.data_ptr()), ctypes.c_void_p(expect.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                   ctypes.c_size_t(ws.numel()), 0, stream))
    torch.cuda.synchronize()
    return last, expect


@pytest.mark.parametrize("n_qubits,variants,batch", [(13, (0, 2), 2), (16, (0, 2, 14), 1), (20, (0, 1), 1), (22, (0, 1), 1), (24, (0,), 1), (26, (1,), 1)])
def test_native_values_equal_torch_on_the_stored_states(cuda_device, n_qubits, variants, batch):
    """The reductions alone (the states are pinned elsewhere): the native values of a run against the same sums formed by torch
    index arithmetic from that run's own stored states; store_states=False and final_state_only give the same numbers."""
    terms = random_terms(n_qubits, 9, 0.002, seed=700 + n_qubits, local=n_qubits < 20)
    tsave = torch.linspace(0, 0.014, 3 if n_qubits >= 24 else 4, dtype=torch.float64)
    gen = torch.Generator().manual_seed(n_qubits)
    psi = torch.randn(batch, 2**n_qubits, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm(dim=1, keepdim=True)).to(cuda_device)
    obs = observable_set(n_qubits)
    tol = 1e-10 if n_qubits < 21 else 1e-9
    first = None
    for v in variants:
        states, expect, _ = native_values(terms, tsave, psi, cuda_device, variant=v, with_diag=False)
        for o, ob in enumerate(obs):
            for b in range(batch):
                want = expect_pauli(ob, states[:, b, :, None]).real
                err = (expect[o, :, b] - want).abs().max().item()
                assert err < tol * max(weight_sum(ob), 1.0), (n_qubits, v, o, err)
        del states
        torch.cuda.empty_cache()
        if first is None:
            first = expect
        assert (expect - first).abs().max().item() < tol
        _, e2, _ = native_values(terms, tsave, psi, cuda_device, variant=v, with_diag=False, store_states=False)
        assert (e2 - first).abs().max().item() < tol
    _, e3 = _raw_final_state_only(terms, tsave, psi, cuda_device, obs)
    assert (e3 - first).abs().max().item() < tol


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def _coefficients(n_obs, n_t, batch, seed):
    return torch.randn(n_obs, n_t, batch, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("n_qubits,batch,store", [(4, 1, True), (6, 1, False), (8, 1, True), (10, 1, False), (5, 3, False), (7, 3, True)])
def test_gradients_match_oracle_autograd(cuda_device, n_qubits, batch, store):
    """loss = sum_k sum_o c_ok <O_o>(t_k) over ALL save points, the diagonal observable included: g_amp (complex tables), g_det, g_u,
    g_tsave, g_psi0 against torch autograd through the oracle's dense map and dense operators."""
    n_samples, dt = 33, 0.004
    terms = random_terms(n_qubits, n_samples, dt, seed=800 + n_qubits, local=True)
    n_t = 5 if n_qubits >= 10 else 9
    tsave0 = torch.linspace(0, dt * (n_samples - 1), n_t, dtype=torch.float64)
    tsave0 = tsave0 + torch.cat([torch.zeros(1), 0.0007 * torch.rand(n_t - 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64), torch.zeros(1)])
    gen = torch.Generator().manual_seed(7)
    psi0 = torch.randn(2**n_qubits, batch, generator=gen, dtype=torch.complex128)
    psi0 = psi0 / psi0.norm(dim=0, keepdim=True)
    obs = observable_set(n_qubits)
    zdiag = R.total_magnetization_diag(n_qubits)
    c = _coefficients(1 + len(obs), n_t, batch, 11)

    o_terms = R.HamTerms(n_qubits, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                         terms.det_coeff.clone().requires_grad_(True), dt, n_samples, terms.amp_targets, terms.det_targets)
    o_terms.extra_amp = [(a.clone().requires_grad_(True), tg) for a, tg in terms.extra_amp]
    o_terms.extra_det = [(a.clone().requires_grad_(True), tg) for a, tg in terms.extra_det]
    o_ts = tsave0.clone().requires_grad_(True)
    o_psi = psi0.clone().requires_grad_(True)
    o_states = R.krylov_map_dense(o_terms, o_psi, o_ts)  # (n_t, dim, B)
    rows = [(o_states.abs() ** 2 * zdiag[None, :, None]).sum(1)]
    for ob in obs:
        rows.append(torch.einsum("tib,ij,tjb->tb", o_states.conj(), ob.to_dense(), o_states).real)
    o_exp = torch.stack(rows)
    o_loss = (c * o_exp).sum()
    o_loss.backward()
    o_amp = torch.stack([a.grad for a, _ in o_terms.amp_terms()])
    o_det = torch.stack([a.grad for a, _ in o_terms.det_terms()])

    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=store, batch_tables=batch)
    spec.pauli = obs
    for t in (amp, det, u):
        t.requires_grad_(True)
    ts = tsave0.clone().requires_grad_(True)
    psi_bd = psi0.T.contiguous().to(cuda_device).requires_grad_(True)
    _, expect = evolve(amp, det, u, ts, psi_bd, spec, zdiag[None].to(cuda_device))
    assert (expect.detach().cpu() - o_exp.detach()).abs().max().item() < VALUE_ATOL * n_qubits
    (c.to(cuda_device) * expect).sum().backward()
    torch.cuda.synchronize()
    got = {"amp": amp.grad.sum(0).cpu().numpy(), "det": det.grad.sum(0).cpu().numpy(), "u": u.grad.cpu().numpy(), "tsave": ts.grad.numpy(),
           "psi0": psi_bd.grad.T.cpu().numpy()}
    want = {"amp": o_amp.numpy(), "det": o_det.numpy(), "u": o_terms.u_pairs.grad.numpy(), "tsave": o_ts.grad.numpy(), "psi0": o_psi.grad.numpy()}
    for name in got:
        err = rel_err(got[name], want[name])
        print(f"N={n_qubits} B={batch} {name}: rel err {err:.3e}")
        assert err < GRAD_RTOL, (name, err)


def _grads_of(loss, leaves, retain=False):
    gs = torch.autograd.grad(loss, leaves, retain_graph=retain, allow_unused=True)
    return [None if g is None else g.detach().clone() for g in gs]


@pytest.mark.parametrize("n_qubits,tape,variant,phase", [(13, "steps", 1, True), (13, "full", 0, True), (14, "full", 2, True), (14, "partial", 2, True),
                                                         (17, "steps", 14, True), (17, "full", 17, False), (20, "full", 19, False),
                                                         (20, "partial", 0, False), (21, "steps", 0, True)])
def test_native_cotangent_equals_the_route_through_stored_states(cuda_device, n_qubits, tape, variant, phase):
    """Same loss two ways: from the native Pauli values (cotangent formed in the workspace by k_pauli_apply) and — what the parent
    commit offers — by torch from the stored states of a second run (cotangent handed back as grad_states)."""
    terms = random_terms(n_qubits, 13, 0.002, seed=900 + n_qubits, local=False, phase=phase)
    tsave0 = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)
    gen = torch.Generator().manual_seed(n_qubits)
    psi = torch.randn(1, 2**n_qubits, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm()).to(cuda_device)
    obs = observable_set(n_qubits)
    zd = R.total_magnetization_diag(n_qubits)[None].to(cuda_device)
    c = _coefficients(1 + len(obs), len(tsave0), 1, 13).to(cuda_device)
    tol = 1e-10 if n_qubits < 21 else 1e-9

    def run(native):
        amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=not native)
        if not phase:
            amp = amp.real.contiguous()  # a drive without phase: real tables, real_amp_grad
        spec.kernel_variant = variant
        spec.tape = tape
        if tape == "partial":
            spec.tape_steps = 2
        if native:
            spec.pauli = obs
        leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True), tsave0.clone().requires_grad_(True),
                  psi.clone().requires_grad_(True)]
        states, expect = evolve(*leaves, spec, zd)
        if not native:
            rows = [expect[0]] + [expect_pauli(ob, states.permute(0, 2, 1)).real[:, None] for ob in obs]
            expect = torch.stack(rows)
        return leaves, expect

    leaves_a, exp_a = run(True)
    leaves_b, exp_b = run(False)
    assert (exp_a - exp_b).abs().max().item() < tol
    one_hot = [torch.zeros_like(c) for _ in range(2)]
    one_hot[0][:, 1] = c[:, 1]
    one_hot[1][:, -1] = c[:, -1]
    for weights, retain in ((one_hot[0], True), (one_hot[1], True), (c, False)):
        ga = _grads_of((weights * exp_a).sum(), leaves_a, retain)
        gb = _grads_of((weights * exp_b).sum(), leaves_b, retain)
        torch.cuda.synchronize()
        for name, a, b in zip(("amp", "det", "u", "tsave", "psi0"), ga, gb):
            err = rel_err(a.cpu().numpy(), b.cpu().numpy())
            assert err < tol, (name, err)


# ---- emulator ---------------------------------------------------------------------------------------------------------------
def _phase_sequence(n, area=None, phase=0.3):
    coords = {f"q{j}": torch.tensor([8.0 * (j % 3), 8.0 * (j // 3)], dtype=torch.float64) for j in range(n)}
    seq = pl.Sequence(pl.Register(coords), pl.MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(200, 2.5 if area is None else area), pl.RampWaveform(200, -4.0, 2.0), phase), "ch")
    seq.add(pl.Pulse.ConstantPulse(100, 5.0, 1.0, phase), "ch")
    return seq, torch.stack(list(coords.values()))


@pytest.mark.parametrize("n_qubits", [4, 6])
def test_emulator_in_the_rotating_frame_against_the_oracle(cuda_device, n_qubits):
    seq, coords = _phase_sequence(n_qubits)
    emu = P.TorchEmulator.from_sequence(seq, sampling_rate=0.2)
    assert emu._hamiltonian.frame_phase is not None
    ox = emu.build_observable([("X", "global")])
    oxy = emu.build_observable([("X", ["q0"]), ("Y", [f"q{n_qubits - 1}"])])
    zobs = DiagonalObservable(total_magnetization_diag(n_qubits))
    res = emu.run(solver=SolverType.KRYLOV_SE, observables=[ox, zobs, oxy], store_states=False)
    got = [r.real.cpu().numpy() for r in res.expect([ox, zobs, oxy])]
    oseq = R.concat_pulses([(R.blackman_waveform(200, 2.5), R.ramp_waveform(200, -4.0, 2.0), 0.3),
                            (R.constant_waveform(100, 5.0), R.constant_waveform(100, 1.0), 0.3)])
    oterms = R.build_terms(oseq, coords, 0.2)
    ost = R.krylov_map_dense(oterms, R.all_ground_state(n_qubits), emu.evaluation_times)
    dense_x = emu.build_operator([(XMAT.clone(), "global")]).to_dense()
    want_x = R.expect(dense_x, ost).real.numpy().reshape(-1)
    assert np.abs(got[0] - want_x).max() < VALUE_ATOL * n_qubits
    assert np.abs(got[2] - R.expect(oxy.to_dense(), ost).real.numpy().reshape(-1)).max() < VALUE_ATOL
    assert np.abs(got[1] - R.expect(torch.diag(zobs.diag.to(torch.complex128)), ost).real.numpy().reshape(-1)).max() < VALUE_ATOL * n_qubits
    # torch fallback: a run with stored states and no observables= gives the same through results.expect
    res2 = emu.run(solver=SolverType.KRYLOV_SE)
    fb = res2.expect([ox, oxy])
    assert np.abs(fb[0].real.cpu().numpy() - got[0]).max() < 1e-10 * n_qubits
    assert np.abs(fb[1].real.cpu().numpy() - got[2]).max() < 1e-10


def test_xy_mode_transverse_magnetisation(cuda_device):
    seq = pl.Sequence(pl.Register.from_coordinates([[0.0, 0.0], [6.5, 1.0], [13.0, 0.0], [6.0, 7.0]]), pl.MockDevice)
    seq.declare_channel("g", "mw_global")
    seq.add(pl.Pulse.ConstantPulse(60, 3.0, 1.0, 0.0), "g")
    emu = P.TorchEmulator.from_sequence(seq, xy_hermitian=True)
    ox = emu.build_observable([("X", "global")])
    res = emu.run(solver=SolverType.KRYLOV_SE, observables=[ox])
    native = res.expect([ox])[0].real.cpu().numpy()
    dense = res.expect([emu.build_operator([(XMAT.clone(), "global")]).to_dense().to(cuda_device)])[0].real.cpu().numpy()
    assert np.abs(native - dense).max() < VALUE_ATOL * 4
    assert np.abs(native).max() > 1e-3


def test_quantum_model_expectation_backpropagates_to_a_pulse_parameter(cuda_device):
    from pulser_diff_amd.model import QuantumModel

    def model():
        reg = pl.Register.rectangle(2, 2, spacing=8, prefix="q")
        seq = pl.Sequence(reg, pl.MockDevice)
        seq.declare_channel("rydberg_global", "rydberg_global")
        area = seq.declare_variable("area")
        seq.add(pl.Pulse(pl.BlackmanWaveform(400, area), pl.RampWaveform(400, 5.0, 0.0), 0.4), "rydberg_global")
        return QuantumModel(seq, {"area": torch.tensor([2.0], dtype=torch.float64, requires_grad=True)}, sampling_rate=0.5,
                            solver=SolverType.KRYLOV_SE)

    obs = PauliObservable(4, [(1.0, {j: "X"}) for j in range(4)] + [(0.5, {0: "Y", 3: "Y"})])
    grads, values = [], []
    for o in (obs, obs.to_dense()):
        m = model()
        _, e = m.expectation(o.to(cuda_device) if isinstance(o, torch.Tensor) else o)
        e.real[-1].backward()
        grads.append(dict(m.named_parameters())["seq_param_values.area"].grad.item())
        values.append(e.real.detach().cpu().numpy().reshape(-1))
    assert np.abs(values[0] - values[1]).max() < VALUE_ATOL * weight_sum(obs)
    assert abs(grads[0] - grads[1]) < GRAD_RTOL * max(abs(grads[1]), 1e-3) and abs(grads[1]) > 1e-6


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_sharded_runs_refuse_pauli_observables(cuda_device):
    n = 6
    terms = random_terms(n, 9, 0.002, seed=1, local=False)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
    spec.pauli = observable_set(n)
    call = _Call(spec, amp, det, u, np.linspace(0, 0.01, 3), 2, None)
    call.problem.shard_bits = 1
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=cuda_device)
    info = _native.RydPlanInfo()
    with pytest.raises(NotImplementedError):
        _native.check(_native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream), ctypes.byref(info)))


def test_c_abi_validates_the_pauli_arrays(cuda_device):
    n = 4
    terms = random_terms(n, 9, 0.002, seed=2, local=False)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
    spec.pauli = observable_set(n)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=cuda_device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)

    def plan(mutate):
        call = _Call(spec, amp, det, u, np.linspace(0, 0.01, 3), 1, None)
        mutate(call)
        _native.check(_native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()), stream,
                                                ctypes.byref(_native.RydPlanInfo())))

    plan(lambda call: None)
    with pytest.raises(ValueError):  # mask bit >= N
        plan(lambda call: call.pauli[1].__setitem__(0, 1 << n))
    with pytest.raises(ValueError):  # NULL arrays with a non-zero count
        plan(lambda call: setattr(call.problem, "pauli_w", None))
    with pytest.raises(ValueError):  # non-monotone pauli_first
        plan(lambda call: call.pauli[0].__setitem__(1, int(call.pauli[0][2]) + 1))
    with pytest.raises(ValueError):  # more strings than the cap
        plan(lambda call: setattr(call.problem, "n_pauli_strings", _native.MAX_PAULI_STRINGS + 1))


def test_three_level_basis_refuses_pauli_observables(cuda_device):
    coords = {f"q{j}": torch.tensor([8.0 * j, 0.0], dtype=torch.float64) for j in range(2)}
    seq = pl.Sequence(pl.Register(coords), pl.MockDevice)
    seq.declare_channel("ryd", "rydberg_global")
    seq.declare_channel("ram", "raman_local", initial_target="q0")
    seq.add(pl.Pulse.ConstantPulse(100, 3.0, 0.5, 0.0), "ryd")
    seq.add(pl.Pulse.ConstantPulse(100, 2.0, 0.0, 0.0), "ram")
    emu = P.TorchEmulator.from_sequence(seq, sampling_rate=0.5)
    with pytest.raises(NotImplementedError):
        emu.build_observable([("X", "global")])
    with pytest.raises(NotImplementedError):
        emu.run(solver=SolverType.KRYLOV_SE, observables=[PauliObservable(2, [(1.0, "XI")])])
