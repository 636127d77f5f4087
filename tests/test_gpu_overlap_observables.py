"""State-overlap observables on the GPU: c[k][b] = <phi_b|psi_b(t_k)> and its gradients through the C ABI
(pulser_diff_amd.solver.evolve), the emulator and QuantumModel, against the CPU oracle and against the route through stored states
and grad_states.

Bars (tests/test_gpu_solver_parity.py), with normalised targets and states: values vs the oracle 1e-9 absolute; gradients vs oracle
autograd 1e-8 relative to the largest entry; one native route against another 1e-10."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd.observables import PauliObservable, StateOverlap, expect_pauli, overlap_states, pack_overlaps
from pulser_diff_amd.solver import SolverType, _Call, evolve, split_expect
from tests.helpers import random_terms, rel_err, to_native

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9
GRAD_RTOL = 1e-8
ROUTE_TOL = 1e-10


def target_set(n, batch, seed=3):
    """A basis state, a random normalised vector shared by the batch, random normalised vectors per trajectory."""
    dim = 2**n
    g = torch.Generator().manual_seed(seed + n)
    basis = torch.zeros(dim, dtype=torch.complex128)
    basis[3 % dim] = 1.0
    shared = torch.randn(dim, generator=g, dtype=torch.complex128)
    per = torch.randn(dim, batch, generator=g, dtype=torch.complex128)
    return [StateOverlap(basis), StateOverlap(shared / shared.norm()), StateOverlap(per / per.norm(dim=0, keepdim=True))]


def pauli_of(n):
    return PauliObservable(n, [(0.7, {j: "X"}) for j in range(n)] + [(-0.4, {0: "Y"})])


def ref_overlaps(obs_list, states_tdb):
    """(n_ov, n_t, B) complex from states (n_t, dim, B), numpy."""
    st = np.asarray(states_tdb)
    return np.stack([np.einsum("db,tdb->tb", np.conj(np.broadcast_to(o.targets.numpy(), st.shape[1:])), st) for o in obs_list])


def native_values(terms, tsave, psi_bd, device, obs_list, solver=SolverType.KRYLOV_SE, variant=0, store_states=True, others=True, tol=0.0):
    """-> states, real rows (diagonal, Pauli), complex overlaps (n_ov, n_t, B)."""
    amp, det, u, spec = to_native(terms, device, solver, store_states=store_states, tol=tol)
    n = terms.n_qubits
    spec.overlaps = pack_overlaps(obs_list, 2**n, psi_bd.shape[0], device)
    spec.kernel_variant = variant
    zd = None
    if others:
        spec.pauli = [pauli_of(n)]
        zd = R.total_magnetization_diag(n)[None].to(device)
    states, expect = evolve(amp, det, u, tsave, psi_bd.to(device), spec, zd)
    torch.cuda.synchronize()
    assert expect.shape[0] == (2 if others else 0) + 2 * len(obs_list)
    real, ov = split_expect(expect, len(obs_list))
    return states, real, ov


def check_values(real, ov, obs_list, ref_tdb, n, label):
    ref = np.asarray(ref_tdb)
    # row order: the diagonal observable, the Pauli observable, then Re / Im of every overlap
    zd = R.total_magnetization_diag(n).numpy()
    assert np.abs(real[0].cpu().numpy() - (np.abs(ref) ** 2 * zd[None, :, None]).sum(1)).max() < VALUE_ATOL * n
    if n <= 10:
        want_p = np.einsum("tib,ij,tjb->tb", np.conj(ref), pauli_of(n).to_dense().numpy(), ref).real
    else:  # no 2^N x 2^N operator: the index-arithmetic fallback (pinned against dense operators in tests/test_pauli_observables_host.py)
        st = torch.from_numpy(ref)
        want_p = torch.stack([expect_pauli(pauli_of(n), st[:, :, b:b + 1]).real for b in range(st.shape[2])], dim=1).numpy()
    assert np.abs(real[1].cpu().numpy() - want_p).max() < VALUE_ATOL * (0.7 * n + 0.4)
    err = np.abs(ov.cpu().numpy() - ref_overlaps(obs_list, ref)).max()
    print(f"N={n} {label}: |native - oracle| = {err:.3e}")
    assert err < VALUE_ATOL, (n, label, err)


def _random_psi0(n, batch):
    psi0 = torch.randn(2**n, batch, generator=torch.Generator().manual_seed(n), dtype=torch.complex128)
    return psi0 / psi0.norm(dim=0, keepdim=True)


@pytest.mark.parametrize("n_qubits,batch,variants", [(1, 1, (0,)), (3, 1, (0,)), (5, 1, (0,)), (5, 3, (0,)), (8, 1, (0,)), (10, 1, (0, 1))])
def test_values_match_dense_oracle(cuda_device, n_qubits, batch, variants):
    """dim below the block size (1 qubit), one wave (3, 5), one workgroup (8, 10), launch per factor (variant 1); both packings
    (overlap_batch 1 and B), both store_states settings, next to a diagonal and a Pauli observable."""
    terms = random_terms(n_qubits, 41, 0.004, seed=520 + n_qubits, local=True)
    tsave = torch.linspace(0, 0.16, 11, dtype=torch.float64)
    psi0 = _random_psi0(n_qubits, batch)
    ref = R.krylov_map_dense(terms, psi0, tsave).numpy()
    tg = target_set(n_qubits, batch)
    for v in variants:
        for store in (True, False):
            for label, obs_list in (("shared targets", tg[:2]), ("targets per trajectory", tg)):
                _, real, ov = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, obs_list, variant=v, store_states=store)
                check_values(real, ov, obs_list, ref, n_qubits, f"B={batch} variant {v} store={store} {label}")


def test_sixteen_targets_in_one_call(cuda_device):
    """The widest instantiation (16 accumulator pairs) and an odd count (5, padded to 8)."""
    n = 5
    terms = random_terms(n, 41, 0.004, seed=525, local=True)
    tsave = torch.linspace(0, 0.16, 5, dtype=torch.float64)
    psi0 = _random_psi0(n, 2)
    ref = R.krylov_map_dense(terms, psi0, tsave).numpy()
    many = [target_set(n, 2, seed=s)[1 + s % 2] for s in range(16)]
    for obs_list in (many, many[:5]):
        _, real, ov = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, obs_list, store_states=False)
        check_values(real, ov, obs_list, ref, n, f"{len(obs_list)} targets")


def test_values_match_continuous_oracle_dp5(cuda_device):
    n = 5
    terms = random_terms(n, 61, 0.002, seed=505, local=True)
    tsave = torch.linspace(0, 0.12, 7, dtype=torch.float64)
    psi0 = R.all_ground_state(n)
    cont = R.continuous_solution(terms, psi0.numpy(), tsave.numpy())
    tg = target_set(n, 1)
    _, real, ov = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, tg, solver=SolverType.DP5_SE, store_states=False, tol=1e-12)
    check_values(real, ov, tg, cont, n, "DP5_SE")


@pytest.mark.parametrize("n_qubits,variants", [(12, (0, 1)), (14, (0, 2))])
def test_values_match_matrix_free_oracle(cuda_device, n_qubits, variants):
    terms = random_terms(n_qubits, 7, 0.002, seed=620 + n_qubits, local=True)  # (short run: the CPU oracle is the cost of this test)
    tsave = torch.linspace(0, 0.011, 5, dtype=torch.float64)
    psi0 = R.all_ground_state(n_qubits)
    ref = R.krylov_map_matrix_free(terms, psi0.numpy(), tsave.numpy(), save_all=True, tol=1e-14)
    tg = target_set(n_qubits, 1)
    for v in variants:
        for store in (True, False):
            _, real, ov = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, tg, variant=v, store_states=store)
            check_values(real, ov, tg, ref, n_qubits, f"variant {v} store={store}")


def _raw_final_state_only(terms, tsave, psi_bd, device, obs_list):
    """rydiff_forward with final_state_only through ctypes: overlaps at every save point, one state out."""
    amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE)
    spec.overlaps = pack_overlaps(obs_list, psi_bd.shape[1], psi_bd.shape[0], device)
    call = _Call(spec, amp, det, u, tsave.numpy(), psi_bd.shape[0], None)
    call.problem.final_state_only = 1
    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=device)
    info = _native.RydPlanInfo()
    _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()), stream, ctypes.byref(info)))
    ws = torch.empty(info.workspace_bytes, dtype=torch.uint8, device=device)
    last = torch.empty((1,) + tuple(psi_bd.shape), dtype=torch.complex128, device=device)
    expect = torch.empty((2 * len(obs_list), len(tsave), psi_bd.shape[0]), dtype=torch.float64, device=device)
    _native.check(L.rydiff_forward(ctypes.byref(call.problem), ctypes.byref(info), ctypes.c_void_p(psi_bd.data_ptr()),
                                   ctypes.c_void_p(last.data_ptr()), ctypes.c_void_p(expect.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                   ctypes.c_size_t(ws.numel()), 0, stream))
    torch.cuda.synchronize()
    return last, split_expect(expect, len(obs_list))[1]


@pytest.mark.parametrize("n_qubits,batch", [(13, 2), (16, 1), (20, 1)])
def test_native_values_equal_torch_on_the_stored_states(cuda_device, n_qubits, batch):
    """The reductions alone (several blocks per state, grid-stride loop at 20 qubits): torch.vdot on the same run's stored states;
    store_states=False and final_state_only give the same numbers."""
    terms = random_terms(n_qubits, 9, 0.002, seed=720 + n_qubits, local=n_qubits < 20)
    tsave = torch.linspace(0, 0.014, 4, dtype=torch.float64)
    psi = _random_psi0(n_qubits, batch).T.contiguous().to(cuda_device)
    tg = target_set(n_qubits, batch)
    states, _, ov = native_values(terms, tsave, psi, cuda_device, tg, others=False)
    for o, ob in enumerate(tg):
        phi = ob.targets.to(cuda_device)
        for b in range(batch):
            for k in range(len(tsave)):
                want = torch.vdot(phi[:, b if ob.batch > 1 else 0], states[k, b])
                assert abs((ov[o, k, b] - want).item()) < ROUTE_TOL, (n_qubits, o, k, b)
    del states
    _, _, ov2 = native_values(terms, tsave, psi, cuda_device, tg, others=False, store_states=False)
    assert (ov2 - ov).abs().max().item() < ROUTE_TOL
    _, ov3 = _raw_final_state_only(terms, tsave, psi, cuda_device, tg)
    assert (ov3 - ov).abs().max().item() < ROUTE_TOL


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def _weights(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _loss(real, ov, w):
    """sum_k w_k |c_k|^2 + sum_k (a_k Re c_k + b_k Im c_k), next to a diagonal and a Pauli observable."""
    return (w["abs"] * (ov.real ** 2 + ov.imag ** 2)).sum() + (w["re"] * ov.real).sum() + (w["im"] * ov.imag).sum() + (w["real"] * real).sum()


@pytest.mark.parametrize("n_qubits,batch,store", [(4, 1, True), (6, 1, False), (8, 1, True), (10, 1, False), (5, 3, False), (7, 3, True)])
def test_gradients_match_oracle_autograd(cuda_device, n_qubits, batch, store):
    """Random weights on ALL save points (k = 0 and k = T included): g_amp (complex tables), g_det, g_u, g_tsave, g_psi0 against torch
    autograd through the oracle's dense map and einsum overlaps."""
    n_samples, dt = 33, 0.004
    terms = random_terms(n_qubits, n_samples, dt, seed=820 + n_qubits, local=True)
    n_t = 5 if n_qubits >= 10 else 9
    tsave0 = torch.linspace(0, dt * (n_samples - 1), n_t, dtype=torch.float64)
    tsave0 = tsave0 + torch.cat([torch.zeros(1), 0.0007 * torch.rand(n_t - 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64), torch.zeros(1)])
    psi0 = torch.randn(2**n_qubits, batch, generator=torch.Generator().manual_seed(7), dtype=torch.complex128)
    psi0 = psi0 / psi0.norm(dim=0, keepdim=True)
    tg = target_set(n_qubits, batch)
    zdiag = R.total_magnetization_diag(n_qubits)
    w = {"abs": _weights((3, n_t, batch), 11), "re": _weights((3, n_t, batch), 12), "im": _weights((3, n_t, batch), 13),
         "real": _weights((2, n_t, batch), 14)}

    o_terms = R.HamTerms(n_qubits, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                         terms.det_coeff.clone().requires_grad_(True), dt, n_samples, terms.amp_targets, terms.det_targets)
    o_terms.extra_amp = [(a.clone().requires_grad_(True), t) for a, t in terms.extra_amp]
    o_terms.extra_det = [(a.clone().requires_grad_(True), t) for a, t in terms.extra_det]
    o_ts = tsave0.clone().requires_grad_(True)
    o_psi = psi0.clone().requires_grad_(True)
    o_states = R.krylov_map_dense(o_terms, o_psi, o_ts)  # (n_t, dim, B)
    o_real = torch.stack([(o_states.abs() ** 2 * zdiag[None, :, None]).sum(1),
                          torch.einsum("tib,ij,tjb->tb", o_states.conj(), pauli_of(n_qubits).to_dense(), o_states).real])
    o_ov = torch.stack([torch.einsum("db,tdb->tb", ob.targets.conj().expand(-1, batch), o_states) for ob in tg])
    _loss(o_real, o_ov, w).backward()
    o_amp = torch.stack([a.grad for a, _ in o_terms.amp_terms()])
    o_det = torch.stack([a.grad for a, _ in o_terms.det_terms()])

    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=store, batch_tables=batch)
    spec.pauli = [pauli_of(n_qubits)]
    spec.overlaps = pack_overlaps(tg, 2**n_qubits, batch, cuda_device)
    for t in (amp, det, u):
        t.requires_grad_(True)
    ts = tsave0.clone().requires_grad_(True)
    psi_bd = psi0.T.contiguous().to(cuda_device).requires_grad_(True)
    _, expect = evolve(amp, det, u, ts, psi_bd, spec, zdiag[None].to(cuda_device))
    real, ov = split_expect(expect, 3)
    assert (ov.detach().cpu() - o_ov.detach()).abs().max().item() < VALUE_ATOL
    _loss(real, ov, {k: v.to(cuda_device) for k, v in w.items()}).backward()
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


@pytest.mark.parametrize("n_qubits,tape,variant,phase", [(13, "steps", 1, True), (13, "full", 0, True), (14, "partial", 2, True),
                                                         (17, "full", 17, False), (20, "partial", 0, False)])
def test_native_cotangent_equals_the_route_through_stored_states(cuda_device, n_qubits, tape, variant, phase):
    """Same loss two ways: from the native overlaps (cotangent formed in the workspace by k_overlap_apply) and — the parent commit's
    route — by torch from the stored states of a second run (cotangent handed back as grad_states)."""
    terms = random_terms(n_qubits, 13, 0.002, seed=920 + n_qubits, local=False, phase=phase)
    tsave0 = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)
    psi = _random_psi0(n_qubits, 1).T.contiguous().to(cuda_device)
    tg = target_set(n_qubits, 1)
    n_t = len(tsave0)
    w = {k: _weights((3, n_t, 1), s).to(cuda_device) for k, s in (("abs", 21), ("re", 22), ("im", 23))}
    w["real"] = _weights((1, n_t, 1), 24).to(cuda_device)
    zd = R.total_magnetization_diag(n_qubits)[None].to(cuda_device)

    def run(native):
        amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=not native)
        if not phase:
            amp = amp.real.contiguous()  # a drive without phase: real tables, real_amp_grad
        spec.kernel_variant = variant
        spec.tape = tape
        if tape == "partial":
            spec.tape_steps = 2
        if native:
            spec.overlaps = pack_overlaps(tg, 2**n_qubits, 1, cuda_device)
        leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True), tsave0.clone().requires_grad_(True),
                  psi.clone().requires_grad_(True)]
        states, expect = evolve(*leaves, spec, zd)
        if native:
            real, ov = split_expect(expect, 3)
        else:
            real, ov = expect, torch.stack([overlap_states(ob, states.permute(0, 2, 1)) for ob in tg])
        return leaves, real, ov

    leaves_a, real_a, ov_a = run(True)
    leaves_b, real_b, ov_b = run(False)
    assert (ov_a - ov_b).abs().max().item() < ROUTE_TOL

    def placed(k):  # the weights at save point k only
        out = {}
        for name, v in w.items():
            out[name] = torch.zeros_like(v)
            out[name][:, k] = v[:, k]
        return out

    for weights, retain in ((placed(2), True), (placed(n_t - 1), True), (w, False)):
        ga = _grads_of(_loss(real_a, ov_a, weights), leaves_a, retain)
        gb = _grads_of(_loss(real_b, ov_b, weights), leaves_b, retain)
        torch.cuda.synchronize()
        for name, a, b in zip(("amp", "det", "u", "tsave", "psi0"), ga, gb):
            err = rel_err(a.cpu().numpy(), b.cpu().numpy())
            assert err < ROUTE_TOL, (name, err)


# ---- emulator and model -------------------------------------------------------------------------------------------------------
def test_emulator_in_the_rotating_frame_against_the_oracle(cuda_device):
    from tests.test_gpu_pauli_observables import _phase_sequence

    n = 4
    seq, coords = _phase_sequence(n)
    emu = P.TorchEmulator.from_sequence(seq, sampling_rate=0.2)
    assert emu._hamiltonian.frame_phase is not None
    obs = target_set(n, 1)[1]
    res = emu.run(solver=SolverType.KRYLOV_SE, observables=[obs], store_states=False)
    got = res.overlap(obs)
    assert got.shape == (len(emu.evaluation_times), 1) and got.dtype == torch.complex128
    oseq = R.concat_pulses([(R.blackman_waveform(200, 2.5), R.ramp_waveform(200, -4.0, 2.0), 0.3),
                            (R.constant_waveform(100, 5.0), R.constant_waveform(100, 1.0), 0.3)])
    ost = R.krylov_map_dense(R.build_terms(oseq, coords, 0.2), R.all_ground_state(n), emu.evaluation_times)
    assert np.abs(got.cpu().numpy() - ref_overlaps([obs], ost.numpy())[0]).max() < VALUE_ATOL
    assert np.abs(np.angle(got.cpu().numpy()[1:, 0])).max() > 1e-2  # a complex number: the frame would show
    res2 = emu.run(solver=SolverType.KRYLOV_SE)  # torch fallback on a stored-states run
    assert (res2.overlap(obs) - got).abs().max().item() < ROUTE_TOL
    proj = res.expect([obs])[0]
    assert (proj.real - (got.abs() ** 2).sum(-1)).abs().max().item() < 1e-14 and (res2.expect([obs])[0] - proj).abs().max().item() < ROUTE_TOL


def test_three_level_overlap_against_the_stored_states(cuda_device):
    from tests.test_host_logic import _three_level_emulator

    sim, _ = _three_level_emulator(compute_device="cuda", n=2)
    g = torch.Generator().manual_seed(4)
    phi = torch.randn(9, generator=g, dtype=torch.complex128)
    obs = StateOverlap(phi / phi.norm())
    res = sim.run(solver=SolverType.KRYLOV_SE, observables=[obs], store_states=False)
    stored = sim.run(solver=SolverType.KRYLOV_SE)
    got, want = res.overlap(obs), stored.overlap(obs)
    assert got.shape == want.shape == (len(sim.evaluation_times), 1)
    assert (got - want).abs().max().item() < ROUTE_TOL and want.abs().max().item() > 1e-2


def test_quantum_model_overlap_gradient_equals_the_forward_route(cuda_device):
    """One epoch of the 6-atom state preparation: d(1 - |c(T)|^2)/d(parameters) from model.overlap (no stored states) against the
    infidelity formed from model.forward()."""
    from pulser_diff_amd.utils import basis_state
    from tests.test_gpu_optimal_control import _device, _shaped_model, _state_infidelity

    torch.manual_seed(1)
    a0, d0 = 2 * torch.rand(30) - 1.0, 2 * torch.rand(30) - 1.0
    target = basis_state(2**6, 0).to(torch.complex128)
    grads, losses = [], []
    for native in (True, False):
        model = _shaped_model(_device(6.28), 6, 7.0, 30, 0.02, a0.clone(), d0.clone())
        if native:
            times, c = model.overlap(target)
            assert c.shape == (len(times), 1)
            loss = 1 - c[-1, 0].abs() ** 2
        else:
            loss = _state_infidelity(model, 6)
        loss.backward()
        grads.append(torch.cat([p.grad.reshape(-1) for _, p in sorted(model.named_parameters())]).cpu().numpy())
        losses.append(float(loss.detach()))
    assert abs(losses[0] - losses[1]) < VALUE_ATOL
    assert np.abs(grads[1]).max() > 1e-6 and rel_err(grads[0], grads[1]) < GRAD_RTOL


def test_sharded_runs_refuse_overlaps(cuda_device):
    n = 6
    terms = random_terms(n, 9, 0.002, seed=1, local=False)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
    spec.overlaps = pack_overlaps(target_set(n, 1)[:1], 2**n, 2, cuda_device)
    call = _Call(spec, amp, det, u, np.linspace(0, 0.01, 3), 2, None)
    call.problem.shard_bits = 1
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=cuda_device)
    info = _native.RydPlanInfo()
    with pytest.raises(NotImplementedError):
        _native.check(_native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream), ctypes.byref(info)))
