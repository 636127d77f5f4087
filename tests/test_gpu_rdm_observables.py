"""Reduced density matrices on the GPU: rho_A[k][b] = Tr_E |psi_b(t_k)><psi_b(t_k)| and its gradients through the C ABI
(pulser_diff_amd.solver.evolve), the emulator and QuantumModel, against the CPU oracle and against the route through stored states
and grad_states.

Bars (tests/test_gpu_solver_parity.py), with normalised states (|rho entries| <= 1): values vs the oracle 1e-9 absolute; gradients vs
oracle autograd 1e-8 relative to the largest entry; one native route against another 1e-10.  The reference matrices are the torch
route (observables.reduced_density_matrix) on the oracle's states; tests/test_rdm_observables_host.py pins that route against an
independent partial trace."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd.observables import PauliObservable, ReducedDensityMatrix, StateOverlap, pack_overlaps, reduced_density_matrix
from pulser_diff_amd.solver import SolverType, _Call, evolve, evolve_tangent, split_observables
from pulser_diff_amd.utils import purity
from tests.helpers import random_terms, rel_err, to_native

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9
GRAD_RTOL = 1e-8
ROUTE_TOL = 1e-10


def pauli_of(n):
    return PauliObservable(n, [(0.7, {j: "X"}) for j in range(n)] + [(-0.4, {0: "Y"})])


def overlap_of(n):
    phi = torch.randn(2**n, generator=torch.Generator().manual_seed(40 + n), dtype=torch.complex128)
    return StateOverlap(phi / phi.norm())


def subsystems(n):
    """One that contains qubit N-1 (index bit 0), one that contains qubit 0, a scrambled order, the whole register (N <= 6), every
    m from 1 to min(N, 6); the first eight (mixed m) make one call."""
    subs = [(n - 1,), (0,)]
    if n >= 2:
        subs.append((n - 1, 0))
    if n >= 6:
        subs.append((5, 1, 3))
    g = torch.Generator().manual_seed(n)
    for m in range(1, min(n, 6) + 1):
        subs.append(tuple(torch.randperm(n, generator=g)[:m].tolist()))
    if n <= 6:
        subs.append(tuple(reversed(range(n))))
    if n >= 3:
        subs.append((1, n - 1, 0))
    return [ReducedDensityMatrix(q) for q in subs]


def _random_psi0(n, batch):
    psi0 = torch.randn(2**n, batch, generator=torch.Generator().manual_seed(n), dtype=torch.complex128)
    return psi0 / psi0.norm(dim=0, keepdim=True)


def native_values(terms, tsave, psi_bd, device, rdms, variant=0, store_states=True, others=True):
    """-> states, real rows (diagonal, Pauli), complex overlap, list of rho (n_t, B, 2^m, 2^m)."""
    amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE, store_states=store_states)
    n = terms.n_qubits
    spec.rdms = rdms
    spec.kernel_variant = variant
    zd = None
    if others:
        spec.pauli = [pauli_of(n)]
        spec.overlaps = pack_overlaps([overlap_of(n)], 2**n, psi_bd.shape[0], device)
        zd = R.total_magnetization_diag(n)[None].to(device)
    states, expect = evolve(amp, det, u, tsave, psi_bd.to(device), spec, zd)
    torch.cuda.synchronize()
    assert expect.shape[0] == (4 if others else 0) + sum(2 * 4 ** o.n_sub for o in rdms)
    real, ov, rho = split_observables(expect, 1 if others else 0, rdms)
    return states, real, ov, rho


def check_values(real, ov, rho, rdms, ref_tdb, n, label):
    """Row offsets: the diagonal observable, the Pauli observable, Re / Im of the overlap, then the matrices."""
    ref = torch.as_tensor(ref_tdb)
    if real is not None and real.shape[0]:
        zd = R.total_magnetization_diag(n)
        assert (real[0].cpu() - (ref.abs() ** 2 * zd[None, :, None]).sum(1)).abs().max().item() < VALUE_ATOL * n
        if n <= 10:
            want_p = torch.einsum("tib,ij,tjb->tb", ref.conj(), pauli_of(n).to_dense(), ref).real
            assert (real[1].cpu() - want_p).abs().max().item() < VALUE_ATOL * (0.7 * n + 0.4)
        want_o = torch.einsum("d,tdb->tb", overlap_of(n).targets[:, 0].conj(), ref)
        assert (ov[0].cpu() - want_o).abs().max().item() < VALUE_ATOL
    for o, r in zip(rdms, rho):
        got = r.cpu()
        err = (got - reduced_density_matrix(o, ref)).abs().max().item()
        print(f"N={n} {label} A={o.qubits}: |native - oracle| = {err:.3e}")
        assert err < VALUE_ATOL, (n, label, o.qubits, err)
        d = torch.arange(2 ** o.n_sub)
        assert (got[:, :, d, d].imag == 0).all(), "Im rho[a][a] is an exact 0"
        assert (got - got.mH).abs().max().item() < 1e-13  # both triangles are written


@pytest.mark.parametrize("n_qubits,batch,variants", [(1, 1, (0,)), (3, 1, (0,)), (5, 3, (0,)), (6, 1, (0,)), (8, 1, (0,)), (10, 1, (0, 1))])
def test_values_match_dense_oracle(cuda_device, n_qubits, batch, variants):
    """A register smaller than a tile row (1 qubit), one-wave and one-workgroup sweeps, launch per factor (variant 1); every m, both
    reduction schemes (m <= 3, m >= 4), A = the whole register (one environment setting), eight matrices in one call; both
    store_states settings; next to a diagonal, a Pauli and an overlap observable."""
    terms = random_terms(n_qubits, 41, 0.004, seed=540 + n_qubits, local=True)
    tsave = torch.linspace(0, 0.16, 7, dtype=torch.float64)
    psi0 = _random_psi0(n_qubits, batch)
    ref = R.krylov_map_dense(terms, psi0, tsave)
    subs = subsystems(n_qubits)
    for v in variants:
        for store in (True, False):
            for first in range(0, len(subs), 8):
                rdms = subs[first:first + 8]
                _, real, ov, rho = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, rdms, variant=v, store_states=store)
                check_values(real, ov, rho, rdms, ref, n_qubits, f"B={batch} variant {v} store={store}")
    if n_qubits >= 3:
        assert len(subs) >= 8 and len({o.n_sub for o in subs[:8]}) >= 3  # the eight-matrix call mixes m


@pytest.mark.parametrize("n_qubits,variants", [(12, (0, 1)), (14, (0, 2))])
def test_values_match_matrix_free_oracle(cuda_device, n_qubits, variants):
    """12 qubits: the last one-launch size, one tile per state.  14: the chained family, four tiles per state: A = {0, 1, N-1} has two
    bits above the tile and index bit 0; the m = 6 subsystem has qubits on both sides of index bit 12."""
    terms = random_terms(n_qubits, 7, 0.002, seed=640 + n_qubits, local=True)  # (short run: the CPU oracle is the cost of this test)
    tsave = torch.linspace(0, 0.011, 5, dtype=torch.float64)
    psi0 = R.all_ground_state(n_qubits)
    ref = R.krylov_map_matrix_free(terms, psi0.numpy(), tsave.numpy(), save_all=True, tol=1e-14)
    rdms = [ReducedDensityMatrix((0, 1, n_qubits - 1)), ReducedDensityMatrix((n_qubits - 1, 2, 0, 9, 1, 5)), ReducedDensityMatrix((n_qubits - 2,))]
    for v in variants:
        for store in (True, False):
            _, real, ov, rho = native_values(terms, tsave, psi0.T.contiguous(), cuda_device, rdms, variant=v, store_states=store)
            check_values(real, ov, rho, rdms, ref, n_qubits, f"variant {v} store={store}")


def _raw_final_state_only(terms, tsave, psi_bd, device, rdms):
    """rydiff_forward with final_state_only through ctypes: matrices at every save point, one state out."""
    amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE)
    spec.rdms = rdms
    call = _Call(spec, amp, det, u, tsave.numpy(), psi_bd.shape[0], None)
    call.problem.final_state_only = 1
    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=device)
    info = _native.RydPlanInfo()
    _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()), stream, ctypes.byref(info)))
    ws = torch.empty(info.workspace_bytes, dtype=torch.uint8, device=device)
    last = torch.empty((1,) + tuple(psi_bd.shape), dtype=torch.complex128, device=device)
    expect = torch.empty((spec.rdm_rows(), len(tsave), psi_bd.shape[0]), dtype=torch.float64, device=device)
    _native.check(L.rydiff_forward(ctypes.byref(call.problem), ctypes.byref(info), ctypes.c_void_p(psi_bd.data_ptr()),
                                   ctypes.c_void_p(last.data_ptr()), ctypes.c_void_p(expect.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                   ctypes.c_size_t(ws.numel()), 0, stream))
    torch.cuda.synchronize()
    return split_observables(expect, 0, rdms)[2]


@pytest.mark.parametrize("n_qubits,batch", [(13, 2), (16, 1)])
def test_native_values_equal_torch_on_the_stored_states(cuda_device, n_qubits, batch):
    """The reductions alone (2 and 16 tiles per state, a batch): the torch route on the same run's stored states; store_states=False
    and final_state_only give the same numbers."""
    terms = random_terms(n_qubits, 9, 0.002, seed=740 + n_qubits, local=True)
    tsave = torch.linspace(0, 0.014, 4, dtype=torch.float64)
    psi = _random_psi0(n_qubits, batch).T.contiguous().to(cuda_device)
    rdms = [ReducedDensityMatrix(q) for q in ((n_qubits - 1,), (3, 0, n_qubits - 1), (12, 7, 0, 2), (n_qubits - 1, 1, 6, 0, 11, 4))]
    states, _, _, rho = native_values(terms, tsave, psi, cuda_device, rdms, others=False)
    for o, r in zip(rdms, rho):
        err = (r - reduced_density_matrix(o, states.permute(0, 2, 1))).abs().max().item()
        print(f"N={n_qubits} A={o.qubits}: |native - torch on stored states| = {err:.3e}")
        assert err < ROUTE_TOL, (n_qubits, o.qubits, err)
    del states
    _, _, _, rho2 = native_values(terms, tsave, psi, cuda_device, rdms, others=False, store_states=False)
    rho3 = _raw_final_state_only(terms, tsave, psi, cuda_device, rdms)
    for a, b, c in zip(rho, rho2, rho3):
        assert (a - b).abs().max().item() < ROUTE_TOL and (a - c).abs().max().item() < ROUTE_TOL


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def _weights(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _loss(rho, w):
    """A random real-linear functional of all 2 * 4^m rows at every save point, plus sum_k purity_k."""
    out = 0.0
    for r, (wr, wi) in zip(rho, w):
        out = out + (wr.to(r.device) * r.real).sum() + (wi.to(r.device) * r.imag).sum() + purity(r).sum()
    return out


@pytest.mark.parametrize("n_qubits,batch,store", [(4, 1, True), (6, 1, False), (8, 1, True), (10, 1, False), (5, 3, False)])
def test_gradients_match_oracle_autograd(cuda_device, n_qubits, batch, store):
    """m = 1, 3 and (where the register has them) 6, scrambled: g_amp (complex tables), g_det, g_u, g_tsave, g_psi0 against torch
    autograd through the oracle's dense map and the torch route."""
    n_samples, dt = 33, 0.004
    terms = random_terms(n_qubits, n_samples, dt, seed=840 + n_qubits, local=True)
    n_t = 5 if n_qubits >= 10 else 9
    tsave0 = torch.linspace(0, dt * (n_samples - 1), n_t, dtype=torch.float64)
    tsave0 = tsave0 + torch.cat([torch.zeros(1), 0.0007 * torch.rand(n_t - 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64), torch.zeros(1)])
    psi0 = _random_psi0(n_qubits, batch)
    rdms = [ReducedDensityMatrix((n_qubits - 1,)), ReducedDensityMatrix((n_qubits - 1, 0, 2))]
    if n_qubits >= 6:
        rdms.append(ReducedDensityMatrix((5, 1, 3, 0, 4, 2) if n_qubits == 6 else (n_qubits - 1, 1, 3, 0, 6, 4)))
    w = [(_weights((n_t, batch, 2 ** o.n_sub, 2 ** o.n_sub), 11 + i), _weights((n_t, batch, 2 ** o.n_sub, 2 ** o.n_sub), 21 + i))
         for i, o in enumerate(rdms)]

    o_terms = R.HamTerms(n_qubits, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                         terms.det_coeff.clone().requires_grad_(True), dt, n_samples, terms.amp_targets, terms.det_targets)
    o_terms.extra_amp = [(a.clone().requires_grad_(True), t) for a, t in terms.extra_amp]
    o_terms.extra_det = [(a.clone().requires_grad_(True), t) for a, t in terms.extra_det]
    o_ts = tsave0.clone().requires_grad_(True)
    o_psi = psi0.clone().requires_grad_(True)
    o_states = R.krylov_map_dense(o_terms, o_psi, o_ts)  # (n_t, dim, B)
    o_rho = [reduced_density_matrix(o, o_states) for o in rdms]
    _loss(o_rho, w).backward()
    o_amp = torch.stack([a.grad for a, _ in o_terms.amp_terms()])
    o_det = torch.stack([a.grad for a, _ in o_terms.det_terms()])

    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=store, batch_tables=batch)
    spec.rdms = rdms
    for t in (amp, det, u):
        t.requires_grad_(True)
    ts = tsave0.clone().requires_grad_(True)
    psi_bd = psi0.T.contiguous().to(cuda_device).requires_grad_(True)
    _, expect = evolve(amp, det, u, ts, psi_bd, spec, None)
    _, _, rho = split_observables(expect, 0, rdms)
    for a, b in zip(rho, o_rho):
        assert (a.detach().cpu() - b.detach()).abs().max().item() < VALUE_ATOL
    _loss(rho, w).backward()
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


@pytest.mark.parametrize("n_qubits,tape,variant", [(13, "steps", 1), (13, "full", 0), (14, "partial", 2)])
def test_native_cotangent_equals_the_route_through_stored_states(cuda_device, n_qubits, tape, variant):
    """Same loss two ways: from the native matrices (cotangent formed in the workspace by k_rdm_apply) and by torch from the stored
    states of a second run (cotangent handed back as grad_states).  Once with weights at a single interior save point only: every
    other save point takes the kernel's skip path."""
    terms = random_terms(n_qubits, 13, 0.002, seed=940 + n_qubits, local=False)
    tsave0 = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)
    psi = _random_psi0(n_qubits, 1).T.contiguous().to(cuda_device)
    rdms = [ReducedDensityMatrix((0, 1, n_qubits - 1)), ReducedDensityMatrix((n_qubits - 1, 2, 0, 9, 1, 5)), ReducedDensityMatrix((4,))]
    n_t = len(tsave0)
    w = [(_weights((n_t, 1, 2 ** o.n_sub, 2 ** o.n_sub), 31 + i).to(cuda_device), _weights((n_t, 1, 2 ** o.n_sub, 2 ** o.n_sub), 41 + i).to(cuda_device))
         for i, o in enumerate(rdms)]

    def run(native):
        amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=not native)
        spec.kernel_variant = variant
        spec.tape = tape
        if tape == "partial":
            spec.tape_steps = 2
        if native:
            spec.rdms = rdms
        leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True), tsave0.clone().requires_grad_(True),
                  psi.clone().requires_grad_(True)]
        states, expect = evolve(*leaves, spec, None)
        rho = split_observables(expect, 0, rdms)[2] if native else [reduced_density_matrix(o, states.permute(0, 2, 1)) for o in rdms]
        return leaves, rho

    leaves_a, rho_a = run(True)
    leaves_b, rho_b = run(False)
    for a, b in zip(rho_a, rho_b):
        assert (a - b).abs().max().item() < ROUTE_TOL

    def linear_at(rho, k):  # the linear functional at save point k only (no purity: zero cotangent everywhere else)
        return sum((wr[k] * r[k].real).sum() + (wi[k] * r[k].imag).sum() for r, (wr, wi) in zip(rho, w))

    for loss_of, retain in ((lambda rho: linear_at(rho, 2), True), (lambda rho: _loss(rho, w), False)):
        ga = _grads_of(loss_of(rho_a), leaves_a, retain)
        gb = _grads_of(loss_of(rho_b), leaves_b, retain)
        torch.cuda.synchronize()
        for name, a, b in zip(("amp", "det", "u", "tsave", "psi0"), ga, gb):
            err = rel_err(a.cpu().numpy(), b.cpu().numpy())
            print(f"N={n_qubits} tape {tape} variant {variant} {name}: rel err {err:.3e}")
            assert err < ROUTE_TOL, (name, err)


# ---- emulator and model -------------------------------------------------------------------------------------------------------
def test_emulator_in_the_rotating_frame_against_the_oracle(cuda_device):
    from tests.test_gpu_pauli_observables import _phase_sequence

    n = 4
    seq, coords = _phase_sequence(n)
    emu = P.TorchEmulator.from_sequence(seq, sampling_rate=0.2)
    assert emu._hamiltonian.frame_phase is not None
    obs = emu.build_reduced_density_matrix(["q3", "q0"])
    assert obs.qubits == (3, 0)
    single = emu.build_reduced_density_matrix(["q1"])
    res = emu.run(solver=SolverType.KRYLOV_SE, observables=[obs, single], store_states=False)
    got = res.reduced_density_matrix(obs)
    assert got.shape == (len(emu.evaluation_times), 1, 4, 4) and got.dtype == torch.complex128
    oseq = R.concat_pulses([(R.blackman_waveform(200, 2.5), R.ramp_waveform(200, -4.0, 2.0), 0.3),
                            (R.constant_waveform(100, 5.0), R.constant_waveform(100, 1.0), 0.3)])
    ost = R.krylov_map_dense(R.build_terms(oseq, coords, 0.2), R.all_ground_state(n), emu.evaluation_times)
    want = reduced_density_matrix(obs, ost)
    assert (got.cpu() - want).abs().max().item() < VALUE_ATOL
    assert (res.reduced_density_matrix(single).cpu() - reduced_density_matrix(single, ost)).abs().max().item() < VALUE_ATOL
    # an off-diagonal entry between settings with different numbers of ones: the frame phase (0.3) would show
    assert want[-1, 0, 0, 1].abs().item() > 1e-3 and (want[-1, 0, 0, 1] * (1 - np.exp(0.3j))).abs().item() > 100 * VALUE_ATOL
    res2 = emu.run(solver=SolverType.KRYLOV_SE)  # torch route on a stored-states run
    assert (res2.reduced_density_matrix(obs) - got).abs().max().item() < ROUTE_TOL
    s_native, s_stored = res.entanglement_entropy(obs), res2.entanglement_entropy(obs)
    # x log x is not Lipschitz at 0 (the early, nearly pure states): eigenvalues that differ by d = ROUTE_TOL move it by at most
    # d (1 + |ln d|) = 2.4e-9 each, / ln 2, four of them: 1.4e-8
    assert s_native.shape == (len(emu.evaluation_times), 1) and (s_native - s_stored).abs().max().item() < 1.4e-8
    with pytest.raises(NotImplementedError):
        emu.run_sensitivities([torch.zeros(1, requires_grad=True)], [obs], solver=SolverType.KRYLOV_SE)


def _model_grads(loss_of):
    from tests.test_gpu_optimal_control import _device, _shaped_model

    torch.manual_seed(1)
    a0, d0 = 2 * torch.rand(30) - 1.0, 2 * torch.rand(30) - 1.0
    grads, losses = [], []
    for native in (True, False):
        model = _shaped_model(_device(6.28), 6, 7.0, 30, 0.02, a0.clone(), d0.clone())
        loss = loss_of(model, native)
        loss.backward()
        grads.append(torch.cat([p.grad.reshape(-1) for _, p in sorted(model.named_parameters())]).cpu().numpy())
        losses.append(float(loss.detach()))
    return grads, losses


def test_quantum_model_rdm_gradient_equals_the_stored_states_route(cuda_device):
    """One epoch of the 6-atom chain: d purity(rho_A(T)) / d(parameters), A = half the chain in scrambled order, from
    model.reduced_density_matrix (no stored states) against the torch route on model.forward()'s states."""
    obs = ReducedDensityMatrix((2, 0, 1))

    def loss_of(model, native):
        if native:
            times, rho = model.reduced_density_matrix(obs.qubits)
            assert rho.shape == (len(times), 1, 8, 8)
            return purity(rho[-1, 0])
        _, states = model.forward()
        return purity(reduced_density_matrix(obs, states)[-1, 0])

    grads, losses = _model_grads(loss_of)
    assert abs(losses[0] - losses[1]) < ROUTE_TOL and losses[0] < 1 - 1e-3  # entangled
    assert np.abs(grads[1]).max() > 1e-6 and rel_err(grads[0], grads[1]) < ROUTE_TOL


def test_entanglement_entropy_gradient_equals_the_stored_states_route(cuda_device):
    """results.entanglement_entropy of one atom at the final time (a generic, non-degenerate spectrum), native against stored states."""
    obs = ReducedDensityMatrix((3,))

    def loss_of(model, native):
        _, results = model._run(observables=[obs], store_states=False) if native else model._run()
        s = results.entanglement_entropy(obs)
        assert s.shape[1] == 1
        return s[-1, 0]

    grads, losses = _model_grads(loss_of)
    assert abs(losses[0] - losses[1]) < ROUTE_TOL and 1e-3 < losses[0] <= 1.0
    assert np.abs(grads[1]).max() > 1e-6 and rel_err(grads[0], grads[1]) < ROUTE_TOL


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_sharded_runs_refuse_rdms(cuda_device):
    n = 6
    terms = random_terms(n, 9, 0.002, seed=1, local=False)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
    spec.rdms = [ReducedDensityMatrix((2, 5))]
    call = _Call(spec, amp, det, u, np.linspace(0, 0.01, 3), 2, None)
    call.problem.shard_bits = 1
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=cuda_device)
    info = _native.RydPlanInfo()
    with pytest.raises(NotImplementedError, match="reduced density"):
        _native.check(_native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream), ctypes.byref(info)))


def test_tangent_sweep_refuses_rdms(cuda_device):
    n = 4
    terms = random_terms(n, 9, 0.002, seed=2, local=False)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
    spec.rdms = [ReducedDensityMatrix((1,))]
    psi = _random_psi0(n, 1).T.contiguous().to(cuda_device)
    with pytest.raises(NotImplementedError, match="reduced density"):
        evolve_tangent(amp, det, u, torch.linspace(0, 0.01, 3, dtype=torch.float64), psi, spec, d_amp=torch.ones_like(amp)[None])
    call = _Call(spec, amp, det, u, np.linspace(0, 0.01, 3), 1, None)  # and the library itself
    tg = _native.RydTangent()
    tg.n_dir = 1
    rc = _native.lib().rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(_native.RydPlanInfo()), ctypes.byref(tg), None, None,
                                              None, None, 0, None)
    assert rc == _native.RYDIFF_ENOTIMPL and "reduced density" in _native.last_error()


def test_master_equation_and_three_level_runs_refuse_rdms(cuda_device):
    from tests.test_gpu_pauli_observables import _phase_sequence
    from tests.test_host_logic import _three_level_emulator

    seq, _ = _phase_sequence(2)
    emu = P.TorchEmulator.from_sequence(seq, sampling_rate=0.2)
    obs = ReducedDensityMatrix((0,))
    with pytest.raises(NotImplementedError, match="master-equation"):
        emu.run(solver=SolverType.DP5_ME, observables=[obs])
    sim, _ = _three_level_emulator(compute_device="cuda", n=2)
    with pytest.raises(NotImplementedError, match="three-level"):
        sim.run(solver=SolverType.KRYLOV_SE, observables=[obs], store_states=False)
