"""Gradient w.r.t. the evaluation times (g_tsave) of NATIVELY driven state-sharded runs (rydiff_backward with shard_bits and
g_tsave; pulser_diff_amd.sharded.grad_virtual_native / grad_distributed_native with time_grad=True) on one GPU: against the
oracle's goldens, against the single-GPU adjoint (KRYLOV_SE and DP5_SE), with the ranks in separate processes, and a guard that
the other four gradients do not move when the time gradient is asked for.  Evaluation times lie off the sample grid everywhere.
Bars: 1e-8 relative against the oracle's goldens, 1e-9 relative sharded against un-sharded (the suite's own)."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import restatement as R
from pulser_diff_amd.sharded import ShardedProblem
from tests.helpers import mask_of, random_terms, rel_err, to_native, unpack_terms
from tests.test_gpu_baseline_fixtures import _load, _z_diag
from tests.test_gpu_sharded import _problem

pytestmark = pytest.mark.gpu


def _off_grid(t_end, n):
    """n evaluation times on [0, ~t_end]: evenly spaced, then shifted by uneven fractions of a millisecond (t_0 stays 0)."""
    shift = torch.tensor([0.0, 0.3, -0.2, 0.4, 0.15, -0.35, 0.25], dtype=torch.float64)[:n] * 1e-3
    return torch.linspace(0, t_end, n, dtype=torch.float64) + shift


def _single_gpu(terms, tsave, w, device, solver, tol=0.0, psi0=None):
    """Un-sharded adjoint of the same problem: expectation values and all five gradients."""
    from pulser_diff_amd.solver import evolve

    n = terms.n_qubits
    amp, det, u, spec = to_native(terms, device, solver, tol=tol)
    for t in (amp, det, u):
        t.requires_grad_(True)
    ts = tsave.clone().requires_grad_(True)
    if psi0 is None:
        psi0 = R.all_ground_state(n).T.contiguous()
    psi0 = psi0.to(device).requires_grad_(True)
    zd = R.total_magnetization_diag(n).to(device)
    _, expect = evolve(amp, det, u, ts, psi0, spec, zd[None])
    (expect[0, :, 0] * w.to(device)).sum().backward()
    return {"expect": expect[0, :, 0].detach().cpu().numpy(), "g_amp": amp.grad[0].cpu().numpy(), "g_det": det.grad[0].cpu().numpy(),
            "g_u": u.grad.cpu().numpy(), "g_tsave": ts.grad.numpy(), "g_psi0": psi0.grad[0].cpu().numpy()}


def _report(tag, out, ref, real_amp=False):
    errs = {"g_amp": rel_err(out["g_amp"].real, ref["g_amp"].real) if real_amp else rel_err(out["g_amp"], ref["g_amp"]),
            "g_det": rel_err(out["g_det"], ref["g_det"]), "g_u": rel_err(out["g_u"], ref["g_u"]),
            "g_tsave": rel_err(out["g_tsave"], ref["g_tsave"]), "g_psi0": rel_err(out["g_psi0"].cpu().numpy(), ref["g_psi0"]),
            "expect": float(np.abs(out["expect"].cpu().numpy() - ref["expect"]).max())}
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    return errs


# ---- 4. oracle goldens --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,g,family", [("grad_dense_n8", 1, "direct"), ("grad_dense_n8", 3, "direct"), ("grad_dense_n10", 2, "direct"),
                                           ("grad_mf_n14", 1, "chained-tiles"), ("grad_mf_n14", 2, "direct"),
                                           ("grad_mf_n14_real", 1, "chained-tiles")])
def test_native_sharded_time_gradient_matches_oracle_golden(cuda_device, name, g, family):
    """g_tsave of the natively driven sharded reverse sweep against autograd through the oracle (dense exponential at 8 / 10 qubits,
    matrix-free Taylor map at 14) for the loss sum_k w_k <sum Z>(t_k): irregular off-grid times, a global and a local drive with
    phases, a detuning term on a rank qubit and a slab qubit.  13-qubit slabs: run_chain_bwd's call site of k_dot_hx; up to 12:
    adjoint_direct's.  grad_mf_n14_real: phase-free tables, the adjoint instantiation without signed sums."""
    from pulser_diff_amd.sharded import grad_virtual_native

    fx = _load(name)
    terms = unpack_terms(fx)
    n = terms.n_qubits
    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    prob = ShardedProblem(n, g, terms.dt, np.stack([c.numpy() for c, _ in amp_terms]), np.stack([c.numpy() for c, _ in det_terms]),
                          [mask_of(tg) for _, tg in amp_terms], [mask_of(tg) for _, tg in det_terms], terms.u_pairs.numpy(), tol=1e-13)
    out = grad_virtual_native(prob, torch.as_tensor(fx["psi0"]).to(cuda_device), fx["tsave"], _z_diag(n, cuda_device), fx["w"],
                              time_grad=True)
    err = rel_err(out["g_tsave"], fx["g_tsave_A"])
    print(f"{name} g={g}: g_tsave rel err {err:.2e} ({out['stats']['kernel_bwd']})")
    assert out["stats"]["kernel_family"] == family
    assert np.abs(out["expect"].cpu().numpy() - fx["z_t"]).max() < 1e-9
    assert out["g_tsave"].shape == fx["g_tsave_A"].shape
    assert err < 1e-8


# ---- 5. single-GPU adjoint, KRYLOV_SE -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_qubits,g,variant,tape", [(6, 1, 0, 1), (11, 2, 0, 1), (13, 3, 0, 1), (15, 2, 0, 1), (16, 3, 0, 1), (16, 3, 2, 1), (17, 1, 0, 1),
                                                     (16, 2, 1, 1), (17, 3, 14, 1), (16, 2, 14, 1)])
def test_native_sharded_five_gradients_match_single_gpu_adjoint(cuda_device, n_qubits, g, variant, tape):
    """All four older gradients AND g_tsave of the native sharded sweep against the single-GPU adjoint of the un-sharded problem."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.sharded import grad_virtual_native
    from pulser_diff_amd.solver import SolverType

    terms, prob = _problem(n_qubits, g, seed=60 + n_qubits)
    tsave = _off_grid(0.02, 5)
    w = torch.linspace(-0.3, 1.2, len(tsave), dtype=torch.float64)
    ref = _single_gpu(terms, tsave, w, cuda_device, SolverType.KRYLOV_SE)
    zd = R.total_magnetization_diag(n_qubits).to(cuda_device)
    _native.set_kernel_variant(variant)
    try:
        out = grad_virtual_native(prob, R.all_ground_state(n_qubits)[:, 0].to(cuda_device), tsave.numpy(), zd, w.numpy(), time_grad=True)
    finally:
        _native.set_kernel_variant(0)
    errs = _report(f"krylov ({n_qubits},{g},{variant}):", out, ref)
    assert out["stats"]["kernel_family"] == ("chained-tiles" if (n_qubits - g > 12 and variant != 1) else "direct")
    assert errs["expect"] < 1e-10
    for key in ("g_amp", "g_det", "g_u", "g_tsave", "g_psi0"):
        assert errs[key] < 1e-9, key


@pytest.mark.parametrize("n_qubits,g,variant", [(16, 3, 0), (17, 3, 14)])
def test_native_sharded_five_gradients_of_a_phase_free_global_drive(cuda_device, n_qubits, g, variant):
    """The same through the adjoint instantiation without signed sums (one global drive without phase)."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.sharded import grad_virtual_native
    from pulser_diff_amd.solver import SolverType

    terms = random_terms(n_qubits, 17, 0.002, seed=777, local=False, phase=False)
    all_mask = (1 << n_qubits) - 1
    prob = ShardedProblem(n_qubits, g, terms.dt, terms.amp_coeff.numpy()[None], terms.det_coeff.numpy()[None], [all_mask], [all_mask],
                          terms.u_pairs.numpy(), tol=1e-13)
    tsave = _off_grid(0.03, 6)
    w = torch.linspace(0.4, -0.9, len(tsave), dtype=torch.float64)
    ref = _single_gpu(terms, tsave, w, cuda_device, SolverType.KRYLOV_SE)
    zd = R.total_magnetization_diag(n_qubits).to(cuda_device)
    _native.set_kernel_variant(variant)
    try:
        out = grad_virtual_native(prob, R.all_ground_state(n_qubits)[:, 0].to(cuda_device), tsave.numpy(), zd, w.numpy(), time_grad=True)
    finally:
        _native.set_kernel_variant(0)
    errs = _report(f"phase-free ({n_qubits},{g},{variant}):", out, ref, real_amp=True)
    assert out["stats"]["kernel_family"] == "chained-tiles"
    assert errs["expect"] < 1e-10
    for key in ("g_amp", "g_det", "g_u", "g_tsave", "g_psi0"):
        assert errs[key] < 1e-9, key


# ---- 6. DP5_SE --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_qubits,g,final_only", [(9, 2, False), (15, 2, True), (16, 3, False)])
def test_native_sharded_dp5_matches_single_gpu_dp5(cuda_device, n_qubits, g, final_only):
    """The continuous-time solver (an interval = many exponentials, interpolation weights on both ends) on slabs: expectation
    values and all five gradients against evolve(..., DP5_SE) of the un-sharded problem at the same tolerance."""
    from pulser_diff_amd.sharded import grad_virtual_native
    from pulser_diff_amd.solver import SolverType

    tol = 1e-9
    terms, prob = _problem(n_qubits, g, seed=160 + n_qubits)
    prob = dataclasses.replace(prob, tol=tol)
    tsave = _off_grid(0.02, 5)
    w = torch.linspace(-0.3, 1.2, len(tsave), dtype=torch.float64)
    if final_only:  # the cotangent on the final time only
        w = torch.zeros(len(tsave), dtype=torch.float64)
        w[-1] = 1.0
    ref = _single_gpu(terms, tsave, w, cuda_device, SolverType.DP5_SE, tol=tol)
    zd = R.total_magnetization_diag(n_qubits).to(cuda_device)
    out = grad_virtual_native(prob, R.all_ground_state(n_qubits)[:, 0].to(cuda_device), tsave.numpy(), zd, w.numpy(), time_grad=True,
                              solver=SolverType.DP5_SE)
    errs = _report(f"dp5 ({n_qubits},{g}) factors {out['stats']['total_factors']}:", out, ref)
    assert out["stats"]["kernel_family"] == ("chained-tiles" if n_qubits - g > 12 else "direct")
    assert errs["expect"] < 1e-10
    for key in ("g_amp", "g_det", "g_u", "g_tsave", "g_psi0"):
        assert errs[key] < 1e-9, key


# ---- 7. ranks in separate processes ------------------------------------------------------------------------------------
def _time_grad_worker(rank, world, port, n_qubits, g, seed, out_q, backend="gloo"):
    import datetime
    import os

    import torch.distributed as dist

    from pulser_diff_amd.sharded import grad_distributed_native

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "nccl":
        dev = torch.device("cuda", rank)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=datetime.timedelta(seconds=120))
    else:
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        terms, prob = _problem(n_qubits, g, seed=seed)
        tsave = _off_grid(0.02, 5).numpy()
        psi0 = R.all_ground_state(n_qubits)[:, 0]
        dloc = 2 ** (n_qubits - g)
        zd = R.total_magnetization_diag(n_qubits)
        w = np.linspace(-0.3, 1.2, len(tsave))
        args = (prob, psi0[rank * dloc:(rank + 1) * dloc].to(dev), tsave, zd[rank * dloc:(rank + 1) * dloc].to(dev), w)
        plain = grad_distributed_native(*args)
        timed = grad_distributed_native(*args, time_grad=True)
        out_q.put((rank, timed["g_tsave"], timed["g_amp"], timed["g_det"], timed["g_u"], "g_tsave" in plain,
                   plain["stats"]["exchange_posts"], timed["stats"]["exchange_posts"], timed["stats"]["kernel_family"]))
    finally:
        dist.destroy_process_group()


def _run_ranks(n_qubits, g, seed, backend):
    import socket

    import torch.multiprocessing as mp

    world = 2**g
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_time_grad_worker, args=(r, world, port, n_qubits, g, seed, q, backend)) for r in range(world)]
    for p_ in procs:
        p_.start()
    try:
        results = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    finally:
        for p_ in procs:
            p_.join(timeout=60)
            if p_.is_alive():
                p_.kill()
    assert all(p_.exitcode == 0 for p_ in procs)
    return results


def _check_ranks(results, n_qubits, g, seed, device):
    from pulser_diff_amd.solver import SolverType

    terms, _ = _problem(n_qubits, g, seed=seed)
    tsave = _off_grid(0.02, 5)
    ref = _single_gpu(terms, tsave, torch.linspace(-0.3, 1.2, len(tsave), dtype=torch.float64), device, SolverType.KRYLOV_SE)
    for r in results:  # every rank holds the all-reduced time gradient
        err = rel_err(r[1], ref["g_tsave"])
        print(f"rank {r[0]} of ({n_qubits},{g}): g_tsave rel err {err:.2e}, exchanges posted {r[6]} without / {r[7]} with time_grad")
        assert r[1].shape == (len(tsave),) and err < 1e-9
        assert rel_err(r[2], ref["g_amp"]) < 1e-9 and rel_err(r[3], ref["g_det"]) < 1e-9 and rel_err(r[4], ref["g_u"]) < 1e-9
        assert not r[5]                 # no "g_tsave" unless asked for
        assert r[6] > 0 and r[7] == r[6]  # the time gradient costs no slab exchange
        assert r[8] == ("chained-tiles" if n_qubits - g > 12 else "direct")


@pytest.mark.parametrize("n_qubits,g", [(9, 1), (15, 2)])
def test_native_sharded_time_gradient_over_processes(cuda_device, n_qubits, g):
    """One slab per process (all on the one GPU, gloo as transport): k_dot_hx reads the RECEIVED cotangent slabs; g_tsave rides in
    the one packed all-reduce; a run with time_grad posts exactly as many slab exchanges as one without."""
    seed = 800 + n_qubits
    _check_ranks(_run_ranks(n_qubits, g, seed, "gloo"), n_qubits, g, seed, cuda_device)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="the RCCL path needs one GPU per rank")
def test_native_sharded_time_gradient_over_rccl(cuda_device):
    """RCCL twin: one GPU per rank, cotangent slabs over xGMI.  Bounded by the ranks' 120 s collective timeout and the 240 s
    queue timeout."""
    _check_ranks(_run_ranks(15, 1, 950, "nccl"), 15, 1, 950, cuda_device)


# ---- 8. what must not move ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_qubits,g", [(11, 2), (15, 2)])
def test_time_grad_leaves_the_other_gradients_alone(cuda_device, n_qubits, g):
    """With and without time_grad the sweep issues the same adjoint launches; the results differ by the order of fp64 atomic adds
    only: 1e-12 relative (two orders above the 1e-14 seen between sweeps of one kernel family)."""
    from pulser_diff_amd.sharded import grad_virtual_native

    terms, prob = _problem(n_qubits, g, seed=60 + n_qubits)
    tsave = _off_grid(0.02, 5)
    w = np.linspace(-0.3, 1.2, len(tsave))
    zd = R.total_magnetization_diag(n_qubits).to(cuda_device)
    psi0 = R.all_ground_state(n_qubits)[:, 0].to(cuda_device)
    plain = grad_virtual_native(prob, psi0, tsave.numpy(), zd, w)
    timed = grad_virtual_native(prob, psi0, tsave.numpy(), zd, w, time_grad=True)
    assert "g_tsave" not in plain and "g_tsave" in timed
    for key in ("g_amp", "g_det", "g_u"):
        err = rel_err(plain[key], timed[key])
        print(f"({n_qubits},{g}) {key}: {err:.2e}")
        assert err < 1e-12, key
    for key in ("g_psi0", "expect"):
        err = rel_err(plain[key].cpu().numpy(), timed[key].cpu().numpy())
        print(f"({n_qubits},{g}) {key}: {err:.2e}")
        assert err < 1e-12, key
