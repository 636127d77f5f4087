"""Adjoint passes in blocks of two factors per launch (k_chain2_bwd, pair_kernels.hpp): variant 17 forces them wherever legal (one
phase-free global drive, at most one detuning group, 13..20 qubits, real_amp_grad), variant 19 keeps the one-factor adjoint next
to the automatic forward blocks; both against the direct kernels (variant 1) — every gradient kind (amplitude, detuning, U_ij,
evaluation times, initial state) with expectation and state cotangents."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import random_terms, rel_err, to_native

pytestmark = pytest.mark.gpu

NAMES = ("states", "expect", "amp", "det", "u", "tsave", "psi0")


def _terms(n, n_samples, seed, det_groups, amp_scale=6.0):
    terms = random_terms(n, n_samples, 0.002, seed=seed, local=False, phase=False, amp_scale=amp_scale)
    if det_groups == 0:
        terms = R.HamTerms(terms.n_qubits, terms.u_pairs, terms.amp_coeff, None, terms.dt, terms.n_samples, terms.amp_targets, [])
    return terms


def _run(variant, terms, tsave, psi, device, obs, tape, zero_last, batch=1):
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    _native.set_kernel_variant(variant)
    try:
        amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE, batch_tables=batch)
        spec.tape = tape
        amp = amp.real.contiguous()  # a phase-free drive handed over as a real table: the real-drive adjoint
        if zero_last:
            amp[..., -1] = 0.0  # the padded last sample: amplitude exactly zero
        ts = tsave.clone().requires_grad_(True)
        ps = psi.clone().requires_grad_(True)
        for t_ in (amp, det, u):
            t_.requires_grad_(True)
        states, expect = evolve(amp, det, u, ts, ps, spec, obs)
        w = torch.linspace(0.5, 1.5, expect.shape[1], dtype=torch.float64, device=device)
        loss = (expect * w[None, :, None]).sum()
        gst = torch.linspace(-1.0, 1.0, states.numel(), dtype=torch.float64, device=device)
        loss = loss + 1e-3 * (states.real * gst.view(states.shape)).sum()  # state cotangents at every save point
        loss.backward()
        torch.cuda.synchronize()
        st = dict(spec.options["_last_stats"])
        grads = [amp.grad.cpu(), det.grad.cpu() if det.numel() else torch.zeros(0), u.grad.cpu(), ts.grad.cpu(), ps.grad.cpu()]
        return st, [states.detach().cpu(), expect.detach().cpu()] + grads
    finally:
        _native.set_kernel_variant(0)


def _compare(out):
    for v in (19, 17):
        for name, ref, got in zip(NAMES, out[1], out[v]):
            if ref.numel() == 0:  # no detuning group
                continue
            tol = 1e-12 if name == "states" else (1e-10 if name == "expect" else 1e-9)
            assert rel_err(got.numpy(), ref.numpy()) < tol, (v, name)
    for name, a, b in zip(NAMES, out[19], out[17]):
        if a.numel() == 0:
            continue
        assert np.abs((a - b).numpy()).max() <= 1e-8 * max(1.0, float(np.abs(a.numpy()).max())), name


def _case(device, n, det_groups, zero_last, batch, tsave, seed, amp_scale=6.0, tape="full"):
    terms = _terms(n, 13, seed, det_groups, amp_scale)
    gen = torch.Generator().manual_seed(seed)
    psi = torch.randn(batch, 2**n, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm(dim=1, keepdim=True)).to(device)
    obs = R.total_magnetization_diag(n)[None].to(device)
    out, stats = {}, {}
    for v in (1, 19, 17):
        stats[v], out[v] = _run(v, terms, tsave, psi, device, obs, tape, zero_last, batch)
        torch.cuda.empty_cache()
    assert stats[17]["kernel_bwd"].startswith("k_chain2_bwd<"), stats[17]
    assert not stats[19]["kernel_bwd"].startswith("k_chain2_bwd<"), stats[19]
    _compare(out)
    return stats[17]


# save points at irregular times (not at every step)
TS = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)


@pytest.mark.parametrize("n_qubits,det_groups,zero_last,batch", [(13, 1, False, 1), (16, 1, True, 1), (16, 0, False, 1),
                                                                 (16, 1, False, 2), (20, 1, True, 1), (20, 0, False, 1)])
def test_adjoint_blocks_match_one_factor_adjoint_and_direct_kernels(cuda_device, n_qubits, det_groups, zero_last, batch):
    _case(cuda_device, n_qubits, det_groups, zero_last, batch, TS, 700 + n_qubits + 10 * det_groups + batch)


def test_adjoint_blocks_on_the_recomputed_tape(cuda_device):
    """Tape per save point: the factor inputs of an interval are recomputed into the chain buffers, the blocks read them there."""
    _case(cuda_device, 16, 1, False, 1, TS, 777, tape="steps")


def test_adjoint_blocks_with_an_odd_plan_degree(cuda_device):
    """An exponential of odd degree starts (forward order) with a one-factor block: round B skipped, beta_a = 0."""
    for scale in (6.0, 3.0, 9.0, 1.5, 12.0, 4.5, 7.5):
        st = _case(cuda_device, 13, 1, False, 1, TS, 811, amp_scale=scale)
        if st["degree"] % 2 == 1:
            return
    pytest.fail("no amplitude scale gave an odd polynomial degree")


def test_adjoint_blocks_are_automatic_where_the_forward_blocks_are(cuda_device):
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    for n, variant, real, want in ((20, 0, True, True), (20, 17, True, True), (20, 18, True, False), (20, 19, True, False),
                                   (16, 0, True, False), (20, 17, False, False)):
        terms = random_terms(n, 5, 0.002, seed=3, local=False, phase=False)
        _native.set_kernel_variant(variant)
        try:
            amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=False)
            if real:
                amp = amp.real.contiguous()  # complex table: the adjoint needs both partner sums, k_chain keeps it
            amp.requires_grad_(True)
            psi = torch.zeros(1, 2**n, dtype=torch.complex128, device=cuda_device)
            psi[0, 0] = 1.0
            obs = R.total_magnetization_diag(n)[None].to(cuda_device)
            _, expect = evolve(amp, det, u, torch.tensor([0.0, 0.008], dtype=torch.float64), psi, spec, obs)
            expect[0, -1, 0].backward()
            torch.cuda.synchronize()
            bwd = spec.options["_last_stats"]["kernel_bwd"]
        finally:
            _native.set_kernel_variant(0)
        assert bwd.startswith("k_chain2_bwd<") == want, (n, variant, real, bwd)
