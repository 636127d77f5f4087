"""Block-of-two forward passes (k_chain2, pair_kernels.hpp): two factors of one exponential per launch, three vectors per layout
change.  Variant 17 forces them wherever legal (one phase-free global drive, at most one detuning group, 13..20 qubits), variant 18
keeps the one-factor chain; both against the direct kernels (variant 1) — states at every save point, <O> at every step, every
gradient kind with both tape modes."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import random_terms, rel_err, to_native

pytestmark = pytest.mark.gpu


def _run(variant, terms, tsave, psi, device, obs, tape, zero_last):
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    _native.set_kernel_variant(variant)
    try:
        amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE)
        spec.tape = tape
        amp = amp.real.contiguous()  # a phase-free drive handed over as a real table
        if zero_last:
            amp[..., -1, :] = 0.0  # the padded last sample: amplitude exactly zero
        ts = tsave.clone().requires_grad_(True)
        ps = psi.clone().requires_grad_(True)
        for t_ in (amp, det, u):
            t_.requires_grad_(True)
        states, expect = evolve(amp, det, u, ts, ps, spec, obs)
        w = torch.linspace(0.5, 1.5, expect.shape[1], dtype=torch.float64, device=device)
        loss = (expect[0] * w[:, None]).sum()
        gst = torch.linspace(-1.0, 1.0, states.numel() // 2 * 2, dtype=torch.float64, device=device)[: states.numel()]
        loss = loss + 1e-3 * (states.real * gst.view(states.shape)).sum()  # state cotangents at every save point
        loss.backward()
        torch.cuda.synchronize()
        st = dict(spec.options["_last_stats"])
        return st, [states.detach().cpu(), expect.detach().cpu(), amp.grad.cpu(), det.grad.cpu(), u.grad.cpu(), ts.grad.cpu(), ps.grad.cpu()]
    finally:
        _native.set_kernel_variant(0)


@pytest.mark.parametrize("n_qubits,tape,zero_last", [(13, "full", False), (16, "steps", True), (16, "full", False), (20, "full", True),
                                                     (20, "steps", False)])
def test_block_of_two_passes_match_one_factor_chain_and_direct_kernels(cuda_device, n_qubits, tape, zero_last):
    terms = random_terms(n_qubits, 13, 0.002, seed=900 + n_qubits, local=False, phase=False)
    tsave = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)
    gen = torch.Generator().manual_seed(n_qubits)
    psi = torch.randn(1, 2**n_qubits, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm()).to(cuda_device)
    obs = R.total_magnetization_diag(n_qubits)[None].to(cuda_device)
    out = {}
    for v in (1, 18, 17):
        st, out[v] = _run(v, terms, tsave, psi, cuda_device, obs, tape, zero_last)
        if v == 17:
            assert st["kernel_fwd"].startswith("k_chain2<"), st
        if v == 18:
            assert st["kernel_fwd"].startswith("k_chain<") or st["kernel_family"] != "chained-tiles", st
        torch.cuda.empty_cache()
    names = ("states", "expect", "amp", "det", "u", "tsave", "psi0")
    for v in (18, 17):
        for name, ref, got in zip(names, out[1], out[v]):
            tol = 1e-12 if name == "states" else (1e-10 if name == "expect" else 1e-9)
            assert rel_err(got.numpy(), ref.numpy()) < tol, (v, name)
    # the two chained forms against each other: the same adjoint kernels on forward tapes that differ by rounding only
    for name, a, b in zip(names, out[18], out[17]):
        assert np.abs((a - b).numpy()).max() <= 1e-8 * max(1.0, float(np.abs(a.numpy()).max())), name


def test_block_of_two_passes_are_the_automatic_choice_at_20_qubits_only(cuda_device):
    """Automatic on the measured shape (one 20-qubit trajectory); a smaller register keeps the one-factor chain unless forced."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    for n, variant, want in ((20, 0, "k_chain2<"), (20, 18, "k_chain<"), (16, 0, "")):
        terms = random_terms(n, 5, 0.002, seed=3, local=False, phase=False)
        _native.set_kernel_variant(variant)
        try:
            amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=False)
            psi = torch.zeros(1, 2**n, dtype=torch.complex128, device=cuda_device)
            psi[0, 0] = 1.0
            obs = R.total_magnetization_diag(n)[None].to(cuda_device)
            evolve(amp.real.contiguous(), det, u, torch.tensor([0.0, 0.008], dtype=torch.float64), psi, spec, obs)
            torch.cuda.synchronize()
            fwd = spec.options["_last_stats"]["kernel_fwd"]
        finally:
            _native.set_kernel_variant(0)
        if want:
            assert fwd.startswith(want), (n, variant, fwd)
        else:
            assert not fwd.startswith("k_chain2<"), (n, variant, fwd)
