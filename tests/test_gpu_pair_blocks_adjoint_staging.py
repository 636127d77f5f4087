"""Tape staging of the adjoint block kernel (k_chain2_bwd, pair_kernels.hpp): variant 21 requests both tape vectors at the top of the
kernel by LDS-DMA (x_a into the idle tile buffer, part of x_b into a staging area behind the parked partials), variant 20 stages them
through registers in two load phases; both force the blocks wherever legal (as 17, which takes the automatic staging).  Every
gradient kind against the direct kernels (variant 1) and against each other, on what the staging can get wrong: the batch offset in
the DMA source address, both tile layouts, a one-factor block (x_a == x_b, round B skipped), a chain of a single block, the
zero-amplitude last sample, stale LDS from an earlier launch, and the life of x_b's staging area up to the cotangent injection.
Helpers and tolerances are those of tests/test_gpu_pair_blocks_adjoint.py."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import rel_err, to_native
from tests.test_gpu_pair_blocks_adjoint import NAMES, TS, _run, _terms

pytestmark = pytest.mark.gpu

REGS, DMA = 20, 21
BLOCKS = (17, REGS, DMA)  # 17: the automatic staging


def _compare(out):
    """Gradients within 1e-9 relative of the direct kernels (states 1e-12, expectation values 1e-10: as the one-factor adjoint's
    test), block variants within 1e-8 max(1, |g|) of each other."""
    for v in out:
        if v == 1:
            continue
        for name, ref, got in zip(NAMES, out[1], out[v]):
            if ref.numel() == 0:  # no detuning group
                continue
            tol = 1e-12 if name == "states" else (1e-10 if name == "expect" else 1e-9)
            err = rel_err(got.numpy(), ref.numpy())
            print(f"variant {v} {name}: {err:.3e} relative to the direct kernels")
            assert err < tol, (v, name, err)
    blocks = [v for v in out if v != 1]
    for i, va in enumerate(blocks):
        for vb in blocks[i + 1:]:
            for name, a, b in zip(NAMES, out[va], out[vb]):
                if a.numel() == 0:
                    continue
                assert np.abs((a - b).numpy()).max() <= 1e-8 * max(1.0, float(np.abs(a.numpy()).max())), (va, vb, name)


def _check_kernels(stats):
    assert stats[REGS]["kernel_bwd"].startswith("k_chain2_bwd<") and stats[REGS]["kernel_bwd"].endswith(",false>"), stats[REGS]
    assert stats[DMA]["kernel_bwd"].startswith("k_chain2_bwd<") and stats[DMA]["kernel_bwd"].endswith(",true>"), stats[DMA]
    if 17 in stats:
        assert stats[17]["kernel_bwd"] in (stats[REGS]["kernel_bwd"], stats[DMA]["kernel_bwd"]), stats[17]


def _inputs(device, n, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    psi = torch.randn(batch, 2**n, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm(dim=1, keepdim=True)).to(device)
    return psi, R.total_magnetization_diag(n)[None].to(device)


def _case(device, n, det_groups, zero_last, batch, tsave, seed, amp_scale=6.0, variants=(1,) + BLOCKS):
    terms = _terms(n, 13, seed, det_groups, amp_scale)
    psi, obs = _inputs(device, n, batch, seed)
    out, stats = {}, {}
    for v in variants:
        stats[v], out[v] = _run(v, terms, tsave, psi, device, obs, "full", zero_last, batch)
        torch.cuda.empty_cache()
    _check_kernels(stats)
    _compare(out)
    return stats[DMA]


# 13 qubits: two tiles, layout B with lo = 11; 16 qubits, batch of 3: per-trajectory tables, the batch offset in the DMA source
# address; 20 qubits: 256-byte runs in layout B, once with a single long save interval; zero_last: the padded zero-amplitude sample
@pytest.mark.parametrize("n_qubits,det_groups,zero_last,batch,tsave", [
    (13, 1, False, 1, TS), (13, 0, True, 1, TS), (16, 1, False, 3, TS), (16, 1, True, 1, TS), (20, 1, True, 1, TS),
    (20, 0, False, 1, torch.tensor([0.0, 0.024], dtype=torch.float64))])
def test_both_stagings_match_the_direct_kernels_and_each_other(cuda_device, n_qubits, det_groups, zero_last, batch, tsave):
    _case(cuda_device, n_qubits, det_groups, zero_last, batch, tsave, 900 + n_qubits + 10 * det_groups + batch + len(tsave))


def test_one_factor_block_with_both_stagings(cuda_device):
    """An exponential of odd degree starts (forward order) with a one-factor block: x_a == x_b (both DMAs read the same vector),
    round B is skipped and e is never written over x_a's slots."""
    for scale in (6.0, 3.0, 9.0, 1.5, 12.0, 4.5, 7.5):
        st = _case(cuda_device, 13, 1, False, 1, TS, 811, amp_scale=scale, variants=(1, REGS, DMA))
        if st["degree"] % 2 == 1:
            return
    pytest.fail("no amplitude scale gave an odd polynomial degree")


def test_chain_of_a_single_block(cuda_device):
    """One short save interval and a loose tolerance: one exponential of degree 2, i.e. a chain of two launches.  The first has
    no block to finish (its tape pointers are the cotangent itself), the second starts none."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    n = 13
    terms = _terms(n, 13, 955, 1)
    psi, obs = _inputs(cuda_device, n, 1, 955)
    tsave = torch.tensor([0.0061, 0.0066], dtype=torch.float64)

    def run(variant, tol):
        _native.set_kernel_variant(variant)
        try:
            amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, tol=tol)
            spec.tape = "full"
            amp = amp.real.contiguous()
            ts, ps = tsave.clone().requires_grad_(True), psi.clone().requires_grad_(True)
            for t_ in (amp, det, u):
                t_.requires_grad_(True)
            states, expect = evolve(amp, det, u, ts, ps, spec, obs)
            gst = torch.linspace(-1.0, 1.0, states.numel(), dtype=torch.float64, device=cuda_device)
            (expect.sum() + 1e-3 * (states.real * gst.view(states.shape)).sum()).backward()
            torch.cuda.synchronize()
            grads = [amp.grad.cpu(), det.grad.cpu(), u.grad.cpu(), ts.grad.cpu(), ps.grad.cpu()]
            return dict(spec.options["_last_stats"]), [states.detach().cpu(), expect.detach().cpu()] + grads
        finally:
            _native.set_kernel_variant(0)

    for tol in (1e-4, 1e-3, 1e-5, 3e-4, 3e-5, 1e-2, 1e-6):
        st, ref = run(1, tol)
        if st["degree"] == 2 and st["total_factors"] == 2:
            break
    else:
        pytest.fail("no tolerance gave one exponential of degree 2")
    out, stats = {1: ref}, {}
    for v in (REGS, DMA):
        stats[v], out[v] = run(v, tol)
        assert stats[v]["degree"] == 2 and stats[v]["total_factors"] == 2, stats[v]
    _check_kernels(stats)
    _compare(out)


def test_no_stale_lds_between_two_problems(cuda_device):
    """Two different problems back to back in one process, 13 then 16 qubits, on the DMA kernel first: a read of staged data before
    it has landed would see what the previous launch left in the tile buffers."""
    cases = [(13, 1, 1, 971), (16, 1, 2, 972)]
    got = []
    for n, det_groups, batch, seed in cases:
        psi, obs = _inputs(cuda_device, n, batch, seed)
        got.append(_run(DMA, _terms(n, 13, seed, det_groups), TS, psi, cuda_device, obs, "full", False, batch))
    for (n, det_groups, batch, seed), (st, res) in zip(cases, got):
        psi, obs = _inputs(cuda_device, n, batch, seed)
        terms = _terms(n, 13, seed, det_groups)
        out, stats = {DMA: res}, {DMA: st}
        for v in (1, REGS):
            stats[v], out[v] = _run(v, terms, TS, psi, cuda_device, obs, "full", False, batch)
        _check_kernels(stats)
        _compare({v: out[v] for v in (1, REGS, DMA)})


def test_state_cotangent_at_an_inner_save_point_only(cuda_device):
    """The loss sits on the state at ONE inner save point: the only source of the cotangent is the injection, which reads x_b after
    both rounds — its staging area has to live until then."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    n = 16
    terms = _terms(n, 13, 981, 1)
    psi, obs = _inputs(cuda_device, n, 1, 981)
    out, stats = {}, {}
    for v in (1, REGS, DMA):
        _native.set_kernel_variant(v)
        try:
            amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
            spec.tape = "full"
            amp = amp.real.contiguous()
            ts, ps = TS.clone().requires_grad_(True), psi.clone().requires_grad_(True)
            for t_ in (amp, det, u):
                t_.requires_grad_(True)
            states, expect = evolve(amp, det, u, ts, ps, spec, obs)
            inner = states[2]  # (n_t, B, dim)
            gst = torch.linspace(-1.0, 1.0, inner.numel(), dtype=torch.float64, device=cuda_device).view(inner.shape)
            ((inner.real * gst).sum() + 0.5 * (inner.imag * gst.flip(-1)).sum()).backward()
            torch.cuda.synchronize()
            stats[v] = dict(spec.options["_last_stats"])
            out[v] = [states.detach().cpu(), expect.detach().cpu(), amp.grad.cpu(), det.grad.cpu(), u.grad.cpu(), ts.grad.cpu(), ps.grad.cpu()]
        finally:
            _native.set_kernel_variant(0)
        torch.cuda.empty_cache()
    assert float(out[1][2].abs().max()) > 0.0  # the injected cotangent reaches the amplitude gradient
    _check_kernels(stats)
    _compare(out)

    # and the expectation-value injection (2 g <O> x_b) alone, at the same save point
    out2 = {}
    for v in (1, REGS, DMA):
        _native.set_kernel_variant(v)
        try:
            amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
            spec.tape = "full"
            amp = amp.real.contiguous().requires_grad_(True)
            det.requires_grad_(True)
            states, expect = evolve(amp, det, u, TS, psi, spec, obs)
            expect[0, 2, 0].backward()
            torch.cuda.synchronize()
            out2[v] = [amp.grad.cpu(), det.grad.cpu()]
        finally:
            _native.set_kernel_variant(0)
    for v in (REGS, DMA):
        for ref, got in zip(out2[1], out2[v]):
            assert rel_err(got.numpy(), ref.numpy()) < 1e-9, v
