"""Paced input requests of the block kernels (template parameter PACE of k_chain2 and k_chain2_bwd; pair_kernels.hpp, DESIGN.md
section 3).  Variants 31..34 force the blocks wherever legal, as 20 does: 31 paces the forward kernel (w requested once half of the
wave's v is back, round A on v alone, t requested behind round A once half of w is back), 32 the adjoint kernel (w and x_a once half
of mu is back, round A on mu alone, x_a consumed from registers), 33 both, 34 the forward kernel with t requested before round A.
Pacing changes when a request is issued and where it is awaited, and no arithmetic statement, so every stored state of a run is
bit-identical to variant 20's; expectation values and gradients pass through atomics and are held to the bars of
tests/test_gpu_pair_blocks_phases.py: against the direct kernels (variant 1) states 1e-12, expectation values 1e-10, gradients 1e-9
relative, and gradients within 1e-8 max(1, |g|) of variant 20.  Sizes are the smallest at which the request structure can go
wrong: 13 qubits (two tiles, one Y' bit), 14 and 16 (more Y' bits and workgroups), batch 3 (the batch offset of the paced t request
and of the always-issued v_mid stores), 0 / 1 detuning groups, a zero-amplitude padded last sample, an exponential of odd degree
(a one-factor block: round B is skipped and t's request is retired unused; no v_mid destination, so the four v_mid stores are dropped
by the range check), a one-interval run (the first launch, has_p = 0, next to the last, has_q = 0), and the full tape, a partial
tape and the recomputed one.  Helpers are those of tests/test_gpu_pair_blocks_adjoint.py."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import rel_err, to_native
from tests.test_gpu_pair_blocks_adjoint import NAMES, TS, _run, _terms

pytestmark = pytest.mark.gpu

DIRECT, BASE = 1, 20
# variant -> (PACE of k_chain2, PACE of k_chain2_bwd)
PACED = {31: (1, 0), 32: (0, 1), 33: (1, 1), 34: (2, 0)}
NEW = tuple(PACED)
FWD0, BWD0 = "k_chain2<12,10,true,3>", "k_chain2_bwd<12,10,true,3,false>"  # variant 20: unchanged by this family


def _check_kernels(stats, fwd_blocks=True):
    """fwd_blocks: the forward pass runs in blocks (not with a partial tape, whose forward pass is k_chain for every variant)."""
    for v, st in stats.items():
        if v == DIRECT:
            continue
        pf, pb = PACED.get(v, (0, 0))
        if fwd_blocks:
            assert st["kernel_fwd"] == (f"k_chain2<12,10,true,3,{pf}>" if pf else FWD0), (v, st)
        else:
            assert st["kernel_fwd"] == stats[BASE]["kernel_fwd"] and not st["kernel_fwd"].startswith("k_chain2<"), (v, st)
        assert st["kernel_bwd"] == (f"k_chain2_bwd<12,10,true,3,false,{pb}>" if pb else BWD0), (v, st)


def _compare(out):
    """out: {variant: [states, expect, gradients...]} with DIRECT, BASE and new variants."""
    for v in out:
        if v == DIRECT:
            continue
        for name, ref, got in zip(NAMES, out[DIRECT], out[v]):
            if ref.numel() == 0:  # no detuning group
                continue
            tol = 1e-12 if name == "states" else (1e-10 if name == "expect" else 1e-9)
            err = rel_err(got.numpy(), ref.numpy())
            print(f"variant {v} {name}: {err:.3e} relative to the direct kernels")
            assert err < tol, (v, name, err)
    for v in out:
        if v in (DIRECT, BASE):
            continue
        assert torch.equal(out[BASE][0], out[v][0]), (v, "stored states differ from variant 20's")
        for name, a, b in zip(NAMES[2:], out[BASE][2:], out[v][2:]):
            if a.numel() == 0:
                continue
            diff = float(np.abs((a - b).numpy()).max())
            print(f"variant {v} {name}: {diff:.3e} from variant 20")
            assert diff <= 1e-8 * max(1.0, float(np.abs(a.numpy()).max())), (v, name, diff)


def _inputs(device, n, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    psi = torch.randn(batch, 2**n, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm(dim=1, keepdim=True)).to(device)
    return psi, R.total_magnetization_diag(n)[None].to(device)


def _case(device, n, det_groups, zero_last, batch, tape, seed, amp_scale=6.0):
    terms = _terms(n, 13, seed, det_groups, amp_scale)
    psi, obs = _inputs(device, n, batch, seed)
    out, stats = {}, {}
    for v in (DIRECT, BASE) + NEW:
        stats[v], out[v] = _run(v, terms, TS, psi, device, obs, tape, zero_last, batch)
    _check_kernels(stats)
    _compare(out)
    return stats[BASE]


# tapes: "full", and "steps" (one state per save point: the factor inputs of an interval are recomputed by forward block launches)
@pytest.mark.parametrize("n_qubits,det_groups,zero_last,batch,tape", [
    (13, 1, False, 1, "full"), (13, 0, True, 3, "full"), (14, 1, True, 3, "full"), (14, 0, False, 1, "steps"),
    (16, 1, False, 3, "full"), (16, 1, True, 1, "steps"), (16, 0, False, 1, "full")])
def test_paced_requests_match_the_direct_kernels_and_variant_20(cuda_device, n_qubits, det_groups, zero_last, batch, tape):
    _case(cuda_device, n_qubits, det_groups, zero_last, batch, tape, 1300 + n_qubits + 10 * det_groups + batch + len(tape))


def test_one_factor_block(cuda_device):
    """An exponential of odd degree ends (forward order) in a one-factor block: the second finishing round is skipped, the paced t
    request is retired without a use, and the v_mid stores have no destination."""
    for scale in (6.0, 3.0, 9.0, 1.5, 12.0, 4.5, 7.5):
        st = _case(cuda_device, 13, 1, False, 1, "full", 811, amp_scale=scale)
        if st["degree"] % 2 == 1:
            return
    pytest.fail("no amplitude scale gave an odd polynomial degree")


def _custom(device, n, seed, tsave, loss_fn, tol=None, variants=(DIRECT, BASE) + NEW, tape="full", tape_steps=None):
    """Runs with a loss, a tolerance and a tape of the caller's: loss_fn(states, expect) -> scalar."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    terms = _terms(n, 13, seed, 1)
    psi, obs = _inputs(device, n, 1, seed)
    out, stats = {}, {}
    for v in variants:
        _native.set_kernel_variant(v)
        try:
            kw = {} if tol is None else {"tol": tol}
            amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE, **kw)
            spec.tape = tape
            if tape_steps is not None:
                spec.tape_steps = tape_steps
            amp = amp.real.contiguous()
            ts, ps = tsave.clone().requires_grad_(True), psi.clone().requires_grad_(True)
            for t_ in (amp, det, u):
                t_.requires_grad_(True)
            states, expect = evolve(amp, det, u, ts, ps, spec, obs)
            loss_fn(states, expect).backward()
            torch.cuda.synchronize()
            stats[v] = dict(spec.options["_last_stats"])
            out[v] = [states.detach().cpu(), expect.detach().cpu(), amp.grad.cpu(), det.grad.cpu(), u.grad.cpu(), ts.grad.cpu(), ps.grad.cpu()]
        finally:
            _native.set_kernel_variant(0)
    return stats, out


def _loss(states, expect):
    gst = torch.linspace(-1.0, 1.0, states.numel(), dtype=torch.float64, device=states.device)
    return expect.sum() + 1e-3 * (states.real * gst.view(states.shape)).sum()


def test_chain_of_a_single_block(cuda_device):
    """One short save interval and a loose tolerance: one exponential of degree 2, i.e. a chain of two launches.  The first has no
    block to finish (w is the start vector itself, t is never requested, y is taken from w), the second starts none and returns
    behind its y stores."""
    tsave = torch.tensor([0.0061, 0.0066], dtype=torch.float64)
    for tol in (1e-4, 1e-3, 1e-5, 3e-4, 3e-5, 1e-2, 1e-6):
        st, _ = _custom(cuda_device, 13, 955, tsave, _loss, tol, variants=(DIRECT,))
        if st[DIRECT]["degree"] == 2 and st[DIRECT]["total_factors"] == 2:
            break
    else:
        pytest.fail("no tolerance gave one exponential of degree 2")
    stats, out = _custom(cuda_device, 13, 955, tsave, _loss, tol)
    for v in (BASE,) + NEW:
        assert stats[v]["degree"] == 2 and stats[v]["total_factors"] == 2, stats[v]
    _check_kernels(stats)
    _compare(out)


def test_partial_tape(cuda_device):
    """Two trailing save intervals on the tape, the others recomputed: the adjoint blocks read a tape that the one-factor forward
    pass (k_chain, for every variant) and the recomputing forward block launches wrote."""
    stats, out = _custom(cuda_device, 14, 967, TS, _loss, tape="partial", tape_steps=2)
    assert stats[BASE]["tape"] == "partial", stats[BASE]
    _check_kernels(stats, fwd_blocks=stats[BASE]["kernel_fwd"].startswith("k_chain2<"))
    _compare(out)
