"""P_X v on the tape between the two factors of a block (variant 35; pair_launch.hpp: pair_wtape, pair_kernels.hpp: the XW
instantiation of k_chain2_bwd).  The forward block launches write their w = P_X v into the tape slot that held
v_mid and store no v_mid; the adjoint block kernel rebuilds v_mid from the two tape vectors with one more partner-sum round.

Forward arithmetic is unchanged, so the stored states of a run are compared bit for bit with variant 20's.  <O> is reduced from
those states by the same code, but through atomic adds of up to 1024 workgroup partials per value (k_expect_diag at the first save
point: 32 at 13 qubits), whose order differs from run to run: variant 20 does not reproduce its own <O> bit for bit, so <O> is held
to the rounding of such a reordered sum, 1024 * 2^-52 * max(1, max |<O>|), not to the last bit.  Gradients are held to the bars of tests/test_gpu_pair_blocks_adjoint.py against the direct kernels (variant 1: states
1e-12, expectation values 1e-10, gradients 1e-9 relative; 1e-8 max(1, |g|) against variant 20), and to ten times the difference
that variant 20 shows against itself over two runs.  At these sizes that difference is often exactly zero (one gradient replica per
tile: nothing lands in another order), while variant 35 adds the same terms in another order whenever the run-wide block count
makes its adjoint launches run in the other layout than variant 20's, or an odd degree makes its blocks differ.  What another
valid order of the same sums costs is measured in the same run, by variant 20 against the direct kernels, so the allowance is the
larger of ten times variant 20's own spread and ten times its distance from the direct kernels.  (Where the launches of the two
variants run in the same layouts the rebuilt mid-block state agrees with the stored one to the last bit and the gradients of
13-qubit runs come out bit-identical; the figures are printed.)

Sizes are the smallest at which each trap exists: 13 qubits (two tiles, one Y' bit) and 16; three and four save intervals, so that
the run-wide index of the last block takes both parities (the adjoint's layouts are offset by it); 0 / 1 detuning group; a
zero-amplitude padded last sample; batch 1 and 3; every gradient kind with cotangents at every save point (tests' _run); an
exponential of odd degree (the forward pairs from the front, so the adjoint has to take the forward's blocks); one 20-qubit run;
one run whose adjoint splits its chain at 2^16 factors (the second chain's parity comes from the run-wide block count)."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import random_terms, rel_err, to_native
from tests.test_gpu_pair_blocks_adjoint import NAMES, TS, _run, _terms

pytestmark = pytest.mark.gpu

DIRECT, BASE, NEW = 1, 20, 35
XW_KERNEL = "k_chain2_bwd<12,10,true,3,false,0,true>"
TS3 = TS[:4].clone()  # three save intervals; TS has four


def _inputs(device, n, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    psi = torch.randn(batch, 2**n, generator=gen, dtype=torch.complex128)
    psi = (psi / psi.norm(dim=1, keepdim=True)).to(device)
    return psi, R.total_magnetization_diag(n)[None].to(device)


TIGHT = {"states": 1e-12, "expect": 1e-10, "grad": 1e-9}  # the bars of tests/test_gpu_pair_blocks_adjoint.py (runs of tens of factors)
LONG = {"states": 1e-9, "expect": 1e-9, "grad": 1e-8}      # the project's bars on values and gradients (a run of 10^5 factors)


def _compare(label, out, new_keys, tols=TIGHT):
    """out: {"direct", "base", "base2" (variant 20 twice), *new_keys: [states, expect, gradients...]}"""
    for key in ("base",) + tuple(new_keys):
        for name, ref, got in zip(NAMES, out["direct"], out[key]):
            if ref.numel() == 0:  # no detuning group
                continue
            tol = tols.get(name, tols["grad"])
            err = rel_err(got.numpy(), ref.numpy())
            print(f"WTAPE {label} {key} {name}: {err:.3e} relative to the direct kernels")
            assert err < tol, (label, key, name, err)
    for key in new_keys:
        assert torch.equal(out["base"][0], out[key][0]), (label, key, "stored states differ from variant 20's")
        omax = float(out["direct"][1].abs().max())
        ediff = float((out["base"][1] - out[key][1]).abs().max())
        enoise = float((out["base"][1] - out["base2"][1]).abs().max())
        print(f"WTAPE_PARITY {label} {key} expect: {ediff:.3e} from variant 20; variant 20 from itself {enoise:.3e}; max |<O>| {omax:.3e}")
        assert ediff <= 1024 * 2.0**-52 * max(1.0, omax), (label, key, "<O> differs from variant 20's", ediff)
        for name, a, a2, b, d in zip(NAMES[2:], out["base"][2:], out["base2"][2:], out[key][2:], out["direct"][2:]):
            if a.numel() == 0:
                continue
            noise = float(np.abs((a - a2).numpy()).max())
            diff = float(np.abs((a - b).numpy()).max())
            order = float(np.abs((a - d).numpy()).max())
            print(f"WTAPE_PARITY {label} {key} {name}: {diff:.3e} from variant 20; variant 20 from itself {noise:.3e}, from the direct kernels "
                  f"{order:.3e}; max |g| {float(a.abs().max()):.3e}")
            assert diff <= 1e-8 * max(1.0, float(np.abs(a.numpy()).max())), (label, key, name, diff)
            assert diff <= 10.0 * max(noise, order), (label, key, name, diff, noise, order)


def _case(device, n, det_groups, zero_last, batch, tsave, seed, amp_scale=6.0, new=(NEW,), terms=None, tols=TIGHT):
    terms = _terms(n, 13, seed, det_groups, amp_scale) if terms is None else terms
    psi, obs = _inputs(device, n, batch, seed)
    out, stats = {}, {}
    for key, v in (("direct", DIRECT), ("base", BASE), ("base2", BASE)) + tuple((f"v{v}", v) for v in new):
        stats[key], out[key] = _run(v, terms, tsave, psi, device, obs, "full", zero_last, batch)
        torch.cuda.empty_cache()
    label = f"N{n} g{det_groups} z{int(zero_last)} B{batch} T{len(tsave) - 1}"
    st = stats[f"v{NEW}"]
    assert st["tape"] == "full" and st["kernel_fwd"] == stats["base"]["kernel_fwd"] and st["kernel_bwd"] == XW_KERNEL, st
    assert stats["base"]["kernel_bwd"] == "k_chain2_bwd<12,10,true,3,false>", stats["base"]
    print(f"WTAPE {label}: degree {st['degree']}, factors {st['total_factors']}")
    _compare(label, out, tuple(f"v{v}" for v in new), tols)
    return stats


def _last_block(st, n_intervals):
    """Run-wide index of the last forward block of a run of one exponential per save interval."""
    assert st["n_stages"] == n_intervals and st["total_factors"] == n_intervals * st["degree"], st
    return n_intervals * ((st["degree"] + 1) // 2) - 1


# (the two 13-qubit cases with one detuning group and batch 1 differ in the number of intervals only: the parity pair)
@pytest.mark.parametrize("n_qubits,det_groups,zero_last,batch,tsave", [
    (13, 1, False, 1, TS3), (13, 1, False, 1, TS), (13, 0, True, 3, TS), (13, 1, True, 3, TS3),
    (16, 1, True, 3, TS3), (16, 0, False, 1, TS), (16, 1, False, 1, TS3), (16, 0, True, 1, TS3), (16, 1, False, 3, TS)])
def test_w_on_the_tape_matches_variant_20_and_the_direct_kernels(cuda_device, n_qubits, det_groups, zero_last, batch, tsave):
    _case(cuda_device, n_qubits, det_groups, zero_last, batch, tsave, 3500 + n_qubits + 10 * det_groups + batch)


def test_both_parities_of_the_last_block(cuda_device):
    """Three and four intervals of the same pulse at degree 10 are 15 and 20 blocks: the adjoint's first launch runs in layout 0 for
    the one and in layout 1 for the other."""
    def uniform(n_intervals, h):  # equal intervals: the degree follows from h alone
        return torch.arange(n_intervals + 1, dtype=torch.float64) * h

    for h in (0.003, 0.0025, 0.0035, 0.002, 0.004, 0.0015, 0.0045):  # shorter intervals than above: a lower degree than their 13 .. 16
        st = _case(cuda_device, 13, 1, False, 1, uniform(3, h), 3524)[f"v{NEW}"]
        if st["degree"] == 10:
            break
    else:
        pytest.fail("no interval length gave degree 10")
    seen = {_last_block(st, 3) & 1}
    st = _case(cuda_device, 13, 1, False, 1, uniform(4, h), 3524)[f"v{NEW}"]
    assert st["degree"] == 10, st
    seen.add(_last_block(st, 4) & 1)
    assert seen == {0, 1}, seen


def test_odd_degree_takes_the_forward_blocks(cuda_device):
    """An exponential of odd degree: the forward pass ends it with a one-factor block, the adjoint (which pairs from the end on its
    own) has to start it with that block; the one-factor block skips the x-round."""
    for scale in (3.0, 9.0, 1.5, 12.0, 4.5, 7.5, 6.0):
        st = _case(cuda_device, 13, 1, False, 1, TS3, 811, amp_scale=scale)[f"v{NEW}"]
        if st["degree"] % 2 == 1:
            return
    pytest.fail("no amplitude scale gave an odd polynomial degree")


def test_twenty_qubits_automatic(cuda_device):
    """The flagship shape, four intervals: variant 35 and the automatic choice against variant 20 and the direct kernels."""
    stats = _case(cuda_device, 20, 1, True, 1, TS, 3520, new=(NEW, 0))
    assert stats["v0"]["kernel_bwd"] == XW_KERNEL and stats["v0"]["kernel_fwd"] == stats["base"]["kernel_fwd"], stats["v0"]


def test_adjoint_chain_split(cuda_device):
    """More than 2^16 factors: the adjoint sweep runs two chains, and the layouts of the second follow from the number of blocks in
    front of it, not from its own length.  The tape takes about 9 GB."""
    free, _ = torch.cuda.mem_get_info(cuda_device)
    if free < 24 * 2**30:
        pytest.skip("needs about 24 GB of free device memory")
    n, k = 13, 6600
    dt = TS[-1].item() / 4 * k / 12  # the pulse of the small cases, stretched so that every interval is as long as theirs
    terms = random_terms(n, 13, dt, seed=3526, local=False, phase=False, amp_scale=6.0)
    tsave = torch.linspace(0.0, 12 * dt, k + 1, dtype=torch.float64)
    st = _case(cuda_device, n, 1, False, 1, tsave, 3526, terms=terms, tols=LONG)[f"v{NEW}"]
    assert st["total_factors"] > 2**16, st


def _custom(device, variant, n, seed, real=True, tape="full", tape_steps=None, backward_variant=None):
    """One run with every gradient; backward_variant: the adjoint call is made with another kernel_variant than the forward call."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import SolverType, evolve

    terms = _terms(n, 13, seed, 1)
    psi, obs = _inputs(device, n, 1, seed)
    _native.set_kernel_variant(variant)
    try:
        amp, det, u, spec = to_native(terms, device, SolverType.KRYLOV_SE)
        spec.tape = tape
        if tape_steps is not None:
            spec.tape_steps = tape_steps
        if real:
            amp = amp.real.contiguous()
        ts, ps = TS.clone().requires_grad_(True), psi.clone().requires_grad_(True)
        for t_ in (amp, det, u):
            t_.requires_grad_(True)
        states, expect = evolve(amp, det, u, ts, ps, spec, obs)
        if backward_variant is not None:
            expect.grad_fn.kernel_variant = backward_variant
        gst = torch.linspace(-1.0, 1.0, states.numel(), dtype=torch.float64, device=device)
        (expect.sum() + 1e-3 * (states.real * gst.view(states.shape)).sum()).backward()
        torch.cuda.synchronize()
        grads = [amp.grad.cpu(), det.grad.cpu(), u.grad.cpu(), ts.grad.cpu(), ps.grad.cpu()]
        return dict(spec.options["_last_stats"]), [states.detach().cpu(), expect.detach().cpu()] + grads
    finally:
        _native.set_kernel_variant(0)


@pytest.mark.parametrize("variant,real,tape", [(19, True, "full"), (NEW, False, "full"), (NEW, True, "partial"), (NEW, True, "steps")])
def test_other_readers_keep_the_mid_block_state(cuda_device, variant, real, tape):
    """Where the block adjoint does not read the full tape (variant 19, complex tables, the partial tape, recomputed factor inputs)
    the forward pass keeps v_mid and the adjoint reads it as before: results match the direct kernels."""
    kw = dict(real=real, tape=tape, tape_steps=2 if tape == "partial" else None)
    st, got = _custom(cuda_device, variant, 14, 3530, **kw)
    _, ref = _custom(cuda_device, DIRECT, 14, 3530, **kw)
    # ("steps" with stored states: the adjoint reads the caller's states and recomputes the factor inputs; reported as no tape)
    assert st["kernel_bwd"] != XW_KERNEL and (st["tape"] == tape or (tape == "steps" and st["tape"] in ("steps", "none"))), st
    for name, a, b in zip(NAMES, ref, got):
        tol = 1e-12 if name == "states" else (1e-10 if name == "expect" else 1e-9)
        err = rel_err(b.numpy(), a.numpy())
        print(f"WTAPE guard variant {variant} real {real} tape {tape} {name}: {err:.3e} ({st['kernel_fwd']} / {st['kernel_bwd']})")
        assert err < tol, (name, err)


@pytest.mark.parametrize("fwd,bwd", [(NEW, BASE), (BASE, NEW), (NEW, 19)])
def test_backward_on_a_tape_of_the_other_format_is_an_error(cuda_device, fwd, bwd):
    with pytest.raises(ValueError, match="full tape in this workspace holds"):
        _custom(cuda_device, fwd, 13, 3531, backward_variant=bwd)
