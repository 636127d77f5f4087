"""Request order and store policy of the block kernels (k_chain2, k_chain2_bwd; pair_kernels.hpp).  Variants
22..30 force the blocks wherever legal, as 20 does, and select one combination: 22 requests the inputs vector-major (v of every wave,
bare barrier, w, bare barrier, t or the tape vectors; forward: tables and coefficients ahead of them), 23 / 24 / 25 store v_mid and y
(adjoint: mu_out) / also w' / everything write-through, 26 / 27 / 28 do both, 29 is 22 with the LDS-DMA staging of 21, 30 does
neither; 20 takes the automatic combination (that of 28).  Neither
change touches the arithmetic, so every stored state of a run is bit-identical to variant 20's; expectation values and gradients
pass through atomics and are held to the bars of tests/test_gpu_pair_blocks_adjoint_staging.py: against the direct kernels (variant
1) states 1e-12, expectation values 1e-10, gradients 1e-9 relative, and gradients within 1e-8 max(1, |g|) of variant 20.  Sizes are
the smallest at which the layout (13 qubits: two tiles, one Y' bit; 14 and 16: more Y' bits, more workgroups), the batch offset in
the store descriptor (batch 3), the detuning coefficient fetched at the top (0 / 1 groups) and the padded zero-amplitude sample can
go wrong.  Helpers are those of tests/test_gpu_pair_blocks_adjoint.py."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import rel_err, to_native
from tests.test_gpu_pair_blocks_adjoint import NAMES, TS, _run, _terms

pytestmark = pytest.mark.gpu

DIRECT, BASE = 1, 20
# variant -> (vector-major requests, write-through level, LDS-DMA staging)
PHASES = {22: (True, 0, False), 23: (False, 1, False), 24: (False, 2, False), 25: (False, 3, False),
          26: (True, 1, False), 27: (True, 2, False), 28: (True, 3, False), 29: (True, 0, True), 30: (False, 0, False)}
NEW = tuple(PHASES)
AUTOMATIC = PHASES[28]  # what variant 20 (and 17, and the automatic choice) takes


def _b(v):
    return "true" if v else "false"


def _check_kernels(stats):
    for v, st in stats.items():
        if v == DIRECT:
            continue
        order, level, dma = PHASES.get(v, AUTOMATIC)
        assert st["kernel_fwd"] == f"k_chain2<12,10,{_b(order)},{level}>", (v, st)
        assert st["kernel_bwd"] == f"k_chain2_bwd<12,10,{_b(order)},{level},{_b(dma)}>", (v, st)


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


def _case(device, n, det_groups, zero_last, batch, tape, seed, amp_scale=6.0, tsave=TS):
    terms = _terms(n, 13, seed, det_groups, amp_scale)
    psi, obs = _inputs(device, n, batch, seed)
    out, stats = {}, {}
    for v in (DIRECT, BASE) + NEW:
        stats[v], out[v] = _run(v, terms, tsave, psi, device, obs, tape, zero_last, batch)
    _check_kernels(stats)
    _compare(out)
    return stats[BASE]


# tapes: "full", and "steps" (one state per save point: the factor inputs of an interval are recomputed by forward block launches)
@pytest.mark.parametrize("n_qubits,det_groups,zero_last,batch,tape", [
    (13, 1, False, 1, "full"), (13, 0, True, 3, "full"), (14, 1, True, 3, "full"), (14, 0, False, 1, "steps"),
    (16, 1, False, 3, "full"), (16, 1, True, 1, "steps"), (16, 0, False, 1, "full")])
def test_every_combination_matches_the_direct_kernels_and_variant_20(cuda_device, n_qubits, det_groups, zero_last, batch, tape):
    _case(cuda_device, n_qubits, det_groups, zero_last, batch, tape, 1200 + n_qubits + 10 * det_groups + batch + len(tape))


def test_one_factor_block(cuda_device):
    """An exponential of odd degree ends (forward order) in a one-factor block: the second finishing round is skipped, so t is never
    used on that launch although it was requested behind the second barrier."""
    for scale in (6.0, 3.0, 9.0, 1.5, 12.0, 4.5, 7.5):
        st = _case(cuda_device, 13, 1, False, 1, "full", 811, amp_scale=scale)
        if st["degree"] % 2 == 1:
            return
    pytest.fail("no amplitude scale gave an odd polynomial degree")


def _custom(device, n, seed, tsave, loss_fn, tol=None, variants=(DIRECT, BASE) + NEW):
    """Runs with a loss of the caller's: loss_fn(states, expect) -> scalar."""
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
            spec.tape = "full"
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


def test_chain_of_a_single_block(cuda_device):
    """One short save interval and a loose tolerance: one exponential of degree 2, i.e. a chain of two launches.  The first has no
    block to finish (w and t are the start vector itself; with vector-major requests y is taken from the last request), the second
    starts none and returns behind its y stores."""
    tsave = torch.tensor([0.0061, 0.0066], dtype=torch.float64)

    def loss(states, expect):
        gst = torch.linspace(-1.0, 1.0, states.numel(), dtype=torch.float64, device=states.device)
        return expect.sum() + 1e-3 * (states.real * gst.view(states.shape)).sum()

    for tol in (1e-4, 1e-3, 1e-5, 3e-4, 3e-5, 1e-2, 1e-6):
        st, _ = _custom(cuda_device, 13, 955, tsave, loss, tol, variants=(DIRECT,))
        if st[DIRECT]["degree"] == 2 and st[DIRECT]["total_factors"] == 2:
            break
    else:
        pytest.fail("no tolerance gave one exponential of degree 2")
    stats, out = _custom(cuda_device, 13, 955, tsave, loss, tol)
    for v in (BASE,) + NEW:
        assert stats[v]["degree"] == 2 and stats[v]["total_factors"] == 2, stats[v]
    _check_kernels(stats)
    _compare(out)


def test_state_cotangent_at_an_inner_save_point_only(cuda_device):
    """The loss sits on the state at ONE inner save point: the only source of the cotangent is the injection, which is added to
    mu_out just before it is stored (write-through from level 1 on)."""

    def loss(states, expect):
        inner = states[2]  # (n_t, B, dim)
        gst = torch.linspace(-1.0, 1.0, inner.numel(), dtype=torch.float64, device=states.device).view(inner.shape)
        return (inner.real * gst).sum() + 0.5 * (inner.imag * gst.flip(-1)).sum()

    stats, out = _custom(cuda_device, 14, 981, TS, loss)
    assert float(out[DIRECT][2].abs().max()) > 0.0  # the injected cotangent reaches the amplitude gradient
    _check_kernels(stats)
    _compare(out)


def test_no_stale_lds_between_two_problems(cuda_device):
    """Two different problems back to back on each new variant, 13 then 16 qubits: a barrier in the wrong place or a read of a tile
    buffer before it is published would see what the previous launch left in LDS."""
    cases = [(13, 1, 1, 971), (16, 1, 2, 972)]
    refs = []
    for n, det_groups, batch, seed in cases:
        psi, obs = _inputs(cuda_device, n, batch, seed)
        terms = _terms(n, 13, seed, det_groups)
        refs.append({v: _run(v, terms, TS, psi, cuda_device, obs, "full", False, batch) for v in (DIRECT, BASE)})
    for v in NEW:
        got = []
        for n, det_groups, batch, seed in cases:  # back to back on variant v
            psi, obs = _inputs(cuda_device, n, batch, seed)
            got.append(_run(v, _terms(n, 13, seed, det_groups), TS, psi, cuda_device, obs, "full", False, batch))
        for ref, (st, res) in zip(refs, got):
            _check_kernels({v: st})
            _compare({DIRECT: ref[DIRECT][1], BASE: ref[BASE][1], v: res})
