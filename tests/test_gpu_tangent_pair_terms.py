"""Tangent sweep on kets with dense pair terms (k_factor_tangent<D, true>, pair_apply_all): the XY exchange and, on the doubled register,
the dissipator are such terms — constants in every tangent direction.

7. Random NON-Hermitian 4x4 blocks on random qubit pairs, entry by entry against tests.tangent_pair_reference (the dense forward-mode
   reference of tests/test_gpu_tangent_matrix.py with sum_p embed(T_p) added to H): 4 qubits (below one workgroup), 8 (exactly one)
   and 10 (four; the pair's partner lines lie in other workgroups), 1 / 3 / RYDIFF_MAX_PAIR_TERMS = 28 blocks (every block has all
   four relative flips; the one-block cases also zero all but the diagonal and the double flip — the masks of relaxation), D = 2 and
   8 directions (three and two flips in flight at a time), both solvers, B = 2.  Bars of tests/test_gpu_tangent_matrix.py:
   ORACLE_RTOL = 1e-8 relative to the largest entry of the direction, VALUE_ATOL = 1e-9 times the row's weight.
8. The XY emulator (tests/test_gpu_master_equation_sizes._xy_problem, 3 atoms): run_sensitivities(route="tangent") runs the sweep and agrees
   with route="adjoint-loop" at 1e-9 relative.  (Same solver on both sides: a duality check; 7 carries the correctness.)
9. Geometry with pair terms on kets: the Gram matrices of two calls are bit-identical, and gram[0, 0] is the squared norm of the
   (non-unitary) state evolve returns.

Measured on an MI355X: 7. tangents 5.3e-12 of the direction's largest entry, values 1.1e-13 of the row weight; 8. 6.5e-14 absolute;
9. 1.3e-15, and <psi|dpsi_d> 1.1e-14 against the dense reference.  Reference CPU time per 10-qubit problem (shared by its D = 2 and
D = 8 cases): 7 to 10 s (KRYLOV_SE), 4 to 5 s (DP5_SE) on 8 cores; below a second at 4 and 8 qubits."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd.lindblad import MAX_PAIR_TERMS
from pulser_diff_amd.observables import StateOverlap, pack_overlaps
from pulser_diff_amd.solver import SolverType, evolve, evolve_geometry, evolve_tangent
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import random_terms, tangent_rows_reference, to_native
from tests.tangent_pair_reference import tangent_pair_reference
from tests.test_gpu_tangent import ORACLE_RTOL, PUBLIC_RTOL, _randn, observable_set

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9
N_SAMPLES, DT = 41, 0.004
TSAVE = {"KRYLOV_SE": (0.0, 0.0313, 0.0622), "DP5_SE": (0.0, 0.0019, 0.0043)}  # tests/test_gpu_tangent_matrix.py: TSAVE_9, TSAVE_DP5_SHORT
BATCH = 2


def _blocks(n, count, gen, masks_of_relaxation=False):
    """`count` seeded non-Hermitian blocks of size ~1 rad/us on random qubit pairs (a != b, either order)."""
    out = []
    for _ in range(count):
        a, b = (int(v) for v in torch.randperm(n, generator=gen)[:2])
        blk = 0.7 * _randn(gen, 4, 4, cplx=True)
        if masks_of_relaxation:  # keep T[own][own] and T[own][own ^ 3] only
            keep = torch.zeros(4, 4)
            for own in range(4):
                keep[own, own] = keep[own, own ^ 3] = 1.0
            blk = blk * keep
        out.append((a, b, blk.numpy()))
    return tuple(out)


@lru_cache(maxsize=None)
def _problem(n, count, solver_name, sparse):
    """Problem and dense reference for 8 directions (sliced by the 2-direction cases): computed once, shared, never modified."""
    terms = random_terms(n, N_SAMPLES, DT, seed=2300 + n, local=True, phase=True)
    amp, det, u, _ = to_native(terms, "cpu", SolverType.KRYLOV_SE)
    gen = torch.Generator().manual_seed(91000 + 131 * n + count + (7 if sparse else 0))
    pairs = _blocks(n, count, gen, sparse)
    dim, n_dir = 2 ** n, 8
    psi0 = _randn(gen, BATCH, dim, cplx=True)
    psi0 = psi0 / psi0.norm(dim=1, keepdim=True)
    scale = 8.0 if solver_name == "KRYLOV_SE" else 1.0  # (tests/test_gpu_tangent_matrix.py: KRYLOV_SE reads the tables once per interval)
    d_amp = scale * float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)
    d_det = scale * float(det.abs().max()) * _randn(gen, n_dir, *det.shape)
    d_u = float(u.abs().max()) * _randn(gen, n_dir, *u.shape)
    d_psi = _randn(gen, n_dir, BATCH, dim, cplx=True) / np.sqrt(dim)
    d_amp[7], d_det[7], d_u[7], d_psi[7] = 0.0, 0.0, 0.0, 0.0  # one direction that is zero
    target = psi0.T + 0.5 * _randn(gen, dim, BATCH, cplx=True) / np.sqrt(dim)
    target = target / target.norm(dim=0, keepdim=True)
    tsave = torch.tensor(TSAVE[solver_name], dtype=torch.float64)
    ref = tangent_pair_reference(terms, pairs, d_amp[:, 0], d_det[:, 0], d_u, psi0.T.contiguous(), d_psi.permute(0, 2, 1).contiguous(),
                                 tsave, SolverType[solver_name])
    return dict(terms=terms, amp=amp, det=det, u=u, pairs=pairs, psi0=psi0, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi=d_psi,
                target=target, tsave=tsave, ref=ref)


PAIR_CASES = [(n, count, sparse) for n in (4, 8, 10) for count, sparse in ((1, False), (1, True), (3, False), (MAX_PAIR_TERMS, False))]


@pytest.mark.parametrize("n_dir", [2, 8])
@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
@pytest.mark.parametrize("n,count,sparse", PAIR_CASES, ids=[f"N{n}-P{c}{'-relax' if s else ''}" for n, c, s in PAIR_CASES])
def test_kets_with_dense_pair_blocks_match_the_dense_reference(cuda_device, n, count, sparse, solver_name, n_dir):
    dev = cuda_device
    prob = _problem(n, count, solver_name, sparse)
    dim = 2 ** n
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[solver_name], store_states=False)
    spec.pair_terms = prob["pairs"]
    pauli = observable_set(n)
    spec.pauli = pauli
    spec.overlaps = pack_overlaps([StateOverlap(prob["target"])], dim, BATCH, dev)
    diag = total_magnetization_diag(n)[None]
    sl = slice(8 - n_dir, 8)  # (ends with the zero direction)
    expect, dexpect = evolve_tangent(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), prob["tsave"], prob["psi0"].to(dev), spec,
                                     diag.to(dev), d_amp=prob["d_amp"][sl].to(dev), d_det=prob["d_det"][sl].to(dev),
                                     d_u=prob["d_u"][sl].to(dev), d_psi0=prob["d_psi"][sl].to(dev), flags=_native.TANGENT_PAIR_TERMS)
    states, tangents = prob["ref"]
    want_val, want_der = tangent_rows_reference(states, tangents[:, sl], diag, pauli, [prob["target"]])
    got_val, got_der = expect.cpu(), dexpect.cpu()
    assert tuple(got_der.shape) == tuple(want_der.shape) and tuple(got_val.shape) == tuple(want_val.shape)
    assert bool(torch.isfinite(got_der).all()) and bool(torch.isfinite(got_val).all())
    weights = torch.tensor([float(diag.abs().max())] + [sum(abs(w) for w, _, _ in p.terms) for p in pauli] + [1.0, 1.0], dtype=torch.float64)
    val_err = float(((got_val - want_val).abs().amax(dim=(1, 2)) / weights).max())
    print(f"PAIR N={n} P={count} {solver_name} D={n_dir}: values, largest error / row weight {val_err:.2e}")
    for d in range(n_dir):
        scale = float(want_der[d].abs().max())
        err = float((got_der[d] - want_der[d]).abs().max())
        print(f"PAIR N={n} P={count} {solver_name} D={n_dir}: direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        if d == n_dir - 1:
            assert float(got_der[d].abs().max()) == 0.0 and scale <= 1e-14  # the zero direction stays exactly zero
        else:
            assert scale > 1e-2  # nothing passes on zeros
            assert err <= ORACLE_RTOL * scale
    assert float(want_val.abs().max()) > 1e-2
    assert val_err <= VALUE_ATOL


def test_xy_emulator_takes_the_tangent_route(cuda_device, monkeypatch):
    from tests.test_gpu_master_equation_sizes import _xy_problem

    sim, ham, _, _ = _xy_problem(3, True, monkeypatch, cuda_device)
    # the sequence of _xy_problem carries no differentiable parameter: scale / shift its tables by leaves
    knobs = torch.tensor([1.0, 0.0], dtype=torch.float64, requires_grad=True)
    ham.amp_tables = ham.amp_tables.detach() * knobs[0]
    ham.det_tables = ham.det_tables.detach() + knobs[1]
    obs = [DiagonalObservable(total_magnetization_diag(3)), observable_set(3)[0]]
    tan = sim.run_sensitivities([knobs], obs, route="tangent")
    assert tan.route == "tangent"
    loop = sim.run_sensitivities([knobs], obs, route="adjoint-loop")
    assert loop.route == "adjoint-loop"
    assert float((tan.values.cpu() - loop.values.cpu()).abs().max()) <= 4e-9
    got, want = tan.grads[0].cpu(), loop.grads[0].cpu()
    assert got.shape == want.shape == (2, len(sim.evaluation_times), 2)
    for o in range(2):  # relative to the observable's largest derivative over both knobs and all times
        scale = float(want[o].abs().max())
        err = float((got[o] - want[o]).abs().max())
        print(f"XY observable {o}: largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 1e-3
        assert err <= PUBLIC_RTOL * scale

def test_geometry_with_pair_terms_on_kets(cuda_device):
    dev = cuda_device
    prob = _problem(8, 3, "KRYLOV_SE", False)
    _, _, _, spec = to_native(prob["terms"], dev, SolverType.KRYLOV_SE, store_states=True)
    spec.pair_terms = prob["pairs"]
    args = (prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), prob["tsave"], prob["psi0"].to(dev), spec)
    kw = dict(d_amp=prob["d_amp"][:3].to(dev), d_det=prob["d_det"][:3].to(dev), d_u=prob["d_u"][:3].to(dev),
              d_psi0=prob["d_psi"][:3].to(dev), flags=_native.TANGENT_PAIR_TERMS)
    _, _, g1 = evolve_geometry(*args, **kw)
    _, _, g2 = evolve_geometry(*args, **kw)
    assert torch.equal(g1, g2)
    with torch.no_grad():
        states, _ = evolve(*args)  # (n_t, B, dim): not normalised — the blocks are not Hermitian
    norm2 = (states.abs() ** 2).sum(-1)
    assert float((norm2 - 1.0).abs().max()) > 1e-3
    err = float((g1[:, :, 0, 0].real - norm2).abs().max() / norm2.max())
    print(f"geometry with pair terms: gram[0,0] against |psi|^2 {err:.2e}")
    assert err <= 1e-12 and float(g1[:, :, 0, 0].imag.abs().max()) <= 1e-12  # sums of 256 products of doubles: rounding only
    ref_states, ref_tangents = prob["ref"]
    want = torch.einsum("txb,tdxb->tbd", ref_states.conj(), ref_tangents[:, :3])
    gerr = float((g1[:, :, 0, 1:].cpu() - want).abs().max() / want.abs().max())
    print(f"geometry with pair terms: <psi|dpsi_d> against the dense reference {gerr:.2e}")
    assert gerr <= ORACLE_RTOL
