"""Density-matrix observables (RydProblem.dm_*; csrc/dm_kernels.hpp, csrc/dm_launch.hpp) past one block: 9 to 12 atoms, every
fidelity width, every composition of the cotangent, the chained kernels and the tape modes, and the grid.y chunking of the four
observable families.  tests/test_gpu_dm_observables.py stops at 7 atoms (2^n = 128: one block, one entry per thread of k_dm_shots).

All cases drive the C ABI through solver.evolve on a doubled register with spec.dm: the rows are functionals of whatever vector is on
the device, so there is no Lindblad solve here.  The vectors are random, complex and deliberately non-Hermitian as matrices.

Which case reaches which line:
  k_dm_shots, seg = 2 / 4 / 16 (running sums inside a segment, off + C[x], whole zero segments, the full 32 KiB C[] at 12 atoms)
                                                                  test_shots_past_one_segment_per_thread (9, 10, 12 atoms)
  k_dm_scatter, xblocks = 2 (blockIdx.x / xblocks, % xblocks)      test_cotangent_entry_by_entry at 9 atoms
  k_dm_trace on several blocks (block_atomic_add across blocks)    test_values_past_one_block (9, 10, 12 atoms)
  k_dm_fidelity grid-stride loop, 4 / 64 trips                    test_values_past_one_block (10 / 12 atoms)
  k_dm_fidelity<1> (no target; one target), <2>, <4>, <8>, <16>, purity off with targets
                                                                  test_every_fidelity_instantiation (4 atoms), ..._at_ten_atoms
  launch_dm_apply: diagonal rows alone (placeholder group, count 0), xm = 0 strings without diagonal rows, fidelities alone
  (g_pur == nullptr), purity alone, base == out with the dense pass skipped
                                                                  test_cotangent_entry_by_entry, compositions a, b, d, e, h
  cotangent injected by the chained tile kernels, wide tiles, tape "steps" / "full" / "partial" (purity: state_at(k))
                                                                  test_native_cotangent_equals_the_route_through_stored_rho
  kmax chunking of grid.y in launch_dm_expect, launch_pauli_expect, launch_overlap_expect, launch_rdm_expect
                                                                  test_grid_y_chunking_of_all_four_families
  workspace read before written at a wide size                    test_a_poisoned_workspace_changes_nothing_at_nine_atoms

Kernel families (asserted from the plan; rydiff.h, kernel_variant: one-launch sweeps up to 12 qubits, the direct kernels while
B * 2^N <= 2^18 — with gradients 2^19 — amplitudes are in flight, except that from 7 * 2^16 (forward only: above 2^18) up to 2^19
amplitudes the chained passes run on small tiles; the chained passes beyond): see FAMILY and ROUTE_CASES.

References (tests/helpers.py, pinned on the CPU by tests/test_dm_reference_host.py): numpy on rho = v.reshape(2^n, 2^n), Pauli strings as
flips and signs of tensor axes; every value comes with the sum of the absolute values of its terms.  Bars:
  values        |got - want| <= 1e-12 * sum|terms| per row: a term passes at most 64 grid-stride trips + 6 shuffle levels + 4 waves +
                1024 block atomics ~ 1.1e3 additions, a-priori bound 1.1e3 * 2 * 2^-53 * sum|terms| = 2.4e-13 * sum|terms|; at 12 atoms one
                dropped entry is ~6e-8 * sum|terms|
  cotangents    |got - want| <= 64 * 2^-52 * sum|contributions to the entry| (fewer than 32 fused additions per entry)
  two routes    1e-10 relative to the largest entry below 21 doubled qubits, 1e-9 from 21 (tests/test_gpu_pauli_observables.py)
  shots         equality with sample_indices_reference outside |u S - C[x]| <= 4 D 2^-53 S (C = numpy.cumsum), at most 1 % of the shots
                left out; p[x] > 0, monotonicity in u and bitwise repeatability take no tolerance.  u = 0 and u = 1 - 2^-53 lie in the
                band by construction (C[x] = 0 on the leading zero segments; 2^-53 S below C[D - 1]): u = 0 is asserted separately to
                return the first populated entry, which no rounding can change."""
import functools

import numpy as np
import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.observables import DensityMatrixObservables, PauliObservable, expect_pauli
from pulser_diff_amd.shots import SHOT_NONE, ShotRequest, sample_indices_reference
from pulser_diff_amd.solver import SolverType, evolve
from tests.helpers import (DM_SHOTS, dm_cotangent_reference, dm_rows_reference, dm_shot_inputs, ket_pauli_cotangent, ket_pauli_row, pauli_string_apply,
                           random_terms, rel_err, shot_band, to_native)
from tests.test_gpu_dm_observables import _paulis
from tests.test_gpu_workspace_contents import _filled

pytestmark = pytest.mark.gpu

_BY_NAME = {name: name for name in _native.KERNEL_FAMILIES}  # (a renamed family is a KeyError here, not a silently different case)
LANES, PERSISTENT, DIRECT, CHAINED = (_BY_NAME[k] for k in ("lanes", "persistent", "direct", "chained-tiles"))
# atoms -> family of the cases with two trajectories (B = 1 at 12 atoms), forward only and with a gradient on psi0 alike:
# 4 / 8 doubled qubits: one-launch sweeps; 18 qubits, B = 2: 2^19 amplitudes in flight, chained passes on small tiles; 20 / 24: chained
FAMILY = {2: LANES, 4: PERSISTENT, 9: CHAINED, 10: CHAINED, 12: CHAINED}
VALUE_RTOL = 1e-12
COT_BAR = 64 * 2.0 ** -52
TSAVE = (0.0, 0.0037, 0.0091)


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


def _problem(n, dev, store_states=True):
    terms = random_terms(2 * n, 9, 0.002, seed=5100 + n, local=True)
    return to_native(terms, dev, SolverType.KRYLOV_SE, store_states=store_states)


# ----------------------------------------------------------------------------------------------------------------------
# 1. / 2. values
# ----------------------------------------------------------------------------------------------------------------------
def _check_values(dev, tag, n, batch, n_diag, paulis, n_fid, fid_batch, purity, tsave=TSAVE):
    """One evolve call with the given rows; every row at every save point against dm_rows_reference on the states the call stored."""
    dim = 2 ** n
    gen = torch.Generator().manual_seed(6000 + 17 * n + n_fid)
    amp, det, u, spec = _problem(n, dev)
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    diag = _randn(gen, n_diag, dim) if n_diag else None
    targets = _randn(gen, n_fid, fid_batch, dim, cplx=True) if n_fid else None
    spec.dm = DensityMatrixObservables(n, diag=None if diag is None else diag.to(dev), pauli=paulis or None,
                                       targets=None if targets is None else targets.to(dev), purity=purity)
    states, expect = evolve(amp, det, u, torch.tensor(tsave, dtype=torch.float64), v0.to(dev), spec, None)
    torch.cuda.synchronize()
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n], spec.options["_last_stats"]
    kinds = [("diag", n_diag), ("pauli", len(paulis)), ("fidelity", n_fid), ("purity", int(purity))]
    assert expect.shape == (sum(c for _, c in kinds), len(tsave), batch)
    got = expect.cpu().numpy()
    st = states.cpu().numpy()
    del states
    assert np.array_equal(st[0], v0.numpy())  # save point 0 is psi0, bitwise
    worst = {name: 0.0 for name, c in kinds if c}
    for k in range(len(tsave)):
        for b in range(batch):
            tg = () if targets is None else targets[:, b if fid_batch > 1 else 0].numpy()
            want, tot = dm_rows_reference(st[k, b], n, () if diag is None else diag.numpy(), paulis, tg, purity)
            ratio = np.abs(got[:, k, b] - want) / tot
            r = 0
            for name, c in kinds:
                if c:
                    worst[name] = max(worst[name], float(ratio[r:r + c].max()))
                r += c
            assert (ratio <= VALUE_RTOL).all(), (k, b, np.flatnonzero(ratio > VALUE_RTOL), ratio.max())
    for name, w in worst.items():
        print(f"DM-WIDE-VAL {tag} n={n} B={batch} n_fid={n_fid} fid_batch={fid_batch} purity={int(purity)} {name}: "
              f"{w:.2e} of sum|terms| (bar {VALUE_RTOL:.0e})")


@pytest.mark.parametrize("n,batch,fid_batch,n_fid,tsave", [(9, 2, 1, 3, TSAVE), (10, 2, 1, 16, TSAVE), (10, 2, 2, 16, TSAVE),
                                                          (12, 1, 1, 3, TSAVE[:2])])
def test_values_past_one_block(cuda_device, n, batch, fid_batch, n_fid, tsave):
    """k_dm_trace on 2 / 4 / 16 blocks per row, k_dm_fidelity with 1 / 4 / 64 grid-stride trips; 12 atoms forward only (268 MB per state)."""
    _check_values(cuda_device, "past-one-block", n, batch, 2, _paulis(n), n_fid, fid_batch, True, tsave)


FID_CASES = [(0, True, 1)] + [(nf, pur, fb) for nf in (1, 2, 3, 5, 8, 9, 16) for pur in (True, False) for fb in (1, 2)]


@pytest.mark.parametrize("n_fid,purity,fid_batch", FID_CASES)
def test_every_fidelity_instantiation(cuda_device, n_fid, purity, fid_batch):
    """k_dm_fidelity<1> (purity alone; one target), <2>, <4> (3), <8> (5, 8), <16> (9, 16), each with the purity row on and off and with
    shared and per-trajectory targets; 4 atoms, B = 2, no diagonal or Pauli rows."""
    _check_values(cuda_device, "fid", 4, 2, 0, [], n_fid, fid_batch, purity)


@pytest.mark.parametrize("n_fid,purity,fid_batch", [(0, True, 1), (16, False, 2), (16, True, 1)])
def test_every_fidelity_instantiation_at_ten_atoms(cuda_device, n_fid, purity, fid_batch):
    _check_values(cuda_device, "fid", 10, 2, 0, [], n_fid, fid_batch, purity, TSAVE[:2])


# ----------------------------------------------------------------------------------------------------------------------
# 3. cotangents, entry by entry
# ----------------------------------------------------------------------------------------------------------------------
def _z_paulis(n):
    return [PauliObservable(n, [(0.8, {0: "Z"}), (-0.3, {0: "Z", n - 1: "Z"})]), PauliObservable(n, [(0.5, {n - 1: "Z"})])]


def _flip_paulis(n):
    """No string with xm = 0."""
    a, z = 0, n - 1
    return [PauliObservable(n, [(0.7, {a: "Y", z: "Y"}), (-1.1, {a: "X", z: "Y"}), (0.9, {z: "Y"})]),
            PauliObservable(n, [(-0.8, {a: "X"}), (0.5, {a: "Y", z: "X"})])]


def _ket_pauli(n):
    """One ket-style observable on the doubled register: Y on row and column qubits, first, last and middle."""
    return PauliObservable(2 * n, [(0.6, {0: "Y", 2 * n - 1: "Y", n: "X"}), (-0.9, {n - 1: "Z", 0: "Y"}), (0.4, {1: "X"})])


# composition -> (diagonal tables, Pauli rows, targets, fid_batch = B, purity, ket-style Pauli row, ket-style overlap)
COMPOSITIONS = {
    "a-diag-only": (2, None, 0, False, False, False, False),
    "b-z-strings-only": (0, _z_paulis, 0, False, False, False, False),
    "c-diag-and-flip-strings": (2, _flip_paulis, 0, False, False, False, False),
    "d-fidelities-only": (0, None, 3, False, False, False, False),
    "e-purity-only": (0, None, 0, False, True, False, False),
    "f-everything": (2, _paulis, 3, True, True, False, False),
    "g-everything-and-ket-rows": (2, _paulis, 3, False, True, True, True),
    "h-diag-and-ket-pauli-in-place": (2, None, 0, False, False, True, False),
}


@pytest.mark.parametrize("comp", list(COMPOSITIONS))
@pytest.mark.parametrize("n", [4, 9])
def test_cotangent_entry_by_entry(cuda_device, n, comp):
    """Only save point 0 (= psi0) carries weight, so psi0.grad IS the cotangent launch_observable_cotangent formed there; compared entry
    by entry with the dense matrix rydiff.h writes down.  Two weights are exact zeros (the go == 0.0 skips)."""
    n_diag, make_paulis, n_fid, per_traj, purity, with_kp, with_ov = COMPOSITIONS[comp]
    dim, batch = 2 ** n, 2
    gen = torch.Generator().manual_seed(7000 + n)
    amp, det, u, spec = _problem(n, cuda_device)
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    diag = _randn(gen, max(n_diag, 1), dim)[:n_diag]
    targets = _randn(gen, max(n_fid, 1), batch if per_traj else 1, dim, cplx=True)[:n_fid]
    paulis = make_paulis(n) if make_paulis else []
    spec.dm = DensityMatrixObservables(n, diag=diag.to(cuda_device) if n_diag else None, pauli=paulis or None,
                                       targets=targets.to(cuda_device) if n_fid else None, purity=purity)
    ket_pauli = _ket_pauli(n)
    phi = _randn(gen, 1, batch, dim * dim, cplx=True)
    if with_kp:
        spec.pauli = [ket_pauli]
    if with_ov:
        spec.overlaps = phi.to(cuda_device)
    n_ket = int(with_kp) + 2 * int(with_ov)
    n_dm = spec.dm.rows()
    w = torch.zeros(n_ket + n_dm, len(TSAVE), batch, dtype=torch.float64)
    w[:, 0] = _randn(gen, n_ket + n_dm, batch)
    # two density-matrix rows with an exact zero weight (the go == 0.0 skips): from three rows on, row 1 for trajectory 0 and another
    # row for both trajectories; with two rows, row 1 for trajectory 0 and row 0 for trajectory 1; the purity alone has one row, zero
    # for trajectory 0 (whose whole cotangent is then an exact zero)
    w[n_ket + (1 % n_dm), 0, 0] = 0.0
    if n_dm > 2:
        w[n_ket + (n_dm - 2 if n_dm > 3 else 2), 0, :] = 0.0
    elif n_dm == 2:
        w[n_ket, 0, 1] = 0.0
    assert int((w[n_ket:, 0] == 0).any(dim=1).sum()) == min(n_dm, 2)
    psi0 = v0.to(cuda_device).requires_grad_(True)
    _, expect = evolve(amp, det, u, torch.tensor(TSAVE, dtype=torch.float64), psi0, spec, None)
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n], spec.options["_last_stats"]
    assert expect.shape == w.shape
    (expect * w.to(cuda_device)).sum().backward()
    torch.cuda.synchronize()
    got = psi0.grad.cpu().numpy()
    assert np.isfinite(got).all(), (comp, np.argwhere(~np.isfinite(got))[:8])
    worst = 0.0
    for b in range(batch):
        g = w[:, 0, b].numpy()
        tg = targets[:, b if per_traj else 0].numpy() if n_fid else ()
        want, tot = dm_cotangent_reference(v0[b].numpy(), n, g[n_ket:], diag.numpy(), paulis, tg, purity)
        if with_kp:
            c, t = ket_pauli_cotangent(v0[b].numpy(), 2 * n, ket_pauli.terms, g[0])
            want, tot = want + c, tot + t
        if with_ov:
            g_re, g_im = g[int(with_kp)], g[int(with_kp) + 1]
            want = want + (g_re + 1j * g_im) * phi[0, b].numpy()
            tot = tot + (abs(g_re) + abs(g_im)) * np.abs(phi[0, b].numpy())
        err = np.abs(got[b] - want)
        bad = np.flatnonzero(~(err <= COT_BAR * tot))  # (a NaN is not within the bar)
        assert bad.size == 0, (comp, b, bad[:8] // dim, bad[:8] % dim, err[bad[:8]], tot[bad[:8]])
        if (tot > 0).any():  # (purity alone with a zero weight: the whole cotangent of that trajectory is an exact zero)
            worst = max(worst, float((err[tot > 0] / tot[tot > 0]).max()))
    print(f"DM-WIDE-COT n={n} {comp}: {worst:.2e} of sum|contributions| (bar {COT_BAR:.2e})")


# ----------------------------------------------------------------------------------------------------------------------
# 4. the cotangent through the chained kernels and the tape modes
# ----------------------------------------------------------------------------------------------------------------------
# (doubled qubits, tape, kernel variant) -> family.  B = 1 everywhere.  14 qubits: variant 2 = chained passes on 2^12-amplitude tiles
# (the variant tests/test_gpu_pauli_observables.py takes at 14).  18 qubits, automatic: 2^18 amplitudes with gradients is below the
# 7 * 2^16 of the small tiles and within the 2^19 of the direct kernels, so the automatic choice is DIRECT (with the full tape); the
# chained kernels with the full tape run in the extra case (18, "full", 2).  20: chained; 22: chained on wide tiles (2^13 amplitudes).
ROUTE_CASES = {(14, "steps", 2): CHAINED, (14, "partial", 2): CHAINED, (18, "full", 0): DIRECT, (18, "full", 2): CHAINED,
               (20, "partial", 0): CHAINED, (22, "steps", 0): CHAINED}
ROUTE_TSAVE = (0.0, 0.0041, 0.0102, 0.0163, 0.024)


@functools.lru_cache(maxsize=None)
def _route_inputs(nq):
    """CPU inputs shared by the two routes and by the poisoned-workspace case; never modified."""
    n = nq // 2
    dim = 2 ** n
    gen = torch.Generator().manual_seed(8000 + nq)
    psi = _randn(gen, 1, dim * dim, cplx=True)
    diag = _randn(gen, 2, dim)
    targets = _randn(gen, 2, 1, dim, cplx=True)
    targets = targets / targets.norm(dim=2, keepdim=True)
    weights = _randn(gen, 2 + 2 + 2 + 1, len(ROUTE_TSAVE), 1)
    return random_terms(nq, 13, 0.002, seed=900 + nq, local=False), psi / psi.norm(), diag, targets, weights


def _rows_from_stored_rho(states, n, diag, paulis, targets):
    """The seven rows by torch on stored states (n_t, 1, 4^n), on their device, differentiable."""
    dim = 2 ** n
    rho = states.reshape(states.shape[0], dim, dim)
    rows = [(d * rho.diagonal(dim1=1, dim2=2).real).sum(1) for d in diag]
    rows += [expect_pauli(p, rho[..., None]).real for p in paulis]
    rows += [torch.einsum("x,txy,y->t", t[0].conj(), rho, t[0]).real for t in targets]
    rows.append((states.real ** 2 + states.imag ** 2).sum(dim=(1, 2)))
    return torch.stack(rows)[:, :, None]


def _route(dev, nq, tape, variant, native):
    terms, psi, diag, targets, _ = _route_inputs(nq)
    n = nq // 2
    paulis = _paulis(n)
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=not native)
    spec.kernel_variant = variant
    spec.tape = tape
    if tape == "partial":
        spec.tape_steps = 2
    diag, targets = diag.to(dev), targets.to(dev)
    if native:
        spec.dm = DensityMatrixObservables(n, diag=diag, pauli=paulis, targets=targets, purity=True)
    leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True),
              torch.tensor(ROUTE_TSAVE, dtype=torch.float64, requires_grad=True), psi.to(dev).requires_grad_(True)]
    states, expect = evolve(*leaves, spec, None)
    assert spec.options["_last_stats"]["kernel_family"] == ROUTE_CASES[(nq, tape, variant)], spec.options["_last_stats"]
    if not native:
        expect = _rows_from_stored_rho(states, n, diag, paulis, targets)
    return leaves, expect


def _grads_of(loss, leaves, retain):
    return [g.detach().cpu().numpy() for g in torch.autograd.grad(loss, leaves, retain_graph=retain)]


LEAF_NAMES = ("amp", "det", "u", "tsave", "psi0")


@pytest.mark.parametrize("nq,tape,variant", list(ROUTE_CASES))
def test_native_cotangent_equals_the_route_through_stored_rho(cuda_device, nq, tape, variant):
    """The same loss over all four differentiable row kinds two ways: from the native rows (cotangent formed per save point in the one
    reused workspace buffer and injected by the adjoint sweep) and by torch from the stored states of a second run (grad_states).
    One-hot weights at save point 1 and at the last one, then all save points: stale content of the reused buffer would show."""
    weights = _route_inputs(nq)[4].to(cuda_device)
    tol = 1e-10 if nq < 21 else 1e-9
    leaves_a, exp_a = _route(cuda_device, nq, tape, variant, True)
    leaves_b, exp_b = _route(cuda_device, nq, tape, variant, False)
    err = rel_err(exp_a.detach().cpu().numpy(), exp_b.detach().cpu().numpy())
    print(f"DM-WIDE-ROUTES N={nq} tape={tape} variant={variant} rows: {err:.2e} (bar {tol:.0e})")
    assert err < tol
    one_hot = [torch.zeros_like(weights) for _ in range(2)]
    one_hot[0][:, 1] = weights[:, 1]
    one_hot[1][:, -1] = weights[:, -1]
    for label, w, retain in (("k=1", one_hot[0], True), ("k=last", one_hot[1], True), ("all", weights, False)):
        ga = _grads_of((w * exp_a).sum(), leaves_a, retain)
        gb = _grads_of((w * exp_b).sum(), leaves_b, retain)
        errs = {name: rel_err(a, b) for name, a, b in zip(LEAF_NAMES, ga, gb)}
        print(f"DM-WIDE-ROUTES N={nq} tape={tape} variant={variant} weights {label}: "
              + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bar {tol:.0e})")
        for name, e in errs.items():
            assert e < tol, (label, name, e)


def test_a_poisoned_workspace_changes_nothing_at_nine_atoms(cuda_device, monkeypatch):
    """The (18, "full") configuration above with every workspace filled with quiet NaNs against zero-filled ones
    (tests/test_gpu_workspace_contents.py): the cotangent buffer, the string tables and the tape are written before they are read."""
    weights = _route_inputs(18)[4].to(cuda_device)
    out = {}
    for name, value in (("zeros", 0.0), ("nans", float("nan"))):
        monkeypatch.setattr(S, "_new_workspace", _filled(value))
        leaves, expect = _route(cuda_device, 18, "full", 0, True)
        grads = _grads_of((weights * expect).sum(), leaves, False)
        out[name] = dict(zip(("rows",) + LEAF_NAMES, [expect.detach().cpu().numpy()] + grads))
    for key in out["zeros"]:
        assert np.isfinite(out["nans"][key]).all(), f"{key}: a region is read before it is written"
        err = rel_err(out["nans"][key], out["zeros"][key])
        print(f"DM-WIDE-POISON N=18 {key}: {err:.2e} (bar 1e-12)")
        assert err < 1e-12, key


# ----------------------------------------------------------------------------------------------------------------------
# 5. shots past one segment per thread
# ----------------------------------------------------------------------------------------------------------------------
def _shot_run(n, dev, v0, uniforms):
    amp, det, u, spec = _problem(n, dev)
    spec.dm = DensityMatrixObservables(n, shots=True)
    spec.shots = ShotRequest(DM_SHOTS, times=[0, 2], uniforms=uniforms)
    states, _ = evolve(amp, det, u, torch.tensor(TSAVE, dtype=torch.float64), v0.to(dev), spec, None)
    torch.cuda.synchronize()
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n], spec.options["_last_stats"]
    dim = 2 ** n
    diagonal = states.reshape(len(TSAVE), v0.shape[0], dim, dim).diagonal(dim1=2, dim2=3).real
    return diagonal.clamp(min=0.0).cpu().numpy(), spec.shots.indices.cpu().numpy()


@pytest.mark.parametrize("n,batch", [(9, 2), (10, 2), (12, 1)])
def test_shots_past_one_segment_per_thread(cuda_device, n, batch):
    """seg = 2, 4, 16 entries per thread.  The diagonal of v0 (tests/helpers.py: dm_shot_inputs; pinned on the CPU by
    tests/test_dm_reference_host.py): random sign, the first two / last three / four middle thread segments dead, every third live
    entry zero; uniforms with 0 and 1 - 2^-53."""
    v0, uniforms = dm_shot_inputs(n, batch, 1100 + n)
    p_all, got = _shot_run(n, cuda_device, v0, uniforms)
    assert got.shape == (2, batch, DM_SHOTS)
    left_out = 0
    for si, k in enumerate((0, 2)):
        want = sample_indices_reference(p_all[k], uniforms[si].numpy())
        for b in range(batch):
            p, uu, x = p_all[k, b], uniforms[si, b].numpy(), got[si, b]
            assert (x < 2 ** n).all() and (p[x] > 0).all()  # never an x with p[x] == 0, boundary shots included
            near = shot_band(p, uu)
            left_out += int(near.sum())
            assert (x[~near] == want[b][~near]).all(), (k, b, np.flatnonzero(x != want[b])[:8])
            pop = np.flatnonzero(p > 0)
            assert x[0] == pop[0]  # u = 0: the first populated entry (at k = 0: in the third segment or later)
            # u = 1 - 2^-53: the last populated entry, through C[last] > tau or through the l == D fallback alike.  Either prefix sum is
            # within D 2^-53 S of the exact one, so a last step p[last] above the band width keeps C[x] below tau for every x < last.
            assert p[pop[-1]] > 4.0 * len(p) * 2.0 ** -53 * p.sum() and x[1] == pop[-1], (k, b, x[1], pop[-2:])
            assert (np.diff(x[np.argsort(uu, kind="stable")]) >= 0).all()  # non-decreasing in u
    print(f"DM-WIDE-SHOTS n={n} B={batch}: {left_out} of {got.size} shots inside the band (cap {0.01 * got.size:.0f})")
    assert left_out <= 0.01 * got.size, left_out
    _, again = _shot_run(n, cuda_device, v0, uniforms)
    assert np.array_equal(got, again)  # bit-reproducible
    _, none = _shot_run(n, cuda_device, torch.zeros_like(v0), uniforms)
    assert (none == SHOT_NONE).all()


# ----------------------------------------------------------------------------------------------------------------------
# 6. grid.y chunking: B * n_tsave > 65535 in the four observable families at once
# ----------------------------------------------------------------------------------------------------------------------
def test_grid_y_chunking_of_all_four_families(cuda_device):
    """2 atoms (4 doubled qubits, one-launch sweep), B = 256 different vectors, 257 irregular save points: B * n_tsave = 65792, kmax = 255,
    so launch_dm_expect, launch_pauli_expect, launch_overlap_expect and launch_rdm_expect each run a second chunk of two save points
    (a.k0 = k0 + k, a.v + k * kstride).  Every row at every (k, b) against numpy on the stored states; k >= 255 asserted separately."""
    n, batch, n_t = 2, 256, 257
    dim, nq = 4, 4
    gen = torch.Generator().manual_seed(9000)
    amp, det, u, spec = _problem(n, cuda_device)
    steps = 0.2 + torch.rand(n_t - 1, generator=gen, dtype=torch.float64) ** 2
    tsave = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(steps, 0)]) * (0.0159 / float(steps.sum()))
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    diag = _randn(gen, 1, dim)
    targets = _randn(gen, 2, batch, dim, cplx=True)
    dm_pauli = _paulis(n)[:1]
    ket_pauli = _ket_pauli(n)
    phi = _randn(gen, 1, batch, dim * dim, cplx=True)
    spec.dm = DensityMatrixObservables(n, diag=diag.to(cuda_device), pauli=dm_pauli, targets=targets.to(cuda_device), purity=True)
    spec.pauli = [ket_pauli]
    spec.overlaps = phi.to(cuda_device)
    spec.rdms = [0b0101]  # qubits 0 and 2: one row qubit, one column qubit
    states, expect = evolve(amp, det, u, tsave, v0.to(cuda_device), spec, None)
    torch.cuda.synchronize()
    assert spec.options["_last_stats"]["kernel_family"] == LANES, spec.options["_last_stats"]
    assert batch * n_t > 65535 and expect.shape == (1 + 2 + 32 + 5, n_t, batch)
    got = expect.cpu().numpy()
    assert np.isfinite(got).all(), np.argwhere(~np.isfinite(got))[:8]
    st = states.cpu().numpy()  # (n_t, B, 16)
    assert np.array_equal(st[0], v0.numpy())
    want, tot = np.zeros_like(got), np.zeros_like(got)
    # ket-style rows: Pauli, overlap (Re, Im), reduced density matrix of qubits (0, 2) (entry (a, a') at 2 (4 a + a'), Re then Im)
    t = np.moveaxis(st.reshape(n_t, batch, 2, 2, 2, 2), (2, 3, 4, 5), (0, 1, 2, 3))  # qubit axes first
    want[0], tot[0] = ket_pauli_row(t, nq, ket_pauli.terms)
    c = (phi[0].numpy().conj()[None] * st).sum(-1)
    want[1], want[2] = c.real, c.imag
    tot[1] = tot[2] = (np.abs(phi[0].numpy())[None] * np.abs(st)).sum(-1)
    m = st.reshape(n_t, batch, 2, 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n_t, batch, 4, 4)  # (a = (q0, q2), e = (q1, q3))
    rdm = np.einsum("kbae,kbce->kbac", m, m.conj())
    rdm_tot = np.einsum("kbae,kbce->kbac", np.abs(m), np.abs(m))
    for a in range(4):
        for a2 in range(4):
            r = 3 + 2 * (4 * a + a2)
            want[r], want[r + 1] = rdm[:, :, a, a2].real, rdm[:, :, a, a2].imag
            tot[r] = tot[r + 1] = rdm_tot[:, :, a, a2]
    # density-matrix rows: diagonal table, Pauli observable, two per-trajectory targets, purity
    rho = st.reshape(n_t, batch, dim, dim)
    re_diag = np.einsum("kbxx->kbx", rho).real
    want[35] = (diag[0].numpy() * re_diag).sum(-1)
    tot[35] = np.abs(diag[0].numpy() * re_diag).sum(-1)
    ta = np.moveaxis(st.reshape(n_t, batch, 2, 2, dim), (2, 3, 4), (0, 1, 2))  # atom axes of the row index first
    for w_s, x, z in dm_pauli[0].terms:
        want[36] += w_s * np.einsum("xxkb->kb", pauli_string_apply(ta, x, z, n).reshape(dim, dim, n_t, batch)).real
        tot[36] += abs(w_s) * np.abs(np.einsum("xxkb->xkb", pauli_string_apply(ta, x, 0, n).reshape(dim, dim, n_t, batch))).sum(0)
    for o in range(2):
        ph = targets[o].numpy()
        want[37 + o] = np.einsum("bx,kbxy,by->kb", ph.conj(), rho, ph).real
        tot[37 + o] = np.einsum("bx,kbxy,by->kb", np.abs(ph), np.abs(rho), np.abs(ph))
    want[39] = tot[39] = (np.abs(st) ** 2).sum(-1)
    ratio = np.abs(got - want) / np.where(tot > 0, tot, 1.0)
    assert (np.abs(got - want)[tot == 0] == 0).all()  # (Im of the diagonal RDM entries: an exact 0)
    names = (("pauli", slice(0, 1)), ("overlap", slice(1, 3)), ("rdm", slice(3, 35)), ("dm-diag", slice(35, 36)), ("dm-pauli", slice(36, 37)),
             ("dm-fidelity", slice(37, 39)), ("dm-purity", slice(39, 40)))
    for name, sl in names:
        first, second = float(ratio[sl, :255].max()), float(ratio[sl, 255:].max())
        print(f"DM-WIDE-CHUNK {name}: chunk 1 {first:.2e}, chunk 2 (k >= 255) {second:.2e} of sum|terms| (bar {VALUE_RTOL:.0e})")
    for name, sl in names:
        bad = np.argwhere(~(ratio[sl, 255:] <= VALUE_RTOL))  # (a NaN is not within the bar)
        assert bad.size == 0, (name, "second chunk", bad[:8])
        bad = np.argwhere(~(ratio[sl, :255] <= VALUE_RTOL))
        assert bad.size == 0, (name, "first chunk", bad[:8])
