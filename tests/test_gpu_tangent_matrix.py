"""Forward-mode (tangent) sweep, entry by entry against a plain dense forward-mode reference, over the direction widths, row layouts,
batch shapes and chunkings the kernels and launches distinguish — and, at 19 qubits, the reductions beyond one grid trip.

Parts (the reference is tests.helpers.tangent_dense_reference: the oracle's discrete map advanced with the block identity
exp([[A, dA], [0, A]]), no autograd, checked against reverse-mode autograd in tests/test_tangent_host.py; the rows are formed from
its states in float64 on the CPU by tests.helpers.tangent_rows_reference):

B. dexpect[d, row, k, b] of evolve_tangent against the reference, ORACLE_RTOL = 1e-8 relative to the largest entry of direction d
   (the project's bar for native against dense oracle, gradients); expect against the reference's values, 1e-9 times the weight
   of the row's operator (max |diagonal|, sum |w_s|, 1 for a normalised target), as in the overlap and Pauli value tests.  The
   largest reference entry of every direction and row family (diagonal, Pauli, overlap) must exceed 1e-2.
   k_factor_tangent is instantiated for 1, 2, 3, 4, 6, 8 directions (5 and 7 are padded with a zero direction) and loads the
   partners of 8 / 4 / 2 flip bits at a time: the widths 2, 4, 5, 6, 7 at 9 qubits (two blocks, bit 8 pairs across them; 9 driven
   qubits) and 4, 5, 6, 7 at 3 qubits (3 driven qubits against chunks of 2: a short last chunk at every width); row layouts with
   0 and 3 diagonal rows, 3 overlaps (the <4> instantiation, shared and per-trajectory targets), Pauli rows alone; B = 1 and
   B = 3; a single tangent input next to a padded direction; 13 directions = a chunk of 8 and a padded chunk of 5 through one
   workspace.
C. 19 qubits, where the reductions' grids (capped at 1024 blocks of 256) loop twice: (1) with a tangent of psi0 alone,
   dpsi(t) = U(t) d_psi0, so evolve(store_states=True) on the columns [psi0, d_psi0[d]] gives psi and dpsi without any tangent
   kernel and every row follows in float64 torch: 1e-10 relative to the largest entry (one native value route against another);
   (2) two duality cases against the native adjoint at DUALITY_RTOL = 1e-9.

Measured on an MI355X (largest error over the directions and cases of each group, relative to the direction's largest entry;
values: largest error over the row weight):
  B  9 qubits KRYLOV_SE widths 2..7   1.1e-12 (values 1.1e-14)     9 qubits DP5_SE width 5          2.7e-14 (values 4.9e-16)
     3 qubits KRYLOV_SE widths 4..7   1.1e-12 (values 5.2e-14)     3 qubits DP5_SE widths 4..7      1.6e-13 (values 8.1e-14)
     row layouts, 3 qubits            7.1e-13 (values 5.2e-14)     row layouts, 9 qubits            1.5e-12 (values 1.1e-14)
     B = 1, 8 directions              1.6e-12 (values 3.9e-14)     B = 3, per-trajectory tables     3.8e-13 (values 8.5e-14)
     only d_amp / d_u / d_psi0        2.0e-13 / 2.6e-13 / 3.8e-14  13 directions, 3 / 9 qubits      4.1e-13 / 1.6e-13
     — against the bars 1e-8 (tangents) and 1e-9 (values)
  C  19 qubits against stored states  1.8e-15 (values 1.8e-15 absolute) against 1e-10
     19 qubits duality                KRYLOV_SE 4.1e-15, DP5_SE 6.3e-15 against 1e-9
Reference CPU time on 16 cores (on 8 cores): 9 qubits KRYLOV_SE, 7 directions, per-trajectory tables, two
intervals 5.6 s (11.9 s); 9 qubits DP5_SE, 5 directions, three pieces 3.9 s (7.4 s); 13 directions at 9 qubits 4.4 s (10.3 s); one
tangent input, 5 directions 1.7 s (4.1 s).
"""
import time
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import restatement as R
from pulser_diff_amd.observables import StateOverlap, expect_pauli, pack_overlaps
from pulser_diff_amd.solver import SolverType, evolve, evolve_tangent
from pulser_diff_amd.utils import total_magnetization_diag
from tests.helpers import random_terms, tangent_dense_reference, tangent_rows_reference, to_native
from tests.test_gpu_tangent import DUALITY_RTOL, ORACLE_RTOL, _randn, observable_set

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9      # values against the dense oracle (tests/test_gpu_pauli_observables.py, tests/test_gpu_overlap_observables.py)
NATIVE_RTOL = 1e-10    # one native value route against another
N_SAMPLES, DT = 41, 0.004
TSAVE = (0.0, 0.0313, 0.0622, 0.0951)  # off the sample grid
TSAVE_9 = TSAVE[:3]  # 9 qubits: two intervals keep the 7-direction, per-trajectory reference (28 block exponentials of 1024 x 1024) near 10 s
# DP5_SE at 9 qubits: three pieces ([0, 1.9], [1.9, 4.0], [4.0, 4.3] ns), each below the native sub-step limit of 4.4 ns (and
# below it up to a generator half width of 570 rad/us, where the limit has shrunk to 2.1 ns): one CF4 step per piece on both sides
TSAVE_DP5_SHORT = (0.0, 0.0019, 0.0043)


def _terms_with_tables(terms, amp_rows, det_rows):
    """HamTerms with the same structure as `terms` and the given table rows (amp_terms() / det_terms() order)."""
    out = R.HamTerms(terms.n_qubits, terms.u_pairs, None, None, terms.dt, terms.n_samples)
    out.extra_amp = [(amp_rows[k], tg) for k, (_, tg) in enumerate(terms.amp_terms())]
    out.extra_det = [(det_rows[k], tg) for k, (_, tg) in enumerate(terms.det_terms())]
    return out


@lru_cache(maxsize=None)
def _problem(n, batch, cb, n_dir):
    """One seeded problem on the CPU: tables (cb, K, n_samples) that really differ per trajectory, psi0 (B, dim), all four tangent
    inputs for n_dir directions scaled like the inputs they perturb, overlap targets, random diagonals."""
    terms = random_terms(n, N_SAMPLES, DT, seed=1300 + n, local=True, phase=True)
    amp, det, u, _ = to_native(terms, "cpu", SolverType.KRYLOV_SE, batch_tables=cb)
    gen = torch.Generator().manual_seed(52000 + 97 * n + 13 * batch + cb)
    if cb > 1:
        amp = amp * (1.0 + 0.1 * _randn(gen, cb, 1, 1))
        det = det * (1.0 + 0.1 * _randn(gen, cb, 1, 1))
    dim = 2**n
    psi0 = _randn(gen, batch, dim, cplx=True)
    psi0 = psi0 / psi0.norm(dim=1, keepdim=True)
    unit = lambda t: t / t.norm(dim=0, keepdim=True)  # noqa: E731
    # overlap targets the tangents have weight on (a random target would give entries of order 2^(-n/2) |dpsi|): psi0, its
    # single-qubit flips with seeded complex weights (where a drive tangent sends it first) and a random part, then normalised
    idx = torch.arange(dim)
    near = lambda: psi0.T + sum(complex(_randn(gen, 1, cplx=True)) * psi0.T[idx ^ (1 << j)] for j in range(n))  # noqa: E731
    mixed = lambda t, cols: unit(t + 0.5 * float(t.norm(dim=0).mean()) * unit(_randn(gen, dim, cols, cplx=True)))  # noqa: E731
    prob = {
        "n": n, "batch": batch, "cb": cb, "terms": terms, "amp": amp, "det": det, "u": u, "psi0": psi0,
        # (the table tangents 8 times the tables' size: KRYLOV_SE reads the tables at one time per interval, and with two
        # intervals a tangent of the tables' own size leaves some Pauli rows of a direction below the 1e-2 the checks ask for)
        "d_amp": 8.0 * float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True),
        "d_det": 8.0 * float(det.abs().max()) * _randn(gen, n_dir, *det.shape),
        "d_u": float(u.abs().max()) * _randn(gen, n_dir, *u.shape) if u.numel() else None,
        "d_psi0": _randn(gen, n_dir, batch, dim, cplx=True) / np.sqrt(dim),
        "targets_shared": [mixed(near().sum(1, keepdim=True), 1)[:, 0] for _ in range(3)],
        "targets_traj": [mixed(near(), batch) for _ in range(3)],
        "diags": torch.cat([total_magnetization_diag(n)[None], _randn(gen, 2, dim)]),  # sum Z, two random diagonals
    }
    prob["ref_terms"] = ([_terms_with_tables(terms, amp[b], det[b]) for b in range(batch)] if cb > 1
                         else _terms_with_tables(terms, amp[0], det[0]))
    return prob


def _inputs(prob, which, d0, d1):
    """The tangent inputs of directions d0:d1 named in `which` (a / d / u / p), or None."""
    pick = lambda key, flag: prob[key][d0:d1] if (flag in which and prob[key] is not None) else None  # noqa: E731
    return pick("d_amp", "a"), pick("d_det", "d"), pick("d_u", "u"), pick("d_psi0", "p")


REFERENCE_SECONDS = {}


@lru_cache(maxsize=None)
def _reference(n, batch, cb, n_dir_max, solver_name, tsave, which):
    """Dense states (n_t, dim, B) and tangent states (n_t, n_dir_max, dim, B) of one problem: built once, sliced by the cases."""
    prob = _problem(n, batch, cb, n_dir_max)
    d_amp, d_det, d_u, d_psi = _inputs(prob, which, 0, n_dir_max)
    if cb == 1:  # shared tables: (n_dir, K, n)
        d_amp = None if d_amp is None else d_amp[:, 0]
        d_det = None if d_det is None else d_det[:, 0]
    t0 = time.perf_counter()
    out = tangent_dense_reference(prob["ref_terms"], d_amp, d_det, d_u, prob["psi0"].T.contiguous(),
                                  None if d_psi is None else d_psi.permute(0, 2, 1).contiguous(),
                                  torch.tensor(tsave, dtype=torch.float64), SolverType[solver_name])
    REFERENCE_SECONDS[(n, batch, cb, n_dir_max, solver_name, which)] = time.perf_counter() - t0
    return out


def _rows(prob, layout):
    """(diagonal rows or None, Pauli observables, overlap targets) of a named row layout."""
    n, diags = prob["n"], prob["diags"]
    pauli = observable_set(n)
    shared, traj = prob["targets_shared"], prob["targets_traj"]
    return {
        "full": (diags[:1], pauli, traj[:1] if prob["batch"] > 1 else shared[:1]),
        "no_diag": (None, pauli, shared[:1]),                 # n_obs = 0
        "diag3": (diags, pauli, shared[:1]),                  # n_obs = 3: the Pauli and overlap rows sit behind three rows
        "ov3_shared": (diags[:1], pauli, shared),             # three overlaps: the <4> instantiation
        "ov3_traj": (diags[:1], pauli, traj),
        "pauli_only": (None, pauli, []),
    }[layout]


def _check(case_id, prob, solver_name, tsave, which, n_dir, layout, ref, dev):
    """Run evolve_tangent on directions 0:n_dir and compare every entry of dexpect and expect with the dense reference."""
    diag, pauli, targets = _rows(prob, layout)
    n, batch = prob["n"], prob["batch"]
    dim = 2**n
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[solver_name], store_states=False)
    spec.pauli = pauli or None
    spec.overlaps = pack_overlaps([StateOverlap(t) for t in targets], dim, batch, dev) if targets else None
    to_dev = lambda t: None if t is None else t.to(dev)  # noqa: E731
    d_amp, d_det, d_u, d_psi = (to_dev(t) for t in _inputs(prob, which, 0, n_dir))
    expect, dexpect = evolve_tangent(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), torch.tensor(tsave, dtype=torch.float64),
                                     prob["psi0"].to(dev), spec, to_dev(diag), d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi)
    states, tangents = ref
    want_val, want_der = tangent_rows_reference(states, tangents[:, :n_dir], diag, pauli, targets)
    n_diag, n_pauli = (0 if diag is None else len(diag)), len(pauli)
    assert tuple(dexpect.shape) == tuple(want_der.shape) and tuple(expect.shape) == tuple(want_val.shape)
    got_der, got_val = dexpect.cpu(), expect.cpu()
    assert bool(torch.isfinite(got_der).all()) and bool(torch.isfinite(got_val).all())
    weights = ([float(d.abs().max()) for d in (diag if diag is not None else [])] + [sum(abs(w) for w, _, _ in p.terms) for p in pauli]
               + [1.0] * (2 * len(targets)))
    val_err = (got_val - want_val).abs().amax(dim=(1, 2)) / torch.tensor(weights, dtype=torch.float64)
    print(f"{case_id}: values, largest |expect| {float(want_val.abs().max()):.3e}, largest error / row weight {float(val_err.max()):.2e}")
    families = {"diagonal": slice(0, n_diag), "pauli": slice(n_diag, n_diag + n_pauli), "overlap": slice(n_diag + n_pauli, None)}
    worst = 0.0
    for d in range(n_dir):
        scale = float(want_der[d].abs().max())
        err = float((got_der[d] - want_der[d]).abs().max())
        fam = {name: float(want_der[d, sl].abs().max()) for name, sl in families.items() if want_der[d, sl].numel()}
        print(f"{case_id}: direction {d}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative); largest per family "
              + ", ".join(f"{k} {v:.2e}" for k, v in fam.items()))
        assert all(v > 1e-2 for v in fam.values())  # nothing passes on zeros
        assert err <= ORACLE_RTOL * scale
        worst = max(worst, err / scale)
    assert float(want_val.abs().max()) > 1e-2
    assert float(val_err.max()) <= VALUE_ATOL
    return worst


# ---- B. widths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dir", [2, 4, 5, 6, 7])
def test_widths_at_nine_qubits_krylov(n_dir, cuda_device):
    """9 qubits (two 256-thread blocks, bit 8 pairs across them), KRYLOV_SE, B = 2 with per-trajectory tables that differ, all four
    tangent inputs.  One 7-direction reference, sliced."""
    prob = _problem(9, 2, 2, 7)
    ref = _reference(9, 2, 2, 7, "KRYLOV_SE", TSAVE_9, "adup")
    print(f"reference: {REFERENCE_SECONDS[(9, 2, 2, 7, 'KRYLOV_SE', 'adup')]:.1f} s of CPU")
    _check(f"N9-KRYLOV-D{n_dir}", prob, "KRYLOV_SE", TSAVE_9, "adup", n_dir, "full", ref, cuda_device)


def test_padded_width_at_nine_qubits_dp5(cuda_device):
    """9 qubits, DP5_SE, 5 directions (padded to 6), B = 2, shared tables, three CF4 pieces.  The reference takes 3.9 s of CPU on
    16 cores, 7.4 s on 8."""
    prob = _problem(9, 2, 1, 5)
    ref = _reference(9, 2, 1, 5, "DP5_SE", TSAVE_DP5_SHORT, "adup")
    print(f"reference: {REFERENCE_SECONDS[(9, 2, 1, 5, 'DP5_SE', 'adup')]:.1f} s of CPU")
    _check("N9-DP5-D5", prob, "DP5_SE", TSAVE_DP5_SHORT, "adup", 5, "full", ref, cuda_device)


@pytest.mark.parametrize("n_dir", [4, 5, 6, 7])
@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_widths_at_three_qubits(solver_name, n_dir, cuda_device):
    """3 qubits, both solvers: three driven qubits (in two flip groups) against the chunk of 2 flip bits of the widths 4 .. 8 — the
    last chunk is short (the "own line again, weight 0" branch) at every width."""
    prob = _problem(3, 2, 2, 7)
    ref = _reference(3, 2, 2, 7, solver_name, TSAVE, "adup")
    _check(f"N3-{solver_name}-D{n_dir}", prob, solver_name, TSAVE, "adup", n_dir, "full", ref, cuda_device)


# ---- B. row layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["no_diag", "diag3", "ov3_shared", "ov3_traj", "pauli_only"])
@pytest.mark.parametrize("n", [3, 9])
def test_row_layouts(n, layout, cuda_device):
    """n_obs = 0 and 3, n_overlaps = 3 (shared and per-trajectory targets), Pauli rows alone: KRYLOV_SE, 3 directions, B = 2 with
    per-trajectory tables.  The states are those of the width tests' reference; only the rows differ."""
    prob = _problem(n, 2, 2, 7)
    tsave = TSAVE if n == 3 else TSAVE_9
    ref = _reference(n, 2, 2, 7, "KRYLOV_SE", tsave, "adup")
    _check(f"N{n}-{layout}", prob, "KRYLOV_SE", tsave, "adup", 3, layout, ref, cuda_device)


# ---- B. batch shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,cb,n_dir", [(1, 1, 8), (3, 3, 2)], ids=["B1-D8", "B3-cb3-D2"])
@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_batch_shapes_at_three_qubits(solver_name, batch, cb, n_dir, cuda_device):
    prob = _problem(3, batch, cb, n_dir)
    ref = _reference(3, batch, cb, n_dir, solver_name, TSAVE, "adup")
    _check(f"N3-{solver_name}-B{batch}-D{n_dir}", prob, solver_name, TSAVE, "adup", n_dir, "full", ref, cuda_device)


# ---- B. one input next to a padded direction ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "u", "p"])
def test_single_inputs_with_padding_at_nine_qubits(which, cuda_device):
    """9 qubits, 5 directions (padded to 6), only d_amp / only d_u / only d_psi0: the padded direction's zero records, zero diagonal
    rows and zeroed tangent vector are set up by different code for each.  B = 2, shared tables, two intervals."""
    prob = _problem(9, 2, 1, 5)
    ref = _reference(9, 2, 1, 5, "KRYLOV_SE", TSAVE_9, which)
    print(f"reference: {REFERENCE_SECONDS[(9, 2, 1, 5, 'KRYLOV_SE', which)]:.1f} s of CPU")
    _check(f"N9-only-{which}", prob, "KRYLOV_SE", TSAVE_9, which, 5, "full", ref, cuda_device)


# ---- B. chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 9])
def test_thirteen_directions_in_two_chunks(n, cuda_device):
    """13 directions = a chunk of 8 and a chunk of 5 (padded to 6) that reuses the first chunk's larger workspace with another
    layout and passes no expect_out: d_amp and d_psi0, diagonal + Pauli set + one overlap, B = 2, two intervals.  Every direction
    is compared; expect comes from the first chunk only."""
    prob = _problem(n, 2, 1, 13)
    ref = _reference(n, 2, 1, 13, "KRYLOV_SE", TSAVE_9, "ap")
    print(f"reference: {REFERENCE_SECONDS[(n, 2, 1, 13, 'KRYLOV_SE', 'ap')]:.1f} s of CPU")
    _check(f"N{n}-13-directions", prob, "KRYLOV_SE", TSAVE_9, "ap", 13, "full", ref, cuda_device)


# ---- C. 19 qubits: reductions beyond one grid trip -------------------------------------------------------------------------------
N_BIG, BIG_SAMPLES, BIG_DT = 19, 5, 0.004
BIG_TSAVE = (0.0, 0.0061, 0.0127)


@lru_cache(maxsize=None)
def _big_problem(solver_name, batch):
    terms = random_terms(N_BIG, BIG_SAMPLES, BIG_DT, seed=1900, local=True, phase=True)
    dev = torch.device("cuda:0")
    amp, det, u, spec = to_native(terms, dev, SolverType[solver_name], store_states=False)
    gen = torch.Generator().manual_seed(190019)
    dim = 2**N_BIG
    psi0 = _randn(gen, batch, dim, cplx=True)
    psi0 = (psi0 / psi0.norm(dim=1, keepdim=True)).to(dev)
    return terms, amp, det, u, spec, psi0


def test_reductions_at_nineteen_qubits_against_stored_states(cuda_device):
    """The tangent of psi0 alone evolves linearly, dpsi(t) = U(t) d_psi0: evolve(store_states=True) on the columns
    [psi0_b, d_psi0[d]_b] gives psi(t_k) and dpsi_d(t_k) without any tangent kernel; every row of dexpect then follows in float64
    torch — diagonals and overlaps as direct sums, the Pauli rows by polarisation
    (<psi+dpsi|O|psi+dpsi> - <psi-dpsi|O|psi-dpsi>) / 2 through the matrix-free expect_pauli.  2^19 amplitudes = 2048 blocks of 256
    against the reductions' 1024-block grids: every thread makes two trips.  B = 2, n_dir = 2, n_obs = 2, the Pauli set, two
    overlaps; 1e-10 relative to the largest entry of the direction.  Measured: 1.8e-15 and 1.7e-15 (values: 1.8e-15 absolute)."""
    dev = cuda_device
    terms, amp, det, u, spec, psi0 = _big_problem("KRYLOV_SE", 2)
    gen = torch.Generator().manual_seed(190020)
    n, dim, batch, n_dir = N_BIG, 2**N_BIG, 2, 2
    diags = torch.cat([total_magnetization_diag(n)[None], _randn(gen, 1, dim)]).to(dev)
    # tangents the rows have weight on (against a random tangent 2 Re<psi|O|dpsi> is of order 2^-9.5): sum Z psi0, the
    # single-qubit flips of psi0 and a random part, each of norm about one, with seeded complex weights
    idx = torch.arange(dim, device=dev)
    flips = lambda: sum(complex(_randn(gen, 1, cplx=True)) * psi0[:, idx ^ (1 << j)] for j in range(n)) / np.sqrt(n)  # noqa: E731
    d_psi = torch.stack([complex(_randn(gen, 1, cplx=True)) * diags[0] * psi0 / np.sqrt(n) + flips()
                         + (_randn(gen, batch, dim, cplx=True) / np.sqrt(dim)).to(dev) for _ in range(n_dir)])
    pauli = observable_set(n)
    unit = lambda t: t / t.norm(dim=0, keepdim=True)  # noqa: E731
    # targets that overlap with the tangents (a random target would give entries of 2^-9.5): one shared, one per trajectory
    targets = [unit(d_psi[0, 0] + d_psi[1, 1] + 0.1 * _randn(gen, dim, cplx=True).to(dev) / np.sqrt(dim)),
               unit((psi0 + d_psi[0] - d_psi[1]).T + 0.1 * _randn(gen, dim, batch, cplx=True).to(dev) / np.sqrt(dim))]
    tsave = torch.tensor(BIG_TSAVE, dtype=torch.float64)
    spec_t = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=False)[3]
    spec_t.pauli = pauli
    spec_t.overlaps = pack_overlaps([StateOverlap(t) for t in targets], dim, batch, dev)
    expect, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec_t, diags, d_psi0=d_psi)
    # psi and dpsi from the forward kernels alone: columns [psi0_0, psi0_1, d0_0, d0_1, d1_0, d1_1]
    spec_s = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=True)[3]
    cols = torch.cat([psi0, d_psi.reshape(n_dir * batch, dim)])
    with torch.no_grad():
        stored, _ = evolve(amp, det, u, tsave, cols, spec_s)  # (n_t, 6, dim)
    psi = stored[:, :batch].permute(0, 2, 1)  # (n_t, dim, B)
    for d in range(n_dir):
        dpsi = stored[:, batch * (1 + d):batch * (2 + d)].permute(0, 2, 1)
        want = [2.0 * (psi.conj() * o[None, :, None] * dpsi).real.sum(1) for o in diags]
        for p in pauli:  # expect_pauli sums over the batch: one column at a time
            plus, minus = psi + dpsi, psi - dpsi
            want.append(torch.stack([(expect_pauli(p, plus[:, :, b:b + 1]) - expect_pauli(p, minus[:, :, b:b + 1])).real / 2.0
                                     for b in range(batch)], dim=1))
        for t in targets:
            phi = t[:, None] if t.ndim == 1 else t
            c = (phi.conj()[None] * dpsi).sum(1)
            want += [c.real, c.imag]
        want = torch.stack(want)
        assert want.shape == dexpect[d].shape
        scale = float(want.abs().max())
        err = float((dexpect[d] - want).abs().max())
        fam = [float(want[:2].abs().max()), float(want[2:2 + len(pauli)].abs().max()), float(want[2 + len(pauli):].abs().max())]
        print(f"N19 direction {d}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative); largest per family "
              f"diagonal {fam[0]:.2e}, pauli {fam[1]:.2e}, overlap {fam[2]:.2e}")
        assert min(fam) > 1e-2
        assert bool(torch.isfinite(dexpect[d]).all())
        assert err <= NATIVE_RTOL * scale
    # the values of the tangent call against the same stored states
    val = [(psi.abs() ** 2 * o[None, :, None]).sum(1) for o in diags]
    val += [torch.stack([expect_pauli(p, psi[:, :, b:b + 1]).real for b in range(batch)], dim=1) for p in pauli]
    for t in targets:
        phi = t[:, None] if t.ndim == 1 else t
        c = (phi.conj()[None] * psi).sum(1)
        val += [c.real, c.imag]
    val = torch.stack(val)
    verr = float((expect - val).abs().max())
    print(f"N19 values: largest |expect| {float(val.abs().max()):.3e}, max error {verr:.3e}")
    assert float(val.abs().max()) > 1e-2
    assert verr <= NATIVE_RTOL * max(1.0, float(val.abs().max()))


# (n_qubits, solver, batch, coeff_batch, n_dir, which tangent inputs are given), in the style of tests/test_gpu_tangent.py
BIG_DUALITY_CASES = [(19, "KRYLOV_SE", 1, 1, 1, "adup"), (19, "DP5_SE", 1, 1, 2, "ad")]


@pytest.mark.parametrize("case", BIG_DUALITY_CASES, ids=[f"N{n}-{s}-B{b}-cb{cb}-D{d}-{w}" for n, s, b, cb, d, w in BIG_DUALITY_CASES])
def test_tangent_sweep_is_dual_to_the_native_adjoint_at_nineteen_qubits(case, cuda_device):
    """sum w * dexpect_d == Re<g_amp, d_amp> + <g_det, d_det> + <g_u, d_u> + Re<g_psi0, d_psi0> with the g_* of evolve(...).backward
    under a seeded random cotangent w (tests/test_gpu_tangent.py), at 19 qubits with 5 samples and 3 save points."""
    n, solver_name, batch, cb, n_dir, which = case
    dev = cuda_device
    terms, amp, det, u, spec, psi0 = _big_problem(solver_name, batch)
    gen = torch.Generator().manual_seed(77019 + n_dir)
    dim = 2**n
    target = _randn(gen, dim, 1, cplx=True)
    spec = to_native(terms, dev, SolverType[solver_name], store_states=False)[3]
    spec.pauli = observable_set(n)
    spec.overlaps = pack_overlaps([StateOverlap(target / target.norm())], dim, batch, dev)
    zdiag = total_magnetization_diag(n)[None].to(dev)
    tsave = torch.tensor(BIG_TSAVE, dtype=torch.float64)
    d_amp = (float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)).to(dev) if "a" in which else None
    d_det = (float(det.abs().max()) * _randn(gen, n_dir, *det.shape)).to(dev) if "d" in which else None
    d_u = (float(u.abs().max()) * _randn(gen, n_dir, *u.shape)).to(dev) if "u" in which else None
    d_psi = (_randn(gen, n_dir, batch, dim, cplx=True) / np.sqrt(dim)).to(dev) if "p" in which else None
    _, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec, zdiag, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi)
    leaves = [t.clone().requires_grad_(True) for t in (amp, det, u, psi0)]
    _, expect = evolve(leaves[0], leaves[1], leaves[2], tsave, leaves[3], spec, zdiag)
    w = _randn(gen, *expect.shape).to(dev)
    (w * expect).sum().backward()
    g_amp, g_det, g_u, g_psi = (t.grad for t in leaves)
    for d in range(n_dir):
        prod = (w * dexpect[d]).double()
        lhs, abs_sum = float(prod.sum()), float(prod.abs().sum())
        rhs = 0.0
        if d_amp is not None:
            rhs += float((g_amp.conj() * d_amp[d]).real.sum())
        if d_det is not None:
            rhs += float((g_det * d_det[d]).sum())
        if d_u is not None:
            rhs += float((g_u * d_u[d]).sum())
        if d_psi is not None:
            rhs += float((g_psi.conj() * d_psi[d]).real.sum())
        big = max(abs(lhs), abs(rhs))
        print(f"direction {d}: tangent {lhs:+.15e}  adjoint {rhs:+.15e}  rel {abs(lhs - rhs) / big:.2e}  big / sum|terms| {big / abs_sum:.2e}")
        assert big > 1e-3 * abs_sum > 0.0  # cannot pass on zeros
        assert abs(lhs - rhs) <= DUALITY_RTOL * big
