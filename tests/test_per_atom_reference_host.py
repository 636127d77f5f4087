"""Per-atom addressing (one single-qubit amplitude term and one single-qubit detuning term per atom), CPU side: the builder, the two
references that tests/test_gpu_per_atom_terms.py pins the kernels to, and the per-row check itself.

1. tests.helpers.per_atom_terms through R.dense_hamiltonian equals tests.helpers.dense_from_structured_terms (the C ABI's term
   semantics) of the same term list at 5 qubits, entry by entry.
2. The two references — autograd through R.krylov_map_dense and through R.krylov_map_matrix_free_torch — agree per row at 10 qubits.
   Their worst per-row disagreement is the noise floor of the reference; it is printed, and profiles/per_atom_parity.txt records it.
   The bars of the GPU file (1e-8 per row for gradients, 1e-9 for states and <O>) must stay at least 10 times above it.
3. assert_rows_close fails where two rows of a correct gradient are swapped, and where one small row is zeroed while the project's
   max-norm check (rel_err) still passes — the hole the per-row check closes.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import (PER_ATOM_TSAVE, ROW_FLOOR, assert_rows_close, dense_from_structured_terms, mask_of, oracle_value_and_grads,
                           per_atom_problem, per_atom_terms, per_atom_terms_batch, product_state, rel_err, row_errors, stack_tables)

N_SAMPLES, DT = 9, 0.003
ORACLE_GRAD_RTOL, ORACLE_STATE_RTOL = 1e-8, 1e-9  # the GPU file's bars against the oracle


@pytest.mark.parametrize("kw", [dict(), dict(phase=False), dict(undriven=(1,), undetuned=(3,)), dict(global_drive=True, undetuned=(0,))],
                         ids=["all", "phase_free", "holes", "global_drive"])
def test_builder_through_the_oracle_equals_the_structured_term_semantics(kw):
    n = 5
    terms = per_atom_terms(n, N_SAMPLES, DT, seed=505, **kw)
    assert terms.amp_coeff is None and terms.det_coeff is None
    driven = [tg for _, tg in terms.extra_amp]
    if kw.get("global_drive"):
        assert driven == [list(range(n))]
    else:
        assert driven == [[q] for q in range(n) if q not in kw.get("undriven", ())]
    assert [tg for _, tg in terms.extra_det] == [[q] for q in range(n) if q not in kw.get("undetuned", ())]
    if not kw.get("phase", True):
        assert all(float(c.imag.abs().max()) == 0.0 for c, _ in terms.extra_amp)
    for t in (0.0, 0.0041, 0.0163, 0.024):
        # (0-d float64 / complex128 tensors: a Python float times the helper's integer bit tables would round to float32)
        amp = [(R.interp_coeff(c, t, DT, N_SAMPLES), mask_of(tg)) for c, tg in terms.amp_terms()]
        det = [(R.interp_coeff(c, t, DT, N_SAMPLES), mask_of(tg)) for c, tg in terms.det_terms()]
        want = dense_from_structured_terms(n, terms.u_pairs, amp, det)
        got = R.dense_hamiltonian(terms, t)
        assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
        assert float((got - got.conj().T).abs().max()) == 0.0


def test_no_two_rows_of_the_builder_are_proportional():
    """Swapping two groups must change the problem: the normalised rows differ by more than 1e-2 pairwise."""
    terms = per_atom_terms(13, N_SAMPLES, DT, seed=1313)
    for rows in (torch.stack([c for c, _ in terms.extra_amp]), torch.stack([c for c, _ in terms.extra_det]).to(torch.complex128)):
        unit = rows / rows.norm(dim=1, keepdim=True)
        gram = (unit.conj() @ unit.T).abs() - torch.eye(len(rows), dtype=torch.float64)
        assert float(gram.max()) < 1.0 - 1e-4


def test_product_state_and_table_stacking():
    gen = torch.Generator().manual_seed(3)
    psi = product_state(4, gen)
    assert psi.shape == (16,) and abs(float(psi.norm()) - 1.0) < 1e-14
    m = psi.reshape(2, 8)  # a product state has Schmidt rank one across every cut
    assert float(torch.linalg.svdvals(m)[1]) < 1e-15
    sets = per_atom_terms_batch(4, N_SAMPLES, DT, seeds=(1, 2, 3), undriven=(1,))
    amp, det = stack_tables(sets)
    assert amp.shape == (3, 3, N_SAMPLES) and det.shape == (3, 4, N_SAMPLES)
    assert all(torch.equal(s.u_pairs, sets[0].u_pairs) for s in sets)
    assert float((amp[0] - amp[1]).abs().min(dim=1).values.max()) > 0 and torch.equal(amp[2, 1], sets[2].extra_amp[1][0])
    with pytest.raises(AssertionError):
        stack_tables([sets[0], per_atom_terms(4, N_SAMPLES, DT, seed=1)])


@lru_cache(maxsize=None)
def _two_references():
    n = 10
    terms = per_atom_terms(n, N_SAMPLES, DT, seed=1010, undriven=(1,), undetuned=(n - 2,))
    psi0, obs, w, cot = per_atom_problem(n, 1, seed=1011)
    return tuple(oracle_value_and_grads(terms, psi0, PER_ATOM_TSAVE, obs, w, cot, method=m) for m in ("dense", "matrix_free"))


def test_the_two_references_agree_per_row_at_ten_qubits():
    dense, mf = _two_references()
    floor = {}
    for key in ("amp", "det"):
        err, ratio = row_errors(mf[key], dense[key])
        assert float(ratio.min()) >= ROW_FLOOR
        floor[key] = float(err.max())
    for key in ("states", "expect", "u", "tsave", "psi0"):
        floor[key] = rel_err(mf[key], dense[key])
    print("reference against reference at 10 qubits (matrix-free Taylor against dense matrix_exp): "
          + ", ".join(f"{k} {v:.2e}" for k, v in floor.items()))
    for key, v in floor.items():  # the bars must stay 10 times above the floor
        assert v <= 0.1 * (ORACLE_STATE_RTOL if key in ("states", "expect") else ORACLE_GRAD_RTOL), (key, v)


def test_per_row_check_fails_on_swapped_rows():
    dense, _ = _two_references()
    for key in ("amp", "det"):
        ref = dense[key]
        assert_rows_close(ref.copy(), ref, 1e-8, key)
        _, ratio = row_errors(ref, ref)
        order = np.argsort(ratio)
        for a, b in ((order[0], order[1]), (order[0], order[-1]), (0, 1)):
            bad = ref.copy()
            bad[[a, b]] = bad[[b, a]]
            with pytest.raises(AssertionError):
                assert_rows_close(bad, ref, 1e-8, key)


def test_per_row_check_fails_on_a_zeroed_small_row_that_the_max_norm_lets_through():
    """The hole: one group row with a small gradient lost (or never accumulated) passes a max-norm bar relative to the whole tensor."""
    ref = np.zeros((4, 6))
    ref[0] = [3.0, -2.0, 1.0, 0.5, 2.5, -1.0]
    ref[1] = [1.0, 0.2, -0.7, 0.3, 0.9, 0.1]
    ref[2] = 0.5 * ref[0][::-1]
    ref[3] = 0.02 * np.array([1.0, -1.0, 0.5, 0.3, -0.2, 0.9])  # 6.7e-3 of the largest row: small, and below the 1e-2 floor
    bad = ref.copy()
    bad[3] = 0.0
    assert rel_err(bad, ref) < 1e-2  # the max-norm check at a bar of 1e-2 passes
    with pytest.raises(AssertionError, match="of the largest row"):  # ... and the reference-side guard refuses such a row outright
        assert_rows_close(ref.copy(), ref, 1e-2, "small")
    ref[3] *= 2.0  # 1.3e-2 of the largest row: legal
    bad = ref.copy()
    bad[3] = 0.0
    assert rel_err(bad, ref) < 2e-2
    with pytest.raises(AssertionError, match="off by"):
        assert_rows_close(bad, ref, 2e-2, "small")
    # the real gradients: the smallest row of the 10-qubit reference zeroed, at a bar the max-norm check passes
    dense, _ = _two_references()
    for key in ("amp", "det"):
        g = dense[key]
        _, ratio = row_errors(g, g)
        r = int(np.argmin(ratio))
        bad = g.copy()
        bad[r] = 0.0
        assert float(ratio[r]) < 0.9
        bar = 0.5 * (float(ratio[r]) + 1.0)  # between the max-norm error of the zeroed row (its share of the largest row) and its per-row error (1)
        assert rel_err(bad, g) < bar
        with pytest.raises(AssertionError, match="off by"):
            assert_rows_close(bad, g, bar, key)
