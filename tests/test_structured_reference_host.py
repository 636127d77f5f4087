"""The two matrix-free references of tests/structured_reference.py, on the CPU: (a) against the explicit matrix of the same term list
and against the oracle's matrix-free map, (b) against (a), and the SENSITIVITY of every GPU case of
tests/test_gpu_three_level_references.py: three wrong term semantics, each of which has to move what that case compares by at least 100
times the gradient bar.  The bar between references is 1e-11, two orders under the tightest GPU bar (1e-9): a reference never uses
more than 1 % of it."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import structured_reference as S
from tests.helpers import mask_of, random_terms, rel_err

REF_BAR = 1e-11
MOVE = 1e-6        # a wrong semantics moves states and gradients by at least this fraction of the largest entry ...
GRAD_FLOOR = 1e-6  # ... and every compared gradient kind of the reference is at least this large (absolute)


def _dense_value_and_grads(case):
    st = case["st"]
    leaves = {k: case[k].clone().requires_grad_(True) for k in S.GRAD_KINDS}
    states = S.dense_krylov_map(st, leaves["amp"], leaves["det"], leaves["u"], leaves["tsave"], leaves["psi0"])
    expect = (states.abs().square() * case["obs"][0][None, None, :]).sum(2)[None]
    S.case_loss(states, expect, case["w"], case["cot"]).backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    out.update(states=states.detach().numpy(), expect=expect.detach().numpy())
    return out


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("n_qubits", [4, 6, 8])
def test_matrix_free_reference_matches_the_dense_matrix_of_the_same_terms(n_qubits, extended):
    """(a) against dense_from_structured_terms + accurate_matrix_exp (not torch.linalg.matrix_exp: its degree-4 branch is off by up to
    2e-10 on small arguments): two trajectories with tables of their own, the term list of the three-level C ABI test (extended: plus
    the local terms on the last atom); states, <O> and all five gradients.  Measured at 8 qubits: 1.3e-13."""
    case = S.three_level_case(n_qubits, 2, True, extended)
    got, ref = S.reference_value_and_grads(case), _dense_value_and_grads(case)
    for name in ("states", "expect") + S.GRAD_KINDS:
        err = rel_err(got[name], ref[name])
        print(f"{n_qubits} qubits, extended={extended}: {name} {err:.2e}")
        assert err <= REF_BAR, name
    assert 5 <= min(got["taylor_terms"]) and max(got["taylor_terms"]) < 60


def test_matrix_free_reference_matches_the_oracle_on_a_plain_register():
    """No flags: (a) against R.krylov_map_matrix_free_torch at 10 qubits (a global drive with a phase and local channels), two
    trajectories on shared tables; states and all five gradients of the same loss."""
    n, ns, dt, batch = 10, 9, 0.003, 2
    terms = random_terms(n, ns, dt, seed=41, local=True)
    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    st = S.Structure(n, dt, ns, tuple(mask_of(tg) for _, tg in amp_terms), tuple(mask_of(tg) for _, tg in det_terms))
    gen = torch.Generator().manual_seed(9)
    psi0 = torch.randn(batch, 2**n, generator=gen, dtype=torch.complex128)
    psi0 = psi0 / psi0.norm(dim=1, keepdim=True)
    tsave = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)
    cot = torch.randn(len(tsave), batch, 2**n, generator=gen, dtype=torch.complex128) / 2 ** (n / 2)
    obs = torch.rand(1, 2**n, generator=gen, dtype=torch.float64)
    w = torch.linspace(0.4, 1.3, len(tsave), dtype=torch.float64)

    def loss_of(states):  # (n_t, B, dim)
        return S.case_loss(states, (states.abs().square() * obs[0]).sum(2)[None], w, cot)

    amp = torch.stack([c.to(torch.complex128) for c, _ in amp_terms]).requires_grad_(True)
    det = torch.stack([c.to(torch.float64) for c, _ in det_terms]).requires_grad_(True)
    mine = [amp, det, terms.u_pairs.clone().requires_grad_(True), tsave.clone().requires_grad_(True), psi0.clone().requires_grad_(True)]
    states = S.krylov_map(st, *mine)
    loss_of(states).backward()

    o = R.HamTerms(n, terms.u_pairs.clone().requires_grad_(True), None, None, dt, ns)
    o.extra_amp = [(c.clone().to(torch.complex128).requires_grad_(True), tg) for c, tg in amp_terms]
    o.extra_det = [(c.clone().requires_grad_(True), tg) for c, tg in det_terms]
    o_ts, o_psi = tsave.clone().requires_grad_(True), psi0.T.contiguous().clone().requires_grad_(True)
    ref = R.krylov_map_matrix_free_torch(o, o_psi, o_ts, tol=1e-19).permute(0, 2, 1)
    loss_of(ref).backward()
    assert rel_err(states.detach().numpy(), ref.detach().numpy()) <= REF_BAR
    pairs = {"amp": (amp.grad, torch.stack([c.grad for c, _ in o.extra_amp])), "det": (det.grad, torch.stack([c.grad for c, _ in o.extra_det])),
             "u": (mine[2].grad, o.u_pairs.grad), "tsave": (mine[3].grad, o_ts.grad), "psi0": (mine[4].grad, o_psi.grad.T)}
    for name, (a, b) in pairs.items():
        assert float(b.abs().max()) > GRAD_FLOOR, name
        assert rel_err(a.numpy(), b.numpy()) <= REF_BAR, name


@pytest.mark.parametrize("name", ["tl8", "tl10"])
def test_cluster_reference_matches_the_matrix_free_reference(name):
    """(b) against (a) with flags: 2 + 2 atoms at 8 qubits, 3 + 2 atoms at 10.  The product of the cluster states against the states of
    the whole register, <O>(t_k) of a cluster-sum observable, and the gradients of sum_k w_k <O>(t_k) in amp, det, tsave and the
    intra-cluster entries of u."""
    case = S.cluster_case(name)
    ref_b = S.cluster_reference(case)
    st, n_t = case["st"], len(case["tsave"])
    leaves = {k: case[k].clone().requires_grad_(True) for k in S.CLUSTER_GRAD_KINDS}
    psi0 = S.product_state(case["psi0"])[None]
    states = S.krylov_map(st, leaves["amp"], leaves["det"], leaves["u"], leaves["tsave"], psi0)
    table = S.cluster_sum_table(case["tables"])
    values = (states[:, 0].abs().square() * table[None]).sum(1)
    (values * case["w"]).sum().backward()
    prod = torch.stack([S.product_state([s[k] for s in ref_b["states"]]) for k in range(n_t)])
    assert rel_err(prod.numpy(), states[:, 0].detach().numpy()) <= REF_BAR
    assert rel_err(ref_b["expect"], values.detach().numpy()) <= REF_BAR
    for kind in S.CLUSTER_GRAD_KINDS:
        a, b = ref_b[kind], leaves[kind].grad.numpy()
        if kind == "u":
            a, b = a[case["intra"]], b[case["intra"]]
        assert float(np.abs(b).max()) > GRAD_FLOOR, kind
        assert rel_err(a, b) <= REF_BAR, kind


def _moved(got, ref) -> float:
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max())


# the mistakes the GPU cases have to see: (kind, term).  Three-level term lists (three_level_structure): amp 0 = the a qubits, amp 2 =
# the b qubits but the first (both conditioned), det 1 = the b qubits (ones-counting)
THREE_LEVEL_WRONG = (("sibling0", 0), ("ones_sign", 1), ("swap_conj", 2))
# the GPU cases against (a): (qubits, batch, per-trajectory tables).  The DP5_SE case runs on the inputs of (12, 1, False).
MATRIX_FREE_CASES = [(12, 1, False), (12, 2, True), (14, 1, False), (14, 2, False)]


@pytest.mark.parametrize("n_qubits,batch,per_trajectory", MATRIX_FREE_CASES)
def test_wrong_term_semantics_move_what_the_matrix_free_cases_compare(n_qubits, batch, per_trajectory):
    """On the exact inputs of a GPU case: the condition taken on sibling value 0, the sign of a ones-counting term flipped, c and conj c
    swapped — each for ONE term — move the states and every one of the five gradients by at least 1e-6 of the largest entry (100
    times the gradient bar), and every gradient of the reference exceeds 1e-6."""
    case = S.three_level_case(n_qubits, batch, per_trajectory)
    ref = S.reference_value_and_grads(case)
    print(f"reference (a), {n_qubits} qubits x {batch}: {ref['seconds']:.2f} s, Taylor terms {ref['taylor_terms']}")
    for kind in S.GRAD_KINDS:
        assert float(np.abs(ref[kind]).max()) > GRAD_FLOOR, kind
    for wrong in THREE_LEVEL_WRONG:
        bad = S.reference_value_and_grads(case, wrong)
        for name in ("states",) + S.GRAD_KINDS:
            moved = _moved(bad[name], ref[name])
            print(f"  {wrong}: {name} moves by {moved:.2e}")
            assert moved >= MOVE, (wrong, name)


def test_wrong_term_semantics_move_the_continuous_solution():
    """The DP5_SE case (12 qubits, the inputs of the first matrix-free case) compares stored states with the DOP853 solution of (a)'s
    right-hand side: the three mistakes move that right-hand side at t = 0 and at a time inside the tables, on the case's initial
    state, by far more than 1e-6 of its largest entry — and with it the solution (its derivative at the start)."""
    case = S.three_level_case(12, 1, False)
    st = case["st"]
    for t in (0.0, 0.0095):
        ref = S.rhs(st, case["amp"][0], case["det"][0], case["u"], t, case["psi0"])
        for wrong in THREE_LEVEL_WRONG:
            bad = S.rhs(st, case["amp"][0], case["det"][0], case["u"], t, case["psi0"], S.Operator(st, "cpu", wrong))
            assert _moved(bad.numpy(), ref.numpy()) >= MOVE, (t, wrong)


def test_continuous_solution_matches_the_oracle_on_a_plain_register():
    """rhs / continuous_solution without flags against R.continuous_solution (the oracle's DOP853 run) at 6 qubits.  Both runs control
    their local error to rtol 1e-12 over some ten steps and choose the steps from their own rounding, so they agree to about 1e-11, not
    to the last bit (measured 3.2e-12): the bar between references, 20 times under the tightest DP5_SE bar (2e-10)."""
    n, ns, dt = 6, 9, 0.003
    terms = random_terms(n, ns, dt, seed=43, local=True)
    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    st = S.Structure(n, dt, ns, tuple(mask_of(tg) for _, tg in amp_terms), tuple(mask_of(tg) for _, tg in det_terms))
    psi0 = torch.randn(1, 2**n, generator=torch.Generator().manual_seed(3), dtype=torch.complex128)
    psi0 = psi0 / psi0.norm()
    tsave = torch.tensor([0.0, 0.0041, 0.0102, 0.0163, 0.024], dtype=torch.float64)
    got = S.continuous_solution(st, torch.stack([c.to(torch.complex128) for c, _ in amp_terms]),
                                torch.stack([c.to(torch.float64) for c, _ in det_terms]), terms.u_pairs, tsave, psi0)
    ref = R.continuous_solution(terms, psi0.T.numpy(), tsave.numpy())  # (n_t, dim, 1)
    assert np.abs(got[:, 0] - ref[:, :, 0]).max() <= REF_BAR


# the GPU cases against (b); three-level term lists (cluster_case): amp 0 = the a qubits, amp 1 = the b qubits, det 1 = the b qubits
# (ones-counting), each present in EVERY cluster.  The plain registers have no conditioned and no ones-counting term: there only the
# swap of c and conj c applies, on the global drive.
CLUSTER_WRONG = {True: (("sibling0", 0), ("ones_sign", 1), ("swap_conj", 1)), False: (("swap_conj", 0),)}


@pytest.mark.parametrize("name", ["tl20", "tl22", "tl24", "plain22", "plain25"])
def test_wrong_term_semantics_move_what_the_cluster_cases_compare(name):
    """The cluster cases, on their per-cluster states: (b) agrees with (a) run per cluster, each mistake moves the states of EVERY
    cluster and each compared gradient kind (amp, det, tsave, intra-cluster u) by at least 1e-6 of the largest entry, and every
    gradient kind of the reference exceeds 1e-6."""
    case = S.cluster_case(name)
    ref = S.cluster_reference(case)
    same = S.cluster_reference(case, "matrix_free")
    intra = case["intra"]
    pick = lambda r, kind: r[kind][intra] if kind == "u" else r[kind]  # noqa: E731
    for c, (a, b) in enumerate(zip(same["states"], ref["states"])):
        assert rel_err(a.numpy(), b.numpy()) <= REF_BAR, c
    for kind in S.CLUSTER_GRAD_KINDS:
        assert float(np.abs(pick(ref, kind)).max()) > GRAD_FLOOR, kind
        assert rel_err(pick(same, kind), pick(ref, kind)) <= REF_BAR, kind
    for wrong in CLUSTER_WRONG[CLUSTER_IS_THREE_LEVEL[name]]:
        bad = S.cluster_reference(case, "matrix_free", wrong)
        for c, (a, b) in enumerate(zip(bad["states"], ref["states"])):
            assert _moved(a.numpy(), b.numpy()) >= MOVE, (wrong, "cluster", c)
        for kind in S.CLUSTER_GRAD_KINDS:
            assert _moved(pick(bad, kind), pick(ref, kind)) >= MOVE, (wrong, kind)


CLUSTER_IS_THREE_LEVEL = {k: v[1] for k, v in S.CLUSTER_CASES.items()}
