"""Three-level registers (conditioned flips, ones-counting detunings) past the dense limit, and the tile layouts at full size, against
references that share nothing with the library (tests/structured_reference.py; their own parity, and what each case below is
sensitive to, is in tests/test_structured_reference_host.py):

  (a) the matrix-free map with torch autograd — 12 qubits (persistent forward + direct adjoint, and the direct kernels) and 14 qubits
      (a multi-workgroup direct grid, and every chained 2^12-tile variant and tape mode): states, <O>(t_k) and all five gradients;
      DP5_SE at 12 qubits against the DOP853 solution of the same right-hand side;
  (b) the cluster-separable product state, exact at any size — 20 / 22 / 24 qubits of three-level atoms and 22 / 25 qubits of a plain
      register: the states on the device, <O>(t_k) of a cluster-sum and of a hashed table, the gradients in amp, det, tsave and the
      intra-cluster U.

Bars: 1e-9 for states and <O>, 1e-8 for gradients (those of tests/test_gpu_three_level.py); DP5_SE 1e-8 at the default tolerance and
2e-10 at tol = 1e-12 (those of tests/test_gpu_dp5.py).  The references are computed once per problem and shared by the variants.
Measured figures: profiles/three_level_parity.txt."""
import numpy as np
import pytest
import torch

from tests import structured_reference as S
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

VALUE_BAR, GRAD_BAR = 1e-9, 1e-8
TAPE_STAT = {"full": "full", "steps": "none", "partial": "partial"}  # stored states serve as the one-state-per-save-point tape
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def matrix_free_reference(n_qubits, batch, per_trajectory):
    """(case, reference (a)) of one three-level problem: computed once, shared by every variant, never modified."""
    def make():
        case = S.three_level_case(n_qubits, batch, per_trajectory)
        ref = S.reference_value_and_grads(case)
        print(f"[reference a] {n_qubits} qubits x {batch}{' per-trajectory tables' if per_trajectory else ''}: {ref['seconds']:.2f} s CPU, "
              f"Taylor terms {ref['taylor_terms']}")
        return case, ref
    return _cached(("a", n_qubits, batch, per_trajectory), make)


def _spec(st, solver, variant, **kw):
    from pulser_diff_amd.solver import ProblemSpec

    return ProblemSpec(st.n_qubits, st.dt, st.n_samples, st.amp_masks, st.det_masks, solver=solver, amp_conditioned=st.amp_conditioned,
                       det_ones=st.det_ones, kernel_variant=variant, **kw)


def _krylov_cases():
    cases = []
    for batch, per_trajectory in ((1, False), (2, True)):
        cases += [(12, batch, per_trajectory, 0, "auto", "persistent"), (12, batch, per_trajectory, 1, "auto", "direct")]
    for batch in (1, 2):
        cases.append((14, batch, False, 1, "auto", "direct"))
        cases += [(14, batch, False, v, tape, "chained-tiles") for v in (2, 3, 4) for tape in ("full", "steps", "partial")]
        # 10: the chained tiles with trajectory-per-XCD placement forced; 12: automatic with plain tile order — and the automatic
        # choice for 2^14 or 2^15 amplitudes in flight is the direct family
        cases += [(14, batch, False, 10, "auto", "chained-tiles"), (14, batch, False, 12, "auto", "direct")]
    return cases


@pytest.mark.parametrize("n_qubits,batch,per_trajectory,variant,tape,family", _krylov_cases())
def test_three_level_terms_match_the_matrix_free_reference(cuda_device, n_qubits, batch, per_trajectory, variant, tape, family):
    """The term list of test_conditioned_flips_and_ones_counting_terms_through_the_c_abi plus a conditioned flip and a ones-counting
    detuning on the LAST atom (the lowest index bits), a random state inside the valid codes, loss = weighted <O>(t_k) plus a state
    cotangent at every save point: stored states, <O>(t_k) and the amp, det, u, tsave and psi0 gradients against reference (a).
    12 qubits (6 atoms, the state-preparation notebook's size): the one-workgroup forward sweep with the direct adjoint (0) and the direct
    kernels (1), one trajectory and two with tables of their own.  14 qubits, the smallest even size with chained passes and a
    multi-workgroup direct grid: the direct kernels every other three-level test leans on, the 512 / 256 / 1024-thread chained tiles
    with each tape mode, forced XCD placement, plain tile order; one trajectory and two on shared tables."""
    from pulser_diff_amd.solver import SolverType, evolve

    case, ref = matrix_free_reference(n_qubits, batch, per_trajectory)
    st = case["st"]
    spec = _spec(st, SolverType.KRYLOV_SE, variant, store_states=True, tape=tape, tape_steps=2 if tape == "partial" else None)
    leaves = [case[k].to(cuda_device).requires_grad_(True) for k in ("amp", "det", "u")] + [case["tsave"].clone().requires_grad_(True),
                                                                                           case["psi0"].to(cuda_device).requires_grad_(True)]
    states, expect = evolve(*leaves, spec, case["obs"].to(cuda_device))
    S.case_loss(states, expect, case["w"].to(cuda_device), case["cot"].to(cuda_device)).backward()
    stats = dict(spec.options["_last_stats"])
    assert stats["kernel_family"] == family, stats
    if tape != "auto":
        assert stats["tape"] == TAPE_STAT[tape], stats
    if family == "chained-tiles":
        assert stats["kernel_fwd"].startswith("k_chain<12,") and stats["kernel_bwd"].startswith("k_chain<12,"), stats
    invalid = torch.ones(2**n_qubits, dtype=torch.bool)
    invalid[S.valid_codes(n_qubits)] = False
    assert float(states.detach()[..., invalid.to(cuda_device)].abs().max()) == 0.0  # the unused code 00 of every atom stays empty
    errs = {"states": rel_err(states.detach().cpu().numpy(), ref["states"]), "expect": rel_err(expect.detach().cpu().numpy(), ref["expect"])}
    for name, leaf in zip(S.GRAD_KINDS, leaves):
        errs[name] = rel_err(leaf.grad.detach().cpu().numpy(), ref[name])
    print(f"[parity a] {n_qubits}x{batch} variant {variant} tape {tape} {stats['kernel_fwd']} / {stats['kernel_bwd']}: "
          + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for name, err in errs.items():
        assert err < (VALUE_BAR if name in ("states", "expect") else GRAD_BAR), (name, err)


@pytest.mark.parametrize("variant,family", [(0, "persistent"), (1, "direct")])
def test_three_level_terms_on_the_continuous_solver_match_dop853(cuda_device, variant, family):
    """DP5_SE with conditioned flips and ones-counting detunings at 12 qubits (checked at 6 so far): every stored state against the
    DOP853 solution of reference (a)'s right-hand side -i H(t) psi, at the default tolerance (1e-8) and at tol = 1e-12 (2e-10)."""
    from pulser_diff_amd.solver import SolverType, evolve

    def make():
        import time

        case = S.three_level_case(12, 1, False)
        t0 = time.perf_counter()
        cont = S.continuous_solution(case["st"], case["amp"][0], case["det"][0], case["u"], case["tsave"], case["psi0"])
        print(f"[reference a] DOP853, 12 qubits: {time.perf_counter() - t0:.2f} s CPU")
        return case, cont
    case, cont = _cached(("dop853", 12), make)
    args = [case[k].to(cuda_device) for k in ("amp", "det", "u")] + [case["tsave"], case["psi0"].to(cuda_device)]
    for tol, bar in ((0.0, 1e-8), (1e-12, 2e-10)):
        spec = _spec(case["st"], SolverType.DP5_SE, variant, store_states=True, tol=tol)
        with torch.no_grad():
            states, _ = evolve(*args, spec, None)
        assert dict(spec.options["_last_stats"])["kernel_family"] == family
        err = float(np.abs(states.cpu().numpy() - cont).max())
        print(f"[parity a] DP5_SE 12 qubits variant {variant} tol {tol:g}: states {err:.1e} (absolute; bar {bar:g})")
        assert err < bar, (tol, err)


def _hashed_table(n_qubits, device):
    x = torch.arange(2**n_qubits, device=device)
    return ((x * 2654435761) % 1000003).to(torch.float64) / 1000003.0


# (case, kernel variant, tape, family, what the forward and the adjoint kernel names start with)
CLUSTER_RUNS = [("tl20", 0, "auto", "chained-tiles", "k_chain<12,"), ("tl20", 1, "auto", "direct", "k_factor"),
                ("tl22", 4, "steps", "chained-tiles", "k_chain<12,10,"), ("tl24", 2, "steps", "chained-tiles", "k_chain<12,9,"),
                ("plain22", 0, "steps", "chained-tiles", "k_chain_wide<13,"), ("plain25", 0, "steps", "chained-tiles", "k_chain<12,")]


@pytest.mark.parametrize("name,variant,tape,family,kernel", CLUSTER_RUNS, ids=[f"{r[0]}-{r[1]}-{r[3]}" for r in CLUSTER_RUNS])
def test_tile_layouts_at_full_size_match_the_cluster_separable_reference(cuda_device, name, variant, tape, family, kernel):
    """KRYLOV_SE on a register cut into clusters of at most 6 consecutive qubits of unequal sizes with different local terms, U only
    inside clusters (a distinct value per pair), psi0 the product of random cluster states: H = sum_c H_c (x) 1, so the exact state is
    the product of cluster states evolved with 64 x 64 matrices at most (reference (b)).  Three-level atoms at 20 qubits (the automatic
    chained passes, and the direct kernels), 22 (1024-thread tiles) and 24 (512-thread tiles, three layouts); plain registers with a
    global drive with a phase and local channels on the first, a middle and the last qubit at 22 (automatic: wide tiles, two layouts)
    and 25 qubits (automatic: 2^12 tiles, three layouts).  Compared: every stored state on the device against the product state;
    <O>(t_k) for a cluster-sum table (against sum_c <o_c>_c, nothing of size 2^N) and for a hashed generic table (against the product
    state on the device); the gradients of sum_k w_k <O_clustersum>(t_k) in amp, det, tsave and the intra-cluster entries of U.
    NOT compared here: the U gradient between clusters (U is zero there, its gradient is not) and the psi0 gradient — they stay with
    the A/B test against the direct kernels (tests/test_gpu_three_level.py, tests/test_gpu_solver_parity.py)."""
    from pulser_diff_amd.solver import SolverType, evolve

    def make():
        case = S.cluster_case(name)
        ref = S.cluster_reference(case)
        print(f"[reference b] {name}: clusters {case['sizes']}, {ref['seconds'] * 1e3:.0f} ms CPU")
        return case, ref
    case, ref = _cached(("b", name), make)
    st, n_t = case["st"], len(case["tsave"])
    n = st.n_qubits
    obs = torch.stack([S.cluster_sum_table(case["tables"], cuda_device), _hashed_table(n, cuda_device)])
    psi0 = S.product_state(case["psi0"], cuda_device)[None]
    leaves = {k: (case[k][None] if k in ("amp", "det") else case[k]).clone().to(cuda_device if k != "tsave" else "cpu").requires_grad_(True)
              for k in S.CLUSTER_GRAD_KINDS}  # (clones: the cached case is shared by the variants and stays as it is)
    spec = _spec(st, SolverType.KRYLOV_SE, variant, store_states=True, tape=tape)
    states, expect = evolve(leaves["amp"], leaves["det"], leaves["u"], leaves["tsave"], psi0, spec, obs)
    (expect[0, :, 0] * case["w"].to(cuda_device)).sum().backward()
    stats = dict(spec.options["_last_stats"])
    assert stats["kernel_family"] == family and stats["kernel_fwd"].startswith(kernel) and stats["kernel_bwd"].startswith(kernel), stats
    errs = {"states": 0.0, "hashed": 0.0}
    with torch.no_grad():
        for k in range(n_t):
            prod = S.product_state([s[k] for s in ref["states"]], cuda_device)
            errs["states"] = max(errs["states"], float((states[k, 0] - prod).abs().max() / prod.abs().max()))
            hashed = float((prod.abs().square() * obs[1]).sum())
            errs["hashed"] = max(errs["hashed"], abs(float(expect[1, k, 0]) - hashed) / abs(hashed))
            del prod
    errs["clustersum"] = rel_err(expect[0, :, 0].detach().cpu().numpy(), ref["expect"])
    for kind in S.CLUSTER_GRAD_KINDS:
        got = leaves[kind].grad.detach().cpu().numpy()
        got = got[0] if kind in ("amp", "det") else got
        errs[kind] = rel_err(got[case["intra"]], ref[kind][case["intra"]]) if kind == "u" else rel_err(got, ref[kind])
    print(f"[parity b] {name} variant {variant} {stats['kernel_fwd']} / {stats['kernel_bwd']}: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    del states, expect, obs, psi0, leaves
    torch.cuda.empty_cache()
    for kind, err in errs.items():
        assert err < (GRAD_BAR if kind in S.CLUSTER_GRAD_KINDS else VALUE_BAR), (kind, err)
