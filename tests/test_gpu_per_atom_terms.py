"""Per-atom addressing past 12 qubits: ONE single-qubit amplitude term and ONE single-qubit detuning term per atom (what noisy runs, SLM
masks and local channels hand over), so that every kernel's loop over coefficient groups runs with up to one group per qubit.

Parts (tests.helpers.per_atom_terms builds the tables: no two rows proportional; product initial states; the loss per_atom_loss
weights <O_0> at every save point, <O_1> at one, and the states at every save point after the first; every case checks the states at every save point, <O>(t_k) of
two diagonal observables and all five gradient kinds, the amplitude and detuning gradients ROW BY ROW — tests.helpers.assert_rows_close):

a. 13 and 14 qubits against autograd through R.krylov_map_matrix_free_torch (computed once per table set): direct kernels (variant 1),
   chained 2^12 tiles at 512 / 256 / 1024 threads (2 / 3 / 4), 2^11 and 2^10 tiles (15 / 16), wide tiles (14, at 14 qubits), the
   automatic choice (0) and blocks of two (17, which a per-atom problem must not take); complex tables (signed-sum adjoint) and
   phase-free tables handed over as real tensors (real_amp_grad adjoint); tapes full / steps / partial.  A per-atom problem must run the
   group-looped chained instantiation (FAST = false), ONE global drive with per-atom detunings the loop-free one (FAST = true).
b. 8 and 10 qubits against autograd through R.krylov_map_dense, and through magnus_cf4_dense for DP5_SE: the generic direct kernels
   (variant 1) and the persistent per-bit sweep (variant 0).
c. Per-trajectory tables at 13 qubits: 3 trajectories against the oracle run per trajectory; 9 trajectories, trajectory-per-XCD
   placement (variant 10) against variants 2 and 1; 16 trajectories on the automatic route against variant 1.
d. Larger registers against variant 1 (pinned by a and b): 16 (automatic, wide), 20 (automatic), 21 (variant 7: three layouts),
   22 qubits (automatic: wide tiles, 22 + 22 groups); DP5_SE at 13 qubits, variant 2.
e. The tangent sweep: 9 qubits with 9 + 9 groups against tangent_dense_reference entry by entry, 13 qubits dual to the native adjoint
   with directions that are one-hot in single atoms' tables.
f. State sharding with the rank qubits in groups of their own, one of them undriven and another undetuned (and, with two rank qubits,
   also both driven): run_virtual_native / grad_virtual_native against the single-GPU solver, run_virtual against the dense oracle.

Bars, the project's own: against the oracle 1e-9 for states and <O>, 1e-8 for gradients; native against variant 1 1e-11 for states,
1e-10 for <O>, 1e-9 for gradients.  Per row: max|got_r - ref_r| <= bar * max(max|ref_r|, 1e-2 max|ref|), and every reference row must
reach 1e-2 of the largest.  The measured figures are in profiles/per_atom_parity.txt.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import (PER_ATOM_TSAVE, assert_rows_close, mask_of, oracle_value_and_grads, per_atom_loss,
                           per_atom_problem, per_atom_terms, per_atom_terms_batch, product_state, rel_err, row_errors, stack_tables,
                           tangent_dense_reference, tangent_rows_reference, to_native)

pytestmark = pytest.mark.gpu

N_SAMPLES, DT = 9, 0.003
ORACLE_BARS = {"states": 1e-9, "expect": 1e-9, "grad": 1e-8}
AB_BARS = {"states": 1e-11, "expect": 1e-10, "grad": 1e-9}
# one seed per register size (the reference-side guard of assert_rows_close — every row at least 1e-2 of the largest — holds for these)
SEEDS = {8: 818, 9: 909, 10: 1010, 13: 1313, 14: 1414, 16: 1616, 20: 2020, 21: 2121, 22: 2222}
TSAVE_SHORT = (0.0, 0.0041)            # DP5_SE at 10 qubits: the dense Magnus reference costs 2 matrix exponentials per piece
TSAVE_THREE = (0.0, 0.0102, 0.024)     # 22 qubits, the tangent reference


def _holes(n):
    return dict(undriven=(1,), undetuned=(n - 2,))


@lru_cache(maxsize=None)
def _terms(n, real=False, global_drive=False):
    return per_atom_terms(n, N_SAMPLES, DT, SEEDS[n], phase=not real, global_drive=global_drive, **_holes(n))


@lru_cache(maxsize=None)
def _inputs(n, batch=1, n_t=len(PER_ATOM_TSAVE)):
    return per_atom_problem(n, batch, SEEDS[n] + 1, n_t)


@lru_cache(maxsize=None)
def _oracle(n, real, global_drive, method="matrix_free", tsave=PER_ATOM_TSAVE):
    """The CPU reference of one table set: computed once, shared by the cases, never modified (numpy arrays of a cached dict)."""
    psi0, obs, w, cot = _inputs(n, 1, len(tsave))
    return oracle_value_and_grads(_terms(n, real, global_drive), psi0, tsave, obs, w, cot, method=method)


def _run(terms, inputs, device, variant, tape="auto", real=False, solver="KRYLOV_SE", tsave=PER_ATOM_TSAVE):
    """evolve + backward of per_atom_loss on one kernel variant.  terms: one HamTerms or a list of B (per-trajectory tables).  Returns
    the detached device tensors states (n_t, B, dim), expect, the five gradients and the plan statistics."""
    from pulser_diff_amd.solver import SolverType, evolve

    sets = list(terms) if isinstance(terms, (list, tuple)) else [terms]
    amp, det = stack_tables(sets, device, real_amp=real)
    _, _, u, spec = to_native(sets[0], device, SolverType[solver])
    spec.kernel_variant, spec.tape = variant, tape
    if tape == "partial":
        spec.tape_steps = 2
    psi0, obs, w, cot = (t.to(device) for t in inputs)
    leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True),
              torch.tensor(tsave, dtype=torch.float64).requires_grad_(True), psi0.clone().requires_grad_(True)]
    states, expect = evolve(*leaves, spec, obs)
    per_atom_loss(states, expect, w, cot).backward()
    torch.cuda.synchronize()
    out = {"states": states.detach(), "expect": expect.detach(), "stats": dict(spec.options["_last_stats"])}
    out.update({k: l.grad.detach() for k, l in zip(("amp", "det", "u", "tsave", "psi0"), leaves)})
    return out


def _on(device, x):
    return (x if isinstance(x, torch.Tensor) else torch.as_tensor(x)).to(device)


def _check(label, got, ref, bars, real=False):
    """Every figure first (printed: the measurement tables of profiles/per_atom_parity.txt come from these lines), then the bars."""
    dev = got["states"].device
    fig = {}
    for key in ("states", "u", "tsave", "psi0"):
        a, b = got[key].to(dev), _on(dev, ref[key]).reshape(got[key].shape)
        fig[key] = float((a - b).abs().max() / b.abs().max())
    fig["expect"] = float((got["expect"] - _on(dev, ref["expect"])).abs().max())
    rows = {}
    for key in ("amp", "det"):
        a = got[key].cpu().numpy()
        b = _on("cpu", ref[key]).numpy().reshape((-1,) + a.shape[-2:])
        b = b.real if (key == "amp" and real and np.iscomplexobj(b)) else b
        rows[key] = (a, b.reshape(a.shape))
        err, ratio = row_errors(*rows[key])
        fig[key + "_rows"], fig[key + "_smallest_row"] = float(err.max()), float(ratio.min())
    st = got["stats"]
    print(f"PER_ATOM {label}: family={st['kernel_family']} fwd={st.get('kernel_fwd')} bwd={st.get('kernel_bwd')} tape={st.get('tape')} | "
          + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fig["states"] <= bars["states"], (label, "states", fig["states"])
    assert fig["expect"] <= bars["expect"], (label, "expect", fig["expect"])
    for key in ("amp", "det"):
        assert_rows_close(*rows[key], bars["grad"], f"{label} {key}")
    for key in ("u", "tsave", "psi0"):
        assert fig[key] <= bars["grad"], (label, key, fig[key])
    return fig


def _instantiation(name):
    """'k_chain<12,9,true,false,false,false>' -> ('k_chain', ['12', '9', 'true', 'false', 'false', 'false'])."""
    base, _, args = name.partition("<")
    return base, args.rstrip(">").split(",") if args else []


def _assert_chained(st, fast, real, lt=None, lgt=None, wide=False):
    """The chained-tile instantiations of both sweeps (rocprofv3 spelling: k_chain<LT, LGT, CPLX, BWD, FAST, RES>,
    k_chain_wide<LT, CPLX, BWD, FAST>): tile size, threads, the group loop (FAST = false) or the loop-free form, and for the adjoint
    the signed-sum (CPLX) or the real_amp_grad form."""
    assert st["kernel_family"] == "chained-tiles", st
    for key, bwd in (("kernel_fwd", False), ("kernel_bwd", True)):
        base, a = _instantiation(st[key])
        if wide:
            assert base == "k_chain_wide" and a[0] == "13", st
            cplx, is_bwd, is_fast = a[1:4]
        else:
            assert base == "k_chain" and (lt is None or a[0] == str(lt)) and (lgt is None or a[1] == str(lgt)), st
            cplx, is_bwd, is_fast = a[2:5]
        assert is_bwd == ("true" if bwd else "false"), st
        assert is_fast == ("true" if fast else "false"), st
        if bwd:
            assert cplx == ("false" if real else "true"), st


# variant -> (tile bits, log2 threads) of the 2^12 / 2^11 / 2^10 tiles; 14: wide tiles
TILES = {2: (12, 9), 3: (12, 8), 4: (12, 10), 15: (11, 10), 16: (10, 10)}
TAPE_STAT = {"full": "full", "steps": "none", "partial": "partial"}  # stored states serve as the one-state-per-save-point tape


def _assert_kernels(st, variant, fast, real, n):
    if variant == 1:
        assert st["kernel_family"] == "direct", st
        # the generic direct kernels loop over the groups; one global drive takes the unrolled ones
        assert st["kernel_fwd"].startswith("k_factor_direct_global<" if fast else "k_factor_direct") and (fast or "global" not in st["kernel_fwd"]), st
        assert st["kernel_bwd"].startswith("k_factor_bwd_direct_global<" if fast else "k_factor_bwd_direct") and (fast or "global" not in st["kernel_bwd"]), st
    elif variant in TILES:
        _assert_chained(st, fast, real, *TILES[variant])
    elif variant == 14:
        _assert_chained(st, fast, real, wide=True)
    elif variant == 17:  # blocks of two need ONE global drive: a per-atom problem stays on the one-factor passes
        assert "k_chain2" not in st["kernel_fwd"] and "k_chain2" not in st["kernel_bwd"], st
        _assert_chained(st, fast, real, lt=12)
    else:  # automatic
        assert st["kernel_family"] in ("direct", "chained-tiles"), st
        if st["kernel_family"] == "chained-tiles" and "k_chain2" not in st["kernel_fwd"]:
            _assert_chained(st, fast, real, wide="wide" in st["kernel_fwd"])


# ---- a. 13 and 14 qubits against the matrix-free oracle ----------------------------------------------------------------------------------
PARITY_CASES = [
    # (qubits, variant, real tables, tape): every variant with a complex and a real case, the tapes spread over them
    (13, 1, False, "full"), (13, 1, True, "steps"), (13, 2, False, "steps"), (13, 2, True, "full"), (13, 3, False, "partial"),
    (13, 3, True, "steps"), (13, 4, False, "full"), (13, 4, True, "partial"), (13, 15, False, "steps"), (13, 15, True, "full"),
    (13, 16, False, "full"), (13, 16, True, "steps"), (13, 0, False, "full"), (13, 0, True, "steps"), (13, 17, False, "steps"),
    (14, 1, False, "steps"), (14, 1, True, "full"), (14, 2, False, "full"), (14, 2, True, "partial"), (14, 3, False, "steps"),
    (14, 3, True, "full"), (14, 4, False, "partial"), (14, 4, True, "steps"), (14, 14, False, "full"), (14, 14, True, "steps"),
    (14, 14, False, "partial"), (14, 15, False, "full"), (14, 15, True, "steps"), (14, 16, False, "steps"), (14, 16, True, "full"),
    (14, 0, False, "steps"), (14, 0, True, "full"), (14, 17, False, "full"), (14, 17, True, "full"),
]


@pytest.mark.parametrize("n,variant,real,tape", PARITY_CASES)
def test_per_atom_terms_match_the_oracle_at_thirteen_and_fourteen_qubits(cuda_device, n, variant, real, tape):
    """13 qubits: the smallest register with two tiles, so one index bit lies outside the tile in each layout (groups whose start /
    finish mask is empty in one layout).  Every atom its own group, atom 1 undriven, atom n-2 undetuned."""
    ref = _oracle(n, real, False)
    got = _run(_terms(n, real), _inputs(n), cuda_device, variant, tape=tape, real=real)
    st = got["stats"]
    assert got["amp"].shape[1] == n - 1 and got["det"].shape[1] == n - 1 and got["amp"].is_complex() != real
    _assert_kernels(st, variant, False, real, n)
    if st["kernel_family"] == "chained-tiles" or tape != "partial":
        assert st["tape"] == TAPE_STAT[tape], st
    _check(f"a N{n} v{variant} {'real' if real else 'cplx'} {tape}", got, ref, ORACLE_BARS, real)


@pytest.mark.parametrize("variant,real,tape", [(1, False, "full"), (1, True, "steps"), (2, False, "steps"), (2, True, "full"),
                                               (14, False, "full"), (14, True, "partial"), (0, False, "full"), (0, True, "steps")])
def test_global_drive_with_per_atom_detunings_matches_the_oracle(cuda_device, variant, real, tape):
    """ONE amplitude term on all atoms and one detuning term per atom (gd = N - 1 groups; the doppler / SLM shape): the loop-free
    FAST instantiation, with real tables the single-tape-read adjoint."""
    n = 14
    ref = _oracle(n, real, True)
    got = _run(_terms(n, real, True), _inputs(n), cuda_device, variant, tape=tape, real=real)
    assert got["amp"].shape[1] == 1 and got["det"].shape[1] == n - 1
    _assert_kernels(got["stats"], variant, True, real, n)
    _check(f"a-global N{n} v{variant} {'real' if real else 'cplx'} {tape}", got, ref, ORACLE_BARS, real)


# ---- b. small registers against the dense oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("n,solver,real,tsave", [(8, "KRYLOV_SE", False, PER_ATOM_TSAVE), (8, "KRYLOV_SE", True, PER_ATOM_TSAVE),
                                                 (8, "DP5_SE", False, PER_ATOM_TSAVE), (10, "KRYLOV_SE", False, PER_ATOM_TSAVE),
                                                 (10, "DP5_SE", False, TSAVE_SHORT)])
def test_per_atom_terms_match_the_dense_oracle_on_small_registers(cuda_device, n, solver, real, tsave, variant):
    """The persistent per-bit sweep (variant 0) and the generic direct kernels (variant 1) pinned to the oracle for per-atom terms;
    DP5_SE against the dense CF4 Magnus model of the continuous scheme (several stages per interval, tsave-dependent nodes)."""
    ref = _oracle(n, real, False, "dense" if solver == "KRYLOV_SE" else "magnus", tsave)
    got = _run(_terms(n, real), _inputs(n, 1, len(tsave)), cuda_device, variant, real=real, solver=solver, tsave=tsave)
    assert got["stats"]["kernel_family"] == ("direct" if variant == 1 else "persistent"), got["stats"]
    if variant == 1:
        assert got["stats"]["kernel_fwd"] == "k_factor_direct" and got["stats"]["kernel_bwd"] == "k_factor_bwd_direct", got["stats"]
    _check(f"b N{n} {solver} v{variant} {'real' if real else 'cplx'}", got, ref, ORACLE_BARS, real)


# ---- c. per-trajectory tables ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _trajectory_sets(batch):
    return tuple(per_atom_terms_batch(13, N_SAMPLES, DT, seeds=tuple(1331 + b for b in range(batch)), **_holes(13)))


@lru_cache(maxsize=None)
def _trajectory_oracle():
    psi0, obs, w, cot = _inputs(13, 3)
    return oracle_value_and_grads(list(_trajectory_sets(3)), psi0, PER_ATOM_TSAVE, obs, w, cot)


@pytest.mark.parametrize("variant,tape", [(1, "full"), (2, "steps"), (4, "full"), (0, "full")])
def test_three_trajectories_with_their_own_tables_match_the_oracle(cuda_device, variant, tape):
    """coeff_batch = batch = 3 with three different table sets on one register, against the oracle run per trajectory (the U and tsave
    gradients summed over the trajectories)."""
    ref = _trajectory_oracle()
    got = _run(list(_trajectory_sets(3)), _inputs(13, 3), cuda_device, variant, tape=tape)
    assert got["amp"].shape == (3, 12, N_SAMPLES)
    _assert_kernels(got["stats"], variant, False, False, 13)
    _check(f"c N13 B3 v{variant} {tape}", got, ref, ORACLE_BARS)


@pytest.mark.parametrize("batch,variants", [(9, (1, 2, 10)), (16, (1, 0))])
def test_ragged_and_chip_filling_batches_of_per_atom_tables(cuda_device, batch, variants):
    """9 trajectories (ragged for the groups of 8 of the trajectory-per-XCD placement, variant 10) against the plain grid (2) and
    against the direct kernels (1); 16 trajectories on the automatic route against the direct kernels."""
    sets, inputs = list(_trajectory_sets(batch)), _inputs(13, batch)
    runs = {v: _run(sets, inputs, cuda_device, v, tape="full") for v in variants}
    assert runs[1]["stats"]["kernel_family"] == "direct"
    if 10 in runs:
        _assert_chained(runs[10]["stats"], False, False, lt=12)
        _assert_chained(runs[2]["stats"], False, False, lt=12, lgt=9)
        _check(f"c N13 B{batch} v10 against v2", runs[10], runs[2], AB_BARS)
    for v in variants[1:]:
        _check(f"c N13 B{batch} v{v} against v1", runs[v], runs[1], AB_BARS)


# ---- d. larger registers against the direct kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,real,tape,tsave", [(16, 0, False, "full", PER_ATOM_TSAVE), (16, 14, True, "steps", PER_ATOM_TSAVE),
                                                       (20, 0, False, "full", PER_ATOM_TSAVE), (21, 7, False, "full", PER_ATOM_TSAVE),
                                                       (22, 0, False, "steps", TSAVE_THREE)])
def test_per_atom_terms_on_larger_registers_match_the_direct_kernels(cuda_device, n, variant, real, tape, tsave):
    """Up to 22 + 22 groups (minus the undriven and the undetuned atom): the automatic choice at 16, 20 (2^12 tiles; a single 20-qubit
    trajectory would take blocks of two with ONE global drive, and must not here) and 22 qubits (wide tiles, the parked gradient
    slots behind a 128 KiB tile), three layouts at 21; every gradient row on its own."""
    terms = per_atom_terms(n, N_SAMPLES, DT, SEEDS[n], phase=not real, **_holes(n))
    inputs = per_atom_problem(n, 1, SEEDS[n] + 1, len(tsave), device=cuda_device)  # (formed on the GPU, not kept)
    ref = _run(terms, inputs, cuda_device, 1, tape=tape, real=real, tsave=tsave)
    assert ref["stats"]["kernel_family"] == "direct" and ref["stats"]["kernel_fwd"] == "k_factor_direct", ref["stats"]
    torch.cuda.empty_cache()
    got = _run(terms, inputs, cuda_device, variant, tape=tape, real=real, tsave=tsave)
    st = got["stats"]
    _assert_kernels(st, variant if variant != 7 else 0, False, real, n)
    assert "k_chain2" not in st["kernel_fwd"] and "k_chain2" not in st["kernel_bwd"], st
    if n >= 20 or variant == 14:
        assert st["kernel_family"] == "chained-tiles", st
    if n == 22 or variant == 14:
        assert "k_chain_wide" in st["kernel_fwd"] and "k_chain_wide" in st["kernel_bwd"], st
    _check(f"d N{n} v{variant} {'real' if real else 'cplx'} {tape} against v1", got, ref, AB_BARS)
    del got, ref, inputs
    torch.cuda.empty_cache()


def test_continuous_solver_with_per_atom_terms_on_the_chained_tiles(cuda_device):
    """DP5_SE at 13 qubits (several stages per interval, tsave-dependent interpolation nodes), variant 2 against variant 1."""
    terms, inputs = _terms(13), _inputs(13)
    ref = _run(terms, inputs, cuda_device, 1, solver="DP5_SE")
    got = _run(terms, inputs, cuda_device, 2, solver="DP5_SE")
    assert ref["stats"]["kernel_family"] == "direct"
    _assert_chained(got["stats"], False, False, lt=12, lgt=9)
    _check("d N13 DP5_SE v2 against v1", got, ref, AB_BARS)


# ---- e. the tangent sweep ------------------------------------------------------------------------------------------------------------------
TANGENT_ORACLE_RTOL, TANGENT_VALUE_ATOL, TANGENT_DUALITY_RTOL = 1e-8, 1e-9, 1e-9  # tests/test_gpu_tangent.py, tests/test_gpu_tangent_matrix.py


@lru_cache(maxsize=None)
def _tangent_problem():
    """9 qubits, every atom driven and detuned (9 + 9 groups), five directions with all four tangent inputs."""
    n, n_dir = 9, 5
    terms = per_atom_terms(n, N_SAMPLES, DT, SEEDS[n])
    gen = torch.Generator().manual_seed(9090)
    psi0 = product_state(n, gen)[None]
    amp, det = stack_tables([terms])
    randn = lambda *s, c=False: torch.randn(*s, generator=gen, dtype=torch.complex128 if c else torch.float64)  # noqa: E731
    d = {"d_amp": 8.0 * float(amp.abs().max()) * randn(n_dir, *amp.shape, c=True), "d_det": 8.0 * float(det.abs().max()) * randn(n_dir, *det.shape),
         "d_u": float(terms.u_pairs.abs().max()) * randn(n_dir, len(terms.u_pairs)), "d_psi0": randn(n_dir, 1, 2**n, c=True) / np.sqrt(2**n)}
    # sum Z, and occupations with a weight per atom plus a random diagonal
    diags = torch.stack([R.total_magnetization_diag(n), (0.5 + 0.1 * torch.arange(n, dtype=torch.float64)) @ R.occupation_table(n) / n
                         + torch.rand(2**n, generator=gen, dtype=torch.float64)])
    states, tangents = tangent_dense_reference(terms, d["d_amp"][:, 0], d["d_det"][:, 0], d["d_u"], psi0.T.contiguous(),
                                               d["d_psi0"].permute(0, 2, 1).contiguous(), torch.tensor(TSAVE_THREE, dtype=torch.float64),
                                               _solver("KRYLOV_SE"))
    return terms, psi0, amp, det, d, diags, states, tangents


def _solver(name):
    from pulser_diff_amd.solver import SolverType

    return SolverType[name]


@pytest.mark.parametrize("n_dir", [2, 5])
def test_tangent_sweep_with_one_group_per_atom_matches_the_dense_reference(cuda_device, n_dir):
    """fbg[] = index bit | group << 8 with nine different groups: dexpect entry by entry against the plain dense forward mode."""
    from pulser_diff_amd.solver import evolve_tangent

    terms, psi0, amp, det, d, diags, states, tangents = _tangent_problem()
    dev = cuda_device
    _, _, u, spec = to_native(terms, dev, _solver("KRYLOV_SE"), store_states=False)
    expect, dexpect = evolve_tangent(amp.to(dev), det.to(dev), u, torch.tensor(TSAVE_THREE, dtype=torch.float64), psi0.to(dev), spec, diags.to(dev),
                                     **{k: v[:n_dir].to(dev) for k, v in d.items()})
    want_val, want_der = tangent_rows_reference(states, tangents[:, :n_dir], diags)
    got_val, got_der = expect.cpu(), dexpect.cpu()
    assert tuple(got_der.shape) == tuple(want_der.shape) and bool(torch.isfinite(got_der).all())
    val_err = float(((got_val - want_val).abs().amax(dim=(1, 2)) / diags.abs().amax(dim=1)).max())
    worst = 0.0
    for k in range(n_dir):
        scale = float(want_der[k].abs().max())
        err = float((got_der[k] - want_der[k]).abs().max())
        worst = max(worst, err / scale)
        assert all(float(want_der[k, r].abs().max()) > 1e-2 for r in range(len(diags)))  # nothing passes on zeros
    print(f"PER_ATOM e N9 tangent n_dir={n_dir}: dexpect worst {worst:.2e} of the direction's largest entry, values {val_err:.2e} of the row weight")
    assert worst <= TANGENT_ORACLE_RTOL and val_err <= TANGENT_VALUE_ATOL


def test_tangent_sweep_is_dual_to_the_native_adjoint_for_single_atom_directions(cuda_device):
    """13 qubits, directions one-hot in ONE atom's amplitude or detuning table (a smooth bump on that row, zero elsewhere), so that one
    group's tangent is isolated:  sum w dexpect_d = Re<g_amp, d_amp_d> + <g_det, d_det_d>  with the g of evolve(...).backward()."""
    from pulser_diff_amd.solver import evolve, evolve_tangent

    n, dev = 13, cuda_device
    terms = _terms(n)
    psi0, obs, _, _ = (t.to(dev) for t in _inputs(n))
    amp, det = stack_tables([terms], dev)
    _, _, u, spec = to_native(terms, dev, _solver("KRYLOV_SE"), store_states=False)
    tsave = torch.tensor(PER_ATOM_TSAVE, dtype=torch.float64)
    bump = torch.sin(torch.linspace(0.3, 2.8, N_SAMPLES, dtype=torch.float64)).to(dev)
    rows_a, rows_d = (0, 1, 6, 11), (0, 5, 10, 11)  # first, second (atom 2: atom 1 is undriven), middle and last rows
    d_amp = torch.zeros(8, *amp.shape, dtype=torch.complex128, device=dev)
    d_det = torch.zeros(8, *det.shape, dtype=torch.float64, device=dev)
    for k, r in enumerate(rows_a):
        d_amp[k, 0, r] = (0.8 - 0.6j) * bump
    for k, r in enumerate(rows_d):
        d_det[4 + k, 0, r] = bump
    _, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec, obs, d_amp=d_amp, d_det=d_det)
    leaves = [amp.clone().requires_grad_(True), det.clone().requires_grad_(True)]
    _, expect = evolve(leaves[0], leaves[1], u, tsave, psi0, spec, obs)
    w = torch.randn(*expect.shape, generator=torch.Generator().manual_seed(1399), dtype=torch.float64).to(dev)
    (w * expect).sum().backward()
    worst = 0.0
    for k in range(8):
        prod = w * dexpect[k]
        lhs, abs_sum = float(prod.sum()), float(prod.abs().sum())
        rhs = float((leaves[0].grad.conj() * d_amp[k]).real.sum()) + float((leaves[1].grad * d_det[k]).sum())
        big = max(abs(lhs), abs(rhs))
        print(f"PER_ATOM e N13 duality direction {k}: tangent {lhs:+.15e} adjoint {rhs:+.15e} rel {abs(lhs - rhs) / big:.2e} big / sum|terms| {big / abs_sum:.2e}")
        assert big > 1e-3 * abs_sum > 0.0  # cannot pass on zeros
        assert abs(lhs - rhs) <= TANGENT_DUALITY_RTOL * big
        worst = max(worst, abs(lhs - rhs) / big)
    others = [float(dexpect[a].abs().max()) for a in range(8)]
    assert min(others) > 0.0


# ---- f. state sharding with the rank qubits in groups of their own -----------------------------------------------------------------------
def _sharded(n, g, all_driven):
    """Per-atom terms with the rank qubits (0 .. g-1) in single-atom groups: rank qubit g-1 undriven and rank qubit 0 undetuned (one
    rank qubit: qubit 0 driven, undetuned) — or, all_driven, every atom driven, so that two rank qubits sit in DIFFERENT flip groups."""
    from pulser_diff_amd.sharded import ShardedProblem

    undriven = () if (all_driven or g == 1) else (g - 1,)
    terms = per_atom_terms(n, N_SAMPLES, DT, 7000 + 10 * n + g, undriven=undriven, undetuned=(0,))
    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    prob = ShardedProblem(n, g, terms.dt, np.stack([c.numpy() for c, _ in amp_terms]), np.stack([c.numpy() for c, _ in det_terms]),
                          [mask_of(tg) for _, tg in amp_terms], [mask_of(tg) for _, tg in det_terms], terms.u_pairs.numpy(), tol=1e-13)
    gen = torch.Generator().manual_seed(7001 + n)
    psi0 = product_state(n, gen)
    x = torch.arange(2**n)
    obs = torch.zeros(2**n, dtype=torch.float64)
    for j in range(n):  # a weighted magnetisation: every atom's tables move it
        obs += (1.0 + 0.1 * j) * (1.0 - 2.0 * ((x >> (n - 1 - j)) & 1).to(torch.float64))
    return terms, prob, psi0, obs / n


@pytest.mark.parametrize("n,g,variant,all_driven", [(13, 3, 0, False), (15, 2, 0, False), (15, 2, 0, True), (17, 3, 14, False),
                                                    (16, 2, 1, False), (16, 2, 1, True)])
def test_sharded_runs_with_rank_qubits_in_their_own_groups_match_the_single_gpu_solver(cuda_device, n, g, variant, all_driven):
    """sh_grp[k] != 0 and sh_grp[k] < 0 (a rank qubit that is not driven): slabs of 10 qubits on the direct kernels, of 13 on the chained
    tiles, of 14 on wide tiles, of 14 on the direct kernels; final state, <O>(t_k) and every gradient (g_tsave included), per row."""
    from pulser_diff_amd import _native
    from pulser_diff_amd.sharded import grad_virtual_native, run_virtual_native
    from pulser_diff_amd.solver import evolve

    dev = cuda_device
    terms, prob, psi0, obs = _sharded(n, g, all_driven)
    psi0, obs = psi0.to(dev), obs.to(dev)
    w = torch.linspace(-0.3, 1.2, len(PER_ATOM_TSAVE), dtype=torch.float64)
    amp, det = stack_tables([terms], dev)
    _, _, u, spec = to_native(terms, dev, _solver("KRYLOV_SE"))
    leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True),
              torch.tensor(PER_ATOM_TSAVE, dtype=torch.float64).requires_grad_(True), psi0[None].clone().requires_grad_(True)]
    states, expect = evolve(*leaves, spec, obs[None])
    (expect[0, :, 0] * w.to(dev)).sum().backward()
    _native.set_kernel_variant(variant)
    try:
        final, e_sh, stats = run_virtual_native(prob, psi0, np.asarray(PER_ATOM_TSAVE), obs_diag=obs)
        out = grad_virtual_native(prob, psi0, np.asarray(PER_ATOM_TSAVE), obs, w.numpy(), time_grad=True)
    finally:
        _native.set_kernel_variant(0)
    family = "chained-tiles" if (n - g > 12 and variant != 1) else "direct"
    assert stats["kernel_family"] == family and out["stats"]["kernel_family"] == family
    if family == "chained-tiles":
        for name in (stats["kernel_fwd"], out["stats"]["kernel_fwd"], out["stats"]["kernel_bwd"]):
            base, a = _instantiation(name)
            assert base == ("k_chain_wide" if variant == 14 else "k_chain") and a[3 if variant == 14 else 4] == "false", name
    ref_e = expect[0, :, 0].detach()
    fig = {"final": float((final - states[-1, 0].detach()).abs().max() / states[-1, 0].detach().abs().max()),
           "expect": float((e_sh - ref_e).abs().max()), "expect_grad_run": float((out["expect"] - ref_e).abs().max())}
    g_ref = {k: l.grad.detach().cpu().numpy() for k, l in zip(("amp", "det", "u", "tsave", "psi0"), leaves)}
    rows = {"amp": (out["g_amp"], g_ref["amp"][0]), "det": (out["g_det"], g_ref["det"][0])}
    if not all_driven and g > 1:
        # The detuning of the UNDRIVEN atom g-1 (row g-2: atom 0 has no detuning term) only turns the phase of its |r> component, which
        # no diagonal observable sees: that row of the gradient is zero for the exact exponential (what is left is the truncation error
        # of the polynomial, measured at 5e-12 of the largest row, the same on both sides).  It is held to the bar of a row at the
        # floor (|got - ref| <= bar * 1e-2 * the largest row) and taken out of the per-row comparison, whose reference-side guard
        # would rightly refuse it.
        a, b = rows["det"]
        top = float(np.abs(b).max())
        fig["det_zero_row_ref"], fig["det_zero_row_diff"] = float(np.abs(b[g - 2]).max()) / top, float(np.abs(a[g - 2] - b[g - 2]).max()) / top
        keep = [r for r in range(len(b)) if r != g - 2]
        rows["det"] = (a[keep], b[keep])
    for key, (a, b) in rows.items():
        err, ratio = row_errors(a, b)
        fig[key + "_rows"], fig[key + "_smallest_row"] = float(err.max()), float(ratio.min())
    fig["u"] = rel_err(out["g_u"], g_ref["u"])
    fig["tsave"] = rel_err(out["g_tsave"], g_ref["tsave"])
    fig["psi0"] = rel_err(out["g_psi0"].cpu().numpy(), g_ref["psi0"][0])
    print(f"PER_ATOM f N{n} g{g} v{variant} {'all driven' if all_driven else 'holes'}: family={family} fwd={out['stats']['kernel_fwd']} "
          f"bwd={out['stats']['kernel_bwd']} | " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fig["final"] <= AB_BARS["states"] and fig["expect"] <= AB_BARS["expect"] and fig["expect_grad_run"] <= AB_BARS["expect"], fig
    assert fig.get("det_zero_row_ref", 0.0) <= 1e-10 and fig.get("det_zero_row_diff", 0.0) <= AB_BARS["grad"] * 1e-2, fig
    for key, (a, b) in rows.items():
        assert_rows_close(a, b, AB_BARS["grad"], f"sharded {key}")
    for key in ("u", "tsave", "psi0"):
        assert fig[key] <= AB_BARS["grad"], (key, fig)


@pytest.mark.parametrize("n,g", [(6, 1), (9, 2)])
def test_virtual_sharding_with_rank_qubits_in_their_own_groups_matches_the_dense_oracle(cuda_device, n, g):
    from pulser_diff_amd.sharded import run_virtual

    terms, prob, psi0, obs = _sharded(n, g, False)
    tsave = torch.tensor(PER_ATOM_TSAVE, dtype=torch.float64)
    final, expect = run_virtual(prob, psi0.to(cuda_device), tsave.numpy(), obs_diag=obs.to(cuda_device))
    ref = R.krylov_map_dense(terms, psi0[:, None], tsave)[:, :, 0]
    err_s = rel_err(final.cpu().numpy(), ref[-1].numpy())
    err_e = float(np.abs(expect.cpu().numpy() - (ref.abs() ** 2 * obs[None]).sum(1).numpy()).max())
    print(f"PER_ATOM f N{n} g{g} run_virtual against the dense oracle: final={err_s:.2e} expect={err_e:.2e}")
    assert err_s <= ORACLE_BARS["states"] and err_e <= ORACLE_BARS["expect"]
