"""Sub-stepped exponentials: save intervals so long that tau * half_width exceeds the cap of 6 (kRhoCap, csrc/plan.hpp) and
finish_runtime splits the interval's exponential into nsub = ceil(tau * half_width / 6) sub-exponentials — nsub * degree factors for
one stage, which every consumer of the factor list sees: the on-device factor table of the one-launch sweeps (k_build_ptable), the
host chain of the launch-per-factor families (build_step_chain), the block pairing of k_chain2 / k_chain2_bwd, the staging window of
the one-launch adjoint (at most 64 factors per interval, else the launch-per-factor adjoint takes over), the tape maps with unequal
interval lengths, the g_tsave contraction, the slab exchange of sharded runs and the tangent sweep's factor walk.

The save times come from the CPU restatement of the library's spectral bound (tests.helpers.gershgorin_half_width) and one of two
patterns of interval lengths in units of 6 / half_width (tests.helpers.SUBSTEP_RATIOS):
    MIXED  (0.6, 1.6, 0.3, 2.5, 1.4)  ->  nsub (1, 2, 1, 3, 2), 9 sub-exponentials; the longest interval has 3 * degree factors
    TWOS   (0.6, 1.6, 0.3, 1.9, 1.4)  ->  nsub (1, 2, 1, 2, 2), 8 sub-exponentials; the longest interval has 2 * degree factors
At the default tolerance the design gives degree 23 (MIXED, design rho 5.19) and 24 (TWOS, 5.91): 69 factors are past the staging
window of the one-launch adjoint, 48 are inside; the tests assert that from the plan.  The sample spacing dt is chosen AFTER the save
times (the tables of random_terms do not depend on it) so that the last save time lies inside the interpolated part of the table; the
save times are not rounded to the sample grid.

Every native run asserts, from the plan the library reports (spec.options["_last_stats"]): the half width equals the restatement
to 1e-9 relative, total_factors == degree * sum(nsub expected), the kernel family and kernels named are the ones the case is
about, and, for the one-launch families, whether the one-launch adjoint was kept (TWOS; MIXED on the lanes' full tape) or handed
over to the launch-per-factor adjoint (MIXED otherwise).  Each prints its plan: run with -s to see them.

Cases and bars (those of the sibling tests):
 1. dense oracle (R.krylov_map_dense, autograd through it): states 1e-9, gradients 1e-8 relative — one-wave lanes (4, 6 qubits),
    one-workgroup kernel (6, variant 8), persistent (8), direct and generic direct (8, variants 1 / 9); both patterns, tapes "steps"
    and "full"; B = 2 with per-trajectory tables on the lanes (4) and the persistent (8) kernels; forward values at 10 qubits.
 2. family against family (reference: the direct kernels, pinned by 1.), 1e-10 relative: 12 qubits (one-launch forward, launch-per-
    factor adjoint), 13 (automatic), 14 (chained tiles 1024 / 512 threads, XCD placement, wide tiles, 2^11 tiles); tapes "steps",
    "full" and "partial" with the tape boundary between a one-exponential and a sub-stepped interval; 13 qubits forward against the
    matrix-free Lanczos oracle at 1e-9.
 3. blocks of two factors (variants 17 / 19 against 1; bars of tests/test_gpu_pair_blocks_adjoint.py): 13 and 16 qubits, tapes "full"
    and "steps", an odd degree (a block straddles two sub-exponentials of one interval; forward blocks pair from the front, adjoint
    blocks from the back) and an even one.
 4. state-sharded (15 qubits, 4 slabs in one call) against the un-sharded run: final state 1e-11, <O> 1e-10, five gradients 1e-9.
 5. tangent sweep at 5 and 9 qubits, three directions (amplitude, detuning and U_ij tangents together), against the dense forward-mode
    reference at the bars of tests/test_gpu_tangent_matrix.py.
 6. Pauli and overlap observables next to a diagonal one at 8 qubits without stored states: rows at the right save points."""
import dataclasses
import time
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests.helpers import (SUBSTEP_COUNTS, SUBSTEP_RATIOS, gershgorin_half_width, mask_of, random_terms, rel_err, substepped_tsave,
                           tangent_dense_reference, to_native)

pytestmark = pytest.mark.gpu

STATE_RTOL = 1e-9     # native states against the dense map (tests/test_gpu_solver_parity.py)
GRAD_RTOL = 1e-8      # native gradients against autograd through the dense map
FAMILY_RTOL = 1e-10   # one kernel family against another
N_SAMPLES = 15
STAGE_CHUNK = 64      # kStageChunk (csrc/persist_kernels.hpp): factors of one interval the one-launch adjoint stages
GRAD_NAMES = ("amp", "det", "u", "tsave", "psi0")


def _with_dt(terms, tsave, n_samples):
    """`terms` with the sample spacing that puts the last save time half a sample before the clamped end of the table
    (R.interp_indices: from sample n - 2 on the coefficients are held constant)."""
    return dataclasses.replace(terms, dt=float(tsave[-1]) / (n_samples - 2.5))


def _scaled(terms, s):
    """`terms` with every drive amplitude times s: the second table set of the per-trajectory cases."""
    return dataclasses.replace(terms, amp_coeff=terms.amp_coeff * s, extra_amp=[(c * s, tg) for c, tg in terms.extra_amp])


@lru_cache(maxsize=None)
def _problem(n, pattern, batch=1, local=True, phase=True, det_groups=1, seed=None):
    """One seeded problem on the CPU: `batch` trajectories, each with its own table set (drive amplitudes times 1, 0.8, ...), the
    half width over all of them, the save times of `pattern`, psi0 (B, dim), cotangents of the states at every save point (n_t, B, dim),
    weights of <sum Z> at every save point."""
    base = random_terms(n, N_SAMPLES, 1.0, seed=(4100 + n) if seed is None else seed, local=local and n > 1, phase=phase)
    if det_groups == 0:
        base = R.HamTerms(base.n_qubits, base.u_pairs, base.amp_coeff, None, base.dt, base.n_samples, base.amp_targets, [])
    scale = torch.linspace(1.0, 0.8, batch, dtype=torch.float64) if batch > 1 else torch.ones(1, dtype=torch.float64)
    sets = [_scaled(base, float(s)) for s in scale]
    hw = gershgorin_half_width(sets)
    tsave = substepped_tsave(hw, SUBSTEP_RATIOS[pattern])
    sets = [_with_dt(t, tsave, N_SAMPLES) for t in sets]
    gen = torch.Generator().manual_seed(977 * n + batch)
    dim = 2**n
    psi0 = torch.randn(batch, dim, generator=gen, dtype=torch.complex128)
    psi0 = psi0 / psi0.norm(dim=1, keepdim=True)
    cot = torch.randn(len(tsave), batch, dim, generator=gen, dtype=torch.complex128) / 2 ** (n / 2)
    w = torch.linspace(-0.4, 0.9, len(tsave), dtype=torch.float64)
    return {"n": n, "pattern": pattern, "sets": sets, "scale": scale, "half_width": hw, "tsave": tsave, "psi0": psi0, "cot": cot, "w": w,
            "zd": R.total_magnetization_diag(n)}


def _loss(states_tbd, expect, cot, w):
    """Cotangents on the states AND on <sum Z> at every save point.  states (n_t, B, dim), expect (n_obs, n_t, B)."""
    return (cot.conj() * states_tbd).real.sum() + (w[:, None] * expect[0]).sum()


@lru_cache(maxsize=None)
def _oracle(n, pattern, batch, grads=True):
    """The dense map of every trajectory (exact matrix exponentials) and, if asked, autograd through it: numpy arrays shaped like
    the native outputs."""
    prob = _problem(n, pattern, batch)
    t0 = time.perf_counter()
    u = prob["sets"][0].u_pairs.clone().requires_grad_(grads)
    ts = prob["tsave"].clone().requires_grad_(grads)
    p0 = prob["psi0"].clone().requires_grad_(grads)
    o_sets, states = [], []
    with torch.set_grad_enabled(grads):
        for b, tr in enumerate(prob["sets"]):
            o = R.HamTerms(n, u, tr.amp_coeff.clone().requires_grad_(grads), tr.det_coeff.clone().requires_grad_(grads), tr.dt,
                           tr.n_samples, tr.amp_targets, tr.det_targets)
            o.extra_amp = [(c.clone().requires_grad_(grads), tg) for c, tg in tr.extra_amp]
            o.extra_det = [(c.clone().requires_grad_(grads), tg) for c, tg in tr.extra_det]
            o_sets.append(o)
            states.append(R.krylov_map_dense(o, p0[b][:, None], ts)[:, :, 0])
        st = torch.stack(states, dim=1)  # (n_t, B, dim)
        expect = (st.abs() ** 2 * prob["zd"][None, None]).sum(2)[None]  # (1, n_t, B)
        out = {"states": st.detach().numpy(), "expect": expect.detach().numpy()}
        if grads:
            _loss(st, expect, prob["cot"], prob["w"]).backward()
            out.update(amp=torch.stack([torch.stack([c.grad for c, _ in o.amp_terms()]) for o in o_sets]).numpy(),
                       det=torch.stack([torch.stack([c.grad for c, _ in o.det_terms()]) for o in o_sets]).numpy(),
                       u=u.grad.numpy(), tsave=ts.grad.numpy(), psi0=p0.grad.numpy())
    out["seconds"] = time.perf_counter() - t0
    return out


def _check_plan(tag, stats, prob, family=None, fwd=None, bwd=None, tape=None):
    """The preconditions: the run really was sub-stepped as the pattern says, on the kernels the case is about."""
    counts = SUBSTEP_COUNTS[prob["pattern"]]
    lo, hi = stats["spectral"]
    print(f"{tag}: half width {0.5 * (hi - lo):.6f} (restated {prob['half_width']:.6f}), design rho {stats.get('rho', float('nan')):.4f}, "
          f"degree {stats['degree']}, factors {stats['total_factors']} = {stats['degree']} x {stats['total_factors'] / stats['degree']:g} "
          f"(expected nsub {counts}), family {stats['kernel_family']}, fwd {stats['kernel_fwd']}, bwd {stats.get('kernel_bwd', '')}, "
          f"tape {stats.get('tape', '')}")
    assert abs(0.5 * (hi - lo) - prob["half_width"]) <= 1e-9 * prob["half_width"], stats
    assert stats["total_factors"] == stats["degree"] * sum(counts), stats
    if "n_stages" in stats:
        assert stats["n_stages"] == len(counts), stats  # one exponential per save interval: the sub-steps share its stage
    if family is not None:
        assert stats["kernel_family"] == family, stats
    if fwd is not None:
        assert stats["kernel_fwd"].startswith(fwd), stats
    if bwd is not None:
        assert stats["kernel_bwd"].startswith(bwd), stats
    if tape is not None:
        assert stats["tape"] == tape, stats


def _native(prob, device, variant, tape="steps", grads=True, store_states=True, real_amp=False, tol=0.0, state_loss=True):
    """evolve (+ backward of _loss) on `device`: (stats, dict of numpy arrays).  tape: "steps" | "full" | "partial:<trailing intervals>"."""
    from pulser_diff_amd.solver import SolverType, evolve

    sets = prob["sets"]
    amp, det, u, spec = to_native(sets[0], device, SolverType.KRYLOV_SE, tol=tol, store_states=store_states, batch_tables=len(sets))
    amp = amp * prob["scale"].to(device)[:, None, None]
    if real_amp:
        assert float(amp.imag.abs().max()) == 0.0
        amp = amp.real.contiguous()  # a phase-free drive handed over as a real table: the real-drive adjoint
    spec.kernel_variant = variant
    spec.tape, _, steps = tape.partition(":")
    spec.tape_steps = int(steps) if steps else None
    leaves = [amp.detach().clone(), det.detach().clone(), u.detach().clone(), prob["tsave"].clone(), prob["psi0"].to(device)]
    obs = prob["zd"][None].to(device)
    if not grads:
        with torch.no_grad():
            states, expect = evolve(*leaves, spec, obs)
        torch.cuda.synchronize()
        return dict(spec.options["_last_stats"]), {"states": states.cpu().numpy(), "expect": expect.cpu().numpy()}
    for t in leaves:
        t.requires_grad_(True)
    states, expect = evolve(*leaves, spec, obs)
    loss = _loss(states, expect, prob["cot"].to(device), prob["w"].to(device)) if state_loss else (prob["w"].to(device)[:, None] * expect[0]).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = {"states": states.detach().cpu().numpy(), "expect": expect.detach().cpu().numpy()}
    for name, leaf in zip(GRAD_NAMES, leaves):
        out[name] = (torch.zeros(0) if leaf.grad is None or leaf.numel() == 0 else leaf.grad).detach().cpu().numpy()
    return dict(spec.options["_last_stats"]), out


def _tape_name(tape, store_states=True):
    """What stats["tape"] says for a requested tape (stored states ARE the per-save-point tape: "none")."""
    return {"steps": "none" if store_states else "steps", "full": "full"}.get(tape, "partial")


# ---- 1. against the dense oracle -----------------------------------------------------------------------------------------------
ORACLE_CASES = [  # qubits, variant, batch (= table sets), family, forward kernel, one-launch adjoint kernel
    (4, 0, 2, "lanes", "k_lanes", "k_lanes_bwd"),
    (6, 0, 1, "lanes", "k_lanes", "k_lanes_bwd"),
    (6, 8, 1, "persistent", "k_persist", "k_persist_bwd"),
    (8, 0, 2, "persistent", "k_persist", "k_persist_bwd"),
    (8, 1, 1, "direct", "k_factor_direct", None),
    (8, 9, 1, "direct", "k_factor_direct", None),
]


@pytest.mark.parametrize("tape", ["steps", "full"])
@pytest.mark.parametrize("pattern", ["MIXED", "TWOS"])
@pytest.mark.parametrize("n_qubits,variant,batch,family,fwd,one_launch_bwd", ORACLE_CASES,
                         ids=[f"N{c[0]}-v{c[1]}-B{c[2]}-{c[3]}" for c in ORACLE_CASES])
def test_substepped_intervals_match_the_dense_oracle(cuda_device, n_qubits, variant, batch, family, fwd, one_launch_bwd, pattern, tape):
    """States, <sum Z> and all five gradients (amplitude and detuning tables, U_ij, evaluation times, psi0) with state and expectation
    cotangents at every save point, against autograd through the oracle's dense map.  The one-launch adjoint stays while the longest
    interval has at most 64 factors (TWOS) — on the one-wave lanes also beyond, with the full tape — and otherwise the launch-per-factor
    adjoint reads what the one-launch forward sweep left (MIXED: 3 * degree factors)."""
    prob = _problem(n_qubits, pattern, batch)
    ref = _oracle(n_qubits, pattern, batch)
    stats, got = _native(prob, cuda_device, variant, tape)
    longest = max(SUBSTEP_COUNTS[pattern]) * stats["degree"]
    assert (longest <= STAGE_CHUNK) == (pattern == "TWOS"), (longest, stats)  # the premise of the two patterns
    if one_launch_bwd is None:
        bwd = "k_factor_bwd_direct"
    else:
        kept = pattern == "TWOS" or (family == "lanes" and tape == "full")
        bwd = one_launch_bwd if kept else "k_factor_bwd_direct"
    _check_plan(f"oracle N{n_qubits} v{variant} B{batch} {pattern} {tape}", stats, prob, family, fwd, bwd, _tape_name(tape))
    errs = {"states": rel_err(got["states"], ref["states"]), "expect": float(np.abs(got["expect"] - ref["expect"]).max())}
    errs.update({k: rel_err(got[k], ref[k]) for k in GRAD_NAMES})
    print("  errors: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  (oracle {ref['seconds']:.1f} s)")
    assert got["amp"].shape == ref["amp"].shape and got["det"].shape == ref["det"].shape
    assert errs["states"] < STATE_RTOL
    assert errs["expect"] < 1e-9
    assert np.abs((np.abs(got["states"]) ** 2).sum(2) - 1.0).max() < 1e-11
    for k in GRAD_NAMES:
        assert float(np.abs(ref[k]).max()) > 0.0, k  # nothing passes on zeros
        assert errs[k] < GRAD_RTOL, k


@pytest.mark.parametrize("pattern", ["MIXED", "TWOS"])
@pytest.mark.parametrize("variant,family,fwd", [(0, "persistent", "k_persist"), (1, "direct", "k_factor_direct")])
def test_substepped_forward_values_at_ten_qubits_match_the_dense_oracle(cuda_device, variant, family, fwd, pattern):
    """10 qubits (1024 amplitudes: four per thread in the one-workgroup sweep), forward only: every stored state and <sum Z>."""
    prob = _problem(10, pattern)
    ref = _oracle(10, pattern, 1, grads=False)
    stats, got = _native(prob, cuda_device, variant, grads=False)
    _check_plan(f"forward N10 v{variant} {pattern}", stats, prob, family, fwd)
    err = rel_err(got["states"], ref["states"])
    print(f"  states {err:.2e}  (oracle {ref['seconds']:.1f} s)")
    assert err < STATE_RTOL
    assert np.abs(got["expect"] - ref["expect"]).max() < 1e-9


# ---- 2. family against family ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _direct_reference(n):
    """The direct kernels (variant 1) on MIXED with the full tape: what section 1 pins to the oracle at 8 qubits."""
    prob = _problem(n, "MIXED")
    stats, out = _native(prob, torch.device("cuda:0"), 1, "full")
    _check_plan(f"reference N{n} v1 MIXED full", stats, prob, "direct", "k_factor_direct", "k_factor_bwd_direct", "full")
    return out


FAMILY_CASES = [  # qubits, variant, family, forward kernel, adjoint kernel
    (12, 0, "persistent", "k_persist", "k_factor_bwd_direct"),  # 12 qubits: the one-launch forward, never the one-launch adjoint
    (13, 0, "direct", "k_factor_direct", "k_factor_bwd_direct"),  # automatic: one 13-qubit trajectory is two tiles
    (14, 2, "chained-tiles", "k_chain<12,9,", "k_chain<12,9,"),    # 512 threads per tile
    (14, 4, "chained-tiles", "k_chain<12,10,", "k_chain<12,10,"),  # 1024 threads per tile
    (14, 10, "chained-tiles", "k_chain<12,", "k_chain<12,"),
    (14, 14, "chained-tiles", "k_chain_wide", "k_chain_wide"),
    (14, 15, "chained-tiles", "k_chain<11,", "k_chain<11,"),
]


# (the partial tape belongs to the launch-per-factor sweeps from 13 qubits on)
FAMILY_PARAMS = [c + (tape,) for c in FAMILY_CASES for tape in ("steps", "full", "partial:2", "partial:4") if c[0] >= 13 or ":" not in tape]


@pytest.mark.parametrize("n_qubits,variant,family,fwd,bwd,tape", FAMILY_PARAMS, ids=[f"N{c[0]}-v{c[1]}-{c[5]}" for c in FAMILY_PARAMS])
def test_substepped_intervals_agree_across_kernel_families(cuda_device, n_qubits, variant, family, fwd, bwd, tape):
    """MIXED beyond the dense oracle's reach, every gradient kind, against the direct kernels.  Partial tapes keep the factor outputs
    of the trailing 2 intervals (nsub 3, 2: the boundary lies behind a one-exponential interval) or 4 (nsub 2, 1, 3, 2: behind the
    first interval), so that region B holds intervals of 2 * degree - 1, degree - 1 and 3 * degree - 1 entries."""
    prob = _problem(n_qubits, "MIXED")
    ref = _direct_reference(n_qubits)
    stats, got = _native(prob, cuda_device, variant, tape)
    _check_plan(f"family N{n_qubits} v{variant} MIXED {tape}", stats, prob, family, fwd, bwd, _tape_name(tape))
    if variant == 10:
        assert stats["kernel_fwd"].endswith(",true>"), stats  # trajectory-per-XCD placement
    if tape.startswith("partial"):
        assert stats["tape_steps"] == int(tape.partition(":")[2]), stats
    errs = {k: rel_err(got[k], ref[k]) for k in ("states", "expect") + GRAD_NAMES}
    print("  errors: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < FAMILY_RTOL, k


def test_substepped_thirteen_qubits_match_the_matrix_free_oracle(cuda_device):
    """The reference of the family-against-family cases itself, at 13 qubits: every stored state of the MIXED run against the oracle's
    matrix-free Lanczos map (up to 80 Krylov vectors per interval, tolerance 1e-14; 0.1 s of CPU for the five intervals)."""
    prob = _problem(13, "MIXED")
    tr = prob["sets"][0]
    t0 = time.perf_counter()
    ref = R.krylov_map_matrix_free(tr, prob["psi0"].T.contiguous().numpy(), prob["tsave"].numpy(), save_all=True, tol=1e-14)
    seconds = time.perf_counter() - t0
    stats, got = _native(prob, cuda_device, 1, grads=False)
    _check_plan("matrix-free N13 v1 MIXED", stats, prob, "direct", "k_factor_direct")
    err = rel_err(got["states"][:, 0, :], ref[:, :, 0])
    print(f"  states {err:.2e}  (oracle {seconds:.1f} s)")
    assert err < STATE_RTOL


# ---- 3. blocks of two factors ----------------------------------------------------------------------------------------------------
def _degree_for(prob, device, tol):
    from pulser_diff_amd.solver import SolverType, evolve

    amp, det, u, spec = to_native(prob["sets"][0], device, SolverType.KRYLOV_SE, tol=tol, store_states=False)
    spec.kernel_variant = 1
    with torch.no_grad():
        evolve(amp, det, u, prob["tsave"], prob["psi0"].to(device), spec, None)
    return spec.options["_last_stats"]["degree"]


@pytest.mark.parametrize("n_qubits,tape,odd,det_groups", [(13, "full", True, 1), (13, "steps", False, 1), (16, "full", False, 0),
                                                          (16, "steps", True, 1)])
def test_substepped_intervals_in_blocks_of_two_factors(cuda_device, n_qubits, tape, odd, det_groups):
    """k_chain2 / k_chain2_bwd (variant 17) and the one-factor adjoint next to them (19) against the direct kernels (1), phase-free
    global drive as a real table.  All sub-exponentials of an interval share the stage index, so with an ODD degree a block spans
    the kappa-scaled last factor of one sub-exponential and the first factor of the next (nsub = 2: even interval; nsub = 1, 3: odd
    interval, a one-factor block at its end in the forward pass and at its start in the adjoint); with an EVEN degree no block
    does.  The degree follows from the design rho (fixed by the pattern: the amplitude scale cancels in tau * half_width) and the
    tolerance, so the tolerance is scanned for the wanted parity (1e-13, the default: 23; 1e-12: 22)."""
    from tests.test_gpu_pair_blocks_adjoint import NAMES, _compare

    prob = _problem(n_qubits, "MIXED", local=False, phase=False, det_groups=det_groups, seed=4300 + n_qubits)
    tol = next((t for t in (0.0, 1e-12, 1e-11, 3e-13) if (_degree_for(prob, cuda_device, t) % 2 == 1) == odd), None)
    assert tol is not None, "no tolerance gave the wanted parity of the polynomial degree"
    out, stats = {}, {}
    for v in (1, 19, 17):
        stats[v], res = _native(prob, cuda_device, v, tape, real_amp=True, tol=tol)
        out[v] = [torch.as_tensor(res[k]) for k in NAMES]
        torch.cuda.empty_cache()
    _check_plan(f"blocks N{n_qubits} v1 MIXED {tape}", stats[1], prob, "direct", "k_factor_direct", "k_factor_bwd_direct", _tape_name(tape))
    _check_plan(f"blocks N{n_qubits} v19 MIXED {tape}", stats[19], prob, tape=_tape_name(tape))
    assert not stats[19]["kernel_bwd"].startswith("k_chain2_bwd<"), stats[19]
    _check_plan(f"blocks N{n_qubits} v17 MIXED {tape}", stats[17], prob, "chained-tiles", "k_chain2<", "k_chain2_bwd<", _tape_name(tape))
    assert (stats[17]["degree"] % 2 == 1) == odd, stats[17]
    assert stats[1]["degree"] == stats[17]["degree"] == stats[19]["degree"]
    _compare(out)


# ---- 4. state-sharded ------------------------------------------------------------------------------------------------------------
def test_substepped_intervals_on_a_state_sharded_run(cuda_device):
    """15 qubits on 4 slabs of 13 (chained tiles, one slab exchange per factor), all ranks in one call: final state, <sum Z> and every
    gradient including g_tsave against the un-sharded run (bars of tests/test_gpu_sharded.py and test_gpu_sharded_time_grad.py)."""
    from pulser_diff_amd.sharded import ShardedProblem, grad_virtual_native, run_virtual_native

    n, g = 15, 2
    prob = _problem(n, "MIXED")
    tr = prob["sets"][0]
    amp_terms, det_terms = tr.amp_terms(), tr.det_terms()
    sharded = ShardedProblem(n, g, tr.dt, np.stack([c.numpy() for c, _ in amp_terms]), np.stack([c.numpy() for c, _ in det_terms]),
                             [mask_of(tg) for _, tg in amp_terms], [mask_of(tg) for _, tg in det_terms], tr.u_pairs.numpy(), tol=1e-13)
    stats, ref = _native(prob, cuda_device, 0, "steps", state_loss=False)
    _check_plan(f"un-sharded N{n} v0 MIXED", stats, prob)
    psi0, zd = prob["psi0"][0].to(cuda_device), prob["zd"].to(cuda_device)
    final, e_sh, st_fwd = run_virtual_native(sharded, psi0, prob["tsave"].numpy(), obs_diag=zd)
    _check_plan(f"sharded forward ({n},{g}) MIXED", st_fwd, prob, "chained-tiles", "k_chain")
    out = grad_virtual_native(sharded, psi0, prob["tsave"].numpy(), zd, prob["w"].numpy(), time_grad=True)
    st = out["stats"]
    print(f"sharded adjoint ({n},{g}) MIXED: degree {st['degree']}, factors {st['total_factors']}, family {st['kernel_family']}, bwd {st['kernel_bwd']}")
    assert st["total_factors"] == st["degree"] * sum(SUBSTEP_COUNTS["MIXED"]) and st["degree"] == stats["degree"], st
    assert st["kernel_family"] == "chained-tiles" and st["kernel_bwd"].startswith("k_chain"), st
    errs = {"final": rel_err(final.cpu().numpy(), ref["states"][-1, 0]), "expect fwd": float(np.abs(e_sh.cpu().numpy() - ref["expect"][0, :, 0]).max()),
            "expect": float(np.abs(out["expect"].cpu().numpy() - ref["expect"][0, :, 0]).max()),
            "amp": rel_err(out["g_amp"], ref["amp"][0]), "det": rel_err(out["g_det"], ref["det"][0]), "u": rel_err(out["g_u"], ref["u"]),
            "tsave": rel_err(out["g_tsave"], ref["tsave"]), "psi0": rel_err(out["g_psi0"].cpu().numpy(), ref["psi0"][0])}
    print("  errors: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["final"] < 1e-11
    assert errs["expect fwd"] < 1e-10 and errs["expect"] < 1e-10
    for k in GRAD_NAMES:
        assert errs[k] < 1e-9, k


# ---- 5. tangent sweep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_qubits", [5, 9])
def test_substepped_intervals_in_the_tangent_sweep(cuda_device, n_qubits):
    """evolve_tangent walks the same factor list: three directions with amplitude, detuning and U_ij tangents together, diagonal, Pauli
    and overlap rows, entry by entry against the dense forward-mode reference (tests/test_gpu_tangent_matrix.py's check and bars).
    The sweep reports no plan of its own: the preconditions are read from a plain evolve of the same problem and save times."""
    from tests import test_gpu_tangent_matrix as M

    base = dict(M._problem(n_qubits, 1, 1, 3))
    hw = gershgorin_half_width(base["terms"])
    tsave = substepped_tsave(hw, SUBSTEP_RATIOS["MIXED"])
    base["terms"] = _with_dt(base["terms"], tsave, M.N_SAMPLES)
    base["ref_terms"] = M._terms_with_tables(base["terms"], base["amp"][0], base["det"][0])
    plan = {"n": n_qubits, "pattern": "MIXED", "sets": [base["terms"]], "scale": torch.ones(1, dtype=torch.float64), "half_width": hw,
            "tsave": tsave, "psi0": base["psi0"], "zd": R.total_magnetization_diag(n_qubits)}
    stats, _ = _native(plan, cuda_device, 0, grads=False, store_states=False)
    _check_plan(f"tangent N{n_qubits} MIXED (plan of evolve)", stats, plan)
    d_amp, d_det, d_u, _ = M._inputs(base, "adu", 0, 3)
    t0 = time.perf_counter()
    ref = tangent_dense_reference(base["ref_terms"], d_amp[:, 0], d_det[:, 0], d_u, base["psi0"].T.contiguous(), None, tsave,
                                  M.SolverType.KRYLOV_SE)
    print(f"reference: {time.perf_counter() - t0:.1f} s of CPU")
    worst = M._check(f"N{n_qubits}-MIXED-D3", base, "KRYLOV_SE", tuple(float(t) for t in tsave), "adu", 3, "full", ref, cuda_device)
    print(f"worst relative error of a direction {worst:.2e}")


# ---- 6. observables at the save points -------------------------------------------------------------------------------------------
def test_substepped_observable_rows_land_at_their_save_points(cuda_device):
    """8 qubits, MIXED, no stored states: a diagonal, a Pauli-string and a state-overlap observable from the dense oracle's states
    (bars: 1e-9 times the weight of the row's operator, as in the Pauli and overlap value tests)."""
    from pulser_diff_amd.observables import PauliObservable, StateOverlap, pack_overlaps
    from pulser_diff_amd.solver import SolverType, evolve, split_expect

    n = 8
    prob = _problem(n, "MIXED")
    ref = torch.as_tensor(_oracle(n, "MIXED", 1)["states"])[:, 0]  # (n_t, dim)
    pauli = PauliObservable(n, [(0.7, {0: "X", n - 1: "X"}), (-0.4, {1: "Y", 2: "Z"}), (0.5, {3: "Z"})])
    gen = torch.Generator().manual_seed(86)
    target = torch.randn(2**n, generator=gen, dtype=torch.complex128) + 4.0 * ref[3]  # weight on the state after the longest interval
    target = target / target.norm()
    amp, det, u, spec = to_native(prob["sets"][0], cuda_device, SolverType.KRYLOV_SE, store_states=False)
    spec.pauli = [pauli]
    spec.overlaps = pack_overlaps([StateOverlap(target)], 2**n, 1, cuda_device)
    with torch.no_grad():
        states, expect = evolve(amp, det, u, prob["tsave"], prob["psi0"].to(cuda_device), spec, prob["zd"][None].to(cuda_device))
    assert states.numel() == 0
    _check_plan(f"observables N{n} MIXED", spec.options["_last_stats"], prob, "persistent", "k_persist")
    rows, ov = split_expect(expect.cpu(), 1)
    want_z = (ref.abs() ** 2 * prob["zd"][None]).sum(1)
    want_p = torch.einsum("ti,ij,tj->t", ref.conj(), pauli.to_dense(), ref).real
    want_o = (target.conj()[None] * ref).sum(1)
    errs = {"diagonal": float((rows[0, :, 0] - want_z).abs().max()) / n, "pauli": float((rows[1, :, 0] - want_p).abs().max()) / 1.6,
            "overlap": float((ov[0, :, 0] - want_o).abs().max())}
    print("  errors over the row weight: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert float(want_p.abs().max()) > 1e-2 and float(want_o.abs().max()) > 1e-2  # nothing passes on zeros
    for k, v in errs.items():
        assert v < 1e-9, k
