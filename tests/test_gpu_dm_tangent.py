"""Tangent sweep of master-equation runs (lindblad.mesolve_tangent; k_factor_tangent<D, true> on the doubled register, the
density-matrix rows and their tangents at every save point): d<O>(t_k)/d theta for every evaluation time from ONE forward-mode sweep.

1. Every row kind against the oracle: R.lindblad_magnus_dense on terms + s * direction, torch.autograd.functional.jacobian of the
   rows (tests/test_gpu_dm_observables._torch_rows) w.r.t. s at s = 0 — recorded in tests/golden/dm_tangent_oracle.npz by
   tests/dm_tangent_reference.py (the oracle takes minutes per case).  2, 3 and 4 atoms (doubled dimension 16, 64, 256: below,
   inside and exactly one 256-thread workgroup), three noise sets chosen for the relative-flip masks of their dissipator block
   (dephasing: diagonal; + relaxation: diagonal and double flip; a non-normal eff_noise: all four), 1, 3, 5 (padded to 6) and 8
   directions that mix d_amp, d_det and d_u, one of them zero.  Bars (the project's own for this path): values 1e-8 absolute,
   dexpect[d] within 1e-7 of the reference relative to the direction's largest entry; h_max and tol = 1e-12 as in
   test_gradients_of_all_row_kinds_match_dense_autograd.
2. 5 and 7 atoms (1024 and 16384 amplitudes: four workgroups / partner lines in other workgroups) against the gradients of
   mesolve(..., store_states=False): sum_k w_k dexpect[d, row, k] == <grad of sum_k w_k row_k, direction_d> at DUALITY_RTOL = 1e-9,
   tol = 1e-12.  This is the SAME solver on both sides — forward against reverse mode of one discrete map: it shows that the sweep
   is the adjoint's dual at sizes the dense oracle does not reach, not that either is right.  Case 1 carries the correctness.
3. A tangent of psi0: d rho0 = |dpsi><psi| + |psi><dpsi|, against the oracle's linearity in rho0.
4. A NaN-filled workspace gives bit-identical results (3 atoms, 5 directions: a padded one).
5. The emulator: run_sensitivities(route="tangent") runs the sweep for diagonal, Pauli, fidelity and purity observables and agrees
   with route="adjoint-loop" at 1e-9; QuantumModel / deriv_param_all_times reach it.  (route=None keeps looping for noisy runs:
   tests/test_gpu_tangent.py pins that.)
6. The refusals, each before any launch, as the exception _native.check maps its code to.

Measured on an MI355X: 1. values 5.3e-12, tangents 2.4e-9 of the direction's largest entry (the purity row, whose derivative is
1e-3 of the others over these 4.6 ns, is the one that sets it); 2. 2.0e-15; 3. 3.3e-12 absolute; 4. bit-identical; 5. 1.2e-14 absolute."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd import pulses as pl
from pulser_diff_amd import solver as S
from pulser_diff_amd.derivative import deriv_param_all_times
from pulser_diff_amd.lindblad import mesolve, mesolve_tangent
from pulser_diff_amd.observables import DensityMatrixObservables, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap
from pulser_diff_amd.shots import ShotRequest
from pulser_diff_amd.solver import SolverType, evolve_geometry, evolve_tangent
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.dm_tangent_reference import NOISE, TSAVE, ZERO_DIRECTION, case_terms, directions as _directions, load_case, observables
from tests.helpers import random_terms, to_native
from tests.test_gpu_dm_observables import _me_observables, _torch_rows
from tests.test_gpu_master_equation_sizes import _ham_like, _noise_model, _random_kets
from tests.test_gpu_tangent import DUALITY_RTOL
from tests.test_gpu_workspace_contents import _filled

pytestmark = pytest.mark.gpu
BOTH = _native.TANGENT_PAIR_TERMS | _native.TANGENT_DENSITY_MATRIX  # RydTangent.flags of a master-equation sweep

VALUE_ATOL = 1e-8
TANGENT_RTOL = 1e-7
PUBLIC_RTOL = 1e-9


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


@lru_cache(maxsize=None)
def _oracle_case(n, noise_key):
    """The recorded oracle case (tests/dm_tangent_reference.py: inputs, values, Jacobian for 8 directions; the cases slice) with its
    terms and observables — loaded once, shared, never modified."""
    case = load_case(n, noise_key)
    case.update(terms=case_terms(n), obs=observables(n, case["target"]), tsave=torch.tensor(TSAVE, dtype=torch.float64))
    return case


@pytest.mark.parametrize("n_dir", [1, 3, 5, 8])
@pytest.mark.parametrize("noise_key", list(NOISE))
@pytest.mark.parametrize("n", [2, 3, 4])
def test_every_row_kind_matches_the_oracle(cuda_device, n, noise_key, n_dir):
    dev = cuda_device
    case = _oracle_case(n, noise_key)
    ham = _ham_like(case["terms"], dev)
    expect, dexpect = mesolve_tangent(ham, case["psi0"].to(dev), case["tsave"], _noise_model(NOISE[noise_key]), {"tol": 1e-12}, case["obs"],
                                      d_amp=case["d_amp"][:n_dir].to(dev), d_det=case["d_det"][:n_dir].to(dev), d_u=case["d_u"][:n_dir].to(dev))
    got_val, got_der = expect.cpu(), dexpect.cpu()
    assert tuple(got_val.shape) == tuple(case["val"].shape) == (7, 4, case["psi0"].shape[1])
    assert tuple(got_der.shape) == (n_dir,) + tuple(case["der"].shape[1:])
    assert bool(torch.isfinite(got_val).all()) and bool(torch.isfinite(got_der).all())
    val_err = float((got_val - case["val"]).abs().max())
    print(f"DM-TAN n={n} {noise_key} D={n_dir}: values, max error {val_err:.2e}")
    for d in range(n_dir):
        want = case["der"][d]
        scale, err = float(want.abs().max()), float((got_der[d] - want).abs().max())
        per_row = ", ".join(f"{type(o).__name__} {float((got_der[d, r] - want[r]).abs().max()):.1e}" for r, o in enumerate(case["obs"]))
        print(f"DM-TAN n={n} {noise_key} D={n_dir}: direction {d}: largest entry {scale:.3e}, max error {err:.3e}; per row: {per_row}")
        if d == ZERO_DIRECTION:
            assert float(got_der[d].abs().max()) == 0.0 and scale == 0.0
        else:
            assert scale > 1e-3  # nothing passes on zeros (the recorded directions: 2e-3 .. 2e-1 over the 4.6 ns of TSAVE)
            assert err <= TANGENT_RTOL * scale
    assert val_err < VALUE_ATOL


@pytest.mark.parametrize("n", [5, 7])
def test_duality_with_the_native_adjoint_past_one_workgroup(cuda_device, n):
    """Same solver on both sides (see the module docstring): forward mode against reverse mode of the one discrete map."""
    dev = cuda_device
    noise = _noise_model(NOISE["deph+relax"])
    terms = random_terms(n, 8, 0.004, seed=6400 + n, local=True)
    gen = torch.Generator().manual_seed(6500 + n)
    psi0 = _random_kets(2 ** n, 1, seed=6600 + n).to(dev)
    obs = _me_observables(n, gen, 1)
    tsave = torch.tensor([0.0, 0.0047, 0.0093], dtype=torch.float64)
    ham = _ham_like(terms, dev, requires_grad=True)
    d_amp, d_det, d_u = _directions(ham.amp_tables.detach().cpu(), ham.det_tables.detach().cpu(), ham.u_pairs.detach().cpu(), gen, 2)
    d_amp, d_det, d_u = d_amp.to(dev), d_det.to(dev), d_u.to(dev)
    expect, dexpect = mesolve_tangent(ham, psi0, tsave, noise, {"tol": 1e-12}, obs, d_amp=d_amp, d_det=d_det, d_u=d_u)
    res = mesolve(ham, psi0, tsave, noise, options={"tol": 1e-12}, observables=obs, store_states=False)
    rows = torch.stack(res.expect)
    assert float((expect - rows.detach()).abs().max()) <= 1e-10 * max(1.0, float(rows.abs().max()))  # one native value route against another
    w = _randn(gen, *rows.shape).to(dev)
    (w * rows).sum().backward()
    for d in range(2):
        prod = w * dexpect[d]
        lhs, abs_sum = float(prod.sum()), float(prod.abs().sum())
        rhs = (float((ham.amp_tables.grad.conj() * d_amp[d]).real.sum()) + float((ham.det_tables.grad * d_det[d]).sum())
               + float((ham.u_pairs.grad * d_u[d]).sum()))
        big = max(abs(lhs), abs(rhs))
        print(f"DM-DUAL n={n} direction {d}: tangent {lhs:+.15e}  adjoint {rhs:+.15e}  rel {abs(lhs - rhs) / big:.2e}  big / sum|terms| {big / abs_sum:.2e}")
        assert big > 1e-3 * abs_sum > 0.0  # cannot pass on zeros
        assert abs(lhs - rhs) <= DUALITY_RTOL * big


def test_tangent_of_psi0_on_a_density_matrix(cuda_device):
    """d rho0 = |dpsi><psi| + |psi><dpsi|; rho(t) is linear in rho0, so the oracle's integrator applied to d rho0 is d rho(t): the linear
    rows are the rows of d rho(t), the purity row 2 Re sum conj(rho) d rho."""
    dev, n, n_dir = cuda_device, 3, 2
    terms = random_terms(n, 8, 0.004, seed=6700, local=True)
    gen = torch.Generator().manual_seed(6701)
    psi0 = _random_kets(2 ** n, 1, seed=6702)
    dpsi = _randn(gen, n_dir, 2 ** n, 1, cplx=True) / np.sqrt(2 ** n)
    obs = _me_observables(n, gen, 1)
    tsave = torch.tensor(TSAVE, dtype=torch.float64)
    noise = NOISE["non-normal"]
    expect, dexpect = mesolve_tangent(_ham_like(terms, dev), psi0.to(dev), tsave, _noise_model(noise), {"tol": 1e-12}, obs, d_psi0=dpsi.to(dev))
    collapse = R.collapse_operators(n, noise)
    rho = R.lindblad_magnus_dense(terms, collapse, torch.outer(psi0[:, 0], psi0[:, 0].conj()), tsave, h_max=0.0002)
    linear = [o for o in obs if not isinstance(o, Purity)]
    assert isinstance(obs[-1], Purity) and len(linear) == len(obs) - 1
    val_err = float((expect.cpu() - torch.stack(_torch_rows(rho[..., None], obs))).abs().max())
    print(f"DM-PSI0 values: {val_err:.2e}")
    assert val_err < VALUE_ATOL
    for d in range(n_dir):
        drho0 = torch.outer(dpsi[d, :, 0], psi0[:, 0].conj()) + torch.outer(psi0[:, 0], dpsi[d, :, 0].conj())
        drho = R.lindblad_magnus_dense(terms, collapse, drho0, tsave, h_max=0.0002)
        want = torch.stack(_torch_rows(drho[..., None], linear) + [2.0 * (rho.conj() * drho).real.sum(dim=(1, 2))[:, None]])
        scale, err = float(want.abs().max()), float((dexpect[d].cpu() - want).abs().max())
        print(f"DM-PSI0 direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 1e-2 and err <= TANGENT_RTOL * scale


def test_poisoned_workspace_gives_bit_identical_results(cuda_device, monkeypatch):
    dev, n, n_dir = cuda_device, 3, 5
    case = _oracle_case(n, "non-normal")
    ham = _ham_like(case["terms"], dev)
    out = []
    for value in (0.0, float("nan")):
        monkeypatch.setattr(S, "_new_workspace", _filled(value))
        out.append(mesolve_tangent(ham, case["psi0"].to(dev), case["tsave"], _noise_model(NOISE["non-normal"]), {"tol": 1e-12}, case["obs"],
                                   d_amp=case["d_amp"][:n_dir].to(dev), d_det=case["d_det"][:n_dir].to(dev), d_u=case["d_u"][:n_dir].to(dev)))
        torch.cuda.synchronize()
    (v0, d0), (v1, d1) = out
    assert bool(torch.isfinite(v1).all()) and bool(torch.isfinite(d1).all()), "a region of the workspace is read before it is written"
    assert float(d0.abs().max()) > 1e-2
    assert torch.equal(v0, v1) and torch.equal(d0, d1)


def _noisy_emulator(dev):
    """Three atoms, dephasing + relaxation; float64 leaves: the amplitude of the constant pulse, the area of the Blackman pulse, the
    final detuning of the ramp."""
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)  # noqa: E731
    reg = pl.Register({"q0": torch.tensor([0.0, 0.0], dtype=torch.float64), "q1": torch.tensor([0.0, 8.0], dtype=torch.float64),
                       "q2": torch.tensor([8.0, 0.0], dtype=torch.float64)})
    seq = pl.Sequence(reg, pl.MockDevice)
    seq.declare_channel("rydberg_global", "rydberg_global")
    omega, area, det = f64([5.0]), f64([torch.pi]), f64([2.0])
    seq.add(pl.Pulse(pl.BlackmanWaveform(400, area), pl.RampWaveform(400, -5.0, det), 0.3), "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(400, omega, 0.0, 0.3), "rydberg_global")
    cfg = P.SimConfig(noise=("dephasing", "relaxation"), dephasing_rate=0.5, relaxation_rate=0.3)
    sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.1, config=cfg, evaluation_times=0.1, compute_device=dev)
    return sim, [omega, area, det]


def test_emulator_takes_the_tangent_route_for_noisy_runs(cuda_device):
    sim, x = _noisy_emulator(cuda_device)
    gen = torch.Generator().manual_seed(6800)
    target = _randn(gen, 8, cplx=True)
    obs = [DiagonalObservable(total_magnetization_diag(3)), PauliObservable(3, [(0.8, {0: "X", 2: "Y"}), (-0.5, {1: "Z"})]),
           StateOverlap(target / target.norm()), Purity()]
    tan = deriv_param_all_times(sim, x, obs, route="tangent")
    assert tan.route == "tangent"
    loop = sim.run_sensitivities(x, obs, route="adjoint-loop")
    assert loop.route == "adjoint-loop"
    n_t = len(sim.evaluation_times)
    assert tuple(tan.values.shape) == (4, n_t) and [tuple(g.shape) for g in tan.grads] == [(4, n_t, 1)] * 3
    assert float((tan.values.cpu() - loop.values.cpu()).abs().max()) <= 4e-9
    for o, ob in enumerate(obs):  # relative to the observable's largest derivative over all parameters and times
        scale = max(float(want[o].abs().max()) for want in loop.grads)
        assert scale > 1e-3  # nothing passes on zeros
        for name, got, want in zip(("omega", "area", "detuning"), tan.grads, loop.grads):
            err = float((got[o].cpu() - want[o].cpu()).abs().max())
            print(f"DM-EMU d {type(ob).__name__} / d {name}: largest entry {float(want[o].abs().max()):.3e}, max error {err:.3e}")
            assert err <= PUBLIC_RTOL * scale


def test_quantum_model_reaches_the_tangent_route(cuda_device):
    """A QuantumModel with collapse noise: the emulator it keeps (after one run) hands its parameters' sensitivities to the sweep."""
    from pulser_diff_amd.model import QuantumModel

    seq = pl.Sequence(pl.Register.rectangle(1, 3, spacing=8, prefix="q"), pl.MockDevice)
    seq.declare_channel("rydberg_global", "rydberg_global")
    omega, area = seq.declare_variable("omega"), seq.declare_variable("area")
    seq.add(pl.Pulse.ConstantPulse(400, omega, 0.0, 0.0), "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(400, area), pl.RampWaveform(400, 5.0, 0.0), 0), "rydberg_global")
    cfg = P.SimConfig(noise=("dephasing", "relaxation"), dephasing_rate=0.5, relaxation_rate=0.3)
    model = QuantumModel(seq, {"omega": torch.tensor([5.0], dtype=torch.float64, requires_grad=True),
                               "area": torch.tensor([torch.pi], dtype=torch.float64, requires_grad=True)},
                         sampling_rate=0.1, noise_config=cfg, compute_device=cuda_device)
    model.expectation()
    params = list(model.parameters())
    obs = [DiagonalObservable(total_magnetization_diag(3)), Purity()]
    tan = deriv_param_all_times(model._sim, params, obs, route="tangent")
    assert tan.route == "tangent"
    loop = deriv_param_all_times(model._sim, params, obs, route="adjoint-loop")
    for o in range(len(obs)):
        scale = max(float(want[o].abs().max()) for want in loop.grads)
        assert scale > 1e-3
        for got, want in zip(tan.grads, loop.grads):
            err = float((got[o].cpu() - want[o].cpu()).abs().max())
            print(f"DM-MODEL observable {o}: largest entry {float(want[o].abs().max()):.3e}, max error {err:.3e}")
            assert err <= PUBLIC_RTOL * scale


def test_refusals_arrive_before_any_launch(cuda_device):
    dev, n = cuda_device, 2
    terms = random_terms(n, 8, 0.004, seed=6900, local=True)
    ham = _ham_like(terms, dev)
    psi0 = _random_kets(4, 1, seed=6901).to(dev)
    tsave = torch.tensor(TSAVE, dtype=torch.float64)
    noise = _noise_model(NOISE["dephasing"])
    d_det = torch.ones(1, *ham.det_tables.shape, dtype=torch.float64, device=dev)
    with pytest.raises(NotImplementedError, match="reduced density"):
        mesolve_tangent(ham, psi0, tsave, noise, None, [ReducedDensityMatrix([0])], d_det=d_det)
    # the solver-level entry: a doubled-register spec with an RDM / shots / in evolve_geometry
    amp, det, u, spec = to_native(random_terms(2 * n, 8, 0.004, seed=6902, local=True), dev, SolverType.DP5_SE, store_states=False)
    rho0 = torch.zeros(1, 16, dtype=torch.complex128, device=dev)
    rho0[0, 0] = 1.0
    d_det2 = torch.ones(1, *det.shape, dtype=torch.float64, device=dev)
    spec.dm = DensityMatrixObservables(n, purity=True, rdms=[ReducedDensityMatrix([0])])
    with pytest.raises(NotImplementedError, match="reduced density"):
        evolve_tangent(amp, det, u, tsave, rho0, spec, None, d_det=d_det2, flags=BOTH)
    spec.dm = DensityMatrixObservables(n, purity=True)
    spec.shots = ShotRequest(4)
    with pytest.raises(NotImplementedError, match="shots"):
        evolve_tangent(amp, det, u, tsave, rho0, spec, None, d_det=d_det2, flags=BOTH)
    spec.shots = None
    with pytest.raises(NotImplementedError, match="TANGENT_DENSITY_MATRIX"):  # not asked for: refused as it always was
        evolve_tangent(amp, det, u, tsave, rho0, spec, None, d_det=d_det2)
    with pytest.raises(NotImplementedError, match="density-matrix"):
        evolve_geometry(amp, det, u, tsave, rho0, spec, None, d_det=d_det2)
    # the C ABI itself, past the Python-side checks: RYDIFF_ENOTIMPL -> NotImplementedError, from validation (a workspace of 0 bytes: a call that passes every check stops at the host-side size test)
    import ctypes

    from pulser_diff_amd.solver import _Call

    def abi(mutate, geometry=False, flags=BOTH):
        call = _Call(spec, amp, det, u, tsave.numpy(), 1, None)
        mutate(call.problem)
        info = _native.RydPlanInfo()
        info.spectral_lo, info.spectral_hi = -1.0, 1.0
        tg = _native.RydTangent()
        tg.n_dir, tg.d_det, tg.flags = 1, d_det2.data_ptr(), flags
        L = _native.lib()
        if geometry:
            rc = L.rydiff_forward_geometry(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(rho0.data_ptr()),
                                           None, None, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
        else:
            rc = L.rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(rho0.data_ptr()),
                                          None, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
        _native.check(rc)

    with pytest.raises(NotImplementedError, match="n_dm_rdms"):
        abi(lambda p: setattr(p, "n_dm_rdms", 1))
    with pytest.raises(NotImplementedError, match="shots"):
        abi(lambda p: setattr(p, "n_shots", 4))
    with pytest.raises(NotImplementedError, match="dm_atoms"):
        abi(lambda p: None, geometry=True)
    with pytest.raises(NotImplementedError, match="conditioned"):
        abi(lambda p: setattr(p, "amp_conditioned_terms", 1))
    with pytest.raises(NotImplementedError, match="shard"):
        abi(lambda p: setattr(p, "shard_bits", 1))
    with pytest.raises(MemoryError, match="workspace too small"):  # a density-matrix problem is a valid one where it is asked for
        abi(lambda p: None)
    with pytest.raises(NotImplementedError, match="RYDIFF_TANGENT_DENSITY_MATRIX"):
        abi(lambda p: None, flags=0)
    with pytest.raises(ValueError, match="flags"):
        abi(lambda p: None, flags=64)
