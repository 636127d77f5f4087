"""Native observables of master-equation runs (RydProblem.dm_*; csrc/dm_kernels.hpp): Tr(rho O) for diagonal tables and Pauli strings,
fidelities <phi|rho|phi>, the purity and measurement shots, evaluated while rho is on the device — no stored (n_t, 4^n) trajectory —
and differentiated through the grad_states route.

Kernel families (asserted from the plan, so a case cannot silently run elsewhere): 2 / 3 atoms = 4 / 6 doubled qubits on the one-wave
lane sweep, 4 atoms = 8 qubits on the one-workgroup persistent sweep, 7 atoms = 14 qubits on the direct kernels (one launch per
factor; the register is four times the 2^12-amplitude tile, the cotangent kernels run on more than one block per row).

References: dense numpy on the very vector the library was handed (the definitions, 1e-12 relative to the largest entry of a row
kind: sums of at most 4^7 products of O(1) doubles), the oracle's dense Lindblad solution (1e-8, the bar of
tests/test_gpu_master_equation_sizes.py for rho) and its differentiable dense Magnus integrator (1e-7, tsave 1e-6: the bars of
test_gradients_with_non_normal_noise_match_dense_autograd), and the stored-rho route of the same build (1e-10, the suite's bar
between two native routes)."""
import functools

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import pulses as pl
from pulser_diff_amd import solver as S
from pulser_diff_amd.lindblad import mesolve
from pulser_diff_amd.observables import DensityMatrixObservables, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap
from pulser_diff_amd.shots import SHOT_NONE, ShotRequest, sample_indices_reference
from pulser_diff_amd.solver import SolverType, evolve, evolve_tangent
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import random_terms, rel_err, to_native
from tests.test_gpu_master_equation_sizes import NON_NORMAL, _fast_H_t, _ham_like, _noise_model, _oracle, _random_kets
from tests.test_gpu_workspace_contents import _filled

pytestmark = pytest.mark.gpu

FAMILY = {2: "lanes", 3: "lanes", 4: "persistent", 7: "direct"}
DEF_RTOL = 1e-12
ROUTE_RTOL = 1e-10


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


def _paulis(n):
    """Two observables; Y on several atoms, four distinct flip masks in the first, one of them shared with the second (the cotangent
    scatter then has one owner per entry only because it groups over ALL observables)."""
    a, z = 0, n - 1
    first = PauliObservable(n, [(0.7, {a: "Y", z: "Y"}), (-1.1, {a: "X", z: "Y"}), (0.4, {a: "Z"}), (0.9, {z: "Y"}), (-0.6, {a: "Y"}),
                                (0.3, {a: "Y", z: "Z"})])
    second = PauliObservable(n, [(1.3, {a: "Z", z: "Z"}), (-0.8, {a: "X"}), (0.5, {a: "Y", z: "X"})])
    return [first, second]


def _definitions(v, diag, paulis, targets, n):
    """Every row of one vector v = vec(rho) (4^n,) in dense numpy; targets: (n_fid, 2^n)."""
    dim = 2 ** n
    rho = v.reshape(dim, dim)
    rows = [float((d * np.real(np.diagonal(rho))).sum()) for d in diag]
    rows += [float(np.trace(o.to_dense().numpy() @ rho).real) for o in paulis]
    rows += [float((t.conj() @ rho @ t).real) for t in targets]
    rows.append(float((np.abs(v) ** 2).sum()))
    return np.asarray(rows)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the definitions, on a deliberately non-Hermitian vector, at every save point of a short run
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid_batch", [1, 2])
@pytest.mark.parametrize("n", [2, 4, 7])
def test_every_row_kind_matches_dense_numpy(cuda_device, n, fid_batch):
    """psi0 is a random complex vector of length 4^n: a dropped imaginary part or a transposed index shows.  Save point 0 is psi0
    itself; the later ones are checked on the states the same call stored."""
    dim, batch = 2 ** n, 2
    gen = torch.Generator().manual_seed(5000 + n)
    terms = random_terms(2 * n, 9, 0.002, seed=5100 + n, local=True)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=True)
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    diag = _randn(gen, 2, dim)
    targets = _randn(gen, 3, fid_batch, dim, cplx=True)  # three targets: the four-target instantiation with one slot idle
    paulis = _paulis(n)
    spec.dm = DensityMatrixObservables(n, diag=diag.to(cuda_device), pauli=paulis, targets=targets.to(cuda_device), purity=True)
    tsave = torch.tensor([0.0, 0.0037, 0.0091], dtype=torch.float64)
    states, expect = evolve(amp, det, u, tsave, v0.to(cuda_device), spec, None)
    torch.cuda.synchronize()
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n], spec.options["_last_stats"]
    assert expect.shape == (2 + 2 + 3 + 1, 3, batch)
    got = expect.cpu().numpy()
    st = states.cpu().numpy()
    assert np.array_equal(st[0], v0.numpy())
    want = np.zeros_like(got)
    for k in range(3):
        for b in range(batch):
            want[:, k, b] = _definitions(st[k, b], diag.numpy(), paulis, targets[:, b if fid_batch > 1 else 0].numpy(), n)
    for name, sl in (("diag", slice(0, 2)), ("pauli", slice(2, 4)), ("fidelity", slice(4, 7)), ("purity", slice(7, 8))):
        for k in range(3):
            err = rel_err(got[sl, k], want[sl, k])
            print(f"DM-DEF n={n} fid_batch={fid_batch} {name} k={k}: {err:.2e}")
            assert err < DEF_RTOL, (name, k)


# ----------------------------------------------------------------------------------------------------------------------
# 2. end to end against the dense Lindblad solution, without stored states
# ----------------------------------------------------------------------------------------------------------------------
# irregular save times across the sample grid (dt = 0.004); 7 atoms: a shorter run of one ket — the dense 128 x 128 solve of the
# oracle is what takes the time
ME_TSAVE = {3: (0.0, 0.0057, 0.0173, 0.0311, 0.0436), 4: (0.0, 0.0057, 0.0173, 0.0311, 0.0436), 7: (0.0, 0.0031, 0.0087, 0.0149)}
ME_BATCH = {3: 2, 4: 2, 7: 1}
ME_NOISE = {3: {"dephasing": 1.1, "relaxation": 0.6}, 4: {"dephasing": 1.5}, 7: {"dephasing": 0.9}}


def _me_observables(n, gen, batch):
    dim = 2 ** n
    target = _randn(gen, dim, batch, cplx=True)
    target = target / target.norm(dim=0, keepdim=True)
    zsum = DiagonalObservable(total_magnetization_diag(n) / n)
    other = torch.linspace(-1.0, 1.0, dim, dtype=torch.float64)
    return [zsum, other] + _paulis(n) + [StateOverlap(target), StateOverlap(target[:, 0].flip(0).clone()), Purity()]


def _torch_rows(rho, obs_list):
    """The rows of `obs_list` on density matrices rho (n_t, dim, dim, B) in torch: the stored-rho route / the dense oracle."""
    out = []
    for obs in obs_list:
        if isinstance(obs, Purity):
            out.append((rho.real ** 2 + rho.imag ** 2).sum(dim=(1, 2)))
        elif isinstance(obs, StateOverlap):
            phi = obs.targets.to(rho.device).expand(-1, rho.shape[3])
            out.append(torch.einsum("xb,txyb,yb->tb", phi.conj(), rho, phi).real)
        elif isinstance(obs, PauliObservable):
            out.append(torch.einsum("xy,tyxb->tb", obs.to_dense().to(rho.device), rho).real)
        else:
            d = (obs.diag if isinstance(obs, DiagonalObservable) else obs).to(rho.device)
            out.append(torch.einsum("x,txxb->tb", d.to(torch.complex128), rho).real)
    return out


@functools.lru_cache(maxsize=None)
def _me_reference(n):
    """(terms, psi0 (dim, B), dense solution (n_t, dim, dim, B)) — computed once, shared, never modified."""
    terms = random_terms(n, 12, 0.004, seed=700 + n, local=True)
    psi0 = _random_kets(2 ** n, ME_BATCH[n], seed=40 + n)
    H_t = _fast_H_t(terms)
    ref = np.stack([_oracle(terms, ME_NOISE[n], psi0[:, b], torch.tensor(ME_TSAVE[n], dtype=torch.float64), H_t=H_t)
                    for b in range(ME_BATCH[n])], axis=-1)
    return terms, psi0, torch.from_numpy(ref)


@pytest.mark.parametrize("n", [3, 4, 7])
def test_native_rows_match_the_dense_lindblad_solution_without_stored_states(cuda_device, n):
    terms, psi0, ref = _me_reference(n)
    obs = _me_observables(n, torch.Generator().manual_seed(5200 + n), ME_BATCH[n])
    res = mesolve(_ham_like(terms, cuda_device), psi0.to(cuda_device), torch.tensor(ME_TSAVE[n], dtype=torch.float64), _noise_model(ME_NOISE[n]),
                  observables=obs, store_states=False)
    assert res.stats["kernel_family"] == FAMILY[n], res.stats
    assert res.states.numel() == 0 and res.states.shape[0] == 0
    rho, stats = res  # (still unpacks like the pair it used to be)
    assert rho is res.states and stats is res.stats
    want = _torch_rows(ref, obs)
    assert len(res.expect) == len(obs)
    for o, g, w in zip(obs, res.expect, want):
        assert g.shape == (len(ME_TSAVE[n]), ME_BATCH[n])
        err = float((g.cpu() - w).abs().max())
        print(f"DM-ME n={n} {type(o).__name__}: {err:.2e}")
        assert err < 1e-8, type(o).__name__


# ----------------------------------------------------------------------------------------------------------------------
# 3. gradients
# ----------------------------------------------------------------------------------------------------------------------
def _loss(rows, weights):
    return sum((r * w.to(r.device)).sum() for r, w in zip(rows, weights))


@pytest.mark.parametrize("n", [3, 4])
def test_gradients_of_all_row_kinds_match_dense_autograd(cuda_device, n):
    """A loss over all four differentiable row kinds and all save points, non-normal noise, against autograd through the oracle's
    dense Magnus integrator: amp, det, u_pairs and tsave."""
    terms = random_terms(n, 8, 0.004, seed=810 + n, local=True)
    noise = {"depolarizing": 0.8, "eff_noise": [(0.6, NON_NORMAL)]}
    tsave0 = torch.tensor([0.0, 0.0067, 0.0158, 0.0243], dtype=torch.float64)
    psi0 = _random_kets(2 ** n, 1, seed=820 + n)
    gen = torch.Generator().manual_seed(5300 + n)
    obs = _me_observables(n, gen, 1)
    weights = [_randn(gen, 4, 1) for _ in obs]
    o = R.HamTerms(n, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                   terms.det_coeff.clone().requires_grad_(True), terms.dt, terms.n_samples, terms.amp_targets, terms.det_targets)
    o.extra_amp = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_amp]
    o.extra_det = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_det]
    o_ts = tsave0.clone().requires_grad_(True)
    o_rho = R.lindblad_magnus_dense(o, R.collapse_operators(n, noise), torch.outer(psi0[:, 0], psi0[:, 0].conj()), o_ts,
                                    h_max=0.0002 if n < 4 else 0.0004)
    o_rows = _torch_rows(o_rho[..., None], obs)
    _loss(o_rows, weights).backward()

    ham = _ham_like(terms, cuda_device, requires_grad=True)
    ts = tsave0.clone().requires_grad_(True)
    res = mesolve(ham, psi0.to(cuda_device), ts, _noise_model(noise), options={"tol": 1e-12}, observables=obs, store_states=False)
    assert res.stats["kernel_family"] == FAMILY[n] and res.states.numel() == 0, res.stats
    _loss(res.expect, weights).backward()
    for ob, g, w in zip(obs, res.expect, o_rows):
        assert float((g.detach().cpu() - w.detach()).abs().max()) < 1e-8, type(ob).__name__
    pairs = (("amp", ham.amp_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c, _ in o.amp_terms()]).numpy(), 1e-7),
             ("det", ham.det_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c, _ in o.det_terms()]).numpy(), 1e-7),
             ("u", ham.u_pairs.grad.cpu().numpy(), o.u_pairs.grad.numpy(), 1e-7),
             ("tsave", ts.grad.numpy(), o_ts.grad.numpy(), 1e-6))
    for name, got, want, bar in pairs:
        err = rel_err(got, want)
        print(f"DM-GRAD n={n} {name}: {err:.2e}")
        assert err < bar, name


def _route(n, dev, native, batch=2, seed=860):
    """Loss and gradients through the native rows (no stored states) or through stored rho and torch autograd."""
    terms = random_terms(n, 12, 0.004, seed=seed + n, local=True)
    noise = {"depolarizing": 0.9, "eff_noise": [(0.5, NON_NORMAL)]}
    psi0 = _random_kets(2 ** n, batch, seed=seed + 10 + n)
    gen = torch.Generator().manual_seed(seed + 20 + n)
    obs = _me_observables(n, gen, batch)
    weights = [_randn(gen, 4, batch) for _ in obs]
    ham = _ham_like(terms, dev, requires_grad=True)
    ts = torch.tensor([0.0, 0.0093, 0.027, 0.041], dtype=torch.float64, requires_grad=True)
    if native:
        res = mesolve(ham, psi0.to(dev), ts, _noise_model(noise), observables=obs, store_states=False)
        assert res.states.numel() == 0
        rows = res.expect
    else:
        res = mesolve(ham, psi0.to(dev), ts, _noise_model(noise))
        rows = _torch_rows(res.states, obs)
    assert res.stats["kernel_family"] == FAMILY[n], res.stats
    loss = _loss(rows, weights)
    loss.backward()
    torch.cuda.synchronize()
    return {"rows": torch.stack([r.detach() for r in rows]).cpu().numpy(), "amp": ham.amp_tables.grad.cpu().numpy(),
            "det": ham.det_tables.grad.cpu().numpy(), "u": ham.u_pairs.grad.cpu().numpy(), "tsave": ts.grad.numpy()}


def test_gradients_at_seven_atoms_agree_with_the_stored_rho_route(cuda_device):
    """14 doubled qubits on the direct kernels: the register is four tiles and k_dm_apply runs many blocks per trajectory (k_dm_scatter
    still has one block per flip mask at 2^7 = 128 entries; tests/test_gpu_dm_observables_wide.py takes it past one block)."""
    got, want = _route(7, cuda_device, True), _route(7, cuda_device, False)
    for key in want:
        err = rel_err(got[key], want[key])
        print(f"DM-ROUTES n=7 {key}: {err:.2e}")
        assert err < ROUTE_RTOL, key


@pytest.mark.parametrize("n", [3, 4, 7])
def test_a_poisoned_workspace_changes_nothing(cuda_device, monkeypatch, n):
    """Every workspace filled with quiet NaNs against zero-filled ones (tests/test_gpu_workspace_contents.py): the scratch trajectory,
    the string tables and the cotangent buffer are written before they are read."""
    out = {}
    for name, value in (("zeros", 0.0), ("nans", float("nan"))):
        monkeypatch.setattr(S, "_new_workspace", _filled(value))
        out[name] = _route(n, cuda_device, True, seed=900)
    for key in out["zeros"]:
        assert np.isfinite(out["nans"][key]).all(), f"{key}: a region is read before it is written"
        assert rel_err(out["nans"][key], out["zeros"][key]) < 1e-12, key


# ----------------------------------------------------------------------------------------------------------------------
# 4. shots
# ----------------------------------------------------------------------------------------------------------------------
N_SHOTS = 4096


def _shot_run(n, dev, v0, uniforms):
    terms = random_terms(2 * n, 9, 0.002, seed=5100 + n, local=True)
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=True)
    spec.dm = DensityMatrixObservables(n, shots=True)
    spec.shots = ShotRequest(N_SHOTS, times=[0, 2], uniforms=uniforms)
    states, _ = evolve(amp, det, u, torch.tensor([0.0, 0.0037, 0.0091], dtype=torch.float64), v0.to(dev), spec, None)
    torch.cuda.synchronize()
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n]
    return states.cpu().numpy(), spec.shots.indices.cpu().numpy()


def _clamped_diagonal(v, n):
    dim = 2 ** n
    return np.maximum(v.reshape(*v.shape[:-1], dim, dim)[..., np.arange(dim), np.arange(dim)].real, 0.0)


@pytest.mark.parametrize("n", [2, 4, 7])
def test_shots_follow_the_rule_on_the_stored_density_matrix(cuda_device, n):
    dim, batch = 2 ** n, 2
    gen = torch.Generator().manual_seed(1000 + n)
    v0 = _randn(gen, batch, dim * dim, cplx=True)  # about half of the diagonal is negative: clamped to zero
    zero_at = np.arange(0, dim, 3)
    for x in zero_at:
        v0[:, x * (dim + 1)] = complex(0.0, 1.0)  # exact zeros on the diagonal (the imaginary part plays no part)
    uniforms = torch.rand(2, batch, N_SHOTS, generator=gen, dtype=torch.float64)
    uniforms[:, :, 0] = 0.0
    uniforms[:, :, 1] = 1.0 - 2.0 ** -53
    states, got = _shot_run(n, cuda_device, v0, uniforms)
    assert got.shape == (2, batch, N_SHOTS)
    left_out = 0
    for si, k in enumerate((0, 2)):
        p = _clamped_diagonal(states[k], n)  # (B, dim)
        want = sample_indices_reference(p, uniforms[si].numpy())
        for b in range(batch):
            cum = np.cumsum(p[b])
            near = np.abs(uniforms[si, b].numpy()[:, None] * cum[-1] - cum[None, :]).min(axis=1) <= 1e-12 * cum[-1]
            left_out += int(near.sum())
            assert (got[si, b][~near] == want[b][~near]).all(), (k, b, np.flatnonzero(got[si, b] != want[b])[:8])
            assert (p[b][got[si, b]] > 0).all()  # never an x with p[x] == 0, boundary shots included
    assert left_out <= 0.01 * got.size, left_out
    assert not np.isin(got[0], zero_at).any()  # exact zeros (and negative entries) of rho(t_0) are never returned
    _, again = _shot_run(n, cuda_device, v0, uniforms)
    assert np.array_equal(got, again)  # bit-reproducible
    _, none = _shot_run(n, cuda_device, torch.zeros_like(v0), uniforms)
    assert (none == SHOT_NONE).all()


# ----------------------------------------------------------------------------------------------------------------------
# 5. the emulator
# ----------------------------------------------------------------------------------------------------------------------
def _emulator(n=3):
    seq = pl.Sequence(pl.Register.rectangle(1, n, spacing=8, prefix="q"), pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(300, 2.4), pl.RampWaveform(300, -3.0, 2.0), 0.2), "g")
    cfg = P.SimConfig(noise=("relaxation", "dephasing"), relaxation_rate=0.5, dephasing_rate=1.0)
    return P.TorchEmulator.from_sequence(seq, config=cfg, evaluation_times=[0.05 * k for k in range(1, 7)])


def test_emulator_serves_native_values_without_stored_states(cuda_device):
    n = 3
    gen = torch.Generator().manual_seed(77)
    target = _randn(gen, 2 ** n, cplx=True)
    zsum = DiagonalObservable(total_magnetization_diag(n))
    xx = PauliObservable(n, [(1.0, {0: "X", 2: "X"}), (0.5, {1: "Y"})])
    fid = StateOverlap(target / target.norm())
    observables = [zsum, xx, fid, Purity()]
    res = _emulator(n).run(observables=observables, store_states=False)
    assert res._states_tbd.numel() == 0
    with pytest.raises(RuntimeError, match="not stored"):
        res.states
    stored = _emulator(n).run()  # the stored-rho route: torch fallbacks of results.expect / fidelity / purity
    assert stored.states.shape == (len(stored), 2 ** n, 2 ** n, 1)
    pairs = (("z", res.expect([zsum])[0], stored.expect([zsum])[0]), ("xx", res.expect([xx])[0], stored.expect([xx])[0]),
             ("fidelity", res.fidelity(fid), stored.fidelity(fid)), ("purity", res.purity(), stored.purity()),
             ("expect(fid)", res.expect([fid])[0], stored.expect([fid])[0]))
    for name, a, b in pairs:
        assert a.shape == b.shape, name
        err = float((a - b).abs().max())
        print(f"DM-EMU {name}: {err:.2e}")
        assert err < ROUTE_RTOL, name
    assert res.fidelity(fid) is res._native_fidelities[0] and res.purity() is res._native_purity
    assert float(res.purity()[0, 0]) > float(res.purity()[-1, 0])  # decoherence


def test_emulator_draws_native_shots_from_rho_without_stored_states(cuda_device):
    res = _emulator(3).run(shots=500, store_states=False)
    counts = res.sample_final_state(500)
    assert sum(counts.values()) == 500 and all(len(k) == 3 for k in counts)
    assert res.native_shots.indices.shape == (1, 1, 500) and int(res.native_shots.indices.max()) < 8


# ----------------------------------------------------------------------------------------------------------------------
# 6. refusals, before anything is launched
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda_device, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("the solver was launched")

    import pulser_diff_amd.lindblad as L

    sim = _emulator(3)
    monkeypatch.setattr(L, "evolve", no_launch)
    with pytest.raises(NotImplementedError, match="ReducedDensityMatrix"):
        sim.run(observables=[ReducedDensityMatrix([0, 1])])
    # with stored density matrices StateOverlap and shots= stay refused (results.fidelity / sample_state read the stored rho)
    with pytest.raises(NotImplementedError, match="store_states=False"):
        sim.run(observables=[StateOverlap(torch.ones(8, dtype=torch.complex128))])
    with pytest.raises(NotImplementedError, match="store_states=False"):
        sim.run(shots=10)
    monkeypatch.undo()
    n = 2
    terms = random_terms(2 * n, 9, 0.002, seed=1, local=True)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
    spec.dm = DensityMatrixObservables(n, purity=True)
    v0 = torch.ones(1, 4 ** n, dtype=torch.complex128, device=cuda_device)
    with pytest.raises(NotImplementedError, match="density-matrix"):
        evolve_tangent(amp, det, u, torch.tensor([0.0, 0.01], dtype=torch.float64), v0, spec, d_u=torch.ones(1, *u.shape, device=cuda_device))


def test_quantum_model_fidelity_takes_the_master_equation_route(cuda_device):
    """QuantumModel.fidelity under collapse-operator noise: <target|rho(t)|target> from the native rows (no stored states), equal to
    the stored-rho fallback of the same run, with a gradient on the pulse parameters."""
    from pulser_diff_amd.utils import basis_state, interpolate_sine

    n, duration, n_param = 2, 120, 4
    seq = pl.Sequence(pl.Register.rectangle(1, n, torch.tensor([7.0])), pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    amp_var = seq.declare_variable("amp", size=duration)
    seq.add(pl.Pulse(pl.CustomWaveform(amp_var), pl.RampWaveform(duration, -2.0, 2.0), 0.0), "g")
    interp = interpolate_sine(n_param, duration)
    torch.manual_seed(3)
    model = P.QuantumModel(seq, {"amp": ((2 * torch.rand(n_param) - 1.0,), lambda p: interp @ (6.0 * torch.sigmoid(p)))},
                           sampling_rate=0.5, noise_config=P.SimConfig(noise="dephasing", dephasing_rate=0.4))
    target = StateOverlap(basis_state(2 ** n, 0).to(torch.complex128))
    times, fid = model.fidelity(target)
    assert fid.shape == (len(times), 1) and not fid.is_complex()
    _, stored = model._run()  # the same master-equation run with stored density matrices
    assert stored.states.ndim == 4
    assert float((fid.detach() - stored.fidelity(target).detach()).abs().max()) < ROUTE_RTOL
    (1 - fid[-1, 0]).backward()
    grads = [p.grad for p in model.parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all() and g.abs().max() > 0 for g in grads)
