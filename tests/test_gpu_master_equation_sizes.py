"""Master equation (SolverType.DP5_ME) at every register size the library takes, on every kernel family that applies the
dissipator blocks, and under dissipation strong enough to dominate the generator's spectral width.

The density matrix is the state of a doubled register (pulser_diff_amd/lindblad.py); the dissipator of atom j is one dense 4x4
pair term on (row qubit j, column qubit j).  Which kernels apply those terms depends on the register size:

    atoms 1-3   doubled qubits 2-6    `lanes`       (at most 3 pair terms)
    atoms 4-6   doubled qubits 8-12   `persistent`  (the LDS tile is the whole register)
    atoms 7-12  doubled qubits 14-24  `direct`      (or any size under kernel variant 1)

Every test asserts the family it means to cover, so that a routing change cannot move the coverage elsewhere unnoticed.

References:
  * 1-8 atoms: the oracle's dense Lindblad solution (DOP853) and its differentiable dense Magnus integrator;
  * 9-12 atoms: with u_pairs = 0 and a product initial state, rho(t) is exactly the Kronecker product of the single-atom
    solutions (each atom with its own drive and the same local collapse operators); gradients of an additive observable are the
    sums of the single-atom gradients, and dL/dU_ij at U = 0 comes from the two-atom problem (i, j) alone.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd import lindblad as L
from pulser_diff_amd.lindblad import MAX_ME_QUBITS, mesolve
from pulser_diff_amd.simconfig import SimConfig
from pulser_diff_amd.solver import SolverType
from tests.helpers import random_terms, rel_err, to_native

pytestmark = pytest.mark.gpu

# a collapse operator that is not normal and has all four relative flips non-zero: the pair kernels skip no flip of its block
NON_NORMAL = [[0.2, 1.0], [0.3j, -0.1]]
ALL_FOUR = {"dephasing": 0.9, "relaxation": 0.5, "depolarizing": 0.3, "eff_noise": [(0.6, NON_NORMAL)]}


def _noise_model(noise):
    cfg = SimConfig(noise=tuple(noise), dephasing_rate=noise.get("dephasing", 0.0), relaxation_rate=noise.get("relaxation", 0.0),
                    depolarizing_rate=noise.get("depolarizing", 0.0),
                    eff_noise_rates=tuple(r for r, _ in noise.get("eff_noise", [])),
                    eff_noise_opers=tuple(torch.tensor(o, dtype=torch.complex128) for _, o in noise.get("eff_noise", [])))
    return cfg.to_noise_model()


def _ham_like(terms, device, requires_grad=False, pair_terms=()):
    amp, det, u, spec = to_native(terms, device, SolverType.DP5_SE)
    if requires_grad:
        for t in (amp, det, u):
            t.requires_grad_(True)
    return SimpleNamespace(amp_tables=amp, det_tables=det, u_pairs=u, amp_masks=spec.amp_masks, det_masks=spec.det_masks,
                           dt=terms.dt, n_samples=terms.n_samples, _size=terms.n_qubits, pair_terms=tuple(pair_terms))


def _random_kets(dim, batch, seed):
    psi = torch.randn(dim, batch, generator=torch.Generator().manual_seed(seed), dtype=torch.complex128)
    return psi / psi.norm(dim=0, keepdim=True)


def _fast_H_t(terms):
    """R.dense_hamiltonian(terms, t) with the operator matrices built once (the long strongly dissipative runs call it ~1e5
    times); checked against the oracle's own assembly before use."""
    n = terms.n_qubits
    dim = 2**n
    occ = R.occupation_table(n).numpy()
    base = R.interaction_diagonal(n, terms.u_pairs.detach()).numpy().astype(complex)
    dets = [(c.detach().numpy().astype(float), 2.0 * occ[list(tg)].sum(0)) for c, tg in terms.det_terms()]
    x = np.arange(dim)
    amps = []
    for c, tg in terms.amp_terms():
        low = np.zeros((dim, dim))
        for j in tg:
            m = 1 << (n - 1 - j)
            rows = x[(x & m) != 0]
            low[rows, rows ^ m] = 1.0
        amps.append((c.detach().numpy().astype(complex), low))

    def H_t(t):
        t = float(t)
        i1, i2 = R.interp_indices(t, terms.dt, terms.n_samples)
        f = (t - i1 * terms.dt) / terms.dt
        diag = base.copy()
        for c, o in dets:
            diag = diag + (c[i1] + (c[i2] - c[i1]) * f) * o
        h = np.diag(diag)
        for c, low in amps:
            v = c[i1] + (c[i2] - c[i1]) * f
            h = h + v * low + np.conj(v) * low.T
        return torch.from_numpy(h)

    span = terms.dt * (terms.n_samples - 1)
    for t in (0.0, 0.37 * span, 0.91 * span):
        assert np.abs(H_t(t).numpy() - R.dense_hamiltonian(terms, torch.tensor(t, dtype=torch.float64)).detach().numpy()).max() < 1e-12
    return H_t


def _oracle(terms, noise, psi, tsave, rtol=1e-12, atol=1e-14, H_t=None):
    """Dense Lindblad solution (n_t, dim, dim) from the ket psi (dim,)."""
    rho0 = np.outer(psi.numpy(), psi.numpy().conj())
    return R.lindblad_continuous_solution(terms, R.collapse_operators(terms.n_qubits, noise), rho0, np.asarray(tsave),
                                          rtol=rtol, atol=atol, H_t=H_t or _fast_H_t(terms))


def _assert_physical(rho, eig=True):
    """rho: (n_t, dim, dim) — trace one, Hermitian, positive at every save point."""
    assert np.abs(np.trace(rho, axis1=1, axis2=2) - 1.0).max() < 1e-9
    for r in rho:
        assert np.abs(r - r.conj().T).max() < 1e-9
        if eig:
            assert np.linalg.eigvalsh(0.5 * (r + r.conj().T)).min() > -1e-9


def _report(what, **vals):
    print("ME-SIZES", what, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in vals.items()))


# ----------------------------------------------------------------------------------------------------------------------
# 1. dense-oracle parity per family, 3-7 atoms (8 atoms: test_product_states_... below; its dense solve alone takes minutes)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,noise,family", [
    (3, {"dephasing": 1.1, "relaxation": 0.6}, "lanes"),
    (4, {"dephasing": 1.5}, "persistent"),
    (5, {"relaxation": 0.8, "depolarizing": 0.4}, "persistent"),
    (6, {"eff_noise": [(0.7, NON_NORMAL)]}, "persistent"),
    (7, {"dephasing": 0.9}, "direct"),
])
def test_density_matrices_match_the_dense_solution_on_every_family(cuda_device, n, noise, family):
    """Local channels, a phase drive, irregular save times, two initial kets in one batch; 1e-8 at the default tolerance."""
    terms = random_terms(n, 12, 0.004, seed=700 + n, local=True)
    tsave = torch.tensor([0.0, 0.0057, 0.0173, 0.0311, 0.0436], dtype=torch.float64)
    psi0 = _random_kets(2**n, 2, seed=40 + n)
    rho, stats = mesolve(_ham_like(terms, cuda_device), psi0.to(cuda_device), tsave, _noise_model(noise))
    assert stats["kernel_family"] == family, stats
    got = rho.cpu().numpy()
    H_t = _fast_H_t(terms)
    err = 0.0
    for b in range(2):
        ref = _oracle(terms, noise, psi0[:, b], tsave, H_t=H_t)
        err = max(err, float(np.abs(got[..., b] - ref).max()))
        _assert_physical(got[..., b])
    _report("parity", n=n, family=family, err=err)
    assert err < 1e-8


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact references at the size limit, 8-12 atoms (u_pairs = 0, product initial state)
# ----------------------------------------------------------------------------------------------------------------------
def _product_problem(n, seed, n_samples):
    terms = random_terms(n, n_samples, 0.004, seed=seed, local=True)
    terms.u_pairs = torch.zeros(n * (n - 1) // 2, dtype=torch.float64)
    kets = [_random_kets(2, 1, seed=seed * 100 + j)[:, 0] for j in range(n)]
    psi = functools.reduce(torch.kron, kets)  # qubit 0 is the top index bit
    return terms, kets, psi


def _sub_terms(terms, atoms, amp=None, det=None, u=None):
    """The terms acting on `atoms` (in that order) as a len(atoms)-qubit problem; amp / det: replacement coefficient arrays
    (e.g. autograd leaves), parallel to terms.amp_terms() / terms.det_terms()."""
    amp = amp or [c for c, _ in terms.amp_terms()]
    det = det or [c for c, _ in terms.det_terms()]
    k = len(atoms)
    sub = R.HamTerms(k, u if u is not None else torch.zeros(k * (k - 1) // 2, dtype=torch.float64), None, None, terms.dt,
                     terms.n_samples)
    sub.extra_amp = [(c, [i for i, q in enumerate(atoms) if q in tg]) for c, (_, tg) in zip(amp, terms.amp_terms())
                     if any(q in tg for q in atoms)]
    sub.extra_det = [(c, [i for i, q in enumerate(atoms) if q in tg]) for c, (_, tg) in zip(det, terms.det_terms())
                     if any(q in tg for q in atoms)]
    return sub


@pytest.mark.parametrize("n", [8, 9, MAX_ME_QUBITS])
def test_product_states_at_the_size_limit_match_the_kronecker_product(cuda_device, n):
    terms, kets, psi = _product_problem(n, seed=900 + n, n_samples=10)
    tsave = torch.tensor([0.0, 0.0133, 0.0291] if n > 10 else [0.0, 0.0061, 0.0187, 0.0342], dtype=torch.float64)
    rho, stats = mesolve(_ham_like(terms, cuda_device), psi[:, None].to(cuda_device), tsave, _noise_model(ALL_FOUR))
    assert stats["kernel_family"] == "direct", stats
    singles = [_oracle(_sub_terms(terms, [j]), ALL_FOUR, kets[j], tsave) for j in range(n)]
    err = 0.0
    for k in range(len(tsave)):
        got = rho[k, :, :, 0].cpu().numpy()
        ref = functools.reduce(np.kron, [s[k] for s in singles])
        err = max(err, float(np.abs(got - ref).max()))
        assert abs(np.trace(got) - 1.0) < 1e-9
        assert np.abs(got - got.conj().T).max() < 1e-9
        if n <= 8:
            assert np.linalg.eigvalsh(0.5 * (got + got.conj().T)).min() > -1e-9
        del got, ref
    _report("product", n=n, err=err)
    assert err < 1e-8


def _assert_grad(got, ref, bar, name):
    got, ref = np.asarray(got), np.asarray(ref)
    scale = float(np.abs(ref).max())
    big = np.abs(ref) > 1e-6 * scale
    worst = float((np.abs(got - ref)[big] / np.abs(ref)[big]).max()) if big.any() else 0.0
    _report("grad", name=name, rel=rel_err(got, ref), entry=worst)
    assert rel_err(got, ref) < bar, name
    assert worst < 1e-6, name


@pytest.mark.parametrize("n", [9, 10])
def test_gradients_at_the_size_limit_match_the_single_and_two_atom_problems(cuda_device, n):
    terms, kets, psi = _product_problem(n, seed=950 + n, n_samples=9)
    tsave0 = torch.tensor([0.0, 0.0071, 0.0183, 0.0297], dtype=torch.float64)
    w = torch.tensor([0.3, -0.6, 0.9, 1.4], dtype=torch.float64)
    noise = ALL_FOUR
    h_max = 0.0002
    # native
    ham = _ham_like(terms, cuda_device, requires_grad=True)
    ts = tsave0.clone().requires_grad_(True)
    rho, stats = mesolve(ham, psi[:, None].to(cuda_device), ts, _noise_model(noise), options={"tol": 1e-12})
    assert stats["kernel_family"] == "direct", stats
    zd = R.total_magnetization_diag(n).to(cuda_device)
    e = torch.stack([(torch.diagonal(rho[k, :, :, 0]).real * zd).sum() for k in range(len(tsave0))])
    (e * w.to(cuda_device)).sum().backward()
    # single atoms: amplitude / detuning tables and tsave (the loss is a sum of single-atom losses)
    amp = [c.detach().clone().requires_grad_(True) for c, _ in terms.amp_terms()]
    det = [c.detach().clone().requires_grad_(True) for c, _ in terms.det_terms()]
    o_ts = tsave0.clone().requires_grad_(True)
    z1 = R.total_magnetization_diag(1)
    e_ref = torch.zeros(len(tsave0), dtype=torch.float64)
    for j in range(n):
        r = R.lindblad_magnus_dense(_sub_terms(terms, [j], amp, det), R.collapse_operators(1, noise),
                                    torch.outer(kets[j], kets[j].conj()), o_ts, h_max=h_max)
        e_ref = e_ref + (torch.diagonal(r, dim1=1, dim2=2).real * z1[None]).sum(1)
    (e_ref * w).sum().backward()
    assert np.abs(e.detach().cpu().numpy() - e_ref.detach().numpy()).max() < 1e-8
    # pairs: dL/dU_ij at U = 0 involves atoms i and j only
    z2 = R.total_magnetization_diag(2)
    u_ref = np.zeros(n * (n - 1) // 2)
    for k, (i, j) in enumerate(itertools.combinations(range(n), 2)):
        u = torch.zeros(1, dtype=torch.float64, requires_grad=True)
        rho0 = torch.kron(torch.outer(kets[i], kets[i].conj()), torch.outer(kets[j], kets[j].conj()))
        r = R.lindblad_magnus_dense(_sub_terms(terms, [i, j], u=u), R.collapse_operators(2, noise), rho0, tsave0, h_max=h_max)
        ((torch.diagonal(r, dim1=1, dim2=2).real * z2[None]).sum(1) * w).sum().backward()
        u_ref[k] = float(u.grad[0])
    _assert_grad(ham.amp_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c in amp]).numpy(), 1e-7, f"amp n={n}")
    _assert_grad(ham.det_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c in det]).numpy(), 1e-7, f"det n={n}")
    _assert_grad(ham.u_pairs.grad.cpu().numpy(), u_ref, 1e-7, f"u n={n}")
    _assert_grad(ts.grad.numpy(), o_ts.grad.numpy(), 1e-6, f"tsave n={n}")


# ----------------------------------------------------------------------------------------------------------------------
# 3. strong dissipation and realistic durations, 1-4 atoms
# ----------------------------------------------------------------------------------------------------------------------
def _weak_drive_terms(n, duration, seed, dt=0.004):
    """Omega <= 1 rad/us with a stretch of exactly zero amplitude, a slow detuning, atoms 10 um apart: the dissipators dominate
    the spectral width."""
    g = torch.Generator().manual_seed(seed)
    ns = int(round(duration / dt)) + 1
    t = torch.arange(ns, dtype=torch.float64) * dt
    amp = torch.sin(np.pi * t / duration) ** 2
    amp[(t > 0.3 * duration) & (t < 0.45 * duration)] = 0.0
    amp_c = 0.5 * amp * torch.exp(-1j * (0.4 + 0.3 * t / duration).to(torch.complex128))
    det_c = -0.5 * 0.8 * torch.cos(3.0 * t + float(torch.rand(1, generator=g)))
    coords = torch.stack([torch.arange(n, dtype=torch.float64) * 10.0, torch.rand(n, generator=g, dtype=torch.float64)], dim=1)
    u = R.interaction_strengths(coords) if n > 1 else torch.zeros(0, dtype=torch.float64)
    return R.HamTerms(n, u, amp_c, det_c, dt, ns, list(range(n)), list(range(n)))


def _strong_case(kind, gamma):
    return {"dephasing": {"dephasing": gamma}, "relaxation": {"relaxation": gamma}, "depolarizing": {"depolarizing": gamma},
            "eff_noise": {"eff_noise": [(gamma, NON_NORMAL)]}}[kind]


# (noise type, rate /us, atoms, duration us): every rate for every noise type, atoms and durations spread over the grid
STRONG = [(kind, gamma, 1 + (a + b) % 4, 3.0 if gamma <= 5.0 and (a + b) % 2 == 0 else 1.0)
          for a, kind in enumerate(("dephasing", "relaxation", "depolarizing", "eff_noise"))
          for b, gamma in enumerate((0.5, 5.0, 20.0, 50.0))]


@pytest.mark.parametrize("kind,gamma,n,duration", STRONG)
def test_strong_dissipation_over_realistic_durations(cuda_device, kind, gamma, n, duration):
    noise = _strong_case(kind, gamma)
    terms = _weak_drive_terms(n, duration, seed=int(10 * gamma) + n)
    tsave = torch.tensor([0.0, 0.0173, 0.11, 0.437, 0.71 * duration, duration - 0.0021, duration], dtype=torch.float64)
    psi0 = _random_kets(2**n, 1, seed=int(gamma) + 7 * n)
    # the oracle below rtol 1e-12: at 50 /us DOP853 at rtol 1e-12 is itself off by ~2e-10
    ref = _oracle(terms, noise, psi0[:, 0], tsave, rtol=1e-13, atol=1e-16)
    errs = {}
    for tol in (None, 1e-12):
        rho, stats = mesolve(_ham_like(terms, cuda_device), psi0.to(cuda_device), tsave, _noise_model(noise),
                             options=None if tol is None else {"tol": tol})
        assert stats["kernel_family"] == ("lanes" if n <= 3 else "persistent"), stats
        got = rho[..., 0].cpu().numpy()
        _assert_physical(got)
        errs[tol] = float(np.abs(got - ref).max())
    _report("strong", kind=kind, gamma=gamma, n=n, T=duration, err_default=errs[None], err_tight=errs[1e-12])
    assert errs[None] < 1e-8
    # a tighter tolerance is no worse (below ~5e-11 both sit at the oracle's own accuracy)
    assert errs[1e-12] <= max(errs[None], 5e-11)


def _xy_problem(n, hermitian, monkeypatch, device):
    """n atoms, a microwave (XY) global channel and a magnetic field: the emulator's tables and XY pair terms, and the oracle's
    literal dense generator (hamiltonian.py:346-366, :536) — plus the adjoint of its exchange part for the Hermitian form."""
    import pulser_diff_amd as P
    from pulser_diff_amd import pulses as pl
    from pulser_diff_amd.hamiltonian import Hamiltonian

    monkeypatch.setattr(Hamiltonian, "XY_HERMITIAN", hermitian)
    monkeypatch.setattr(Hamiltonian, "_warned_xy", True)
    coords = [[0.0, 0.0], [6.5, 1.0], [2.0, 7.0], [8.5, 8.0], [13.0, 2.5]][:n]
    seq = pl.Sequence(pl.Register.from_coordinates(coords), pl.MockDevice)
    seq.declare_channel("g", "mw_global")
    seq.set_magnetic_field(0.0, 1.0, 0.3)
    seq.add(pl.Pulse(pl.BlackmanWaveform(120, 2.1), pl.RampWaveform(120, -4.0, 3.0), 0.4), "g")
    seq.add(pl.Pulse.ConstantPulse(80, 3.0, 1.5, -0.2), "g")
    sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.5, evaluation_times=[0.05, 0.12, 0.2], compute_device=device)
    ham = sim._hamiltonian
    assert ham.basis_name == "XY" and len(ham.pair_terms) == n * (n - 1) // 2
    # the oracle's tables from the sequence's raw per-ns samples (+ the trailing sample of backend.py:113-115)
    raw = pl.sample(seq).samples_list[0]
    zero = torch.zeros(1, dtype=torch.float64)
    n_full = raw.amp.numel() + 1
    c = 0.5 * torch.cat([raw.amp, zero]) * torch.exp(-1j * torch.cat([raw.phase, raw.phase[-1:]]).to(torch.complex128))
    d = -0.5 * torch.cat([raw.det, zero])
    c, d, dt, n_s = R.adapt_to_sampling_rate(c, 0.5, n_full), R.adapt_to_sampling_rate(d, 0.5, n_full), 0.002, int(0.5 * n_full)
    xyz = torch.tensor(coords, dtype=torch.float64)
    atoms = list(range(n))
    H_lit = R.reference_style_dense_H_t(xyz, [(c, atoms)], [(d, atoms)], dt, n_s, "XY", magnetic_field=(0.0, 1.0, 0.3))
    H_t = H_lit
    if hermitian:
        H_int = R.reference_style_dense_H_t(xyz, [(torch.zeros_like(c), atoms)], [], dt, n_s, "XY", magnetic_field=(0.0, 1.0, 0.3))
        H_t = lambda t: H_lit(t) + H_int(t).mH  # noqa: E731
    terms = R.HamTerms(n, torch.zeros(n * (n - 1) // 2, dtype=torch.float64), None, None, ham.dt, ham.n_samples)
    return sim, ham, terms, H_t


@pytest.mark.parametrize("hermitian", [False, True])
@pytest.mark.parametrize("n,noise", [
    (4, {"depolarizing": 5.0}),
    (5, {"dephasing": 2.0, "eff_noise": [(3.0, NON_NORMAL)]}),
])
def test_xy_exchange_with_dissipators_on_the_persistent_kernels(cuda_device, monkeypatch, n, noise, hermitian):
    """4 atoms: 4 dissipator + 12 exchange pair terms; 5 atoms: 5 + 20 = 25 of the 28 the library takes."""
    sim, ham, terms, H_t = _xy_problem(n, hermitian, monkeypatch, "cuda")
    assert len(L.doubled_pair_terms(ham.pair_terms, n, L.dissipator_block(L.local_collapse_operators(_noise_model(noise), "XY")))) \
        == n + n * (n - 1)
    psi0 = _random_kets(2**n, 1, seed=60 + n)
    ts = sim.evaluation_times.detach().cpu()
    rho, stats = mesolve(ham, psi0.to(cuda_device), ts, _noise_model(noise))
    assert stats["kernel_family"] == "persistent", stats
    got = rho[..., 0].cpu().numpy()
    ref = R.lindblad_continuous_solution(terms, R.collapse_operators(n, noise), np.outer(psi0[:, 0].numpy(), psi0[:, 0].numpy().conj()),
                                         ts.numpy(), H_t=H_t)
    err = float(np.abs(got - ref).max())
    _report("xy", n=n, hermitian=hermitian, err=err)
    assert err < 1e-8
    if hermitian:  # the literal (one-directional) exchange does not conserve the trace
        _assert_physical(got)


def test_xy_with_dissipators_beyond_the_pair_term_budget_is_refused_before_launch(cuda_device, monkeypatch):
    """6 atoms: 6 dissipator + 30 exchange pair terms > 28 — NotImplementedError from doubled_pair_terms, nothing launched."""
    import pulser_diff_amd as P
    from pulser_diff_amd import pulses as pl
    from pulser_diff_amd.hamiltonian import Hamiltonian

    monkeypatch.setattr(Hamiltonian, "XY_HERMITIAN", True)

    coords = [[0.0, 0.0], [6.5, 1.0], [2.0, 7.0], [8.5, 8.0], [13.0, 2.5], [4.0, 14.0]]
    seq = pl.Sequence(pl.Register.from_coordinates(coords), pl.MockDevice)
    seq.declare_channel("g", "mw_global")
    seq.set_magnetic_field(0.0, 1.0, 0.3)
    seq.add(pl.Pulse(pl.BlackmanWaveform(120, 2.1), pl.RampWaveform(120, -4.0, 3.0), 0.4), "g")
    ham6 = P.TorchEmulator.from_sequence(seq, sampling_rate=0.5, compute_device="cuda")._hamiltonian
    assert len(ham6.pair_terms) == 15

    def no_launch(*a, **k):
        raise AssertionError("the solver was launched")

    monkeypatch.setattr(L, "evolve", no_launch)
    with pytest.raises(NotImplementedError, match="needs 36 dense two-qubit terms"):
        mesolve(ham6, R.all_ground_state(6).to(cuda_device), torch.tensor([0.0, 0.1], dtype=torch.float64),
                _noise_model({"dephasing": 1.0}))


# ----------------------------------------------------------------------------------------------------------------------
# 4. gradients: dense autograd at 3-4 atoms, direct against persistent at 5-6 atoms
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,family", [(3, "lanes"), (4, "persistent")])
def test_gradients_with_non_normal_noise_match_dense_autograd(cuda_device, n, family):
    terms = random_terms(n, 8, 0.004, seed=810 + n, local=True)
    noise = {"depolarizing": 0.8, "eff_noise": [(0.6, NON_NORMAL)]}
    tsave0 = torch.tensor([0.0, 0.0067, 0.0158, 0.0243], dtype=torch.float64)
    w = torch.tensor([0.4, -0.7, 0.5, 1.1], dtype=torch.float64)
    psi0 = _random_kets(2**n, 1, seed=820 + n)
    zd = R.total_magnetization_diag(n)
    o = R.HamTerms(n, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                   terms.det_coeff.clone().requires_grad_(True), terms.dt, terms.n_samples, terms.amp_targets, terms.det_targets)
    o.extra_amp = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_amp]
    o.extra_det = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_det]
    o_ts = tsave0.clone().requires_grad_(True)
    o_rho = R.lindblad_magnus_dense(o, R.collapse_operators(n, noise), torch.outer(psi0[:, 0], psi0[:, 0].conj()), o_ts,
                                    h_max=0.0002 if n < 4 else 0.0004)
    o_e = (torch.diagonal(o_rho, dim1=1, dim2=2).real * zd[None]).sum(1)
    (o_e * w).sum().backward()
    ham = _ham_like(terms, cuda_device, requires_grad=True)
    ts = tsave0.clone().requires_grad_(True)
    rho, stats = mesolve(ham, psi0.to(cuda_device), ts, _noise_model(noise), options={"tol": 1e-12})
    assert stats["kernel_family"] == family, stats
    e = (torch.diagonal(rho[..., 0], dim1=1, dim2=2).real * zd.to(cuda_device)[None]).sum(1)
    (e * w.to(cuda_device)).sum().backward()
    _assert_physical(rho[..., 0].detach().cpu().numpy())
    assert np.abs(e.detach().cpu().numpy() - o_e.detach().numpy()).max() < 1e-8
    _assert_grad(ham.amp_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c, _ in o.amp_terms()]).numpy(), 1e-7, f"amp n={n}")
    _assert_grad(ham.det_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c, _ in o.det_terms()]).numpy(), 1e-7, f"det n={n}")
    _assert_grad(ham.u_pairs.grad.cpu().numpy(), o.u_pairs.grad.numpy(), 1e-7, f"u n={n}")
    _assert_grad(ts.grad.numpy(), o_ts.grad.numpy(), 1e-6, f"tsave n={n}")


@pytest.mark.parametrize("n", [5, 6])
def test_direct_and_persistent_pair_kernels_agree_at_five_and_six_atoms(cuda_device, n):
    terms = random_terms(n, 13, 0.004, seed=860 + n, local=True)
    noise = {"depolarizing": 0.9, "eff_noise": [(0.5, NON_NORMAL)]}
    tsave0 = torch.tensor([0.0, 0.0093, 0.027, 0.041], dtype=torch.float64)
    psi0 = _random_kets(2**n, 2, seed=870 + n)
    out = {}
    for variant, family in ((1, "direct"), (0, "persistent")):
        _native.set_kernel_variant(variant)
        try:
            ham = _ham_like(terms, cuda_device, requires_grad=True)
            ts = tsave0.clone().requires_grad_(True)
            rho, stats = mesolve(ham, psi0.to(cuda_device), ts, _noise_model(noise))
            assert stats["kernel_family"] == family, stats
            obs = torch.linspace(-1, 1, 2**n, device=cuda_device, dtype=torch.float64)
            (torch.diagonal(rho, dim1=1, dim2=2).real * obs).sum().backward()
            out[variant] = [rho.detach().cpu().numpy(), ham.amp_tables.grad.cpu().numpy(), ham.det_tables.grad.cpu().numpy(),
                            ham.u_pairs.grad.cpu().numpy(), ts.grad.numpy()]
        finally:
            _native.set_kernel_variant(0)
    for name, ref, got in zip(("rho", "amp", "det", "u", "tsave"), out[1], out[0]):
        assert rel_err(got, ref) < 1e-10, name
