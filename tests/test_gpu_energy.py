"""Energy observables on the GPU (RydProblem.energy_rows; csrc/energy_kernels.hpp): the rows E = Re<psi|H_k|psi> and
M2 = |H_k psi|^2 at every evaluation time, their cotangent and the explicit coefficient gradients, through the C ABI
(pulser_diff_amd.solver.evolve).

  1  kernel parity on the call's own states: the rows against the reference H_k (tests/structured_reference.py: structured_matvec)
     applied to the states the same call returns — N = 1, 2, 6, 7, 8, 9, 12, 13, 14, one global drive with a phase plus per-atom drive
     and detuning terms, B = 1 and B = 3 (coeff_batch = B), one and two rows, both solvers, every sweep family that is legal at N
  2  end to end against the dense oracle's trajectory at 4, 8 and 10 qubits
  3  gradients of sum_k (a_k E_k + b_k M2_k): g_amp, g_det, g_u, g_energy_amp, g_energy_det, g_psi0 against autograd through the dense
     map (8 qubits) and through the matrix-free reference (13 qubits); every tape mode, and next to a diagonal row and the moments
  4  the exchange (xy_mode = 1) at N = 3, 9, 13: rows and g_xy with its explicit part; xy_mode = 2 is refused
  5  an eigenstate: M2 - E^2 stays at the cancellation floor
  6  two calls give the same bits (N = 14); zero-filled against NaN-filled workspaces
  7  feature off: the three new pointers are ignored

The energy block has two versions of its kernels, forced through ProblemSpec.energy_kernel (RydProblem.energy_kernel): 1 direct (one
amplitude per thread, every N), 2 LDS-tile (13 .. 24 qubits); 0 takes the one that measured faster.  13 and 14 qubits run every case of
1 with each of them forced and with the automatic choice; 3 and 6 run with the tile version forced as well.

Tolerance of the kernel parity (1, 5): a row is a float64 sum of 2^N products of a matvec with at most N + 1 terms per amplitude on a
state of norm 1: about 50 roundings of 1.1e-16 with a tenfold margin -> 1e-12 R for E and 1e-12 R^2 for M2, R the Gershgorin bound of
H_k computed here from the tables.  Oracle parity (2, 3, 4): the project's bars for expectation rows, 1e-9 for values and 1e-8 for
gradients (tests/test_gpu_pauli_observables.py:23-24), 1e-8 for the exchange (tests/test_gpu_xy_exchange.py).  The 1e-9 is absolute
for E; M2 is a square of size up to R^2 and is held to 1e-9 relative to its own largest entry (never below the absolute 1e-9)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import restatement as R
from pulser_diff_amd import solver as S
from pulser_diff_amd.observables import occupation_moments
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, split_energy, split_moments
from tests import structured_reference as SR
from tests import xy_exchange_reference as XR
from tests.helpers import dense_from_structured_terms, rel_err
from tests.test_gpu_pauli_observables import GRAD_RTOL, VALUE_ATOL  # :24, :23
from tests.test_gpu_workspace_contents import _both_fills, _compare

pytestmark = pytest.mark.gpu

KERNEL_RTOL = 1e-12  # of R (E) and R^2 (M2): see the module docstring
XY_TOL = 1e-8
N_SAMPLES, DT = 6, 0.004
TSAVE = (0.0, 0.0031, 0.0072, 0.0109)  # irregular, off the sample grid, inside the tables
CD, RD = torch.complex128, torch.float64


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=CD if cplx else RD)


def _interp_cols(tab, tsave):
    """tab[..., n_samples] at every evaluation time -> [..., n_t] (tests/structured_reference.py: interp_table, the reference's rule)."""
    return torch.stack([SR.interp_table(tab, t, DT, N_SAMPLES) for t in tsave], dim=-1)


@functools.lru_cache(maxsize=None)
def _problem(n, batch, seed=0):
    """One global drive with a phase, per-atom drives and per-atom detunings; one table set per trajectory (coeff_batch = batch)."""
    gen = torch.Generator().manual_seed(5100 + 17 * n + batch + seed)
    t = torch.linspace(0, 1, N_SAMPLES, dtype=RD)
    amp = [3.0 * torch.sin(np.pi * (0.2 + 0.6 * t)) ** 2 * torch.exp(-1j * (0.7 * t + 0.2).to(CD))]
    amp += [(1.0 + 0.5 * _randn(gen, 1)) * torch.cos(1.5 * t + j).to(CD) * np.exp(-0.3j * (j + 1)) for j in range(n)]
    det = [-0.5 * (2.0 + _randn(gen, 1)) * (2 * t - 0.8 + 0.1 * j) for j in range(n)]
    scale = 1.0 + 0.25 * torch.arange(batch, dtype=RD)
    amp = torch.stack(amp)[None] * scale[:, None, None]
    det = torch.stack(det)[None] * scale[:, None, None]
    coords = torch.stack([torch.arange(n, dtype=RD) * 7.5, torch.rand(n, generator=gen, dtype=RD) * 2.0], dim=1)
    u = R.interaction_strengths(coords) if n > 1 else torch.zeros(0, dtype=RD)
    st = SR.Structure(n, DT, N_SAMPLES, ((1 << n) - 1,) + tuple(1 << j for j in range(n)), tuple(1 << j for j in range(n)))
    psi0 = _randn(gen, batch, 2 ** n, cplx=True)
    psi0 = psi0 / psi0.norm(dim=1, keepdim=True)
    return st, amp, det, u, psi0


def _spec(st, solver, store_states, energy, variant=None, **kw):
    return ProblemSpec(st.n_qubits, st.dt, st.n_samples, st.amp_masks, st.det_masks, solver=solver, store_states=store_states,
                       energy=energy, kernel_variant=variant, **kw)


def _gershgorin(st, e_amp, e_det, u, J=None):
    """max over (b, k) of the largest absolute row sum of H_k, from the tables at the save points."""
    n = st.n_qubits
    c_q = torch.zeros(e_amp.shape[0], n, e_amp.shape[2], dtype=CD)
    d_q = torch.zeros(e_det.shape[0], n, e_det.shape[2], dtype=RD)
    for k, m in enumerate(st.amp_masks):
        for q in range(n):
            if m >> q & 1:
                c_q[:, q] += e_amp[:, k]
    for k, m in enumerate(st.det_masks):
        for q in range(n):
            if m >> q & 1:
                d_q[:, q] += 2.0 * e_det[:, k]
    r = float((c_q.abs().sum(1) + d_q.abs().sum(1)).max()) + float(u.abs().sum())
    return r + (float(J.abs().sum()) if J is not None else 0.0)


def _reference_rows(st, e_amp, e_det, u, states, dev):
    """E, M2 (n_t, B) of states (n_t, B, dim) under H_k of column k, on `dev` (plain torch; differentiable)."""
    op = SR.Operator(st, dev)
    es, ms = [], []
    for k in range(states.shape[0]):
        e_k, m_k = [], []
        for b in range(states.shape[1]):
            bc = b if e_amp.shape[0] > 1 else 0
            psi = states[k, b:b + 1]
            h = SR.structured_matvec(st, e_amp[bc, :, k], e_det[bc, :, k], u, psi, op=op)
            e_k.append((psi.conj() * h).sum().real)
            m_k.append((h.conj() * h).sum().real)
        es.append(torch.stack(e_k))
        ms.append(torch.stack(m_k))
    return torch.stack(es), torch.stack(ms)


# ---- 1. kernel parity on the call's own states ---------------------------------------------------------------------------------
SIZES = (1, 2, 6, 7, 8, 9, 12, 13, 14)


def _variants(n):
    """The sweep families the block must be honoured in: automatic, direct (1, 9), one-launch with the LDS-tile kernels (8, up to 12
    qubits), chained tiles (2, from 13 qubits)."""
    return (0, 1, 9) + ((8,) if n <= 12 else (2,))


# (n, sweep family, energy kernel): below 13 qubits the direct version is the only one; from 13 on each version forced, and automatic
PARITY_CASES = [(n, v, ek) for n in SIZES for v in _variants(n) for ek in ((0,) if n < 13 else (0, 1, 2))]


@pytest.mark.parametrize("n,variant,ek", PARITY_CASES, ids=[f"N{n}-v{v}-{('auto', 'direct', 'tile')[ek]}" for n, v, ek in PARITY_CASES])
def test_rows_match_the_reference_hamiltonian_on_the_returned_states(cuda_device, n, variant, ek):
    dev = cuda_device
    tsave = torch.tensor(TSAVE, dtype=RD)
    for batch in (1, 3):
        st, amp, det, u, psi0 = _problem(n, batch)
        e_amp, e_det = _interp_cols(amp, tsave), _interp_cols(det, tsave)
        bound = _gershgorin(st, e_amp, e_det, u)
        for solver, rows in itertools.product((SolverType.KRYLOV_SE, SolverType.DP5_SE), (1, 2)):
            spec = _spec(st, solver, True, rows, variant, energy_kernel=ek)
            states, expect = evolve(amp.to(dev), det.to(dev), u.to(dev), tsave, psi0.to(dev), spec, None,
                                    energy_amp=e_amp.to(dev), energy_det=e_det.to(dev))
            assert tuple(expect.shape) == (rows, len(TSAVE), batch)
            want_e, want_m = _reference_rows(st, e_amp.to(dev), e_det.to(dev), u.to(dev), states, dev)
            err_e = float((expect[0] - want_e).abs().max())
            print(f"ENERGY N={n} v{variant} B={batch} {solver.name} rows={rows} {spec.options['_last_stats']['kernel_family']}: R {bound:.3e}, "
                  f"|E| <= {float(want_e.abs().max()):.3e}, E error {err_e:.2e}")
            assert float(want_e.abs().max()) > 1e-3  # nothing passes on zeros
            assert err_e <= KERNEL_RTOL * bound
            if rows == 2:
                err_m = float((expect[1] - want_m).abs().max())
                print(f"ENERGY N={n} v{variant} B={batch} {solver.name}: M2 <= {float(want_m.max()):.3e}, M2 error {err_m:.2e}")
                assert err_m <= KERNEL_RTOL * bound ** 2


# ---- 2. end to end against the dense oracle ---------------------------------------------------------------------------------------
def _ham_terms(st, amp, det, u):
    """The oracle's HamTerms of one table set (Ka, n) / (Kd, n): every term an `extra` term with its own target list."""
    n = st.n_qubits
    targets = lambda m: [q for q in range(n) if m >> q & 1]  # noqa: E731
    t = R.HamTerms(n, u, None, None, st.dt, st.n_samples)
    t.extra_amp = [(amp[k], targets(m)) for k, m in enumerate(st.amp_masks)]
    t.extra_det = [(det[k], targets(m)) for k, m in enumerate(st.det_masks)]
    return t


@pytest.mark.parametrize("n", (4, 8, 10))
def test_rows_match_the_oracle_trajectory(cuda_device, n):
    dev = cuda_device
    st, amp, det, u, psi0 = _problem(n, 1)
    tsave = torch.tensor(TSAVE, dtype=RD)
    terms = _ham_terms(st, amp[0], det[0], u)
    o_states = R.krylov_map_dense(terms, psi0.T, tsave)  # (n_t, dim, 1)
    want = []
    for k, t in enumerate(tsave):
        h = R.dense_hamiltonian(terms, t) @ o_states[k]
        want.append((float((o_states[k].conj() * h).sum().real), float((h.conj() * h).sum().real)))
    want = torch.tensor(want, dtype=RD).T  # (2, n_t)
    e_amp, e_det = _interp_cols(amp, tsave), _interp_cols(det, tsave)
    spec = _spec(st, SolverType.KRYLOV_SE, False, 2)
    _, expect = evolve(amp.to(dev), det.to(dev), u.to(dev), tsave, psi0.to(dev), spec, None, energy_amp=e_amp.to(dev), energy_det=e_det.to(dev))
    got = expect[:, :, 0].cpu()
    scale = torch.tensor([1.0, float(want[1].max()) ** 0.5])  # M2 is a square: its bar against its own root
    err = (got - want).abs().max(dim=1).values
    print(f"ENERGY oracle N={n}: E in [{float(want[0].min()):.4f}, {float(want[0].max()):.4f}], M2 <= {float(want[1].max()):.4f}, errors {err.tolist()}")
    assert float(err[0]) <= VALUE_ATOL
    assert float(err[1]) <= VALUE_ATOL * max(1.0, float(want[1].max()))


# ---- 3. gradients -----------------------------------------------------------------------------------------------------------------
def _loss_weights(n_t, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    return _randn(gen, 2, n_t, batch)


def _reference_gradients(n, batch, extra, dev_ref="cpu"):
    """Autograd through the dense map (n <= 10) or the matrix-free one: gradients of sum (a E + b M2) (+ the diagonal row and the
    moments with `extra`) w.r.t. the run's tables, u, psi0 and — separately — the energy tables."""
    st, amp, det, u, psi0 = _problem(n, batch)
    tsave = torch.tensor(TSAVE, dtype=RD)
    leaves = {"amp": amp.clone().requires_grad_(True), "det": det.clone().requires_grad_(True), "u": u.clone().requires_grad_(True),
              "psi0": psi0.clone().requires_grad_(True), "e_amp": _interp_cols(amp, tsave).clone().requires_grad_(True),
              "e_det": _interp_cols(det, tsave).clone().requires_grad_(True)}
    if n <= 10:
        states = torch.cat([R.krylov_map_dense(_ham_terms(st, leaves["amp"][b], leaves["det"][b], leaves["u"]), leaves["psi0"][b][:, None], tsave)
                            for b in range(batch)], dim=2).permute(0, 2, 1)  # (n_t, B, dim)
        es, ms = [], []
        for k in range(len(TSAVE)):
            e_k, m_k = [], []
            for b in range(batch):
                hk = dense_from_structured_terms(n, leaves["u"], [(leaves["e_amp"][b, j, k], m) for j, m in enumerate(st.amp_masks)],
                                                 [(leaves["e_det"][b, j, k], m) for j, m in enumerate(st.det_masks)])
                h = hk @ states[k, b]
                e_k.append((states[k, b].conj() * h).sum().real)
                m_k.append((h.conj() * h).sum().real)
            es.append(torch.stack(e_k))
            ms.append(torch.stack(m_k))
        rows = torch.stack([torch.stack(es), torch.stack(ms)])
    else:
        states = SR.krylov_map(st, leaves["amp"], leaves["det"], leaves["u"], tsave, leaves["psi0"])
        rows = torch.stack(_reference_rows(st, leaves["e_amp"], leaves["e_det"], leaves["u"], states, "cpu"))
    w = _loss_weights(len(TSAVE), batch, 77 + n)
    loss = (w * rows).sum()
    if extra:
        wd, wm = _extra_weights(n, batch)
        loss = loss + (wd * (_diag_table(n)[None, None, :] * states.abs() ** 2).sum(-1)).sum() + (wm * occupation_moments(states.permute(0, 2, 1))).sum()
    g = torch.autograd.grad(loss, list(leaves.values()))
    return {k: v.detach() for k, v in zip(leaves, g)}, rows.detach()


def _diag_table(n):
    x = torch.arange(2 ** n)
    return sum(((x >> j) & 1).to(RD) * (0.3 + 0.1 * j) for j in range(n))


def _extra_weights(n, batch):
    gen = torch.Generator().manual_seed(991 + n)
    return _randn(gen, len(TSAVE), batch), _randn(gen, 1 + n + n * (n - 1) // 2, len(TSAVE), batch)


@functools.lru_cache(maxsize=None)
def _cached_reference(n, batch, extra):
    return _reference_gradients(n, batch, extra)


GRAD_MODES = [("stored", None), ("steps", None), ("full", None), ("partial", 1), ("extra", None)]
GRAD_CASES = [(n, m) for n in (8, 13) for m in GRAD_MODES] + [(13, ("steps-tile", None)), (13, ("extra-tile", None)), (13, ("steps-direct", None))]


@pytest.mark.parametrize("n,mode", GRAD_CASES, ids=[f"N{n}-{m[0]}" for n, m in GRAD_CASES])
def test_gradients_match_autograd_through_the_reference(cuda_device, n, mode):
    """stored: states kept by the caller; steps / full / partial: the tape modes of ProblemSpec without stored states; extra: next
    to a diagonal row and the moments block (the cotangents add in one buffer)."""
    dev = cuda_device
    name, tape_steps = mode
    name, _, forced = name.partition("-")  # (the energy kernel version forced: "tile" / "direct"; none: automatic)
    batch, extra = 2, name == "extra"
    st, amp, det, u, psi0 = _problem(n, batch)
    tsave = torch.tensor(TSAVE, dtype=RD)
    want, want_rows = _cached_reference(n, batch, extra)
    spec = _spec(st, SolverType.KRYLOV_SE, name == "stored", 2, moments=extra, energy_kernel={"": 0, "direct": 1, "tile": 2}[forced])
    if name in ("steps", "full", "partial"):
        spec.tape, spec.tape_steps = name, tape_steps
    leaves = {"amp": amp.to(dev).requires_grad_(True), "det": det.to(dev).requires_grad_(True), "u": u.to(dev).requires_grad_(True),
              "psi0": psi0.to(dev).requires_grad_(True), "e_amp": _interp_cols(amp, tsave).to(dev).requires_grad_(True),
              "e_det": _interp_cols(det, tsave).to(dev).requires_grad_(True)}
    _, expect = evolve(leaves["amp"], leaves["det"], leaves["u"], tsave, leaves["psi0"], spec, _diag_table(n)[None].to(dev) if extra else None,
                       energy_amp=leaves["e_amp"], energy_det=leaves["e_det"])
    rest, en = split_energy(expect, 2)
    assert float((en[0].detach().cpu() - want_rows[0]).abs().max()) <= VALUE_ATOL
    assert float((en[1].detach().cpu() - want_rows[1]).abs().max()) <= VALUE_ATOL * max(1.0, float(want_rows[1].abs().max()))
    loss = (_loss_weights(len(TSAVE), batch, 77 + n).to(dev) * en).sum()
    if extra:
        wd, wm = _extra_weights(n, batch)
        diag_rows, mom = split_moments(rest, n)
        loss = loss + (wd.to(dev) * diag_rows[0]).sum() + (wm.to(dev) * mom).sum()
    got = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    print(f"ENERGY gradients N={n} {name}: tape {spec.options['_last_stats']['tape']}")
    for key in want:
        scale, err = float(want[key].abs().max()), float((got[key].cpu() - want[key]).abs().max())
        print(f"ENERGY gradients N={n} {name}: g_{key} largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 1e-4  # nothing passes on zeros
        assert err <= GRAD_RTOL * scale


# ---- 4. the exchange --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 9, 13))
def test_exchange_rows_and_coupling_gradients(cuda_device, n):
    dev = cuda_device
    st, amp, det, u, psi0 = _problem(n, 1)
    gen = torch.Generator().manual_seed(640 + n)
    J = 0.8 * _randn(gen, n * (n - 1) // 2)
    tsave = torch.tensor(TSAVE[:3], dtype=RD)
    w = _loss_weights(3, 1, 31 + n)
    # reference: the matrix-free map with the exchange, H_k of the rows from separate leaves (the tables at the save points; J is shared)
    o = {"amp": amp[0].clone().requires_grad_(True), "det": det[0].clone().requires_grad_(True), "u": u.clone().requires_grad_(True),
         "J": J.clone().requires_grad_(True)}
    terms = _ham_terms(st, o["amp"], o["det"], o["u"])
    states = (XR.dense_map if n <= 3 else XR.matrix_free_map)(terms, o["J"], 1, psi0.T, tsave, SolverType.KRYLOV_SE)  # (n_t, dim, 1)
    mf = XR.MatrixFree(terms, o["J"], 1)
    rows = []
    for k, t in enumerate(tsave):
        h = mf.apply(t, states[k])
        rows.append(torch.stack([(states[k].conj() * h).sum().real, (h.conj() * h).sum().real]))
    rows = torch.stack(rows).T  # (2, n_t)
    want_g = torch.autograd.grad((w[:, :, 0] * rows).sum(), [o["J"], o["u"]])
    # native: energy tables = the same interpolation, so dL/dJ and dL/dU carry the explicit part as the reference's do
    spec = _spec(st, SolverType.KRYLOV_SE, False, 2, xy_mode=1)
    leaves = [u.to(dev).requires_grad_(True), J.to(dev).requires_grad_(True)]
    _, expect = evolve(amp.to(dev), det.to(dev), leaves[0], tsave, psi0.to(dev), spec, None, xy_pairs=leaves[1],
                       energy_amp=_interp_cols(amp, tsave).to(dev), energy_det=_interp_cols(det, tsave).to(dev))
    got_rows = expect[:, :, 0].cpu()
    err = float(((got_rows - rows.detach()).abs() / torch.tensor([[1.0], [max(1.0, float(rows[1].max()))]])).max())
    got_u, got_J = torch.autograd.grad((w.to(dev) * expect).sum(), leaves)
    print(f"ENERGY XY N={n}: rows error {err:.2e}; g_xy largest {float(want_g[0].abs().max()):.3e}, error {float((got_J.cpu() - want_g[0]).abs().max()):.2e}; "
          f"g_u largest {float(want_g[1].abs().max()):.3e}, error {float((got_u.cpu() - want_g[1]).abs().max()):.2e}")
    assert err <= XY_TOL
    assert float(want_g[0].abs().max()) > 1e-4
    assert rel_err(got_J.cpu().numpy(), want_g[0].numpy()) <= XY_TOL
    assert rel_err(got_u.cpu().numpy(), want_g[1].numpy()) <= XY_TOL


def test_tile_version_is_refused_where_it_does_not_exist(cuda_device):
    dev = cuda_device
    tsave = torch.tensor(TSAVE, dtype=RD)
    for n, xy in ((12, 0), (13, 1)):
        st, amp, det, u, psi0 = _problem(n, 1)
        spec = _spec(st, SolverType.KRYLOV_SE, False, 1, energy_kernel=2, xy_mode=xy)
        with pytest.raises(NotImplementedError, match="energy_kernel = 2"):
            evolve(amp.to(dev), det.to(dev), u.to(dev), tsave, psi0.to(dev), spec, None,
                   xy_pairs=torch.ones(n * (n - 1) // 2, dtype=RD, device=dev) if xy else None,
                   energy_amp=_interp_cols(amp, tsave).to(dev), energy_det=_interp_cols(det, tsave).to(dev))


def test_one_directional_exchange_is_refused(cuda_device):
    dev = cuda_device
    st, amp, det, u, psi0 = _problem(3, 1)
    tsave = torch.tensor(TSAVE, dtype=RD)
    spec = _spec(st, SolverType.KRYLOV_SE, False, 1, xy_mode=2)
    with pytest.raises(NotImplementedError, match="xy_mode = 2"):
        evolve(amp.to(dev), det.to(dev), u.to(dev), tsave, psi0.to(dev), spec, None, xy_pairs=torch.ones(3, dtype=RD, device=dev),
               energy_amp=_interp_cols(amp, tsave).to(dev), energy_det=_interp_cols(det, tsave).to(dev))


# ---- 5. an eigenstate -------------------------------------------------------------------------------------------------------------
def test_variance_of_an_eigenstate_stays_at_the_cancellation_floor(cuda_device):
    """Constant tables and an eigenvector of the dense H at 8 qubits: the state only picks up a phase, E is the eigenvalue and
    M2 - E^2 is what two roundings of numbers of size R^2 leave: below 1e-12 R^2 at every save point (the floor the docstring of
    utils.energy_variance states)."""
    dev = cuda_device
    n = 8
    st, amp, det, u, _ = _problem(n, 1)
    amp_c, det_c = amp[:, :, 2:3].expand(-1, -1, N_SAMPLES).contiguous(), det[:, :, 2:3].expand(-1, -1, N_SAMPLES).contiguous()
    tsave = torch.tensor(TSAVE, dtype=RD)
    h = dense_from_structured_terms(n, u, [(amp_c[0, j, 0], m) for j, m in enumerate(st.amp_masks)], [(det_c[0, j, 0], m) for j, m in enumerate(st.det_masks)])
    evals, evecs = torch.linalg.eigh(h)
    pick = 2 ** n // 3
    e_amp, e_det = _interp_cols(amp_c, tsave), _interp_cols(det_c, tsave)
    bound = _gershgorin(st, e_amp, e_det, u)
    spec = _spec(st, SolverType.KRYLOV_SE, False, 2)
    _, expect = evolve(amp_c.to(dev), det_c.to(dev), u.to(dev), tsave, evecs[:, pick][None].contiguous().to(dev), spec, None,
                       energy_amp=e_amp.to(dev), energy_det=e_det.to(dev))
    e, m2 = expect[0, :, 0].cpu(), expect[1, :, 0].cpu()
    var = (m2 - e ** 2).abs()
    print(f"ENERGY eigenstate: eigenvalue {float(evals[pick]):.6f}, E error {float((e - evals[pick]).abs().max()):.2e}, |M2 - E^2| {float(var.max()):.2e}, R^2 {bound ** 2:.3e}")
    assert float((e - evals[pick]).abs().max()) <= 1e-9 * bound  # (the trajectory itself: the project's bar for values)
    assert float(var.max()) <= KERNEL_RTOL * bound ** 2


# ---- 6. reproducibility and workspace hygiene ---------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits(cuda_device):
    dev = cuda_device
    st, amp, det, u, psi0 = _problem(14, 3)
    tsave = torch.tensor(TSAVE, dtype=RD)
    args = (amp.to(dev), det.to(dev), u.to(dev), tsave, psi0.to(dev))
    kw = dict(energy_amp=_interp_cols(amp, tsave).to(dev), energy_det=_interp_cols(det, tsave).to(dev))
    for ek in (1, 2):  # each version of the kernels against itself
        runs = [evolve(*args, _spec(st, SolverType.KRYLOV_SE, False, 2, energy_kernel=ek), None, **kw)[1].cpu() for _ in range(2)]
        assert torch.isfinite(runs[0]).all() and float(runs[0].abs().max()) > 0
        assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("n,tape,ek", [(3, "auto", 0), (9, "auto", 0), (13, "auto", 1), (13, "steps", 1), (13, "auto", 2), (13, "steps", 2)])
def test_block_does_not_depend_on_workspace_contents(cuda_device, monkeypatch, n, tape, ek):
    dev = cuda_device
    st, amp, det, u, psi0 = _problem(n, 2)
    tsave = torch.tensor(TSAVE, dtype=RD)
    w = _loss_weights(len(TSAVE), 2, 5 + n).to(dev)

    def run():
        spec = _spec(st, SolverType.KRYLOV_SE, False, 2, energy_kernel=ek)
        spec.tape = tape
        leaves = [t.to(dev).requires_grad_(True) for t in (amp, det, u, psi0, _interp_cols(amp, tsave), _interp_cols(det, tsave))]
        _, expect = evolve(leaves[0], leaves[1], leaves[2], tsave, leaves[3], spec, None, energy_amp=leaves[4], energy_det=leaves[5])
        g = torch.autograd.grad((w * expect).sum(), leaves)
        out = dict(zip(("g_amp", "g_det", "g_u", "g_psi0", "g_energy_amp", "g_energy_det"), g), expect=expect)
        return {k: (torch.view_as_real(v) if v.is_complex() else v).detach().cpu().numpy() for k, v in out.items()}

    zeros, nans = _both_fills(monkeypatch, run)
    _compare(f"ENERGY N{n} tape={tape}", zeros, nans)


# ---- 7. feature off ---------------------------------------------------------------------------------------------------------------
def test_fields_are_ignored_with_the_block_off(cuda_device, monkeypatch):
    """energy_rows = 0: expect, the states and every gradient of one 13-qubit case are bit-identical whether the three new pointers
    (and the two gradient pointers) are NULL or garbage.  The case is one whose outputs have ONE summation order, so that two calls
    can agree in every bit at all: the rows are the moments block (fixed order, no atomics; the diagonal and Pauli rows are summed
    with atomics), and one trajectory on the direct kernels has 32 workgroups, each with a gradient replica of its own.  g_u is the
    one output that has no fixed order on any commit: k_ugrad adds the partial sums of its 32 workgroups per pair with atomics, so two
    calls with identical arguments differ in its last bits.  It is held to 1e-12 of its largest entry, the bar
    of tests/test_gpu_workspace_contents.py for repeats of one route; everything else is compared bit for bit."""
    dev = cuda_device
    st, amp, det, u, psi0 = _problem(13, 1)
    tsave = torch.tensor(TSAVE, dtype=RD)
    gen = torch.Generator().manual_seed(12)
    w = _randn(gen, 1 + 13 + 78, len(TSAVE), 1).to(dev)
    garbage = [False]
    real_call = S._Call

    class Call(real_call):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            if garbage[0]:
                self.problem.energy_amp = 0xDEAD0000
                self.problem.energy_det = 0xDEAD0008
                self.problem.g_energy_amp = 0xDEAD0010
                self.problem.g_energy_det = 0xDEAD0018

    monkeypatch.setattr(S, "_Call", Call)

    def run():
        spec = _spec(st, SolverType.KRYLOV_SE, True, 0, variant=1, moments=True)
        leaves = [t.to(dev).requires_grad_(True) for t in (amp, det, u, psi0)]
        states, expect = evolve(leaves[0], leaves[1], leaves[2], tsave, leaves[3], spec, None)
        g = torch.autograd.grad((w * expect).sum(), leaves)
        return [states.detach().cpu(), expect.detach().cpu()] + [x.cpu() for x in g]

    plain = run()
    garbage[0] = True
    poisoned = run()
    for name, a, b in zip(("states", "expect", "g_amp", "g_det", "g_u", "g_psi0"), plain, poisoned):
        assert float(a.abs().max()) > 0, name
        if name == "g_u":
            print(f"ENERGY off: g_u largest entry {float(a.abs().max()):.3e}, garbage against NULL pointers {float((a - b).abs().max()):.2e}")
            assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
        else:
            assert torch.equal(a, b), name
