"""Native XY exchange in the tangent sweep, host side (no GPU): the dense forward-mode reference (tests/xy_tangent_reference.py) against
the pair-block reference (dJ = 0) and against reverse-mode autograd through the dense map (a d_xy-only direction); the argument
validation of RYDIFF_TANGENT_XY / RydTangent.d_xy through the built library, for all three sweeps (every refusal happens before
anything touches a device); and which route the emulator's all-times entry points take with and without ``xy_native=True``."""
import ctypes

import numpy as np
import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd import backend as backend_module
from pulser_diff_amd.hamiltonian import Hamiltonian
from pulser_diff_amd.solver import SolverType
from pulser_diff_amd.utils import DiagonalObservable
from tests import xy_exchange_reference as X
from tests.helpers import random_terms, to_native
from tests.tangent_pair_reference import tangent_pair_reference
from tests.test_tangent_host import _call, _info
from tests.test_xy_exchange_host import emulator, grid
from tests.xy_tangent_reference import pair_blocks, xy_tangent_reference


def _randn(gen, *shape, cplx=False):
    re = torch.randn(*shape, generator=gen, dtype=torch.float64)
    return torch.complex(re, torch.randn(*shape, generator=gen, dtype=torch.float64)) if cplx else re


def _couplings(n, seed):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * (2.0 * torch.rand(n * (n - 1) // 2, generator=g, dtype=torch.float64) - 1.0)


# ---- 1. dJ = 0: the exchange written as pair blocks ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [3, 5])
def test_without_coupling_tangents_the_reference_is_the_pair_block_reference(n, mode):
    terms = random_terms(n, 25, 0.004, seed=60 + n, local=True)
    amp, det, u, _ = to_native(terms, "cpu", SolverType.KRYLOV_SE)
    gen = torch.Generator().manual_seed(700 + n)
    J = _couplings(n, 11 + n)
    dim, n_dir, batch = 2 ** n, 2, 2
    psi0 = _randn(gen, dim, batch, cplx=True)
    psi0 = psi0 / psi0.norm(dim=0, keepdim=True)
    d_amp = float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape[1:], cplx=True)
    d_det = float(det.abs().max()) * _randn(gen, n_dir, *det.shape[1:])
    d_u = _randn(gen, n_dir, u.numel())
    d_psi = _randn(gen, n_dir, dim, batch, cplx=True) / np.sqrt(dim)
    tsave = torch.tensor((0.0, 0.0313, 0.0622), dtype=torch.float64)
    for solver in (SolverType.KRYLOV_SE, SolverType.DP5_SE):
        got = xy_tangent_reference(terms, J, mode, d_amp, d_det, d_u, None, psi0, d_psi, tsave, solver)
        want = tangent_pair_reference(terms, pair_blocks(n, J, mode), d_amp, d_det, d_u, psi0, d_psi, tsave, solver)
        for g, w, name in zip(got, want, ("states", "tangents")):
            err = float((g - w).abs().max())
            print(f"N={n} mode {mode} {solver.name}: {name} differ by {err:.2e} (largest entry {float(w.abs().max()):.2e})")
            assert float(w.abs().max()) > 1e-2 and err <= 1e-12


# ---- 2. a d_xy-only direction against reverse-mode autograd --------------------------------------------------------------------
@pytest.mark.parametrize("solver", [SolverType.KRYLOV_SE, SolverType.DP5_SE])
@pytest.mark.parametrize("mode", [1, 2])
def test_a_coupling_tangent_is_the_jacobian_vector_product_of_the_dense_map(mode, solver):
    n = 3
    terms = random_terms(n, 25, 0.004, seed=63, local=True)
    gen = torch.Generator().manual_seed(900 + mode)
    J = _couplings(n, 21)
    dJ = _randn(gen, 2, J.numel())
    dim = 2 ** n
    psi0 = _randn(gen, dim, 1, cplx=True)
    psi0 = psi0 / psi0.norm()
    tsave = torch.tensor((0.0, 0.0313, 0.0622), dtype=torch.float64)
    states, tangents = xy_tangent_reference(terms, J, mode, None, None, None, dJ, psi0, None, tsave, solver)
    # the Jacobian of every real and imaginary part w.r.t. J by one reverse pass per entry, contracted with dJ
    Jl = J.clone().requires_grad_(True)
    out = X.dense_map(terms, Jl, mode, psi0, tsave, solver)
    assert float((out.detach() - states).abs().max()) <= 1e-12
    flat = torch.view_as_real(out).reshape(-1)
    jac = torch.stack([torch.autograd.grad(flat[i], Jl, retain_graph=True)[0] for i in range(flat.numel())])  # (entries, P)
    for d in range(2):
        want = torch.view_as_complex((jac @ dJ[d]).reshape(tuple(out.shape) + (2,)))
        got = tangents[:, d]
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"mode {mode} {solver.name} direction {d}: largest entry {scale:.2e}, max error {err:.2e}")
        assert scale > 1e-2 and err <= 1e-10 * scale


# ---- 3. the C ABI's validation, through the built library ---------------------------------------------------------------------------
SWEEPS = ("rydiff_forward_tangent", "rydiff_forward_geometry", "rydiff_forward_fisher")


def _sweep_call(sweep, mutate_problem=None, mutate_tangent=None):
    """One of the three sweeps with host dummies for every device pointer: a call that gets past validation would touch them."""
    call = _call()
    tg = _native.RydTangent()
    tg.n_dir = 2
    tg.d_amp = 0x1000
    if mutate_problem:
        mutate_problem(call.problem)
    if mutate_tangent:
        mutate_tangent(tg)
    plan = _info()
    dummy = ctypes.c_void_p(0x1000)
    extra = {"rydiff_forward_tangent": (), "rydiff_forward_geometry": (dummy,), "rydiff_forward_fisher": (dummy, dummy)}[sweep]
    rc = getattr(_native.lib(), sweep)(ctypes.byref(call.problem), ctypes.byref(plan), ctypes.byref(tg), dummy, None, dummy, *extra,
                                       dummy, 0, None)
    _native.check(rc)


def _with_xy(p, mode=1):
    p.xy_mode, p.xy_pairs = mode, 0x1000


def _flags(*bits):
    value = 0
    for b in bits:
        value |= b
    return lambda t: setattr(t, "flags", value)


def test_rydtangent_mirror_has_the_new_last_field():
    assert _native.TANGENT_XY == 16
    assert [f[0] for f in _native.RydTangent._fields_][-2:] == ["flags", "d_xy"]
    assert ctypes.sizeof(_native.RydTangent) == _native.lib().rydiff_sizeof_tangent()


@pytest.mark.parametrize("sweep", SWEEPS)
def test_the_flag_and_d_xy_are_validated_before_anything_touches_a_device(sweep):
    with pytest.raises(ValueError, match="RYDIFF_TANGENT_XY"):  # the flag on a problem without the exchange
        _sweep_call(sweep, mutate_tangent=_flags(_native.TANGENT_XY))
    with pytest.raises(ValueError, match="unknown bits"):
        _sweep_call(sweep, mutate_tangent=_flags(32))
    with pytest.raises(ValueError, match="d_xy"):  # the tangent of couplings the problem does not have
        _sweep_call(sweep, mutate_tangent=lambda t: setattr(t, "d_xy", 0x1000))
    for mode in (1, 2):
        with pytest.raises(NotImplementedError, match="XY exchange"):  # without the flag: the refusal callers were written against
            _sweep_call(sweep, lambda p, m=mode: _with_xy(p, m))
    with pytest.raises(ValueError, match="xy_mode"):
        _sweep_call(sweep, lambda p: _with_xy(p, 3), _flags(_native.TANGENT_XY))
    # with the flag the problem is taken: the (host-side) workspace test stops the call, nothing launched
    with pytest.raises(MemoryError, match="workspace too small"):
        _sweep_call(sweep, _with_xy, _flags(_native.TANGENT_XY))

    def only_d_xy(t):
        t.flags, t.d_amp, t.d_xy = _native.TANGENT_XY, None, 0x1000

    with pytest.raises(MemoryError, match="workspace too small"):  # d_xy alone is a tangent input
        _sweep_call(sweep, _with_xy, only_d_xy)
    with pytest.raises(ValueError, match="d_amp, d_det, d_u, d_psi0 are NULL"):
        _sweep_call(sweep, _with_xy, lambda t: (setattr(t, "flags", _native.TANGENT_XY), setattr(t, "d_amp", None)))


@pytest.mark.parametrize("sweep", SWEEPS)
def test_what_the_exchange_is_refused_with_stays_refused_with_the_flag(sweep):
    pair_q = np.array([[0, 1]], dtype=np.uint32)
    pair_t = np.zeros((1, 16), dtype=np.complex128)

    def xy_and(setter):
        def mutate(p):
            _with_xy(p)
            setter(p)
        return mutate

    def with_pair(p):
        p.n_pair_terms, p.pair_qubits, p.pair_tables = 1, pair_q.ctypes.data, pair_t.ctypes.data

    with pytest.raises(NotImplementedError, match="shard"):
        _sweep_call(sweep, xy_and(lambda p: setattr(p, "shard_bits", 1)), _flags(_native.TANGENT_XY))
    for extra in (0, _native.TANGENT_DENSITY_MATRIX):
        with pytest.raises(NotImplementedError, match="dm_atoms"):
            _sweep_call(sweep, xy_and(lambda p: setattr(p, "dm_atoms", 1)), _flags(_native.TANGENT_XY, extra))
    for extra in (0, _native.TANGENT_PAIR_TERMS):
        with pytest.raises(NotImplementedError, match="pair terms"):
            _sweep_call(sweep, xy_and(with_pair), _flags(_native.TANGENT_XY, extra))
    with pytest.raises(NotImplementedError, match="conditioned"):
        _sweep_call(sweep, xy_and(lambda p: setattr(p, "amp_conditioned_terms", 1)), _flags(_native.TANGENT_XY))


def test_workspace_grows_by_the_coupling_tangents():
    L = _native.lib()
    plan = _info()
    plain, xy = _call(), _call()
    _with_xy(xy.problem)
    a = L.rydiff_tangent_workspace_bytes_flags(ctypes.byref(plain.problem), ctypes.byref(plan), 5, 0)
    b = L.rydiff_tangent_workspace_bytes_flags(ctypes.byref(xy.problem), ctypes.byref(plan), 5, _native.TANGENT_XY)
    assert a > 0 and b - a >= 6 * 3 * 8  # 5 directions are padded to 6; 3 pairs of doubles each
    assert L.rydiff_tangent_workspace_bytes_flags(ctypes.byref(xy.problem), ctypes.byref(plan), 5, 0) == 0
    assert "XY exchange" in _native.last_error()


# ---- 4. which route the emulator takes ----------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _entry_points(sim, x):
    obs = DiagonalObservable(torch.linspace(0.0, 1.0, 2 ** 4, dtype=torch.float64))
    return {
        "run_sensitivities": lambda: sim.run_sensitivities(x, [obs], solver=SolverType.KRYLOV_SE),
        "run_rdm_sensitivities": lambda: sim.run_rdm_sensitivities(x, [[0, 1]], solver=SolverType.KRYLOV_SE),
        "run_occupation_sensitivities": lambda: sim.run_occupation_sensitivities(x, solver=SolverType.KRYLOV_SE),
        "run_quantum_fisher": lambda: sim.run_quantum_fisher(x, solver=SolverType.KRYLOV_SE),
        "run_classical_fisher": lambda: sim.run_classical_fisher(x, solver=SolverType.KRYLOV_SE),
    }


def test_a_default_emulator_still_borrows_the_dense_terms_and_a_native_one_does_not(monkeypatch):
    asked = []

    def spy(self, what):
        asked.append(what)
        raise _Reached(what)

    monkeypatch.setattr(Hamiltonian, "require_dense_xy", spy)
    monkeypatch.setattr(Hamiltonian, "_warned_xy", True)
    knob = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    sim = emulator(grid(4), xy_hermitian=True)
    for name, call in _entry_points(sim, [knob]).items():
        if name.endswith("fisher"):  # they hand no dense pair terms to the sweep: refused as before
            with pytest.raises(NotImplementedError, match=f"{name} is not available with the XY exchange"):
                call()
        else:
            with pytest.raises(_Reached, match=name):
                call()
    assert asked == ["run_sensitivities", "run_rdm_sensitivities", "run_occupation_sensitivities"]

    # xy_native=True: no borrow; the solver's sweeps get the couplings and their tangents w.r.t. the coordinates
    asked.clear()
    seen = []

    def sweep(*args, **kw):
        seen.append(kw)
        raise _Reached("sweep")

    for fn in ("evolve_tangent", "evolve_geometry", "evolve_fisher"):
        monkeypatch.setattr(backend_module, fn, sweep)
    coords = grid(4).requires_grad_(True)
    sim = emulator(coords, xy_hermitian=True, xy_native=True)
    ham = sim._hamiltonian
    for name, call in _entry_points(sim, [coords]).items():
        with pytest.raises(_Reached, match="sweep"):
            call()
        assert ham.xy_mode == 1 and ham.pair_terms == () and ham.problem_spec().xy_mode == 1
    assert asked == [] and len(seen) == 5
    jac = torch.stack([torch.autograd.grad(ham._xy_pairs_host[p], coords, retain_graph=True)[0].reshape(-1) for p in range(6)], dim=1)
    for kw in seen:
        assert kw["xy_pairs"] is ham.xy_pairs and tuple(kw["d_xy"].shape) == (8, 6)
        assert float(jac.abs().max()) > 0 and float((kw["d_xy"] - jac).abs().max()) <= 1e-12 * float(jac.abs().max())


def test_table_tangents_keeps_its_three_outputs_and_adds_the_couplings_on_request():
    coords = grid(4).requires_grad_(True)
    sim = emulator(coords, xy_hermitian=True, xy_native=True)
    assert len(sim._table_tangents([coords])) == 3
    d_xy = sim._table_tangents([coords], with_xy=True)[3]
    assert tuple(d_xy.shape) == (8, 6)
    dense = emulator(grid(4), xy_hermitian=True)  # the dense route has no couplings to differentiate
    assert dense._table_tangents([torch.tensor(1.0, dtype=torch.float64, requires_grad=True)], with_xy=True)[3] is None
    nine = emulator(grid(9), xy_hermitian=True)  # the 8-atom refusal of a default emulator names the way out
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for run_sensitivities.*xy_native=True"):
        nine.run_sensitivities([torch.tensor(1.0, dtype=torch.float64, requires_grad=True)],
                               [DiagonalObservable(torch.ones(2 ** 9, dtype=torch.float64))], solver=SolverType.KRYLOV_SE)
