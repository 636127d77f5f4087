"""Reduced density matrices of master-equation runs (RydProblem.n_dm_rdms / dm_rdm_masks), the host side: where the two fields sit
in the struct, every validation rule of plan.hpp: build_dm for them — answered without a device — the row bookkeeping, the torch route
on stored density matrices against an independent numpy partial trace (tests/dm_rdm_reference.py), pack_dm_observables and
CoherentResults, and the closed forms of the negativity utilities."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd.lindblad import MasterEquationResult, pack_dm_observables
from pulser_diff_amd.observables import (DensityMatrixObservables, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap,
                                         reduced_density_matrix)
from pulser_diff_amd.simresults import CoherentResults
from pulser_diff_amd.utils import DiagonalObservable, logarithmic_negativity, negativity, partial_transpose, von_neumann_entropy
from tests.dm_rdm_reference import partial_trace, rdm_cotangent_reference, rdm_rows_reference
from tests.test_dm_observables_host import N, _dm_call, _plan


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_two_fields_sit_between_the_ket_rdm_block_and_dm_atoms():
    names = [f[0] for f in _native.RydProblem._fields_]
    assert names.index("rdm_masks") + 1 == names.index("n_dm_rdms")
    assert names.index("dm_rdm_masks") + 1 == names.index("dm_atoms")
    assert names.index("n_dm_rdms") + 1 == names.index("dm_rdm_masks")
    assert ctypes.sizeof(_native.RydProblem) == _native.lib().rydiff_sizeof_problem()
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    assert f"#define RYDIFF_MAX_RDMS {_native.MAX_RDMS}" in header and f"#define RYDIFF_MAX_RDM_QUBITS {_native.MAX_RDM_QUBITS}" in header
    assert f"#define RYDIFF_MAX_DM_ATOMS {_native.MAX_DM_ATOMS}" in header
    assert "int32_t n_dm_rdms;" in header and "const uint32_t* dm_rdm_masks;" in header


def _with_masks(call, masks, count=None):
    """Sets the two fields by hand (past the Python validation); the array stays alive on the call."""
    call.raw_dm_rdm_masks = np.asarray(masks, dtype=np.uint32)
    call.problem.n_dm_rdms = len(masks) if count is None else count
    call.problem.dm_rdm_masks = call.raw_dm_rdm_masks.ctypes.data if len(masks) else None
    return call


BAD = [
    ("count-negative", lambda c: _with_masks(c, (1,), count=-1), "n_dm_rdms"),
    ("count-cap", lambda c: _with_masks(c, (1,) * (_native.MAX_RDMS + 1)), "n_dm_rdms"),
    ("null-masks", lambda c: _with_masks(c, (), count=1), "dm_rdm_masks"),
    ("empty-mask", lambda c: _with_masks(c, (0b11, 0)), "empty"),
    ("bit-at-n", lambda c: _with_masks(c, (0b01, 1 << N)), "atom"),  # a legal qubit of the DOUBLED register
    ("bit-far-above", lambda c: _with_masks(c, (1 << 31,)), "atom"),
]


@pytest.mark.parametrize("mutate,match", [b[1:] for b in BAD], ids=[b[0] for b in BAD])
def test_rydiff_plan_rejects_bad_dm_rdm_fields_without_a_device(mutate, match):
    call = mutate(_dm_call(shots=False))
    rc = _plan(call)
    assert rc == _native.RYDIFF_EINVAL, (rc, _native.last_error())
    with pytest.raises(ValueError, match=match):
        _native.check(rc)


def _passes_the_field_checks(call):
    """True when build_plan gets past build_dm: the evaluation times — checked right behind it — are made non-increasing, so a call
    that passes answers RYDIFF_EINVAL about tsave and never reaches a device (the tensors of these calls live on the host)."""
    call.tsave[:] = 0.0
    rc = _plan(call)
    assert rc in (_native.RYDIFF_EINVAL, _native.RYDIFF_ENOTIMPL), (rc, _native.last_error())
    return rc == _native.RYDIFF_EINVAL and "tsave" in _native.last_error()


def _wide_call(n=7):
    """A doubled register of 7 atoms (the two-atom one of _dm_call cannot hold a mask of more than 6 atoms)."""
    from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call

    nq = 2 * n
    spec = ProblemSpec(nq, 0.004, 5, (2 ** nq - 1,), (2 ** nq - 1,), solver=SolverType.DP5_SE, dm=DensityMatrixObservables(n, purity=True))
    return _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(nq * (nq - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, 3), 1, None)


def test_more_than_six_atoms_in_a_mask_are_rejected():
    rc = _plan(_with_masks(_wide_call(), (0b1111111,)))
    assert rc == _native.RYDIFF_EINVAL and "more than 6" in _native.last_error(), (rc, _native.last_error())
    assert _passes_the_field_checks(_with_masks(_wide_call(), (0b0111111, 0b1000000))), _native.last_error()  # six atoms; the last atom alone


def test_well_formed_and_ignored_fields_pass_the_field_checks():
    """A well-formed request passes; dm_atoms = 0 ignores the two fields like the other dm_* fields, garbage included (the call plans
    as it did before the fields existed); a sharded call is still RYDIFF_ENOTIMPL."""
    assert _passes_the_field_checks(_dm_call(shots=False))
    good = _with_masks(_dm_call(shots=False), (0b11, 0b01, 0b10))
    assert _passes_the_field_checks(good), _native.last_error()
    ignored = _with_masks(_dm_call(shots=False), (0, 1 << 30), count=99)
    ignored.problem.dm_atoms = 0
    assert _passes_the_field_checks(ignored), _native.last_error()
    ignored.problem.dm_rdm_masks = None
    assert _passes_the_field_checks(ignored), _native.last_error()
    sharded = _with_masks(_dm_call(shots=False), (0b11,))
    sharded.problem.shard_bits = 1
    assert _plan(sharded) == _native.RYDIFF_ENOTIMPL and "shard" in _native.last_error()
    L = _native.lib()
    info = _native.RydPlanInfo()
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(good.problem), ctypes.byref(info), 1) == 0
    assert "density-matrix" in _native.last_error()


def test_the_call_carries_the_masks_and_the_row_count_grows():
    """_Call fills the two fields and keeps the host array alive; rows() — what the solver sizes expect_out with — grows by
    2 * sum 4^m and not otherwise."""
    from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call

    n, nq = 3, 6
    base = DensityMatrixObservables(n, diag=torch.zeros(2, 8, dtype=torch.float64), purity=True)
    assert base.rows() == 3 and base.rdm_rows() == 0 and base.packed_rdms() is None
    assert DensityMatrixObservables(n, purity=True, rdms=[]).rows() == 1
    dm = DensityMatrixObservables(n, diag=torch.zeros(2, 8, dtype=torch.float64), purity=True,
                                  rdms=[ReducedDensityMatrix([2, 0]), 0b010, ReducedDensityMatrix([0, 1, 2])])
    assert dm.rdm_rows() == 2 * (16 + 4 + 64) and dm.rows() == 3 + 2 * (16 + 4 + 64)
    assert dm.packed_rdms().tolist() == [0b101, 0b010, 0b111] and dm.packed_rdms().dtype == np.uint32
    spec = ProblemSpec(nq, 0.004, 5, (2 ** nq - 1,), (2 ** nq - 1,), solver=SolverType.DP5_SE, dm=dm)
    call = _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(nq * (nq - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, 3), 1, None)
    p = call.problem
    assert p.n_dm_rdms == 3 and p.dm_rdm_masks == call.dm_buffers[3].ctypes.data
    assert call.dm_buffers[3].tolist() == [0b101, 0b010, 0b111]
    assert _passes_the_field_checks(call), _native.last_error()
    plain = _Call(ProblemSpec(nq, 0.004, 5, (2 ** nq - 1,), (2 ** nq - 1,), solver=SolverType.DP5_SE, dm=base),
                  torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                  torch.zeros(nq * (nq - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, 3), 1, None)
    assert plain.problem.n_dm_rdms == 0 and not plain.problem.dm_rdm_masks


def test_python_side_checks():
    for bad, match in (([ReducedDensityMatrix([0, 3])], "outside"), ([0], "mask"), ([1 << 3], "mask"), ([0b1] * 9, "1 to 8"),
                       ([-1], "mask")):
        with pytest.raises(ValueError, match=match):
            DensityMatrixObservables(3, rdms=bad).check(6, 1)
    with pytest.raises(ValueError, match="mask"):
        DensityMatrixObservables(7, rdms=[0b1111111]).check(14, 1)
    with pytest.raises(TypeError):
        DensityMatrixObservables(3, rdms=[None]).check(6, 1)
    DensityMatrixObservables(7, rdms=[0b0111111, ReducedDensityMatrix([6])]).check(14, 1)


# ---- the torch route on stored density matrices -------------------------------------------------------------------------------
ORDERS = {2: [(0,), (1,), (0, 1), (1, 0)], 3: [(1,), (0, 2), (2, 0), (2, 0, 1), (0, 1, 2)], 5: [(4,), (1, 3), (3, 1), (4, 0, 2), (0, 1, 2, 3, 4),
                                                                                             (3, 4, 0, 2, 1)]}


@pytest.mark.parametrize("n", list(ORDERS))
def test_torch_route_matches_an_independent_numpy_partial_trace(n):
    """Random complex, non-Hermitian rho; ascending and non-ascending orders (the latter exercise the ordering the native route takes
    from native_index); m = n keeps every entry (a permutation of rho).  1e-14: sums of at most 2^4 O(1) terms."""
    dim, n_t, batch = 2 ** n, 2, 3
    gen = torch.Generator().manual_seed(90 + n)
    rho = torch.randn(n_t, dim, dim, batch, generator=gen, dtype=torch.complex128)
    assert float((rho - rho.conj().transpose(1, 2)).abs().max()) > 0.1
    for atoms in ORDERS[n]:
        obs = ReducedDensityMatrix(atoms)
        got = reduced_density_matrix(obs, rho)
        assert got.shape == (n_t, batch, 2 ** len(atoms), 2 ** len(atoms)) and got.dtype == torch.complex128
        for k in range(n_t):
            for b in range(batch):
                want = partial_trace(rho[k, :, :, b].numpy(), n, atoms)
                assert np.abs(got[k, b].numpy() - want).max() <= 1e-14, (atoms, k, b)
        # the order of `qubits` is the permutation native_index describes, applied to the ascending-order matrix
        asc = reduced_density_matrix(ReducedDensityMatrix(sorted(atoms)), rho)
        perm = obs.native_index()
        assert float((got - asc.index_select(2, perm).index_select(3, perm)).abs().max()) <= 1e-14
    assert torch.equal(reduced_density_matrix(ReducedDensityMatrix(range(n)), rho), rho.permute(0, 3, 1, 2))


def test_torch_route_is_differentiable_and_checks_its_input():
    rho = torch.randn(1, 4, 4, 1, dtype=torch.complex128, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    w = torch.randn(2, 2, dtype=torch.complex128, generator=torch.Generator().manual_seed(4))
    (reduced_density_matrix(ReducedDensityMatrix([1]), rho)[0, 0] * w).sum().real.backward()
    # d Re(sum w rho_A) / d rho: torch's convention gives conj(w) at every entry (idx(a, e), idx(a', e))
    want = np.kron(np.eye(2), w.numpy().conj())
    assert np.abs(rho.grad[0, :, :, 0].numpy() - want).max() <= 1e-15
    with pytest.raises(ValueError, match="outside"):
        reduced_density_matrix(ReducedDensityMatrix([2]), rho)
    with pytest.raises(ValueError):
        reduced_density_matrix(ReducedDensityMatrix([0]), torch.zeros(1, 4, 2, 1, dtype=torch.complex128))
    with pytest.raises(ValueError):
        reduced_density_matrix(ReducedDensityMatrix([0]), torch.zeros(1, 3, 3, 1, dtype=torch.complex128))


def test_reference_rows_and_cotangent_are_adjoint_to_each_other():
    """The two dense references of the GPU tests: <g, rows(v)> = Re <cot(g), v> (torch's convention: cot = dL/dRe + i dL/dIm) for a
    random v — each is checked by the other — and the rows follow the layout the header writes down."""
    n, masks = 4, (0b0110, 0b1001, 0b0001, 0b1111)
    rng = np.random.default_rng(5)
    v = rng.normal(size=4 ** n) + 1j * rng.normal(size=4 ** n)
    rows, tot = rdm_rows_reference(v, n, masks)
    assert rows.shape == tot.shape == (2 * (16 + 16 + 4 + 256),)
    rho = v.reshape(16, 16)
    # mask 0b0110 = atoms 1, 2; entry (a, a') = (0b10, 0b01): atom 1 = 1, atom 2 = 0 on the row side; atom 1 = 0, atom 2 = 1 on the column side
    want = sum(rho[(e0 << 3) | (1 << 2) | (0 << 1) | e3, (e0 << 3) | (0 << 2) | (1 << 1) | e3] for e0 in (0, 1) for e3 in (0, 1))
    assert abs(complex(rows[2 * (2 * 4 + 1)], rows[2 * (2 * 4 + 1) + 1]) - want) < 1e-14
    g = rng.normal(size=rows.shape)
    cot, ctot = rdm_cotangent_reference(n, masks, g)
    assert abs(float(g @ rows) - float((cot.real * v.real + cot.imag * v.imag).sum())) < 1e-11
    assert (ctot >= np.abs(cot) - 1e-15).all() and ctot.shape == cot.shape == (4 ** n,)


# ---- pack_dm_observables, MasterEquationResult, CoherentResults -----------------------------------------------------------------
def test_pack_dm_observables_takes_rdms_and_keeps_the_real_rows_in_front():
    n, dim = 3, 8
    a, b = ReducedDensityMatrix([0, 2]), ReducedDensityMatrix([1])
    z = DiagonalObservable(torch.linspace(-1, 1, dim, dtype=torch.float64))
    xx = PauliObservable(n, [(1.0, {0: "X", 1: "X"})])
    fid = StateOverlap(torch.ones(dim, dtype=torch.complex128))
    dm, rows = pack_dm_observables([a, z, Purity(), b, xx, fid], n, 1, "cpu")
    # real rows: diag 0, Pauli 1, fidelity 2, purity 3; then a (2 * 16 rows from 4) and b (2 * 4 rows from 36)
    assert rows == [4, 0, 3, 4 + 32, 1, 2]
    assert dm.rdms == [a, b] and dm.rows() == 4 + 32 + 8 and dm.packed_rdms().tolist() == [0b101, 0b010]
    dm.check(2 * n, 1)
    only, rows = pack_dm_observables([b], n, 1, "cpu")
    assert rows == [0] and only.rows() == 8 and only.n_diag == only.n_fid == 0 and not only.purity
    with pytest.raises(ValueError, match="outside"):
        pack_dm_observables([ReducedDensityMatrix([3])], n, 1, "cpu")
    none, rows = pack_dm_observables([], n, 1, "cpu")
    assert none is None and rows == []
    res = MasterEquationResult(torch.zeros(0), {})
    assert res.rdms == [] and res.expect == [] and len(tuple(res)) == 2


def test_coherent_results_serve_native_rdms_and_the_stored_rho_route():
    n, dim, n_t = 2, 4, 3
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(n_t, dim, dim, 1, generator=gen, dtype=torch.complex128)
    rho = torch.einsum("tikb,tjkb->tijb", x, x.conj())
    rho = rho / torch.einsum("tiib->tb", rho)[:, None, None, :]
    handed, other = ReducedDensityMatrix([1]), ReducedDensityMatrix([0])
    native = torch.randn(n_t, 1, 2, 2, dtype=torch.complex128, generator=gen)
    times = torch.linspace(0, 1, n_t)
    res = CoherentResults(rho, n, "ground-rydberg", times, "ground-rydberg", density=True, native_rdms=[native], rdm_observables=[handed])
    assert res.reduced_density_matrix(handed) is native
    got = res.reduced_density_matrix(other)  # not handed to run: the torch route on the stored rho
    for k in range(n_t):
        assert np.abs(got[k, 0].numpy() - partial_trace(rho[k, :, :, 0].numpy(), n, (0,))).max() <= 1e-14
    ent = res.entanglement_entropy(other)
    assert ent.shape == (n_t, 1) and torch.allclose(ent, von_neumann_entropy(got, 2))
    pair = ReducedDensityMatrix([0, 1])
    neg = res.negativity(pair, 1)
    assert neg.shape == (n_t, 1) and torch.allclose(neg, negativity(rho.permute(0, 3, 1, 2), 1)) and bool((neg >= 0).all())
    empty = CoherentResults(torch.zeros(0, dim, dim, 1, dtype=torch.complex128), n, "ground-rydberg", times, "ground-rydberg", density=True,
                            native_rdms=[native], rdm_observables=[handed])
    assert empty.reduced_density_matrix(handed) is native
    with pytest.raises(RuntimeError, match="not stored"):
        empty.reduced_density_matrix(other)


# ---- negativity -----------------------------------------------------------------------------------------------------------------
def _singlet():
    psi = torch.tensor([0.0, 1.0, -1.0, 0.0], dtype=torch.complex128) / math.sqrt(2)
    return torch.outer(psi, psi.conj())


@pytest.mark.parametrize("p", [0.2, 1 / 3, 0.7, 1.0])
def test_negativity_of_the_werner_state(p):
    rho = p * _singlet() + (1 - p) * torch.eye(4, dtype=torch.complex128) / 4
    assert abs(float(negativity(rho, 1)) - max(0.0, (3 * p - 1) / 4)) < 1e-14
    assert abs(float(logarithmic_negativity(rho, 1)) - math.log2(1 + 2 * max(0.0, (3 * p - 1) / 4))) < 1e-14


def test_negativity_closed_forms_shapes_and_exports():
    gen = torch.Generator().manual_seed(8)
    a, b = (torch.randn(2, 2, generator=gen, dtype=torch.complex128) for _ in range(2))
    a, b = a @ a.mH, b @ b.mH
    product = torch.kron(a / a.diagonal().sum(), b / b.diagonal().sum())
    assert abs(float(negativity(product, 1))) < 1e-15
    bell = torch.zeros(4, 4, dtype=torch.complex128)
    bell[0, 0] = bell[0, 3] = bell[3, 0] = bell[3, 3] = 0.5
    assert abs(float(negativity(bell, 1)) - 0.5) < 1e-15
    assert abs(float(logarithmic_negativity(bell, 1)) - 1.0) < 1e-14  # one bit
    assert abs(float(logarithmic_negativity(bell, 1, base=math.e)) - math.log(2)) < 1e-14
    # the partial transpose on the leading qubits, entry by entry, on a three-qubit matrix split 1 | 2 and 2 | 1
    m = torch.randn(8, 8, generator=gen, dtype=torch.complex128)
    for n_first in (1, 2):
        d2 = 2 ** (3 - n_first)
        pt = partial_transpose(m, n_first)
        for i in range(8):
            for j in range(8):
                assert pt[i, j] == m[(j // d2) * d2 + i % d2, (i // d2) * d2 + j % d2]
    stack = torch.stack([bell, product]).reshape(2, 1, 4, 4)
    assert negativity(stack, 1).shape == (2, 1)
    # GHZ on three qubits, any 1 | 2 cut: 1/2
    ghz = torch.zeros(8, 8, dtype=torch.complex128)
    ghz[0, 0] = ghz[0, 7] = ghz[7, 0] = ghz[7, 7] = 0.5
    assert abs(float(negativity(ghz, 1)) - 0.5) < 1e-15 and abs(float(negativity(ghz, 2)) - 0.5) < 1e-15
    for bad in (0, 2):
        with pytest.raises(ValueError):
            partial_transpose(bell, bad)
    with pytest.raises(ValueError):
        partial_transpose(torch.zeros(3, 3), 1)
    for name in ("partial_transpose", "negativity", "logarithmic_negativity"):
        assert name in P.__all__ and getattr(P, name) is globals()[name]


def test_negativity_gradcheck_on_a_generic_hermitian_matrix():
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(4, 4, generator=gen, dtype=torch.complex128)
    base = 0.3 * x @ x.mH / (x @ x.mH).diagonal().sum().real + 0.7 * _singlet()  # a negative partial-transpose eigenvalue, no degeneracy
    assert float(negativity(base, 1)) > 1e-2
    re = base.real.clone().requires_grad_(True)
    im = base.imag.clone().requires_grad_(True)

    def herm(f):
        def wrapped(r, i):
            z = torch.complex(r, i)
            return f(0.5 * (z + z.mH), 1)
        return wrapped

    for f in (negativity, logarithmic_negativity):
        assert torch.autograd.gradcheck(herm(f), (re, im), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda r, i: partial_transpose(torch.complex(r, i), 1).abs().pow(2).sum(), (re, im), eps=1e-6, atol=1e-7)
