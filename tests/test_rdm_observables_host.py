"""Reduced density matrices without a GPU: the ReducedDensityMatrix object, its torch route against an independent partial trace,
the identities the solver layer relies on (cotangent formula, rotating frame, row layout), entropies, the ABI mirror and the
validation in front of the device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd.observables import MAX_RDM_QUBITS, MAX_RDMS, ReducedDensityMatrix, pack_rdms, reduced_density_matrix
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, _check_shapes, frame_factor, split_expect, split_observables
from pulser_diff_amd.utils import purity, von_neumann_entropy


def _kets(n, batch, seed, n_t=3):
    v = torch.randn(n_t, 2**n, batch, generator=torch.Generator().manual_seed(seed), dtype=torch.complex128)
    return v / v.norm(dim=1, keepdim=True)


def _partial_trace(states, qubits):
    """Independent route: numpy, one axis per qubit, einsum over explicitly named axes."""
    st = states.numpy()
    n_t, dim, batch = st.shape
    n = int(round(math.log2(dim)))
    m = len(qubits)
    out = np.zeros((n_t, batch, 2**m, 2**m), dtype=np.complex128)
    letters = "abcdefghijklmnop"
    for t in range(n_t):
        for b in range(batch):
            psi = st[t, :, b].reshape((2,) * n)
            bra = list(letters[:n])
            ket = [letters[n + qubits.index(q)] if q in qubits else letters[q] for q in range(n)]
            res = [letters[n + i] for i in range(m)] + [letters[q] for q in qubits]  # (ket-side a', bra-side a)
            rho = np.einsum("".join(bra) + "," + "".join(ket) + "->" + "".join(res), psi, psi.conj())
            out[t, b] = rho.reshape(2**m, 2**m).T  # rho[a][a'] = sum psi[a, e] conj psi[a', e]
    return out


def test_object_properties_and_validation():
    o = ReducedDensityMatrix((5, 1, 3))
    assert o.n_sub == 3 and o.shape == (8, 8) and o.is_sparse is False and o.mask == 0b101010 and o.qubits == (5, 1, 3)
    assert "ReducedDensityMatrix" in P.__all__
    assert MAX_RDMS == _native.MAX_RDMS == 8 and MAX_RDM_QUBITS == _native.MAX_RDM_QUBITS == 6
    with pytest.raises(ValueError):  # duplicate qubits
        ReducedDensityMatrix((1, 2, 1))
    with pytest.raises(ValueError):  # m = 7
        ReducedDensityMatrix(range(7))
    with pytest.raises(ValueError):
        ReducedDensityMatrix(())
    with pytest.raises(ValueError):
        ReducedDensityMatrix((-1, 2))
    with pytest.raises(ValueError):  # index >= N
        pack_rdms([ReducedDensityMatrix((0, 4))], 4)
    with pytest.raises(ValueError):
        reduced_density_matrix(ReducedDensityMatrix((0, 4)), _kets(4, 1, 0))
    pack_rdms([o] * MAX_RDMS, 6)
    with pytest.raises(ValueError):  # 9 RDMs
        pack_rdms([o] * (MAX_RDMS + 1), 6)
    with pytest.raises(TypeError):
        pack_rdms([(0, 1)], 4)
    with pytest.raises(ValueError):
        pack_rdms([], 4)


def test_pack_rdms_masks():
    masks = pack_rdms([ReducedDensityMatrix((0,)), ReducedDensityMatrix((5, 1, 3)), ReducedDensityMatrix((2, 0))], 6)
    assert masks.dtype == np.uint32 and masks.tolist() == [0b1, 0b101010, 0b101]


@pytest.mark.parametrize("n,qubits", [(5, (2,)), (5, (4, 0)), (6, (5, 1, 3)), (6, (0, 1, 2, 3, 4, 5)), (4, (3, 2, 1, 0)), (7, (6, 0, 3, 2, 5, 1)),
                                      (1, (0,))])
def test_torch_route_against_an_independent_partial_trace(n, qubits):
    """Scrambled orders, A = the whole register, m = 1; Hermitian, trace = |psi|^2."""
    st = _kets(n, 2, 10 + n) * torch.tensor([1.0, 0.7])[None, None, :]  # second trajectory not normalised
    got = reduced_density_matrix(ReducedDensityMatrix(qubits), st)
    assert got.shape == (3, 2, 2 ** len(qubits), 2 ** len(qubits)) and got.dtype == torch.complex128
    assert np.abs(got.numpy() - _partial_trace(st, list(qubits))).max() < 1e-14
    assert (got - got.mH).abs().max().item() < 1e-15
    tr = torch.einsum("tbaa->tb", got)
    assert (tr.real - (st.abs() ** 2).sum(1)).abs().max().item() < 1e-14 and tr.imag.abs().max().item() < 1e-15


def test_native_index_is_the_permutation_from_ascending_order():
    """What split_observables does with the library's rows: ascending order -> the user's."""
    st = _kets(6, 1, 3)
    user = ReducedDensityMatrix((5, 1, 3))
    asc = reduced_density_matrix(ReducedDensityMatrix((1, 3, 5)), st)
    perm = user.native_index()
    assert sorted(perm.tolist()) == list(range(8))
    assert (asc.index_select(2, perm).index_select(3, perm) - reduced_density_matrix(user, st)).abs().max().item() < 1e-15
    assert ReducedDensityMatrix((0, 2, 4)).native_index().tolist() == list(range(8))


def test_split_observables_row_layout():
    """Entry (a, a') of RDM o at row first_o + 2 (a 2^m + a'), Re then Im, behind the overlap rows; split_expect is unchanged."""
    n_t, batch = 2, 3
    rdms = [ReducedDensityMatrix((1,)), ReducedDensityMatrix((3, 0))]
    rows = 2 + 2 * 1 + 2 * 4 + 2 * 16
    expect = torch.arange(rows * n_t * batch, dtype=torch.float64).reshape(rows, n_t, batch)
    real, ov, rho = split_observables(expect, 1, rdms)
    assert torch.equal(real, expect[:2]) and torch.equal(ov[0], torch.complex(expect[2], expect[3]))
    assert rho[0].shape == (n_t, batch, 2, 2) and rho[1].shape == (n_t, batch, 4, 4)
    assert torch.equal(rho[0][:, :, 1, 0], torch.complex(expect[4 + 2 * 2], expect[4 + 2 * 2 + 1]))
    # qubits (3, 0): user index a = 2 b3 + b0, native index = 2 b0 + b3
    assert torch.equal(rho[1][:, :, 0b10, 0b01], torch.complex(expect[12 + 2 * (0b01 * 4 + 0b10)], expect[12 + 2 * (0b01 * 4 + 0b10) + 1]))
    r2, o2, none = split_observables(expect[:4], 1, None)
    assert none is None and torch.equal(r2, split_expect(expect[:4], 1)[0]) and torch.equal(o2, ov)
    _, _, by_mask = split_observables(expect, 1, [0b10, 0b1001])  # masks: ascending order, no permutation
    assert torch.equal(by_mask[1][:, :, 1, 2], torch.complex(expect[12 + 2 * 6], expect[12 + 2 * 6 + 1]))


def test_bell_pair_in_a_larger_register_and_product_state():
    n = 5
    bell = torch.zeros(2**n, dtype=torch.complex128)  # qubits 1 and 3 in (|00> + |11>)/sqrt 2, the others in |1>, |0>, |1>
    for b in (0, 1):
        bits = [1, b, 0, b, 1]
        bell[int("".join(map(str, bits)), 2)] = 2 ** -0.5
    st = bell[None, :, None]
    s1 = von_neumann_entropy(reduced_density_matrix(ReducedDensityMatrix((1,)), st))
    assert abs(s1.item() - 1.0) < 1e-14
    assert abs(von_neumann_entropy(reduced_density_matrix(ReducedDensityMatrix((3, 0)), st)).item() - 1.0) < 1e-14
    assert abs(von_neumann_entropy(reduced_density_matrix(ReducedDensityMatrix((3, 1)), st)).item()) < 1e-14  # the pair itself is pure
    assert abs(von_neumann_entropy(reduced_density_matrix(ReducedDensityMatrix((1,)), st), base=math.e).item() - math.log(2)) < 1e-14
    g = torch.Generator().manual_seed(5)
    single = [torch.randn(2, generator=g, dtype=torch.complex128) for _ in range(4)]
    prod = single[0]
    for v in single[1:]:
        prod = torch.kron(prod, v)
    prod = (prod / prod.norm())[None, :, None]
    for qubits in ((0,), (2, 1), (3, 0, 1)):
        rho = reduced_density_matrix(ReducedDensityMatrix(qubits), prod)
        assert von_neumann_entropy(rho).abs().item() < 1e-12 and abs(purity(rho).item() - 1.0) < 1e-14


def test_purity_of_the_whole_register_is_one():
    st = _kets(4, 2, 8)
    rho = reduced_density_matrix(ReducedDensityMatrix((2, 0, 3, 1)), st)
    assert (purity(rho) - 1.0).abs().max().item() < 1e-14
    mixed = torch.eye(4, dtype=torch.complex128) / 4
    assert abs(purity(mixed).item() - 0.25) < 1e-15 and abs(von_neumann_entropy(mixed).item() - 2.0) < 1e-14


@pytest.mark.parametrize("n,qubits", [(3, (1,)), (5, (4, 0, 2)), (6, (5, 1, 3, 0, 4, 2)), (7, (6, 2, 0, 5, 1, 3))])
def test_autograd_of_the_torch_route_is_the_cotangent_the_library_forms(n, qubits):
    """Every entry an independent output: with G = gRe + i gIm the cotangent of psi is ((G + G^dagger)_A (x) 1_E) psi."""
    m = len(qubits)
    g = torch.Generator().manual_seed(n)
    psi = torch.randn(1, 2**n, 1, generator=g, dtype=torch.complex128, requires_grad=True)
    G = torch.randn(2**m, 2**m, generator=g, dtype=torch.complex128)
    rho = reduced_density_matrix(ReducedDensityMatrix(qubits), psi)[0, 0]
    ((G.real * rho.real).sum() + (G.imag * rho.imag).sum()).backward()
    rest = [q for q in range(n) if q not in qubits]
    t = psi.detach()[0, :, 0].reshape((2,) * n).permute(list(qubits) + rest).reshape(2**m, -1)
    want = ((G + G.mH) @ t).reshape((2,) * n).permute(list(np.argsort(list(qubits) + rest))).reshape(-1)
    assert (psi.grad[0, :, 0] - want).abs().max().item() < 1e-13


def test_frame_factor_on_a_hand_made_example():
    """V = exp(i phi ones): rho of V psi times the factor is rho of psi."""
    phi = 0.37
    f = frame_factor(1, phi)
    assert f[0, 0] == 1 and f[1, 1] == 1 and abs(f[0, 1] - np.exp(1j * phi)) < 1e-15 and abs(f[1, 0] - np.exp(-1j * phi)) < 1e-15
    n = 4
    st = _kets(n, 1, 2)
    ones = torch.tensor([bin(x).count("1") for x in range(2**n)], dtype=torch.float64)
    framed = st * torch.exp(1j * phi * ones)[None, :, None]
    for qubits in ((2,), (3, 0), (1, 2, 0)):
        o = ReducedDensityMatrix(qubits)
        lab = reduced_density_matrix(o, framed) * frame_factor(o.n_sub, phi)
        assert (lab - reduced_density_matrix(o, st)).abs().max().item() < 1e-15
        assert (reduced_density_matrix(o, framed) - reduced_density_matrix(o, st)).abs().max().item() > 1e-3


def _spec(n, rdms):
    return ProblemSpec(n_qubits=n, dt=0.001, n_samples=4, amp_masks=(2**n - 1,), det_masks=(), solver=SolverType.KRYLOV_SE, rdms=rdms)


def test_abi_mirror_and_the_fields_the_call_fills():
    L = _native.lib()
    assert L.rydiff_sizeof_problem() == ctypes.sizeof(_native.RydProblem)
    names = [f[0] for f in _native.RydProblem._fields_]
    assert names.index("n_rdms") + 1 == names.index("rdm_masks") and names.index("rdm_masks") < names.index("n_overlaps")  # in front of the overlap block
    assert names[-1] == "pauli_w"  # the Pauli block stays the tail
    n = 4
    spec = _spec(n, [ReducedDensityMatrix((3, 0)), ReducedDensityMatrix((1,))])
    assert spec.rdm_rows() == 2 * 16 + 2 * 4
    amp = torch.zeros(1, 1, 4, dtype=torch.complex128)
    call = _Call(spec, amp, torch.zeros(1, 0, 4), torch.zeros(6), np.linspace(0, 0.003, 3), 1, None)
    assert call.problem.n_rdms == 2 and call.rdm_masks.tolist() == [0b1001, 0b10]
    assert _Call(_spec(n, None), amp, torch.zeros(1, 0, 4), torch.zeros(6), np.linspace(0, 0.003, 3), 1, None).problem.n_rdms == 0


def _raw_call(n=8, masks=(0b101,)):
    """A _Call whose rdm fields are then set by hand (past the Python validation).  HOST tensors: validation follows no pointer."""
    amp = torch.zeros(1, 1, 4, dtype=torch.complex128)
    call = _Call(_spec(n, None), amp, torch.zeros(1, 0, 4), torch.zeros(n * (n - 1) // 2), np.linspace(0, 0.003, 3), 2, None)
    call.rdm_masks = np.asarray(masks, dtype=np.uint32)
    call.problem.n_rdms = len(masks)
    call.problem.rdm_masks = call.rdm_masks.ctypes.data
    return call


def test_rydiff_plan_rejects_bad_rdm_fields():
    """plan.hpp: build_rdms runs with the other field checks, before anything touches a device."""
    L = _native.lib()
    scratch = (ctypes.c_char * _native.PLAN_SCRATCH_BYTES)()

    def plan(call):
        _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.cast(scratch, ctypes.c_void_p), None, ctypes.byref(_native.RydPlanInfo())))

    with pytest.raises(ValueError, match="empty"):
        plan(_raw_call(masks=(0b11, 0)))
    with pytest.raises(ValueError, match="more than 6"):
        plan(_raw_call(masks=(0b1111111,)))
    with pytest.raises(ValueError, match="outside the register"):
        plan(_raw_call(masks=(1 << 8,)))
    with pytest.raises(ValueError, match="n_rdms"):
        plan(_raw_call(masks=(1,) * 9))
    bad = _raw_call()
    bad.problem.n_rdms = -1
    with pytest.raises(ValueError, match="n_rdms"):
        plan(bad)
    bad = _raw_call()
    bad.problem.rdm_masks = None
    with pytest.raises(ValueError, match="rdm_masks"):
        plan(bad)
    sharded = _raw_call()
    sharded.problem.shard_bits = 1
    with pytest.raises(NotImplementedError, match="reduced density"):
        plan(sharded)


def test_tangent_entry_points_refuse_rdms():
    from pulser_diff_amd.solver import evolve_tangent

    L = _native.lib()
    call = _raw_call()
    info = _native.RydPlanInfo()
    assert L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0
    assert "reduced density" in _native.last_error()
    tg = _native.RydTangent()
    tg.n_dir = 1
    rc = L.rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), None, None, None, None, 0, None)
    assert rc == _native.RYDIFF_ENOTIMPL and "reduced density" in _native.last_error()
    amp = torch.zeros(1, 1, 4, dtype=torch.complex128)
    with pytest.raises(NotImplementedError, match="reduced density"):  # before the device is looked at
        evolve_tangent(amp, torch.zeros(1, 0, 4), torch.zeros(6), torch.linspace(0, 0.003, 3), torch.zeros(1, 16, dtype=torch.complex128),
                       _spec(4, [ReducedDensityMatrix((0,))]), d_amp=amp[None])


def test_python_validation_in_front_of_the_device():
    n = 4
    amp, det, u = torch.zeros(1, 1, 4, dtype=torch.complex128), torch.zeros(1, 0, 4), torch.zeros(6)
    _check_shapes(_spec(n, [ReducedDensityMatrix((0, 3))]), amp, det, u, None, 1)
    _check_shapes(_spec(n, [0b1001]), amp, det, u, None, 1)
    for bad in ([ReducedDensityMatrix((0, 4))], [0], [1 << 4], [ReducedDensityMatrix((0,))] * 9, [1] * 9):
        with pytest.raises(ValueError):
            _check_shapes(_spec(n, bad), amp, det, u, None, 1)
    with pytest.raises(ValueError):
        _check_shapes(_spec(8, [0b1111111]), torch.zeros(1, 1, 4, dtype=torch.complex128), det, torch.zeros(28), None, 1)
