"""Quantum geometry from the tangent sweep, host side (no GPU): the formula helpers on the Gram matrix against direct dense
computations, the pairing of direction groups into sweeps of at most 8, the C ABI's argument validation (every refusal happens before
anything touches a device) and the refusals of the public route."""
import ctypes
from itertools import combinations

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd.derivative import quantum_fisher_information_all_times
from pulser_diff_amd.geometry import (berry_curvature, geometry_sweeps, quantum_fisher_information, quantum_geometric_tensor)
from tests.test_host_logic import _three_level_emulator
from tests.test_tangent_host import _basic_usage_emulator, _call, _info, _params


# ---- formula helpers -------------------------------------------------------------------------------------------------------------
def _vectors(seed, dim=24, n_dir=5, norm=1.7):
    """psi (deliberately unnormalised, <psi|psi> = norm^2) and n_dir tangents, complex128."""
    gen = torch.Generator().manual_seed(seed)
    psi = torch.randn(dim, generator=gen, dtype=torch.complex128)
    psi = norm * psi / psi.norm()
    dpsi = torch.randn(n_dir, dim, generator=gen, dtype=torch.complex128)
    return psi, dpsi


def _gram(psi, dpsi):
    v = torch.cat([psi[None], dpsi])
    return torch.einsum("iy,jy->ij", v.conj(), v)


def _dense_qgt(psi, dpsi):
    """Q_ij = <d_i psi|(1 - |psi><psi| / N)|d_j psi> / N with the projector as a dense matrix."""
    n2 = float((psi.conj() * psi).real.sum())
    proj = torch.eye(psi.numel(), dtype=torch.complex128) - torch.outer(psi, psi.conj()) / n2
    return torch.einsum("iy,yz,jz->ij", dpsi.conj(), proj, dpsi) / n2


@pytest.mark.parametrize("norm", [1.0, 1.7])
def test_helpers_match_the_dense_projector_form(norm):
    psi, dpsi = _vectors(5, norm=norm)
    gram = _gram(psi, dpsi)
    want = _dense_qgt(psi, dpsi)
    scale = float(want.abs().max())
    assert scale > 1e-2
    assert float((quantum_geometric_tensor(gram) - want).abs().max()) <= 1e-13 * scale
    assert float((quantum_fisher_information(gram) - 4.0 * want.real).abs().max()) <= 4e-13 * scale
    assert float((berry_curvature(gram) + 2.0 * want.imag).abs().max()) <= 2e-13 * scale
    # leading axes pass through
    stacked = torch.stack([gram, 2.0 * gram]).reshape(2, 1, 6, 6)
    assert quantum_fisher_information(stacked).shape == (2, 1, 5, 5)
    assert torch.equal(quantum_fisher_information(stacked)[0, 0], quantum_fisher_information(gram))
    with pytest.raises(ValueError):
        quantum_geometric_tensor(torch.zeros(1, 1, dtype=torch.complex128))


def test_fisher_matrix_is_real_symmetric_positive_semidefinite():
    psi, dpsi = _vectors(6)
    f = quantum_fisher_information(_gram(psi, dpsi))
    assert f.dtype == torch.float64
    scale = float(f.abs().max())
    assert float((f - f.T).abs().max()) <= 1e-14 * scale
    assert float(torch.linalg.eigvalsh(0.5 * (f + f.T)).min()) >= -1e-13 * scale
    b = berry_curvature(_gram(psi, dpsi))
    assert float((b + b.T).abs().max()) <= 1e-14 * float(b.abs().max())  # antisymmetric


def test_fisher_matrix_is_gauge_invariant():
    """d_i psi -> d_i psi + i alpha_i psi (a parameter-dependent global phase) leaves F unchanged."""
    psi, dpsi = _vectors(7)
    alpha = torch.tensor([0.3, -1.1, 2.0, 0.0, 0.7], dtype=torch.float64)
    shifted = dpsi + 1j * alpha[:, None] * psi[None]
    f0, f1 = quantum_fisher_information(_gram(psi, dpsi)), quantum_fisher_information(_gram(psi, shifted))
    assert float((_gram(psi, dpsi) - _gram(psi, shifted)).abs().max()) > 0.1  # the Gram matrices do differ
    assert float((f0 - f1).abs().max()) <= 1e-12 * float(f0.abs().max())


def test_geometric_tensor_is_scale_invariant():
    """psi -> c psi, d psi -> c d psi with a complex c leaves Q unchanged."""
    psi, dpsi = _vectors(8)
    c = 0.4 - 1.3j
    q0, q1 = quantum_geometric_tensor(_gram(psi, dpsi)), quantum_geometric_tensor(_gram(c * psi, c * dpsi))
    assert float((q0 - q1).abs().max()) <= 1e-13 * float(q0.abs().max())


# ---- pairing of direction groups ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dir", range(1, 18))
def test_sweeps_cover_every_pair_of_directions(n_dir):
    sweeps = geometry_sweeps(n_dir)
    assert all(1 <= len(s) <= _native.MAX_TANGENTS and len(set(s)) == len(s) for s in sweeps)
    assert all(0 <= d < n_dir for s in sweeps for d in s)
    if n_dir <= 8:
        assert sweeps == [list(range(n_dir))]
    covered = {(a, b) for s in sweeps for a in s for b in s}
    for d in range(n_dir):
        assert (d, d) in covered  # diagonal blocks
    for a, b in combinations(range(n_dir), 2):
        assert (a, b) in covered and (b, a) in covered
    n_groups = -(-n_dir // 4)
    assert len(sweeps) == (1 if n_dir <= 8 else n_groups * (n_groups - 1) // 2)


def test_sweeps_refuse_zero_directions():
    with pytest.raises(ValueError):
        geometry_sweeps(0)


# ---- C ABI validation --------------------------------------------------------------------------------------------------------------
def _geometry_call(mutate_problem=None, mutate_tangent=None, gram=0x1000, dexpect=0x1000, info=True):
    """rydiff_forward_geometry with host dummies for every device pointer: a call that gets past validation would touch them."""
    call = _call()
    tg = _native.RydTangent()
    tg.n_dir = 2
    tg.d_amp = 0x1000
    if mutate_problem:
        mutate_problem(call.problem)
    if mutate_tangent:
        mutate_tangent(tg)
    plan = _info()
    rc = _native.lib().rydiff_forward_geometry(ctypes.byref(call.problem), ctypes.byref(plan) if info else None, ctypes.byref(tg),
                                               ctypes.c_void_p(0x1000), None, ctypes.c_void_p(dexpect) if dexpect else None,
                                               ctypes.c_void_p(gram) if gram else None, ctypes.c_void_p(0x1000), 0, None)
    _native.check(rc)


def _with_pair(p, keep=[]):
    pair_q = np.array([[0, 1]], dtype=np.uint32)
    pair_t = np.zeros((1, 16), dtype=np.complex128)
    keep += [pair_q, pair_t]
    p.n_pair_terms, p.pair_qubits, p.pair_tables = 1, pair_q.ctypes.data, pair_t.ctypes.data


def test_forward_geometry_validates_before_touching_a_device():
    with pytest.raises(ValueError, match="gram_out"):
        _geometry_call(gram=0)
    for n_dir in (0, -1, _native.MAX_TANGENTS + 1):
        with pytest.raises(ValueError, match="n_dir"):
            _geometry_call(mutate_tangent=lambda t, n=n_dir: setattr(t, "n_dir", n))
    with pytest.raises(ValueError, match="info"):
        _geometry_call(info=False)
    with pytest.raises(ValueError, match="d_amp, d_det, d_u, d_psi0 are NULL"):
        _geometry_call(mutate_tangent=lambda t: setattr(t, "d_amp", None))
    with pytest.raises(NotImplementedError, match="shard"):
        _geometry_call(lambda p: setattr(p, "shard_bits", 1))
    with pytest.raises(NotImplementedError, match="pair terms"):
        _geometry_call(_with_pair)
    with pytest.raises(NotImplementedError, match="conditioned"):
        _geometry_call(lambda p: setattr(p, "amp_conditioned_terms", 1))
    with pytest.raises(NotImplementedError, match="ones-counting"):
        _geometry_call(lambda p: setattr(p, "det_ones_terms", 1))
    with pytest.raises(NotImplementedError, match="shots"):
        _geometry_call(lambda p: setattr(p, "n_shots", 4))
    with pytest.raises(NotImplementedError, match="reduced density"):
        _geometry_call(lambda p: setattr(p, "n_rdms", 1))
    with pytest.raises(NotImplementedError, match="dm_atoms"):
        _geometry_call(lambda p: setattr(p, "dm_atoms", 2))
    # a fully valid call — with and without the row tangents — is stopped by the (host-side) workspace test: nothing launched
    with pytest.raises(MemoryError, match="geometry workspace too small"):
        _geometry_call()
    with pytest.raises(MemoryError, match="geometry workspace too small"):
        _geometry_call(dexpect=0)


def test_geometry_workspace_bytes_is_host_only_and_holds_the_tangent_sweep():
    L = _native.lib()
    call, plan = _call(), _info()
    for d in (1, 2, 5, 8):
        tangent = L.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), d)
        geometry = L.rydiff_geometry_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), d)
        padded = {5: 6, 7: 8}.get(d, d)
        # one block per trajectory at 3 qubits, B = 2: at least one partial of (1 + padded)^2 doubles per trajectory behind the sweep's
        assert tangent > 0 and geometry >= tangent + 2 * (1 + padded) ** 2 * 8
    assert L.rydiff_geometry_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), 9) == 0
    assert "n_dir" in _native.last_error()
    assert L.rydiff_geometry_workspace_bytes(ctypes.byref(call.problem), None, 2) == 0
    call.problem.shard_bits = 1
    assert L.rydiff_geometry_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(plan), 1) == 0
    assert "not implemented" in _native.last_error()


# ---- public refusals ---------------------------------------------------------------------------------------------------------------
def test_run_quantum_fisher_refusals():
    prm = _params()
    args = (prm["q0"], prm["omega"], prm["area"], prm["phase"])
    emu = _basic_usage_emulator(*args)
    with pytest.raises(ValueError, match="deriv_time"):
        emu.run_quantum_fisher([prm["omega"], emu.evaluation_times])
    with pytest.raises(TypeError):
        quantum_fisher_information_all_times(emu, [])
    with pytest.raises(ValueError, match="shape"):
        emu.run_quantum_fisher([prm["omega"]], [P.DiagonalObservable(torch.ones(8, dtype=torch.float64))])
    with pytest.raises(NotImplementedError, match="master-equation"):
        emu.run_quantum_fisher([prm["omega"]], solver=P.SolverType.DP5_ME)
    dephasing = _basic_usage_emulator(*args, config=P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="density matrix"):
        quantum_fisher_information_all_times(dephasing, [prm["omega"]])
    doppler = _basic_usage_emulator(*args, config=P.SimConfig(noise="doppler", runs=2, temperature=50.0))
    with pytest.raises(NotImplementedError, match="average"):
        doppler.run_quantum_fisher([prm["omega"]])
    three, _ = _three_level_emulator()
    leaf = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="three-level"):
        three.run_quantum_fisher([leaf])
