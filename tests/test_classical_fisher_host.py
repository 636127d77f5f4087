"""Classical Fisher information of the occupation-basis measurement, host side (no GPU): the two exports and their argument validation
(every refusal happens before anything touches a device), the workspace region of the block partials, ``observables.classical_gram``
against a brute-force loop, ``geometry.classical_fisher_information`` against central finite differences of the distribution, the
invariants of F_C (symmetric, positive semidefinite, below F_Q, scale-invariant, the zero rule), the assembly of more than 8
directions and the refusals of the public route."""
import ctypes
import math

import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd.derivative import classical_fisher_information_all_times
from pulser_diff_amd.geometry import (MeasurementFisher, classical_fisher_information, fisher_efficiency, geometry_sweeps,
                                      place_sweep_block, quantum_fisher_information)
from pulser_diff_amd.observables import classical_gram
from tests.test_geometry_host import _with_pair
from tests.test_host_logic import _emulator_for_basis, _three_level_emulator
from tests.test_tangent_host import _basic_usage_emulator, _call, _info, _params


# ---- C ABI validation --------------------------------------------------------------------------------------------------------------
def _fisher_call(mutate_problem=None, mutate_tangent=None, cgram=0x1000, gram=0x1000, dexpect=0x1000, info=True):
    """rydiff_forward_fisher with host dummies for every device pointer: a call that gets past validation would touch them."""
    call = _call()
    tg = _native.RydTangent()
    tg.n_dir = 2
    tg.d_amp = 0x1000
    if mutate_problem:
        mutate_problem(call.problem)
    if mutate_tangent:
        mutate_tangent(tg)
    plan = _info()
    opt = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    rc = _native.lib().rydiff_forward_fisher(ctypes.byref(call.problem), ctypes.byref(plan) if info else None, ctypes.byref(tg),
                                             ctypes.c_void_p(0x1000), None, opt(dexpect), opt(gram), opt(cgram), ctypes.c_void_p(0x1000), 0,
                                             None)
    _native.check(rc)


def test_exports_exist():
    L = _native.lib()
    assert "rydiff_forward_fisher" in _native.EXPORTS and "rydiff_fisher_workspace_bytes_flags" in _native.EXPORTS
    assert L.rydiff_forward_fisher.restype is ctypes.c_int and L.rydiff_fisher_workspace_bytes_flags.restype is ctypes.c_size_t
    for name in ("MeasurementFisher", "classical_fisher_information", "fisher_efficiency"):
        assert name in P.__all__
    assert P.MeasurementFisher is MeasurementFisher and P.classical_fisher_information is classical_fisher_information


def test_forward_fisher_validates_before_touching_a_device():
    with pytest.raises(ValueError, match="cgram_out"):
        _fisher_call(cgram=0)
    for n_dir in (0, -1, _native.MAX_TANGENTS + 1):
        with pytest.raises(ValueError, match="n_dir"):
            _fisher_call(mutate_tangent=lambda t, n=n_dir: setattr(t, "n_dir", n))
    with pytest.raises(ValueError, match="info"):
        _fisher_call(info=False)
    with pytest.raises(ValueError, match="d_amp, d_det, d_u, d_psi0 are NULL"):
        _fisher_call(mutate_tangent=lambda t: setattr(t, "d_amp", None))
    with pytest.raises(ValueError, match="unknown bits"):
        _fisher_call(mutate_tangent=lambda t: setattr(t, "flags", 128))
    with pytest.raises(ValueError, match="unknown bits"):
        _fisher_call(mutate_tangent=lambda t: setattr(t, "flags", 1 << 20))
    with pytest.raises(NotImplementedError, match="dm_atoms"):
        _fisher_call(lambda p: setattr(p, "dm_atoms", 2))
    with pytest.raises(NotImplementedError, match="dm_atoms"):  # whatever the flags
        _fisher_call(lambda p: setattr(p, "dm_atoms", 2), lambda t: setattr(t, "flags", _native.TANGENT_DENSITY_MATRIX))
    with pytest.raises(NotImplementedError, match="shard"):
        _fisher_call(lambda p: setattr(p, "shard_bits", 1))
    with pytest.raises(NotImplementedError, match="shots"):
        _fisher_call(lambda p: setattr(p, "n_shots", 4))
    with pytest.raises(NotImplementedError, match="conditioned"):
        _fisher_call(lambda p: setattr(p, "amp_conditioned_terms", 1))
    with pytest.raises(NotImplementedError, match="ones-counting"):
        _fisher_call(lambda p: setattr(p, "det_ones_terms", 1))
    with pytest.raises(NotImplementedError, match="pair terms"):
        _fisher_call(_with_pair)
    with pytest.raises(NotImplementedError, match="reduced density"):
        _fisher_call(lambda p: setattr(p, "n_rdms", 1))
    # a fully valid call — with and without the Gram matrix and the row tangents — is stopped by the (host-side) workspace test
    with pytest.raises(MemoryError, match="fisher workspace too small: need"):
        _fisher_call()
    with pytest.raises(MemoryError, match="fisher workspace too small"):
        _fisher_call(gram=0)
    with pytest.raises(MemoryError, match="fisher workspace too small"):
        _fisher_call(dexpect=0, gram=0)


@pytest.mark.parametrize("n", [3, 13])
def test_fisher_workspace_is_the_geometry_workspace_plus_the_partial_region(n):
    L = _native.lib()
    batch = 2
    call, plan = _call(n, batch), _info()
    blocks = min((2**n + 255) // 256, 1024)
    for d in (1, 5, 8):
        geometry = L.rydiff_geometry_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(plan), d, 0)
        fisher = L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(plan), d, 0)
        npad = 1 + {5: 6, 7: 8}.get(d, d)
        region = blocks * batch * (npad * (npad + 1) // 2) * 8  # one upper triangle per block and trajectory (include/rydiff.h)
        assert geometry > 0 and fisher >= geometry
        assert fisher - geometry == (region + 255) // 256 * 256
    assert L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(plan), 9, 0) == 0
    assert "n_dir" in _native.last_error()
    assert L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(call.problem), None, 2, 0) == 0
    assert L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(plan), 2, 128) == 0
    call.problem.dm_atoms = 1
    assert L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(plan), 1, _native.TANGENT_DENSITY_MATRIX) == 0


# ---- classical_gram -----------------------------------------------------------------------------------------------------------------
def _vectors(seed, dim=8, n_dir=3, norm=1.7):
    gen = torch.Generator().manual_seed(seed)
    psi = torch.randn(dim, generator=gen, dtype=torch.complex128)
    psi = norm * psi / psi.norm()
    dpsi = torch.randn(n_dir, dim, generator=gen, dtype=torch.complex128)
    return psi, dpsi


def _gram(psi, dpsi):
    v = torch.cat([psi[None], dpsi])
    return torch.einsum("iy,jy->ij", v.conj(), v)


def _loop_cgram(psi, dpsi):
    """C in a plain Python loop over the amplitudes, from the definition."""
    n = 1 + dpsi.shape[0]
    c = [[0.0] * n for _ in range(n)]
    for y in range(psi.shape[0]):
        a = complex(psi[y])
        mod = abs(a)
        if mod == 0.0:
            continue
        u = a / mod
        w = [mod] + [2.0 * (u.conjugate() * complex(dpsi[d, y])).real for d in range(n - 1)]
        for i in range(n):
            for j in range(n):
                c[i][j] += w[i] * w[j]
    return torch.tensor(c, dtype=torch.float64)


def test_classical_gram_matches_the_loop_at_three_qubits():
    psi, dpsi = _vectors(11)
    psi[5] = 0.0  # the zero rule in both
    got, want = classical_gram(psi, dpsi), _loop_cgram(psi, dpsi)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, 4)
    assert float(want.abs().max()) > 1e-1
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    assert torch.equal(got, got.T)
    # C_00 = <psi|psi>, C_0d = d<psi|psi> = 2 Re <psi|dpsi_d>
    g = _gram(psi, dpsi)
    assert abs(float(got[0, 0]) - float(g[0, 0].real)) <= 1e-14 * float(g[0, 0].real)
    assert float((got[0, 1:] - 2.0 * g[0, 1:].real).abs().max()) <= 1e-14 * float(g.abs().max())
    # leading axes
    stacked = classical_gram(torch.stack([psi, 2.0 * psi])[:, None], torch.stack([dpsi, dpsi])[:, None])
    assert tuple(stacked.shape) == (2, 1, 4, 4) and torch.equal(stacked[0, 0], got)
    with pytest.raises(ValueError):
        classical_gram(psi, dpsi[0])
    with pytest.raises(TypeError):
        classical_gram(psi.real, dpsi)
    with pytest.raises(ValueError):
        classical_fisher_information(torch.zeros(1, 1, dtype=torch.float64))
    with pytest.raises(TypeError):
        classical_fisher_information(g)


def test_classical_gram_neither_overflows_nor_underflows():
    psi, dpsi = _vectors(12)
    for scale in (1e-170, 1e150):
        c = classical_gram(scale * psi, scale * dpsi)
        assert bool(torch.isfinite(c).all())
    tiny = classical_gram(1e-170 * psi, dpsi)  # w_0 underflows in the products, w_d stays O(1)
    ref = classical_gram(psi, dpsi)
    assert float((tiny[1:, 1:] - ref[1:, 1:]).abs().max()) <= 1e-13 * float(ref.abs().max())


def test_classical_fisher_information_matches_central_differences():
    """psi(theta) = psi_0 + theta_1 a + theta_2 b with a, b smooth (low Fourier modes over the index), orthogonal to each other:
    F_C from classical_gram at theta = 0 against central differences of p_theta(y) = |psi_theta[y]|^2 / <psi_theta|psi_theta>.
    p is a ratio of quadratics in theta: the central difference with h = 1e-5 is off by O(h^2) ~ 1e-10 relative and by rounding
    eps / h ~ 1e-11; the bar is 1e-8 of the largest entry."""
    gen = torch.Generator().manual_seed(2024)
    psi0 = torch.randn(8, generator=gen, dtype=torch.complex128)
    psi0 = psi0 / psi0.norm()
    y = torch.arange(8, dtype=torch.float64)
    a = torch.cos(2 * math.pi * y / 8) * torch.exp(0.3j * y)
    b = torch.sin(2 * math.pi * y / 8) * torch.exp(0.3j * y)
    assert abs(complex(torch.vdot(a, b))) <= 1e-14  # orthogonal
    a, b = 0.5 * a / a.norm(), 0.5 * b / b.norm()
    h = 1e-5
    # no amplitude crosses zero inside the difference window
    assert float(psi0.abs().min()) > 1e3 * h * float(torch.maximum(a.abs(), b.abs()).max())

    def prob(t1, t2):
        psi = psi0 + t1 * a + t2 * b
        p = psi.real**2 + psi.imag**2
        return p / p.sum()

    dp = torch.stack([(prob(h, 0.0) - prob(-h, 0.0)) / (2 * h), (prob(0.0, h) - prob(0.0, -h)) / (2 * h)])
    want = torch.einsum("dy,ey,y->de", dp, dp, 1.0 / prob(0.0, 0.0))
    got = classical_fisher_information(classical_gram(psi0, torch.stack([a, b])))
    scale = float(want.abs().max())
    assert scale > 1e-2
    assert float((got - want).abs().max()) <= 1e-8 * scale


# ---- invariants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [21, 22, 23])
def test_invariants_on_random_unnormalised_vectors(seed):
    psi, dpsi = _vectors(seed)
    fc = classical_fisher_information(classical_gram(psi, dpsi))
    fq = quantum_fisher_information(_gram(psi, dpsi))
    scale = float(fq.abs().max())
    assert float(fc.abs().max()) > 1e-2
    assert float((fc - fc.T).abs().max()) <= 1e-14 * scale
    assert float(torch.linalg.eigvalsh(0.5 * (fc + fc.T)).min()) >= -1e-13 * scale
    gap = fq - fc
    assert float(torch.linalg.eigvalsh(0.5 * (gap + gap.T)).min()) >= -1e-12 * float(torch.linalg.matrix_norm(fq))
    # a common complex factor leaves F_C unchanged
    c = 0.4 - 1.3j
    scaled = classical_fisher_information(classical_gram(c * psi, c * dpsi))
    assert float((scaled - fc).abs().max()) <= 1e-13 * float(fc.abs().max())
    # the efficiency: per diagonal entry and along a direction, in [0, 1]
    eff = fisher_efficiency(classical_gram(psi, dpsi), _gram(psi, dpsi))
    assert tuple(eff.shape) == (3,) and bool(((eff >= 0) & (eff <= 1 + 1e-12)).all())
    n = torch.tensor([0.3, -1.0, 0.5], dtype=torch.float64)
    along = fisher_efficiency(classical_gram(psi, dpsi), _gram(psi, dpsi), direction=n)
    assert along.ndim == 0 and abs(float(along) - float(n @ fc @ n) / float(n @ fq @ n)) <= 1e-14
    with pytest.raises(ValueError):
        fisher_efficiency(classical_gram(psi, dpsi), _gram(psi, dpsi), direction=n[:2])


def test_zero_amplitude_contributes_nothing():
    psi, dpsi = _vectors(31)
    psi[2] = 0.0
    assert float(dpsi[:, 2].abs().min()) > 0.0
    with_tangent = classical_gram(psi, dpsi)
    dpsi0 = dpsi.clone()
    dpsi0[:, 2] = 0.0
    assert torch.equal(with_tangent, classical_gram(psi, dpsi0))
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert float((with_tangent - classical_gram(psi[keep], dpsi[:, keep])).abs().max()) <= 1e-14 * float(with_tangent.abs().max())


def test_efficiency_is_nan_where_nothing_depends_on_the_parameter():
    psi, dpsi = _vectors(41, n_dir=2)
    dpsi[1] = 0.0
    eff = fisher_efficiency(classical_gram(psi, dpsi), _gram(psi, dpsi))
    assert 0.0 <= float(eff[0]) <= 1.0 + 1e-12 and math.isnan(float(eff[1]))


# ---- more than 8 directions -----------------------------------------------------------------------------------------------------------
def test_ten_directions_fill_every_block():
    """The assembly evolve_fisher and evolve_geometry share: every sweep of geometry_sweeps(10) hands in the matrix of its own
    directions; the full 11 x 11 matrix comes out with every (d, e) block filled."""
    psi, dpsi = _vectors(51, n_dir=10)
    want = classical_gram(psi, dpsi).expand(2, 1, 11, 11).contiguous()
    full = torch.full((2, 1, 11, 11), float("nan"), dtype=torch.float64)
    sweeps = geometry_sweeps(10)
    assert len(sweeps) == 3
    for idx in sweeps:
        block = classical_gram(psi, dpsi[idx])  # what the sweep over `idx` returns: the same sums up to their order
        sel = [0] + [1 + d for d in idx]
        assert float((block - want[0, 0][sel][:, sel]).abs().max()) <= 1e-13 * float(want.abs().max())
        place_sweep_block(full, idx, want[:, :, sel][:, :, :, sel].clone())
    assert bool(torch.isfinite(full).all()) and torch.equal(full, want)


# ---- public refusals ---------------------------------------------------------------------------------------------------------------
def test_run_classical_fisher_refusals():
    prm = _params()
    args = (prm["q0"], prm["omega"], prm["area"], prm["phase"])
    emu = _basic_usage_emulator(*args)
    with pytest.raises(ValueError, match="run_classical_fisher.*deriv_time"):
        emu.run_classical_fisher([prm["omega"], emu.evaluation_times])
    with pytest.raises(TypeError):
        classical_fisher_information_all_times(emu, [])
    with pytest.raises(ValueError, match="shape"):
        emu.run_classical_fisher([prm["omega"]], [P.DiagonalObservable(torch.ones(8, dtype=torch.float64))])
    with pytest.raises(NotImplementedError, match="run_classical_fisher does not take OccupationCorrelations"):
        emu.run_classical_fisher([prm["omega"]], [P.OccupationCorrelations()])
    with pytest.raises(NotImplementedError, match="run_classical_fisher is not available for master-equation"):
        emu.run_classical_fisher([prm["omega"]], solver=P.SolverType.DP5_ME)
    dephasing = _basic_usage_emulator(*args, config=P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="run_classical_fisher.*density matrix"):
        classical_fisher_information_all_times(dephasing, [prm["omega"]])
    doppler = _basic_usage_emulator(*args, config=P.SimConfig(noise="doppler", runs=2, temperature=50.0))
    with pytest.raises(NotImplementedError, match="run_classical_fisher.*average.*run_classical_fisher"):
        doppler.run_classical_fisher([prm["omega"]])
    xy, _ = _emulator_for_basis("XY")
    with pytest.raises(NotImplementedError, match="run_classical_fisher is not available with the XY exchange"):
        xy.run_classical_fisher([torch.tensor([1.0], dtype=torch.float64, requires_grad=True)])
    three, _ = _three_level_emulator()
    leaf = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="run_classical_fisher.*three-level"):
        three.run_classical_fisher([leaf])
