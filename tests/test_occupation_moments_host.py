"""Occupation correlations (RydProblem.bit_moments), the host side: the struct handshake, the torch route against a brute-force loop
over basis states, the row order, the conversions on states with known correlations, every refusal in front of the device, and the
row count of a call."""
import ctypes
import itertools
import re

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.observables import (OccupationCorrelations, ReducedDensityMatrix, moment_pair_row, moment_rows, occupation_moments)
from pulser_diff_amd.simresults import CoherentResults
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, split_moments, split_observables
from pulser_diff_amd.utils import (connected_correlations, occupation_correlations_from_moments, occupations_from_moments,
                                   structure_factor)


def test_the_observable_is_exported():
    assert "OccupationCorrelations" in P.__all__ and P.OccupationCorrelations is OccupationCorrelations


def test_ctypes_mirror_carries_the_field_where_the_header_has_it():
    names = [f[0] for f in _native.RydProblem._fields_]
    at = names.index("bit_moments")
    assert names[at - 1] == "shots_out" and names[at + 1] == "n_rdms"
    assert ctypes.sizeof(_native.RydProblem) == _native.lib().rydiff_sizeof_problem()
    header = (_native._CSRC.parent.parent / "include" / "rydiff.h").read_text()
    fields = re.findall(r"^\s+(?:const\s+)?\w+\*?\s+\*?(\w+);", header[header.index("typedef struct RydProblem"):header.index("} RydProblem;")],
                        flags=re.M)
    assert fields[fields.index("bit_moments") - 1] == "shots_out" and fields[fields.index("bit_moments") + 1] == "n_rdms"
    # the pins of the neighbouring blocks hold
    assert names.index("n_rdms") + 1 == names.index("rdm_masks") and names[-1] == "pauli_w"


def _brute_force(states: torch.Tensor) -> torch.Tensor:
    """S, B_q, B_qr by a loop over basis states: (rows, n_t, B)."""
    n_t, dim, batch = states.shape
    n = dim.bit_length() - 1
    out = torch.zeros(moment_rows(n), n_t, batch, dtype=torch.float64)
    for y in range(dim):
        p = states[:, y, :].abs() ** 2
        bits = [(y >> (n - 1 - q)) & 1 for q in range(n)]
        out[0] += p
        for q in range(n):
            if bits[q]:
                out[1 + q] += p
        for q, r in itertools.combinations(range(n), 2):
            if bits[q] and bits[r]:
                out[moment_pair_row(n, q, r)] += p
    return out


@pytest.mark.parametrize("n,batch", [(1, 1), (2, 1), (5, 2)])
def test_occupation_moments_against_a_loop_over_basis_states(n, batch):
    g = torch.Generator().manual_seed(11 + n)
    states = 0.7 * torch.randn(3, 2 ** n, batch, generator=g, dtype=torch.complex128)  # not normalised
    got = occupation_moments(states)
    assert got.shape == (moment_rows(n), 3, batch) and got.dtype == torch.float64
    assert (got - _brute_force(states)).abs().max() < 1e-13
    assert moment_rows(1) == 2  # no pair rows


def test_occupation_moments_is_differentiable():
    g = torch.Generator().manual_seed(5)
    states = torch.randn(2, 8, 1, generator=g, dtype=torch.complex128, requires_grad=True)
    w = torch.randn(moment_rows(3), 2, 1, generator=g, dtype=torch.float64)
    (occupation_moments(states) * w).sum().backward()
    # d/dpsi of sum_y q(y) |psi[y]|^2 in torch's convention: 2 q(y) psi[y]
    q = torch.zeros(2, 8, 1, dtype=torch.float64)
    for y in range(8):
        bits = [(y >> (2 - j)) & 1 for j in range(3)]
        q[:, y] = w[0] + sum(w[1 + j] * bits[j] for j in range(3)) + sum(
            w[moment_pair_row(3, a, b)] * bits[a] * bits[b] for a, b in itertools.combinations(range(3), 2))
    assert (states.grad - 2.0 * q * states.detach()).abs().max() < 1e-13


@pytest.mark.parametrize("n", [2, 3, 7, 12])
def test_pair_row_offsets_enumerate_the_pairs_in_lexicographic_order(n):
    rows = [moment_pair_row(n, q, r) for q, r in itertools.combinations(range(n), 2)]
    assert rows == list(range(1 + n, moment_rows(n)))
    with pytest.raises(ValueError):
        moment_pair_row(n, 1, 1)


def _ket(amplitudes: dict, n: int) -> torch.Tensor:
    """(1, dim, 1) from {bitstring in index order (qubit 0 first): amplitude}."""
    psi = torch.zeros(1, 2 ** n, 1, dtype=torch.complex128)
    for bits, a in amplitudes.items():
        psi[0, int(bits, 2), 0] = a
    return psi


def test_conversions_on_a_product_state():
    n = 3
    theta = [0.3, 1.1, 2.0]  # qubit j: cos|0> + sin|1> (index value 0 = r)
    psi = torch.ones(1, dtype=torch.complex128)
    for t in theta:
        psi = torch.kron(psi, torch.tensor([np.cos(t), 1j * np.sin(t)], dtype=torch.complex128))
    rows = occupation_moments(psi.reshape(1, -1, 1)).sum(dim=-1)
    occ = occupations_from_moments(rows, n)  # ground-rydberg: occupied = index value 0
    assert occ.shape == (1, n) and (occ[0] - torch.tensor([np.cos(t) ** 2 for t in theta])).abs().max() < 1e-14
    occ1 = occupations_from_moments(rows, n, occupied_bit=1)
    assert (occ1[0] - torch.tensor([np.sin(t) ** 2 for t in theta])).abs().max() < 1e-14
    nn = occupation_correlations_from_moments(rows, n)
    assert nn.shape == (1, n, n) and (nn - nn.transpose(1, 2)).abs().max() == 0
    assert (torch.diagonal(nn[0]) - occ[0]).abs().max() < 1e-14
    for bit in (0, 1):
        g = connected_correlations(rows, n, occupied_bit=bit)
        off = g[0] - torch.diag(torch.diagonal(g[0]))
        assert off.abs().max() < 1e-14  # a product state has no connected correlations off the diagonal
        o = occupations_from_moments(rows, n, bit)[0]
        assert (torch.diagonal(g[0]) - (o - o ** 2)).abs().max() < 1e-14
    sf = structure_factor(connected_correlations(rows, n), [1, -1, 1])
    assert abs(float(sf[0]) - float((occ[0] - occ[0] ** 2).sum() / n)) < 1e-14
    with pytest.raises(ValueError):
        structure_factor(connected_correlations(rows, n), [1, -1])
    with pytest.raises(ValueError):
        structure_factor(connected_correlations(rows, n), [1, 0.5, 1])
    with pytest.raises(ValueError, match="rows"):
        occupations_from_moments(rows[:-1], n)


def test_conversions_on_ghz_like_states():
    n = 4
    # (|0000> + |1111>) / sqrt(2): <n_i> = 1/2, <n_i n_j> = 1/2, g_ij = 1/4 everywhere
    rows = occupation_moments(_ket({"0000": 2 ** -0.5, "1111": 2 ** -0.5}, n)).sum(dim=-1)
    for bit in (0, 1):
        assert (occupations_from_moments(rows, n, bit) - 0.5).abs().max() < 1e-15
        assert (occupation_correlations_from_moments(rows, n, bit) - 0.5).abs().max() < 1e-15
        g = connected_correlations(rows, n, bit)
        assert (g - 0.25).abs().max() < 1e-15
        assert abs(float(structure_factor(g, [1, 1, 1, 1])[0]) - 0.25 * n) < 1e-14   # ferromagnetic pattern: N^2 / 4 / N
        assert abs(float(structure_factor(g, [1, -1, 1, -1])[0])) < 1e-14            # the Neel pattern sees nothing
    # the Neel cat (|0101> + |1010>) / sqrt(2): g_ij = (-1)^(i+j) / 4, structure factor N / 4 for the Neel pattern
    rows = occupation_moments(_ket({"0101": 2 ** -0.5, "1010": 2 ** -0.5}, n)).sum(dim=-1)
    g = connected_correlations(rows, n)
    want = torch.tensor([[(-1.0) ** (i + j) / 4 for j in range(n)] for i in range(n)], dtype=torch.float64)
    assert (g[0] - want).abs().max() < 1e-15
    assert abs(float(structure_factor(g, [1, -1, 1, -1])[0]) - n / 4) < 1e-14
    # not normalised: S enters as it is (norm^2 = 4)
    rows = occupation_moments(2.0 * _ket({"0101": 2 ** -0.5, "1010": 2 ** -0.5}, n)).sum(dim=-1)
    assert (occupations_from_moments(rows, n) - 2.0).abs().max() < 1e-14


N, B, N_T = 3, 2, 3


def _call(moments=True, rdms=None):
    """A _Call on three qubits.  HOST tensors: the validation never follows the device pointers."""
    spec = ProblemSpec(N, 0.004, 5, (2 ** N - 1,), (2 ** N - 1,), solver=SolverType.DP5_SE, moments=moments, rdms=rdms)
    return _Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128), torch.zeros(1, 1, 5, dtype=torch.float64),
                 torch.zeros(N * (N - 1) // 2, dtype=torch.float64), np.linspace(0, 0.008, N_T), B, None)


def _plan(call):
    scratch = (ctypes.c_char * _native.PLAN_SCRATCH_BYTES)()
    return _native.lib().rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.cast(scratch, ctypes.c_void_p), None,
                                    ctypes.byref(_native.RydPlanInfo()))


def test_the_call_carries_the_flag_and_counts_the_block():
    assert _call().problem.bit_moments == 1 and _call(moments=False).problem.bit_moments == 0
    assert _call(moments=False).expect_rows() == 0
    assert _call().expect_rows() == 1 + 3 + 3
    rdms = [ReducedDensityMatrix([0]), ReducedDensityMatrix([1, 2])]
    assert _call(moments=False, rdms=rdms).expect_rows() == 8 + 32
    assert _call(rdms=rdms).expect_rows() == 8 + 32 + 7


def test_split_moments_takes_the_block_off_the_end_in_front_of_split_observables():
    rdms = [ReducedDensityMatrix([0])]
    expect = torch.arange((2 + 8 + 7) * 2.0, dtype=torch.float64).reshape(2 + 8 + 7, 2, 1)
    rest, mom = split_moments(expect, 3)
    assert torch.equal(mom, expect[10:]) and torch.equal(rest, expect[:10])
    real, ov, rho = split_observables(rest, 0, rdms)
    assert torch.equal(real, expect[:2]) and ov is None and rho[0].shape == (2, 1, 2, 2)
    with pytest.raises(ValueError):
        split_moments(expect[:3], 3)


def test_rydiff_plan_refuses_bad_moment_requests_without_a_device():
    """Answered before anything touches a device (this test runs without one)."""
    for bad in (2, -1):
        call = _call()
        call.problem.bit_moments = bad
        rc = _plan(call)
        assert rc == _native.RYDIFF_EINVAL, (rc, _native.last_error())
        with pytest.raises(ValueError, match="bit_moments"):
            _native.check(rc)
    call = _call()
    call.problem.shard_bits = 1
    rc = _plan(call)
    assert rc == _native.RYDIFF_ENOTIMPL
    with pytest.raises(NotImplementedError, match="not implemented together with state sharding"):
        _native.check(rc)
    call = _call()
    call.problem.n_qubits, call.problem.dm_atoms = 4, 2
    rc = _plan(call)
    assert rc == _native.RYDIFF_ENOTIMPL
    with pytest.raises(NotImplementedError, match="dm_atoms"):
        _native.check(rc)


def test_the_tangent_and_geometry_sweeps_refuse_moments_without_a_device():
    lib = _native.lib()
    info = _native.RydPlanInfo()
    info.spectral_lo, info.spectral_hi, info.flags = -1.0, 1.0, 0
    call = _call()
    for size_fn in (lib.rydiff_tangent_workspace_bytes, lib.rydiff_geometry_workspace_bytes):
        assert size_fn(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0
        assert "bit moments are not implemented" in _native.last_error()
    for flags in (0, _native.TANGENT_RDMS | _native.TANGENT_PAIR_TERMS):
        assert lib.rydiff_tangent_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(info), 2, flags) == 0
        assert lib.rydiff_geometry_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(info), 2, flags) == 0
    tg = _native.RydTangent()
    tg.n_dir, tg.d_det = 2, 0x1000
    rc = lib.rydiff_forward_tangent(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None,
                                    ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
    with pytest.raises(NotImplementedError, match="tangent sweep: bit moments are not implemented"):
        _native.check(rc)
    rc = lib.rydiff_forward_geometry(ctypes.byref(call.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None, None,
                                     ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
    with pytest.raises(NotImplementedError, match="tangent sweep: bit moments are not implemented"):
        _native.check(rc)
    # with the flag off the same call gets as far as the host-side workspace test
    off = _call(moments=False)
    rc = lib.rydiff_forward_tangent(ctypes.byref(off.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None,
                                    ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
    with pytest.raises(MemoryError, match="workspace too small"):
        _native.check(rc)
    # the Python entry points refuse before they prepare anything
    spec = ProblemSpec(N, 0.004, 5, (7,), (7,), moments=True)
    z = torch.zeros(1)
    for fn in (S.evolve_tangent, S.evolve_geometry):
        with pytest.raises(NotImplementedError, match="occupation correlations"):
            fn(z, z, z, z, z, spec, d_det=z)


def test_the_backend_refuses_what_it_does_not_serve():
    from tests.test_pauli_observables_host import _emulator
    from tests.test_tangent_host import _basic_usage_emulator, _params

    obs = OccupationCorrelations()
    emu = _emulator(3)
    with pytest.raises(NotImplementedError, match="master-equation"):
        emu.run(solver=P.SolverType.DP5_ME, observables=[obs])
    with pytest.raises(TypeError, match="OccupationCorrelations"):
        emu.run(observables=["n"])
    with pytest.raises(NotImplementedError, match="three-level"):
        _emulator(2, basis="all").run(observables=[obs])
    noisy = _emulator(3)
    noisy.set_config(P.SimConfig(noise="doppler", runs=2))
    with pytest.raises(NotImplementedError, match="average"):
        noisy.run(observables=[obs])
    dephasing = _emulator(3)
    dephasing.set_config(P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="master-equation"):  # collapse operators force the master equation
        dephasing.run(observables=[obs])
    prm = _params()
    sens = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"])
    with pytest.raises(NotImplementedError, match="OccupationCorrelations"):
        sens.run_sensitivities([prm["omega"]], [obs])
    with pytest.raises(NotImplementedError, match="OccupationCorrelations"):
        sens.run_rdm_sensitivities([prm["omega"]], [obs])
    with pytest.raises(NotImplementedError, match="OccupationCorrelations"):
        sens.run_quantum_fisher([prm["omega"]], [obs])


def test_results_serve_the_accessors_from_stored_states_and_from_native_rows():
    """The same numbers whether the rows were handed over (native) or come from the stored kets; "occupied" follows the basis."""
    g = torch.Generator().manual_seed(3)
    n, n_t = 3, 2
    states_tbd = torch.randn(n_t, 1, 2 ** n, generator=g, dtype=torch.complex128)  # (n_t, B, dim)
    times = torch.linspace(0, 1, n_t, dtype=torch.float64)
    rows = occupation_moments(states_tbd.permute(0, 2, 1))
    for basis, bit in (("ground-rydberg", 0), ("digital", 1)):
        stored = CoherentResults(states_tbd, n, basis, times, basis, atom_order=("a", "b", "c"))
        native = CoherentResults(states_tbd[:0], n, basis, times, basis, atom_order=("a", "b", "c"), native_moments=rows)
        want = occupations_from_moments(rows.sum(dim=-1), n, bit)
        assert stored.occupations().shape == (n_t, n)
        assert torch.equal(stored.occupations(), want) and torch.equal(native.occupations(), want)
        for connected in (False, True):
            a, b = stored.occupation_correlations(connected), native.occupation_correlations(connected)
            assert a.shape == (n_t, n, n) and torch.equal(a, b)
        assert torch.equal(stored.structure_factor([1, -1, 1]), native.structure_factor([1, -1, 1]))
    # <n_i> is what sampling reports as "1" on atom i
    res = CoherentResults(states_tbd, n, "ground-rydberg", times, "ground-rydberg", atom_order=("a", "b", "c"))
    dist = res[1].sampling_dist
    norm = float(rows[0, 1, 0])
    for i in range(n):
        p1 = sum(p for bits, p in dist.items() if bits[i] == "1")
        assert abs(p1 - float(res.occupations()[1, i]) / norm) < 1e-12
    with pytest.raises(RuntimeError, match="not stored"):
        CoherentResults(states_tbd[:0], n, "ground-rydberg", times, "ground-rydberg").occupations()
