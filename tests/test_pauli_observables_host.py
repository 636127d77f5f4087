"""Host side of the Pauli-string observables (no GPU): the mask conventions of include/rydiff.h against kron of the 2x2 matrices,
the matrix-free torch expectation against the dense route, build_observable against build_operator, the rotating frame, and the
checks that stand between a caller and the C ABI."""
import itertools

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import pulses as pl
from pulser_diff_amd.observables import MAX_PAULI_STRINGS, PauliObservable, check_pauli, pack_pauli
from pulser_diff_amd.solver import ProblemSpec, SolverType, _check_shapes
from pulser_diff_amd.utils import IMAT, XMAT, YMAT, ZMAT, expect, kron

MATS = {"I": IMAT, "X": XMAT, "Y": YMAT, "Z": ZMAT}


def _dense(n, paulis: dict):
    return kron(*[MATS[paulis.get(j, "I")] for j in range(n)])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_to_dense_is_kron_of_the_two_by_two_matrices(n):
    for j in range(n):
        for name in "XYZ":
            got = PauliObservable(n, [(1.0, {j: name})]).to_dense()
            assert torch.equal(got, _dense(n, {j: name})), (n, j, name)
    if n >= 3:
        rng = np.random.default_rng(n)
        for _ in range(12):
            qs = rng.choice(n, size=3, replace=False)
            paulis = {int(q): "XYZ"[rng.integers(3)] for q in qs}
            w = float(rng.uniform(-1, 1))
            assert (PauliObservable(n, [(w, paulis)]).to_dense() - w * _dense(n, paulis)).abs().max() < 1e-15


def test_all_three_qubit_strings_and_the_string_form():
    for s in itertools.product("IXYZ", repeat=3):
        s = "".join(s)
        want = kron(*[MATS[c] for c in s])
        assert torch.equal(PauliObservable(3, [(1.0, s)]).to_dense(), want), s


def test_algebra_merges_equal_strings():
    a = PauliObservable(3, [(0.5, "XIZ"), (0.25, {1: "Y"})])
    b = PauliObservable(3, [(1.5, {0: "X", 2: "Z"}), (-0.25, "IYI")])
    c = a + 2.0 * b
    assert len(c) == 2 and c.shape == (8, 8) and not c.is_sparse
    assert (c.to_dense() - (a.to_dense() + 2.0 * b.to_dense())).abs().max() < 1e-15
    assert (( a - b).to_dense() - (a.to_dense() - b.to_dense())).abs().max() < 1e-15


@pytest.mark.parametrize("n", [1, 2, 4, 6])
def test_matrix_free_expectation_equals_the_dense_route(n):
    g = torch.Generator().manual_seed(40 + n)
    rng = np.random.default_rng(n)
    terms = [(float(rng.uniform(-1, 1)), {j: "XYZ"[rng.integers(3)] for j in rng.choice(n, size=min(n, 1 + k % 3), replace=False)})
             for k in range(7)]
    obs = PauliObservable(n, terms)
    dense = obs.to_dense()
    kets = torch.randn(5, 2**n, 1, generator=g, dtype=torch.complex128)
    assert (expect(obs, kets) - expect(dense, kets)).abs().max() < 1e-12
    rho = torch.randn(5, 2**n, 2**n, 1, generator=g, dtype=torch.complex128)
    assert (expect(obs, rho) - expect(dense, rho)).abs().max() < 1e-12
    # hermitian observable on a state: real
    assert expect(obs, kets).imag.abs().max() < 1e-12


def _emulator(n=3, basis="ground-rydberg"):
    coords = {f"q{j}": torch.tensor([8.0 * j, 0.3 * j], dtype=torch.float64) for j in range(n)}
    seq = pl.Sequence(pl.Register(coords), pl.MockDevice)
    if basis == "all":
        seq.declare_channel("ryd", "rydberg_global")
        seq.declare_channel("ram", "raman_local", initial_target="q0")
        seq.add(pl.Pulse.ConstantPulse(100, 3.0, 0.5, 0.0), "ryd")
        seq.add(pl.Pulse.ConstantPulse(100, 2.0, 0.0, 0.0), "ram")
    else:
        seq.declare_channel("ch", "rydberg_global")
        seq.add(pl.Pulse.ConstantPulse(100, 3.0, 0.5, 0.4), "ch")
    return P.TorchEmulator.from_sequence(seq, sampling_rate=0.5, compute_device="cpu")


def test_build_observable_equals_build_operator():
    emu = _emulator(4)
    bo = lambda ops: emu.build_operator(ops).to_dense()  # noqa: E731
    x = XMAT.clone()
    sgr = emu._hamiltonian.op_matrix["sigma_gr"].to_dense()
    cases = [
        [(x, "global")],
        [(ZMAT.clone(), ["q0", "q2"]), (YMAT.clone(), ["q3"])],
        [("sigma_rr", ["q1"])],
        [(sgr + sgr.mH, ["q2"])],
    ]
    for ops in cases:
        got = emu.build_observable(ops)
        assert isinstance(got, PauliObservable)
        assert (got.to_dense() - bo(ops)).abs().max() < 1e-14
    # the Pauli names are accepted directly
    assert (emu.build_observable([("X", "global")]).to_dense() - bo([(x, "global")])).abs().max() < 1e-14
    assert (emu.build_observable([("Z", ["q0", "q2"]), ("Y", ["q3"])]).to_dense() - bo(cases[1])).abs().max() < 1e-14
    with pytest.raises(ValueError, match="Hermitian"):
        emu.build_observable([("sigma_gr", ["q1"])])


def test_build_observable_refuses_the_three_level_basis():
    emu = _emulator(2, basis="all")
    with pytest.raises(NotImplementedError):
        emu.build_observable([("X", "global")])


@pytest.mark.parametrize("phi", [0.37, -1.9])
def test_rotated_is_the_frame_transform(phi):
    n = 3
    ones = torch.tensor([bin(i).count("1") for i in range(2**n)], dtype=torch.float64)
    V = torch.diag(torch.exp(1j * phi * ones))
    for s in ["ZIZ", "IXI", "ZYI", "XIY", "YZX", "XYX", "YYY"]:  # 0, 1, 2, 3 flipped qubits
        obs = PauliObservable(n, [(0.8, s), (-0.3, "IIZ")])
        rot = obs.rotated(phi)
        assert (rot.to_dense() - V @ obs.to_dense() @ V.mH).abs().max() < 1e-14, s
        flips = sum(c in "XY" for c in s)
        assert len(rot) <= 2**flips + 1


def test_masks_and_the_checks_in_front_of_the_c_abi():
    obs = PauliObservable(4, [(0.5, "XIYZ"), (1.0, {3: "Z"})])
    first, x, z, w = obs.masks()
    assert first.tolist() == [0, 2] and first.dtype == np.int32 and x.dtype == np.uint32 and w.dtype == np.float64
    assert sorted(zip(x.tolist(), z.tolist(), w.tolist())) == [(0, 8, 1.0), (0b0101, 0b1100, 0.5)]
    f2, x2, _, _ = pack_pauli([obs, PauliObservable(4), obs * 2.0], 4)
    assert f2.tolist() == [0, 2, 2, 4] and len(x2) == 4
    with pytest.raises(ValueError):
        PauliObservable(3, [(1.0, {3: "X"})])
    with pytest.raises(ValueError):
        pack_pauli([obs], 3)

    def spec(pauli):
        return ProblemSpec(3, 0.01, 8, (0b111,), (), solver=SolverType.KRYLOV_SE, pauli=pauli)

    amp = torch.zeros(1, 1, 8, dtype=torch.complex128)
    det = torch.zeros(1, 0, 8)
    u = torch.zeros(3)
    ok = (np.array([0, 1]), np.array([0b101]), np.array([0b010]), np.array([1.0]))
    _check_shapes(spec(ok), amp, det, u, None, 1)
    with pytest.raises(ValueError, match="n_qubits"):  # mask bit at N
        _check_shapes(spec((np.array([0, 1]), np.array([0b1000]), np.array([0]), np.array([1.0]))), amp, det, u, None, 1)
    with pytest.raises(ValueError):  # counts disagree
        _check_shapes(spec((np.array([0, 2]), np.array([1]), np.array([0]), np.array([1.0]))), amp, det, u, None, 1)
    many = MAX_PAULI_STRINGS + 1
    with pytest.raises(ValueError, match="too many"):
        _check_shapes(spec((np.array([0, many]), np.ones(many, dtype=np.uint32), np.zeros(many, dtype=np.uint32), np.ones(many))),
                      amp, det, u, None, 1)
    with pytest.raises(ValueError, match="too many"):
        check_pauli((np.array([0, many]), np.ones(many, dtype=np.uint32), np.zeros(many, dtype=np.uint32), np.ones(many)), 3)


def test_ctypes_mirror_carries_the_pauli_fields():
    from pulser_diff_amd import _native

    names = [f[0] for f in _native.RydProblem._fields_]
    assert names[-6:] == ["n_pauli_obs", "n_pauli_strings", "pauli_first", "pauli_x", "pauli_z", "pauli_w"]
    assert _native.MAX_PAULI_STRINGS == MAX_PAULI_STRINGS >= 512
