"""The oracle side of tests/test_gpu_dm_tangent.py: values and directional derivatives of the density-matrix rows from
R.lindblad_magnus_dense on terms + s * direction and torch.autograd.functional.jacobian w.r.t. s at s = 0.

The oracle is dense torch with Python-level loops: one case (28 reverse passes per trajectory through ~26 exponentials of the 4^n x 4^n
Liouvillian) takes 1.5 to 3 minutes of CPU at 3 and 4 atoms.  The suite therefore reads the RECORDED results,
tests/golden/dm_tangent_oracle.npz — inputs (so that no random-number stream has to reproduce) and outputs of `oracle_case` for every
(n, noise) of the test — and `python -m tests.dm_tangent_reference` regenerates the file (one process per case).
tests/test_dm_tangent_host.py recomputes the smallest case and compares it with the record."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

from oracle import restatement as R
from pulser_diff_amd.observables import Purity, StateOverlap
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import random_terms, shifted_terms, to_native

GOLDEN = Path(__file__).resolve().parent / "golden" / "dm_tangent_oracle.npz"
NON_NORMAL = [[0.2, 1.0], [0.3j, -0.1]]  # tests/test_gpu_master_equation_sizes.py: all four relative flips in the dissipator block
NOISE = {"dephasing": {"dephasing": 1.1}, "deph+relax": {"dephasing": 1.1, "relaxation": 0.6},
         "non-normal": {"eff_noise": [(0.6, NON_NORMAL)]}}
TSAVE = (0.0, 0.0011, 0.0027, 0.0046)  # 4 save points off the sample grid (dt = 0.004); the last interval crosses a grid line
BATCH = {2: 1, 3: 2, 4: 1}
N_DIR = 8
ZERO_DIRECTION = 2
SIZES = (2, 3, 4)


def h_max(n: int) -> float:
    return 0.0002 if n < 4 else 0.0004  # tests/test_gpu_dm_observables.py: test_gradients_of_all_row_kinds_match_dense_autograd


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


def case_terms(n: int):
    return random_terms(n, 8, 0.004, seed=6100 + n, local=True)


def directions(amp, det, u, gen, n_dir=N_DIR):
    """Directions that mix the three table tangents: 0 all three, 1 d_amp only, 2 ZERO, 3 d_det only, 4 d_u only, the rest all three;
    each scaled like the input it perturbs."""
    d_amp = float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)
    d_det = float(det.abs().max()) * _randn(gen, n_dir, *det.shape)
    d_u = float(u.abs().max()) * _randn(gen, n_dir, *u.shape)
    for d, keep in ((1, "a"), (ZERO_DIRECTION, ""), (3, "d"), (4, "u")):
        if d < n_dir:
            d_amp[d] *= float("a" in keep)
            d_det[d] *= float("d" in keep)
            d_u[d] *= float("u" in keep)
    return d_amp, d_det, d_u


def case_inputs(n: int, noise_key: str) -> dict:
    """Seeded inputs of one case: psi0 (dim, B), a fidelity target per trajectory (dim, B), the table tangents (N_DIR, 1, K, n_samples)
    and d_u (N_DIR, n_pairs)."""
    batch, dim = BATCH[n], 2 ** n
    amp, det, u, _ = to_native(case_terms(n), "cpu", None)
    gen = torch.Generator().manual_seed(6200 + 17 * n + len(noise_key))
    psi0 = _randn(gen, dim, batch, cplx=True)
    target = _randn(gen, dim, batch, cplx=True)
    d_amp, d_det, d_u = directions(amp, det, u, gen)
    return dict(psi0=psi0 / psi0.norm(dim=0, keepdim=True), target=target / target.norm(dim=0, keepdim=True), d_amp=d_amp, d_det=d_det, d_u=d_u)


def observables(n: int, target: torch.Tensor) -> list:
    """The row set of tests/test_gpu_dm_observables._me_observables on a given target: two diagonals, two Pauli sums, a per-trajectory
    and a shared fidelity target, the purity."""
    from tests.test_gpu_dm_observables import _paulis

    zsum = DiagonalObservable(total_magnetization_diag(n) / n)
    other = torch.linspace(-1.0, 1.0, 2 ** n, dtype=torch.float64)
    return [zsum, other] + _paulis(n) + [StateOverlap(target), StateOverlap(target[:, 0].flip(0).clone()), Purity()]


def oracle_case(n: int, noise_key: str, inputs: dict | None = None) -> tuple:
    """(values (rows, n_t, B), derivatives (N_DIR, rows, n_t, B)) of the oracle for one case."""
    from tests.test_gpu_dm_observables import _torch_rows

    inp = inputs or case_inputs(n, noise_key)
    terms = case_terms(n)
    obs = observables(n, inp["target"])
    tsave = torch.tensor(TSAVE, dtype=torch.float64)
    collapse = R.collapse_operators(n, NOISE[noise_key])
    vals, jacs = [], []
    for b in range(BATCH[n]):
        rho0 = torch.outer(inp["psi0"][:, b], inp["psi0"][:, b].conj())
        obs_b = [StateOverlap(o.targets[:, b if o.targets.shape[1] > 1 else 0].clone()) if isinstance(o, StateOverlap) else o for o in obs]

        def rows(s):
            rho = R.lindblad_magnus_dense(shifted_terms(terms, inp["d_amp"][:, 0], inp["d_det"][:, 0], inp["d_u"], s), collapse, rho0, tsave,
                                          h_max=h_max(n))
            return torch.stack(_torch_rows(rho[..., None], obs_b))[..., 0]  # (rows, n_t)

        s0 = torch.zeros(N_DIR, dtype=torch.float64)
        vals.append(rows(s0).detach())
        jacs.append(torch.autograd.functional.jacobian(rows, s0))  # (rows, n_t, N_DIR)
    return torch.stack(vals, dim=-1), torch.stack(jacs, dim=-1).permute(2, 0, 1, 3).contiguous()


def key(n: int, noise_key: str, name: str) -> str:
    return f"n{n}/{noise_key}/{name}"


def load_case(n: int, noise_key: str) -> dict:
    """The recorded case: inputs and oracle outputs as CPU tensors."""
    with np.load(GOLDEN) as z:
        out = {name: torch.from_numpy(z[key(n, noise_key, name)]) for name in ("psi0", "target", "d_amp", "d_det", "d_u", "val", "der")}
    return out


def _record_one(n: int, noise_key: str, path: Path) -> None:
    torch.set_num_threads(1)
    inp = case_inputs(n, noise_key)
    val, der = oracle_case(n, noise_key, inp)
    np.savez(path, **{key(n, noise_key, k): v.numpy() for k, v in {**inp, "val": val, "der": der}.items()})


if __name__ == "__main__":
    import subprocess
    import tempfile

    if len(sys.argv) == 4:  # worker: n, noise, output file
        _record_one(int(sys.argv[1]), sys.argv[2], Path(sys.argv[3]))
        sys.exit(0)
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(n, nk, Path(tmp) / f"{n}_{i}.npz") for n in SIZES for i, nk in enumerate(NOISE)]
        procs = [subprocess.Popen([sys.executable, "-m", "tests.dm_tangent_reference", str(n), nk, str(p)]) for n, nk, p in jobs]
        assert all(p.wait() == 0 for p in procs)
        merged = {}
        for _, _, p in jobs:
            with np.load(p) as z:
                merged.update({k: z[k] for k in z.files})
    np.savez_compressed(GOLDEN, **merged)
    print("wrote", GOLDEN, GOLDEN.stat().st_size, "bytes")
