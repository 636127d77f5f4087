"""What is in a workspace when the library gets it must not matter.

Every workspace and the plan scratch are uninitialised device memory (pulser_diff_amd.solver._new_workspace).  Fresh device pages
tend to be zero, so a region that is read before it is written would pass every other test and misbehave in a training loop on
recycled memory.  Here the seam is replaced: the same problem runs once on zero-filled buffers and once on buffers whose every
8 bytes are a quiet NaN.  Every output must be finite and agree with the zero-filled run at 1e-12 relative to its largest entry —
the bar of tests/test_gpu_solver_parity.py for repeats of one route, whose atomics leave the summation order free.  A NaN anywhere
is a read-before-write.  (The regions that hold indices or counts — stage records, factor-table inputs, Pauli tables, save-point
flags, backward stage records — are uploaded by each call before any kernel reads them: established by reading prepare, carve,
upload_pauli_tables, build_persist_table_device and scatter_gradients, so a poisoned buffer can only show up as a NaN.)

  evolve + backward   cotangent on every row (diagonal + Pauli + overlap), all five gradients (tables, U, tsave, psi0); 3, 9 and 13
                      qubits = the lane, direct and chained kernel families; both solvers, automatic kernel choice; at 13 qubits
                      every tape mode of ProblemSpec; stored states with a cotangent on the states once
  evolve_tangent      3 and 9 qubits, 5 directions (one padded), only d_amp / only d_u; 13 directions in two chunks at 3 qubits

Measured on an MI355X: no output differs by more than 4.5e-15 relative between the two fills (the tangent sweep: bit-identical);
no region is read before it is written.
"""
import numpy as np
import pytest
import torch

from pulser_diff_amd import solver as S
from pulser_diff_amd.observables import StateOverlap, pack_overlaps
from pulser_diff_amd.solver import SolverType, evolve, evolve_tangent
from pulser_diff_amd.utils import total_magnetization_diag
from tests.helpers import random_terms, rel_err, to_native
from tests.test_gpu_tangent import _randn, observable_set

pytestmark = pytest.mark.gpu

SAME_ROUTE_RTOL = 1e-12
N_SAMPLES, DT = 41, 0.004
TSAVE = (0.0, 0.0313, 0.0622, 0.0951)


def _filled(value):
    """A replacement for solver._new_workspace: nbytes of uint8 whose every 8 bytes are the float64 `value`."""
    def new_workspace(nbytes, dev):
        words = torch.full(((int(nbytes) + 7) // 8,), value, dtype=torch.float64, device=dev)
        return words.view(torch.uint8)[:int(nbytes)]
    return new_workspace


def _problem(n, solver_name, dev, store_states=False, tape="auto", tape_steps=None):
    terms = random_terms(n, N_SAMPLES, DT, seed=4100 + n, local=True, phase=True)
    amp, det, u, spec = to_native(terms, dev, SolverType[solver_name], store_states=store_states)
    spec.tape, spec.tape_steps = tape, tape_steps
    gen = torch.Generator().manual_seed(88000 + n)
    dim, batch = 2**n, 2
    psi0 = _randn(gen, batch, dim, cplx=True)
    psi0 = (psi0 / psi0.norm(dim=1, keepdim=True)).to(dev)
    target = _randn(gen, dim, batch, cplx=True)
    spec.pauli = observable_set(n)
    spec.overlaps = pack_overlaps([StateOverlap(target / target.norm(dim=0, keepdim=True))], dim, batch, dev)
    zdiag = total_magnetization_diag(n)[None].to(dev)
    return amp, det, u, spec, psi0, zdiag, gen


def _both_fills(monkeypatch, run):
    out = {}
    for name, value in (("zeros", 0.0), ("nans", float("nan"))):
        monkeypatch.setattr(S, "_new_workspace", _filled(value))
        out[name] = run()
        torch.cuda.synchronize()
    return out["zeros"], out["nans"]


def _compare(label, zeros, nans):
    assert zeros.keys() == nans.keys()
    for key in zeros:
        a, b = zeros[key], nans[key]
        assert a.shape == b.shape and a.size > 0, key
        assert np.isfinite(a).all(), f"{label}: {key} is not finite on a zero-filled workspace"
        assert np.isfinite(b).all(), f"{label}: {key} is not finite on a NaN-filled workspace: a region is read before it is written"
        scale = float(np.abs(a).max())
        err = rel_err(b, a)
        print(f"{label}: {key}: largest entry {scale:.3e}, NaN-filled against zero-filled {err:.2e} relative")
        assert scale > 0.0
        assert err <= SAME_ROUTE_RTOL, key


BACKWARD_CASES = ([(n, s, False, "auto", None) for n in (3, 9, 13) for s in ("KRYLOV_SE", "DP5_SE")]
                  + [(13, s, False, tape, steps) for s in ("KRYLOV_SE", "DP5_SE") for tape, steps in (("steps", None), ("full", None), ("partial", 1))]
                  + [(9, "DP5_SE", True, "auto", None)])


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=[f"N{n}-{s}-{'states' if st else 'nostates'}-{tape}" for n, s, st, tape, _ in BACKWARD_CASES])
def test_evolve_and_backward_do_not_depend_on_workspace_contents(case, cuda_device, monkeypatch):
    n, solver_name, store_states, tape, tape_steps = case
    amp, det, u, spec, psi0, zdiag, gen = _problem(n, solver_name, cuda_device, store_states, tape, tape_steps)
    tsave0 = torch.tensor(TSAVE, dtype=torch.float64)
    rows = 1 + len(spec.pauli) + 2
    w = _randn(gen, rows, len(TSAVE), psi0.shape[0]).to(cuda_device)
    w_states = _randn(gen, len(TSAVE), *psi0.shape, cplx=True).to(cuda_device) if store_states else None
    modes = []

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (amp, det, u, tsave0, psi0)]
        states, expect = evolve(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], spec, zdiag)
        modes.append(spec.options["_last_stats"]["tape"])
        loss = (w * expect).sum()
        if store_states:
            loss = loss + (w_states.conj() * states).real.sum()
        loss.backward()
        out = {"expect": expect, "g_amp": leaves[0].grad, "g_det": leaves[1].grad, "g_u": leaves[2].grad, "g_tsave": leaves[3].grad,
               "g_psi0": leaves[4].grad}
        if store_states:
            out["states"] = states
        return {k: (torch.view_as_real(v) if v.is_complex() else v).detach().cpu().numpy() for k, v in out.items()}

    zeros, nans = _both_fills(monkeypatch, run)
    assert modes[0] == modes[1]
    if tape != "auto":
        assert modes[0] == tape  # the mode asked for is the mode that ran
    _compare(f"N{n} {solver_name} tape={modes[0]}", zeros, nans)


TANGENT_CASES = [(3, 5, "a"), (3, 5, "u"), (9, 5, "a"), (9, 5, "u"), (3, 13, "ap")]


@pytest.mark.parametrize("n,n_dir,which", TANGENT_CASES, ids=[f"N{n}-D{d}-{w}" for n, d, w in TANGENT_CASES])
@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_evolve_tangent_does_not_depend_on_workspace_contents(solver_name, n, n_dir, which, cuda_device, monkeypatch):
    amp, det, u, spec, psi0, zdiag, gen = _problem(n, solver_name, cuda_device)
    tsave = torch.tensor(TSAVE, dtype=torch.float64)
    d_amp = (float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)).to(cuda_device) if "a" in which else None
    d_u = (float(u.abs().max()) * _randn(gen, n_dir, *u.shape)).to(cuda_device) if "u" in which else None
    d_psi = (_randn(gen, n_dir, *psi0.shape, cplx=True) / np.sqrt(psi0.shape[1])).to(cuda_device) if "p" in which else None

    def run():
        expect, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec, zdiag, d_amp=d_amp, d_u=d_u, d_psi0=d_psi)
        return {"expect": expect.cpu().numpy(), "dexpect": dexpect.cpu().numpy()}

    zeros, nans = _both_fills(monkeypatch, run)
    _compare(f"N{n} {solver_name} D={n_dir} {which}", zeros, nans)
