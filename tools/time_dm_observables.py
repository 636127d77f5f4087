"""Master-equation observables: the native route (RydProblem.dm_*, no stored density matrices) against the stored-rho route (the
whole (n_t, 4^n) trajectory returned, torch expectation values, autograd through the stored states), same shapes, same build:

    python tools/time_dm_observables.py [atoms, comma separated = 8,10] [evaluation times = 200] [repeats = 5] [big = 12]

Per size: a Z-sum and one target-state fidelity at every evaluation time; forward only, and forward + gradient of the final values
w.r.t. the amplitude / detuning tables and the interactions.  One warm-up, then `repeats` timed runs bracketed by device
synchronisation; median, min and max of the wall time and the peak device memory of the run are printed: torch.cuda.max_memory_allocated,
reset before every run after a garbage collection, minus what was allocated at that moment (the problem's tables, and whatever
persistent workspace torch's BLAS took in an earlier stored-route run; printed as `held`).  Forward-only runs are repeated at half the evaluation times to show what grows with n_t.  `big` (0: skip):
one forward-only run at that many atoms with half the evaluation times and no stored states — 4^12 amplitudes are 256 MiB per
density matrix, which the stored-rho route cannot hold for a few hundred times.

    python tools/time_dm_observables.py rdm [atoms = 8,10,12] [evaluation times = 50] [repeats = 3] [times at 12 atoms = 8]

The reduced-density-matrix leg: Tr_E rho on m = 2 and m = 6 atoms (the leading ones) at every evaluation time, natively with
store_states=False against stored rho plus the torch partial trace (observables.reduced_density_matrix); forward only and, below 12
atoms, forward + gradient of sum |rho_A(T)|^2.  Same measurement as above; 12 atoms runs forward only on few evaluation times (the
stored route holds 256 MiB per time and torch's permuted copy of it)."""
import gc
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import pulser_diff_amd as P  # noqa: E402
from pulser_diff_amd import pulses as pl  # noqa: E402
from pulser_diff_amd.lindblad import mesolve  # noqa: E402
from pulser_diff_amd.observables import ReducedDensityMatrix, StateOverlap, reduced_density_matrix  # noqa: E402
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag  # noqa: E402

DURATION_NS = 200


def problem(n, n_t, dev):
    seq = pl.Sequence(pl.Register.rectangle(1, n, spacing=8, prefix="q"), pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(DURATION_NS, 2.0), pl.RampWaveform(DURATION_NS, -3.0, 2.0), 0.0), "g")
    cfg = P.SimConfig(noise=("dephasing", "relaxation"), dephasing_rate=0.2, relaxation_rate=0.1)
    sim = P.TorchEmulator.from_sequence(seq, config=cfg, compute_device=dev)
    ham = sim._hamiltonian
    tsave = torch.linspace(0.0, 1e-3 * DURATION_NS, n_t, dtype=torch.float64)
    dim = 2 ** n
    target = torch.zeros(dim, dtype=torch.complex128)
    target[0] = target[dim - 1] = 2 ** -0.5  # (|r..r> + |g..g>) / sqrt 2
    psi0 = torch.zeros(dim, 1, dtype=torch.complex128, device=dev)
    psi0[dim - 1] = 1.0
    return ham, tsave, psi0, DiagonalObservable(total_magnetization_diag(n)), StateOverlap(target)


def leaf_ham(ham, grad):
    return SimpleNamespace(amp_tables=ham.amp_tables.detach().clone().requires_grad_(grad), det_tables=ham.det_tables.detach().clone().requires_grad_(grad),
                           u_pairs=ham.u_pairs.detach().clone().requires_grad_(grad), amp_masks=ham.amp_masks, det_masks=ham.det_masks, dt=ham.dt,
                           n_samples=ham.n_samples, _size=ham._size, pair_terms=getattr(ham, "pair_terms", ()), piece_refine=getattr(ham, "piece_refine", None),
                           config=ham.config, basis_name=ham.basis_name)


def run(route, ham, tsave, psi0, zsum, fid, grad):
    h = leaf_ham(ham, grad)
    with torch.set_grad_enabled(grad):
        if route == "native":
            res = mesolve(h, psi0, tsave, ham.config, observables=[zsum, fid], store_states=False)
            z, f = res.expect
        else:  # the whole trajectory, expectation values in torch
            rho, _ = mesolve(h, psi0, tsave, ham.config)
            z = torch.einsum("x,txxb->tb", zsum.diag.to(rho.device, torch.complex128), rho).real
            phi = fid.targets.to(rho.device)
            f = torch.einsum("xb,txyb,yb->tb", phi.conj(), rho, phi).real
        if grad:
            (z[-1] + f[-1]).sum().backward()
    return float(z[-1, 0].detach()), float(f[-1, 0].detach())


def run_rdm(route, ham, tsave, psi0, obs, grad):
    h = leaf_ham(ham, grad)
    with torch.set_grad_enabled(grad):
        if route == "native":
            rho_a = mesolve(h, psi0, tsave, ham.config, observables=[obs], store_states=False).rdms[0]
        else:  # the whole trajectory, the partial trace in torch
            rho, _ = mesolve(h, psi0, tsave, ham.config)
            rho_a = reduced_density_matrix(obs, rho)
        pur = (rho_a[-1].real ** 2 + rho_a[-1].imag ** 2).sum()
        if grad:
            pur.backward()
    return float(torch.einsum("baa->b", rho_a[-1].detach()).real[0]), float(pur.detach())


def measure(route, args, grad, repeats, run=run):
    run(route, *args, grad)  # warm-up (allocator, plan cache, code objects)
    times, peak, held, vals = [], 0, 0, None
    for _ in range(repeats):
        gc.collect()  # (autograd contexts of the previous run hold their tape workspace until the cycle collector has run)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        vals = run(route, *args, grad)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - held)
    return statistics.median(times), min(times), max(times), peak, held, vals


def main_rdm(argv):
    sizes = [int(s) for s in (argv[0] if len(argv) > 0 else "8,10,12").split(",")]
    n_t = int(argv[1]) if len(argv) > 1 else 50
    repeats = int(argv[2]) if len(argv) > 2 else 3
    n_t_big = int(argv[3]) if len(argv) > 3 else 8
    dev = "cuda"
    print(f"device: {torch.cuda.get_device_name(0)}; {DURATION_NS} ns pulse, dephasing + relaxation; Tr_E rho on the m leading atoms at every "
          f"evaluation time; 1 warm-up, {repeats} timed runs, median [min, max]")
    print(f"{'atoms':>5} {'m':>2} {'n_t':>4} {'mode':>8} {'route':>7} {'median ms':>10} {'min ms':>9} {'max ms':>9} {'peak MiB':>10} {'held MiB':>9}   "
          "Tr rho_A(T), sum |rho_A(T)|^2")
    for n in sizes:
        nt = n_t if n < 12 else n_t_big
        ham, tsave, psi0, _, _ = problem(n, nt, dev)
        for m in (2, 6):
            obs = ReducedDensityMatrix(range(m))
            for grad in ((False, True) if n < 12 else (False,)):
                for route in ("native", "stored"):
                    med, lo, hi, peak, held, vals = measure(route, (ham, tsave, psi0, obs), grad, repeats, run=run_rdm)
                    print(f"{n:>5} {m:>2} {nt:>4} {'fwd+grad' if grad else 'fwd':>8} {route:>7} {1e3 * med:>10.1f} {1e3 * lo:>9.1f} {1e3 * hi:>9.1f} "
                          f"{peak / 2**20:>10.1f} {held / 2**20:>9.1f}   {vals[0]:.9f} {vals[1]:.9f}", flush=True)
        del ham, tsave, psi0
        gc.collect()
        torch.cuda.empty_cache()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rdm":
        return main_rdm(sys.argv[2:])
    sizes = [int(s) for s in (sys.argv[1] if len(sys.argv) > 1 else "8,10").split(",")]
    n_t = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    big = int(sys.argv[4]) if len(sys.argv) > 4 else 12
    dev = "cuda"
    print(f"device: {torch.cuda.get_device_name(0)}; {DURATION_NS} ns pulse, dephasing + relaxation; Z-sum + one fidelity; 1 warm-up, "
          f"{repeats} timed runs, median [min, max]")
    print(f"{'atoms':>5} {'n_t':>4} {'mode':>8} {'route':>7} {'median ms':>10} {'min ms':>9} {'max ms':>9} {'peak MiB':>10} {'held MiB':>9}   <Z>(T), fidelity(T)")
    for n in sizes:
        for nt, modes in ((n_t, (False, True)), (n_t // 2, (False,))):
            args = problem(n, nt, dev)
            for grad in modes:
                for route in ("native", "stored"):
                    med, lo, hi, peak, held, vals = measure(route, args, grad, repeats)
                    print(f"{n:>5} {nt:>4} {'fwd+grad' if grad else 'fwd':>8} {route:>7} {1e3 * med:>10.1f} {1e3 * lo:>9.1f} {1e3 * hi:>9.1f} "
                          f"{peak / 2**20:>10.1f} {held / 2**20:>9.1f}   {vals[0]:+.9f} {vals[1]:.9f}", flush=True)
            del args
            torch.cuda.empty_cache()
    if big:
        args = problem(big, n_t // 2, dev)
        med, lo, hi, peak, held, vals = measure("native", args, False, max(repeats // 2, 1))
        print(f"{big:>5} {n_t // 2:>4} {'fwd':>8} {'native':>7} {1e3 * med:>10.1f} {1e3 * lo:>9.1f} {1e3 * hi:>9.1f} {peak / 2**20:>10.1f} {held / 2**20:>9.1f}   "
              f"{vals[0]:+.9f} {vals[1]:.9f}   (stored route: {(n_t // 2) * 4 ** big * 16 / 2**30:.0f} GiB of states alone)", flush=True)


if __name__ == "__main__":
    main()
