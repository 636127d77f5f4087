#!/usr/bin/env python3
"""Half-chain entanglement entropy of a small Rydberg chain under a Blackman pulse, evaluated natively (needs a GPU): the state of
the left half, rho_A(t) = Tr_E |psi(t)><psi(t)|, is a ReducedDensityMatrix observable evaluated inside the solver at every evaluation
time, so the run keeps no trajectory (store_states=False).  Then one gradient step on the purity of rho_A at the final time — the
smooth entanglement loss (the entropy's gradient is undefined at degenerate spectra) — with respect to the pulse area and the
final detuning.  Usage:  python examples/entanglement_growth.py [n_atoms]   (default 8)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SolverType, TorchEmulator
from pulser_diff_amd.pulses import BlackmanWaveform, MockDevice, Pulse, RampWaveform, Register, Sequence
from pulser_diff_amd.utils import purity

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 8
area = torch.tensor([3.0], requires_grad=True)
detuning = torch.tensor([1.0], requires_grad=True)


def simulate():
    seq = Sequence(Register.rectangle(1, n_atoms, torch.tensor([7.0])), MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(Pulse(BlackmanWaveform(600, area), RampWaveform(600, -2.0, detuning), 0), "ch")
    sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1)
    left_half = sim.build_reduced_density_matrix(list(seq.register.qubits)[: n_atoms // 2])
    results = sim.run(solver=SolverType.KRYLOV_SE, observables=[left_half], store_states=False)
    return sim, left_half, results


sim, left_half, results = simulate()
entropy = results.entanglement_entropy(left_half)  # (n_t, 1), in bits
for t, s in list(zip(sim.evaluation_times.tolist(), entropy[:, 0].tolist()))[:: max(1, len(entropy) // 12)]:
    print(f"t = {t:6.3f} us   S(left half) = {s:.6f} bits")
rho_final = results.reduced_density_matrix(left_half)[-1, 0]
loss = purity(rho_final)
loss.backward()
print(f"final purity {float(loss.detach()):.6f};  d purity / d area = {float(area.grad):+.6f},  d purity / d final detuning = {float(detuning.grad):+.6f}")
with torch.no_grad():  # one step towards MORE entanglement (lower purity)
    area -= 0.5 * area.grad
    detuning -= 0.5 * detuning.grad
area.grad = detuning.grad = None
_, left_half, results = simulate()
print(f"after one gradient step: final purity {float(purity(results.reduced_density_matrix(left_half)[-1, 0])):.6f}")
