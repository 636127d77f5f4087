#!/usr/bin/env python3
"""How entanglement decays under dephasing (needs a GPU): a short Rydberg chain driven by a Blackman pulse with collapse-operator
noise, so the run is a master-equation run.  The states of a pair of atoms and of a single atom, Tr_E rho(t), are
ReducedDensityMatrix observables evaluated inside the solver at every evaluation time: the run keeps no (n_t, 4^n) trajectory
(store_states=False).  The register state is mixed, so the entropy of a subsystem no longer measures entanglement (it also counts the
noise); the negativity of the pair does.  Then one gradient of the final negativity with respect to the pulse area.
Usage:  python examples/noisy_entanglement.py [n_atoms = 3] [dephasing rate = 0.3]."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SimConfig, TorchEmulator
from pulser_diff_amd.pulses import BlackmanWaveform, MockDevice, Pulse, RampWaveform, Register, Sequence

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 3
rate = float(sys.argv[2]) if len(sys.argv) > 2 else 0.3
area = torch.tensor([3.0], requires_grad=True)

seq = Sequence(Register.rectangle(1, n_atoms, torch.tensor([7.0])), MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse(BlackmanWaveform(600, area), RampWaveform(600, -2.0, 1.0), 0), "ch")
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, config=SimConfig(noise="dephasing", dephasing_rate=rate))
atoms = list(seq.register.qubits)
pair = sim.build_reduced_density_matrix(atoms[:2])
single = sim.build_reduced_density_matrix(atoms[:1])
results = sim.run(observables=[pair, single], store_states=False)  # collapse-operator noise: the master equation

negativity = results.negativity(pair, 1)         # (n_t, 1): atom 0 against atom 1
entropy = results.entanglement_entropy(single)   # (n_t, 1), bits: the entropy of atom 0 (entanglement AND noise)
for t, neg, s in list(zip(sim.evaluation_times.tolist(), negativity[:, 0].tolist(), entropy[:, 0].tolist()))[:: max(1, len(entropy) // 12)]:
    print(f"t = {t:6.3f} us   negativity(0|1) = {neg:.6f}   S(atom 0) = {s:.6f} bits")
final = negativity[-1, 0]
final.backward()
print(f"final negativity {float(final.detach()):.6f};  d negativity / d area = {float(area.grad):+.6f}")
