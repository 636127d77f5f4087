#!/usr/bin/env python3
"""State preparation under dephasing (needs a GPU): the loss is 1 - <target| rho(T) |target> of a MASTER-EQUATION run, with the
fidelity evaluated and differentiated inside the solver (`model.fidelity`: a StateOverlap observable on the density matrix) — no
density matrix is stored (`store_states=False`: a stored trajectory would be n_t x 4^n amplitudes) and autograd never sees a
4^n-sized tensor.  Pulse shapes and optimiser of state_preparation_native.py on a few atoms; dephasing caps the reachable fidelity,
and the purity of the final state (native as well) says by how much.
Usage:  python examples/noisy_state_preparation.py [n_atoms [epochs [dephasing_rate [seed]]]]   (defaults 3, 60, 0.05, 1)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import torch

from optimal_control_loop import load_parameters, train
from pulser_diff_amd import Purity, QuantumModel, SimConfig, StateOverlap
from pulser_diff_amd.pulses import CustomWaveform, Pulse, Register, Rydberg, Sequence, VirtualDevice
from pulser_diff_amd.utils import basis_state, interpolate_sine

n_qubits = int(sys.argv[1]) if len(sys.argv) > 1 else 3
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 60
rate = float(sys.argv[3]) if len(sys.argv) > 3 else 0.05
device = VirtualDevice(name="MockDevice", dimensions=2, rydberg_level=60,
                       channel_objects=(Rydberg.Global(6.28, 12.566370614359172, max_duration=None),))
duration, n_param, gamma = 600, 20, 0.02
reg = Register.rectangle(1, n_qubits, torch.tensor([7.0]))
target = StateOverlap(basis_state(2 ** n_qubits, 0).to(torch.complex128))  # all atoms in the Rydberg state

seq = Sequence(reg, device)
seq.declare_channel("rydberg_global", "rydberg_global")
amp_var = seq.declare_variable("amp_custom", size=duration)
det_var = seq.declare_variable("det_custom", size=duration)
seq.add(Pulse(CustomWaveform(amp_var), CustomWaveform(det_var), 0.0), "rydberg_global")

channel = device.channels["rydberg_global"]
interp = interpolate_sine(n_param, duration)


def amp_shape(params):
    return interp @ (int(channel.max_amp) * torch.sigmoid(gamma * params))


def det_shape(params):
    return interp @ (int(channel.max_abs_detuning) * torch.tanh(gamma * params))


torch.manual_seed(int(sys.argv[4]) if len(sys.argv) > 4 else 1)
model = QuantumModel(seq, {"amp_custom": ((2 * torch.rand(n_param) - 1.0,), amp_shape),
                           "det_custom": ((2 * torch.rand(n_param) - 1.0,), det_shape)},
                     sampling_rate=0.05, noise_config=SimConfig(noise="dephasing", dephasing_rate=rate))  # collapse noise: DP5_ME


def infidelity(m):
    _, f = m.fidelity(target)  # real (n_t, 1): <target| rho(t) |target> at every evaluation time
    return 1 - f[-1, 0]


(best_loss, best_params, best_epoch), _ = train(model, infidelity, epochs, lr=5.0)
load_parameters(model, best_params)
with torch.no_grad():
    purity = Purity()
    _, results = model._run(observables=[target, purity], store_states=False, shots=1000)
print(f"best loss {best_loss:.6f} at epoch {best_epoch};  fidelity {100 * float(results.fidelity(target)[-1, 0]):.2f} %, "
      f"purity of the final state {float(results.purity()[-1, 0]):.4f} (dephasing rate {rate})")
shots = results.sample_final_state(1000)  # drawn from the diagonal of rho(T) on the device ('1' = Rydberg)
print("1000 shots of the final state:", ", ".join(f"{bits}: {count}" for bits, count in shots.most_common(4)))
