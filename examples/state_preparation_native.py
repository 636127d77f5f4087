#!/usr/bin/env python3
"""examples/state_preparation.py with the fidelity evaluated natively (needs a GPU): the loss is 1 - |c(T)|^2 with
c = <target|psi(T)> from `model.overlap` — a StateOverlap observable evaluated and differentiated inside the solver, so no trajectory
is stored and autograd never sees a 2^N-sized tensor.  Same register, pulse shapes, seeds and optimiser as state_preparation.py, and
the same fidelity to the printed digits; the atom count is an argument because this route keeps working where the stored trajectory
and its dense grad_states no longer fit.  Usage:  python examples/state_preparation_native.py [n_atoms [epochs [seed]]]
(defaults 6, 300, 1)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import torch

from optimal_control_loop import load_parameters, train
from pulser_diff_amd import QuantumModel, SolverType, StateOverlap
from pulser_diff_amd.pulses import CustomWaveform, Pulse, Register, Rydberg, Sequence, VirtualDevice
from pulser_diff_amd.utils import basis_state, interpolate_sine

n_qubits = int(sys.argv[1]) if len(sys.argv) > 1 else 6
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 300
device = VirtualDevice(name="MockDevice", dimensions=2, rydberg_level=60,
                       channel_objects=(Rydberg.Global(6.28, 12.566370614359172, max_duration=None),))
duration, n_param, gamma = 1100, 30, 0.02
reg = Register.rectangle(1, n_qubits, torch.tensor([7.0]))
target = StateOverlap(basis_state(2 ** n_qubits, 0).to(torch.complex128))

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


torch.manual_seed(int(sys.argv[3]) if len(sys.argv) > 3 else 1)
model = QuantumModel(seq, {"amp_custom": ((2 * torch.rand(n_param) - 1.0,), amp_shape),
                           "det_custom": ((2 * torch.rand(n_param) - 1.0,), det_shape)},
                     sampling_rate=0.05, solver=SolverType.DP5_SE)


def infidelity(m):
    _, c = m.overlap(target)  # complex (n_t, 1): the overlap at every evaluation time
    return 1 - c[-1, 0].abs() ** 2


(best_loss, best_params, best_epoch), _ = train(model, infidelity, epochs, lr=5.0)
load_parameters(model, best_params)
print(f"best loss {best_loss:.6f} at epoch {best_epoch};  state fidelity now {100 * (1 - float(infidelity(model).detach())):.2f} %")
# measurement shots of the trained run, drawn natively as well: still no stored states ('1' = Rydberg; the target is all-Rydberg)
shots = model.sample_final_state(1000)
print("1000 shots of the final state:", ", ".join(f"{bits}: {count}" for bits, count in shots.most_common(4)))
