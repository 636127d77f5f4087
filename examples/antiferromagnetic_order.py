#!/usr/bin/env python3
"""Antiferromagnetic-state preparation on a chain of Rydberg atoms, steered by the observable experiments report (needs a GPU): every
<n_i> and <n_i n_j> of the register is an OccupationCorrelations observable, evaluated inside the solver from one read of the state per
evaluation time, so the run keeps no trajectory (store_states=False) and hands autograd no 2^N-sized tensor.  The pulse is the usual
rise - sweep - fall: the amplitude ramps up at a negative detuning, the detuning sweeps to a positive value, the amplitude ramps down.
Its three parameters (plateau amplitude, initial and final detuning) are trained with Adam on
    loss = - S_Neel(T),   S_Neel = sum_ij (-1)^(i+j) g_ij / N,   g_ij = <n_i n_j> - <n_i><n_j>,
the Neel structure factor of the connected correlations at the final time.
Usage:  python examples/antiferromagnetic_order.py [n_atoms [steps]]   (defaults 8, 200)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import OccupationCorrelations, SolverType, TorchEmulator
from pulser_diff_amd.pulses import MockDevice, Pulse, RampWaveform, Register, Sequence

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
omega = torch.tensor([4.0], dtype=torch.float64, requires_grad=True)       # plateau amplitude, rad/us
delta_start = torch.tensor([-6.0], dtype=torch.float64, requires_grad=True)  # detuning during the rise
delta_stop = torch.tensor([6.0], dtype=torch.float64, requires_grad=True)    # detuning during the fall
neel = [(-1) ** i for i in range(n_atoms)]
t_rise, t_sweep, t_fall = 200, 600, 200  # ns


def simulate():
    seq = Sequence(Register.rectangle(1, n_atoms, torch.tensor([6.5])), MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(Pulse.ConstantDetuning(RampWaveform(t_rise, 0.0, omega), delta_start, 0), "ch")
    seq.add(Pulse.ConstantAmplitude(omega, RampWaveform(t_sweep, delta_start, delta_stop), 0), "ch")
    seq.add(Pulse.ConstantDetuning(RampWaveform(t_fall, omega, 0.0), delta_stop, 0), "ch")
    sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1)
    return sim.run(solver=SolverType.KRYLOV_SE, observables=[OccupationCorrelations()], store_states=False)


first = float(simulate().structure_factor(neel)[-1].detach())
optimiser = torch.optim.Adam([omega, delta_start, delta_stop], lr=0.1)
for step in range(steps):
    optimiser.zero_grad()
    loss = -simulate().structure_factor(neel)[-1]
    loss.backward()
    optimiser.step()
    if step % max(1, steps // 10) == 0:
        print(f"step {step:4d}   S_Neel(T) = {-float(loss.detach()):.6f}")
results = simulate()
print(f"Neel structure factor at the final time: {first:.6f} before, {float(results.structure_factor(neel)[-1].detach()):.6f} after {steps} Adam steps")
print(f"  amplitude {float(omega.detach()):.4f} rad/us, detuning {float(delta_start.detach()):+.4f} -> {float(delta_stop.detach()):+.4f} rad/us")
print("  <n_i>(T):", " ".join(f"{v:.3f}" for v in results.occupations()[-1].detach().tolist()))
g = results.occupation_correlations(connected=True)[-1].detach()
print("  g_0j(T) along the chain:", " ".join(f"{v:+.3f}" for v in g[0].tolist()))
