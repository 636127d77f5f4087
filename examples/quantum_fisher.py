#!/usr/bin/env python3
"""Quantum Fisher information of a Ramsey sequence at every evaluation time, from ONE forward-mode sweep (needs a GPU).

Three atoms far apart (30 um: interactions of 0.007 rad/us) get a pi/2 pulse and then precess freely under a detuning delta.  Used
as a sensor for delta, n independent atoms give F(t) = n t^2 — the shot-noise line; the Cramer-Rao bound on the variance of an
estimate of delta from M repetitions is 1 / (M F).  `run_quantum_fisher` carries the state and d psi / d delta through the sequence
together and reduces their inner products at every evaluation time: no state is stored, nothing is differentiated twice."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SolverType, TorchEmulator
from pulser_diff_amd.pulses import MockDevice, Pulse, Register, Sequence

n, t_pulse, t_free = 3, 100, 1000  # ns
reg = Register({f"q{j}": torch.tensor([30.0 * j, 0.0], dtype=torch.float64) for j in range(n)})
delta = torch.tensor([0.8], dtype=torch.float64, requires_grad=True)
omega = torch.tensor([torch.pi / 2 / (t_pulse / 1000)], dtype=torch.float64, requires_grad=True)  # area pi / 2
seq = Sequence(reg, MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse.ConstantPulse(t_pulse, omega, 0.0, 0.0), "ch")
seq.add(Pulse.ConstantPulse(t_free, 0.0, delta, 0.0), "ch")
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, evaluation_times=0.1)

geo = sim.run_quantum_fisher([delta, omega], solver=SolverType.DP5_SE)
print(f"route: {geo.route}; qfi {tuple(geo.qfi.shape)} = (evaluation times, parameters, parameters)")
print("   t [us]   F_delta,delta   n (t - t_pulse)^2   F_omega,omega   F_delta,omega")
for t, f in zip(geo.times.tolist(), geo.qfi.cpu()):
    free = max(t - t_pulse / 1000, 0.0)
    print(f"  {t:7.3f}   {f[0, 0].item():13.6f}   {n * free**2:17.6f}   {f[1, 1].item():13.6f}   {f[0, 1].item():+13.6f}")
