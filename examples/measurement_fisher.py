#!/usr/bin/env python3
"""Classical against quantum Fisher information of a Ramsey sequence at every evaluation time, from ONE forward-mode sweep (needs a
GPU).

Three atoms far apart (30 um) get a pi/2 pulse, precess freely under a detuning delta and get a second pi/2 pulse.  The quantum
Fisher information F_Q(t) is the bound for the best conceivable measurement of the state at time t; a Rydberg device has one
measurement, bitstrings in the occupation basis, and the classical Fisher information F_C(t) of their distribution is what M shots
taken at time t can deliver: Var(estimate) >= 1 / (M F_C).  During the free precession delta only moves phases — F_Q grows like
n t^2 while F_C stays 0: the information is in the state, the measurement does not see it.  The second pulse turns the phase into
populations and F_C rises to F_Q.  For the drive amplitude omega the occupations carry the information all along.
`run_classical_fisher` reduces both from the state and the tangent states the sweep holds at every evaluation time: no state is
stored, no probability vector is differentiated."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SolverType, TorchEmulator, fisher_efficiency
from pulser_diff_amd.pulses import MockDevice, Pulse, Register, Sequence

n, t_pulse, t_free = 3, 100, 600  # ns
reg = Register({f"q{j}": torch.tensor([30.0 * j, 0.0], dtype=torch.float64) for j in range(n)})
delta = torch.tensor([0.8], dtype=torch.float64, requires_grad=True)
omega = torch.tensor([torch.pi / 2 / (t_pulse / 1000)], dtype=torch.float64, requires_grad=True)  # area pi / 2
seq = Sequence(reg, MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse.ConstantPulse(t_pulse, omega, 0.0, 0.0), "ch")
seq.add(Pulse.ConstantPulse(t_free, 0.0, delta, 0.0), "ch")
seq.add(Pulse.ConstantPulse(t_pulse, omega, 0.0, 0.0), "ch")
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, evaluation_times=0.1)

out = sim.run_classical_fisher([delta, omega], solver=SolverType.DP5_SE)
ratio = fisher_efficiency(out.cgram, out.gram).cpu()  # per parameter; NaN where the state does not depend on it yet
print(f"route: {out.route}; cfi {tuple(out.cfi.shape)} = (evaluation times, parameters, parameters)")
print("   t [us]   F_C delta     F_Q delta     F_C / F_Q   |   F_C omega     F_Q omega     F_C / F_Q")
for t, fc, fq, r in zip(out.times.tolist(), out.cfi.cpu(), out.qfi.cpu(), ratio):
    print(f"  {t:7.3f}   {fc[0, 0].item():11.6f}   {fq[0, 0].item():11.6f}   {r[0].item():9.6f}   |   "
          f"{fc[1, 1].item():11.6f}   {fq[1, 1].item():11.6f}   {r[1].item():9.6f}")
