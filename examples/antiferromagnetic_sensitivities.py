#!/usr/bin/env python3
"""At which time is the Neel order of a chain most sensitive to the pulse (needs a GPU)?  The rise - sweep - fall pulse of
examples/antiferromagnetic_order.py on a 6-atom chain; run_occupation_sensitivities returns every <n_i> and <n_i n_j> AND their
derivatives w.r.t. the three pulse parameters at EVERY evaluation time from one forward-mode sweep: the state and one tangent state per
parameter advance together, and the moments of |psi|^2 and of 2 Re(conj psi . dpsi) are formed natively at every save point.  Printed:
    S_Neel(t) = sum_ij (-1)^(i+j) g_ij(t) / N   and   d S_Neel(t) / d (amplitude, initial detuning, final detuning)
and, for the last time only, the loop this replaces: one reverse sweep per evaluation time through run(observables=[OccupationCorrelations()]).
Usage:  python examples/antiferromagnetic_sensitivities.py [n_atoms]   (default 6)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import OccupationCorrelations, SolverType, TorchEmulator
from pulser_diff_amd.derivative import deriv_occupations_all_times
from pulser_diff_amd.pulses import MockDevice, Pulse, RampWaveform, Register, Sequence

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 6
omega = torch.tensor([4.0], dtype=torch.float64, requires_grad=True)         # plateau amplitude, rad/us
delta_start = torch.tensor([-6.0], dtype=torch.float64, requires_grad=True)  # detuning during the rise
delta_stop = torch.tensor([6.0], dtype=torch.float64, requires_grad=True)    # detuning during the fall
neel = [(-1) ** i for i in range(n_atoms)]

seq = Sequence(Register.rectangle(1, n_atoms, torch.tensor([6.5])), MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse.ConstantDetuning(RampWaveform(200, 0.0, omega), delta_start, 0), "ch")
seq.add(Pulse.ConstantAmplitude(omega, RampWaveform(600, delta_start, delta_stop), 0), "ch")
seq.add(Pulse.ConstantDetuning(RampWaveform(200, omega, 0.0), delta_stop, 0), "ch")
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, evaluation_times=0.2)

x = [omega, delta_start, delta_stop]
sens = deriv_occupations_all_times(sim, x, solver=SolverType.KRYLOV_SE)
s_neel = sens.structure_factor(neel)[:, 0]
d_omega, d_start, d_stop = (g[:, 0, 0] for g in sens.d_structure_factor(neel))
for k in range(len(sens.times)):
    print(f"t = {float(sens.times[k]):6.3f} us   S_Neel = {float(s_neel[k]):+.6f}   d/dOmega = {float(d_omega[k]):+.6f}   "
          f"d/ddelta_start = {float(d_start[k]):+.6f}   d/ddelta_stop = {float(d_stop[k]):+.6f}")
k_max = int(d_stop.abs().argmax())
print(f"the structure factor is most sensitive to the final detuning at t = {float(sens.times[k_max]):.3f} us")
g01 = sens.d_correlations(connected=True)[2][:, 0, 0, 1, 0]
print("d g_01(t) / d delta_stop:", " ".join(f"{float(v):+.4f}" for v in g01))

# the loop this replaces, for the last evaluation time only: one reverse sweep per time (and per scalar functional)
results = sim.run(solver=SolverType.KRYLOV_SE, observables=[OccupationCorrelations()], store_states=False)
loop = torch.autograd.grad(results.structure_factor(neel)[-1], x)
print("last time, reverse sweep:", " ".join(f"{float(g):+.6f}" for g in loop), "  tangent sweep:",
      " ".join(f"{float(v[-1]):+.6f}" for v in (d_omega, d_start, d_stop)))
