#!/usr/bin/env python3
"""How the entanglement of half a Rydberg chain responds to the pulse, at EVERY evaluation time, from one sweep (needs a GPU): the
6-atom chain of examples/entanglement_growth.py under a Blackman pulse followed by a constant one.  run_rdm_sensitivities carries the
state and one tangent state per parameter through the solver once and forms rho_A(t_k) = Tr_E |psi><psi| and
d rho_A(t_k) / d(Omega, delta, area) natively at every save point; d purity = 2 Re tr(rho_A d rho_A) follows in torch.  The loop it
replaces — one reverse sweep per evaluation time through run(observables=[left_half]) — is run for the last time only, as a check.
Usage:  python examples/entanglement_sensitivities.py [n_atoms]   (default 6)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SolverType, TorchEmulator
from pulser_diff_amd.derivative import deriv_rdm_all_times
from pulser_diff_amd.pulses import BlackmanWaveform, MockDevice, Pulse, RampWaveform, Register, Sequence
from pulser_diff_amd.utils import purity

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 6
omega = torch.tensor([4.0], dtype=torch.float64, requires_grad=True)
delta = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
area = torch.tensor([3.0], dtype=torch.float64, requires_grad=True)

seq = Sequence(Register.rectangle(1, n_atoms, torch.tensor([7.0], dtype=torch.float64)), MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse(BlackmanWaveform(400, area), RampWaveform(400, -2.0, delta), 0), "ch")
seq.add(Pulse.ConstantPulse(200, omega, delta, 0.0), "ch")
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1)
left_half = sim.build_reduced_density_matrix(list(seq.register.qubits)[: n_atoms // 2])

sens = deriv_rdm_all_times(sim, [omega, delta, area], [left_half], solver=SolverType.KRYLOV_SE)
p = sens.purity(0)[:, 0]
d_omega, d_delta, d_area = (g[:, 0, 0] for g in sens.d_purity(0))
step = max(1, len(sens.times) // 12)
for k in range(0, len(sens.times), step):
    print(f"t = {float(sens.times[k]):6.3f} us   purity(left half) = {float(p[k]):.6f}   d/dOmega = {float(d_omega[k]):+.6f}   "
          f"d/ddelta = {float(d_delta[k]):+.6f}   d/darea = {float(d_area[k]):+.6f}")

# the loop this replaces, for the last evaluation time only: one reverse sweep per time (and per scalar functional of rho_A)
results = sim.run(solver=SolverType.KRYLOV_SE, observables=[left_half], store_states=False)
purity(results.reduced_density_matrix(left_half)[-1, 0]).backward()
print(f"reverse sweep at the final time: d/dOmega = {float(omega.grad):+.6f}   d/ddelta = {float(delta.grad):+.6f}   d/darea = {float(area.grad):+.6f}")
