#!/usr/bin/env python3
"""Quantum and classical Fisher information of a 3 x 3 XY register with respect to its lattice spacing, at every evaluation time, from
ONE forward-mode sweep on the native exchange term (needs a GPU).

Nine atoms on a square lattice of spacing a exchange excitations with J_ij = C3 (1 - 3 cos^2 theta_ij) / r_ij^3 while a microwave
drive turns them.  Every coupling scales like a^-3, so the state carries information about the spacing: F_Q(t) bounds what any
measurement of the state at time t can tell about a, F_C(t) is what the device's one measurement — bitstrings in the occupation
basis — delivers, Var(estimate) >= 1 / (M F_C) for M shots.  Nine atoms are past the 8 of the dense pair-term route, and a coordinate
is a direction dense blocks cannot take at all: `xy_native=True` runs the sweep on the exchange stencil, whose couplings have tangents
of their own (RydTangent.d_xy).  No state is stored and no reverse sweep runs."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SolverType, TorchEmulator, fisher_efficiency
from pulser_diff_amd.pulses import MockDevice, Pulse, Register, Sequence

spacing = torch.tensor(8.0, dtype=torch.float64, requires_grad=True)  # um
cells = torch.tensor([[i, j] for i in range(3) for j in range(3)], dtype=torch.float64)
reg = Register.from_coordinates(spacing * cells)
seq = Sequence(reg, MockDevice)
seq.declare_channel("mw", "mw_global")
seq.set_magnetic_field(0.0, 1.0, 0.3)
seq.add(Pulse.ConstantPulse(400, 2.0 * torch.pi, 0.0, 0.0), "mw")
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, evaluation_times=0.25, xy_hermitian=True, xy_native=True)

out = sim.run_classical_fisher([spacing], solver=SolverType.KRYLOV_SE)
ratio = fisher_efficiency(out.cgram, out.gram).cpu()  # NaN where the state does not depend on the spacing yet
print(f"route: {out.route}; exchange route: {sim._hamiltonian.xy_route()}; sum |J| = {float(sim._hamiltonian.xy_pairs.detach().abs().sum()):.3f} rad/us")
print("   t [us]   F_Q spacing [1/um^2]   F_C spacing   F_C / F_Q   shots for 10 nm")
for t, fq, fc, r in zip(out.times.tolist(), out.qfi.cpu(), out.cfi.cpu(), ratio):
    shots = float("inf") if fc[0, 0].item() <= 0.0 else 1.0 / (fc[0, 0].item() * 0.01**2)
    print(f"  {t:7.3f}   {fq[0, 0].item():18.6f}   {fc[0, 0].item():11.6f}   {r[0].item():9.6f}   {shots:14.0f}")
