#!/usr/bin/env python3
"""Sensitivities of a NOISY run at every evaluation time, from ONE forward-mode sweep (needs a GPU).

Three atoms with dephasing and relaxation: the state is a density matrix, and the master equation runs on the doubled register.  The
tangent sweep carries vec(rho) and one tangent d vec(rho) / d theta per parameter through the sequence together — the dissipator is a
constant pair term of the same kernel — and emits d<sum Z>(t) / d(area, final detuning) and the derivative of the purity Tr rho^2(t) at
every evaluation time.  The loop of one-hot reverse sweeps it replaces (route="adjoint-loop") is run once for comparison."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import DiagonalObservable, SimConfig, TorchEmulator
from pulser_diff_amd.derivative import deriv_param_all_times
from pulser_diff_amd.observables import Purity
from pulser_diff_amd.pulses import BlackmanWaveform, MockDevice, Pulse, RampWaveform, Register, Sequence
from pulser_diff_amd.utils import total_magnetization_diag

n = 3
reg = Register({f"q{j}": torch.tensor([8.0 * j, 0.0], dtype=torch.float64) for j in range(n)})
area = torch.tensor([torch.pi], dtype=torch.float64, requires_grad=True)
detuning = torch.tensor([2.0], dtype=torch.float64, requires_grad=True)
seq = Sequence(reg, MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse(BlackmanWaveform(800, area), RampWaveform(800, -5.0, detuning), 0.0), "ch")
cfg = SimConfig(noise=("dephasing", "relaxation"), dephasing_rate=0.5, relaxation_rate=0.3)
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, config=cfg, evaluation_times=0.2)

obs = [DiagonalObservable(total_magnetization_diag(n)), Purity()]
sens = deriv_param_all_times(sim, [area, detuning], obs, route="tangent")
loop = deriv_param_all_times(sim, [area, detuning], obs, route="adjoint-loop")
worst = max(float((a.cpu() - b.cpu()).abs().max()) for a, b in zip(sens.grads, loop.grads))
print(f"route: {sens.route} (against {loop.route}: largest difference {worst:.1e})")
print("   t [us]     <sum Z>   d/d area   d/d detuning      purity   d/d area   d/d detuning")
for k, t in enumerate(sens.times.tolist()):
    z, p = sens.values[0, k].item(), sens.values[1, k].item()
    dz = (sens.grads[0][0, k, 0].item(), sens.grads[1][0, k, 0].item())
    dp = (sens.grads[0][1, k, 0].item(), sens.grads[1][1, k, 0].item())
    print(f"  {t:7.3f}   {z:+9.5f}   {dz[0]:+8.5f}   {dz[1]:+12.5f}   {p:9.5f}   {dp[0]:+8.5f}   {dp[1]:+12.5f}")
