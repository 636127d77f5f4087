#!/usr/bin/env python3
"""The noisy twin of examples/antiferromagnetic_order.py (needs a GPU): antiferromagnetic order on a small ring of Rydberg atoms under
dephasing.  Collapse noise makes the run a master-equation one; OccupationCorrelations() is then served from the diagonal of rho while
it is on the device (RydProblem.dm_moments: every <n_i> and <n_i n_j> from 2^n real parts per evaluation time), so the run keeps no
4^n trajectory (store_states=False) and its gradient needs none.  The pulse is the rise - sweep - fall of the clean example; printed
are the Neel structure factor
    S_Neel = sum_ij (-1)^(i+j) g_ij / N,   g_ij = <n_i n_j> - <n_i><n_j>
along the run, at the final time for several dephasing rates, and its gradient w.r.t. the two ends of the detuning ramp.
Usage:  python examples/noisy_antiferromagnetic_order.py [n_atoms [dephasing_rate]]   (defaults 6, 0.2; an even number of atoms)."""
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import OccupationCorrelations, SimConfig, TorchEmulator
from pulser_diff_amd.pulses import MockDevice, Pulse, RampWaveform, Register, Sequence

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 6
rate = float(sys.argv[2]) if len(sys.argv) > 2 else 0.2
omega = torch.tensor([4.0], dtype=torch.float64)                               # plateau amplitude, rad/us
delta_start = torch.tensor([-6.0], dtype=torch.float64, requires_grad=True)  # detuning during the rise
delta_stop = torch.tensor([6.0], dtype=torch.float64, requires_grad=True)    # detuning during the fall
neel = [(-1) ** i for i in range(n_atoms)]
t_rise, t_sweep, t_fall = 200, 600, 200  # ns
radius = 6.5 / (2.0 * math.sin(math.pi / n_atoms))  # neighbours 6.5 um apart
ring = {f"q{i}": torch.tensor([radius * math.cos(2 * math.pi * i / n_atoms), radius * math.sin(2 * math.pi * i / n_atoms)], dtype=torch.float64)
        for i in range(n_atoms)}


def simulate(dephasing_rate):
    seq = Sequence(Register(ring), MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(Pulse.ConstantDetuning(RampWaveform(t_rise, 0.0, omega), delta_start, 0), "ch")
    seq.add(Pulse.ConstantAmplitude(omega, RampWaveform(t_sweep, delta_start, delta_stop), 0), "ch")
    seq.add(Pulse.ConstantDetuning(RampWaveform(t_fall, omega, 0.0), delta_stop, 0), "ch")
    config = SimConfig(noise="dephasing", dephasing_rate=dephasing_rate)
    sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1, config=config, evaluation_times=0.1)
    return sim, sim.run(observables=[OccupationCorrelations()], store_states=False)  # dephasing forces the master equation


sim, results = simulate(rate)
s_neel = results.structure_factor(neel)
times = sim.evaluation_times
print(f"{n_atoms} atoms on a ring, dephasing rate {rate} / us: S_Neel along the run")
for k in range(0, len(times), max(1, len(times) // 8)):
    print(f"  t = {float(times[k]) * 1000:6.0f} ns   S_Neel = {float(s_neel[k].detach()):+.6f}")
g_start, g_stop = torch.autograd.grad(s_neel[-1], [delta_start, delta_stop])
print(f"S_Neel(T) = {float(s_neel[-1].detach()):.6f};  d S_Neel(T) / d delta_start = {float(g_start):+.6f},  / d delta_stop = {float(g_stop):+.6f} us/rad")
print("  <n_i>(T):", " ".join(f"{v:.3f}" for v in results.occupations()[-1].detach().tolist()))
g = results.occupation_correlations(connected=True)[-1].detach()
print("  g_0j(T) around the ring:", " ".join(f"{v:+.3f}" for v in g[0].tolist()))
for other in (0.0, 0.05, 1.0):
    value = float(simulate(other)[1].structure_factor(neel)[-1].detach())
    print(f"  dephasing rate {other:4.2f} / us: S_Neel(T) = {value:.6f}")
