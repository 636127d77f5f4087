#!/usr/bin/env python3
"""Ground-state preparation scored by the energy itself (needs a GPU): a 3 x 4 array of Rydberg atoms is driven through the usual
rise - sweep - fall ramp towards the antiferromagnetic phase, and the three pulse parameters (plateau amplitude, initial and final
detuning) are trained with Adam on
    loss = E(T) = <psi(T)| H(T) |psi(T)>,
the energy of the final state under the sequence's own final Hamiltonian — no target state is known or needed.  Energy() is
evaluated inside the solver from the state while it is on the device, so the run keeps no trajectory (store_states=False), and
H(t_k) is the sequence's Hamiltonian at the evaluation times: the gradient includes the explicit dependence of H(T) on the final
detuning.  The variance <H^2> - <H>^2 along the sequence tells how far the state is from any eigenstate of H(t): the adiabaticity
of the ramp at every time.
Usage:  python examples/ground_state_energy.py [rows cols [steps]]   (defaults 3 4, 60)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import Energy, SolverType, TorchEmulator
from pulser_diff_amd.pulses import MockDevice, Pulse, RampWaveform, Register, Sequence

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cols = int(sys.argv[2]) if len(sys.argv) > 2 else 4
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 60
omega = torch.tensor([4.0], dtype=torch.float64, requires_grad=True)         # plateau amplitude, rad/us
delta_start = torch.tensor([-6.0], dtype=torch.float64, requires_grad=True)  # detuning during the rise
delta_stop = torch.tensor([5.0], dtype=torch.float64, requires_grad=True)    # detuning during the fall
t_rise, t_sweep, t_fall = 200, 600, 200  # ns


def simulate():
    seq = Sequence(Register.rectangle(rows, cols, torch.tensor([6.5])), MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(Pulse.ConstantDetuning(RampWaveform(t_rise, 0.0, omega), delta_start, 0), "ch")
    seq.add(Pulse.ConstantAmplitude(omega, RampWaveform(t_sweep, delta_start, delta_stop), 0), "ch")
    seq.add(Pulse.ConstantDetuning(RampWaveform(t_fall, omega, 0.0), delta_stop, 0), "ch")
    sim = TorchEmulator.from_sequence(seq, sampling_rate=0.1)
    return sim, sim.run(solver=SolverType.KRYLOV_SE, observables=[Energy()], store_states=False)


first = float(simulate()[1].energy()[-1].detach())
optimiser = torch.optim.Adam([omega, delta_start, delta_stop], lr=0.1)
for step in range(steps):
    optimiser.zero_grad()
    loss = simulate()[1].energy()[-1]
    loss.backward()
    optimiser.step()
    with torch.no_grad():
        omega.clamp_(0.5, 10.0)
    if step % max(1, steps // 10) == 0:
        print(f"step {step:4d}   E(T) = {float(loss.detach()):+.6f} rad/us")
sim, results = simulate()
energy, variance = results.energy().detach(), results.energy_variance().detach()
print(f"final energy: {first:+.6f} before, {float(energy[-1]):+.6f} rad/us after {steps} Adam steps ({rows} x {cols} atoms)")
print(f"  amplitude {float(omega.detach()):.4f} rad/us, detuning {float(delta_start.detach()):+.4f} -> {float(delta_stop.detach()):+.4f} rad/us")
print("  along the sequence:   t (ns)        E(t)      <H^2> - <H>^2")
times = sim.evaluation_times.detach()
for k in range(0, len(times), max(1, len(times) // 12)):
    print(f"                      {1000 * float(times[k]):8.1f}  {float(energy[k]):+10.4f}  {float(variance[k]):12.5f}")
