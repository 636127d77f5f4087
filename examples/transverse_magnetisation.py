#!/usr/bin/env python3
"""Transverse magnetisation <sum_j X_j>(t) of an 18-atom register and its gradient w.r.t. a pulse area, evaluated natively
(needs a GPU).  The dense route — `build_operator` and `results.expect` on stored states — would need a 2^18 x 2^18 operator;
here the observable is 18 Pauli strings and the trajectory is never stored."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from pulser_diff_amd import SolverType, TorchEmulator
from pulser_diff_amd.pulses import BlackmanWaveform, MockDevice, Pulse, RampWaveform, Register, Sequence

reg = Register.rectangle(3, 6, spacing=8, prefix="q")
area = torch.tensor(2.5, dtype=torch.float64, requires_grad=True)
seq = Sequence(reg, MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(Pulse(BlackmanWaveform(300, area), RampWaveform(300, -4.0, 2.0), 0.3), "ch")  # a constant phase: the solver's rotating frame
sim = TorchEmulator.from_sequence(seq, sampling_rate=0.2)

sum_x = sim.build_observable([("X", "global")])  # a PauliObservable: 18 strings
xx = sim.build_observable([("X", ["q0"]), ("X", ["q17"])])
results = sim.run(solver=SolverType.KRYLOV_SE, observables=[sum_x, xx], store_states=False)
mx, cxx = (v.real for v in results.expect([sum_x, xx]))
(d_area,) = torch.autograd.grad(mx[-1], area)
print(f"{len(mx)} evaluation times; <sum X>(T) = {mx[-1].item():+.6f}, <X_0 X_17>(T) = {cxx[-1].item():+.6f}, "
      f"d<sum X>(T)/d area = {d_area.item():+.6f}")
print("kernels:", results.solver_stats.get("kernel_fwd"), "/", results.solver_stats.get("kernel_bwd"))
