"""MI355X-native differentiable time-evolution backend for Rydberg pulse sequences.

Drop-in for the hot path of ``pulser_diff`` (``pulser_diff/__init__.py:17-18`` exports ``TorchEmulator`` and
``SimConfig``): same class / method names and argument meaning; the per-step Hamiltonian assembly, the
matrix-exponential-on-vector, expectation values and the adjoint gradient sweep run as hand-written HIP kernels
behind the C ABI in ``include/rydiff.h``.
"""
from pulser_diff_amd.backend import OccupationSensitivities, TorchEmulator  # noqa: F401
from pulser_diff_amd.model import QuantumModel  # noqa: F401
from pulser_diff_amd.simconfig import SimConfig  # noqa: F401
from pulser_diff_amd.solver import SolverType  # noqa: F401
from pulser_diff_amd.utils import DiagonalObservable, logarithmic_negativity, negativity, partial_transpose  # noqa: F401
from pulser_diff_amd.observables import Energy, OccupationCorrelations, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap  # noqa: F401
from pulser_diff_amd.geometry import (MeasurementFisher, QuantumGeometry, berry_curvature, classical_fisher_information,  # noqa: F401
                                      fisher_efficiency, quantum_fisher_information, quantum_geometric_tensor)

__all__ = ["TorchEmulator", "SimConfig", "SolverType", "DiagonalObservable", "PauliObservable", "StateOverlap", "ReducedDensityMatrix", "Purity", "OccupationCorrelations", "Energy", "OccupationSensitivities", "QuantumModel",
           "QuantumGeometry", "quantum_geometric_tensor", "quantum_fisher_information", "berry_curvature",
           "MeasurementFisher", "classical_fisher_information", "fisher_efficiency",
           "partial_transpose", "negativity", "logarithmic_negativity"]
