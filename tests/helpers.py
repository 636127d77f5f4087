"""Shared helpers for the parity tests: build the same problem for the CPU oracle and for the native library."""
from __future__ import annotations

import itertools

import numpy as np
import torch

from oracle import restatement as R


def random_terms(n_qubits: int, n_samples: int, dt: float, seed: int, local: bool = False, spacing: float = 8.0,
                 amp_scale: float = 6.0, det_scale: float = 5.0, phase: bool = True) -> R.HamTerms:
    """Random but smooth coefficient arrays (seeded) on a jittered chain register."""
    g = torch.Generator().manual_seed(seed)
    coords = torch.stack([torch.arange(n_qubits, dtype=torch.float64) * spacing,
                          torch.rand(n_qubits, generator=g, dtype=torch.float64) * 2.0], dim=1)
    t = torch.linspace(0, 1, n_samples, dtype=torch.float64)
    amp = amp_scale * torch.sin(np.pi * t) ** 2 * (1 + 0.3 * torch.rand(1, generator=g, dtype=torch.float64))
    ph = (0.7 * t + 0.2) if phase else torch.zeros_like(t)
    amp_c = 0.5 * amp * torch.exp(-1j * ph.to(torch.complex128))
    det_c = -0.5 * det_scale * (2 * t - 1 + 0.1 * torch.rand(1, generator=g, dtype=torch.float64))
    terms = R.HamTerms(n_qubits, R.interaction_strengths(coords), amp_c, det_c, dt, n_samples,
                       list(range(n_qubits)), list(range(n_qubits)))
    if local:
        q1 = [n_qubits // 2]
        q2 = [0, n_qubits - 1] if n_qubits > 1 else [0]
        terms.extra_amp = [(0.5 * 3.0 * torch.cos(2.0 * t).to(torch.complex128) * np.exp(-0.4j), q1)]
        terms.extra_det = [(-0.5 * 2.0 * torch.sin(3.0 * t), q2)]
    return terms


RHO_CAP = 6.0  # kRhoCap (csrc/plan.hpp): an exponential with tau * half_width above it is split into ceil(tau * half_width / 6) sub-exponentials
# Save-interval lengths in units of RHO_CAP / half_width; every entry at least 0.1 away from an integer, so that the sub-step
# counts ceil(ratio) do not hinge on rounding.  MIXED: (1, 2, 1, 3, 2) sub-exponentials; TWOS: (1, 2, 1, 2, 2).
SUBSTEP_RATIOS = {"MIXED": (0.6, 1.6, 0.3, 2.5, 1.4), "TWOS": (0.6, 1.6, 0.3, 1.9, 1.4)}
SUBSTEP_COUNTS = {"MIXED": (1, 2, 1, 3, 2), "TWOS": (1, 2, 1, 2, 2)}


def gershgorin_half_width(terms) -> float:
    """CPU restatement of the library's spectral bound (k_table_stats / run_stats, csrc) for a HamTerms without pair terms, or for a
    list of them (one table set per trajectory on one register: every maximum runs over all of them).  With c_q / det_q the flip
    and detuning coefficients summed per qubit,  flip = max over samples of sum_q |c_q|,  d+ / d- = max over samples of
    sum_q max(+-2 det_q, 0),  U+ / U- = sum of the positive / negative pair interactions:
        half width = (U+ + U- + d+ + d-) / 2 + flip,
    an upper bound of (lambda_max - lambda_min) / 2 of H(t) at every sample (and, H being linear in the tables, in between)."""
    sets = list(terms) if isinstance(terms, (list, tuple)) else [terms]
    flip = dpos = dneg = 0.0
    for tr in sets:
        c_q = torch.zeros(tr.n_qubits, tr.n_samples, dtype=torch.complex128)
        d_q = torch.zeros(tr.n_qubits, tr.n_samples, dtype=torch.float64)
        for c, targets in tr.amp_terms():
            for q in targets:
                c_q[q] += c.detach().to(torch.complex128)
        for d, targets in tr.det_terms():
            for q in targets:
                d_q[q] += 2.0 * d.detach().to(torch.float64)
        flip = max(flip, float(c_q.abs().sum(0).max()))
        dpos = max(dpos, float(d_q.clamp(min=0).sum(0).max()))
        dneg = max(dneg, float((-d_q).clamp(min=0).sum(0).max()))
    u = sets[0].u_pairs.detach().to(torch.float64)
    return 0.5 * (float(u.clamp(min=0).sum()) + float((-u).clamp(min=0).sum()) + dpos + dneg) + flip


def substepped_tsave(half_width: float, ratios) -> torch.Tensor:
    """Save times 0 = t_0 < t_1 < ... with t_{k+1} - t_k = ratios[k] * RHO_CAP / half_width: interval k then takes
    ceil(ratios[k]) sub-exponentials.  Not rounded to any sample grid."""
    tau = torch.tensor(ratios, dtype=torch.float64) * (RHO_CAP / float(half_width))
    return torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(tau, 0)])


def mask_of(targets) -> int:
    m = 0
    for q in targets:
        m |= 1 << q
    return m


def to_native(terms: R.HamTerms, device, solver, tol: float = 0.0, store_states: bool = True, batch_tables: int = 1):
    """HamTerms -> (amp_tables, det_tables, u_pairs, spec) on `device` (tables shaped [Bc, K, n])."""
    from pulser_diff_amd.solver import ProblemSpec

    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    n = terms.n_samples
    amp = (torch.stack([c.to(torch.complex128) for c, _ in amp_terms]) if amp_terms
           else torch.zeros(0, n, dtype=torch.complex128))
    det = (torch.stack([c.to(torch.float64) for c, _ in det_terms]) if det_terms
           else torch.zeros(0, n, dtype=torch.float64))
    amp = amp.unsqueeze(0).repeat(batch_tables, 1, 1).to(device)
    det = det.unsqueeze(0).repeat(batch_tables, 1, 1).to(device)
    spec = ProblemSpec(terms.n_qubits, terms.dt, n, tuple(mask_of(tg) for _, tg in amp_terms),
                       tuple(mask_of(tg) for _, tg in det_terms), solver=solver, tol=tol, store_states=store_states)
    return amp, det, terms.u_pairs.detach().to(device), spec


def rel_err(a, b) -> float:
    a = np.asarray(a)
    b = np.asarray(b)
    den = max(float(np.abs(b).max()), 1e-300)
    return float(np.abs(a - b).max() / den)


def magnus_cf4_dense(terms, psi0, tsave, h_max=2.5e-3):
    """Torch (differentiable) model of the native continuous-time scheme: cut every tsave interval at the sample grid
    (H(t) is linear in t on each piece, hamiltonian.py:532-542), advance each piece with S = ceil(h/h_max) CF4 Magnus
    sub-steps exp(-i h/2 H(t0+5h/6)) exp(-i h/2 H(t0+h/6)).  Used to check the native adjoint tightly; the accuracy
    claim itself is checked against the DOP853 oracle (R.continuous_solution)."""
    import math

    dt, n = terms.dt, terms.n_samples
    psi = psi0
    out = [psi]
    for k in range(len(tsave) - 1):
        a, b = tsave[k], tsave[k + 1]
        fa, fb = float(a), float(b)
        pts = [a]
        i = math.floor(fa / dt) + 1
        while i <= n - 2 and i * dt < fb - 1e-13:
            if i * dt > fa + 1e-13:
                pts.append(torch.tensor(i * dt, dtype=torch.float64))
            i += 1
        pts.append(b)
        for p0, p1 in zip(pts[:-1], pts[1:]):
            hf = p1 - p0
            S = max(1, math.ceil(float(hf) / h_max - 1e-9))
            for sub in range(S):
                for theta in (1.0 / 6.0, 5.0 / 6.0):
                    mu = (sub + theta) / S
                    h = R.dense_hamiltonian(terms, p0 + mu * hf)
                    psi = torch.linalg.matrix_exp(-1j * h * (hf / (2.0 * S))) @ psi
        out.append(psi)
    return torch.stack(out)


DP5_DEFAULT_H_MAX = 2.5e-3 * (1e-9 / 1e-10) ** 0.25  # the native default (tol 1e-9), as tests/test_gpu_tangent.py's oracle test


def map_exponentials(terms, tsave, solver, h_max=DP5_DEFAULT_H_MAX):
    """The exponentials exp(-i tau H(t)) of the oracle's discrete map, per save interval, in the order they are applied: a list
    (one entry per interval) of lists of (t, tau).  KRYLOV_SE: one per interval at the right endpoint (R.krylov_map_dense);
    DP5_SE: the two CF4 exponentials per piece and sub-step, the cuts and the sub-step count of magnus_cf4_dense."""
    import math

    name = getattr(solver, "name", str(solver))
    ts = [float(t) for t in tsave]
    out = []
    for a, b in zip(ts[:-1], ts[1:]):
        if name == "KRYLOV_SE":
            out.append([(b, b - a)])
            continue
        if name != "DP5_SE":
            raise ValueError(f"no dense map for solver {name}")
        dt, n = terms.dt, terms.n_samples
        pts = [a]
        i = math.floor(a / dt) + 1
        while i <= n - 2 and i * dt < b - 1e-13:
            if i * dt > a + 1e-13:
                pts.append(i * dt)
            i += 1
        pts.append(b)
        steps = []
        for p0, p1 in zip(pts[:-1], pts[1:]):
            hf = p1 - p0
            S = max(1, math.ceil(hf / h_max - 1e-9))
            for sub in range(S):
                for theta in (1.0 / 6.0, 5.0 / 6.0):
                    steps.append((p0 + (sub + theta) / S * hf, hf / (2.0 * S)))
        out.append(steps)
    return out


def accurate_matrix_exp(m):
    """exp of a (batch of) square matrices to rounding error at every size of the argument.  torch.linalg.matrix_exp takes its
    degree-4 polynomial up to a 1-norm of 4.99e-2, where that polynomial is no longer exact to double precision: measured against
    the eigendecomposition of a Hermitian generator its error grows from 7e-14 at 1-norm 1e-2 to 1.9e-10 at 4.9e-2 and is back at
    2e-15 from 5.1e-2 on.  Arguments below 6e-2 therefore get a plain degree-14 Taylor sum (remainder < 1e-30) instead."""
    out = torch.linalg.matrix_exp(m)
    small = torch.linalg.matrix_norm(m, 1) < 6e-2
    if bool(small.any()):
        ms = m[small] if m.ndim > 2 else m
        eye = torch.eye(m.shape[-1], dtype=m.dtype).expand_as(ms)
        acc = eye.clone()
        for k in range(14, 0, -1):  # Horner: 1 + m/1 (1 + m/2 (1 + ... m/14))
            acc = eye + ms @ acc / k
        if m.ndim > 2:
            out[small] = acc
        else:
            out = acc
    return out


def _direction_terms(terms, d_amp, d_det, d_u):
    """The HamTerms whose dense H is dH of one direction (H is linear in the tables and in U); a tangent left out is zero."""
    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    u = torch.zeros_like(terms.u_pairs) if d_u is None else d_u.to(torch.float64)
    out = R.HamTerms(terms.n_qubits, u, None, None, terms.dt, terms.n_samples)
    if d_amp is not None:
        out.extra_amp = [(d_amp[k].to(torch.complex128), tg) for k, (_, tg) in enumerate(amp_terms)]
    if d_det is not None:
        out.extra_det = [(d_det[k].to(torch.float64), tg) for k, (_, tg) in enumerate(det_terms)]
    return out


def shifted_terms(terms, d_amp, d_det, d_u, s):
    """terms + sum_j s[j] * direction_j as HamTerms (tables in the order of amp_terms() / det_terms(); d_amp (n_dir, Ka, n),
    d_det (n_dir, Kd, n), d_u (n_dir, n_pairs)); differentiable in s."""
    amps = [c + sum(s[j] * d_amp[j][k] for j in range(len(s))) for k, (c, _) in enumerate(terms.amp_terms())]
    dets = [c + sum(s[j] * d_det[j][k] for j in range(len(s))) for k, (c, _) in enumerate(terms.det_terms())]
    out = R.HamTerms(terms.n_qubits, terms.u_pairs + sum(s[j] * d_u[j] for j in range(len(s))), None, None, terms.dt, terms.n_samples)
    out.extra_amp = [(c, tg) for c, (_, tg) in zip(amps, terms.amp_terms())]
    out.extra_det = [(c, tg) for c, (_, tg) in zip(dets, terms.det_terms())]
    return out


def tangent_dense_reference(terms, d_amp, d_det, d_u, psi0, d_psi0, tsave, solver, h_max=DP5_DEFAULT_H_MAX):
    """Plain dense forward mode of the oracle's discrete map, no autograd: every exponential exp(A), A = -i tau H(t), of the map
    (map_exponentials) is advanced together with its directional derivative through the block identity
        exp([[A, dA], [0, A]]) = [[e^A, L], [0, e^A]],   psi' = e^A psi,   dpsi' = e^A dpsi + L psi,
    with dA = -i tau * dense_hamiltonian(the direction's tables and U, t).
      terms   HamTerms shared by the trajectories, or a list of B HamTerms (per-trajectory tables)
      d_amp   (n_dir, Ka, n) complex | (n_dir, B, Ka, n) per trajectory | None;  d_det likewise, real;  d_u (n_dir, n_pairs) | None
      psi0    (dim, B);  d_psi0 (n_dir, dim, B) | None
    Returns the states (n_t, dim, B) and the tangent states (n_t, n_dir, dim, B), complex128 on the CPU."""
    per_traj = isinstance(terms, (list, tuple))
    psi0 = psi0.to(torch.complex128)
    dim, batch = psi0.shape
    given = [t for t in (d_amp, d_det, d_u, d_psi0) if t is not None]
    n_dir = int(given[0].shape[0])
    groups = [(terms[b], [b]) for b in range(batch)] if per_traj else [(terms, list(range(batch)))]
    n_t = len(tsave)
    states = torch.zeros(n_t, dim, batch, dtype=torch.complex128)
    tangents = torch.zeros(n_t, n_dir, dim, batch, dtype=torch.complex128)
    have_dh = d_amp is not None or d_det is not None or d_u is not None

    def table(t, d, b):  # direction d of a table tangent, for trajectory b
        if t is None:
            return None
        return t[d, b] if t.ndim == 4 else t[d]

    for g_terms, cols in groups:
        dirs = [_direction_terms(g_terms, table(d_amp, d, cols[0]), table(d_det, d, cols[0]), None if d_u is None else d_u[d])
                for d in range(n_dir)] if have_dh else []
        psi = psi0[:, cols]
        dpsi = (d_psi0[:, :, cols].to(torch.complex128) if d_psi0 is not None
                else torch.zeros(n_dir, dim, len(cols), dtype=torch.complex128))
        states[0][:, cols] = psi
        tangents[0][:, :, cols] = dpsi
        for k, steps in enumerate(map_exponentials(g_terms, tsave, solver, h_max)):
            for t, tau in steps:
                a = -1j * tau * R.dense_hamiltonian(g_terms, t)
                if have_dh:
                    blk = torch.zeros(n_dir, 2 * dim, 2 * dim, dtype=torch.complex128)
                    blk[:, :dim, :dim] = a
                    blk[:, dim:, dim:] = a
                    for d in range(n_dir):
                        blk[d, :dim, dim:] = -1j * tau * R.dense_hamiltonian(dirs[d], t)
                    e = accurate_matrix_exp(blk)
                    ea, el = e[0, :dim, :dim], e[:, :dim, dim:]
                    dpsi = ea @ dpsi + el @ psi
                else:
                    ea = accurate_matrix_exp(a)
                    dpsi = ea @ dpsi
                psi = ea @ psi
            states[k + 1][:, cols] = psi
            tangents[k + 1][:, :, cols] = dpsi
    return states, tangents


def tangent_rows_reference(states, tangents, obs_diag=None, paulis=(), overlaps=()):
    """The rows of evolve_tangent from dense states (n_t, dim, B) and tangent states (n_t, n_dir, dim, B), float64 on the CPU:
    values (rows, n_t, B) and their directional derivatives (n_dir, rows, n_t, B).  Rows: the diagonal observables
    (obs_diag (n_obs, dim)), 2 Re(psi^H O dpsi) each, then the dense PauliObservable.to_dense() ones, then Re and Im of
    <phi|dpsi> for every overlap target ((dim,) or (dim, B))."""
    val, der = [], []
    for o in ([] if obs_diag is None else obs_diag):
        o = o.to(torch.float64)
        val.append((states.abs() ** 2 * o[None, :, None]).sum(1))
        der.append(2.0 * (states.conj()[:, None] * o[None, None, :, None] * tangents).sum(2).real)
    for p in paulis:
        m = p.to_dense()
        val.append(torch.einsum("tib,ij,tjb->tb", states.conj(), m, states).real)
        der.append(2.0 * torch.einsum("tib,ij,tdjb->tdb", states.conj(), m, tangents).real)
    for phi in overlaps:
        phi = phi.to(torch.complex128)
        phi = phi[:, None] if phi.ndim == 1 else phi
        c = (phi.conj()[None] * states).sum(1)
        dc = (phi.conj()[None, None] * tangents).sum(2)
        val += [c.real, c.imag]
        der += [dc.real, dc.imag]
    n_t, n_dir, _, batch = tangents.shape
    if not val:
        return torch.zeros(0, n_t, batch, dtype=torch.float64), torch.zeros(n_dir, 0, n_t, batch, dtype=torch.float64)
    return torch.stack(val), torch.stack(der).permute(2, 0, 1, 3).contiguous()  # (rows, n_t, n_dir, B) -> (n_dir, rows, n_t, B)


def pack_terms(terms: R.HamTerms) -> dict:
    """HamTerms -> plain arrays (golden fixtures store their inputs next to the expected outputs)."""
    amp_terms, det_terms = terms.amp_terms(), terms.det_terms()
    return {"n_qubits": terms.n_qubits, "dt": terms.dt, "n_samples": terms.n_samples, "u_pairs": terms.u_pairs.detach().numpy(),
            "amp_tables": torch.stack([c.detach().to(torch.complex128) for c, _ in amp_terms]).numpy(),
            "det_tables": torch.stack([c.detach().to(torch.float64) for c, _ in det_terms]).numpy(),
            "amp_masks": np.array([mask_of(tg) for _, tg in amp_terms], dtype=np.int64),
            "det_masks": np.array([mask_of(tg) for _, tg in det_terms], dtype=np.int64)}


def unpack_terms(d) -> R.HamTerms:
    """Inverse of pack_terms (every term becomes an `extra` term with its own target list)."""
    n = int(d["n_qubits"])
    targets = lambda m: [q for q in range(n) if int(m) >> q & 1]  # noqa: E731
    t = R.HamTerms(n, torch.as_tensor(d["u_pairs"]), None, None, float(d["dt"]), int(d["n_samples"]))
    t.extra_amp = [(torch.as_tensor(c), targets(m)) for c, m in zip(d["amp_tables"], d["amp_masks"])]
    t.extra_det = [(torch.as_tensor(c), targets(m)) for c, m in zip(d["det_tables"], d["det_masks"])]
    return t


def dense_from_structured_terms(n_qubits, u_pairs, amp_terms, det_terms, amp_conditioned=(), det_ones=()):
    """The C ABI's term semantics (include/rydiff.h) as an explicit 2^N x 2^N matrix, for small N: test infrastructure.
      amp term (c, mask):  <bit_j = 1| H |bit_j = 0> = c, <0|H|1> = conj(c) for every qubit j of the mask; a CONDITIONED term acts
                           only where the sibling qubit j ^ 1 is 1;
      det term (d, mask):  2 d * (#zeros of the mask), a ONES-counting term 2 d * (0 - #ones);
      u_pairs:             U_ij on (1 - bit_i)(1 - bit_j), itertools.combinations order.  Qubit j = index bit N-1-j."""
    import itertools

    dim = 2**n_qubits
    x = torch.arange(dim)
    bit = lambda j: (x >> (n_qubits - 1 - j)) & 1  # noqa: E731
    diag = torch.zeros(dim, dtype=torch.complex128)
    for k, (i, j) in enumerate(itertools.combinations(range(n_qubits), 2)):
        diag = diag + u_pairs[k] * ((1 - bit(i)) * (1 - bit(j)))
    for k, (d, mask) in enumerate(det_terms):
        ones = bool(det_ones[k]) if det_ones else False
        for j in range(n_qubits):
            if mask >> j & 1:
                diag = diag + 2.0 * d * ((0 - bit(j)) if ones else (1 - bit(j)))
    h = torch.diag(diag)
    for k, (c, mask) in enumerate(amp_terms):
        cond = bool(amp_conditioned[k]) if amp_conditioned else False
        for j in range(n_qubits):
            if not (mask >> j & 1):
                continue
            m = 1 << (n_qubits - 1 - j)
            rows = x[(x & m) != 0]
            if cond:
                rows = rows[((rows >> (n_qubits - 1 - (j ^ 1))) & 1) == 1]
            h[rows, rows ^ m] += c
            h[rows ^ m, rows] += complex(c).conjugate() if not isinstance(c, torch.Tensor) else torch.conj(c)
    return h


# ----------------------------------------------------------------------------------------------------------------------
# Density-matrix observables (include/rydiff.h: RydProblem.dm_*): plain references on rho = v.reshape(2^n, 2^n).  Pauli strings act as
# tensor operations on the atom axes (atom j = axis j of rho.reshape((2,) * n + ...)): X flips the axis, Z signs index 1, Y flips and
# multiplies by (-i, +i) — no index masks, no dense 2^n x 2^n operator.  Every value comes with the sum of the absolute values of the
# products it adds, which is what the tolerances of tests/test_gpu_dm_observables_wide.py are stated against.
# ----------------------------------------------------------------------------------------------------------------------
_AXIS_PHASE = {(0, 0): (1.0, 1.0), (1, 0): (1.0, 1.0), (0, 1): (1.0, -1.0), (1, 1): (-1j, 1j)}  # (x bit, z bit): I, X, Z, Y by result index


def string_phase(x: int, z: int, n: int) -> np.ndarray:
    """The phases of one string as a (2,) * n tensor over the RESULT index: the product over the atoms of (1, 1) for I and X,
    (1, -1) for Z, (-i, i) for Y = [[0, -i], [i, 0]]  (masks: bit j = atom j, as PauliObservable.terms gives them)."""
    ph = np.ones((2,) * n, dtype=np.complex128)
    for j in range(n):
        vec = np.asarray(_AXIS_PHASE[(x >> j & 1, z >> j & 1)], dtype=np.complex128)
        ph = ph * vec.reshape((1,) * j + (2,) + (1,) * (n - 1 - j))
    return ph


def pauli_string_apply(t, x: int, z: int, n: int):
    """P t for a numpy array or torch tensor t of shape (2,) * n + rest: the string acts on the first n axes."""
    axes = [j for j in range(n) if x >> j & 1]
    ph = string_phase(x, z, n)
    ph = ph.reshape(ph.shape + (1,) * (t.ndim - n))
    if isinstance(t, torch.Tensor):
        return (torch.flip(t, axes) if axes else t) * torch.from_numpy(ph).to(t.device)
    return (np.flip(t, axes) if axes else t) * ph


def dm_pauli_row(rho: np.ndarray, terms, n: int) -> tuple[float, float]:
    """(sum_s w_s Re Tr(P_s rho), sum_s |w_s| sum_x |rho[x ^ flips, x]|) for terms = [(w, x_mask, z_mask), ...].  The flip is a view
    of rho.reshape((2,) * 2n) and the diagonal an einsum over that view, so a 4096 x 4096 matrix is never copied per string."""
    t = rho.reshape((2,) * (2 * n))
    idx = list(range(n))
    val = tot = 0.0
    for w, x, z in terms:
        axes = [j for j in range(n) if x >> j & 1]
        d = np.einsum(np.flip(t, axes) if axes else t, idx + idx, idx)  # d[x] = rho[x with the X / Y atoms flipped][x]
        val += w * float((string_phase(x, z, n) * d).sum().real)
        tot += abs(w) * float(np.abs(d).sum())
    return val, tot


def dm_pauli_row_torch(rho: torch.Tensor, terms, n: int) -> torch.Tensor:
    """sum_s w_s Re Tr(P_s rho) in differentiable torch: P_s applied to rho.reshape((2,) * n + (2^n,)), then the trace."""
    dim = 2 ** n
    out = torch.zeros((), dtype=torch.float64, device=rho.device)
    for w, x, z in terms:
        out = out + w * pauli_string_apply(rho.reshape((2,) * n + (dim,)), x, z, n).reshape(dim, dim).diagonal().sum().real
    return out


def dm_rows_reference(v: np.ndarray, n: int, diag=(), paulis=(), targets=(), purity: bool = False):
    """Every density-matrix row of one vector v = vec(rho) (4^n,), in the order of expect_out (diagonal tables, Pauli observables,
    fidelities, purity): (values, sums of absolute terms), float64 arrays.  diag: (n_diag, 2^n) real; targets: (n_fid, 2^n) complex."""
    dim = 2 ** n
    rho = v.reshape(dim, dim)
    val, tot = [], []
    re_diag = np.diagonal(rho).real
    for o in diag:
        val.append(float((o * re_diag).sum()))
        tot.append(float(np.abs(o * re_diag).sum()))
    for p in paulis:
        a, b = dm_pauli_row(rho, p.terms, n)
        val.append(a)
        tot.append(b)
    if len(targets):
        arho = np.abs(rho)
        for phi in targets:
            val.append(float((phi.conj() @ (rho @ phi)).real))
            tot.append(float(np.abs(phi) @ (arho @ np.abs(phi))))
    if purity:
        s = float((np.abs(v) ** 2).sum())
        val.append(s)
        tot.append(s)
    return np.asarray(val), np.asarray(tot)


def dm_cotangent_reference(v: np.ndarray, n: int, g, diag=(), paulis=(), targets=(), purity: bool = False):
    """The cotangent rydiff.h writes down for the density-matrix rows of one vector v (4^n,), row weights g in the order of
    dm_rows_reference:  g o[x] on the diagonal;  g w_s conj(phase_s(x)) at the entries Re Tr(P_s rho) reads (torch.autograd through
    dm_pauli_row_torch);  g phi[x] conj(phi[y]);  2 g v.  Returns (cotangent (4^n,) complex, sum of the absolute contributions per
    entry (4^n,) real)."""
    dim = 2 ** n
    rho = v.reshape(dim, dim)
    cot = np.zeros((dim, dim), dtype=np.complex128)
    tot = np.zeros((dim, dim), dtype=np.float64)
    g = [float(x) for x in g]
    r = 0
    at = np.arange(dim)
    for o in diag:
        cot[at, at] += g[r] * o
        tot[at, at] += np.abs(g[r] * o)
        r += 1
    if len(paulis):
        leaf = torch.from_numpy(rho.copy()).requires_grad_(True)
        leaf_abs = torch.from_numpy(rho.copy()).requires_grad_(True)
        loss = loss_abs = 0.0
        for p in paulis:
            loss = loss + g[r] * dm_pauli_row_torch(leaf, p.terms, n)
            loss_abs = loss_abs + dm_pauli_row_torch(leaf_abs, [(abs(g[r] * w), x, 0) for w, x, _ in p.terms], n)  # moduli: X for Y, no Z
            r += 1
        loss.backward()
        loss_abs.backward()
        cot += leaf.grad.numpy()
        tot += leaf_abs.grad.numpy().real
    for phi in targets:
        cot += g[r] * np.outer(phi, phi.conj())
        tot += abs(g[r]) * np.outer(np.abs(phi), np.abs(phi))
        r += 1
    if purity:
        cot += 2.0 * g[r] * rho
        tot += 2.0 * abs(g[r]) * np.abs(rho)
        r += 1
    assert r == len(g)
    return cot.reshape(-1), tot.reshape(-1)


def ket_pauli_cotangent(v: np.ndarray, n_qubits: int, terms, g: float):
    """2 g O v for a ket-style Pauli observable O = sum_s w_s P_s on the whole register (here: the doubled one), and the sum of the
    absolute contributions per entry."""
    t = v.reshape((2,) * n_qubits)
    cot = np.zeros(t.shape, dtype=np.complex128)
    tot = np.zeros(t.shape, dtype=np.float64)
    for w, x, z in terms:
        cot += 2.0 * g * w * pauli_string_apply(t, x, z, n_qubits)
        tot += 2.0 * abs(g * w) * np.abs(pauli_string_apply(t, x, 0, n_qubits))
    return cot.reshape(-1), tot.reshape(-1)


def ket_pauli_row(t: np.ndarray, n_qubits: int, terms):
    """(<v|O|v>.real, sum of the absolute products) for a ket-style Pauli observable on the whole register; t: the vector(s) with the
    qubit axes first, shape (2,) * n_qubits + rest — the results have shape rest."""
    axes = tuple(range(n_qubits))
    val = tot = 0.0
    for w, x, z in terms:
        val = val + w * (t.conj() * pauli_string_apply(t, x, z, n_qubits)).sum(axis=axes).real
        tot = tot + abs(w) * (np.abs(t) * np.abs(pauli_string_apply(t, x, 0, n_qubits))).sum(axis=axes)
    return val, tot


# ---- shots from the diagonal of rho: the shaped inputs of the wide cases and a second float64 prefix sum ------------------------------
DM_SHOTS = 4096
DM_SHOT_THREADS = 256  # k_dm_shots: one contiguous segment of ceil(2^n / 256) entries per thread


def dm_shot_inputs(n: int, batch: int, seed: int):
    """(v0 (B, 4^n) complex, uniforms (2, B, DM_SHOTS)) for the shot cases past one segment per thread.  The diagonal of v0 has a random
    sign (about half is clamped); the first two and the last three whole thread segments and four consecutive segments in the middle
    are zero or negative; every third remaining entry is an exact zero; the uniforms hold 0 and 1 - 2^-53."""
    dim = 2 ** n
    seg = (dim + DM_SHOT_THREADS - 1) // DM_SHOT_THREADS
    n_seg = dim // seg
    gen = torch.Generator().manual_seed(seed)
    v0 = torch.randn(batch, dim * dim, generator=gen, dtype=torch.complex128)
    d = torch.randn(batch, dim, generator=gen, dtype=torch.float64)
    x = torch.arange(dim)
    segment = x // seg
    mid = n_seg // 2
    dead = (segment < 2) | (segment >= n_seg - 3) | ((segment >= mid) & (segment < mid + 4))
    d[:, dead] = -d[:, dead].abs()          # negative ...
    d[:, dead & (x % 2 == 0)] = 0.0         # ... or exactly zero
    live = torch.nonzero(~dead).squeeze(1)
    d[:, live[::3]] = 0.0
    v0[:, x * (dim + 1)] = torch.complex(d, torch.ones_like(d))  # (the imaginary part plays no part)
    uniforms = torch.rand(2, batch, DM_SHOTS, generator=gen, dtype=torch.float64)
    uniforms[:, :, 0] = 0.0
    uniforms[:, :, 1] = 1.0 - 2.0 ** -53
    return v0, uniforms


def segmented_prefix(p: np.ndarray, threads: int = DM_SHOT_THREADS) -> np.ndarray:
    """A float64 prefix sum of p (dim,) in another order than numpy.cumsum's: running sums inside `threads` contiguous segments, a
    serial scan of the segment totals, then offset + running sum."""
    dim = len(p)
    seg = (dim + threads - 1) // threads
    out = np.empty(dim, dtype=np.float64)
    acc = 0.0
    for lo in range(0, dim, seg):
        local = np.cumsum(p[lo:lo + seg])
        out[lo:lo + seg] = acc + local
        acc = acc + float(local[-1])
    return out


def sample_with_prefix(p: np.ndarray, cum: np.ndarray, u: np.ndarray) -> np.ndarray:
    """The shot rule on a given float64 prefix sum: the smallest x with cum[x] > u * cum[-1], u clamped into [0, 1); where there is
    none, the last x with p[x] > 0."""
    uc = np.where(u > 0, np.minimum(u, 1.0 - 2.0 ** -53), 0.0)
    pos = np.searchsorted(cum, uc * cum[-1], side="right")
    return np.where(pos < len(p), pos, np.flatnonzero(p > 0)[-1])


def shot_band(p: np.ndarray, u: np.ndarray) -> np.ndarray:
    """True for the shots left out of an equality check between two float64 prefix sums: |u S - C[x]| <= 4 D 2^-53 S for some x, C =
    numpy.cumsum(p).  Either prefix sum is within (D - 1) 2^-53 S of the exact one; the band doubles their largest disagreement."""
    cum = np.cumsum(p)
    s, dim = cum[-1], len(p)
    tau = np.where(u > 0, np.minimum(u, 1.0 - 2.0 ** -53), 0.0) * s
    hi = np.minimum(np.searchsorted(cum, tau, side="left"), dim - 1)
    lo = np.maximum(hi - 1, 0)
    return np.minimum(np.abs(tau - cum[hi]), np.abs(tau - cum[lo])) <= 4.0 * dim * 2.0 ** -53 * s


# ---- per-atom addressing: one single-qubit amplitude term and one single-qubit detuning term per atom --------------------------------
def per_atom_terms(n, n_samples, dt, seed, phase=True, undriven=(), undetuned=(), global_drive=False) -> R.HamTerms:
    """What the stochastic-noise runs, SLM masks and local channels hand over: amp_coeff = det_coeff = None, one extra_amp entry ([q])
    per driven atom and one extra_det entry ([q]) per detuned atom, on a jittered chain.  With t = linspace(0, 1, n_samples):
        amplitude of atom q  0.5 * 6 * (s_q sin^2(pi t) + 0.2 cos((q + 1) t)) * exp(-i (0.7 t + phi_q)),  s_q in [1, 1.3], phi_q in [0, 1)
                             (phase=False: no phase factor at all, a real profile stored as complex)
        detuning of atom q   -2.5 (2 t - 1) + 0.7 xi_q + 0.3 sin((q + 2) t),  xi_q standard normal
    No two rows are proportional (every atom has its own frequency), so swapping two groups changes values and gradients.
    global_drive=True: ONE amplitude term (the profile of "atom 0") on all atoms next to the per-atom detunings — the doppler / SLM
    shape.  The seeded draws do not depend on undriven / undetuned / global_drive."""
    g = torch.Generator().manual_seed(seed)
    coords = torch.stack([torch.arange(n, dtype=torch.float64) * 8.0, torch.rand(n, generator=g, dtype=torch.float64) * 2.0], dim=1)
    s = 1.0 + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)
    phi = torch.rand(n, generator=g, dtype=torch.float64)
    xi = torch.randn(n, generator=g, dtype=torch.float64)
    t = torch.linspace(0, 1, n_samples, dtype=torch.float64)

    def amp_row(q):
        a = 0.5 * 6.0 * (s[q] * torch.sin(np.pi * t) ** 2 + 0.2 * torch.cos((q + 1) * t))
        return (a * torch.exp(-1j * (0.7 * t + phi[q]).to(torch.complex128))) if phase else a.to(torch.complex128)

    terms = R.HamTerms(n, R.interaction_strengths(coords), None, None, dt, n_samples)
    if global_drive:
        terms.extra_amp = [(amp_row(0), list(range(n)))]
    else:
        terms.extra_amp = [(amp_row(q), [q]) for q in range(n) if q not in undriven]
    terms.extra_det = [(-2.5 * (2 * t - 1) + 0.7 * xi[q] + 0.3 * torch.sin((q + 2) * t), [q]) for q in range(n) if q not in undetuned]
    return terms


def per_atom_terms_batch(n, n_samples, dt, seeds, **kw) -> list:
    """Per-trajectory tables: one per_atom_terms per seed, all on the register (u_pairs) of the first."""
    sets = [per_atom_terms(n, n_samples, dt, seed, **kw) for seed in seeds]
    for tr in sets[1:]:
        tr.u_pairs = sets[0].u_pairs
    return sets


def stack_tables(sets, device="cpu", real_amp: bool = False):
    """A list of B HamTerms with the same term structure -> (amp [B, Ka, n], det [B, Kd, n]) for evolve (to_native only repeats one
    table set).  real_amp: the amplitude tables as a REAL tensor (they must be phase-free)."""
    masks = [[tuple(tg) for _, tg in tr.amp_terms()] + [None] + [tuple(tg) for _, tg in tr.det_terms()] for tr in sets]
    assert all(m == masks[0] for m in masks), "the table sets must share one term structure"
    amp = torch.stack([torch.stack([c.detach().to(torch.complex128) for c, _ in tr.amp_terms()]) for tr in sets])
    det = torch.stack([torch.stack([c.detach().to(torch.float64) for c, _ in tr.det_terms()]) for tr in sets])
    if real_amp:
        assert float(amp.imag.abs().max()) == 0.0
        amp = amp.real.contiguous()
    return amp.to(device), det.to(device)


def product_state(n, gen) -> torch.Tensor:
    """The Kronecker product of n random normalised single-qubit states, (2^n,) complex128 (qubit 0 = the most significant index bit).
    A Haar-random register state makes every gradient tiny; a product state keeps them at their natural size.  The single-qubit states
    are (cos(th/2), e^{i phi} sin(th/2)) with cos(th) uniform in [-0.8, 0.8] and phi uniform: both populations at least 0.1.  The
    detuning of atom q acts through its occupation n_q and its drive through <X_q>, <Y_q>, so an atom that starts at a pole of its
    Bloch sphere has a gradient row close to zero — with twenty atoms or sixteen trajectories there would always be one."""
    psi = torch.ones(1, dtype=torch.complex128)
    for _ in range(n):
        r = torch.rand(2, generator=gen, dtype=torch.float64)
        p1 = 0.5 * (1.0 - 0.8 * (2.0 * float(r[0]) - 1.0))
        v = torch.tensor([np.sqrt(1.0 - p1), np.sqrt(p1) * np.exp(2j * np.pi * float(r[1]))], dtype=torch.complex128)
        psi = torch.kron(psi, v)
    return psi


ROW_FLOOR = 1e-2  # assert_rows_close: a row is measured against max(its own largest entry, ROW_FLOOR * the tensor's largest entry)


def row_errors(got, ref):
    """Per row r of a [..., K, n_samples] tensor (rows = everything but the last axis): max|got_r - ref_r| / max(max|ref_r|,
    ROW_FLOOR * max|ref|), and max|ref_r| / max|ref|.  float64 numpy arrays of shape [..., K]."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref).max(axis=-1)
    top = float(scale.max())
    err = np.abs(got - ref).max(axis=-1) / np.maximum(np.maximum(scale, ROW_FLOOR * top), 1e-300)
    return err, scale / max(top, 1e-300)


def assert_rows_close(got, ref, rtol, name="") -> float:
    """Every row of a gradient [..., K, n_samples] on its own:  max|got_r - ref_r| <= rtol * max(max|ref_r|, 1e-2 * max|ref|).  So that
    the floor never hides a row, first asserts — on the reference alone — that every row reaches 1e-2 of the largest.  Returns the
    worst per-row error (for the measurement tables)."""
    err, ratio = row_errors(got, ref)
    assert np.isfinite(np.asarray(got)).all(), f"{name}: non-finite entries"
    assert float(ratio.min()) >= ROW_FLOOR, f"{name}: reference row {np.unravel_index(ratio.argmin(), ratio.shape)} is {ratio.min():.2e} of the largest row"
    worst = float(err.max())
    assert worst <= rtol, f"{name}: row {np.unravel_index(err.argmax(), err.shape)} off by {worst:.3e} of its scale (bar {rtol:.0e})"
    return worst


PER_ATOM_TSAVE = (0.0, 0.0041, 0.0102, 0.0163, 0.024)  # four unequal save intervals, off the sample grid


def per_atom_loss(states, expect, w, cot):
    """The loss of the per-atom parity cases, torch on either side: states (n_t, B, dim), expect (n_obs >= 2, n_t, B), w (n_t,), cot
    (n_t, B, dim).  Every save point is weighted through <O_0>, one through <O_1>, and the states themselves through cot."""
    return (w[:, None] * expect[0]).sum() - 0.4 * expect[1, expect.shape[1] // 2].sum() + (cot.conj() * states).real.sum()


def per_atom_problem(n, batch, seed, n_t=len(PER_ATOM_TSAVE), device="cpu"):
    """The seeded non-table inputs of a per-atom case on the CPU: psi0 (B, dim) product states, two random diagonal observables (2, dim),
    the weights linspace(0.5, 1.5, n_t) and state cotangents (n_t, B, dim) at every save point after the first:
        cot_k = c_k psi0 + sum_q (e_kq Z_q + f_kq X_q) psi0 / sqrt(2 n) + a random part of norm 0.3,   c, e, f seeded complex normals.
    Z_q psi0 and X_q psi0 are the directions in which a change of atom q's detuning / drive moves the state at first order.  With psi0
    alone (a random vector would weigh 2^(-n/2)) the gradient row of atom q scales with <Z_q> or <X_q>, <Y_q> of its random single-qubit
    state, and among many atoms one of those is always close to zero; with its own weight at every save point each row keeps a part
    of the common size, whatever the atom's state.  device: where the tensors are formed and returned (the seeded draws are the
    CPU generator's either way; the large registers form their cotangents on the GPU)."""
    gen = torch.Generator().manual_seed(seed)
    dim = 2**n
    psi0 = torch.stack([product_state(n, gen) for _ in range(batch)]).to(device)
    obs = torch.rand(2, dim, generator=gen, dtype=torch.float64).to(device)
    w = torch.linspace(0.5, 1.5, n_t, dtype=torch.float64).to(device)
    c = torch.randn(n_t, generator=gen, dtype=torch.complex128).to(device)
    ef = (torch.randn(2, n_t, n, generator=gen, dtype=torch.complex128) / np.sqrt(2.0 * n)).to(device)
    cot = c[:, None, None] * psi0[None] + (0.3 * torch.randn(n_t, batch, dim, generator=gen, dtype=torch.complex128) / np.sqrt(dim)).to(device)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device=device)
    for q in range(n):
        v = psi0.reshape(batch, 2**q, 2, 2 ** (n - 1 - q))  # axis 2: the bit of atom q (qubit 0 = the most significant index bit)
        zq = (v * sign[None, None, :, None]).reshape(batch, dim)
        xq = torch.flip(v, dims=(2,)).reshape(batch, dim)
        cot += ef[0, :, q, None, None] * zq[None] + ef[1, :, q, None, None] * xq[None]
    cot[0] = 0.0
    return psi0, obs, w, cot


def oracle_value_and_grads(terms, psi0, tsave, obs, w, cot, method="matrix_free"):
    """States, <O>(t_k), the loss per_atom_loss and its five gradients from torch autograd through one of the CPU references:
    "matrix_free" (R.krylov_map_matrix_free_torch), "dense" (R.krylov_map_dense) or "magnus" (magnus_cf4_dense at the native default
    sub-step, the model of DP5_SE).  terms: one HamTerms shared by the B trajectories, or a list of B (per-trajectory tables on one
    register: run one by one; the U and tsave gradients are summed).  psi0 (B, dim), cot (n_t, B, dim).  Returns numpy arrays: states
    (n_t, B, dim), expect (n_obs, n_t, B), amp ([B,] Ka, n) complex, det ([B,] Kd, n), u, tsave, psi0 (B, dim)."""
    if isinstance(terms, (list, tuple)):
        parts = [oracle_value_and_grads(tr, psi0[b:b + 1], tsave, obs, w, cot[:, b:b + 1], method) for b, tr in enumerate(terms)]
        out = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ("states", "expect")}
        out["expect"] = np.concatenate([p["expect"] for p in parts], axis=2)
        out.update({k: np.stack([p[k] for p in parts]) for k in ("amp", "det")})
        out.update({k: sum(p[k] for p in parts) for k in ("u", "tsave", "loss")})
        out["psi0"] = np.concatenate([p["psi0"] for p in parts], axis=0)
        return out
    o = R.HamTerms(terms.n_qubits, terms.u_pairs.clone().requires_grad_(True), None, None, terms.dt, terms.n_samples)
    o.extra_amp = [(c.clone().requires_grad_(True), tg) for c, tg in terms.amp_terms()]
    o.extra_det = [(c.clone().requires_grad_(True), tg) for c, tg in terms.det_terms()]
    ts = torch.as_tensor(tsave, dtype=torch.float64).clone().requires_grad_(True)
    p0 = psi0.T.contiguous().clone().requires_grad_(True)  # (dim, B)
    if method == "matrix_free":
        st = R.krylov_map_matrix_free_torch(o, p0, ts)
    elif method == "dense":
        st = R.krylov_map_dense(o, p0, ts)
    elif method == "magnus":
        st = magnus_cf4_dense(o, p0, ts, h_max=DP5_DEFAULT_H_MAX)
    else:
        raise ValueError(method)
    st = st.permute(0, 2, 1)  # (n_t, B, dim)
    expect = torch.stack([(st.abs() ** 2 * d[None, None, :]).sum(2) for d in obs])
    loss = per_atom_loss(st, expect, w, cot)
    loss.backward()
    return {"states": st.detach().numpy(), "expect": expect.detach().numpy(), "loss": float(loss),
            "amp": torch.stack([c.grad for c, _ in o.extra_amp]).numpy(), "det": torch.stack([c.grad for c, _ in o.extra_det]).numpy(),
            "u": o.u_pairs.grad.numpy(), "tsave": ts.grad.numpy(), "psi0": p0.grad.T.contiguous().numpy()}
