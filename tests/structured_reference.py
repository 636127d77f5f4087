"""Two exact references for the C ABI's term semantics (include/rydiff.h) that need no 2^N x 2^N matrix: test infrastructure, plain
torch, CPU or device.

  amp term (c, mask)   <bit_j = 1| H |bit_j = 0> = c, <0|H|1> = conj(c) for every qubit j of the mask; a CONDITIONED term
                       (amp_conditioned) acts only where the sibling qubit j ^ 1 is 1
  det term (d, mask)   2 d * (#zeros of the mask); a ONES-counting term (det_ones) 2 d * (0 - #ones)
  u_pairs              U_ij on (1 - bit_i)(1 - bit_j), itertools.combinations order
  tables at time t     c(t) = c[i1] + (c[i2] - c[i1]) (t - i1 dt) / dt,  i1 = max(min(floor(t / dt), n - 2), 0),  i2 = min(i1 + 1, n - 2)
Qubit j is index bit N-1-j; bit j of a mask is qubit j.  Plain registers are the unflagged case.

(a) MATRIX-FREE: structured_matvec applies H(t) through psi.view(B, 2^j, 2, 2^(N-1-j)).flip(2); krylov_map is the KRYLOV_SE map
    psi_{k+1} = exp(-i (t_{k+1} - t_k) H(t_{k+1})) psi_k with the exponential as a Taylor sum run until a term falls below 1e-19 of
    the state; torch autograd differentiates it in the tables, u, tsave and psi0.  rhs / continuous_solution: -i H(t) psi and its
    DOP853 solution, the target of DP5_SE.
(b) CLUSTER-SEPARABLE: the register cut into clusters of consecutive qubits (at most 6 each; an even first qubit where terms are
    conditioned, so that siblings stay together), every mask restricted to each cluster, u_pairs non-zero only inside a cluster.
    Then H = sum_c H_c (x) 1 exactly, a product state stays a product state, and each factor is evolved with the explicit matrix of
    its cluster (tests/helpers.py: dense_from_structured_terms, accurate_matrix_exp) — exact at ANY register size.

`wrong=(kind, term)` turns ONE term into a deliberately wrong semantics ("sibling0": the condition taken on sibling value 0;
"ones_sign": the sign of a ones-counting term flipped; "swap_conj": c and conj(c) swapped).  Only the sensitivity tests
(tests/test_structured_reference_host.py) use it: they show that each of these mistakes moves what the GPU cases compare."""
from __future__ import annotations

import itertools
import math
import time
from dataclasses import dataclass, replace

import numpy as np
import torch

from tests.helpers import accurate_matrix_exp, dense_from_structured_terms

MAX_CLUSTER_QUBITS = 6


@dataclass(frozen=True)
class Structure:
    """The non-tensor part of a structured problem (ProblemSpec's n_qubits, dt, n_samples, masks and per-term flags)."""

    n_qubits: int
    dt: float
    n_samples: int
    amp_masks: tuple
    det_masks: tuple
    amp_conditioned: tuple = ()
    det_ones: tuple = ()

    def conditioned(self, k: int) -> bool:
        return bool(self.amp_conditioned[k]) if self.amp_conditioned else False

    def ones(self, k: int) -> bool:
        return bool(self.det_ones[k]) if self.det_ones else False


def interp_indices(t: float, dt: float, n_samples: int):
    i1 = max(int(min(math.floor(t / dt), n_samples - 2)), 0)
    return i1, min(i1 + 1, n_samples - 2)


def interp_table(tab, t, dt: float, n_samples: int):
    """tab[..., n_samples] at time t (a float or a 0-d tensor: differentiable in t and in the table)."""
    i1, i2 = interp_indices(float(t.detach()) if isinstance(t, torch.Tensor) else float(t), dt, n_samples)
    return tab[..., i1] + (tab[..., i2] - tab[..., i1]) * (t - i1 * dt) / dt


# ----------------------------------------------------------------------------------------------------------------------
# (a) matrix-free
# ----------------------------------------------------------------------------------------------------------------------
def _flip(psi, n: int, j: int):
    """psi[..., x ^ m_j] for qubit j (index bit n-1-j), psi of shape (B, 2^n)."""
    return psi.reshape(psi.shape[0], 2**j, 2, 2 ** (n - 1 - j)).flip(2).reshape(psi.shape)


class _WeightedFlips(torch.autograd.Function):
    """t1[x] = sum_j w1_j[x] psi[x ^ m_j],  t0[x] = sum_j w0_j[x] psi[x ^ m_j] over the qubits of one term, w real and constant: real-
    linear maps, so nothing is kept for the backward pass (the transpose of a flip is the flip: grad = sum_j flip_j(w1_j g1 + w0_j g0))."""

    @staticmethod
    def forward(ctx, psi, n, qubits, w1, w0):
        ctx.meta = (n, qubits, w1, w0)
        t1, t0 = torch.zeros_like(psi), torch.zeros_like(psi)
        for j, a, b in zip(qubits, w1, w0):
            fl = _flip(psi, n, j)
            t1 += a * fl
            t0 += b * fl
        return t1, t0

    @staticmethod
    def backward(ctx, g1, g0):
        n, qubits, w1, w0 = ctx.meta
        out = torch.zeros_like(g1)
        for j, a, b in zip(qubits, w1, w0):
            out += _flip((a * g1 + b * g0).contiguous(), n, j)
        return out, None, None, None, None


class Operator:
    """The constant index structure of one Structure on one device: per amp term the weights of <1|.|0> and <0|.|1> per qubit, per
    det term the counted occupation, the pair table of u_pairs."""

    def __init__(self, st: Structure, device="cpu", wrong=None):
        n = st.n_qubits
        self.st, self.device = st, torch.device(device)
        x = torch.arange(2**n, device=self.device)
        bit = lambda j: ((x >> (n - 1 - j)) & 1).to(torch.float64)  # noqa: E731
        kind, which = wrong if wrong is not None else (None, -1)
        assert kind in (None, "sibling0", "ones_sign", "swap_conj"), kind
        self.amp = []
        for k, mask in enumerate(st.amp_masks):
            qubits = tuple(j for j in range(n) if mask >> j & 1)
            w1, w0 = [], []
            for j in qubits:
                cond = torch.ones(2**n, dtype=torch.float64, device=self.device)
                if st.conditioned(k):
                    cond = (1.0 - bit(j ^ 1)) if (kind == "sibling0" and which == k) else bit(j ^ 1)
                a, b = bit(j) * cond, (1.0 - bit(j)) * cond
                if kind == "swap_conj" and which == k:
                    a, b = b, a
                w1.append(a)
                w0.append(b)
            self.amp.append((qubits, tuple(w1), tuple(w0)))
        if kind in ("sibling0", "swap_conj"):
            assert 0 <= which < len(st.amp_masks) and (kind == "swap_conj" or st.conditioned(which))
        counts = []
        for k, mask in enumerate(st.det_masks):
            c = torch.zeros(2**n, dtype=torch.float64, device=self.device)
            for j in range(n):
                if mask >> j & 1:
                    c = c + ((0.0 - bit(j)) if st.ones(k) else (1.0 - bit(j)))
            if kind == "ones_sign" and which == k:
                assert st.ones(k)
                c = -c
            counts.append(c)
        self.det_counts = torch.stack(counts) if counts else torch.zeros(0, 2**n, dtype=torch.float64, device=self.device)
        pairs = [(1.0 - bit(i)) * (1.0 - bit(j)) for i, j in itertools.combinations(range(n), 2)]
        self.pair_table = torch.stack(pairs) if pairs else torch.zeros(0, 2**n, dtype=torch.float64, device=self.device)

    def diagonal(self, det_t, u):
        """The diagonal of H for interpolated detunings det_t (Kd,) and u (n_pairs,): (2^N,) real, differentiable in both."""
        return u.to(torch.float64) @ self.pair_table + 2.0 * (det_t.to(torch.float64) @ self.det_counts)

    def apply(self, amp_t, diag, psi):
        """H psi for interpolated amplitudes amp_t (Ka,) complex and a diagonal (2^N,); psi (B, 2^N) complex128."""
        out = diag * psi
        for k, (qubits, w1, w0) in enumerate(self.amp):
            if not qubits:
                continue
            t1, t0 = _WeightedFlips.apply(psi, self.st.n_qubits, qubits, w1, w0)
            out = out + amp_t[k] * t1 + torch.conj(amp_t[k]) * t0
        return out


def structured_matvec(st: Structure, amp_t, det_t, u, psi, wrong=None, op: Operator | None = None):
    """H psi from the term list, no matrix: amp_t (Ka,) complex and det_t (Kd,) are the coefficients already interpolated, u
    (n_pairs,), psi (B, 2^N)."""
    op = op if op is not None else Operator(st, psi.device, wrong)
    return op.apply(amp_t.to(torch.complex128), op.diagonal(det_t, u), psi)


TAYLOR_TOL = 1e-19  # a Taylor term below this fraction of the state ends the sum (asked: converged below 1e-18 of the state)


def krylov_map(st: Structure, amp, det, u, tsave, psi0, wrong=None, tol: float = TAYLOR_TOL, counts: list | None = None):
    """The KRYLOV_SE map psi_{k+1} = exp(-i (t_{k+1} - t_k) H(t_{k+1})) psi_k: states (n_t, B, 2^N), differentiable in everything.
    amp (Ka, n) complex / det (Kd, n) shared by the trajectories, or (B, Ka, n) / (B, Kd, n) per trajectory (then run one trajectory
    at a time); psi0 (B, 2^N).  counts: receives the Taylor terms taken per interval."""
    if amp.ndim == 3:
        assert amp.shape[0] == det.shape[0] == psi0.shape[0]
        return torch.cat([krylov_map(st, amp[b], det[b], u, tsave, psi0[b:b + 1], wrong, tol, counts) for b in range(psi0.shape[0])], dim=1)
    op = Operator(st, psi0.device, wrong)
    psi = psi0.to(torch.complex128)
    out = [psi]
    for k in range(len(tsave) - 1):
        t = tsave[k + 1]
        amp_t = interp_table(amp, t, st.dt, st.n_samples).to(torch.complex128)
        diag = op.diagonal(interp_table(det, t, st.dt, st.n_samples), u)
        tau = tsave[k + 1] - tsave[k]
        term = acc = psi
        ref = float(torch.linalg.vector_norm(psi.detach()))
        for m in range(1, 400):
            term = op.apply(amp_t, diag, term) * (-1j * tau / m)
            acc = acc + term
            if float(torch.linalg.vector_norm(term.detach())) < tol * ref:
                break
        else:
            raise RuntimeError("the Taylor sum of the exponential did not converge")
        if counts is not None:
            counts.append(m)
        psi = acc
        out.append(psi)
    return torch.stack(out)


def rhs(st: Structure, amp, det, u, t, psi, op: Operator | None = None):
    """-i H(t) psi with the tables (shared by the trajectories) interpolated at t; psi (B, 2^N)."""
    op = op if op is not None else Operator(st, psi.device)
    amp_t = interp_table(amp, t, st.dt, st.n_samples).to(torch.complex128)
    return -1j * op.apply(amp_t, op.diagonal(interp_table(det, t, st.dt, st.n_samples), u), psi)


def continuous_solution(st: Structure, amp, det, u, tsave, psi0, rtol: float = 1e-12, atol: float = 1e-14) -> np.ndarray:
    """The continuous-time solution of d psi / dt = -i H(t) psi at the save times (scipy DOP853, in the style of
    oracle/restatement.py: continuous_solution): numpy (n_t, B, 2^N).  Shared tables; nothing is differentiated.
    H(t) is piecewise linear with a KINK at every sample point, and an adaptive step that straddles a kink can pass its error test
    with a wrong result (seen with these random tables: 3.6e-10 at the last save time on one machine, 6e-13 on another, same versions,
    rtol 1e-12 both).  So the integrator is restarted at every sample point and every save time: each step lies inside one linear
    piece, and the save points are step ends, not dense output."""
    from scipy.integrate import solve_ivp

    op = Operator(st, "cpu")
    amp, det, u = amp.detach().cpu(), det.detach().cpu(), u.detach().cpu()
    shape = tuple(psi0.shape)

    def f(t, y):
        with torch.no_grad():
            return rhs(st, amp, det, u, float(t), torch.from_numpy(y.reshape(shape)), op).numpy().reshape(-1)

    ts = [float(t) for t in tsave.detach().cpu()]
    y = psi0.detach().cpu().to(torch.complex128).numpy().reshape(-1)
    out = [y]
    for a, b in zip(ts[:-1], ts[1:]):
        cuts = [a] + [i * st.dt for i in range(1, st.n_samples - 1) if a + 1e-13 < i * st.dt < b - 1e-13] + [b]
        for p0, p1 in zip(cuts[:-1], cuts[1:]):
            sol = solve_ivp(f, (p0, p1), y, method="DOP853", rtol=rtol, atol=atol)
            assert sol.status == 0, sol.message
            y = sol.y[:, -1]
        out.append(y)
    return np.stack(out).reshape((len(ts),) + shape)


def dense_krylov_map(st: Structure, amp, det, u, tsave, psi0):
    """The same map through the explicit matrix (dense_from_structured_terms) and accurate_matrix_exp, for small N: states
    (n_t, B, 2^N), differentiable.  Shared or per-trajectory tables as krylov_map."""
    if amp.ndim == 3:
        return torch.cat([dense_krylov_map(st, amp[b], det[b], u, tsave, psi0[b:b + 1]) for b in range(psi0.shape[0])], dim=1)
    psi = psi0.to(torch.complex128).T
    out = [psi]
    for k in range(len(tsave) - 1):
        t = tsave[k + 1]
        a, d = interp_table(amp, t, st.dt, st.n_samples), interp_table(det, t, st.dt, st.n_samples)
        h = dense_from_structured_terms(st.n_qubits, u, [(a[i], m) for i, m in enumerate(st.amp_masks)],
                                        [(d[i], m) for i, m in enumerate(st.det_masks)], st.amp_conditioned, st.det_ones)
        psi = accurate_matrix_exp(-1j * h * (tsave[k + 1] - tsave[k])) @ psi
        out.append(psi)
    return torch.stack(out).permute(0, 2, 1)


# ----------------------------------------------------------------------------------------------------------------------
# (b) cluster-separable
# ----------------------------------------------------------------------------------------------------------------------
def cluster_bounds(sizes):
    """Cluster sizes -> [(first qubit, size), ...] of consecutive qubits."""
    out, q = [], 0
    for m in sizes:
        assert 1 <= m <= MAX_CLUSTER_QUBITS
        out.append((q, m))
        q += m
    return out


def pair_index(n: int) -> dict:
    return {p: k for k, p in enumerate(itertools.combinations(range(n), 2))}


def intra_cluster_pairs(n: int, sizes) -> list:
    """Positions in u_pairs of the pairs that lie inside one cluster."""
    idx = pair_index(n)
    return [idx[(q0 + i, q0 + j)] for q0, m in cluster_bounds(sizes) for i, j in itertools.combinations(range(m), 2)]


def restrict_to_cluster(st: Structure, sizes, c: int):
    """The problem of cluster c alone: (Structure on its qubits, positions of its pairs in the register's u_pairs).  A term whose mask
    misses the cluster keeps its place with an empty mask, so the tables need no re-indexing."""
    q0, m = cluster_bounds(sizes)[c]
    assert sum(sizes) == st.n_qubits
    if any(st.conditioned(k) for k in range(len(st.amp_masks))):
        assert q0 % 2 == 0 and m % 2 == 0, "conditioned flips: a cluster holds whole atoms"
    low = (1 << m) - 1
    idx = pair_index(st.n_qubits)
    pairs = [idx[(q0 + i, q0 + j)] for i, j in itertools.combinations(range(m), 2)]
    local = replace(st, n_qubits=m, amp_masks=tuple((mk >> q0) & low for mk in st.amp_masks),
                    det_masks=tuple((mk >> q0) & low for mk in st.det_masks))
    return local, pairs


def assert_separable(st: Structure, sizes, u):
    """u_pairs is zero between clusters (the masks split by construction)."""
    keep = torch.zeros(len(u), dtype=torch.bool)
    keep[intra_cluster_pairs(st.n_qubits, sizes)] = True
    assert float(u.detach().cpu()[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0, "u_pairs couples two clusters"


def cluster_states(st: Structure, sizes, amp, det, u, tsave, psi0_clusters, method: str = "dense", wrong=None):
    """The state of every cluster at every save time: a list (one entry per cluster) of (n_t, 2^m_c) tensors, differentiable in the
    tables (Ka, n) / (Kd, n), u, tsave and the clusters' initial states.  method "dense": the cluster's explicit matrix and
    accurate_matrix_exp; "matrix_free": reference (a) on the cluster (the sensitivity tests: it takes `wrong`)."""
    assert_separable(st, sizes, u)
    out = []
    for c in range(len(sizes)):
        local, pairs = restrict_to_cluster(st, sizes, c)
        u_c = u[pairs] if pairs else u[:0]
        p0 = psi0_clusters[c][None]
        states = (dense_krylov_map(local, amp, det, u_c, tsave, p0) if method == "dense"
                  else krylov_map(local, amp, det, u_c, tsave, p0, wrong))
        out.append(states[:, 0])
    return out


def product_state(cluster_vecs, device="cpu"):
    """The Kronecker product of one vector per cluster, built on `device` (qubit 0 is the most significant index bit: the first cluster
    is the leftmost factor)."""
    psi = torch.ones(1, dtype=torch.complex128, device=device)
    for v in cluster_vecs:
        psi = torch.kron(psi, v.detach().to(device=device, dtype=torch.complex128))
    return psi


def cluster_sum_values(states_per_cluster, tables):
    """<O>(t_k) of O = sum_c o_c (x) 1 (tables: one real (2^m_c,) per cluster) on the product of the cluster states, (n_t,), without
    anything of size 2^N:  sum_c <o_c>_c prod_{c' != c} |psi_c'|^2."""
    norms = [s.abs().square().sum(1) for s in states_per_cluster]
    total = 0.0
    for c, (s, o) in enumerate(zip(states_per_cluster, tables)):
        v = (s.abs().square() * o[None]).sum(1)
        for c2, nr in enumerate(norms):
            if c2 != c:
                v = v * nr
        total = total + v
    return total


def cluster_sum_table(tables, device="cpu"):
    """The diagonal of O = sum_c o_c (x) 1 as a (2^N,) table on `device`."""
    out = torch.zeros(1, dtype=torch.float64, device=device)
    for o in tables:
        out = (out[:, None] + o.to(device=device, dtype=torch.float64)[None, :]).reshape(-1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The seeded inputs of the GPU cases (tests/test_gpu_three_level_references.py); the host tests run their sensitivity checks on
# exactly these.
# ----------------------------------------------------------------------------------------------------------------------
THREE_LEVEL_TSAVE = (0.0, 0.004, 0.0095, 0.013, 0.0211)
THREE_LEVEL_NS, THREE_LEVEL_DT = 7, 0.004


def valid_codes(n_qubits: int) -> torch.Tensor:
    """The indices whose every atom (two qubits) holds one of the codes 01, 11, 10: the three levels."""
    x = torch.arange(2**n_qubits)
    ok = torch.ones(2**n_qubits, dtype=torch.bool)
    for k in range(n_qubits // 2):
        ok &= ((x >> (2 * k)) & 3) != 0
    return x[ok]


def three_level_structure(n_qubits: int, extended: bool = True) -> Structure:
    """The term list of test_conditioned_flips_and_ones_counting_terms_through_the_c_abi (every flip conditioned; the b qubits counted
    as ones) and, extended, one conditioned flip on the a qubit and one ones-counting detuning on the b qubit of the LAST atom, so
    that the lowest index bits carry a local term too."""
    n_atoms = n_qubits // 2
    a_mask, b_mask = sum(1 << (2 * i) for i in range(n_atoms)), sum(1 << (2 * i + 1) for i in range(n_atoms))
    amp_masks, amp_cond = (a_mask, 1 << 1, b_mask & ~(1 << 1)), (True, True, True)
    det_masks, det_ones = (a_mask, b_mask, 1 << 0), (False, True, False)
    if extended:
        amp_masks, amp_cond = amp_masks + (1 << (n_qubits - 2),), amp_cond + (True,)
        det_masks, det_ones = det_masks + (1 << (n_qubits - 1),), det_ones + (True,)
    return Structure(n_qubits, THREE_LEVEL_DT, THREE_LEVEL_NS, amp_masks, det_masks, amp_cond, det_ones)


def three_level_case(n_qubits: int, batch: int, per_trajectory: bool, extended: bool = True, seed: int = 4100) -> dict:
    """CPU tensors of one case: tables [Bc, K, n] (Bc = batch with per-trajectory tables, else 1; amplitudes 3 x complex normal,
    detunings 2 x normal), U in [5, 12) between the a qubits and 0 elsewhere, a random initial state inside the valid codes, a random
    diagonal observable in [0, 1), the weights linspace(0.4, 1.3) of <O>(t_k) and a random state cotangent of norm 1 per save
    point and trajectory (also inside the valid codes: the state never leaves them).  loss = case_loss."""
    st = three_level_structure(n_qubits, extended)
    gen = torch.Generator().manual_seed(seed + 16 * n_qubits + batch + (8 if per_trajectory else 0))
    bc = batch if per_trajectory else 1
    ns, dim = st.n_samples, 2**n_qubits
    amp = torch.randn(bc, len(st.amp_masks), ns, generator=gen, dtype=torch.complex128) * 3.0
    det = torch.randn(bc, len(st.det_masks), ns, generator=gen, dtype=torch.float64) * 2.0
    u = torch.tensor([float(5.0 + 7.0 * torch.rand(1, generator=gen)) if (i % 2 == 0 and j % 2 == 0) else 0.0
                      for i, j in itertools.combinations(range(n_qubits), 2)], dtype=torch.float64)
    valid = valid_codes(n_qubits)
    psi0 = torch.zeros(batch, dim, dtype=torch.complex128)
    psi0[:, valid] = torch.randn(batch, len(valid), generator=gen, dtype=torch.complex128)
    psi0 = psi0 / psi0.norm(dim=1, keepdim=True)
    obs = torch.rand(1, dim, generator=gen, dtype=torch.float64)
    tsave = torch.tensor(THREE_LEVEL_TSAVE, dtype=torch.float64)
    cot = torch.zeros(len(tsave), batch, dim, dtype=torch.complex128)
    cot[:, :, valid] = torch.randn(len(tsave), batch, len(valid), generator=gen, dtype=torch.complex128)
    cot = cot / cot.norm(dim=2, keepdim=True)
    return {"st": st, "amp": amp, "det": det, "u": u, "tsave": tsave, "psi0": psi0, "obs": obs,
            "w": torch.linspace(0.4, 1.3, len(tsave), dtype=torch.float64), "cot": cot}


def case_loss(states, expect, w, cot):
    """states (n_t, B, dim), expect (n_obs, n_t, B): every save point weighted through <O_0>, and the states through a cotangent."""
    return (expect[0] * w[:, None]).sum() + (cot.conj() * states).real.sum()


GRAD_KINDS = ("amp", "det", "u", "tsave", "psi0")


def reference_value_and_grads(case: dict, wrong=None) -> dict:
    """Reference (a) on a three_level_case: numpy states (n_t, B, dim), expect (1, n_t, B), the five gradients of case_loss in the
    shapes of the inputs, the Taylor terms per interval and the CPU seconds it took."""
    t0 = time.perf_counter()
    st = case["st"]
    leaves = {k: case[k].clone().requires_grad_(True) for k in GRAD_KINDS}
    shared = case["amp"].shape[0] == 1
    counts = []
    states = krylov_map(st, leaves["amp"][0] if shared else leaves["amp"], leaves["det"][0] if shared else leaves["det"],
                        leaves["u"], leaves["tsave"], leaves["psi0"], wrong, counts=counts)
    expect = (states.abs().square() * case["obs"][0][None, None, :]).sum(2)[None]
    case_loss(states, expect, case["w"], case["cot"]).backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    out.update(states=states.detach().numpy(), expect=expect.detach().numpy(), taylor_terms=counts, seconds=time.perf_counter() - t0)
    return out


# ---- cluster cases -----------------------------------------------------------------------------------------------------
CLUSTER_CASES = {
    # name: (cluster sizes, three-level?)
    "tl8": ((4, 4), True),      # host only: (b) against (a)
    "tl10": ((6, 4), True),     # host only
    "tl20": ((6, 4, 6, 4), True),
    "tl22": ((4, 6, 2, 6, 4), True),
    "tl24": ((6, 2, 4, 6, 2, 4), True),
    "plain22": ((6, 5, 4, 6, 1), False),
    "plain25": ((5, 6, 3, 6, 4, 1), False),
}


def _random_unit(m: int, gen, valid=None):
    v = torch.zeros(2**m, dtype=torch.complex128)
    idx = torch.arange(2**m) if valid is None else valid
    v[idx] = torch.randn(len(idx), generator=gen, dtype=torch.complex128)
    return v / v.norm()


def cluster_case(name: str, seed: int = 5200) -> dict:
    """CPU tensors of one cluster-separable case (one trajectory, KRYLOV_SE, the save times of the three-level cases).
    Three-level: every flip conditioned — the a qubits, the b qubits, and per cluster one local flip on a qubit whose place inside the
    cluster changes from cluster to cluster; detunings on the a qubits (zeros counted), on the b qubits (ones counted) and per
    cluster one local one (ones-counting on a b qubit, zeros-counting on an a qubit).  U: a distinct value for every pair of a qubits
    inside a cluster.  Plain: a global drive with a phase, a global detuning, local channels (drive and detuning) on the first, a
    middle and the last qubit; U: a distinct value for every pair inside a cluster.  Clusters of unequal sizes with different local
    terms, so that a misplaced index bit changes the product.  psi0: random cluster states (inside the valid codes)."""
    sizes, three_level = CLUSTER_CASES[name]
    n = sum(sizes)
    gen = torch.Generator().manual_seed(seed + n + (100 if three_level else 0))
    bounds = cluster_bounds(sizes)
    if three_level:
        a_mask, b_mask = sum(1 << q for q in range(0, n, 2)), sum(1 << q for q in range(1, n, 2))
        local_amp = [q0 + (c % m) for c, (q0, m) in enumerate(bounds)]
        local_det = [q0 + ((c + 1) % m) for c, (q0, m) in enumerate(bounds)]
        amp_masks = (a_mask, b_mask) + tuple(1 << q for q in local_amp)
        det_masks = (a_mask, b_mask) + tuple(1 << q for q in local_det)
        amp_cond = (True,) * len(amp_masks)
        det_ones = (False, True) + tuple(q % 2 == 1 for q in local_det)
        coupled = lambda i, j: i % 2 == 0 and j % 2 == 0  # noqa: E731
    else:
        every = (1 << n) - 1
        locals_ = (0, n // 2, n - 1)
        amp_masks = (every,) + tuple(1 << q for q in locals_)
        det_masks = (every,) + tuple(1 << q for q in locals_)
        amp_cond, det_ones = (), ()
        coupled = lambda i, j: True  # noqa: E731
    st = Structure(n, THREE_LEVEL_DT, THREE_LEVEL_NS, amp_masks, det_masks, amp_cond, det_ones)
    ns = st.n_samples
    amp = torch.randn(len(amp_masks), ns, generator=gen, dtype=torch.complex128) * (3.0 if three_level else 1.5)
    det = torch.randn(len(det_masks), ns, generator=gen, dtype=torch.float64) * 2.0
    u = torch.zeros(n * (n - 1) // 2, dtype=torch.float64)
    idx = pair_index(n)
    for q0, m in bounds:
        for i, j in itertools.combinations(range(q0, q0 + m), 2):
            if coupled(i, j):
                u[idx[(i, j)]] = float(5.0 + 7.0 * torch.rand(1, generator=gen))
    psi0 = [_random_unit(m, gen, valid_codes(m) if three_level else None) for _, m in bounds]
    tables = [torch.rand(2**m, generator=gen, dtype=torch.float64) for _, m in bounds]
    return {"st": st, "sizes": sizes, "amp": amp, "det": det, "u": u, "tsave": torch.tensor(THREE_LEVEL_TSAVE, dtype=torch.float64),
            "psi0": psi0, "tables": tables, "w": torch.linspace(0.4, 1.3, len(THREE_LEVEL_TSAVE), dtype=torch.float64),
            "intra": intra_cluster_pairs(n, sizes)}


CLUSTER_GRAD_KINDS = ("amp", "det", "u", "tsave")


def cluster_reference(case: dict, method: str = "dense", wrong=None) -> dict:
    """Reference (b) on a cluster_case: the cluster states (list of (n_t, 2^m_c) tensors, detached), <O_clustersum>(t_k) (n_t,) numpy
    and the gradients of sum_k w_k <O_clustersum>(t_k) in amp, det, tsave and u (of which only the entries case["intra"] mean
    anything: u is zero elsewhere and its gradient there is not the register's), the CPU seconds."""
    t0 = time.perf_counter()
    leaves = {k: case[k].clone().requires_grad_(True) for k in CLUSTER_GRAD_KINDS}
    states = cluster_states(case["st"], case["sizes"], leaves["amp"], leaves["det"], leaves["u"], leaves["tsave"], case["psi0"], method, wrong)
    values = cluster_sum_values(states, case["tables"])
    (values * case["w"]).sum().backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    out.update(states=[s.detach() for s in states], expect=values.detach().numpy(), seconds=time.perf_counter() - t0)
    return out
