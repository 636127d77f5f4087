"""Dense numpy references for the reduced density matrices of a density-matrix register (RydProblem.n_dm_rdms / dm_rdm_masks):
the partial trace as a reshape to 2n two-level axes and an einsum over the traced ones — no index arithmetic shared with the library or
with observables.reduced_density_matrix — the sum of the absolute terms of every entry, and the dense cotangent rydiff.h writes down."""
import numpy as np

_LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def _subscripts(n: int, atoms) -> str:
    """einsum subscripts of rho as a (2,) * 2n tensor (row atoms 0..n-1, column atoms 0..n-1) -> (rows of `atoms` in the order given,
    columns likewise): the traced atoms carry the same letter on both sides."""
    atoms = [int(q) for q in atoms]
    assert len(set(atoms)) == len(atoms) and all(0 <= q < n for q in atoms) and 2 * n <= len(_LETTERS)
    row = list(_LETTERS[:n])
    col = [_LETTERS[n + q] if q in atoms else row[q] for q in range(n)]
    return "".join(row) + "".join(col) + "->" + "".join(row[q] for q in atoms) + "".join(col[q] for q in atoms)


def partial_trace(rho: np.ndarray, n: int, atoms) -> np.ndarray:
    """Tr_E rho for rho (2^n, 2^n) -> (2^m, 2^m); the matrix index enumerates the settings of `atoms` with the first listed most
    significant.  No Hermiticity assumed."""
    m = len(atoms)
    return np.einsum(_subscripts(n, atoms), rho.reshape((2,) * (2 * n))).reshape(2 ** m, 2 ** m)


def partial_trace_with_totals(rho: np.ndarray, n: int, atoms):
    """(Tr_E rho, sum over e of |term|) — the second is what a rounding bound of a fixed-order sum is relative to."""
    return partial_trace(rho, n, atoms), partial_trace(np.abs(rho).astype(np.float64), n, atoms)


def mask_atoms(mask: int) -> list:
    """The atoms of a mask (bit j = atom j) in ascending order: the library's layout of the matrix."""
    return [j for j in range(32) if mask >> j & 1]


def rdm_rows_reference(v: np.ndarray, n: int, masks):
    """The RDM rows of one vector v = vec(rho) (4^n,) in the order of expect_out: per mask 2 * 4^m rows, entry (a, a') at offset
    2 * (a * 2^m + a'), Re then Im.  Returns (values, sums of absolute terms) as float64 arrays."""
    rho = v.reshape(2 ** n, 2 ** n)
    val, tot = [], []
    for mask in masks:
        r, t = partial_trace_with_totals(rho, n, mask_atoms(int(mask)))
        val.append(np.stack([r.real, r.imag], axis=-1).reshape(-1))
        tot.append(np.stack([t, t], axis=-1).reshape(-1))
    return np.concatenate(val), np.concatenate(tot)


def rdm_cotangent_reference(n: int, masks, g):
    """The dense cotangent of the RDM rows with weights g (in the order of rdm_rows_reference): G[a][a'] = gRe + i gIm at every entry
    (idx(a, e), idx(a', e)).  Built by scattering through an index tensor (2,) * 2n.  Returns (cotangent (4^n,) complex, sum of the
    absolute contributions per entry (4^n,))."""
    dim = 2 ** n
    cot = np.zeros((dim, dim), dtype=np.complex128)
    tot = np.zeros((dim, dim), dtype=np.float64)
    bits = (np.arange(dim)[:, None] >> (n - 1 - np.arange(n))[None, :]) & 1  # (dim, n): atom j of index x
    g = np.asarray(g, dtype=np.float64)
    r = 0
    for mask in masks:
        atoms = mask_atoms(int(mask))
        m = len(atoms)
        rest = [q for q in range(n) if q not in atoms]
        G = (g[r:r + 2 * 4 ** m:2] + 1j * g[r + 1:r + 2 * 4 ** m:2]).reshape(2 ** m, 2 ** m)
        r += 2 * 4 ** m
        sub = (bits[:, atoms] << (m - 1 - np.arange(m))[None, :]).sum(axis=1)  # setting of A in index x, first atom most significant
        same_e = (bits[:, None, rest] == bits[None, :, rest]).all(axis=2) if rest else np.ones((dim, dim), dtype=bool)
        add = G[sub[:, None], sub[None, :]]
        cot += np.where(same_e, add, 0.0)
        tot += np.where(same_e, np.abs(add), 0.0)
    assert r == len(g)
    return cot.reshape(-1), tot.reshape(-1)
