// tangent_kernels.hpp — forward-mode (tangent) sweep (include/rydiff.h: rydiff_forward_tangent): the state and D tangent states
// advance together through every factor pass,
//   y    = (gamma + beta H) x
//   dy_d = (gamma + beta H) dx_d + beta dH_d x,      dH_d = H built from the tangent coefficient record of direction d
// k_factor_tangent<D>     one launch per factor, one amplitude per thread: (1 + D) reads and (1 + D) writes of the vectors.  The own
//                         value x[y] and every partner x[y ^ bit] are loaded ONCE and serve H x and all D products dH_d x (only the
//                         coefficient records differ); the partners of the dx_d are loaded per direction.  The partner loads of a
//                         chunk of flip bits — of x and of every dx_d — are issued together, before any sum consumes one, so a pass
//                         is NOT a chain of N dependent L2 latencies (DESIGN.md section 3 on the generic direct kernel).
// k_expect_tangent        d<O> of the diagonal observables: 2 sum_y o[y] Re(conj psi[y] dpsi_d[y])
// k_pauli_expect_tangent  d<O> of the Pauli observables: the direct Pauli reduction with bra = psi and ket = dpsi_d, times 2
// k_factor_tangent<D, true>  the same pass with dense pair terms P (constants in every direction: M = H + P, dM_d has no pair part):
//                         beta P on all 1 + D vectors by pair_apply_all (common.hpp) — the collapse operators of a master-equation run
//                         on the doubled register, the XY exchange on kets.  <D, false> is the pass without them, unchanged.
// k_factor_tangent<D, false, true>  the same pass with the XY exchange X(J) of xy_kernels.hpp (RYDIFF_TANGENT_XY), whose couplings have
//                         tangents dJ_d of their own:  dy_d += beta (X(J) dx_d + X(dJ_d) x).  One walk of the stencil (xy_stencil_n)
//                         over all 1 + D vectors: per pair the partner of x is loaded once and serves J x and the D products dJ_d x,
//                         the partners of the dx_d serve J dx_d; TangentChunk<D> pairs of one row in flight together; J and dJ are
//                         read with wave-uniform indices; beta once on each vector's whole exchange sum.
// (the overlap rows are k_overlap_expect on dpsi_d, as it is; the density-matrix rows of a doubled register are k_dm_trace /
// k_dm_fidelity on dpsi_d and k_dm_purity_tangent, dm_kernels.hpp).  Complex coefficients throughout, no rotating frame,
// no conditioned flips, no sharding (refused by the C ABI).
#pragma once

struct TangentFactorArgs {
    const double2* xin;    // vector v (0: the state, 1 + d: tangent d) of trajectory b at xin + v * vstride + b * dim
    double2* xout;
    size_t vstride;        // B * dim
    const double* udiag;   // [dim]
    const double* dudiag;  // [D][dim]: interaction diagonal of the tangent U, or nullptr (no d_u)
    const double* coef;    // record of this exponential, trajectory 0: c_re[ga], c_im[ga], dcoef[gd]
    const double* dcoef;   // the same record of direction 0 (tangent tables)
    long coef_bstride;     // doubles between trajectories' records (0: shared)
    long dcoef_dstride;    // doubles between the record sets of consecutive directions
    uint32_t dim;
    double gr, gi, br, bi;  // gamma, beta
    int ga, gd, nflip;
    uint32_t dmask[kMaxGroups];  // amplitude-index bit masks of the detuning groups
    int dcnt[kMaxGroups];
    uint32_t fbg[RYDIFF_MAX_QUBITS];  // the driven qubits, one word each: amplitude-index bit number | flip group << 8
    PairArgs pair;         // dense pair terms (read by the PAIR instantiations only): constants in every tangent direction
    XyTangentArgs xyt;     // XY exchange and the tangents of its couplings (read by the XY instantiations only)
};

// flip bits whose partner loads are in flight together: CH * (1 + D) loads of 16 bytes per thread
template <int D>
struct TangentChunk {
    static constexpr int value = D <= 1 ? 8 : (D <= 3 ? 4 : 2);
};

template <int D, bool PAIR, bool XY = false>
__global__ __launch_bounds__(256) void k_factor_tangent(TangentFactorArgs a) {
    constexpr int CH = TangentChunk<D>::value;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.dim) return;
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.coef + blockIdx.y * a.coef_bstride;
    const double* __restrict__ dcf = a.dcoef + blockIdx.y * a.coef_bstride;
    const int ga = a.ga;

    // own values: issued first, consumed after the diagonals are formed
    double2 own[1 + D];
#pragma unroll
    for (int v = 0; v <= D; ++v) own[v] = xin[size_t(v) * a.vstride + x];

    // diagonal d(x) and its tangents
    double dg = a.udiag[x];
    double ddg[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ddg[d] = a.dudiag ? a.dudiag[size_t(d) * a.dim + x] : 0.0;
    for (int q = 0; q < a.gd; ++q) {
        const double occ = double(a.dcnt[q] - popc_i(x & a.dmask[q]));
        dg += cf[2 * ga + q] * occ;
#pragma unroll
        for (int d = 0; d < D; ++d) ddg[d] += dcf[d * a.dcoef_dstride + 2 * ga + q] * occ;
    }
    double accr[1 + D], acci[1 + D];
    {
        const double dr = a.gr + a.br * dg, di = a.gi + a.bi * dg;
        accr[0] = dr * own[0].x - di * own[0].y;
        acci[0] = dr * own[0].y + di * own[0].x;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double tr = a.br * ddg[d], ti = a.bi * ddg[d];  // beta * d'(x)
            accr[1 + d] = dr * own[1 + d].x - di * own[1 + d].y + tr * own[0].x - ti * own[0].y;
            acci[1 + d] = dr * own[1 + d].y + di * own[1 + d].x + tr * own[0].y + ti * own[0].x;
        }
    }
    // beta * (dense pair terms) on all 1 + D vectors, while the own values are still in registers: the pair part of M is the same
    // in (gamma + beta M) dx_d, and dM_d has none
    if constexpr (PAIR) pair_apply_all<1 + D>(a.pair, xin, a.vstride, x, own, a.br, a.bi, accr, acci);

    for (int i0 = 0; i0 < a.nflip; i0 += CH) {  // uniform
        // the chunk's flip bits, groups and coefficients first: wave-uniform words (scalar loads), nothing of them waits on the
        // vector-memory counter between the partner loads below
        uint32_t bit[CH];
        double mr[CH], mi[CH], tr[CH][D], ti[CH][D];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const bool in = i0 + c < a.nflip;  // past the end: the own line again, weight 0
            const uint32_t bg = in ? a.fbg[i0 + c] : 0u;
            bit[c] = in ? (1u << (bg & 31u)) : 0u;
            const int q = int(bg >> 8);
            mr[c] = in ? cf[q] : 0.0;
            mi[c] = in ? cf[ga + q] : 0.0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                tr[c][d] = in ? dcf[d * a.dcoef_dstride + q] : 0.0;
                ti[c][d] = in ? dcf[d * a.dcoef_dstride + ga + q] : 0.0;
            }
        }
        double2 part[CH][1 + D];
#pragma unroll
        for (int c = 0; c < CH; ++c)  // the chunk's partner loads, all vectors: in flight together
#pragma unroll
            for (int v = 0; v <= D; ++v) part[c][v] = xin[size_t(v) * a.vstride + (x ^ bit[c])];
        __builtin_amdgcn_sched_barrier(0);  // the scheduler may not sink a later bit's loads below the first bit's sums
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const bool up = (x & bit[c]) != 0u;  // bit_j(x) = 1: coefficient c, else conj(c)
            {
                const double cr = mr[c], ci = up ? mi[c] : -mi[c];
                const double kr = a.br * cr - a.bi * ci, ki = a.br * ci + a.bi * cr;  // beta * (c or conj c)
#pragma unroll
                for (int v = 0; v <= D; ++v) {
                    accr[v] += kr * part[c][v].x - ki * part[c][v].y;
                    acci[v] += kr * part[c][v].y + ki * part[c][v].x;
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {  // beta * (c'_d or its conjugate) * x[y ^ bit]
                const double cr = tr[c][d], ci = up ? ti[c][d] : -ti[c][d];
                const double kr = a.br * cr - a.bi * ci, ki = a.br * ci + a.bi * cr;
                accr[1 + d] += kr * part[c][0].x - ki * part[c][0].y;
                acci[1 + d] += kr * part[c][0].y + ki * part[c][0].x;
            }
        }
    }
    if constexpr (XY) {
        // X(J) on all 1 + D vectors and X(dJ_d) x into vector 1 + d, from the same partner loads
        double er[1 + D], ei[1 + D];
#pragma unroll
        for (int v = 0; v <= D; ++v) er[v] = ei[v] = 0.0;
        const double* __restrict__ dJ = a.xyt.dJ;
        const int P = a.xyt.P;
        xy_stencil_n<false, 1 + D, CH>(a.xyt.xy, xin, a.vstride, x, true, er, ei, [&](int p, const double2(&part)[1 + D]) {
            if (dJ) {  // uniform
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double dj = dJ[d * P + p];  // wave-uniform index
                    er[1 + d] = fma(dj, part[0].x, er[1 + d]);
                    ei[1 + d] = fma(dj, part[0].y, ei[1 + d]);
                }
            }
        });
#pragma unroll
        for (int v = 0; v <= D; ++v) {  // beta once, on each vector's whole exchange sum
            accr[v] += a.br * er[v] - a.bi * ei[v];
            acci[v] += a.br * ei[v] + a.bi * er[v];
        }
    }
#pragma unroll
    for (int v = 0; v <= D; ++v) a.xout[size_t(v) * a.vstride + boff + x] = make_double2(accr[v], acci[v]);
}

// grid (blocks, B, n_dir): out[d][o][k][b] += 2 sum_y obs[o][y] Re(conj psi[y] dpsi_d[y])
__global__ __launch_bounds__(256) void k_expect_tangent(const double2* __restrict__ psi, const double2* __restrict__ dpsi /* direction 0 */,
                                                        size_t vstride, const double* __restrict__ obs, double* __restrict__ out,
                                                        size_t out_dstride, int n_obs, int n_tsave, int k, int B, uint32_t dim) {
    __shared__ double lds[8];
    const int b = blockIdx.y, d = blockIdx.z;
    const double2* __restrict__ p = psi + size_t(b) * dim;
    const double2* __restrict__ t = dpsi + size_t(d) * vstride + size_t(b) * dim;
    for (int o = 0; o < n_obs; ++o) {
        double s = 0.0;
        for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < dim; x += gridDim.x * 256u) {
            const double2 v = p[x], w = t[x];
            s += obs[size_t(o) * dim + x] * (v.x * w.x + v.y * w.y);
        }
        block_atomic_add(2.0 * s, out + size_t(d) * out_dstride + (size_t(o) * n_tsave + k) * B + b, lds);
    }
}

struct PauliTangentArgs {
    const double2* psi;   // the state at the save point, trajectory 0
    const double2* dpsi;  // tangent 0 there
    size_t vstride;       // amplitudes between consecutive tangents
    PauliTables t;
    double* out;          // &dexpect_out[0][n_obs][0][0]
    size_t out_dstride;   // doubles between directions
    int n_pobs, n_tsave, k, B;
    uint32_t dim;
};

// grid (blocks, B, n_pobs * n_dir): 2 sum_s w_s Re<psi|P_s|dpsi_d> — k_pauli_expect_direct with two vectors; every group of the
// observable is evaluated here (no tile passes on this path)
__global__ __launch_bounds__(256) void k_pauli_expect_tangent(PauliTangentArgs a) {
    __shared__ double lds[8];
    const int b = blockIdx.y;
    const int o = int(blockIdx.z) % a.n_pobs, d = int(blockIdx.z) / a.n_pobs;
    const double2* __restrict__ psi = a.psi + size_t(b) * a.dim;
    const double2* __restrict__ ket = a.dpsi + size_t(d) * a.vstride + size_t(b) * a.dim;
    const int g0 = a.t.gfirst[o], g1 = a.t.gfirst[o + 1];
    double acc = 0.0;
    for (uint32_t y = blockIdx.x * 256u + threadIdx.x; y < a.dim; y += gridDim.x * 256u) {
        const double2 v = psi[y];
        for (int g = g0; g < g1; ++g) {  // uniform
            const PauliGroup gr = a.t.groups[g];
            const uint32_t yp = y ^ gr.xm;
            const double2 q = ket[yp];
            const double tr = v.x * q.x + v.y * q.y, ti = v.x * q.y - v.y * q.x;  // conj(psi[y]) * dpsi[y ^ xm]
            for (uint32_t s = gr.first; s < gr.first + gr.count; ++s) {
                const PauliString st = a.t.strings[s];
                const double val = st.wr * tr - st.wi * ti;
                acc += (__popc(yp & st.zm) & 1u) ? -val : val;
            }
        }
    }
    block_atomic_add(2.0 * acc, a.out + size_t(d) * a.out_dstride + (size_t(o) * a.n_tsave + a.k) * a.B + b, lds);
}
