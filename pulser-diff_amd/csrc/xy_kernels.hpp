// xy_kernels.hpp — the XY exchange family (RydProblem.xy_mode, include/rydiff.h): factor pass, its adjoint with the dL/dJ
// contractions, and the dL/dtau dot.  One amplitude per thread like the generic direct kernels (direct_kernels.hpp), whose group
// loops they repeat, plus the exchange stencil
//   mode 1:  (X v)[x] = sum_{i<j, b_i(x) != b_j(x)} J_ij v[x ^ m_i ^ m_j]
//   mode 2:  only the rows with b_i(x) = 0, b_j(x) = 1;  (X^dagger g)[x]: the rows with b_i(x) = 1, b_j(x) = 0   (J is real)
// b_q = index bit N-1-q, m_q = 1 << (N-1-q); pair (i, j) at p = i(2N-i-1)/2 + (j-i-1), the order of u_pairs.  N is a runtime value.
// As in k_factor_direct_global the chain of dependent L2 latencies is the kernel time, so the partner loads of a row i (all j > i,
// kXyRow at a time) are issued together before any sum consumes one; J_ij is read with a wave-uniform index.
#pragma once

struct XyArgs {
    int mode = 0;               // 0: none | 1: Hermitian | 2: one-directional
    int N = 0;                  // qubits = index bits
    const double* J = nullptr;  // [N(N-1)/2]
};

// what the tangent sweep's factor pass adds (k_factor_tangent<D, false, true>, tangent_kernels.hpp): the tangents of the couplings
struct XyTangentArgs {
    XyArgs xy;
    const double* dJ = nullptr;  // [D][P], direction outermost, padded directions zero; nullptr: no d_xy (zero)
    int P = 0;                   // N(N-1)/2
};

constexpr int kXyRow = 8;  // partner loads of one row in flight together (16 bytes each)
constexpr int kXyMaxPairs = RYDIFF_MAX_QUBITS * (RYDIFF_MAX_QUBITS - 1) / 2;

// For each of the NV vectors v + w * vstride (w = 0 .. NV-1):  (er[w], ei[w]) += sum_p J_p * v_w[partner_p(x)] over the pairs whose row x
// belongs to the stencil (ADJ: that of X^dagger), and each(p, part) for EVERY pair in order, wave-uniformly, with part[w] = the partner
// amplitude of vector w where the stencil has one and 0 elsewhere.  ROW pairs of one row at a time: ROW * NV loads in flight.
// x < 2^N always (dead threads pass live = false and x = 0: no loads).
template <bool ADJ, int NV, int ROW, class Each>
__device__ __forceinline__ void xy_stencil_n(const XyArgs& xy, const double2* __restrict__ v, size_t vstride, uint32_t x, bool live,
                                             double (&er)[NV], double (&ei)[NV], Each&& each) {
    const int N = xy.N;
    int p0 = 0;
    for (int i = 0; i + 1 < N; ++i) {  // uniform
        const uint32_t mi = 1u << (N - 1 - i);
        const bool bi = (x & mi) != 0u;
        const int len = N - 1 - i;
        for (int c0 = 0; c0 < len; c0 += ROW) {
            double2 part[ROW][NV];
#pragma unroll
            for (int c = 0; c < ROW; ++c) {
                const int jj = c0 + c;
#pragma unroll
                for (int w = 0; w < NV; ++w) part[c][w] = make_double2(0.0, 0.0);
                if (jj < len) {  // uniform
                    const uint32_t mj = mi >> (jj + 1);
                    const bool bj = (x & mj) != 0u;
                    bool act = live && bi != bj;
                    if (xy.mode == 2) act = act && bi == ADJ;
                    if (act) {
#pragma unroll
                        for (int w = 0; w < NV; ++w) part[c][w] = v[size_t(w) * vstride + (x ^ mi ^ mj)];
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // no sum of this row before all of its loads are issued
#pragma unroll
            for (int c = 0; c < ROW; ++c) {
                const int jj = c0 + c;
                if (jj < len) {  // uniform
                    const double Jv = xy.J[p0 + jj];
#pragma unroll
                    for (int w = 0; w < NV; ++w) {
                        er[w] = fma(Jv, part[c][w].x, er[w]);
                        ei[w] = fma(Jv, part[c][w].y, ei[w]);
                    }
                    each(p0 + jj, part[c]);
                }
            }
        }
        p0 += len;
    }
}

// one vector, kXyRow loads in flight: each(p, part) with the one partner amplitude
template <bool ADJ, class Each>
__device__ __forceinline__ void xy_stencil(const XyArgs& xy, const double2* __restrict__ v, uint32_t x, bool live, double& er, double& ei,
                                           Each&& each) {
    double r[1] = {er}, i[1] = {ei};
    xy_stencil_n<ADJ, 1, kXyRow>(xy, v, 0, x, live, r, i, [&](int p, const double2(&part)[1]) { each(p, part[0]); });
    er = r[0];
    ei = i[0];
}

// c_g * (partner sum over the set bits of x) + conj(c_g) * (partner sum over the clear bits), summed over the flip groups
// (no conditioned flips: refused with the exchange)
__device__ __forceinline__ void xy_group_sums(const GroupArgs& g, const double2* __restrict__ v, uint32_t x, int q, double& s1r, double& s1i,
                                              double& s0r, double& s0i) {
    s1r = s1i = s0r = s0i = 0.0;
    uint32_t m = g.amask[q];
    while (m) {
        const uint32_t bit = m & (0u - m);
        m ^= bit;
        const double2 p = v[x ^ bit];
        if (x & bit) {
            s1r += p.x;
            s1i += p.y;
        } else {
            s0r += p.x;
            s0i += p.y;
        }
    }
}

// y = (gamma + beta (D + flips + X)) x
__global__ __launch_bounds__(256) void k_factor_xy(FactorArgs a, XyArgs xy) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const uint32_t xs = live ? x : 0u;
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.coef + blockIdx.y * a.coef_bstride;
    const double d = diag_value(a.udiag, cf, a.g, xs);
    const double2 v = xin[xs];
    const double dr = a.gr + a.br * d, di = a.gi + a.bi * d;
    double ar = dr * v.x - di * v.y, ai = dr * v.y + di * v.x;
    for (int q = 0; q < a.g.ga; ++q) {
        double s1r, s1i, s0r, s0i;
        xy_group_sums(a.g, xin, xs, q, s1r, s1i, s0r, s0i);
        const double cr = cf[q], ci = cf[a.g.ga + q];
        // beta*c and beta*conj(c)
        const double b1r = a.br * cr - a.bi * ci, b1i = a.br * ci + a.bi * cr;
        const double b0r = a.br * cr + a.bi * ci, b0i = -a.br * ci + a.bi * cr;
        ar += b1r * s1r - b1i * s1i + b0r * s0r - b0i * s0i;
        ai += b1r * s1i + b1i * s1r + b0r * s0i + b0i * s0r;
    }
    double er = 0.0, ei = 0.0;
    xy_stencil<false>(xy, xin, xs, live, er, ei, [](int, const double2&) {});
    ar += a.br * er - a.bi * ei;  // beta once, on the whole exchange sum
    ai += a.br * ei + a.bi * er;
    if (live) a.xout[boff + x] = make_double2(ar, ai);
}

// gout = (conj(gamma) + conj(beta) (D + flips + X)^dagger) gin, the contractions of k_factor_bwd_direct, and
//   dL/dJ_p += Re sum_x beta conj(gin[x]) (dX/dJ_p xin)[x] = Re sum_y beta conj(gin[partner_p(y)]) xin[y]   over the rows y of the
// ADJOINT stencil (the partner of a forward row is an adjoint row): the cotangent's partner loads, which the matvec needs anyway,
// and the own tape element only.  Per pair: wave reduction -> LDS, then one atomic per pair and workgroup into replica
// (workgroup % kXyReplicas) of xy_ge, which accumulates over all factors and trajectories of the sweep.
__global__ __launch_bounds__(256) void k_factor_bwd_xy(FactorBwdArgs a, XyArgs xy, double* __restrict__ xy_ge) {
    __shared__ double lds[8];
    __shared__ double xl[4][kXyMaxPairs];
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const uint32_t xs = live ? x : 0u;
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ gin = a.gin + boff;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.coef + blockIdx.y * a.coef_bstride;
    double* __restrict__ ge = a.ge + blockIdx.y * a.ge_bstride + (blockIdx.x % kGradReplicas) * a.ge_rstride;
    const double d = diag_value(a.udiag, cf, a.g, xs);
    double2 gy = gin[xs];
    double2 xi = xin[xs];
    if (!live) {
        gy = make_double2(0.0, 0.0);
        xi = make_double2(0.0, 0.0);
    }
    const double dr = a.gr + a.br * d, di = -(a.gi + a.bi * d);
    double ar = dr * gy.x - di * gy.y, ai = dr * gy.y + di * gy.x;
    const double pr = a.br * gy.x + a.bi * gy.y, pi = a.bi * gy.x - a.br * gy.y;  // beta conj(gy)
    const double r = pr * xi.x - pi * xi.y;                                       // Re(beta conj(gy) xi)
    if (a.wtot && live) unsafeAtomicAdd(a.wtot + x, r);
    for (int q = 0; q < a.g.ga; ++q) {
        double s1r, s1i, s0r, s0i;  // partner sums of gin: for the matvec AND (re-indexed over the partner) for the contraction
        xy_group_sums(a.g, gin, xs, q, s1r, s1i, s0r, s0i);
        const double cr = cf[q], ci = cf[a.g.ga + q];
        // conj(beta)*c and conj(beta)*conj(c)
        const double b1r = a.br * cr + a.bi * ci, b1i = a.br * ci - a.bi * cr;
        const double b0r = a.br * cr - a.bi * ci, b0i = -a.br * ci - a.bi * cr;
        ar += b1r * s1r - b1i * s1i + b0r * s0r - b0i * s0i;
        ai += b1r * s1i + b1i * s1r + b0r * s0i + b0i * s0r;
        double gre = 0.0, gim = 0.0;
        if (live) {  // as in k_factor_bwd_direct
            const double q0r = a.br * s0r + a.bi * s0i, q0i = a.bi * s0r - a.br * s0i;  // beta conj(s0)
            const double q1r = a.br * s1r + a.bi * s1i, q1i = a.bi * s1r - a.br * s1i;  // beta conj(s1)
            const double S1r = q0r * xi.x - q0i * xi.y, S1i = q0r * xi.y + q0i * xi.x;
            const double S0r = q1r * xi.x - q1i * xi.y, S0i = q1r * xi.y + q1i * xi.x;
            gre = S1r + S0r;
            gim = -(S1i - S0i);
        }
        block_atomic_add(gre, ge + q, lds);
        block_atomic_add(gim, ge + a.g.ga + q, lds);
    }
    for (int q = 0; q < a.g.gd; ++q) {
        const double v = live ? r * double(a.g.dcnt[q] - popc_i(xs & a.g.dmask[q])) : 0.0;
        block_atomic_add(v, ge + 2 * a.g.ga + q, lds);
    }
    // t = beta xi:  Re(beta conj(part) xi) = part.x t.x + part.y t.y   (xi = 0 on dead threads, part = 0 off the stencil)
    const double tr = a.br * xi.x - a.bi * xi.y, ti = a.br * xi.y + a.bi * xi.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double er = 0.0, ei = 0.0;
    xy_stencil<true>(xy, gin, xs, live, er, ei, [&](int p, const double2& part) {
        if (xy_ge) {  // uniform
            const double w = wave_sum(part.x * tr + part.y * ti);
            if (lane == 0) xl[wave][p] = w;
        }
    });
    ar += a.br * er + a.bi * ei;  // conj(beta) once
    ai += a.br * ei - a.bi * er;
    if ((a.inj_gexp || a.inj_gstate) && live) {
        const double2 add = injected_cotangent(a.inj_gstate, a.inj_gexp, a.inj_obs, a.inj_n_obs, a.inj_ostride, a.obs_ostride, a.obs_bstride,
                                               blockIdx.y, boff, x, xi);
        ar += add.x;
        ai += add.y;
    }
    if (live) a.gout[boff + x] = make_double2(ar, ai);
    if (xy_ge) {
        const int P = xy.N * (xy.N - 1) / 2;
        double* __restrict__ rep = xy_ge + size_t((blockIdx.x + blockIdx.y) % kXyReplicas) * P;
        __syncthreads();
        for (int p = threadIdx.x; p < P; p += 256) unsafeAtomicAdd(rep + p, (xl[0][p] + xl[1][p]) + (xl[2][p] + xl[3][p]));
    }
}

// g_xy[p] = sum of the replicas, in a fixed order (overwrites)
__global__ void k_xy_contract(double* __restrict__ g_xy, const double* __restrict__ xy_ge, int P) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int r = 0; r < kXyReplicas; ++r) s += xy_ge[size_t(r) * P + p];
    g_xy[p] = s;
}

// dL/dtau of one exponential, Im( sum_x conj(g[x]) (H x)[x] ) with the exchange in H.  H always acts on x: in mode 2 it is not
// Hermitian and may not change sides.
__global__ __launch_bounds__(256) void k_dot_hx_xy(DotHArgs a, XyArgs xy) {
    __shared__ double lds[8];
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const uint32_t xs = live ? x : 0u;
    const int bt = a.b_first + int(blockIdx.y);
    const size_t boff = size_t(bt) * a.dim;
    const double2* __restrict__ xin = a.x + boff;
    const double* __restrict__ cf = a.coef + bt * a.coef_bstride;
    const double d = diag_value(a.udiag, cf, a.gr, xs);
    const double2 v = xin[xs];
    double hr = d * v.x, hi = d * v.y;
    for (int q = 0; q < a.gr.ga; ++q) {
        double s1r, s1i, s0r, s0i;
        xy_group_sums(a.gr, xin, xs, q, s1r, s1i, s0r, s0i);
        const double cr = cf[q], ci = cf[a.gr.ga + q];
        hr += cr * s1r - ci * s1i + cr * s0r + ci * s0i;
        hi += cr * s1i + ci * s1r + cr * s0i - ci * s0r;
    }
    xy_stencil<false>(xy, xin, xs, live, hr, hi, [](int, const double2&) {});
    const double2 g = a.g[boff + xs];
    const double val = live ? (g.x * hi - g.y * hr) : 0.0;  // Im(conj(g) h)
    block_atomic_add(val, a.out + bt * a.out_bstride + (blockIdx.x % kGradReplicas) * a.out_rstride, lds);
}
