// fisher_kernels.hpp — "classical Gram matrix" of the vectors the tangent sweep holds at a save point (include/rydiff.h:
// rydiff_forward_fisher): with u[y] = psi[y] / |psi[y]| the phase of the amplitude, the REAL vectors
//   w_0[y] = |psi[y]| = sqrt p[y],   w_{1+d}[y] = 2 Re(conj(u[y]) dpsi_d[y]) = dp_d[y] / sqrt p[y]
// and C_ij = sum_y w_i[y] w_j[y], from which the classical Fisher information of the occupation-basis measurement is formed like
// the quantum one from the Gram matrix:  F_C,de = C_{1+d,1+e} / S - C_{0,1+d} C_{0,1+e} / S^2,  S = C_00.  An amplitude that is
// exactly zero contributes nothing (w_i[y] = 0 for every i: the sum over the support).
// k_tangent_cfi<D>    the twin of k_tangent_gram<D> (gram_kernels.hpp): the same grid and grid-stride loop, the 1 + D loads of an
//                     amplitude in flight before the first use, the upper triangle of C in registers — (1 + D)(2 + D) / 2 <= 45
//                     doubles — the block reduction in the FIXED pattern (wave64 shuffle tree, then the four waves through LDS in
//                     order), the block's partial to the workspace with ordinary vector stores.  No atomics: two calls return the
//                     same bits.
//                     The phase without a divide and without forming |psi|^2: the larger of |Re|, |Im| gives a power of two 2^e;
//                     s = psi 2^-e is exact, |s|^2 lies in [1/4, 2), so r = rsqrt(|s|^2) neither overflows nor underflows for any
//                     finite amplitude, denormals included:  u = s r,  |psi| = |s|^2 r 2^e.
// k_cfi_finish        sums the block partials in the fixed tree of k_gram_finish (lane l takes blocks l, l + 64, ... ascending, then
//                     the wave tree) and writes the FULL symmetric matrix: both triangles are the same sum in the same order.  Every
//                     entry of the slice is written.
// Partial layout: [block][B][(1 + D)(2 + D) / 2] doubles, the upper triangle row by row: (i, j), i <= j, at i (1 + D) - i (i - 1) / 2 + j - i.
#pragma once

template <int D>
__global__ __launch_bounds__(256) void k_tangent_cfi(const double2* __restrict__ vec /* [1 + D][B][dim] */, size_t vstride,
                                                     double* __restrict__ partial, uint32_t dim) {
    constexpr int NV = 1 + D, NT = NV * (NV + 1) / 2;
    __shared__ double lds[4][NT];
    const int b = blockIdx.y, B = gridDim.y;
    const double2* __restrict__ v0 = vec + size_t(b) * dim;
    double acc[NT];
#pragma unroll
    for (int e = 0; e < NT; ++e) acc[e] = 0.0;
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < dim; x += gridDim.x * 256u) {
        double2 v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = v0[size_t(i) * vstride + x];  // all loads in flight together
        __builtin_amdgcn_sched_barrier(0);  // the scheduler may not sink a later vector's load below the first products
        int e2;
        (void)frexp(fmax(fabs(v[0].x), fabs(v[0].y)), &e2);  // exponent only; 0 for a zero amplitude
        const double sx = ldexp(v[0].x, -e2), sy = ldexp(v[0].y, -e2);  // exact
        const double s2 = sx * sx + sy * sy;                            // in [1/4, 2), or an exact 0
        const double r = s2 > 0.0 ? rsqrt(s2) : 0.0;                    // the zero rule: u = 0, every w = 0
        const double ux = 2.0 * (sx * r), uy = 2.0 * (sy * r);          // 2 u
        double w[NV];
        w[0] = ldexp(s2 * r, e2);
#pragma unroll
        for (int i = 1; i < NV; ++i) w[i] = ux * v[i].x + uy * v[i].y;  // 2 Re conj(u) dpsi
        int e = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int j = i; j < NV; ++j) acc[e++] += w[i] * w[j];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < NT; ++e) {
        const double s = wave_sum(acc[e]);  // fixed shuffle tree
        if (lane == 0) lds[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < NT) {
        const int e = threadIdx.x;
        partial[(size_t(blockIdx.x) * B + b) * NT + e] = ((lds[0][e] + lds[1][e]) + lds[2][e]) + lds[3][e];
    }
}

// grid (n * n, B), one wave per output entry (i, j): n = 1 + n_dir rows are written, np = 1 + padded width is the partials' triangle
__global__ __launch_bounds__(64) void k_cfi_finish(const double* __restrict__ partial, int nblocks, int np, int n,
                                                   double* __restrict__ cgram /* &cgram_out[k][0][0][0] */) {
    const int b = blockIdx.y, B = gridDim.y;
    const int i = int(blockIdx.x) / n, j = int(blockIdx.x) % n;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int nt = np * (np + 1) / 2;
    const size_t bstride = size_t(B) * nt;
    const double* __restrict__ src = partial + size_t(b) * nt + (lo * np - lo * (lo - 1) / 2 + hi - lo);
    double s = 0.0;
    for (int blk = threadIdx.x; blk < nblocks; blk += 64) s += src[size_t(blk) * bstride];  // ascending, the same trip for every entry
    s = wave_sum(s);
    if (threadIdx.x == 0) cgram[(size_t(b) * n + i) * n + j] = s;
}
