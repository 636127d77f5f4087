// gram_kernels.hpp — Gram matrix of the vectors the tangent sweep holds at a save point (include/rydiff.h: rydiff_forward_geometry):
//   G_ij = <v_i|v_j> = sum_y conj(v_i[y]) v_j[y],   v_0 = psi, v_{1+d} = dpsi_d
// the one reduction the quantum geometric tensor, the quantum Fisher information and the Berry curvature are built from.
// k_tangent_gram<D>   one read of the (1 + D) vectors: every thread walks its amplitudes in a grid-stride loop, loads its amplitude of
//                     all 1 + D vectors before any product consumes one and keeps the upper triangle in registers — (1 + D)^2 doubles:
//                     Re G_ij (i <= j) and Im G_ij (i < j); Im G_ii is never formed.  Block reduction in a FIXED pattern: the wave64
//                     shuffle tree, then the four waves through LDS in wave order; the block's partial goes to the workspace with
//                     ordinary vector stores.  No atomics: F = 4 (G_ii / N - |G_0i|^2 / N^2) subtracts numbers of equal size and is
//                     inverted in natural-gradient solves, so the sums come out in one order and bit for bit the same on every call.
// k_gram_finish       sums the block partials in a fixed tree (lane l takes blocks l, l + 64, ... ascending, then the wave tree) and
//                     writes the FULL Hermitian matrix: the lower triangle is the exact conjugate of the upper one (the same sums in
//                     the same order), Im G_ii is an exact 0.  Every entry of the slice is written.
// Partial layout: [block][B][(1 + D)^2] doubles; slot i * (1 + D) + j holds Re G_ij for i <= j and Im G_ji for i > j.
#pragma once

template <int D>
__global__ __launch_bounds__(256) void k_tangent_gram(const double2* __restrict__ vec /* [1 + D][B][dim] */, size_t vstride,
                                                      double* __restrict__ partial, uint32_t dim) {
    constexpr int NV = 1 + D, NE = NV * NV;
    __shared__ double lds[4][NE];
    const int b = blockIdx.y, B = gridDim.y;
    const double2* __restrict__ v0 = vec + size_t(b) * dim;
    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < dim; x += gridDim.x * 256u) {
        double2 v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = v0[size_t(i) * vstride + x];  // all loads in flight together
        __builtin_amdgcn_sched_barrier(0);  // the scheduler may not sink a later vector's load below the first products
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            acc[i * NV + i] += v[i].x * v[i].x + v[i].y * v[i].y;
#pragma unroll
            for (int j = i + 1; j < NV; ++j) {
                acc[i * NV + j] += v[i].x * v[j].x + v[i].y * v[j].y;  // Re conj(v_i) v_j
                acc[j * NV + i] += v[i].x * v[j].y - v[i].y * v[j].x;  // Im conj(v_i) v_j
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const double s = wave_sum(acc[e]);  // fixed shuffle tree
        if (lane == 0) lds[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < NE) {
        const int e = threadIdx.x;
        partial[(size_t(blockIdx.x) * B + b) * NE + e] = ((lds[0][e] + lds[1][e]) + lds[2][e]) + lds[3][e];
    }
}

// grid (n * n, B), one wave per output entry (i, j): n = 1 + n_dir rows are written, np = 1 + padded width is the partials' stride
__global__ __launch_bounds__(64) void k_gram_finish(const double* __restrict__ partial, int nblocks, int np, int n,
                                                    double2* __restrict__ gram /* &gram_out[k][0][0][0] */) {
    const int b = blockIdx.y, B = gridDim.y;
    const int i = int(blockIdx.x) / n, j = int(blockIdx.x) % n;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const size_t bstride = size_t(B) * np * np;
    const double* __restrict__ pre = partial + size_t(b) * np * np + lo * np + hi;
    const double* __restrict__ pim = partial + size_t(b) * np * np + hi * np + lo;
    double re = 0.0, im = 0.0;
    for (int blk = threadIdx.x; blk < nblocks; blk += 64) {  // ascending, the same trip for every entry
        re += pre[size_t(blk) * bstride];
        if (lo != hi) im += pim[size_t(blk) * bstride];  // uniform
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if (threadIdx.x == 0) gram[(size_t(b) * n + i) * n + j] = make_double2(re, i == j ? 0.0 : (i < j ? im : -im));
}
