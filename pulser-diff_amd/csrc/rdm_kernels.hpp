// rdm_kernels.hpp — reduced density matrices (include/rydiff.h: RydProblem.n_rdms / rdm_masks):
//   rho_A[a][a'] = sum_e psi[idx(a, e)] conj(psi[idx(a', e)]),   A: m <= 6 qubits, rows Re, Im of entry (a, a') at 2 (a 2^m + a')
// A workgroup stages a TILE of 2^t amplitudes (t = min(N, 12)) in LDS: every setting of the A bits times the 2^(t-m) settings of the
// lowest t-m environment bits.  The staged bit set therefore holds index bits 0 .. p-1 for some p >= t-m, so every global run is
// 2^p >= 64 consecutive amplitudes (1 KiB) at t = 12 wherever A sits.  In LDS the tile is the matrix Psi[a][e], row stride
// 2^(t-m) + 1 amplitudes: rows (lanes that differ in a) start 4 banks apart instead of on one bank.
// k_rdm_expect<M>  rho += Psi Psi^dagger out of LDS, upper triangle only, partial sums in registers over all tiles of the workgroup,
//                  atomics once per state (entry and its mirror image; Im of the diagonal is never touched: it stays the 0.0 of the
//                  memset).  M >= 4: 136 upper-triangle blocks of (2^M / 16)^2 entries, one per thread, e split in three parts that
//                  are combined through LDS; M <= 3: fewer entries than threads, so every thread owns all of them for its share of e
//                  and the block reduces (wave shuffle, LDS, 2 * entries atomics).
// k_rdm_apply      the cotangent  out = base + (M_A (x) 1_E) psi,  M = G + G^dagger built in LDS from grad_expect on the device
//                  (4^m amplitudes, 64 KiB at m = 6, where the tile shrinks to 2^11 so that both fit in 160 KiB); no atomics, may
//                  run in place on `base`, skips a (k, b) whose G is identically zero (uniform over the workgroup).
// ONE PASS PER RDM: the staged bit set depends on A, so the RDMs of a call do not share a staging; each gets its own launch.
// Cost per RDM and state (derived, not measured): one read of the state, 8 * 2^(N+m) flops.
#pragma once

constexpr int kRdmThreads = 512;
constexpr int kRdmTileBits = 12;
constexpr int kRdmMaxBlocks = 256;  // workgroups per state (each loops over its tiles)

// how tile number `blk` is gathered: bit i of the staged index j -> a global index bit, and a bit of a or of e
struct RdmTile {
    uint32_t ybit[kRdmTileBits];
    uint32_t abit[kRdmTileBits];
    uint32_t ebit[kRdmTileBits];
    uint32_t hbit[20];  // bit i of the tile number -> global index bit (N - t <= 19)
    int t, m, nh;
    uint32_t stride;    // 2^(t-m) + 1
};

__device__ __forceinline__ void rdm_spread(const RdmTile& g, uint32_t j, uint32_t& y, uint32_t& a, uint32_t& e) {
    y = a = e = 0u;
    for (int i = 0; i < g.t; ++i)
        if (j >> i & 1u) {
            y |= g.ybit[i];
            a |= g.abit[i];
            e |= g.ebit[i];
        }
}

__device__ __forceinline__ uint32_t rdm_tile_base(const RdmTile& g, uint32_t blk) {
    uint32_t y = 0u;
    for (int i = 0; i < g.nh; ++i)
        if (blk >> i & 1u) y |= g.hbit[i];
    return y;
}

// tile[a * stride + e] = psi[tile base | y(j)]: consecutive lanes on consecutive staged indices j, i.e. on consecutive amplitudes
// within a run (the caller synchronises before and after)
__device__ __forceinline__ void rdm_stage(const RdmTile& g, const double2* __restrict__ psi, uint32_t blk, double2* tile) {
    const uint32_t yb = rdm_tile_base(g, blk), n = 1u << g.t;
    uint32_t ylo, alo, elo;
    rdm_spread(g, threadIdx.x & (kRdmThreads - 1), ylo, alo, elo);
    for (uint32_t j0 = 0; j0 < n; j0 += kRdmThreads) {
        uint32_t yhi, ahi, ehi;
        rdm_spread(g, j0, yhi, ahi, ehi);  // uniform
        if (j0 + threadIdx.x < n) tile[(alo | ahi) * g.stride + (elo | ehi)] = psi[yb | ylo | yhi];
    }
}

struct RdmExpectArgs {
    const double2* psi;  // state at save point k0, trajectory 0
    size_t kstride;      // amplitudes between consecutive save points (grid.y covers b_count * n_k states)
    double* out;         // first row of this RDM in expect_out: [2 * 4^m][n_tsave][B]
    RdmTile g;
    int n_tsave, k0, B, b_first, b_count;
    uint32_t dim, nblocks;
};

// entry (a, a2), a <= a2, and its mirror image
__device__ __forceinline__ void rdm_emit(double* out, size_t row, uint32_t D, uint32_t a, uint32_t a2, double re, double im) {
    unsafeAtomicAdd(out + size_t(2 * (a * D + a2)) * row, re);
    if (a == a2) return;
    unsafeAtomicAdd(out + size_t(2 * (a * D + a2) + 1) * row, im);
    unsafeAtomicAdd(out + size_t(2 * (a2 * D + a)) * row, re);
    unsafeAtomicAdd(out + size_t(2 * (a2 * D + a) + 1) * row, -im);
}

// grid (min(tiles, kRdmMaxBlocks), b_count * n_k); dynamic LDS: the tile, or the reduction scratch where that is larger
template <int M>
__global__ __launch_bounds__(kRdmThreads) void k_rdm_expect(RdmExpectArgs a) {
    extern __shared__ double2 rdm_lds[];
    constexpr uint32_t D = 1u << M;
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const double2* __restrict__ psi = a.psi + size_t(kk) * a.kstride + size_t(b) * a.dim;
    const uint32_t E = 1u << (a.g.t - M), stride = a.g.stride;
    double* out = a.out + size_t(a.k0 + kk) * a.B + b;
    const size_t row = size_t(a.n_tsave) * a.B;
    double* red = reinterpret_cast<double*>(rdm_lds);
    if constexpr (M <= 3) {
        constexpr int NE = int(D * (D + 1) / 2);
        double re[NE], im[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) re[i] = im[i] = 0.0;
        for (uint32_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
            __syncthreads();
            rdm_stage(a.g, psi, blk, rdm_lds);
            __syncthreads();
            for (uint32_t e = threadIdx.x; e < E; e += kRdmThreads) {
                double2 v[D];
#pragma unroll
                for (uint32_t r = 0; r < D; ++r) v[r] = rdm_lds[r * stride + e];
                int i = 0;
#pragma unroll
                for (uint32_t r = 0; r < D; ++r)
#pragma unroll
                    for (uint32_t c = r; c < D; ++c, ++i) {
                        re[i] = fma(v[r].x, v[c].x, fma(v[r].y, v[c].y, re[i]));  // psi[a] conj(psi[a'])
                        im[i] = fma(v[r].y, v[c].x, fma(-v[r].x, v[c].y, im[i]));
                    }
            }
        }
        __syncthreads();  // the tile is done with: its LDS becomes red[wave][2 * NE]
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const double sr = wave_sum(re[i]), si = wave_sum(im[i]);
            if (lane == 0) {
                red[wave * 2 * NE + 2 * i] = sr;
                red[wave * 2 * NE + 2 * i + 1] = si;
            }
        }
        __syncthreads();
        if (threadIdx.x < NE) {
            double sr = 0.0, si = 0.0;
            for (int w = 0; w < kRdmThreads / 64; ++w) {
                sr += red[w * 2 * NE + 2 * threadIdx.x];
                si += red[w * 2 * NE + 2 * threadIdx.x + 1];
            }
            uint32_t r = 0, rem = threadIdx.x;  // upper-triangle entry number -> (r, c)
            while (rem >= D - r) rem -= D - r++;
            rdm_emit(out, row, D, r, r + rem, sr, si);
        }
    } else {
        constexpr int RB = int(D / 16), NP = 136, PARTS = 3;  // 16 x 16 blocks of RB x RB entries; 136 of them on or above the diagonal
        const uint32_t part = threadIdx.x / NP, p = threadIdx.x % NP;  // part 3: no work
        uint32_t bi = 0, rem = p;
        while (rem >= 16u - bi) rem -= 16u - bi++;
        const uint32_t bj = bi + rem;
        double re[RB][RB], im[RB][RB];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int c = 0; c < RB; ++c) re[r][c] = im[r][c] = 0.0;
        const uint32_t e0 = part < PARTS ? E * part / PARTS : 0u, e1 = part < PARTS ? E * (part + 1) / PARTS : 0u;
        for (uint32_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
            __syncthreads();
            rdm_stage(a.g, psi, blk, rdm_lds);
            __syncthreads();
            for (uint32_t e = e0; e < e1; ++e) {
                double2 va[RB], vb[RB];
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    va[r] = rdm_lds[(bi * RB + r) * stride + e];
                    vb[r] = rdm_lds[(bj * RB + r) * stride + e];
                }
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int c = 0; c < RB; ++c) {
                        re[r][c] = fma(va[r].x, vb[c].x, fma(va[r].y, vb[c].y, re[r][c]));
                        im[r][c] = fma(va[r].y, vb[c].x, fma(-va[r].x, vb[c].y, im[r][c]));
                    }
            }
        }
        for (uint32_t q = 1; q < PARTS; ++q) {  // parts 1, 2 -> part 0 through red[p][RB * RB][2]
            __syncthreads();
            if (part == q) {
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int c = 0; c < RB; ++c) {
                        red[(p * RB * RB + r * RB + c) * 2] = re[r][c];
                        red[(p * RB * RB + r * RB + c) * 2 + 1] = im[r][c];
                    }
            }
            __syncthreads();
            if (part == 0) {
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int c = 0; c < RB; ++c) {
                        re[r][c] += red[(p * RB * RB + r * RB + c) * 2];
                        im[r][c] += red[(p * RB * RB + r * RB + c) * 2 + 1];
                    }
            }
        }
        if (part == 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int c = 0; c < RB; ++c) {
                    const uint32_t ar = bi * RB + r, ac = bj * RB + c;
                    if (ar <= ac) rdm_emit(out, row, D, ar, ac, re[r][c], im[r][c]);  // (a diagonal block holds both triangles)
                }
        }
    }
}

struct RdmApplyArgs {
    const double2* psi;    // trajectory: the state at save point k is psi + index(k) * B * dim, index(k) = entry ? entry[k] : k * kmul
    const int32_t* entry;  // full tape of the one-launch sweeps: tape entry of every save point; else nullptr
    int kmul;              // 0: psi IS the state at the one save point of this launch
    const double2* base;   // [n_k][B][dim] from k0 on: what this RDM's cotangent is added to, or nullptr
    double2* out;          // [n_k][B][dim]; may be `base`
    const double* gexp;    // first row of this RDM in grad_expect: [2 * 4^m][n_tsave][B]
    RdmTile g;
    int n_tsave, k0, B;
    uint32_t dim, nblocks;
};

// grid (min(tiles, kRdmMaxBlocks), B, n_k): out[kk][b][y] = base[kk][b][y] + sum_a' M[a(y)][a'] psi_k[y with the A bits set to a'],
// M = G + G^dagger, G[a][a'] = g[2 (a 2^m + a')] + i g[2 (a 2^m + a') + 1] at (k, b), k = k0 + kk.  LDS: M (4^m amplitudes), then the tile.
__global__ __launch_bounds__(kRdmThreads) void k_rdm_apply(RdmApplyArgs a) {
    extern __shared__ double2 rdm_lds[];
    const uint32_t D = 1u << a.g.m, stride = a.g.stride, n = 1u << a.g.t;
    const int b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t sv = size_t(a.B) * a.dim;
    const size_t off = size_t(blockIdx.z) * sv + size_t(b) * a.dim;
    const size_t row = size_t(a.n_tsave) * a.B;
    const double* g = a.gexp + size_t(k) * a.B + b;
    double2* mat = rdm_lds;
    double2* tile = rdm_lds + D * D;
    int nz = 0;
    for (uint32_t i = threadIdx.x; i < D * D; i += kRdmThreads) {
        const uint32_t r = i >> a.g.m, c = i & (D - 1u), it = c * D + r;
        const double gr = g[size_t(2 * i) * row], gi = g[size_t(2 * i + 1) * row];
        const double hr = g[size_t(2 * it) * row], hi = g[size_t(2 * it + 1) * row];
        mat[i] = make_double2(gr + hr, gi - hi);
        nz |= (gr != 0.0 || gi != 0.0) ? 1 : 0;
    }
    if (!__syncthreads_or(nz)) {  // uniform: cotangents usually sit at one or a few save points
        if (a.base == a.out) return;
        for (uint32_t y = blockIdx.x * kRdmThreads + threadIdx.x; y < a.dim; y += gridDim.x * kRdmThreads)
            a.out[off + y] = a.base ? a.base[off + y] : make_double2(0.0, 0.0);
        return;
    }
    const double2* __restrict__ psi = a.psi + size_t(a.entry ? a.entry[k] : k * a.kmul) * sv + size_t(b) * a.dim;
    uint32_t ylo, alo, elo;
    rdm_spread(a.g, threadIdx.x & (kRdmThreads - 1), ylo, alo, elo);
    for (uint32_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        __syncthreads();
        rdm_stage(a.g, psi, blk, tile);
        __syncthreads();
        const uint32_t yb = rdm_tile_base(a.g, blk);
        for (uint32_t j0 = 0; j0 < n; j0 += kRdmThreads) {
            uint32_t yhi, ahi, ehi;
            rdm_spread(a.g, j0, yhi, ahi, ehi);  // uniform
            if (j0 + threadIdx.x >= n) continue;
            const uint32_t r = alo | ahi, e = elo | ehi;
            double ar = 0.0, ai = 0.0;
            for (uint32_t c = 0; c < D; ++c) {
                const double2 m = mat[r * D + c], v = tile[c * stride + e];
                ar = fma(m.x, v.x, fma(-m.y, v.y, ar));
                ai = fma(m.x, v.y, fma(m.y, v.x, ai));
            }
            const size_t at = off + (yb | ylo | yhi);
            if (a.base) {
                const double2 g0 = a.base[at];
                ar += g0.x;
                ai += g0.y;
            }
            a.out[at] = make_double2(ar, ai);
        }
    }
}
