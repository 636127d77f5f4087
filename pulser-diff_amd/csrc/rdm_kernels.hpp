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
// k_rdm_tangent<M> the tangent of rho_A along one direction of the tangent sweep, d rho = dPsi Psi^dagger + Psi dPsi^dagger: the
//                  staging, the M <= 3 / M >= 4 register split, the reduction and the atomics of k_rdm_expect, with a Psi tile and a
//                  dPsi tile side by side in LDS (2 * 66 560 B at m = 6, 2 * 65 568 B at m = 1, of 160 KiB) and the sesquilinear form
//                  in place of the quadratic one.  The direction is grid.z: a third tile (two directions per pass) does not fit in
//                  LDS beside 2^12-amplitude tiles, and at M = 6 one direction already holds 32 accumulator doubles per thread
//                  (138 VGPRs; a second direction's 64 more would pass the 256 of a 512-thread workgroup), so Psi is staged again
//                  for every direction.  35 / 79 / 217 / 34 / 62 / 138 VGPRs at M = 1 .. 6, no scratch; k_rdm_expect<M> keeps its
//                  34 / 62 / 182 / 26 / 52 / 114.
// ONE PASS PER RDM: the staged bit set depends on A, so the RDMs of a call do not share a staging; each gets its own launch.
// Cost per RDM and state (derived, not measured): one read of the state, 8 * 2^(N+m) flops.  k_rdm_tangent, per RDM, save point,
// trajectory and direction: two reads of 2^N amplitudes (Psi and dPsi_d: 2 D state reads for D directions), 16 * 2^(N+m) flops.
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

// one (a, a', e) term of entry (a, a'): p = Psi[a][e], q = Psi[a'][e]; tangent: dp, dq the same entries of dPsi
//   value    p conj(q)                 tangent    dp conj(q) + p conj(dq)
template <bool TAN>
__device__ __forceinline__ void rdm_form(double& re, double& im, double2 p, double2 q, double2 dp, double2 dq) {
    if constexpr (TAN) {
        re = fma(dp.x, q.x, fma(dp.y, q.y, fma(p.x, dq.x, fma(p.y, dq.y, re))));
        im = fma(dp.y, q.x, fma(-dp.x, q.y, fma(p.y, dq.x, fma(-p.x, dq.y, im))));
    } else {
        re = fma(p.x, q.x, fma(p.y, q.y, re));  // psi[a] conj(psi[a'])
        im = fma(p.y, q.x, fma(-p.x, q.y, im));
    }
}

// What k_rdm_expect<M> and k_rdm_tangent<M> share: the tiles of this workgroup staged one after the other, the upper triangle summed
// in registers, one round of atomics into out[2 (a 2^M + a') (+ 1)][row].  TAN: dpsi is staged behind psi's tile and the form is the
// sesquilinear one.  Dynamic LDS: the tile(s), or the reduction scratch where that is larger.
template <int M, bool TAN>
__device__ __forceinline__ void rdm_accumulate(const RdmTile& g, const double2* __restrict__ psi, const double2* __restrict__ dpsi,
                                               uint32_t nblocks, double* out, size_t row) {
    extern __shared__ double2 rdm_lds[];
    constexpr uint32_t D = 1u << M;
    const uint32_t E = 1u << (g.t - M), stride = g.stride;
    const double2* dtile = rdm_lds + D * stride;  // (TAN only)
    double* red = reinterpret_cast<double*>(rdm_lds);
    if constexpr (M <= 3) {
        constexpr int NE = int(D * (D + 1) / 2);
        double re[NE], im[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) re[i] = im[i] = 0.0;
        for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
            __syncthreads();
            rdm_stage(g, psi, blk, rdm_lds);
            if constexpr (TAN) rdm_stage(g, dpsi, blk, rdm_lds + D * stride);
            __syncthreads();
            for (uint32_t e = threadIdx.x; e < E; e += kRdmThreads) {
                double2 v[D], w[D];
#pragma unroll
                for (uint32_t r = 0; r < D; ++r) {
                    v[r] = rdm_lds[r * stride + e];
                    w[r] = TAN ? dtile[r * stride + e] : v[r];
                }
                int i = 0;
#pragma unroll
                for (uint32_t r = 0; r < D; ++r)
#pragma unroll
                    for (uint32_t c = r; c < D; ++c, ++i) rdm_form<TAN>(re[i], im[i], v[r], v[c], w[r], w[c]);
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
        for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
            __syncthreads();
            rdm_stage(g, psi, blk, rdm_lds);
            if constexpr (TAN) rdm_stage(g, dpsi, blk, rdm_lds + D * stride);
            __syncthreads();
            for (uint32_t e = e0; e < e1; ++e) {
                double2 va[RB], vb[RB], wa[RB], wb[RB];
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    va[r] = rdm_lds[(bi * RB + r) * stride + e];
                    vb[r] = rdm_lds[(bj * RB + r) * stride + e];
                    wa[r] = TAN ? dtile[(bi * RB + r) * stride + e] : va[r];
                    wb[r] = TAN ? dtile[(bj * RB + r) * stride + e] : vb[r];
                }
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int c = 0; c < RB; ++c) rdm_form<TAN>(re[r][c], im[r][c], va[r], vb[c], wa[r], wb[c]);
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

// grid (min(tiles, kRdmMaxBlocks), b_count * n_k); dynamic LDS: the tile, or the reduction scratch where that is larger
template <int M>
__global__ __launch_bounds__(kRdmThreads) void k_rdm_expect(RdmExpectArgs a) {
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    rdm_accumulate<M, false>(a.g, a.psi + size_t(kk) * a.kstride + size_t(b) * a.dim, nullptr, a.nblocks,
                             a.out + size_t(a.k0 + kk) * a.B + b, size_t(a.n_tsave) * a.B);
}

struct RdmTangentArgs {
    const double2* vec;  // [1 + n_dir][B][dim] at one save point: the state, then the tangent of every direction
    size_t vstride;      // B * dim
    double* out;         // first row of this RDM in direction 0's block of dexpect_out: [2 * 4^m][n_tsave][B]
    size_t out_dstride;  // doubles between the blocks of consecutive directions
    RdmTile g;
    int n_tsave, k, B;
    uint32_t dim, nblocks;
};

// grid (min(tiles, kRdmMaxBlocks), B, n_dir); dynamic LDS: two tiles (rdm_launch.hpp: rdm_tangent_lds).  Adds into rows the
// library has zeroed; Im of the diagonal is never touched.
template <int M>
__global__ __launch_bounds__(kRdmThreads) void k_rdm_tangent(RdmTangentArgs a) {
    const int b = blockIdx.y, d = blockIdx.z;
    const double2* psi = a.vec + size_t(b) * a.dim;
    rdm_accumulate<M, true>(a.g, psi, psi + size_t(1 + d) * a.vstride, a.nblocks,
                            a.out + size_t(d) * a.out_dstride + size_t(a.k) * a.B + b, size_t(a.n_tsave) * a.B);
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
