// dm_kernels.hpp — density-matrix observables (include/rydiff.h: RydProblem.dm_*): functionals of v = vec(rho), rho the state of
// the doubled register of a master-equation run, v[x * 2^n + y] = rho[x][y]  (gfx950, wave64):
//   k_dm_trace      diagonal rows  sum_x o[x] Re v[x (2^n + 1)]  and Pauli rows  sum_s w_s Re Tr(P_s rho): per flip mask xm the 2^n
//                   entries (x ^ xm, x) and nothing else — 2^n * 16 B against 4^n * 16 B for the matrix; one row per grid.z
//   k_dm_fidelity   <phi_o|rho|phi_o> for every target and the purity sum |v|^2 from ONE read of v: consecutive lanes on consecutive
//                   y (rows of rho are contiguous: 16-byte loads), phi re-read from cache (2^n <= 4096 entries), the accumulators in
//                   registers (NO = compile-time bound on the targets, as in k_overlap_expect)
//   k_dm_purity_tangent  2 Re sum conj(v) dv_d: the tangent of the purity in the forward-mode sweep (the rows above are linear in v:
//                   their tangents are the same kernels on dv_d)
//   k_dm_shots      one workgroup per trajectory of a sampled save point: the clamped diagonal p[x] = max(Re v[x (2^n + 1)], 0)
//                   into LDS, a fixed-order float64 prefix (segment sums, one serial scan of the 256 totals), one binary search per
//                   shot — no float atomics: bit-reproducible
//   k_dm_apply      cotangent, dense parts:  out = base + sum_o g_o phi_o[x] conj(phi_o[y]) + 2 g_p v   (streaming, no atomics)
//   k_dm_scatter    cotangent, sparse parts, in place behind k_dm_apply: one thread per (distinct flip mask, x) adds
//                   sum_o g_o o[x] (xm = 0) + sum_s g w_s conj(phase_s(x)) at entry (x ^ xm, x) — one owner per entry, no atomics
//   k_dm_rdm        reduced density matrices  rho_o[a][a'] = sum_e v[idx(a, e) 2^n + idx(a', e)]: a block owns ONE row a of ONE RDM of
//                   ONE state; thread <-> (a' = tid mod 2^m, e-slice = tid / 2^m), the slice sums in registers, added in a fixed order
//                   through LDS — one owner per output, plain stores, no atomics: bit-reproducible.  2^(n+m) entries per RDM and state
//   k_dm_rdm_scatter  cotangent of ONE RDM, in place behind k_dm_apply / k_dm_scatter (one launch per RDM, stream-ordered: two RDMs, or an
//                   RDM and a Pauli row, may own the same entry): thread (a, y) adds G[a][ext_A(y)] at entry (dep_A(a) | (y & E), y)
//   k_dm_moments    occupation correlations of the diagonal (RydProblem.dm_moments): S, B_q, B_qr of p[x] = Re v[x (2^n + 1)], NOT clamped
//                   (the rows are linear in rho).  2^n <= 2^12: the diagonal is one tile of moments_kernels.hpp — one workgroup per
//                   state gathers it (real parts only, 2^n * 8 B) and runs moments_tile_body: fixed order, no atomics, plain stores
//   k_dm_moments_scatter  their cotangent, in place behind everything above (the diagonal is also owned by the dm_diag rows, the
//                   xm = 0 strings and the RDMs: stream order): thread x adds q(x) = g_S + sum_q g_q x_q + sum_{q<r} g_qr x_q x_r to
//                   Re of entry (x, x)
// The final sums of the first two follow the other observable kernels: wave shuffle, LDS, one atomic per block and row.
#pragma once

struct DmTables {
    const int32_t* gfirst = nullptr;        // [n_dm_pobs + 1]: groups of observable o
    const PauliGroup* groups = nullptr;     // per observable, by flip mask (atom-index bits)
    const PauliString* strings = nullptr;
    const PauliGroup* agroups = nullptr;    // all observables, by flip mask: the cotangent scatter (pad of a string = its observable)
    const PauliString* astrings = nullptr;
};

struct DmTraceArgs {
    const double2* v;    // state at save point k0, trajectory 0
    size_t kstride;      // amplitudes between consecutive save points (grid.y covers b_count * n_k states)
    DmTables t;
    const double* diag;  // [n_diag][2^n]
    double* out;         // first density-matrix row of expect_out: [n_diag + n_pobs][n_tsave][B]
    int n_diag, n_tsave, k0, B, b_first, b_count, n;
};

// grid (blocks, b_count * n_k, n_diag + n_pobs)
__global__ __launch_bounds__(256) void k_dm_trace(DmTraceArgs a) {
    __shared__ double lds[8];
    const uint32_t D = 1u << a.n;
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const int row = blockIdx.z;
    const double2* __restrict__ v = a.v + size_t(kk) * a.kstride + (size_t(b) << (2 * a.n));
    double acc = 0.0;
    if (row < a.n_diag) {
        const double* __restrict__ o = a.diag + (size_t(row) << a.n);
        for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < D; x += gridDim.x * 256u) acc = fma(o[x], v[size_t(x) * (D + 1u)].x, acc);
    } else {
        const int ob = row - a.n_diag;
        for (int g = a.t.gfirst[ob]; g < a.t.gfirst[ob + 1]; ++g) {  // uniform
            const PauliGroup gr = a.t.groups[g];
            for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < D; x += gridDim.x * 256u) {
                const uint32_t xp = x ^ gr.xm;
                const double2 q = v[(size_t(xp) << a.n) + x];  // rho[x ^ xm][x]
                for (uint32_t s = gr.first; s < gr.first + gr.count; ++s) {
                    const PauliString st = a.t.strings[s];
                    const double val = st.wr * q.x - st.wi * q.y;  // Re(w i^ny q)
                    acc += (__popc(xp & st.zm) & 1u) ? -val : val;
                }
            }
        }
    }
    block_atomic_add(acc, a.out + (size_t(row) * a.n_tsave + a.k0 + kk) * a.B + b, lds);
}

struct DmFidArgs {
    const double2* v;    // state at save point k0, trajectory 0
    size_t kstride;
    const double2* phi;  // [n_fid][fid_batch][2^n]
    double* out;         // first fidelity row of expect_out: [n_fid + purity][n_tsave][B]
    int n_fid, fid_batch, purity, n_tsave, k0, B, b_first, b_count, n;
};

// grid (blocks, b_count * n_k)
template <int NO>
__global__ __launch_bounds__(256) void k_dm_fidelity(DmFidArgs a) {
    __shared__ double lds[8];
    const uint32_t D = 1u << a.n, total = 1u << (2 * a.n);
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const double2* __restrict__ v = a.v + size_t(kk) * a.kstride + size_t(b) * total;
    const double2* __restrict__ phi = a.phi + (a.fid_batch > 1 ? size_t(b) * D : size_t(0));
    const size_t ostride = size_t(a.fid_batch) * D;
    double f[NO], pur = 0.0;
#pragma unroll
    for (int o = 0; o < NO; ++o) f[o] = 0.0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const double2 q = v[i];
        const uint32_t x = i >> a.n, y = i & (D - 1u);
        pur = fma(q.x, q.x, fma(q.y, q.y, pur));
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (o < a.n_fid) {  // uniform
                const double2 px = phi[size_t(o) * ostride + x], py = phi[size_t(o) * ostride + y];
                const double wr = q.x * py.x - q.y * py.y, wi = q.x * py.y + q.y * py.x;  // rho[x][y] phi[y]
                f[o] = fma(px.x, wr, fma(px.y, wi, f[o]));                               // Re(conj(phi[x]) ...)
            }
        }
    }
    double* out = a.out + size_t(a.k0 + kk) * a.B + b;
    const size_t row = size_t(a.n_tsave) * a.B;
#pragma unroll
    for (int o = 0; o < NO; ++o)
        if (o < a.n_fid) block_atomic_add(f[o], out + size_t(o) * row, lds);
    if (a.purity) block_atomic_add(pur, out + size_t(a.n_fid) * row, lds);
}

struct DmPurityTangentArgs {
    const double2* v;    // vec(rho) at the save point, trajectory 0
    const double2* dv;   // tangent 0 there
    size_t vstride;      // amplitudes between consecutive tangents
    double* out;         // &dexpect_out[0][purity row][0][0]
    size_t out_dstride;  // doubles between directions
    int k, B;
    uint32_t total;      // 4^n
};

// grid (blocks, B, n_dir): out[d][k][b] += 2 Re sum_i conj(v_i) dv_d,i — the tangent of the purity sum |v|^2 (tangent sweep)
__global__ __launch_bounds__(256) void k_dm_purity_tangent(DmPurityTangentArgs a) {
    __shared__ double lds[8];
    const int b = blockIdx.y, d = blockIdx.z;
    const double2* __restrict__ v = a.v + size_t(b) * a.total;
    const double2* __restrict__ w = a.dv + size_t(d) * a.vstride + size_t(b) * a.total;
    double acc = 0.0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.total; i += gridDim.x * 256u) {
        const double2 q = v[i], t = w[i];
        acc = fma(q.x, t.x, fma(q.y, t.y, acc));
    }
    block_atomic_add(2.0 * acc, a.out + size_t(d) * a.out_dstride + size_t(a.k) * a.B + b, lds);
}

constexpr uint32_t kDmShotMax =1u << RYDIFF_MAX_DM_ATOMS;  // probabilities of one density matrix: 32 KiB of LDS

struct DmShotArgs {
    const double2* v;  // the sampled state, trajectory 0
    const double* u;   // [B][n_shots] of this sampled save point
    uint32_t* out;     // [B][n_shots]
    int n, n_shots, b_first;
};

// grid (b_count), 256 threads.  Thread t owns a contiguous segment of the diagonal; the segment totals are scanned serially by thread
// 0, so the last entry of a segment and the offset of the next one are the same number: C is non-decreasing, and C[x] > C[x - 1]
// only where p[x] > 0.
__global__ __launch_bounds__(256) void k_dm_shots(DmShotArgs a) {
    __shared__ double C[kDmShotMax];
    __shared__ double part[256];
    __shared__ int last_pos;
    const uint32_t D = 1u << a.n;
    const int b = a.b_first + int(blockIdx.x);
    const double2* __restrict__ v = a.v + (size_t(b) << (2 * a.n));
    const uint32_t seg = (D + 255u) / 256u;
    const uint32_t lo = min(threadIdx.x * seg, D), hi = min(lo + seg, D);
    double run = 0.0;
    int mine = -1;
    for (uint32_t x = lo; x < hi; ++x) {
        const double re = v[size_t(x) * (D + 1u)].x;
        const double p = re > 0.0 ? re : 0.0;  // (NaN counts as 0)
        run += p;
        C[x] = run;
        if (p > 0.0) mine = int(x);
    }
    part[threadIdx.x] = run;
    if (threadIdx.x == 0) last_pos = -1;
    __syncthreads();
    if (mine >= 0) atomicMax(&last_pos, mine);  // (integer: order does not matter)
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int w = 0; w < 256; ++w) {
            const double t = part[w];
            part[w] = acc;
            acc += t;
        }
    }
    __syncthreads();
    const double off = part[threadIdx.x];
    for (uint32_t x = lo; x < hi; ++x) C[x] = off + C[x];
    __syncthreads();
    const double S = C[D - 1u];
    const int last = last_pos;
    for (int s = threadIdx.x; s < a.n_shots; s += 256) {
        const size_t slot = size_t(b) * a.n_shots + s;
        if (!(S > 0.0) || last < 0) {  // nothing to sample from
            a.out[slot] = RYDIFF_SHOT_NONE;
            continue;
        }
        double u = a.u[slot];
        u = u > 0.0 ? fmin(u, 1.0 - 0x1p-53) : 0.0;  // [0, 1); NaN -> 0
        const double tau = u * S;
        uint32_t l = 0, h = D;  // the smallest x with C[x] > tau
        while (l < h) {
            const uint32_t mid = l + (h - l) / 2;
            if (C[mid] > tau) h = mid;
            else l = mid + 1;
        }
        a.out[slot] = l < D ? l : uint32_t(last);  // rounding left no cumulative value above the target: the last populated entry
    }
}

struct DmApplyArgs {
    const double2* psi;    // trajectory: the state at save point k is psi + index(k) * B * 4^n, index(k) = entry ? entry[k] : k * kmul
    const int32_t* entry;
    int kmul;
    const double2* base;   // [n_k][B][4^n]: what the cotangent is added to, or nullptr
    double2* out;          // [n_k][B][4^n]; may be `base`
    const double2* phi;    // [n_fid][fid_batch][2^n]
    const double* g_fid;   // fidelity rows of grad_expect: [n_fid][n_tsave][B]
    const double* g_pur;   // the purity row of grad_expect [n_tsave][B], or nullptr
    int n_fid, fid_batch, n_tsave, k0, B, n;
};

// grid (4^n / 256, B, n_k): out[kk][b][x 2^n + y] = base[kk][b][..] + sum_o g_o phi_o[x] conj(phi_o[y]) + 2 g_p v_k[..],  k = k0 + kk
__global__ __launch_bounds__(256) void k_dm_apply(DmApplyArgs a) {
    const uint32_t D = 1u << a.n, total = 1u << (2 * a.n);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t sv = size_t(a.B) * total;
    const size_t off = size_t(blockIdx.z) * sv + size_t(b) * total + i;
    const uint32_t x = i >> a.n, y = i & (D - 1u);
    double2 acc = a.base ? a.base[off] : make_double2(0.0, 0.0);
    const double* g = a.g_fid + size_t(k) * a.B + b;
    const size_t row = size_t(a.n_tsave) * a.B;
    const double2* phi = a.phi + (a.fid_batch > 1 ? size_t(b) * D : size_t(0));
    const size_t ostride = size_t(a.fid_batch) * D;
    for (int o = 0; o < a.n_fid; ++o) {
        const double go = g[size_t(o) * row];
        if (go == 0.0) continue;  // uniform: cotangents usually sit at one or a few save points
        const double2 px = phi[size_t(o) * ostride + x], py = phi[size_t(o) * ostride + y];
        acc.x = fma(go, px.x * py.x + px.y * py.y, acc.x);  // phi[x] conj(phi[y])
        acc.y = fma(go, px.y * py.x - px.x * py.y, acc.y);
    }
    const double gp = a.g_pur ? a.g_pur[size_t(k) * a.B + b] : 0.0;
    if (gp != 0.0) {  // uniform
        const double2 q = a.psi[size_t(a.entry ? a.entry[k] : k * a.kmul) * sv + size_t(b) * total + i];
        acc.x = fma(2.0 * gp, q.x, acc.x);
        acc.y = fma(2.0 * gp, q.y, acc.y);
    }
    a.out[off] = acc;
}

struct DmScatterArgs {
    double2* out;        // [n_k][B][4^n], already holding everything else
    DmTables t;
    const double* diag;  // [n_diag][2^n]
    const double* gexp;  // first density-matrix row of grad_expect: [n_diag + n_pobs][n_tsave][B]
    int n_diag, n_tsave, k0, B, n;
    uint32_t xblocks;    // blocks per group
};

// grid (xblocks * groups, B, n_k): thread (group, x) owns entry (x ^ xm, x) — distinct groups have distinct masks
__global__ __launch_bounds__(256) void k_dm_scatter(DmScatterArgs a) {
    const uint32_t D = 1u << a.n;
    const uint32_t gi = blockIdx.x / a.xblocks;
    const uint32_t x = (blockIdx.x % a.xblocks) * 256u + threadIdx.x;
    if (x >= D) return;
    const int b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t row = size_t(a.n_tsave) * a.B;
    const double* g = a.gexp + size_t(k) * a.B + b;
    const PauliGroup gr = a.t.agroups[gi];
    const uint32_t xp = x ^ gr.xm;
    double sr = 0.0, si = 0.0;
    if (gr.xm == 0u)
        for (int o = 0; o < a.n_diag; ++o) {
            const double go = g[size_t(o) * row];
            if (go != 0.0) sr = fma(go, a.diag[(size_t(o) << a.n) + x], sr);
        }
    for (uint32_t s = gr.first; s < gr.first + gr.count; ++s) {
        const PauliString st = a.t.astrings[s];
        const double go = g[size_t(a.n_diag + int(st.pad)) * row];
        if (go == 0.0) continue;
        const bool neg = (__popc(xp & st.zm) & 1u) != 0u;
        sr += neg ? -go * st.wr : go * st.wr;   // g w conj(i^ny (-1)^...)
        si += neg ? go * st.wi : -go * st.wi;
    }
    if (sr == 0.0 && si == 0.0) return;
    double2* dst = a.out + (size_t(blockIdx.z) * a.B + b) * (size_t(D) << a.n) + (size_t(xp) << a.n) + x;
    const double2 cur = *dst;
    *dst = make_double2(cur.x + sr, cur.y + si);
}

// the low bits of `val` deposited into the set bits of `mask`, lowest first (pdep) / the bits of `x` under `mask` gathered (pext)
__device__ __forceinline__ uint32_t dm_deposit(uint32_t val, uint32_t mask) {
    uint32_t r = 0u;
    for (; mask; mask &= mask - 1u, val >>= 1) r |= (val & 1u) ? (mask & (0u - mask)) : 0u;
    return r;
}
__device__ __forceinline__ uint32_t dm_extract(uint32_t x, uint32_t mask) {
    uint32_t r = 0u, bit = 1u;
    for (; mask; mask &= mask - 1u, bit <<= 1) r |= (x & mask & (0u - mask)) ? bit : 0u;
    return r;
}

struct DmRdmArgs {
    const double2* v;    // state at save point k0, trajectory 0
    size_t kstride;
    double* out;         // first RDM row of expect_out
    int n_tsave, k0, B, b_first, b_count, n;
    uint32_t am[RYDIFF_MAX_RDMS];  // atoms of A as bits of an atom index
    int32_t m[RYDIFF_MAX_RDMS], row[RYDIFF_MAX_RDMS];  // atoms kept; first row (relative to `out`)
};

// grid (2^m_max, b_count * n_k, n_dm_rdms), 256 threads.  Consecutive lanes are consecutive a': the trailing atoms of A, the only
// contiguous runs of the access set, fall on consecutive lanes.  Slice s of the settings of E = the settings whose lowest
// log2(256 / 2^m) E-bits spell s; a thread walks the remaining E-bits with a masked increment.
__global__ __launch_bounds__(256) void k_dm_rdm(DmRdmArgs a) {
    __shared__ double2 part[256];
    const int o = blockIdx.z, m = a.m[o];
    if (blockIdx.x >= (1u << m)) return;  // (uniform)
    const uint32_t D = 1u << a.n, am = a.am[o], em = (D - 1u) & ~am;
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const double2* __restrict__ v = a.v + size_t(kk) * a.kstride + (size_t(b) << (2 * a.n));
    const uint32_t ap = threadIdx.x & ((1u << m) - 1u), s = threadIdx.x >> m;
    const int sbits = min(8 - m, a.n - m);  // E-bits spelled by the slice number
    uint32_t elo = 0u, rest = em;           // the lowest `sbits` bits of em / the others
    for (int i = 0; i < sbits; ++i) {
        elo |= rest & (0u - rest);
        rest &= rest - 1u;
    }
    double2 acc = make_double2(0.0, 0.0);
    if (s < (1u << sbits)) {
        const size_t rowbase = size_t(dm_deposit(blockIdx.x, am) | dm_deposit(s, elo)) << a.n;
        const uint32_t colbase = dm_deposit(ap, am) | dm_deposit(s, elo);
        uint32_t e = 0u;
        do {  // every subset of `rest`, ascending
            const double2 q = v[rowbase + (size_t(e) << a.n) + (colbase | e)];
            acc.x += q.x;
            acc.y += q.y;
            e = ((e | ~rest) + 1u) & rest;
        } while (e != 0u);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < (1u << m)) {
        double2 sum = part[threadIdx.x];
        for (uint32_t t = 1; t < (256u >> m); ++t) {  // fixed order
            const double2 q = part[(t << m) + threadIdx.x];
            sum.x += q.x;
            sum.y += q.y;
        }
        const size_t rstride = size_t(a.n_tsave) * a.B;
        double* dst = a.out + (size_t(a.row[o]) + 2u * ((size_t(blockIdx.x) << m) + threadIdx.x)) * rstride + size_t(a.k0 + kk) * a.B + b;
        dst[0] = sum.x;
        dst[rstride] = sum.y;
    }
}

struct DmRdmScatterArgs {
    double2* out;        // [n_k][B][4^n], already holding everything else
    const double* gexp;  // first row of this RDM in grad_expect: [2 * 4^m][n_tsave][B]
    int n_tsave, k0, B, n, m;
    uint32_t am;
};

// grid (2^(n+m) / 256, B, n_k): thread (a, y) owns entry (dep_A(a) | (y & E), y) — distinct (a, y) give distinct entries
__global__ __launch_bounds__(256) void k_dm_rdm_scatter(DmRdmScatterArgs a) {
    const uint32_t D = 1u << a.n;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (D << a.m)) return;
    const uint32_t y = t & (D - 1u), ar = t >> a.n;
    const int b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t rstride = size_t(a.n_tsave) * a.B;
    const double* g = a.gexp + 2u * ((size_t(ar) << a.m) + dm_extract(y, a.am)) * rstride + size_t(k) * a.B + b;
    const double gr = g[0], gi = g[rstride];
    if (gr == 0.0 && gi == 0.0) return;
    const uint32_t x = dm_deposit(ar, a.am) | (y & ~a.am);
    double2* dst = a.out + (size_t(blockIdx.z) * a.B + b) * (size_t(D) << a.n) + (size_t(x) << a.n) + y;
    const double2 cur = *dst;
    *dst = make_double2(cur.x + gr, cur.y + gi);
}

struct DmMomentsArgs {
    const double2* v;    // state at save point k0, trajectory 0
    size_t kstride;
    double* out;         // the DmMoments block of expect_out: [1 + n + n(n-1)/2][n_tsave][B]
    int n_tsave, k0, B, b_first, b_count, n;
};

// the weights of a density matrix: the real parts of its diagonal, as they are (no clamp: the rows are linear in rho)
struct MomLoadDmDiag {
    const double2* __restrict__ v;  // vec(rho) of this state
    uint32_t D;                     // 2^n <= 2^kMomTileBits: positions past D hold 0
    __device__ __forceinline__ void operator()(double* p) const {
#pragma unroll
        for (uint32_t r = 0; r < (1u << kMomLocalBits); ++r) {  // all loads in flight together
            const uint32_t x = r * 256u + threadIdx.x;
            p[r] = x < D ? v[size_t(x) * (size_t(D) + 1u)].x : 0.0;
        }
    }
};

// grid (1, b_count * n_k), 256 threads: the diagonal is one tile, the rows go straight to expect_out
static_assert(RYDIFF_MAX_DM_ATOMS <= kMomTileBits, "k_dm_moments: the diagonal of rho must fit one tile");
__global__ __launch_bounds__(256) void k_dm_moments(DmMomentsArgs a) {
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const double2* v = a.v + size_t(kk) * a.kstride + (size_t(b) << (2 * a.n));
    MomentsTileArgs t{};  // what the body reads: the diagonal is a "register" of n bits in one tile
    t.N = a.n;
    t.n_tsave = a.n_tsave;
    t.k0 = a.k0;
    t.B = a.B;
    t.tiles = 1u;
    moments_tile_body(MomLoadDmDiag{v, 1u << a.n}, t, b, kk, 0u, a.out, nullptr);
}

struct DmMomentsScatterArgs {
    double2* out;        // [n_k][B][4^n], already holding everything else
    const double* gexp;  // the DmMoments block of grad_expect: [1 + n + n(n-1)/2][n_tsave][B]
    int n_tsave, k0, B, n;
};

// grid (max(2^n / 256, 1), B, n_k), 256 threads: thread x owns entry (x, x); atom q <-> bit n-1-q of x
__global__ __launch_bounds__(256) void k_dm_moments_scatter(DmMomentsScatterArgs a) {
    __shared__ double g2[RYDIFF_MAX_DM_ATOMS * RYDIFF_MAX_DM_ATOMS];  // [ba][bb] over index bits: g of the pair, diagonal: g of the single
    const int n = a.n, b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const uint32_t D = 1u << n;
    const size_t row = size_t(a.n_tsave) * a.B;
    const double* __restrict__ g = a.gexp + size_t(k) * a.B + b;
    const double gS = g[0];
    int any = gS != 0.0;
    for (int c = threadIdx.x; c < n * n; c += 256) {
        const int ba = c / n, bb = c % n;
        const double val = g[size_t(ba == bb ? mom_row1(n, ba) : mom_row2(n, ba, bb)) * row];
        g2[c] = val;
        any |= val != 0.0;
    }
    any = __syncthreads_or(any);
    if (!any) return;  // (uniform) cotangents usually sit at one or a few save points
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= D) return;
    double q = gS;
    for (int i = 0; i < n; ++i) {
        if (!(x >> i & 1u)) continue;
        q += g2[i * n + i];
        for (int i2 = i + 1; i2 < n; ++i2)
            if (x >> i2 & 1u) q += g2[i * n + i2];
    }
    double2* dst = a.out + (size_t(blockIdx.z) * a.B + b) * (size_t(D) << n) + size_t(x) * (size_t(D) + 1u);
    dst->x += q;
}
