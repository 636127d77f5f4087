// moments_kernels.hpp — occupation correlations (include/rydiff.h: RydProblem.bit_moments): the moments of p[y] = |psi[y]|^2 over the
// index bits,
//   S = sum_y p[y],   B_q = sum_y p[y] y_q,   B_qr = sum_y p[y] y_q y_r  (q < r),      qubit q <-> index bit N-1-q
// all 1 + N + N(N-1)/2 of them from ONE read of the state.
// A record (S, f[0..L), P[j<k]) holds the moments of a distribution over L bits.  Two records over the same bits, for the halves where
// a new bit is 0 (lo) and 1 (hi), merge to a record over L + 1 bits (mom_merge); the new bit takes position L, pair (j, k) sits at
// k(k-1)/2 + j, so a merge appends and never moves an entry.  The same rule at every level:
// k_moments_tile     one workgroup reduces one tile of 2^12 amplitudes: thread-local over the 4 bits its 16 amplitudes differ in
//                    (registers), across the 6 lane bits by exchanges with the partner lane (every lane leaves a step with the merged
//                    record), across the 4 waves through LDS.  Up to 12 qubits the tile is the state and the rows go straight to
//                    expect_out; beyond, the tile's 79 doubles go to the workspace ([state][entry][tile], plan.hpp: off_moments).
//                    The body (moments_tile_body) takes the 16 weights of a thread from a loader: MomLoadKet here, MomLoadTangent
//                    below, MomLoadDmDiag for the diagonal of a density matrix (dm_kernels.hpp: k_dm_moments).
// k_moments_tangent  the same body (moments_tile<TAN>) on the signed weight dp[y] = 2 Re(conj psi[y] dpsi_d[y]): the tangent of a moment
//                    of p is that moment of dp.  One direction per grid.z; rows into direction d's Moments block of dexpect_out, or
//                    the tile records into the tangent sweep's region ([D][B][79][tiles], tangent_launch.hpp: off_dmoments).
// k_moments_finish   the rows from the tile records, one wave per row: the tile index is the high bits, so low singles / low-low pairs
//                    are plain sums over the tiles, high singles / high-high pairs bit moments of the tile sums S_tau, high-low pairs
//                    bit moments of f_tau[j].  Lane l takes tiles l, l + 64, ... ascending, then the wave tree.
// k_moments_apply    the cotangent  base + 2 q_k(y) psi_k[y],  q_k(y) = g_S + sum_q g_q y_q + sum_{q<r} g_qr y_q y_r  with the g's read
//                    on the device; per workgroup (uniform) the part of q of the high bits and the low bits' coefficients
//                    c_j(hi) = g_j + sum_{i in hi} g_ij hi_i, per thread the same split once more, per amplitude 4 bits.
// No atomics: every sum has one fixed order, two calls on the same input give the same bits.  Every output entry is written.
#pragma once

constexpr int kMomTileBits = 12;                                          // 256 threads x 16 amplitudes
constexpr int kMomLocalBits = 4;                                          // tile bits 8..11: the amplitudes of one thread
constexpr int kMomEntries = 1 + kMomTileBits + kMomTileBits * (kMomTileBits - 1) / 2;  // 79
constexpr int kMomWaveEntries = 1 + 10 + 45;                              // the record of one wave: 10 bits
static_assert(kMomTileBits == 12 && kMomLocalBits == 4, "k_moments_tile: 4 local + 6 lane + 2 wave bits");

template <int L>
struct MomRec {
    double S;
    double f[L ? L : 1];
    double P[L > 1 ? L * (L - 1) / 2 : 1];
};

template <int L>
__device__ __forceinline__ MomRec<L + 1> mom_merge(const MomRec<L>& lo, const MomRec<L>& hi) {
    MomRec<L + 1> r{};
    r.S = lo.S + hi.S;
#pragma unroll
    for (int j = 0; j < L; ++j) r.f[j] = lo.f[j] + hi.f[j];
    r.f[L] = hi.S;
#pragma unroll
    for (int i = 0; i < L * (L - 1) / 2; ++i) r.P[i] = lo.P[i] + hi.P[i];
#pragma unroll
    for (int j = 0; j < L; ++j) r.P[L * (L - 1) / 2 + j] = hi.f[j];
    return r;
}

// 2^L probabilities p[0 .. 2^L) -> their record; bit j of the position is bit j of the record
template <int L>
__device__ __forceinline__ MomRec<L> mom_local(const double* p) {
    if constexpr (L == 0) {
        MomRec<0> r{};
        r.S = p[0];
        return r;
    } else {
        return mom_merge<L - 1>(mom_local<L - 1>(p), mom_local<L - 1>(p + (1 << (L - 1))));
    }
}

// the merge across lane bit `step`: both partners leave with the same record (a + b == b + a bit for bit)
template <int L>
__device__ __forceinline__ MomRec<L + 1> mom_lane_merge(const MomRec<L>& m, int step) {
    const bool up = ((threadIdx.x >> step) & 1u) != 0u;  // this lane holds the half where the bit is 1
    MomRec<L + 1> r{};
    const double oS = __shfl_xor(m.S, 1 << step, 64);
    r.S = m.S + oS;
    r.f[L] = up ? m.S : oS;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const double o = __shfl_xor(m.f[j], 1 << step, 64);
        r.f[j] = m.f[j] + o;
        r.P[L * (L - 1) / 2 + j] = up ? m.f[j] : o;
    }
#pragma unroll
    for (int i = 0; i < L * (L - 1) / 2; ++i) r.P[i] = m.P[i] + __shfl_xor(m.P[i], 1 << step, 64);
    return r;
}

// record position -> tile bit: 0..3 the thread's amplitudes (tile bits 8..11), 4..9 the lane (0..5), 10..11 the wave (6..7)
__device__ __forceinline__ int mom_tile_bit(int pos) { return pos < kMomLocalBits ? pos + 8 : pos - 4; }

// entry e of a tile record -> how many bits it is a moment of (0: S) and which tile bits
__device__ __forceinline__ int mom_entry_bits(int e, int& ba, int& bb) {
    ba = bb = 0;
    if (e == 0) return 0;
    if (e <= kMomTileBits) {
        ba = mom_tile_bit(e - 1);
        return 1;
    }
    const int idx = e - 1 - kMomTileBits;
    int k = 1;
    while ((k + 1) * k / 2 <= idx) ++k;
    ba = mom_tile_bit(idx - k * (k - 1) / 2);
    bb = mom_tile_bit(k);
    return 2;
}

// the row of the single of index bit ba / of the pair of index bits (ba, bb), ba != bb
__device__ __forceinline__ int mom_row1(int N, int ba) { return 1 + (N - 1 - ba); }
__device__ __forceinline__ int mom_row2(int N, int ba, int bb) {
    const int qa = N - 1 - ba, qb = N - 1 - bb;
    const int q = qa < qb ? qa : qb, r = qa < qb ? qb : qa;
    return 1 + N + q * (2 * N - q - 1) / 2 + (r - q - 1);
}

struct MomentsTileArgs {
    const double2* psi;  // state at save point k0, trajectory 0
    size_t kstride;      // amplitudes between consecutive save points (grid.y covers b_count * n_k states)
    double* out;         // the Moments block of expect_out (ExpectRows, plan.hpp): [1 + N + N(N-1)/2][n_tsave][B]
    double* rec;         // more than one tile: [n_k][B][79][tiles] doubles in the workspace
    int N, n_tsave, k0, B, b_first, b_count;
    uint32_t dim, tiles;
};

// The tile reduction, one body for every weight: `load` fills p[r] with the weight of tile position r * 256 + threadIdx.x (0 past the
// end of the state).  Thread-local over the 4 bits of r, across the 6 lane bits, across the 4 waves through LDS; entry e of the
// tile's record leaves through thread e: to the rows of `out` at (a.k0 + kk, b) when the tile is the state (a.tiles == 1), else to
// `rec` as tile `tau` of state kk * a.B + b.  Of `a` the body reads N, n_tsave, k0, B and tiles.
template <class Loader>
__device__ __forceinline__ void moments_tile_body(const Loader& load, const MomentsTileArgs& a, int b, int kk, uint32_t tau, double* out,
                                                  double* rec) {
    __shared__ double wrec[4][kMomWaveEntries];
    double p[1 << kMomLocalBits];
    load(p);
    const MomRec<4> r4 = mom_local<4>(p);
    const MomRec<5> r5 = mom_lane_merge<4>(r4, 0);
    const MomRec<6> r6 = mom_lane_merge<5>(r5, 1);
    const MomRec<7> r7 = mom_lane_merge<6>(r6, 2);
    const MomRec<8> r8 = mom_lane_merge<7>(r7, 3);
    const MomRec<9> r9 = mom_lane_merge<8>(r8, 4);
    const MomRec<10> w = mom_lane_merge<9>(r9, 5);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        wrec[wave][0] = w.S;
#pragma unroll
        for (int j = 0; j < 10; ++j) wrec[wave][1 + j] = w.f[j];
#pragma unroll
        for (int i = 0; i < 45; ++i) wrec[wave][11 + i] = w.P[i];
    }
    __syncthreads();
    const int e = threadIdx.x;
    if (e >= kMomEntries) return;
    // the merge across the two wave bits (positions 10 and 11): entry e of the tile's record
    auto all4 = [&](int c) { return (wrec[0][c] + wrec[1][c]) + (wrec[2][c] + wrec[3][c]); };
    auto bit10 = [&](int c) { return wrec[1][c] + wrec[3][c]; };
    auto bit11 = [&](int c) { return wrec[2][c] + wrec[3][c]; };
    double val;
    if (e <= 10) val = all4(e);
    else if (e == 11) val = bit10(0);
    else if (e == 12) val = bit11(0);
    else {
        const int idx = e - 13;
        if (idx < 45) val = all4(11 + idx);
        else if (idx < 55) val = bit10(1 + idx - 45);
        else if (idx < 65) val = bit11(1 + idx - 55);
        else val = wrec[3][0];
    }
    const size_t state = size_t(kk) * a.B + b;
    if (a.tiles > 1u) {
        rec[(state * kMomEntries + e) * a.tiles + tau] = val;
        return;
    }
    int ba, bb;
    const int nb = mom_entry_bits(e, ba, bb);
    if (ba >= a.N || bb >= a.N) return;  // a bit the register does not have
    const int row = nb == 0 ? 0 : (nb == 1 ? mom_row1(a.N, ba) : mom_row2(a.N, ba, bb));
    out[(size_t(row) * a.n_tsave + a.k0 + kk) * a.B + b] = val;
}

// the weights of a ket: p = |psi|^2
struct MomLoadKet {
    const double2* __restrict__ psi;  // the tile's first amplitude
    uint32_t left;                    // amplitudes from there to the end of the state (a tile past the state: none)
    __device__ __forceinline__ void operator()(double* p) const {
        double2 v[1 << kMomLocalBits];
#pragma unroll
        for (uint32_t r = 0; r < (1u << kMomLocalBits); ++r) {  // all loads in flight together, consecutive lanes on consecutive amplitudes
            const uint32_t t = r * 256u + threadIdx.x;
            v[r] = t < left ? psi[t] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (uint32_t r = 0; r < (1u << kMomLocalBits); ++r) p[r] = v[r].x * v[r].x + v[r].y * v[r].y;
    }
};

// the signed weights of a tangent: dp = 2 Re(conj psi . dpsi)
struct MomLoadTangent {
    const double2* __restrict__ psi;
    const double2* __restrict__ dpsi;  // laid out like psi
    uint32_t left;
    __device__ __forceinline__ void operator()(double* p) const {
        double2 v[1 << kMomLocalBits], w[1 << kMomLocalBits];
#pragma unroll
        for (uint32_t r = 0; r < (1u << kMomLocalBits); ++r) {
            const uint32_t t = r * 256u + threadIdx.x;
            v[r] = t < left ? psi[t] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (uint32_t r = 0; r < (1u << kMomLocalBits); ++r) {
            const uint32_t t = r * 256u + threadIdx.x;
            w[r] = t < left ? dpsi[t] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (uint32_t r = 0; r < (1u << kMomLocalBits); ++r) p[r] = 2.0 * (v[r].x * w[r].x + v[r].y * w[r].y);
    }
};

// The moments of p = |psi|^2 (TAN = false: k_moments_tile) and their tangents, the same moments of dp (TAN = true:
// k_moments_tangent).  `dvec`: the tangent vector laid out like a.psi (TAN only); `out` / `rec`: where this launch's rows / tile
// records go.
template <bool TAN>
__device__ __forceinline__ void moments_tile(const MomentsTileArgs& a, const double2* dvec, double* out, double* rec) {
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const uint32_t tau = blockIdx.x;
    const size_t first = size_t(kk) * a.kstride + size_t(b) * a.dim + (size_t(tau) << kMomTileBits);
    const uint32_t left = a.dim - (tau << kMomTileBits);
    if constexpr (TAN) moments_tile_body(MomLoadTangent{a.psi + first, dvec + first, left}, a, b, kk, tau, out, rec);
    else moments_tile_body(MomLoadKet{a.psi + first, left}, a, b, kk, tau, out, rec);
}

// grid (tiles, b_count * n_k), 256 threads
__global__ __launch_bounds__(256) void k_moments_tile(MomentsTileArgs a) { moments_tile<false>(a, nullptr, a.out, a.rec); }

struct MomentsTangentArgs {
    MomentsTileArgs t;   // psi: the state of vec = [1 + D][B][dim] (one save point: kstride 0); out / rec: those of direction 0
    size_t vstride;      // amplitudes between the vectors of vec: B * dim
    size_t out_dstride;  // doubles between the directions of dexpect_out: ExpectRows::size()
    size_t rec_dstride;  // doubles between the directions' tile records: B * 79 * tiles
};

// grid (tiles, B, n_dir), 256 threads: direction d = blockIdx.z reads psi and dpsi_d
__global__ __launch_bounds__(256) void k_moments_tangent(MomentsTangentArgs a) {
    const size_t d = blockIdx.z;
    moments_tile<true>(a.t, a.t.psi + (1 + d) * a.vstride, a.t.out + d * a.out_dstride, a.t.rec + d * a.rec_dstride);
}

struct MomentsFinishArgs {
    const double* rec;  // [n_k][B][79][tiles]
    double* out;        // the Moments block of expect_out
    int N, n_tsave, k0, B, b_first, b_count;
    uint32_t tiles;     // 2^(N - 12), at least 2
    size_t rec_dstride, out_dstride;  // tangent records: doubles between the directions (grid.z) of rec / of out; else 0
};

// grid (79 + H + 12 H + H (H - 1) / 2, b_count * n_k, directions or 1), H = N - 12 high bits; one wave per row
__global__ __launch_bounds__(64) void k_moments_finish(MomentsFinishArgs a) {
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const int H = a.N - kMomTileBits;
    int o = blockIdx.x;
    int col, row;
    uint32_t mask = 0u;  // the tiles that count: those with these bits set
    if (o < kMomEntries) {  // the tile record's own entries: sums over every tile
        int ba, bb;
        const int nb = mom_entry_bits(o, ba, bb);
        col = o;
        row = nb == 0 ? 0 : (nb == 1 ? mom_row1(a.N, ba) : mom_row2(a.N, ba, bb));
    } else if ((o -= kMomEntries) < H) {  // high singles: bit moments of S_tau
        col = 0;
        mask = 1u << o;
        row = mom_row1(a.N, kMomTileBits + o);
    } else if ((o -= H) < kMomTileBits * H) {  // high-low pairs: bit moments of f_tau[j]
        const int h = o / kMomTileBits, j = o % kMomTileBits;
        col = 1 + j;
        mask = 1u << h;
        row = mom_row2(a.N, kMomTileBits + h, mom_tile_bit(j));
    } else {  // high-high pairs: bit moments of S_tau
        o -= kMomTileBits * H;
        int h2 = 1;
        while ((h2 + 1) * h2 / 2 <= o) ++h2;
        const int h1 = o - h2 * (h2 - 1) / 2;
        col = 0;
        mask = (1u << h1) | (1u << h2);
        row = mom_row2(a.N, kMomTileBits + h1, kMomTileBits + h2);
    }
    const double* __restrict__ src = a.rec + size_t(blockIdx.z) * a.rec_dstride + ((size_t(kk) * a.B + b) * kMomEntries + col) * a.tiles;
    double s = 0.0;
    for (uint32_t tau = threadIdx.x; tau < a.tiles; tau += 64u)  // ascending, the same trip for every row
        if ((tau & mask) == mask) s += src[tau];
    s = wave_sum(s);
    if (threadIdx.x == 0) a.out[size_t(blockIdx.z) * a.out_dstride + (size_t(row) * a.n_tsave + a.k0 + kk) * a.B + b] = s;
}

struct MomentsApplyArgs {
    const double2* psi;    // trajectory: the state at save point k is psi + index(k) * B * dim, index(k) = entry ? entry[k] : k * kmul
    const int32_t* entry;  // full tape of the one-launch sweeps: tape entry of every save point; else nullptr
    int kmul;              // 0: psi IS the state at the one save point of this launch
    const double2* base;   // [n_k][B][dim]: what the cotangent is added to, or nullptr
    double2* out;          // [n_k][B][dim]; may be `base`
    const double* gexp;    // the Moments block of grad_expect: [1 + N + N(N-1)/2][n_tsave][B]
    int N, n_tsave, k0, B;
    uint32_t dim;
};

// grid (max(dim >> 12, 1), B, n_k), 256 threads: out[kk][b][y] = base[kk][b][y] + 2 q(y) psi_k[b][y],  k = k0 + kk
__global__ __launch_bounds__(256) void k_moments_apply(MomentsApplyArgs a) {
    __shared__ double g2[RYDIFF_MAX_QUBITS * RYDIFF_MAX_QUBITS];  // [ba][bb] over index bits: g of the pair, diagonal: g of the single
    __shared__ double cw[kMomTileBits + 1];                       // c_j(hi) of the tile's bits, then the part of q of the high bits
    const int N = a.N, b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t row = size_t(a.n_tsave) * a.B;
    const double* __restrict__ g = a.gexp + size_t(k) * a.B + b;
    const size_t off = (size_t(blockIdx.z) * a.B + b) * a.dim;
    const uint32_t hi = blockIdx.x << kMomTileBits;
    const double gS = g[0];
    int any = gS != 0.0;
    for (int c = threadIdx.x; c < N * N; c += 256) {
        const int ba = c / N, bb = c % N;
        const double v = g[size_t(ba == bb ? mom_row1(N, ba) : mom_row2(N, ba, bb)) * row];
        g2[c] = v;
        any |= v != 0.0;
    }
    any = __syncthreads_or(any);
    if (!any) {  // (uniform) cotangents usually sit at one or a few save points: nothing but the copy of base
        if (a.base == a.out) return;
#pragma unroll
        for (uint32_t r = 0; r < 16u; ++r) {
            const uint32_t y = hi + r * 256u + threadIdx.x;
            if (y < a.dim) a.out[off + y] = a.base ? a.base[off + y] : make_double2(0.0, 0.0);
        }
        return;
    }
    // once per workgroup: the high bits are the same for all of its amplitudes
    const int nlow = N < kMomTileBits ? N : kMomTileBits;
    if (int(threadIdx.x) < nlow) {
        const int j = threadIdx.x;
        double c = g2[j * N + j];
        for (int i = kMomTileBits; i < N; ++i)
            if (hi >> i & 1u) c += g2[i * N + j];
        cw[j] = c;
    } else if (threadIdx.x == 64) {
        double q = gS;
        for (int i = kMomTileBits; i < N; ++i) {
            if (!(hi >> i & 1u)) continue;
            q += g2[i * N + i];
            for (int i2 = i + 1; i2 < N; ++i2)
                if (hi >> i2 & 1u) q += g2[i * N + i2];
        }
        cw[kMomTileBits] = q;
    }
    __syncthreads();
    // once per thread: tile bits 0..7 are the thread's
    const uint32_t t = threadIdx.x;
    double qt = cw[kMomTileBits];
    double cl[4] = {0.0, 0.0, 0.0, 0.0};  // the coefficients of tile bits 8..11 for this thread
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (8 + j < N) cl[j] = cw[8 + j];
    for (int i = 0; i < 8 && i < N; ++i) {
        if (!(t >> i & 1u)) continue;
        qt += cw[i];
        for (int i2 = i + 1; i2 < 8 && i2 < N; ++i2)
            if (t >> i2 & 1u) qt += g2[i * N + i2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (8 + j < N) cl[j] += g2[i * N + 8 + j];
    }
    double pl[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // pairs among tile bits 8..11: (j1, j2) at j2 (j2 - 1) / 2 + j1
#pragma unroll
    for (int j2 = 1; j2 < 4; ++j2)
#pragma unroll
        for (int j1 = 0; j1 < j2; ++j1)
            if (8 + j2 < N) pl[j2 * (j2 - 1) / 2 + j1] = g2[(8 + j1) * N + 8 + j2];
    const double2* __restrict__ psi = a.psi + size_t(a.entry ? a.entry[k] : k * a.kmul) * (size_t(a.B) * a.dim) + size_t(b) * a.dim;
#pragma unroll
    for (uint32_t r = 0; r < 16u; ++r) {
        const uint32_t y = hi + r * 256u + t;
        if (y >= a.dim) continue;
        double q = qt;
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
            if (!(r >> j2 & 1u)) continue;  // compile time
            q += cl[j2];
#pragma unroll
            for (int j1 = 0; j1 < j2; ++j1)
                if (r >> j1 & 1u) q += pl[j2 * (j2 - 1) / 2 + j1];
        }
        const double2 v = psi[y];
        double2 acc = a.base ? a.base[off + y] : make_double2(0.0, 0.0);
        acc.x = fma(2.0 * q, v.x, acc.x);
        acc.y = fma(2.0 * q, v.y, acc.y);
        a.out[off + y] = acc;
    }
}
