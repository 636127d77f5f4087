// energy_kernels.hpp — energy observables (RydProblem.energy_rows, include/rydiff.h): E = Re<psi|H_k|psi> and M2 = |H_k psi|^2 at
// every save point, and their cotangent.  H_k is the Hamiltonian of the factor passes built from the coefficient record of save
// point k (k_expand_coeffs on column k of energy_amp / energy_det: record = c_re[ga], c_im[ga], dcoef[gd]).
//
// One body, energy_h, called three ways.  One amplitude per thread, partners from global memory, as k_dot_hx: the own value, the
// diagonal (diag_value), the partner sums per drive group (xy_group_sums) and, with xy_mode = 1, the exchange stencil (xy_stencil).
//   forward   k_energy_expect   accumulate conj(psi) h and |h|^2; one pair of partial sums per workgroup, k_energy_finish adds them
//                               in index order (no atomics: bit-reproducible rows)
//   backward  k_energy_bwd1     z = g_E psi + g_M h  into the scratch state; with y = g_E psi + 2 g_M h the local contractions
//                               Re(conj(y) psi) n_g(x) (detuning groups) and Re(conj(y) psi) into wtot (u_pairs)
//             k_energy_bwd2     out = base + 2 H_k z
// The contractions whose operator moves amplitudes (drive groups, exchange pairs) need y at the own index and psi at the partners',
// and y is known only when the body is through.  They are taken with the Hermitian operator on the other side,
//   Re<y| dH/dc |psi> = Re<psi| dH/dc |y> = 2 Re<psi| dH/dc |z> - g_E Re<psi| dH/dc |psi>          (y = 2 z - g_E psi)
// the second term in pass 1 (partner sums of psi, own psi), the first in pass 2 (partner sums of z, own psi).  dH/dRe c, dH/dIm c and
// dH/dJ_p are Hermitian: conditioned flips and the one-directional exchange are refused with the block.
// Gradient records [Bc][n_tsave][kEnergyReplicas][NC] take one atomic per value and workgroup (the replica scheme of the adjoint
// passes); k_energy_scatter adds the replicas in a fixed order and writes column k of g_energy_amp / g_energy_det.
#pragma once

struct EnergyArgs {
    const double2* psi;    // the state of the launch's first save point, trajectory 0
    const int32_t* entry;  // optional: tape entry of save point k (states of [B][dim] amplitudes); else save points are kstride apart
    size_t kstride;
    const double* udiag;
    const double* coef;    // records [Bc][n_tsave][NC], trajectory 0, save point 0
    long coef_bstride;     // doubles between the trajectories' record sets (0: shared)
    int NC, n_tsave, k0, B, b_first;
    uint32_t dim;
    int iters;             // forward: amplitudes per thread (grid-stride)
    GroupArgs g;
    XyArgs xy;
    double* part;          // forward: [save point of the launch][grid.y][grid.x][2]
    // backward
    const double* gexp;    // the Energy rows of grad_expect: [rows][n_tsave][B]
    int rows;
    double2* z;            // [save point of the launch][B][dim]
    const double2* base;   // [save point of the launch][B][dim] or nullptr; may be `out`
    double2* out;
    double* ge;            // records [Bc][n_tsave][kEnergyReplicas][NC]
    long ge_bstride;
    double* wtot;          // [dim] or nullptr
    double* xy_ge;         // [kXyReplicas][N(N-1)/2] or nullptr
};

// h = (H v)[x]; group(q, s1r, s1i, s0r, s0i): the partner sums of drive group q over the set / clear bits of x; pair(p, part): the
// exchange partner of pair p (0 off the stencil), wave-uniformly for every pair.  `own` = v[x] (0 on dead threads).
template <bool XY, class Group, class Pair>
__device__ __forceinline__ void energy_h(const EnergyArgs& a, const double* __restrict__ cf, const double2* __restrict__ v, uint32_t xs, bool live,
                                         const double2& own, double& hr, double& hi, Group&& group, Pair&& pair) {
    const double d = diag_value(a.udiag, cf, a.g, xs);
    hr = d * own.x;
    hi = d * own.y;
    for (int q = 0; q < a.g.ga; ++q) {
        double s1r, s1i, s0r, s0i;
        xy_group_sums(a.g, v, xs, q, s1r, s1i, s0r, s0i);
        const double cr = cf[q], ci = cf[a.g.ga + q];
        hr += cr * s1r - ci * s1i + cr * s0r + ci * s0i;
        hi += cr * s1i + ci * s1r + cr * s0i - ci * s0r;
        group(q, s1r, s1i, s0r, s0i);
    }
    if constexpr (XY) xy_stencil<false>(a.xy, v, xs, live, hr, hi, pair);
}

__device__ __forceinline__ const double2* energy_state(const EnergyArgs& a, int kk, int b) {
    return a.psi + (a.entry ? size_t(a.entry[a.k0 + kk]) * (size_t(a.B) * a.dim) : size_t(kk) * a.kstride) + size_t(b) * a.dim;
}

// grid (workgroups, trajectories of the slice, save points), 256 threads
template <bool XY>
__global__ __launch_bounds__(256) void k_energy_expect(EnergyArgs a) {
    __shared__ double lds[8];
    const int kk = blockIdx.z, b = a.b_first + int(blockIdx.y);
    const double2* __restrict__ psi = energy_state(a, kk, b);
    const double* __restrict__ cf = a.coef + b * a.coef_bstride + size_t(a.k0 + kk) * a.NC;
    double e = 0.0, m = 0.0;
    for (int it = 0; it < a.iters; ++it) {  // uniform
        const uint32_t x = (uint32_t(it) * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
        const bool live = x < a.dim;
        const uint32_t xs = live ? x : 0u;
        double2 own = psi[xs];
        if (!live) own = make_double2(0.0, 0.0);
        double hr, hi;
        energy_h<XY>(a, cf, psi, xs, live, own, hr, hi, [](int, double, double, double, double) {}, [](int, const double2&) {});
        if (live) {
            e += own.x * hr + own.y * hi;
            m += hr * hr + hi * hi;
        }
    }
    e = wave_sum(e);
    m = wave_sum(m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds[wave] = e;
        lds[4 + wave] = m;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double* l = lds + 4 * threadIdx.x;
        a.part[((size_t(kk) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = (l[0] + l[1]) + (l[2] + l[3]);
    }
}

// grid (trajectories of the slice, save points), one wave: the workgroups' partial sums in index order, then a fixed shuffle tree
__global__ __launch_bounds__(64) void k_energy_finish(const double* __restrict__ part, double* __restrict__ out, int blocks, int rows, int n_tsave,
                                                      int k0, int B, int b_first) {
    const int kk = blockIdx.y, b = b_first + int(blockIdx.x);
    const double* __restrict__ p = part + (size_t(kk) * gridDim.x + blockIdx.x) * size_t(blocks) * 2;
    double e = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 64) {
        e += p[2 * i];
        m += p[2 * i + 1];
    }
    e = wave_sum(e);
    m = wave_sum(m);
    if (threadIdx.x == 0) {
        out[size_t(k0 + kk) * B + b] = e;
        if (rows > 1) out[size_t(n_tsave) * B + size_t(k0 + kk) * B + b] = m;
    }
}

// the two cotangents of save point k, trajectory b
__device__ __forceinline__ void energy_cotangents(const EnergyArgs& a, int k, int b, double& gE, double& gM) {
    gE = a.gexp[size_t(k) * a.B + b];
    gM = a.rows > 1 ? a.gexp[size_t(a.n_tsave) * a.B + size_t(k) * a.B + b] : 0.0;
}

// fac * Re<own| dH/dc |v> of drive group q from the partner sums of v: d/dRe c = s1 + s0, d/dIm c = i (s1 - s0)
__device__ __forceinline__ void energy_group_grad(double fac, const double2& own, double s1r, double s1i, double s0r, double s0i, double& gre,
                                                  double& gim) {
    gre = fac * (own.x * (s1r + s0r) + own.y * (s1i + s0i));
    gim = -fac * (own.x * (s1i - s0i) - own.y * (s1r - s0r));
}

// the exchange contractions of one workgroup: per pair one wave sum into LDS (each), then one atomic per pair (flush)
struct EnergyXyAcc {
    double (*xl)[kXyMaxPairs];
    __device__ __forceinline__ void each(int p, double v) const {
        const double w = wave_sum(v);
        if ((threadIdx.x & 63) == 0) xl[threadIdx.x >> 6][p] = w;
    }
    __device__ __forceinline__ void flush(double* __restrict__ xy_ge, int N) const {
        const int P = N * (N - 1) / 2;
        double* __restrict__ rep = xy_ge + size_t((blockIdx.x + blockIdx.y + blockIdx.z) % kXyReplicas) * P;
        __syncthreads();
        for (int p = threadIdx.x; p < P; p += 256) unsafeAtomicAdd(rep + p, (xl[0][p] + xl[1][p]) + (xl[2][p] + xl[3][p]));
    }
};

// grid (ceil(dim / 256), B, save points), 256 threads
template <bool XY>
__global__ __launch_bounds__(256) void k_energy_bwd1(EnergyArgs a) {
    __shared__ double lds[8];
    __shared__ double xl[XY ? 4 * kXyMaxPairs : 1];  // (no LDS for the pairs without the exchange)
    const int kk = blockIdx.z, b = blockIdx.y, k = a.k0 + kk;
    double gE, gM;
    energy_cotangents(a, k, b, gE, gM);
    if (gE == 0.0 && gM == 0.0) return;  // (uniform) cotangents usually sit at one or a few save points
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const uint32_t xs = live ? x : 0u;
    const double2* __restrict__ psi = energy_state(a, kk, b);
    const double* __restrict__ cf = a.coef + b * a.coef_bstride + size_t(k) * a.NC;
    double* __restrict__ ge = a.ge + b * a.ge_bstride + (size_t(k) * kEnergyReplicas + blockIdx.x % kEnergyReplicas) * a.NC;
    double2 own = psi[xs];
    if (!live) own = make_double2(0.0, 0.0);
    const EnergyXyAcc acc{reinterpret_cast<double(*)[kXyMaxPairs]>(xl)};
    const bool want_xy = XY && a.xy_ge != nullptr;
    double hr, hi;
    energy_h<XY>(
        a, cf, psi, xs, live, own, hr, hi,
        [&](int q, double s1r, double s1i, double s0r, double s0i) {
            if (gE == 0.0) return;  // uniform
            double gre, gim;
            energy_group_grad(-gE, own, s1r, s1i, s0r, s0i, gre, gim);
            block_atomic_add(gre, ge + q, lds);
            block_atomic_add(gim, ge + a.g.ga + q, lds);
        },
        [&](int p, const double2& part) {
            if (want_xy) acc.each(p, -gE * (own.x * part.x + own.y * part.y));
        });
    if (live) a.z[(size_t(kk) * a.B + b) * a.dim + x] = make_double2(gE * own.x + gM * hr, gE * own.y + gM * hi);
    // y = g_E psi + 2 g_M h at the own index: the diagonal contractions
    const double yr = gE * own.x + 2.0 * gM * hr, yi = gE * own.y + 2.0 * gM * hi;
    const double r = live ? yr * own.x + yi * own.y : 0.0;  // Re(conj(y) psi)
    if (a.wtot && live) unsafeAtomicAdd(a.wtot + x, r);
    for (int q = 0; q < a.g.gd; ++q) block_atomic_add(r * double(a.g.dcnt[q] - popc_i(xs & a.g.dmask[q])), ge + 2 * a.g.ga + q, lds);
    if (want_xy) acc.flush(a.xy_ge, a.xy.N);
}

// grid (ceil(dim / 256), B, save points), 256 threads
template <bool XY>
__global__ __launch_bounds__(256) void k_energy_bwd2(EnergyArgs a) {
    __shared__ double lds[8];
    __shared__ double xl[XY ? 4 * kXyMaxPairs : 1];  // (no LDS for the pairs without the exchange)
    const int kk = blockIdx.z, b = blockIdx.y, k = a.k0 + kk;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const uint32_t xs = live ? x : 0u;
    const size_t off = (size_t(kk) * a.B + b) * a.dim;
    double gE, gM;
    energy_cotangents(a, k, b, gE, gM);
    if (gE == 0.0 && gM == 0.0) {  // (uniform) nothing but the copy of base
        if (a.base != a.out && live) a.out[off + x] = a.base ? a.base[off + x] : make_double2(0.0, 0.0);
        return;
    }
    const double2* __restrict__ psi = energy_state(a, kk, b);
    const double2* __restrict__ z = a.z + off;
    const double* __restrict__ cf = a.coef + b * a.coef_bstride + size_t(k) * a.NC;
    double* __restrict__ ge = a.ge + b * a.ge_bstride + (size_t(k) * kEnergyReplicas + blockIdx.x % kEnergyReplicas) * a.NC;
    double2 own = psi[xs], zo = z[xs];
    if (!live) own = zo = make_double2(0.0, 0.0);
    const EnergyXyAcc acc{reinterpret_cast<double(*)[kXyMaxPairs]>(xl)};
    const bool want_xy = XY && a.xy_ge != nullptr;
    double hr, hi;
    energy_h<XY>(
        a, cf, z, xs, live, zo, hr, hi,
        [&](int q, double s1r, double s1i, double s0r, double s0i) {
            double gre, gim;
            energy_group_grad(2.0, own, s1r, s1i, s0r, s0i, gre, gim);
            block_atomic_add(gre, ge + q, lds);
            block_atomic_add(gim, ge + a.g.ga + q, lds);
        },
        [&](int p, const double2& part) {
            if (want_xy) acc.each(p, 2.0 * (own.x * part.x + own.y * part.y));
        });
    if (live) {
        double2 o = a.base ? a.base[off + x] : make_double2(0.0, 0.0);
        o.x = fma(2.0, hr, o.x);
        o.y = fma(2.0, hi, o.y);
        a.out[off + x] = o;
    }
    if (want_xy) acc.flush(a.xy_ge, a.xy.N);
}

// The records -> column k of g_energy_amp / g_energy_det (overwritten; the rule of k_scatter_grads: a term collects the groups it is
// a member of, the detuning record is d/d(dcoef) with dcoef = 2 sum det).  One thread per (save point, trajectory), replicas in order.
struct EnergyScatterArgs {
    const double* ge;  // [Bc][n_tsave][kEnergyReplicas][NC]
    double2* g_amp;    // [Bc][Ka][n_tsave] or nullptr
    double* g_det;     // [Bc][Kd][n_tsave] or nullptr
    int n_tsave, Ka, Kd, NC, ga, gd;
    uint64_t amem[kMaxGroups], dmem[kMaxGroups];
};

__global__ void k_energy_scatter(EnergyScatterArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= a.n_tsave) return;
    const double* reps = a.ge + (size_t(b) * a.n_tsave + k) * kEnergyReplicas * a.NC;
    double rec[3 * kMaxGroups];
    for (int c = 0; c < a.NC; ++c) {
        double sum = 0.0;
        for (int r = 0; r < kEnergyReplicas; ++r) sum += reps[size_t(r) * a.NC + c];  // fixed order
        rec[c] = sum;
    }
    if (a.g_amp)
        for (int t = 0; t < a.Ka; ++t) {
            double gr = 0.0, gi = 0.0;
            for (int g = 0; g < a.ga; ++g)
                if (a.amem[g] >> t & 1ull) {
                    gr += rec[g];
                    gi += rec[a.ga + g];
                }
            a.g_amp[(size_t(b) * a.Ka + t) * a.n_tsave + k] = make_double2(gr, gi);
        }
    if (a.g_det)
        for (int t = 0; t < a.Kd; ++t) {
            double gd = 0.0;
            for (int g = 0; g < a.gd; ++g)
                if (a.dmem[g] >> t & 1ull) gd += rec[2 * a.ga + g];
            a.g_det[(size_t(b) * a.Kd + t) * a.n_tsave + k] = 2.0 * gd;
        }
}

// ------------------------------------------------------------------------------------------------
// LDS-tile version (13 .. 24 qubits, no exchange; RydProblem.energy_kernel): a workgroup stages 2^12 amplitudes of the vector H acts
// on (64 KiB: two workgroups fit the 160 KiB of a CU), 16 per thread at x_r = tile + 256 r + t.  Partners in the 12 tile bits come
// from LDS, partners in the N - 12 high bits from coalesced global loads (the partner tile at the same offset); the coefficient
// record is read once per workgroup's amplitudes.  The same three epilogues as the direct version, MODE 0 forward / 1 pass 1 /
// 2 pass 2, with ONE workgroup reduction per coefficient (the thread sums its 16 amplitudes first) instead of one per amplitude.
// ------------------------------------------------------------------------------------------------
constexpr int kEnergyTileBits = 12;
constexpr int kEnergyTileR = 16;                                                                    // amplitudes per thread
constexpr size_t kEnergyTileLds = (size_t(1) << kEnergyTileBits) * sizeof(double2) + 8 * sizeof(double);  // the tile + the reduction slots

// hr / hi[r] = (H v)[x_r]; s: the staged tile of v, vg: v of the trajectory in global memory; own[r] = v[x_r]; con[r]: the vector the
// drive-group contractions are taken with (psi at x_r); each(q, gre, gim): the thread's sums over its amplitudes of
// Re<con| dH/dRe c_q |v> and Re<con| dH/dIm c_q |v>
template <class Each>
__device__ __forceinline__ void energy_tile_h(const EnergyArgs& a, const double* __restrict__ cf, const double2* __restrict__ vg,
                                              const double2* __restrict__ s, uint32_t tile, const double2 (&own)[kEnergyTileR],
                                              const double2 (&con)[kEnergyTileR], double (&hr)[kEnergyTileR], double (&hi)[kEnergyTileR], Each&& each) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kEnergyTileR; ++r) {
        const double d = diag_value(a.udiag, cf, a.g, tile + uint32_t(r) * 256u + t);
        hr[r] = d * own[r].x;
        hi[r] = d * own[r].y;
    }
    for (int q = 0; q < a.g.ga; ++q) {
        const double cr = cf[q], ci = cf[a.g.ga + q];
        double gre = 0.0, gim = 0.0;
        uint32_t m = a.g.amask[q];
        while (m) {  // uniform
            const uint32_t bit = m & (0u - m);
            m ^= bit;
            const bool low = bit < (1u << kEnergyTileBits);
            const double2* __restrict__ far = vg + (tile ^ bit);  // (high bit: the partner tile, same offsets)
#pragma unroll
            for (int r = 0; r < kEnergyTileR; ++r) {
                const uint32_t l = uint32_t(r) * 256u + t;
                const double2 p = low ? s[l ^ bit] : far[l];
                const double sgn = ((low ? l : tile) & bit) ? 1.0 : -1.0;  // bit set in x: c, else conj(c)
                hr[r] += cr * p.x - sgn * ci * p.y;
                hi[r] += cr * p.y + sgn * ci * p.x;
                gre += con[r].x * p.x + con[r].y * p.y;
                gim -= sgn * (con[r].x * p.y - con[r].y * p.x);
            }
        }
        each(q, gre, gim);
    }
}

// grid (2^(N-12) tiles, trajectories, save points), 256 threads, kEnergyTileLds bytes of dynamic LDS
template <int MODE>
__global__ __launch_bounds__(256) void k_energy_tile(EnergyArgs a) {
    extern __shared__ double2 e_tile[];
    double* lds = reinterpret_cast<double*>(e_tile + (size_t(1) << kEnergyTileBits));
    const int kk = blockIdx.z, b = (MODE == 0 ? a.b_first : 0) + int(blockIdx.y), k = a.k0 + kk;
    const uint32_t t = threadIdx.x, tile = blockIdx.x << kEnergyTileBits;
    const size_t off = (size_t(kk) * a.B + b) * a.dim;
    double gE = 0.0, gM = 0.0;
    if (MODE != 0) {
        energy_cotangents(a, k, b, gE, gM);
        if (gE == 0.0 && gM == 0.0) {  // uniform
            if (MODE == 2 && a.base != a.out)
                for (int r = 0; r < kEnergyTileR; ++r) {
                    const size_t i = off + tile + uint32_t(r) * 256u + t;
                    a.out[i] = a.base ? a.base[i] : make_double2(0.0, 0.0);
                }
            return;
        }
    }
    const double2* __restrict__ psi = energy_state(a, kk, b);
    const double2* __restrict__ vg = MODE == 2 ? a.z + off : psi;
    const double* __restrict__ cf = a.coef + b * a.coef_bstride + size_t(k) * a.NC;
    double* __restrict__ ge = MODE == 0 ? nullptr : a.ge + b * a.ge_bstride + (size_t(k) * kEnergyReplicas + blockIdx.x % kEnergyReplicas) * a.NC;
    double2 own[kEnergyTileR], con[kEnergyTileR];
#pragma unroll
    for (int r = 0; r < kEnergyTileR; ++r) {
        const uint32_t l = uint32_t(r) * 256u + t;
        own[r] = vg[tile + l];
        e_tile[l] = own[r];
        con[r] = MODE == 2 ? psi[tile + l] : own[r];
    }
    __syncthreads();
    double hr[kEnergyTileR], hi[kEnergyTileR];
    energy_tile_h(a, cf, vg, e_tile, tile, own, con, hr, hi, [&](int q, double gre, double gim) {
        if (MODE == 0 || (MODE == 1 && gE == 0.0)) return;  // uniform
        const double fac = MODE == 1 ? -gE : 2.0;
        block_atomic_add(fac * gre, ge + q, lds);
        block_atomic_add(fac * gim, ge + a.g.ga + q, lds);
    });
    if (MODE == 0) {
        double e = 0.0, m = 0.0;
#pragma unroll
        for (int r = 0; r < kEnergyTileR; ++r) {
            e += own[r].x * hr[r] + own[r].y * hi[r];
            m += hr[r] * hr[r] + hi[r] * hi[r];
        }
        e = wave_sum(e);
        m = wave_sum(m);
        const int lane = t & 63, wave = t >> 6;
        __syncthreads();
        if (lane == 0) {
            lds[wave] = e;
            lds[4 + wave] = m;
        }
        __syncthreads();
        if (t < 2) {
            const double* l = lds + 4 * t;
            a.part[((size_t(kk) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2 + t] = (l[0] + l[1]) + (l[2] + l[3]);
        }
    } else if (MODE == 1) {
        double rr[kEnergyTileR];
#pragma unroll
        for (int r = 0; r < kEnergyTileR; ++r) {
            const uint32_t x = tile + uint32_t(r) * 256u + t;
            a.z[off + x] = make_double2(gE * own[r].x + gM * hr[r], gE * own[r].y + gM * hi[r]);
            const double yr = gE * own[r].x + 2.0 * gM * hr[r], yi = gE * own[r].y + 2.0 * gM * hi[r];
            rr[r] = yr * own[r].x + yi * own[r].y;  // Re(conj(y) psi)
            if (a.wtot) unsafeAtomicAdd(a.wtot + x, rr[r]);
        }
        for (int q = 0; q < a.g.gd; ++q) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < kEnergyTileR; ++r) v += rr[r] * double(a.g.dcnt[q] - popc_i((tile + uint32_t(r) * 256u + t) & a.g.dmask[q]));
            block_atomic_add(v, ge + 2 * a.g.ga + q, lds);
        }
    } else {
#pragma unroll
        for (int r = 0; r < kEnergyTileR; ++r) {
            const size_t i = off + tile + uint32_t(r) * 256u + t;
            double2 o = a.base ? a.base[i] : make_double2(0.0, 0.0);
            o.x = fma(2.0, hr[r], o.x);
            o.y = fma(2.0, hi[r], o.y);
            a.out[i] = o;
        }
    }
}
