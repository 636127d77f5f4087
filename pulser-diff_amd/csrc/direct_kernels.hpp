// direct_kernels.hpp — set-up kernels (interaction diagonal, table statistics, coefficient expansion, metadata upload), the
// one-amplitude-per-thread factor kernels and the reductions / gradient scatter around them (included by rydiff.hip after common.hpp).
#pragma once

// ------------------------------------------------------------------------------------------------
// K6: static interaction diagonal  U(x) = sum_{i<j} U_ij n_i(x) n_j(x),  n_j = 1 - bit_{N-1-j}(x)
// ------------------------------------------------------------------------------------------------
// sharded runs: one table per slab (blockIdx.y), evaluated at the global index x | (rank << nl)
__global__ void k_build_udiag(double* __restrict__ udiag, const double* __restrict__ u_pairs, int N, uint32_t dim, int nl = 0,
                              int rank_first = 0) {
    const uint32_t xl = blockIdx.x * blockDim.x + threadIdx.x;
    if (xl >= dim) return;
    udiag += size_t(blockIdx.y) * dim;
    const uint32_t x = xl | (nl ? ((uint32_t(rank_first) + blockIdx.y) << nl) : 0u);
    double s = 0.0;
    int k = 0;
    for (int i = 0; i < N; ++i) {
        const bool ni = !((x >> (N - 1 - i)) & 1u);
        for (int j = i + 1; j < N; ++j, ++k) {
            const bool nj = !((x >> (N - 1 - j)) & 1u);
            if (ni && nj) s += u_pairs[k];
        }
    }
    udiag[xl] = s;
}

// split form of the interaction diagonal for one tile layout (chain_kernels.hpp):
//   U(x) = utt[i] + vr[t][LT] + sum_{tile bits a with n_a(i)=1} vr[t][a],   x = x(t, i);   LT = 12 or 13 tile bits
__global__ void k_build_split(double* __restrict__ utt, double* __restrict__ vr, const double* __restrict__ u_pairs,
                              int N, int lo, int hs, int hb, unsigned tiles, int LT) {
    const unsigned id = blockIdx.x * blockDim.x + threadIdx.x;
    auto gbit = [&](int b) { return b < lo ? b : hs + (b - lo); };          // tile bit -> index bit
    auto upair = [&](int ib, int jb) {                                       // index bits -> U_ij
        int qi = N - 1 - ib, qj = N - 1 - jb;
        if (qi > qj) { int tmp = qi; qi = qj; qj = tmp; }
        return u_pairs[qi * (2 * N - qi - 1) / 2 + (qj - qi - 1)];
    };
    if (id < (1u << LT)) {
        double s = 0.0;
        for (int a = 0; a < LT; ++a)
            for (int b = a + 1; b < LT; ++b)
                if (!(id >> a & 1u) && !(id >> b & 1u)) s += upair(gbit(a), gbit(b));
        utt[id] = s;
    } else if (id - (1u << LT) < tiles) {
        const unsigned t = id - (1u << LT);
        const int midlow = hs - lo;
        const unsigned xbase = ((t & ((1u << midlow) - 1u)) << lo) | ((t >> midlow) << (hs + hb));
        uint32_t tile_bits = 0;
        for (int a = 0; a < LT; ++a) tile_bits |= 1u << gbit(a);
        double* row = vr + size_t(t) * 16;
        double urr = 0.0;
        for (int ib = 0; ib < N; ++ib) {
            if (tile_bits >> ib & 1u) continue;
            if (xbase >> ib & 1u) continue;  // n = 0
            for (int jb = ib + 1; jb < N; ++jb)
                if (!(tile_bits >> jb & 1u) && !(xbase >> jb & 1u)) urr += upair(ib, jb);
        }
        for (int a = 0; a < LT; ++a) {
            double v = 0.0;
            for (int jb = 0; jb < N; ++jb)
                if (!(tile_bits >> jb & 1u) && !(xbase >> jb & 1u)) v += upair(gbit(a), jb);
            row[a] = v;
        }
        row[LT] = urr;
        for (int c = LT + 1; c < 16; ++c) row[c] = 0.0;
    }
}

// g_u[pair] = sum_x n_i n_j wtot[x]
// sharded runs (slabs > 0): wtot holds one slab of 2^nl weights per rank of the call; amplitude x of slab b sits at the global index
// x | (rank_first + b) << nl — every rank adds its part, the caller sums g_u over the ranks
__global__ void k_ugrad(double* __restrict__ g_u, const double* __restrict__ wtot, int N, uint32_t dim, int slabs = 0, int nl = 0,
                        int rank_first = 0) {
    __shared__ double lds[8];
    const int pair = blockIdx.y;
    int i = 0, rem = pair;
    while (rem >= N - 1 - i) {
        rem -= N - 1 - i;
        ++i;
    }
    const int j = i + 1 + rem;
    const uint32_t mi = 1u << (N - 1 - i), mj = 1u << (N - 1 - j);
    double s = 0.0;
    if (slabs > 0) {
        for (int b = 0; b < slabs; ++b) {
            const uint32_t hi = uint32_t(rank_first + b) << nl;
            for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < dim; x += gridDim.x * blockDim.x)
                if (!((x | hi) & mi) && !((x | hi) & mj)) s += wtot[size_t(b) * dim + x];
        }
    } else {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < dim; x += gridDim.x * blockDim.x)
            if (!(x & mi) && !(x & mj)) s += wtot[x];
    }
    block_atomic_add(s, g_u + pair, lds);
}

// ------------------------------------------------------------------------------------------------
// table statistics for the spectral bound (over sample index i, all trajectories):
//   stats[0] = max_i sum_g |c_g[i]| * count_g         (norm of the flip part, exact for commuting single-qubit terms)
//   stats[1] = max_i sum_g max(+dcoef_g[i],0)*count_g  stats[2] = max_i sum_g max(-dcoef_g[i],0)*count_g
//   stats[3] = sum of max(U_ij, 0)     stats[5] = sum of max(-U_ij, 0)   (the doubled register of the master-equation path
//                                                                        carries -U_ij on its column qubits)
//   stats[4] = max_i sum_g |Im c_g[i]|   (non-zero: some drive has a phase)
//   stats[6] = sum of |J_ij|   (XY exchange, RydProblem.xy_pairs: every row of the exchange has at most this absolute sum)
// all non-negative doubles -> their bit patterns order like unsigned integers (atomicMax on u64).
// ------------------------------------------------------------------------------------------------
struct StatsArgs {
    const double2* amp;
    const double* det;
    const double* u_pairs;
    const double* xy_pairs;  // nullptr: no exchange
    int n_samples, Ka, Kd, n_pairs, Bc;
    int ga, gd;
    uint64_t amem[kMaxGroups], dmem[kMaxGroups];
    int acnt[kMaxGroups], dcnt[kMaxGroups];
    uint32_t dones;  // detuning groups that count ones: (count - popcount) ranges over [-dcnt, 0] instead of [0, dcnt]
};

__global__ void k_table_stats(unsigned long long* __restrict__ stats, StatsArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i < a.n_samples) {
        double flip = 0.0, dpos = 0.0, dneg = 0.0, imabs = 0.0;
        for (int g = 0; g < a.ga; ++g) {
            double re = 0.0, im = 0.0;
            for (int k = 0; k < a.Ka; ++k)
                if (a.amem[g] >> k & 1ull) {
                    double2 v = a.amp[(size_t(b) * a.Ka + k) * a.n_samples + i];
                    re += v.x;
                    im += v.y;
                }
            flip += sqrt(re * re + im * im) * a.acnt[g];
            imabs += fabs(im);
        }
        for (int g = 0; g < a.gd; ++g) {
            double d = 0.0;
            for (int k = 0; k < a.Kd; ++k)
                if (a.dmem[g] >> k & 1ull) d += 2.0 * a.det[(size_t(b) * a.Kd + k) * a.n_samples + i];
            if (a.dones >> g & 1u) d = -d;
            if (d > 0.0) dpos += d * a.dcnt[g];
            else dneg += -d * a.dcnt[g];
        }
        atomicMax(stats + 0, (unsigned long long)__double_as_longlong(flip));
        atomicMax(stats + 1, (unsigned long long)__double_as_longlong(dpos));
        atomicMax(stats + 2, (unsigned long long)__double_as_longlong(dneg));
        atomicMax(stats + 4, (unsigned long long)__double_as_longlong(imabs));
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        double sp = 0.0, sn = 0.0;
        for (int k = 0; k < a.n_pairs; ++k) {
            const double u = a.u_pairs[k];
            if (u > 0.0) sp += u;
            else sn -= u;
        }
        stats[3] = (unsigned long long)__double_as_longlong(sp);
        stats[5] = (unsigned long long)__double_as_longlong(sn);
        double sj = 0.0;
        if (a.xy_pairs)
            for (int k = 0; k < a.n_pairs; ++k) sj += fabs(a.xy_pairs[k]);
        stats[6] = (unsigned long long)__double_as_longlong(sj);
    }
}

// ------------------------------------------------------------------------------------------------
// K0: effective coefficients of every exponential.  record = c_re[ga], c_im[ga], dcoef[gd]
//   c_g   = sum_{terms k in group g} sum_q w[e][q] * amp_k[idx[e][q]]        (hamiltonian.py:542)
//   dcoef = 2 * sum_{terms k in group g} sum_q w[e][q] * det_k[idx[e][q]]    (hamiltonian.py:538-540)
// ------------------------------------------------------------------------------------------------
// per-exponential metadata as it lives on the device (uploaded through kernel arguments, see upload_words)
struct StageDev {     // forward: the two samples entering the coefficient combination and their weights (hamiltonian.py:532-542)
    double w0, w1;
    int32_t i0, i1;
};
struct StageBwdDev {  // backward: how the exponential's duration and interpolation time depend on tsave
    double tau_scale, tnw0, tnw1;
    int32_t tn0, tn1, t_hi, t_lo;  // -1: not a tsave point
};
static_assert(sizeof(StageDev) == 24 && sizeof(StageBwdDev) == 40, "stage records are uploaded as 8-byte words");

struct ExpandArgs {
    const double2* amp;
    const double* det;
    const StageDev* st;  // [E]
    double* coef;        // [Bc][E][NC]
    int E, n_samples, Ka, Kd, NC, ga, gd;
    uint64_t amem[kMaxGroups], dmem[kMaxGroups];
};

__global__ void k_expand_coeffs(ExpandArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= a.E) return;
    double* rec = a.coef + (size_t(b) * a.E + e) * a.NC;
    const StageDev sd = a.st[e];
    const int idx[2] = {sd.i0, sd.i1};
    const double w[2] = {sd.w0, sd.w1};
    for (int g = 0; g < a.ga; ++g) {
        double re = 0.0, im = 0.0;
        for (int k = 0; k < a.Ka; ++k)
            if (a.amem[g] >> k & 1ull) {
                const double2* t = a.amp + (size_t(b) * a.Ka + k) * a.n_samples;
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (w[q] != 0.0) {
                        re += w[q] * t[idx[q]].x;
                        im += w[q] * t[idx[q]].y;
                    }
            }
        rec[g] = re;
        rec[a.ga + g] = im;
    }
    for (int g = 0; g < a.gd; ++g) {
        double d = 0.0;
        for (int k = 0; k < a.Kd; ++k)
            if (a.dmem[g] >> k & 1ull) {
                const double* t = a.det + (size_t(b) * a.Kd + k) * a.n_samples;
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (w[q] != 0.0) d += w[q] * t[idx[q]];
            }
        rec[2 * a.ga + g] = 2.0 * d;
    }
}

// ------------------------------------------------------------------------------------------------
// K1 (direct variant): one amplitude per thread, partners fetched from global memory (L2 / Infinity Cache).
//   y[x] = (gamma + beta*d(x)) psi[x] + beta * sum_g [ c_g * sum_{j in g, bit_j(x)=1} psi[x^m_j]
//                                                   + conj(c_g) * sum_{j in g, bit_j(x)=0} psi[x^m_j] ]
//   d(x) = U(x) + sum_g dcoef_g * (#qubits of g in |r>)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double diag_value(const double* __restrict__ udiag, const double* __restrict__ cf, const GroupArgs& g,
                                             uint32_t x, uint32_t xglob) {
    double d = udiag[x];
    for (int q = 0; q < g.gd; ++q) d += cf[2 * g.ga + q] * double(g.dcnt[q] - popc_i(xglob & g.dmask[q]));
    return d;
}
__device__ __forceinline__ double diag_value(const double* __restrict__ udiag, const double* __restrict__ cf, const GroupArgs& g,
                                             uint32_t x) {
    return diag_value(udiag, cf, g, x, x);
}

__global__ __launch_bounds__(256) void k_factor_direct(FactorArgs a) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.dim) return;
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.use_inline ? a.coef_inline : a.coef + blockIdx.y * a.coef_bstride;
    const unsigned rank = unsigned(a.sh_rank_first) + blockIdx.y;
    const uint32_t xglob = a.sh_bits ? (x | (rank << a.sh_nl)) : x;  // sharded: the diagonal lives at the global index
    const double d = diag_value(a.udiag + (a.sh_bits ? boff : 0), cf, a.g, x, xglob);
    const double2 v = xin[x];
    const double dr = a.gr + a.br * d, di = a.gi + a.bi * d;
    double ar = dr * v.x - di * v.y, ai = dr * v.y + di * v.x;
    for (int k = 0; k < a.sh_bits; ++k) {  // flips of the rank qubits: partner slabs
        if (a.sh_grp[k] < 0) continue;
        const double cr = cf[a.sh_grp[k]], ci = (rank >> k & 1u) ? cf[a.g.ga + a.sh_grp[k]] : -cf[a.g.ga + a.sh_grp[k]];
        const double kr = a.br * cr - a.bi * ci, ki = a.br * ci + a.bi * cr;
        const double2 rv = a.sh_self ? a.xin[size_t(blockIdx.y ^ (1u << k)) * a.dim + x] : a.sh_rem[k][boff + x];
        ar += kr * rv.x - ki * rv.y;
        ai += kr * rv.y + ki * rv.x;
    }
    for (int k = 0; k < a.n_remote; ++k) {
        const double2 rv = a.remote[k][boff + x];
        ar += a.rc[2 * k] * rv.x - a.rc[2 * k + 1] * rv.y;
        ai += a.rc[2 * k] * rv.y + a.rc[2 * k + 1] * rv.x;
    }
    for (int q = 0; q < a.g.ga; ++q) {
        double s1r = 0.0, s1i = 0.0, s0r = 0.0, s0i = 0.0;
        uint32_t m = a.g.amask[q];
        while (m) {
            const uint32_t bit = m & (0u - m);
            m ^= bit;
            if (!flip_acts(a.g.cond, q, x, bit)) continue;
            const double2 p = xin[x ^ bit];
            if (x & bit) {
                s1r += p.x;
                s1i += p.y;
            } else {
                s0r += p.x;
                s0i += p.y;
            }
        }
        const double cr = cf[q], ci = cf[a.g.ga + q];
        // beta*c and beta*conj(c)
        const double b1r = a.br * cr - a.bi * ci, b1i = a.br * ci + a.bi * cr;
        const double b0r = a.br * cr + a.bi * ci, b0i = -a.br * ci + a.bi * cr;
        ar += b1r * s1r - b1i * s1i + b0r * s0r - b0i * s0i;
        ai += b1r * s1i + b1i * s1r + b0r * s0i + b0i * s0r;
    }
    if (a.pair.n) {  // beta * (dense two-qubit terms)
        const double2 pv = pair_apply(a.pair, 0, xin, x);
        ar += a.br * pv.x - a.bi * pv.y;
        ai += a.br * pv.y + a.bi * pv.x;
    }
    a.xout[boff + x] = make_double2(ar, ai);
}

// ------------------------------------------------------------------------------------------------
// K3 (direct variant): adjoint of one factor + gradient contractions.
//   gout = (conj(gamma) + conj(beta) H) gin
//   dL/dRe c_g += Re( beta * sum_x conj(gin[x]) * (partner sums of xin) )      dL/dIm c_g likewise with +-i
//   dL/ddcoef_g += sum_x cnt_g(x) * Re( beta conj(gin[x]) xin[x] )
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_factor_bwd_direct(FactorBwdArgs a) {
    __shared__ double lds[8];
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ gin = a.gin + boff;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.coef + blockIdx.y * a.coef_bstride;
    double* __restrict__ ge = a.ge + blockIdx.y * a.ge_bstride + (blockIdx.x % kGradReplicas) * a.ge_rstride;
    const uint32_t xs = live ? x : 0u;
    const unsigned rank = unsigned(a.sh_rank_first) + blockIdx.y;
    const uint32_t xglob = a.sh_bits ? (xs | (rank << a.sh_nl)) : xs;  // sharded: the diagonal lives at the global index
    const double d = diag_value(a.udiag + (a.sh_bits ? boff : 0), cf, a.g, xs, xglob);
    double2 gy = gin[xs];
    double2 xi = xin[xs];
    if (!live) {
        gy = make_double2(0.0, 0.0);
        xi = make_double2(0.0, 0.0);
    }
    // adjoint matvec with conj(gamma), conj(beta)
    const double dr = a.gr + a.br * d, di = -(a.gi + a.bi * d);
    double ar = dr * gy.x - di * gy.y, ai = dr * gy.y + di * gy.x;
    // a_ = beta * conj(gy)
    const double pr = a.br * gy.x + a.bi * gy.y, pi = a.bi * gy.x - a.br * gy.y;
    const double r = pr * xi.x - pi * xi.y;  // Re(beta conj(gy) xi)
    if (a.wtot && live) unsafeAtomicAdd(a.wtot + (a.sh_bits ? boff : 0) + x, r);  // sharded: one weight slab per rank (k_ugrad)
    for (int q = 0; q < a.g.ga; ++q) {
        double s1r = 0.0, s1i = 0.0, s0r = 0.0, s0i = 0.0;  // partner sums of gin: for the matvec AND for the contraction
        uint32_t m = a.g.amask[q];
        while (m) {
            const uint32_t bit = m & (0u - m);
            m ^= bit;
            if (!flip_acts(a.g.cond, q, xs, bit)) continue;
            const double2 p = gin[xs ^ bit];
            if (xs & bit) {
                s1r += p.x; s1i += p.y;
            } else {
                s0r += p.x; s0i += p.y;
            }
        }
        for (int k = 0; k < a.sh_bits; ++k) {  // flips of the rank qubits of this group: the partner ranks' cotangent slabs
            if (a.sh_grp[k] != q) continue;
            const double2 p = a.sh_self ? a.gin[size_t(blockIdx.y ^ (1u << k)) * a.dim + xs] : a.sh_rem[k][boff + xs];
            if (rank >> k & 1u) {
                s1r += p.x; s1i += p.y;
            } else {
                s0r += p.x; s0i += p.y;
            }
        }
        const double cr = cf[q], ci = cf[a.g.ga + q];
        // conj(beta)*c and conj(beta)*conj(c)
        const double b1r = a.br * cr + a.bi * ci, b1i = a.br * ci - a.bi * cr;
        const double b0r = a.br * cr - a.bi * ci, b0i = -a.br * ci - a.bi * cr;
        ar += b1r * s1r - b1i * s1i + b0r * s0r - b0i * s0i;
        ai += b1r * s1i + b1i * s1r + b0r * s0i + b0i * s0r;
        // S1 = sum_x a_(x) t1(x), S0 = sum_x a_(x) t0(x) with t1 / t0 the partner sums of xin over the bits that are 1 / 0 in x;
        // g_cre = Re(S1+S0), g_cim = -Im(S1-S0).  Re-indexed over the partner (the flip is an involution that toggles the bit):
        // S1 = sum_y xin(y) beta conj(s0(y)), S0 = sum_y xin(y) beta conj(s1(y)) — the cotangent's partner sums, which the matvec
        // needs anyway, and the OWN tape element only: no partner loads of the tape vector.
        double gre = 0.0, gim = 0.0;
        if (live) {
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
        const double v = live ? r * double(a.g.dcnt[q] - popc_i(xglob & a.g.dmask[q])) : 0.0;
        block_atomic_add(v, ge + 2 * a.g.ga + q, lds);
    }
    if (a.pair.n && live) {  // conj(beta) * (pair terms)^dagger applied to the cotangent
        const double2 pv = pair_apply(a.pair, 1, gin, x);
        ar += a.br * pv.x + a.bi * pv.y;
        ai += a.br * pv.y - a.bi * pv.x;
    }
    if ((a.inj_gexp || a.inj_gstate) && live) {
        const double2 add = injected_cotangent(a.inj_gstate, a.inj_gexp, a.inj_obs, a.inj_n_obs, a.inj_ostride, a.obs_ostride, a.obs_bstride,
                                               blockIdx.y, boff, x, xi);
        ar += add.x;
        ai += add.y;
    }
    if (live) a.gout[boff + x] = make_double2(ar, ai);
}

// ------------------------------------------------------------------------------------------------
// Direct kernels for ONE GLOBAL DRIVE on a register of exactly NQ qubits (every bit in the amplitude mask; no remote
// vectors, no pair terms).  The generic kernels above walk the set bits of a runtime mask: one partner load, one wait per bit
// — on 13..18 qubits, where a pass is a few microseconds, that chain of N dependent L2 latencies IS the kernel time.  Here the
// loop over the NQ bits is unrolled, so all partner loads are in flight together and the plain / signed partner sums replace
// the per-bit branch (c*s1 + conj(c)*s0 = cr*(s1+s0) + i*ci*(s1-s0)).
// ------------------------------------------------------------------------------------------------
// ONEXCD (12 and 13 qubits: <= 32 workgroups): the grid is 8x oversubscribed and only the workgroups that the round-robin dispatch
// places on XCD (trajectory % 8) work, so that a trajectory's vectors stay in ONE XCD's L2 from pass to pass — the partner
// loads then hit that L2 instead of crossing the fabric (placement is a speed matter only: results do not depend on it).
// Measured forward steps/s with / without: N=13 39.7 k / 23.9 k, N=14 24.3 k / 22.0 k (but its adjoint 10 % slower), N=15 21.8 k /
// 28.6 k, N=16 13.2 k / 24.6 k — one XCD's 32 CUs are not enough from 14 qubits on.
template <int NQ, bool ONEXCD>
__global__ __launch_bounds__(256) void k_factor_direct_global(FactorArgs a) {
    if (ONEXCD && (blockIdx.x & 7u) != (blockIdx.y & 7u)) return;
    const uint32_t x = (ONEXCD ? (blockIdx.x >> 3) : blockIdx.x) * 256u + threadIdx.x;  // dim = 2^NQ is a multiple of 256
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.use_inline ? a.coef_inline : a.coef + blockIdx.y * a.coef_bstride;
    double2 p[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) p[j] = xin[x ^ (1u << j)];
    const double2 v = xin[x];
    const double d = diag_value(a.udiag, cf, a.g, x);
    double tsr = 0.0, tsi = 0.0, dsr = 0.0, dsi = 0.0;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const double sgn = (x >> j & 1u) ? 1.0 : -1.0;
        tsr += p[j].x;
        tsi += p[j].y;
        dsr = fma(sgn, p[j].x, dsr);
        dsi = fma(sgn, p[j].y, dsi);
    }
    const double dr = a.gr + a.br * d, di = a.gi + a.bi * d;
    const double cr = cf[0], ci = cf[1];
    // F = cr*ts + i*ci*ds
    const double fr = cr * tsr - ci * dsi, fi = cr * tsi + ci * dsr;
    const double2 y = make_double2(dr * v.x - di * v.y + a.br * fr - a.bi * fi, dr * v.y + di * v.x + a.br * fi + a.bi * fr);
    a.xout[boff + x] = y;
    if (a.obs) {  // wave-uniform: <y|O|y> for diagonal observables straight from the register that holds y
        __shared__ double lds[8];
        const double w = y.x * y.x + y.y * y.y;
        for (int o = 0; o < a.n_obs; ++o) block_atomic_add(a.obs[size_t(o) * a.dim + x] * w, a.expect_slot + o * a.exp_ostride + blockIdx.y, lds);
    }
}

template <int NQ, bool ONEXCD>
__global__ __launch_bounds__(256) void k_factor_bwd_direct_global(FactorBwdArgs a) {
    __shared__ double lds[8];
    __shared__ double lds3[12];  // 3 values x 4 waves
    if (ONEXCD && (blockIdx.x & 7u) != (blockIdx.y & 7u)) return;
    const uint32_t wg = ONEXCD ? (blockIdx.x >> 3) : blockIdx.x;
    const uint32_t x = wg * 256u + threadIdx.x;
    const size_t boff = size_t(blockIdx.y) * a.dim;
    const double2* __restrict__ gin = a.gin + boff;
    const double2* __restrict__ xin = a.xin + boff;
    const double* __restrict__ cf = a.coef + blockIdx.y * a.coef_bstride;
    double* __restrict__ ge = a.ge + blockIdx.y * a.ge_bstride + (wg % kGradReplicas) * a.ge_rstride;
    double2 pg[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) pg[j] = gin[x ^ (1u << j)];
    const double2 gy = gin[x], xi = xin[x];
    const double d = diag_value(a.udiag, cf, a.g, x);
    double gsr = 0.0, gsi = 0.0, gdr = 0.0, gdi = 0.0;  // plain / signed partner sums of the cotangent
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const double sgn = (x >> j & 1u) ? 1.0 : -1.0;
        gsr += pg[j].x;
        gsi += pg[j].y;
        gdr = fma(sgn, pg[j].x, gdr);
        gdi = fma(sgn, pg[j].y, gdi);
    }
    const double cr = cf[0], ci = cf[1];
    // adjoint matvec: conj(gamma + beta d) gy + conj(beta) (cr*gs + i*ci*gd)
    const double dr = a.gr + a.br * d, di = -(a.gi + a.bi * d);
    const double fr = cr * gsr - ci * gdi, fi = cr * gsi + ci * gdr;
    double2 go = make_double2(dr * gy.x - di * gy.y + a.br * fr + a.bi * fi, dr * gy.y + di * gy.x + a.br * fi - a.bi * fr);
    if (a.inj_gexp || a.inj_gstate) {
        const double2 add = injected_cotangent(a.inj_gstate, a.inj_gexp, a.inj_obs, a.inj_n_obs, a.inj_ostride, a.obs_ostride, a.obs_bstride,
                                               blockIdx.y, boff, x, xi);
        go.x += add.x;
        go.y += add.y;
    }
    a.gout[boff + x] = go;
    // contractions with a_ = beta * conj(gy):  dL/dRe c = Re(a_ * xs),  dL/dIm c = -Im(a_ * xd)
    const double pr = a.br * gy.x + a.bi * gy.y, pi = a.bi * gy.x - a.br * gy.y;
    const double r = pr * xi.x - pi * xi.y;  // Re(beta conj(gy) xi)
    if (a.wtot) unsafeAtomicAdd(a.wtot + x, r);
    // dL/dRe c = Re sum_x a_(x) xs(x), dL/dIm c = -Im sum_x a_(x) xd(x) with xs / xd the plain / signed partner sums of the TAPE
    // vector — re-indexed over the partner: sum_x a_ xs = sum_y xin(y) beta conj(gs(y)), sum_x a_ xd = -sum_y xin(y) beta conj(gd(y))
    // (flipping bit j toggles its sign): the cotangent's partner sums and the own tape element, no partner loads of the tape.
    const double qsr = a.br * gsr + a.bi * gsi, qsi = a.bi * gsr - a.br * gsi;  // beta conj(gs)
    const double qdr = a.br * gdr + a.bi * gdi, qdi = a.bi * gdr - a.br * gdi;  // beta conj(gd)
    // the two drive gradients and the first detuning gradient share ONE workgroup reduction (one pair of barriers)
    double v0 = wave_sum(qsr * xi.x - qsi * xi.y), v1 = wave_sum(qdr * xi.y + qdi * xi.x);
    double v2 = wave_sum(a.g.gd > 0 ? r * double(a.g.dcnt[0] - popc_i(x & a.g.dmask[0])) : 0.0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds3[wave] = v0;
        lds3[4 + wave] = v1;
        lds3[8 + wave] = v2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double sum = lds3[4 * threadIdx.x] + lds3[4 * threadIdx.x + 1] + lds3[4 * threadIdx.x + 2] + lds3[4 * threadIdx.x + 3];
        if (threadIdx.x < 2 || a.g.gd > 0) unsafeAtomicAdd(ge + threadIdx.x, sum);
    }
    for (int q = 1; q < a.g.gd; ++q) block_atomic_add(r * double(a.g.dcnt[q] - popc_i(x & a.g.dmask[q])), ge + 2 + q, lds);
}

// dL/dtau of one exponential:  Re< g, -i H x >  = Im( sum_x conj(g[x]) (H x)[x] )
// State-sharded runs take the same number as Im( sum_x conj((H g)[x]) x[x] ): H goes onto the cotangent, whose partner slabs the next
// adjoint launch needs anyway, so the state slabs at the exponential's output never travel.
struct DotHArgs {
    const double2* g;
    const double2* x;
    const double* udiag;
    const double* coef;
    long coef_bstride;
    double* out;  // ge record + NC (gtau slot), trajectory 0
    long out_bstride;
    long out_rstride;
    uint32_t dim;
    int b_first;  // the grid's y dimension covers trajectories b_first, b_first + 1, ...
    GroupArgs gr;
    PairArgs pair;
    // state-sharded run (ChainArgs documents the fields): slabs as trajectories, sh_rem = the partner ranks' COTANGENT slabs
    int sh_bits = 0, sh_nl = 0, sh_rank_first = 0, sh_self = 0;
    const double2* sh_rem[kShardMaxBits] = {};
    int sh_grp[kShardMaxBits] = {};
};

__global__ __launch_bounds__(256) void k_dot_hx(DotHArgs a) {
    __shared__ double lds[8];
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const bool live = x < a.dim;
    const uint32_t xs = live ? x : 0u;
    const int bt = a.b_first + int(blockIdx.y);
    const size_t boff = size_t(bt) * a.dim;
    // the vector H acts on and the one it is contracted with: (x, g), sharded (g, x)
    const double2* __restrict__ xin = (a.sh_bits ? a.g : a.x) + boff;
    const double2* __restrict__ oth = (a.sh_bits ? a.x : a.g) + boff;
    const double* __restrict__ cf = a.coef + bt * a.coef_bstride;
    const unsigned rank = unsigned(a.sh_rank_first + bt);
    const uint32_t xglob = a.sh_bits ? (xs | (rank << a.sh_nl)) : xs;  // sharded: the diagonal lives at the global index
    const double d = diag_value(a.udiag + (a.sh_bits ? boff : 0), cf, a.gr, xs, xglob);
    const double2 v = xin[xs];
    double hr = d * v.x, hi = d * v.y;
    // Sharded: H on the cotangent instead of the state is legal because H is Hermitian here — sharded runs take neither pair terms
    // nor conditioned flips (plan.hpp refuses both); whoever lifts the first refusal has to move H back onto x for those terms.
    for (int k = 0; k < a.sh_bits; ++k) {  // flips of the rank qubits: the partner ranks' cotangent slabs at the same local index
        if (a.sh_grp[k] < 0) continue;
        const double cr = cf[a.sh_grp[k]], ci = (rank >> k & 1u) ? cf[a.gr.ga + a.sh_grp[k]] : -cf[a.gr.ga + a.sh_grp[k]];
        const double2 p = a.sh_self ? a.g[size_t(unsigned(bt) ^ (1u << k)) * a.dim + xs] : a.sh_rem[k][boff + xs];
        hr += cr * p.x - ci * p.y;
        hi += cr * p.y + ci * p.x;
    }
    for (int q = 0; q < a.gr.ga; ++q) {
        double s1r = 0.0, s1i = 0.0, s0r = 0.0, s0i = 0.0;
        uint32_t m = a.gr.amask[q];
        while (m) {
            const uint32_t bit = m & (0u - m);
            m ^= bit;
            if (!flip_acts(a.gr.cond, q, xs, bit)) continue;
            const double2 p = xin[xs ^ bit];
            if (xs & bit) { s1r += p.x; s1i += p.y; } else { s0r += p.x; s0i += p.y; }
        }
        const double cr = cf[q], ci = cf[a.gr.ga + q];
        hr += cr * s1r - ci * s1i + cr * s0r + ci * s0i;
        hi += cr * s1i + ci * s1r + cr * s0i - ci * s0r;
    }
    if (a.pair.n) {
        const double2 pv = pair_apply(a.pair, 0, xin, xs);
        hr += pv.x;
        hi += pv.y;
    }
    const double2 g = oth[xs];
    // Im(conj(g) * h) = g.x*hi - g.y*hr;  sharded: Im(conj(h) * x) = -(x.x*hi - x.y*hr)
    double val = live ? (g.x * hi - g.y * hr) : 0.0;
    if (a.sh_bits) val = -val;
    block_atomic_add(val, a.out + bt * a.out_bstride + (blockIdx.x % kGradReplicas) * a.out_rstride, lds);
}

// ------------------------------------------------------------------------------------------------
// K2: expectation values of diagonal observables, one launch per saved state.
// ------------------------------------------------------------------------------------------------
// obs_bstride / obs_ostride: 0 / dim for one observable table shared by the batch; sharded runs: dim / B*dim (one slab per rank)
__global__ __launch_bounds__(256) void k_expect_diag(const double2* __restrict__ psi, const double* __restrict__ obs,
                                                     double* __restrict__ out /* [n_obs][n_tsave][B] */, int n_obs,
                                                     int n_tsave, int k, int B, uint32_t dim, long obs_bstride = 0) {
    __shared__ double lds[8];
    const int b = blockIdx.y;
    const double2* __restrict__ p = psi + size_t(b) * dim;
    const size_t ostride = obs_bstride ? size_t(B) * dim : dim;
    for (int o = 0; o < n_obs; ++o) {
        double s = 0.0;
        for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < dim; x += gridDim.x * 256u) {
            const double2 v = p[x];
            s += obs[size_t(o) * ostride + size_t(b) * obs_bstride + x] * (v.x * v.x + v.y * v.y);
        }
        block_atomic_add(s, out + (size_t(o) * n_tsave + k) * B + b, lds);
    }
}

// ------------------------------------------------------------------------------------------------
// K4: lambda[b][x] (+)= grad_states[k][b][x] + 2 * sum_o ge[o][k][b] * obs[o][x] * psi_k[b][x]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_inject(double2* __restrict__ lam, const double2* __restrict__ gstate,
                                                const double2* __restrict__ psi, const double* __restrict__ obs,
                                                const double* __restrict__ gexp, int n_obs, int n_tsave, int k, int B,
                                                uint32_t dim, int overwrite, long obs_ostride, long obs_bstride) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= dim) return;
    const int b = blockIdx.y;
    const size_t o_ = size_t(b) * dim + x;
    double2 acc = overwrite ? make_double2(0.0, 0.0) : lam[o_];
    if (gstate) {
        const double2 g = gstate[o_];
        acc.x += g.x;
        acc.y += g.y;
    }
    if (gexp && n_obs > 0) {
        double wsum = 0.0;
        for (int o = 0; o < n_obs; ++o) wsum += gexp[(size_t(o) * n_tsave + k) * B + b] * obs[size_t(o) * obs_ostride + size_t(b) * obs_bstride + x];
        const double2 v = psi[o_];
        acc.x += 2.0 * wsum * v.x;
        acc.y += 2.0 * wsum * v.y;
    }
    lam[o_] = acc;
}

// which save points carry a non-zero expectation cotangent (a loss on the final time leaves all others empty):
// flags[k] = any_{o,b} gexp[o][k][b] != 0
__global__ void k_cotangent_flags(const double* __restrict__ gexp, int n_obs, int n_tsave, int B, int32_t* __restrict__ flags) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_tsave) return;
    int any = 0;
    for (int o = 0; o < n_obs; ++o)
        for (int b = 0; b < B; ++b) any |= gexp[(size_t(o) * n_tsave + k) * B + b] != 0.0;
    flags[k] = any;
}

// ------------------------------------------------------------------------------------------------
// K5: scatter per-exponential coefficient gradients back onto the sampled tables and tsave.
// one thread per (exponential, trajectory); atomics because several exponentials touch one sample.
// ------------------------------------------------------------------------------------------------
struct ScatterArgs {
    const double* ge;       // [Bc][E][kGradReplicas][NC+1]
    const StageDev* st;     // [E]
    const StageBwdDev* sb;  // [E] (only read when g_tsave)
    double inv_dt;          // d w1 / d t = -d w0 / d t = 1/dt   (hamiltonian.py:538,542)
    const double2* amp;     // tables (for d coef / d t)
    const double* det;
    double2* g_amp;
    double* g_det;
    double* g_tsave;
    int E, n_samples, Ka, Kd, NC, ga, gd;
    uint64_t amem[kMaxGroups], dmem[kMaxGroups];
};

__global__ void k_scatter_grads(ScatterArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= a.E) return;
    const double* reps = a.ge + (size_t(b) * a.E + e) * kGradReplicas * (a.NC + 1);
    double rec[2 * kMaxGroups + kMaxGroups + 1];
    for (int c = 0; c <= a.NC; ++c) {
        double sum = 0.0;
        for (int r = 0; r < kGradReplicas; ++r) sum += reps[size_t(r) * (a.NC + 1) + c];  // fixed order
        rec[c] = sum;
    }
    double dLdt = 0.0;
    const StageDev sd = a.st[e];
    const double wq[2] = {sd.w0, sd.w1};
    const int iq[2] = {sd.i0, sd.i1};
    const double dwq[2] = {a.g_tsave ? -a.inv_dt : 0.0, a.g_tsave ? a.inv_dt : 0.0};
    for (int k = 0; k < a.Ka; ++k) {
        double gr = 0.0, gi = 0.0;
        for (int g = 0; g < a.ga; ++g)
            if (a.amem[g] >> k & 1ull) {
                gr += rec[g];
                gi += rec[a.ga + g];
            }
        const double2* t = a.amp + (size_t(b) * a.Ka + k) * a.n_samples;
        for (int q = 0; q < 2; ++q) {
            const double w = wq[q], dw = dwq[q];
            const int i = iq[q];
            if (a.g_amp && w != 0.0) {
                double* dst = reinterpret_cast<double*>(a.g_amp + (size_t(b) * a.Ka + k) * a.n_samples + i);
                unsafeAtomicAdd(dst, w * gr);
                unsafeAtomicAdd(dst + 1, w * gi);
            }
            if (dw != 0.0) dLdt += dw * (gr * t[i].x + gi * t[i].y);
        }
    }
    for (int k = 0; k < a.Kd; ++k) {
        double gd = 0.0;
        for (int g = 0; g < a.gd; ++g)
            if (a.dmem[g] >> k & 1ull) gd += rec[2 * a.ga + g];
        const double* t = a.det + (size_t(b) * a.Kd + k) * a.n_samples;
        for (int q = 0; q < 2; ++q) {
            const double w = wq[q], dw = dwq[q];
            const int i = iq[q];
            if (a.g_det && w != 0.0) unsafeAtomicAdd(a.g_det + (size_t(b) * a.Kd + k) * a.n_samples + i, 2.0 * w * gd);
            if (dw != 0.0) dLdt += dw * 2.0 * gd * t[i];
        }
    }
    if (a.g_tsave) {
        const StageBwdDev sb = a.sb[e];
        const double gtau = rec[a.NC] * sb.tau_scale;
        if (sb.tn0 >= 0) unsafeAtomicAdd(a.g_tsave + sb.tn0, dLdt * sb.tnw0);
        if (sb.tn1 >= 0) unsafeAtomicAdd(a.g_tsave + sb.tn1, dLdt * sb.tnw1);
        if (sb.t_hi >= 0) unsafeAtomicAdd(a.g_tsave + sb.t_hi, gtau);
        if (sb.t_lo >= 0) unsafeAtomicAdd(a.g_tsave + sb.t_lo, -gtau);
    }
}

// ------------------------------------------------------------------------------------------------
// Host metadata -> device WITHOUT a copy engine or a synchronisation: the words travel as kernel arguments (the runtime
// copies them into the launch packet before hipLaunchKernel returns, so the host buffer may die right away) and one
// small workgroup writes them out.  Used for the per-exponential records (24 / 40 bytes each) and the pair tables.
// ------------------------------------------------------------------------------------------------
constexpr int kUploadWords = 448;  // 3584 bytes of payload per launch (kernel arguments are limited to 4 KiB)
struct UploadChunk {
    unsigned long long w[kUploadWords];
};

__global__ __launch_bounds__(256) void k_upload(unsigned long long* __restrict__ dst, UploadChunk c, int n) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.w[i];
}
