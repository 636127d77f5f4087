// common.hpp — what every kernel family shares (included first by rydiff.hip): limits, error reporting, device helpers and the
// argument structs of the direct kernels (the tile kernels reuse GroupArgs / PairArgs and the injected-cotangent helper).
#pragma once

// ------------------------------------------------------------------------------------------------
// error handling
// ------------------------------------------------------------------------------------------------
// gradient accumulators are replicated so that concurrent blocks do not serialise on one address
constexpr int kGradReplicas = 64;
constexpr int kMaxRemote = 6;  // up to 2^6 GPUs in a state-sharded run
constexpr int kShardMaxBits = 6;  // natively driven sharded runs: up to 2^6 ranks

static thread_local std::string g_last_error;  // the only mutable per-thread state (include/rydiff.h: rydiff_last_error)

static int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(RYDIFF_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)

#define LAUNCH_CHECK()                                                                                 \
    do {                                                                                               \
        hipError_t _e = hipGetLastError();                                                             \
        if (_e != hipSuccess) return fail(RYDIFF_EHIP, std::string("kernel launch: ") + hipGetErrorString(_e)); \
    } while (0)

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
// HIP's __popc returns UNSIGNED: `count - __popc(x)` with count < popcount (a ones-counting detuning group has count 0) would wrap
__device__ __forceinline__ int popc_i(uint32_t v) { return int(__popc(v)); }

struct GroupArgs {
    int ga, gd;
    uint32_t amask[kMaxGroups];  // amplitude-index bit masks of the flip groups
    uint32_t dmask[kMaxGroups];  // amplitude-index bit masks of the detuning groups
    int dcnt[kMaxGroups];        // qubits per detuning group (0: the group counts ones, RydProblem.det_ones_terms)
    uint32_t cond;               // flip groups whose flips act only where the sibling qubit (index bit ^ 1) is 1 (amp_conditioned_terms)
};

// conditioned flip of index bit `bit` (one-hot): does it act on amplitude x?  Flip and sibling are different bits, so the partner
// x ^ bit passes the same test.
__device__ __forceinline__ bool flip_acts(uint32_t cond_groups, int q, uint32_t x, uint32_t bit) {
    if (!(cond_groups >> q & 1u)) return true;
    const uint32_t sib = (bit & 0x55555555u) ? (bit << 1) : (bit >> 1);
    return (x & sib) != 0u;
}

// dense two-qubit terms of the generator (include/rydiff.h: pair terms)
struct PairArgs {
    int n = 0;
    const double2* tab = nullptr;  // [n][2][16]: forward table, then its conjugate transpose
    uint32_t ma[RYDIFF_MAX_PAIR_TERMS];
    uint32_t mb[RYDIFF_MAX_PAIR_TERMS];
    // which relative flips delta = own ^ s the block of term t has at all (bit delta: some T[own][own ^ delta] != 0, in the block or its
    // conjugate transpose; bit 0 = the diagonal, 1 = flip b, 2 = flip a, 3 = flip both).  Collapse operators populate few of them —
    // dephasing (Z (x) Z) the diagonal only, relaxation / depolarizing the diagonal and the double flip — and the kernels skip the rest
    // uniformly: no coefficient reads, no partner reads.
    uint8_t dl[RYDIFF_MAX_PAIR_TERMS];
};

// sum_p sum_s T_p[4*own + s] * v[x with the pair's bits set to s];  which = 0: T, 1: T^dagger
__device__ __forceinline__ double2 pair_apply(const PairArgs& pa, int which, const double2* __restrict__ v, uint32_t x) {
    double2 acc = make_double2(0.0, 0.0);
    for (int t = 0; t < pa.n; ++t) {
        const uint32_t ma = pa.ma[t], mb = pa.mb[t];
        const int own = ((x & ma) ? 2 : 0) | ((x & mb) ? 1 : 0);
        const double2* __restrict__ row = pa.tab + (size_t(t) * 2 + which) * 16 + own * 4;
        const unsigned dm = pa.dl[t];
#pragma unroll
        for (int dlt = 0; dlt < 4; ++dlt) {
            if (!(dm >> dlt & 1u)) continue;  // uniform
            const double2 c = row[own ^ dlt];
            if (c.x == 0.0 && c.y == 0.0) continue;
            const double2 q = v[x ^ ((dlt & 2) ? ma : 0u) ^ ((dlt & 1) ? mb : 0u)];
            acc.x += c.x * q.x - c.y * q.y;
            acc.y += c.x * q.y + c.y * q.x;
        }
    }
    return acc;
}

// relative flips of one pair term whose partner loads are in flight together in pair_apply_all: PF * NV loads of 16 bytes per thread —
// the budget of the flip-bit chunks of the tangent sweep (tangent_kernels.hpp: TangentChunk), 15 / 14 / 18 loads at NV = 5 / 7 / 9
template <int NV>
struct PairFlips {
    static constexpr int value = NV <= 5 ? 3 : 2;
};

// pair_apply on NV vectors at once (vector i of the caller's trajectory at v + i * vstride; its own values own[i] = v_i[x] are in
// registers already):  acc_i += beta * sum_p sum_s T_p[4*own + s] * v_i[x with the pair's bits set to s].  The mask test per relative
// flip is wave-uniform (flips absent from dl[t] cost nothing), the coefficient T[own][own ^ dlt] is read ONCE and serves all NV
// vectors, dlt = 0 takes the own values, and the partner loads of a group of flips — of every vector — are issued together, before
// any sum consumes one.
template <int NV>
__device__ __forceinline__ void pair_apply_all(const PairArgs& pa, const double2* __restrict__ v, size_t vstride, uint32_t x,
                                               const double2 (&own)[NV], double br, double bi, double (&accr)[NV], double (&acci)[NV]) {
    constexpr int PF = PairFlips<NV>::value;
    for (int t = 0; t < pa.n; ++t) {  // uniform
        const uint32_t ma = pa.ma[t], mb = pa.mb[t];
        const unsigned dm = pa.dl[t];
        const int o = ((x & ma) ? 2 : 0) | ((x & mb) ? 1 : 0);
        const double2* __restrict__ row = pa.tab + size_t(t) * 32 + o * 4;  // the forward table
        if (dm & 1u) {  // uniform: the diagonal of the block on the own values
            const double2 c = row[o];
            const double kr = br * c.x - bi * c.y, ki = br * c.y + bi * c.x;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                accr[i] += kr * own[i].x - ki * own[i].y;
                acci[i] += kr * own[i].y + ki * own[i].x;
            }
        }
#pragma unroll
        for (int d0 = 1; d0 < 4; d0 += PF) {
            if (!((dm >> d0) & ((1u << PF) - 1u))) continue;  // uniform: none of this group's flips in the block
            double2 c[PF], part[PF][NV];
#pragma unroll
            for (int f = 0; f < PF; ++f) {
                const int dlt = d0 + f;
                if (dlt < 4 && (dm >> dlt & 1u)) {  // uniform
                    c[f] = row[o ^ dlt];
                    const uint32_t xp = x ^ ((dlt & 2) ? ma : 0u) ^ ((dlt & 1) ? mb : 0u);
#pragma unroll
                    for (int i = 0; i < NV; ++i) part[f][i] = v[size_t(i) * vstride + xp];
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // the scheduler may not sink a later flip's loads below the first flip's sums
#pragma unroll
            for (int f = 0; f < PF; ++f) {
                const int dlt = d0 + f;
                if (dlt < 4 && (dm >> dlt & 1u)) {  // uniform
                    const double kr = br * c[f].x - bi * c[f].y, ki = br * c[f].y + bi * c[f].x;
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        accr[i] += kr * part[f][i].x - ki * part[f][i].y;
                        acci[i] += kr * part[f][i].y + ki * part[f][i].x;
                    }
                }
            }
        }
    }
}

struct FactorArgs {
    const double2* xin;
    double2* xout;
    const double* udiag;
    const double* coef;   // record of this exponential, trajectory 0: c_re[ga], c_im[ga], dcoef[gd]
    long coef_bstride;    // doubles between trajectories' records (0: shared)
    uint32_t dim;
    double gr, gi, br, bi;  // gamma, beta
    GroupArgs g;
    // optional: coefficient record passed by value, and contributions of vectors owned by OTHER GPUs (state sharding):
    //   y += rc_k * remote_k[x]   (the flip terms of the qubits that select the GPU; see pulser-diff_amd/sharded.py)
    int use_inline;
    double coef_inline[3 * kMaxGroups];
    int n_remote;
    const double2* remote[kMaxRemote];
    double rc[2 * kMaxRemote];
    PairArgs pair;
    // state-sharded run driven natively (ChainArgs documents the fields): slabs as trajectories, rank qubits as partner slabs
    int sh_bits = 0, sh_nl = 0, sh_rank_first = 0, sh_self = 0;
    const double2* sh_rem[kShardMaxBits] = {};
    int sh_grp[kShardMaxBits] = {};
    // fused <y|O|y> of the vector this launch produces (k_factor_direct_global only; last factor of a time step)
    const double* obs = nullptr;   // [n_obs][dim]
    double* expect_slot = nullptr; // &expect_out[0][k][0]
    int n_obs = 0;
    long exp_ostride = 0;          // n_tsave * B
};

struct FactorBwdArgs {
    const double2* gin;   // cotangent w.r.t. the factor's output
    const double2* xin;   // the factor's input (recomputed chain)
    double2* gout;        // cotangent w.r.t. the factor's input
    const double* udiag;
    const double* coef;
    long coef_bstride;
    double* ge;           // gradient record of this exponential, trajectory 0, replica 0: gcre[ga], gcim[ga], gd[gd], gtau
    long ge_bstride;
    long ge_rstride;      // doubles between replicas (NC+1)
    double* wtot;         // optional [dim]: accumulates Re(beta*conj(g)*x) for the U_ij gradient
    uint32_t dim;
    double gr, gi, br, bi;
    GroupArgs g;
    PairArgs pair;
    // Fused cotangent injection (replaces a separate k_inject launch and the host-side decision whether one is needed):
    // when gout is the cotangent at a save point k — xin is then the state there — add
    //   grad_states[k][b][x] + 2 * sum_o grad_expect[o][k][b] * obs[o][x] * xin[x]
    const double2* inj_gstate = nullptr;  // grad_states[k] ([B][dim]) or nullptr
    const double* inj_gexp = nullptr;     // &grad_expect[0][k][0] or nullptr
    const double* inj_obs = nullptr;      // [n_obs][dim]
    int inj_n_obs = 0;
    long inj_ostride = 0;                 // n_tsave * B
    long obs_bstride = 0, obs_ostride = 0;  // observable table: [n_obs][dim] (0, dim); sharded: one slab per rank (dim, B * dim)
    // state-sharded run (ChainArgs documents the fields): the cotangent slabs of the partner ranks enter the adjoint matvec, and —
    // through the re-indexed contraction below — the drive gradients of the rank qubits
    int sh_bits = 0, sh_nl = 0, sh_rank_first = 0, sh_self = 0;
    const double2* sh_rem[kShardMaxBits] = {};
    int sh_grp[kShardMaxBits] = {};
};

// the injected cotangent at amplitude x of trajectory b (see FactorBwdArgs); wave-uniform control flow
__device__ __forceinline__ double2 injected_cotangent(const double2* inj_gstate, const double* inj_gexp, const double* inj_obs,
                                                      int n_obs, long ostride, long obs_ostride, long obs_bstride, int b, size_t boff,
                                                      uint32_t x, const double2& psi) {
    double2 add = make_double2(0.0, 0.0);
    if (inj_gexp) {
        double wsum = 0.0;
        for (int o = 0; o < n_obs; ++o) {
            const double ge = inj_gexp[o * ostride + b];
            if (ge != 0.0) wsum += ge * inj_obs[size_t(o) * obs_ostride + size_t(b) * obs_bstride + x];
        }
        add.x = 2.0 * wsum * psi.x;
        add.y = 2.0 * wsum * psi.y;
    }
    if (inj_gstate) {
        const double2 g = inj_gstate[boff + x];
        add.x += g.x;
        add.y += g.y;
    }
    return add;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// one value per block: wave shuffle -> LDS -> one global atomic
__device__ __forceinline__ void block_atomic_add(double v, double* dst, double* lds /* >= 4 doubles */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 0; w < nw; ++w) s += lds[w];
        unsafeAtomicAdd(dst, s);
    }
}
