// runtime.hpp — planning glue between the C ABI and the kernel families (included by rydiff.hip after the kernel headers): the
// decoded problem (Runtime), tile geometry of the chained passes, the common prologue of every call (prepare), tape maps, the
// factor list of a time step and the launch-argument fills that several families share.
#pragma once

// ---- tile geometry of the chained passes (chain_kernels.hpp) ---------------------------------------------------------
// Tile layouts: every layout keeps a contiguous low run of amplitudes so that global accesses stay coalesced.  LT = tile bits:
// 12 (k_chain: 64 KiB of LDS, 4 amplitudes per thread at 1024 threads) or 13 (k_chain_wide: 128 KiB, two register halves).
//   two layouts:    A = [0,LT)            B = [0,2LT-N) u [LT,N)
//   three layouts:  A = [0,LT)            B = [0,LT-8) u [LT,LT+8)        C = [0,2LT+8-N) u [LT+8,N)
// With three layouts a factor takes two launches (start in A or C, middle pass in B, finish in C or A — the finishing
// launch also starts the next factor), 4R+3W instead of 2R+2W: still far better than 16-byte runs in a two-layout B.
// Which (LT, layout count) a chain uses: chain_geom() below.
struct LayoutDesc {
    int lo, hs, hb;
    uint32_t bits;  // amplitude-index bits covered by the tile
};

struct ChainGeom {
    int lt;       // tile bits: kTileBits (12) or kWideTileBits (13)
    int layouts;  // 2 or 3
};

// split-diagonal tables of one tile size: [3 layouts][2^LT + tiles * 16] doubles; one set per tile size (plan.hpp: off_split)
double* split_tables(const Plan& pl, char* ws, int lt) {
    return reinterpret_cast<double*>(ws + pl.off_split) + pl.split_off_doubles[lt - kSmallTileBits];
}

LayoutDesc chain_layout(int N, int which, const ChainGeom& g) {
    LayoutDesc d{};
    const bool three = g.layouts == 3;
    if (which == 0) {  // A
        d.lo = g.lt;
        d.hs = g.lt;
        d.hb = 0;
    } else if (which == 1) {  // B
        d.hs = g.lt;
        d.hb = three ? 8 : N - g.lt;
        d.lo = g.lt - d.hb;
    } else {  // C (three-layout mode only)
        d.hs = g.lt + 8;
        d.hb = N - d.hs;
        d.lo = g.lt - d.hb;
    }
    d.bits = ((1u << d.lo) - 1u) | (((1u << d.hb) - 1u) << d.hs);
    return d;
}

namespace {

struct Runtime {
    Plan pl;
    PolyDesign poly;
    double sigma = 0.0, width = 1.0, rho_design = 1.0;
    int64_t total_factors = 0;
    int max_step_factors = 0;
    int flags = 0;
    bool real_amp_grad = false;  // RydProblem.real_amp_grad: dL/dIm(amp) is not wanted
    bool prefer_direct = false;  // few tiles in flight: one-amplitude-per-thread kernels instead of the chained tile passes
    bool small_tiles = false;    // ~2^19 amplitudes in flight: chained passes on tiles of 2^11 amplitudes (256 tiles: one per CU)
    // RydProblem.kernel_variant decoded (include/rydiff.h); nothing about the kernel choice lives outside this struct
    int variant = 0;              // 0 auto | 1 direct | 2..4 chained tiles | 8 auto with LDS-tile kernels below 7 qubits
    bool generic_direct = false;  // variant 9: direct kernels without the unrolled global-drive instantiations
    bool plain_tile_order = false;  // variant 12: no line-sharing tile swizzle (ChainArgs.tile_swz)
    int force_three = 0;          // 1: variant 7, three tile layouts wherever they are legal; 2: variant 11, two layouts up to 24 qubits
    int tile_mode = 0;            // 0 automatic | 12: variant 13, 2^12-amplitude tiles everywhere | 13: variant 14, wide tiles from 14 qubits
                                  // 11 / 10: variants 15 / 16, tiles of 2^11 / 2^10 amplitudes where two layouts are legal
    bool force_xcd = false;       // variant 10: trajectory-per-XCD placement of the chained tiles forced
    int pair_mode = 0;            // block-of-two passes (k_chain2, k_chain2_bwd): 0 automatic | 1 variant 17, wherever legal | -1 variant 18, never
    bool pair_bwd_off = false;    // variant 19: automatic, but one factor per adjoint launch (k_chain)
    int pair_bwd_stage = 0;       // tape vectors of k_chain2_bwd: 0 automatic | -1 variant 20, through registers | 1 variant 21, by LDS-DMA
    int pair_phases = -1;         // request order and store policy of the block kernels: -1 automatic | variants 22..30: 4 * ORD + WT (pair_launch.hpp)
    int pair_pace_fwd = -1;       // paced input requests of k_chain2 (its PACE): -1 automatic | 0 variants 17, 20..30, 32 | 1 variants 31, 33 | 2 variant 34
    int pair_pace_bwd = -1;       // ... of k_chain2_bwd: -1 automatic | 0 variants 17, 20..31, 34 | 1 variants 32, 33
    int pair_wtape = 0;           // mid-block tape entry of the block passes (pair_launch.hpp): 0 automatic | 1 variant 35, P_X v | -1 variants 17, 19..34: v_mid
    int chain_lgt = 9;            // log2(threads per tile workgroup) of explicitly chosen chained variants
    // state-sharded run: where the partner slabs arrive and who moves them (RydProblem.shard_recv / shard_exchange)
    void* const* shard_recv = nullptr;
    int (*shard_exchange)(void*, int, const void*, size_t) = nullptr;
    void* shard_user = nullptr;
    GroupArgs garg{};
    PairArgs parg{};
    XyArgs xarg{};               // XY exchange (xy_kernels.hpp); mode 0: none
    double* xy_ge = nullptr;     // rydiff_backward with g_xy: the gradient replicas in the workspace

    // strides of the per-exponential records in the workspace (doubles; 0 between trajectories: one record shared by the batch)
    long coef_bstride() const { return pl.Bc > 1 ? long(pl.stages.size()) * pl.NC : 0; }
    long ge_rec() const { return long(kGradReplicas) * (pl.NC + 1); }  // gradient record of one exponential: [replica][NC + 1]
    long ge_bstride() const { return pl.Bc > 1 ? long(pl.stages.size()) * ge_rec() : 0; }
    // observable table [n_obs][dim]; state-sharded runs: one slab per rank of the call, [n_obs][B][dim]
    long obs_bstride() const { return pl.shard_bits ? long(pl.dim) : 0; }
    long obs_ostride() const { return pl.shard_bits ? long(pl.B) * long(pl.dim) : long(pl.dim); }
    // doubles of one layout's split-diagonal table at tile size 2^lt: [2^lt] + [tiles][16]
    size_t per_layout(int lt) const { return (size_t(1) << lt) + size_t((size_t(1) << pl.N) >> lt) * 16; }
    const double* coef(const char* ws, int stage) const { return reinterpret_cast<const double*>(ws + pl.off_coef) + size_t(stage) * pl.NC; }
    double* ge(char* ws, int stage) const { return reinterpret_cast<double*>(ws + pl.off_ge) + size_t(stage) * ge_rec(); }
};

// RydProblem.kernel_variant -> Runtime (include/rydiff.h lists the values)
int decode_variant(const RydProblem* p, Runtime& rt) {
    int v = p->kernel_variant;
    if (v < 0 || v > 35 || v == 5 || v == 6) return fail(RYDIFF_EINVAL, "kernel_variant must be 0..4 or 7..35");
    rt.pair_mode = (v == 17 || v >= 20) ? 1 : (v == 18 ? -1 : 0);
    rt.pair_bwd_off = v == 19;
    rt.pair_bwd_stage = (v == 21 || v == 29) ? 1 : (v >= 20 ? -1 : 0);
    // 22: requests vector-major | 23..25: write-through level 1..3 | 26..28: both | 29: vector-major with LDS-DMA staging | 30: neither
    // (17, 20 and 21 take the automatic combination)
    static constexpr int kPhases[9] = {4, 1, 2, 3, 5, 6, 7, 4, 0};
    rt.pair_phases = (v >= 22 && v <= 30) ? kPhases[v - 22] : -1;
    // 31..34: as 20 (register staging, the automatic order and store policy) with paced input requests: 31 forward | 32 adjoint |
    // 33 both | 34 forward, t requested before round A.  17 and 20..30 keep the unpaced kernels whatever the automatic choice is.
    const bool pair_forced = v == 17 || v >= 20;
    rt.pair_pace_fwd = (v == 31 || v == 33) ? 1 : (v == 34 ? 2 : (pair_forced ? 0 : -1));
    rt.pair_pace_bwd = (v == 32 || v == 33) ? 1 : (pair_forced ? 0 : -1);
    // 35: as 20, with P_X v on the tape between the two factors of a block (the adjoint block kernel rebuilds the mid-block state);
    // 17 and 19..34 keep v_mid there whatever the automatic choice is
    rt.pair_wtape = v == 35 ? 1 : ((pair_forced || v == 19) ? -1 : 0);
    if (v >= 17) v = 0;
    rt.generic_direct = v == 9;
    if (v == 9) v = 1;
    rt.force_three = v == 7 ? 1 : (v == 11 ? 2 : 0);
    rt.plain_tile_order = v == 12;
    rt.tile_mode = v == 13 ? 12 : (v == 14 ? 13 : (v == 15 ? 11 : (v == 16 ? 10 : 0)));
    if (v == 7 || v == 11 || v >= 12) v = 0;
    rt.force_xcd = v == 10;
    if (v == 10) v = 0;
    rt.variant = v;
    rt.chain_lgt = v == 3 ? 8 : (v == 4 ? 10 : 9);
    rt.shard_recv = p->shard_recv;
    rt.shard_exchange = p->shard_exchange;
    rt.shard_user = p->shard_user;
    return RYDIFF_OK;
}

// Tile size and layout count of the chained passes, forward and adjoint alike.  Measured on MI355X (profiles/r03_wide_tiles.txt): 2^13-amplitude tiles
// (k_chain_wide) win the forward and the adjoint passes at 21-24 qubits (two layouts up to 24: runs of 512 / 256 / 128 / 64 bytes);
// the adjoint WITH signed sums (drive phase gradients) works in register quarters there (in halves it spilled 37 VGPRs and lost at
// 21 and 24 qubits).  Explicit chained variants (2..4, 7, 10, 11) keep the 2^12 tiles they were written for.
ChainGeom chain_geom(const Runtime& rt) {
    const int N = rt.pl.NL;
    int lt = kTileBits;
    if (rt.pl.ga.flagged) lt = kTileBits;  // conditioned flips: sibling pairs must stay inside a tile (even lo and hs)
    else if (rt.tile_mode == 13) lt = N > kWideTileBits ? kWideTileBits : kTileBits;
    else if (rt.tile_mode == 10 || rt.tile_mode == 11) lt = (N > rt.tile_mode && N <= 2 * rt.tile_mode - 2) ? rt.tile_mode : kTileBits;  // two layouts, runs >= 64 bytes
    else if (rt.small_tiles) lt = 11;
    else if (rt.tile_mode == 0 && rt.variant == 0 && !rt.force_three && !rt.force_xcd && ((N >= 21 && N <= 24) || N >= 29))
        lt = kWideTileBits;  // (29, 30 qubits: three layouts of wide tiles keep runs of 512 / 256 bytes in the third; 2^12 tiles end at 28)
    ChainGeom g{lt, 2};
    if (lt == kWideTileBits) g.layouts = N <= 24 ? 2 : 3;
    else if (rt.force_three == 2 && N <= 24) g.layouts = 2;
    else if (N >= 23 || (rt.force_three == 1 && N >= 21)) g.layouts = 3;
    return g;
}

// metadata words -> device through kernel arguments (k_upload): asynchronous, the host buffer may die on return
int upload_words(hipStream_t stream, void* dst, const void* src, size_t bytes) {
    const size_t nwords = (bytes + 7) / 8;  // every destination region is 256-byte aligned and padded (plan.hpp: take)
    const unsigned char* sp = static_cast<const unsigned char*>(src);
    unsigned long long* dp = static_cast<unsigned long long*>(dst);
    for (size_t w0 = 0; w0 < nwords; w0 += kUploadWords) {
        const int n = int(std::min<size_t>(kUploadWords, nwords - w0));
        UploadChunk c;
        const size_t have = std::min<size_t>(size_t(n) * 8, bytes - w0 * 8);
        memcpy(c.w, sp + w0 * 8, have);
        if (have < size_t(n) * 8) memset(reinterpret_cast<unsigned char*>(c.w) + have, 0, size_t(n) * 8 - have);
        hipLaunchKernelGGL(k_upload, dim3(1), dim3(256), 0, stream, dp + w0, c, n);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

struct Runtime;
void assign_pauli_layouts(Runtime& rt);                                  // pauli_launch.hpp
int upload_pauli_tables(const Plan& pl, char* ws, hipStream_t stream);  // pauli_launch.hpp
int upload_dm_tables(const Plan& pl, char* ws, hipStream_t stream);     // dm_launch.hpp
int energy_prepare(const Runtime& rt, const RydProblem* p, char* ws, hipStream_t stream);  // energy_launch.hpp

std::mutex g_poly_mutex;
std::vector<PolyDesign> g_poly_cache;

PolyDesign cached_design(double rho, double tol) {
    std::lock_guard<std::mutex> lk(g_poly_mutex);
    for (const auto& d : g_poly_cache)
        if (d.rho == rho && d.tol == tol) return d;
    PolyDesign d = design_polynomial(rho, tol);
    if (g_poly_cache.size() > 64) g_poly_cache.clear();
    g_poly_cache.push_back(d);
    return d;
}

// detuning groups: amplitude-index bit masks and the count each group's occupation is measured from
template <class Masks, class Counts>
void fill_detuning(Masks& dmask, Counts& dcnt, const Plan& pl) {
    for (int g = 0; g < pl.gd.n; ++g) {
        dmask[g] = pl.gd.amp_index_mask[g];
        dcnt[g] = pl.gd.count[g];
    }
}

void fill_group_args(const Plan& pl, GroupArgs& g) {
    g.ga = pl.ga.n;
    g.gd = pl.gd.n;
    for (int q = 0; q < pl.ga.n; ++q) g.amask[q] = pl.ga.amp_index_mask[q];
    fill_detuning(g.dmask, g.dcnt, pl);
    g.cond = pl.ga.flagged;
}

// half width of the generator's numerical range (same widening as finish_runtime)
double generator_half_width(const Plan& pl, double lo, double hi) { return std::max(0.5 * (hi - lo), 1e-9) + pl.pair_radius; }

int64_t step_factor_count(const Runtime& rt, int k) {
    int64_t f = 0;
    for (int e = rt.pl.step_begin[k]; e < rt.pl.step_begin[k + 1]; ++e) f += int64_t(rt.pl.stages[e].nsub) * rt.poly.degree;
    return f;
}

// apply spectral bounds: sub-steps, design rho, polynomial, factor counts
int finish_runtime(Runtime& rt, double lo, double hi) {
    Plan& pl = rt.pl;
    if (!(hi >= lo) || !std::isfinite(hi) || !std::isfinite(lo)) return fail(RYDIFF_EINVAL, "non-finite spectral bounds (NaN/Inf in the coefficient tables?)");
    lo -= pl.pair_radius;  // dense two-qubit (dissipator) terms: keep the whole numerical range inside the design interval
    hi += pl.pair_radius;
    rt.sigma = 0.5 * (hi + lo);
    rt.width = std::max(0.5 * (hi - lo), 1e-9);
    double rho_d = 1e-6;
    for (auto& s : pl.stages) {
        const double rho = s.tau * rt.width;
        s.nsub = std::max(1, int(std::ceil(rho / kRhoCap)));
        rho_d = std::max(rho_d, rho / s.nsub);
    }
    // quantise rho upward a little so that optimisation epochs with slowly drifting tables reuse the cached design
    const double q = std::pow(2.0, std::ceil(std::log2(rho_d) * 16.0) / 16.0);
    rt.rho_design = q;
    rt.poly = cached_design(rt.rho_design, pl.tol);
    if (rt.poly.degree < 1 || rt.poly.roots.empty()) return fail(RYDIFF_EINVAL, "polynomial design failed");
    rt.total_factors = 0;
    rt.max_step_factors = 0;
    for (int k = 0; k < pl.T; ++k) {
        const int f = int(step_factor_count(rt, k));
        rt.total_factors += f;
        rt.max_step_factors = std::max(rt.max_step_factors, f);
    }
    fill_group_args(pl, rt.garg);
    if (pl.ga.flagged) {
        // conditioned flips (three-level registers): the one-launch kernels up to 12 qubits (their tile IS the register), beyond
        // that the generic one-amplitude-per-thread kernels (never the unrolled global-drive ones) while few tiles are in flight and
        // the chained passes on 2^12-amplitude tiles (sibling pairs stay inside a tile: chain_geom) beyond
        rt.generic_direct = true;
    }
    rt.parg.n = pl.n_pair;
    for (int t = 0; t < pl.n_pair; ++t) {
        rt.parg.ma[t] = pl.pair_ma[t];
        rt.parg.mb[t] = pl.pair_mb[t];
        unsigned dm = 0;  // relative flips present in the block or its conjugate transpose (PairArgs.dl)
        for (int w = 0; w < 2; ++w)
            for (int own = 0; own < 4; ++own)
                for (int s = 0; s < 4; ++s) {
                    const double* e = pl.pair_tab.data() + size_t(t) * 64 + size_t(w) * 32 + size_t(own * 4 + s) * 2;
                    if (e[0] != 0.0 || e[1] != 0.0) dm |= 1u << (own ^ s);
                }
        rt.parg.dl[t] = uint8_t(dm);
    }
    return RYDIFF_OK;
}

int run_stats(const RydProblem* p, const Plan& pl, void* scratch, hipStream_t stream, double& lo, double& hi, int& flags) {
    StatsArgs sa{};
    sa.amp = static_cast<const double2*>(p->amp_tables);
    sa.det = p->det_tables;
    sa.u_pairs = p->u_pairs;
    sa.xy_pairs = pl.xy_mode ? p->xy_pairs : nullptr;
    sa.n_samples = pl.n_samples;
    sa.Ka = pl.Ka;
    sa.Kd = pl.Kd;
    sa.n_pairs = pl.N * (pl.N - 1) / 2;
    sa.Bc = pl.Bc;
    sa.ga = pl.ga.n;
    sa.gd = pl.gd.n;
    for (int g = 0; g < pl.ga.n; ++g) {
        sa.amem[g] = pl.ga.members[g];
        sa.acnt[g] = pl.ga.count[g];
    }
    for (int g = 0; g < pl.gd.n; ++g) {
        sa.dmem[g] = pl.gd.members[g];
        sa.dcnt[g] = pl.gd.nq[g];
    }
    sa.dones = pl.gd.flagged;
    HIP_TRY(hipMemsetAsync(scratch, 0, 8 * sizeof(double), stream));
    const int ns = std::max(pl.n_samples, 1);
    dim3 grid((ns + 127) / 128, pl.Bc);
    hipLaunchKernelGGL(k_table_stats, grid, dim3(128), 0, stream, static_cast<unsigned long long*>(scratch), sa);
    LAUNCH_CHECK();
    double host[7] = {0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(host, scratch, sizeof(host), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the ONE synchronisation of the library: the bounds decide how many launches follow
    // interpolation weights: KRYLOV_SE uses convex combinations (sum |w| = 1); keep the general bound
    double wsum = 1.0;
    for (const auto& s : pl.stages) {
        double a = 0.0;
        for (int q = 0; q < 4; ++q) a += std::fabs(s.w[q]);
        wsum = std::max(wsum, a);
    }
    // Gershgorin: the diagonal ranges over [-sum of negative U_ij, +sum of positive U_ij] (occupations are 0/1) plus the
    // detuning range; the flip part has norm host[0] exactly (commuting single-qubit terms)
    hi = host[3] + wsum * (host[1] + host[0]);
    lo = -host[5] - wsum * (host[2] + host[0]);
    // XY exchange: every row of it sums to at most sum |J_ij| in absolute value — Gershgorin for the Hermitian mode; in the
    // one-directional mode the same number bounds the numerical range (row and column sums alike), as pair_radius does for
    // non-Hermitian pair terms.  Folded into the reported interval, so a call that is handed the plan needs no second look.
    hi += host[6];
    lo -= host[6];
    flags = (host[4] != 0.0) ? 1 : 0;  // bit 0: some flip coefficient has a non-zero imaginary part (phase != 0)
    return RYDIFF_OK;
}

// A tile pass keeps one CU busy for ~10 us per tile whatever the register size, so with few tiles in flight (one 13..18-qubit
// trajectory: 2..64 tiles on 256 CUs) the one-amplitude-per-thread kernels, which spread over the whole chip, are faster.
// Measured crossover (tools/time_small.py, bench.py --workload c4 --batch b, variants 0 / 1): forward-only runs up to 2^18
// amplitudes in flight (N=13: 5.3 vs 9.4 us per pass, N=16 B=4: +13 %), and the same with gradients since the direct kernels
// keep the full tape too and have unrolled instantiations for one global drive (N=18, 200 steps: 50 ms vs 69 ms chained; N=19:
// 83 vs 78 ms).  Explicit kernel variants are left alone (A/B tests).
// Around 2^19 amplitudes in flight (one 19-qubit trajectory, 2 x 18, 4 x 17, 8 x 16 ...) tiles of 2^11 amplitudes give 256 tiles — one
// per CU — where 2^12 tiles fill half of the chip and the direct kernels move every partner through the fabric: forward pass
// 10.8-11.1 -> 9.0 us, fwd+grad +10 ... +20 % (profiles/r03_small_tiles.txt).  Forward-only runs: the whole range (2^18, 2^19]; with
// gradients from 7 * 2^16 amplitudes and 14 qubits on (below, the direct adjoint stays ahead).  Automatic choice only.
bool small_tiles_win(const Runtime& rt, bool with_gradients) {
    const Plan& pl = rt.pl;
    if (rt.pair_mode == 1 || rt.variant != 0 || rt.force_three || rt.force_xcd || rt.tile_mode != 0 || pl.shard_bits || pl.n_pair || pl.ga.flagged) return false;
    if (pl.N < 13 || pl.N > 19) return false;
    const size_t amps = size_t(pl.B) << pl.N;
    if (amps > (size_t(1) << 19)) return false;
    return with_gradients ? (amps >= (size_t(7) << 16) && pl.N >= 14) : amps > (size_t(1) << 18);
}

bool few_tiles(const Runtime& rt, bool with_gradients) {
    const Plan& pl = rt.pl;
    if (rt.small_tiles) return false;
    if (rt.pair_mode == 1 || rt.variant != 0 || rt.force_three || rt.force_xcd || (rt.tile_mode != 0 && rt.tile_mode != kTileBits) || pl.shard_bits) return false;
    // forward only: crossover at 2^18 amplitudes in flight (N = 19: 12.5 us direct vs 10.8 us chained per pass).  With gradients the
    // direct ADJOINT pass (own tape element only, partner reads of the cotangent served by L2) stays ahead of the chained one up to
    // 2^19 (11.6-12.8 vs 14.0-14.7 us) and the pair of passes wins by 1-7 % there (profiles/r02_crossover_direct_vs_chained.txt);
    // at 2^20 (C3, C4's 16 x 2^16) the chained tiles win both passes.
    return (size_t(pl.B) << pl.N) <= (size_t(1) << (with_gradients ? 19 : 18));
}

// The full per-factor tape (the adjoint sweep recomputes nothing) goes with the launch-per-factor ADJOINT kernels, chained or
// direct (12 qubits: the one-launch forward sweep writes it); up to 11 qubits the adjoint sweep is one launch too and keeps
// one state per tsave.
// ... and the one-launch adjoint sweeps (<= 11 qubits), which in tape mode walk the factors without recomputing anything.
bool full_tape_possible(const Plan& pl) {
    if (pl.shard_bits || pl.xy_mode) return false;  // (the exchange: direct kernels, one state per tsave, as for pair terms past 11 qubits)
    if (pl.N <= kPersistBwdMaxQubits) return pl.ga.n <= kPersistGroups && pl.gd.n <= kPersistGroups;
    return pl.n_pair == 0;
}

// PARTIAL tape (need_tape = 3, RydProblem.tape_steps = K): region A = one state per tsave (T + 1 entries, as tape mode 1), region B = the
// intermediate factor outputs (every factor output that is not a step's last) of the LAST K tsave intervals, in run order.  The adjoint
// sweep recomputes the factor inputs of the earlier intervals only.  What the full tape is to a run that fits in HBM, this is to the
// part of a run that fits.  Launch-per-factor sweeps only (13 qubits and up; no pair terms, not sharded).
bool partial_tape_possible(const Runtime& rt) {
    return full_tape_possible(rt.pl) && rt.pl.N > kTileBits;
}

struct TapeMap {
    int k0 = 0;                     // first tsave interval whose intermediate factor outputs are on the tape
    std::vector<int64_t> bprefix;   // [T + 1]: region-B entries before interval k (0 up to k0)
    int64_t entries = 0;            // region A + region B
};

TapeMap partial_tape_map(const Runtime& rt, int tape_steps) {
    const Plan& pl = rt.pl;
    TapeMap m;
    m.k0 = std::max(0, pl.T - std::max(tape_steps, 0));
    m.bprefix.assign(pl.T + 1, 0);
    for (int k = 0; k < pl.T; ++k) m.bprefix[k + 1] = m.bprefix[k] + (k >= m.k0 ? std::max<int64_t>(step_factor_count(rt, k) - 1, 0) : 0);
    m.entries = int64_t(pl.T + 1) + m.bprefix[pl.T];
    return m;
}

// What rydiff_plan and the prologue of forward / backward share: plan, spectral bounds (from `info`, else measured with `scratch`:
// the one device wait), stage list at the known width, polynomial, tape mode granted, workspace layout (its size in `need`).
int plan_runtime(const RydProblem* p, const RydPlanInfo* info, void* scratch, size_t scratch_bytes, int& need_tape, bool need_backward,
                 hipStream_t stream, Runtime& rt, double& lo, double& hi, size_t& need) {
    std::string err;
    if (!p) return fail(RYDIFF_EINVAL, "null problem");
    int rc = decode_variant(p, rt);
    if (rc) return rc;
    if (!build_plan(p, rt.pl, err)) return fail(err.find("not implemented") != std::string::npos ? RYDIFF_ENOTIMPL : RYDIFF_EINVAL, err);
    if (!scratch) return fail(RYDIFF_EINVAL, "null workspace");
    if (info) {
        lo = info->spectral_lo;
        hi = info->spectral_hi;
        rt.flags = info->flags;
    } else {
        if (scratch_bytes < RYDIFF_PLAN_SCRATCH_BYTES) return fail(RYDIFF_EWORKSPACE, "workspace too small");
        rc = run_stats(p, rt.pl, scratch, stream, lo, hi, rt.flags);
        if (rc) return rc;
    }
    rt.real_amp_grad = p->real_amp_grad != 0;
    rt.xarg.mode = rt.pl.xy_mode;
    rt.xarg.N = rt.pl.N;
    rt.xarg.J = rt.pl.xy_mode ? p->xy_pairs : nullptr;
    // the stage list of the continuous solver depends on the spectral width: rebuild it now that the width is known
    if (!build_plan(p, rt.pl, err, generator_half_width(rt.pl, lo, hi))) return fail(RYDIFF_EINVAL, err);
    rc = finish_runtime(rt, lo, hi);
    if (rc) return rc;
    if (need_tape == 2 && !full_tape_possible(rt.pl)) need_tape = 1;  // full tape only with chained passes
    if (need_tape == 3 && (!partial_tape_possible(rt) || p->tape_steps < 1)) need_tape = 1;
    rt.small_tiles = small_tiles_win(rt, need_backward || need_tape != 0);
    rt.prefer_direct = few_tiles(rt, need_backward || need_tape != 0);
    need = carve(rt.pl, need_tape, need_backward, std::max(rt.max_step_factors - 1, 1), rt.total_factors,
                 need_tape == 3 ? partial_tape_map(rt, p->tape_steps).entries : 0);
    return RYDIFF_OK;
}

// K0 on one set of tables: per-exponential coefficient records [Bc][E][NC] into `coef`, from the StageDev records already in the
// workspace.  A nullptr table is a zero table (its terms are left out of the sums): the tangent sweep hands in tangent tables.
// launch_expand_at: the same for E records `st` on the device and tables of n_samples samples (the energy block's save-point records).
int launch_expand_at(const Plan& pl, const StageDev* st, size_t E, int n_samples, const double2* amp, const double* det, double* coef,
                     hipStream_t stream) {
    ExpandArgs ea{};
    ea.amp = amp;
    ea.det = det;
    ea.st = st;
    ea.coef = coef;
    ea.E = int(E);
    ea.n_samples = n_samples;
    ea.Ka = amp ? pl.Ka : 0;
    ea.Kd = det ? pl.Kd : 0;
    ea.NC = pl.NC;
    ea.ga = pl.ga.n;
    ea.gd = pl.gd.n;
    for (int g = 0; g < pl.ga.n; ++g) ea.amem[g] = pl.ga.members[g];
    for (int g = 0; g < pl.gd.n; ++g) ea.dmem[g] = pl.gd.members[g];
    hipLaunchKernelGGL(k_expand_coeffs, dim3((unsigned(E) + 127) / 128, pl.Bc), dim3(128), 0, stream, ea);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

int launch_expand(const Plan& pl, char* ws, const double2* amp, const double* det, double* coef, hipStream_t stream) {
    return launch_expand_at(pl, reinterpret_cast<const StageDev*>(ws + pl.off_meta_idx), pl.stages.size(), pl.n_samples, amp, det, coef, stream);
}

// common prologue of forward / backward: plan_runtime, upload metadata, expand coefficients, udiag.
// With `info` given nothing in here waits for the device.
int prepare(const RydProblem* p, const RydPlanInfo* info, void* workspace, size_t workspace_bytes, int need_tape,
            bool need_backward, hipStream_t stream, Runtime& rt) {
    double lo, hi;
    size_t need;
    int rc = plan_runtime(p, info, workspace, workspace_bytes, need_tape, need_backward, stream, rt, lo, hi, need);
    if (rc) return rc;
    Plan& pl = rt.pl;
    if (pl.shard_bits && pl.n_pair)
        return fail(RYDIFF_ENOTIMPL, "state-sharded runs do not take dense pair terms");
    if (pl.shard_bits) rt.generic_direct = true;  // (the unrolled direct kernels know nothing about rank qubits)
    if (workspace_bytes < need)
        return fail(RYDIFF_EWORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes, got " + std::to_string(workspace_bytes));
    char* ws = static_cast<char*>(workspace);
    const size_t E = pl.stages.size();
    {   // per-exponential records -> device (as kernel arguments: no copy engine, no synchronisation)
        std::vector<StageDev> sd(E);
        for (size_t e = 0; e < E; ++e) sd[e] = {pl.stages[e].w[0], pl.stages[e].w[1], pl.stages[e].idx[0], pl.stages[e].idx[1]};
        rc = upload_words(stream, ws + pl.off_meta_idx, sd.data(), E * sizeof(StageDev));
        if (rc) return rc;
    }
    if (pl.n_pair) {
        rc = upload_words(stream, ws + pl.off_pair, pl.pair_tab.data(), pl.pair_tab.size() * sizeof(double));
        if (rc) return rc;
        rt.parg.tab = reinterpret_cast<const double2*>(ws + pl.off_pair);
    }
    if (pl.n_pobs) {
        assign_pauli_layouts(rt);
        rc = upload_pauli_tables(pl, ws, stream);
        if (rc) return rc;
    }
    if (pl.dm_n) {
        rc = upload_dm_tables(pl, ws, stream);
        if (rc) return rc;
    }
    if (pl.NC > 0) {
        const int rc2 = launch_expand(pl, ws, static_cast<const double2*>(p->amp_tables), p->det_tables,
                                      reinterpret_cast<double*>(ws + pl.off_coef), stream);
        if (rc2) return rc2;
    }
    rc = energy_prepare(rt, p, ws, stream);
    if (rc) return rc;
    double* udiag = reinterpret_cast<double*>(ws + pl.off_udiag);
    if (pl.N > 1) {
        if (pl.shard_bits)  // one table per slab, evaluated at the global index
            hipLaunchKernelGGL(k_build_udiag, dim3((pl.dim + 255) / 256, pl.B), dim3(256), 0, stream, udiag, p->u_pairs, pl.N, uint32_t(pl.dim),
                               pl.NL, pl.rank_first);
        else
            hipLaunchKernelGGL(k_build_udiag, dim3((pl.dim + 255) / 256), dim3(256), 0, stream, udiag, p->u_pairs, pl.N, uint32_t(pl.dim));
        LAUNCH_CHECK();
    } else {
        HIP_TRY(hipMemsetAsync(udiag, 0, pl.dim * sizeof(double), stream));
    }
    if (pl.NL > kTileBits && pl.NL <= 30) {  // split diagonal for the tile layouts of the chained passes
        // (sharded runs: the layouts of the NL slab qubits, rows for every tile of the WHOLE register — rank bits on top)
        const ChainGeom g = chain_geom(rt);
        const unsigned tiles = unsigned((size_t(1) << pl.N) >> g.lt);
        const size_t tile_amps = size_t(1) << g.lt;
        double* split = split_tables(pl, ws, g.lt);
        for (int l = 0; l < g.layouts; ++l) {
            const LayoutDesc d = chain_layout(pl.NL, l, g);
            double* utt = split + l * rt.per_layout(g.lt);
            hipLaunchKernelGGL(k_build_split, dim3(unsigned((tile_amps + tiles + 255) / 256)), dim3(256), 0, stream, utt, utt + tile_amps,
                               p->u_pairs, pl.N, d.lo, d.hs, d.hb, tiles, g.lt);
            LAUNCH_CHECK();
        }
    }
    return RYDIFF_OK;
}

struct FactorScalars {
    double gr, gi, br, bi;
};

// state-sharded run with partner ranks elsewhere: tell the caller which slab the partners need next (phase 0, right after the
// launch that produced it) and when the received slabs are about to be read (phase 1); see RydProblem.shard_exchange
int shard_signal(const Runtime& rt, int phase, const void* src) {
    if (!rt.pl.shard_bits || rt.pl.shard_self) return RYDIFF_OK;
    if (rt.shard_exchange(rt.shard_user, phase, src, rt.pl.dim * sizeof(double2)) != 0)
        return fail(RYDIFF_EHIP, phase == 0 ? "shard_exchange failed to post the slab exchange" : "shard_exchange failed to wait for the partner slabs");
    return RYDIFF_OK;
}

// scalars of factor f of one sub-exponential of duration tau_sub
FactorScalars factor_scalars(const Runtime& rt, double tau_sub, int f) {
    using cd = std::complex<double>;
    const cd z = rt.poly.roots[f];
    // p(x) ~ exp(-i*rho_d*x) with x = tau_sub*(H - sigma)/rho_d, spectrum of x inside [-1,1] because
    // tau_sub*width <= rho_d.  One factor: (1 - x/z) = [1 + tau_sub*sigma/(rho_d z)] - [tau_sub/(rho_d z)] H
    const cd denom = rt.rho_design * z;
    cd beta = -tau_sub / denom;
    cd gamma = cd(1.0, 0.0) + tau_sub * rt.sigma / denom;
    if (f == rt.poly.degree - 1) {
        const cd kappa = std::exp(cd(0.0, -tau_sub * rt.sigma)) * rt.poly.p0;
        beta *= kappa;
        gamma *= kappa;
    }
    return {gamma.real(), gamma.imag(), beta.real(), beta.imag()};
}

struct ChainItem {
    int stage;
    FactorScalars s;
};

void build_step_chain(const Runtime& rt, int k, std::vector<ChainItem>& chain) {
    chain.clear();
    const Plan& pl = rt.pl;
    for (int e = pl.step_begin[k]; e < pl.step_begin[k + 1]; ++e) {
        const Stage& st = pl.stages[e];
        const double tau_sub = st.tau / st.nsub;
        for (int s = 0; s < st.nsub; ++s)
            for (int f = 0; f < rt.poly.degree; ++f) chain.push_back({e, factor_scalars(rt, tau_sub, f)});
    }
}

// state-sharded runs: flip group behind every rank bit (index bit NL + k), -1 if that qubit is not driven
void shard_groups(const Plan& pl, int (&grp)[kShardMaxBits]) {
    for (int k = 0; k < kShardMaxBits; ++k) {
        grp[k] = -1;
        if (k >= pl.shard_bits) continue;
        for (int g = 0; g < pl.ga.n; ++g)
            if (pl.ga.amp_index_mask[g] >> (pl.NL + k) & 1u) grp[k] = g;
    }
}

// Cotangents of the Pauli-string and state-overlap observables: they ride the grad_states route — k_pauli_apply (pauli_launch.hpp)
// writes grad_states[k] + 2 sum_o g_o O_o psi_k into a workspace buffer, k_overlap_apply (overlap_launch.hpp) adds
// sum_o (gRe + i gIm)_o phi_o to it (or to grad_states[k] where no Pauli observable has a cotangent), and the injecting launch reads
// that buffer instead of grad_states[k]; k_rdm_apply (rdm_launch.hpp) adds sum_o ((G + G^dagger)_{A_o} (x) 1) psi_k the same way, and
// k_moments_apply (moments_launch.hpp) 2 q_k psi_k of the occupation-correlation rows, k_energy_bwd1 / k_energy_bwd2 (energy_launch.hpp)
// 2 H_k (g_E + g_M H_k) psi_k of the energy rows, k_dm_apply / k_dm_scatter (dm_launch.hpp) the
// cotangents of the density-matrix rows
struct PauliInject {
    const Runtime* rt = nullptr;
    char* ws = nullptr;
    hipStream_t stream = nullptr;
    const double2* gstate = nullptr;  // the caller's grad_states or nullptr
    // the blocks of grad_expect (ExpectRows::at, plan.hpp), or nullptr: no such rows
    const double* gexp = nullptr;     // Pauli
    const double* ov_gexp = nullptr;  // Overlap
    const double2* ov_targets = nullptr;
    const double* rdm_gexp = nullptr; // Rdm
    const double* moments_gexp = nullptr;  // Moments
    const double* energy_gexp = nullptr;   // Energy
    mutable int rc = 0;                    // the first failure of a cotangent launch that reports one (the energy passes), for rydiff_backward
    double* wtot = nullptr;                // the U_ij gradient weights of the backward call (the energy block's explicit dL/dU), or nullptr
    const double* dm_gexp = nullptr;  // DmTrace .. End: the first density-matrix row
    const double* dm_diag = nullptr;  // RydProblem.dm_diag / dm_fid_targets
    const double2* dm_phi = nullptr;
    double2* buf = nullptr;           // one state (one-launch adjoints: n_tsave states)
    std::function<const double2*(int)> state_at;  // the state at save point k
};
const double2* observable_cotangent(const PauliInject& pi, int k);  // overlap_launch.hpp

// cotangents handed to the backward call (fused injection, see ChainArgs / FactorBwdArgs)
struct InjectSource {
    const double2* gstate = nullptr;  // grad_states [n_tsave][B][dim] or nullptr
    const double* gexp = nullptr;     // grad_expect [n_obs][n_tsave][B] or nullptr
    const double* obs = nullptr;      // [n_obs][dim]
    int n_obs = 0;
    const PauliInject* pauli = nullptr;  // Pauli / overlap observables with a cotangent: replaces gstate
    bool any() const { return gstate || gexp || pauli; }
};

// the cotangents injected at save point k (fields of ChainArgs / Chain2BwdArgs / FactorBwdArgs); k < 0 or nothing handed in: none
template <class Args>
void fill_inject(Args& a, const InjectSource& inj, int k, const Plan& pl) {
    if (k < 0 || !inj.any()) return;
    if (inj.pauli) a.inj_gstate = observable_cotangent(*inj.pauli, k);  // (enqueued ahead of the launch these arguments are for)
    else a.inj_gstate = inj.gstate ? inj.gstate + size_t(k) * pl.B * pl.dim : nullptr;
    a.inj_gexp = inj.gexp ? inj.gexp + size_t(k) * pl.B : nullptr;
    a.inj_obs = inj.obs;
    a.inj_n_obs = inj.n_obs;
    a.inj_ostride = long(pl.T + 1) * pl.B;
}

// state-sharded run: slabs as trajectories, rank qubits as partner slabs (ChainArgs documents the fields)
template <class Args>
void fill_shard(Args& a, const Runtime& rt) {
    const Plan& pl = rt.pl;
    if (!pl.shard_bits) return;
    a.sh_bits = pl.shard_bits;
    a.sh_nl = pl.NL;
    a.sh_rank_first = pl.rank_first;
    a.sh_self = pl.shard_self ? 1 : 0;
    for (int k = 0; k < pl.shard_bits; ++k) a.sh_rem[k] = pl.shard_self ? nullptr : static_cast<const double2*>(rt.shard_recv[k]);
    shard_groups(pl, a.sh_grp);
}

// kernels with more than 64 KiB of dynamic LDS: raise the limit once per kernel and process (idempotent, so a race between two
// first callers is harmless)
template <auto Kernel>
int set_max_dynamic_lds_once(size_t bytes) {
    static std::atomic<bool> attr_set{false};
    if (!attr_set.load(std::memory_order_acquire)) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
        attr_set.store(true, std::memory_order_release);
    }
    return RYDIFF_OK;
}

// the trajectories a chain covers and how its launches are placed (Runtime::xcd_group)
struct BatchSlice {
    int first = 0, count = 0;
    bool xcd = false;  // trajectory-per-XCD placement + L2-resident in-place vectors
};

// ---- what the sweeps of one rydiff_forward / rydiff_backward call share ----------------------------------------------
struct SweepCtx {
    const Runtime& rt;
    const RydProblem* p;
    char* ws;
    hipStream_t stream;
    size_t sv;     // complex elements per saved state
    TapeMap tmap;  // partial tape only
    bool wtape = false;  // full tape: P_X v, not v_mid, between the two factors of a block (pair_wtape, pair_launch.hpp)
    bool full_tape() const { return rt.pl.tape_mode == 2; }
    bool partial_tape() const { return rt.pl.tape_mode == 3; }
};

struct ForwardCtx : SweepCtx {
    const double2* psi0 = nullptr;
    const double2* start = nullptr;  // psi0, or its copy in entry 0 of the tape
    double2* buf[2] = {};          // ping-pong vectors for factor outputs nobody keeps
    double2* tape = nullptr;       // where kept states go: states_out, or the workspace tape (full / partial tape: tape_mode 2 / 3)
    double2* tape_b = nullptr;     // region B of the partial tape
    double2* copy_out = nullptr;   // states_out when the states at the save points are copied out of the workspace tape
    double2* final_dst = nullptr;  // final_state_only: where the last state goes
    const double* obs = nullptr;
    double* expect_out = nullptr;
    bool want_exp = false;
    // the blocks of expect_out (ExpectRows::at, plan.hpp) where such rows are evaluated
    double* pauli_out = nullptr;   // Pauli
    double* overlap_out = nullptr; // Overlap
    double* rdm_out = nullptr;     // Rdm
    double* moments_out = nullptr; // Moments
    double* energy_out = nullptr;  // Energy
    double* moments_drec = nullptr;  // tangent sweep past 12 qubits: the tile records of the moment tangents (TangentLayout::off_dmoments)
    double* dm_out = nullptr;      // DmTrace .. End: the first density-matrix row
    const double* shot_u = nullptr;  // RydProblem.shot_uniforms / shots_out where shots are drawn (rydiff_forward with n_shots > 0)
    uint32_t* shots_out = nullptr;
};

struct BackwardCtx : SweepCtx {
    const double2* tape = nullptr;    // one entry per tsave, or (full tape) one per factor pass; partial tape: region B behind
    const double2* tape_b = nullptr;
    std::vector<int64_t> fprefix;     // [T + 1]: factors before interval k
    double2* lam[2] = {};             // cotangent ping-pong
    double2* chainbuf = nullptr;      // recomputed factor inputs of one interval
    double* ge = nullptr;             // per-exponential gradient records
    double* wtot = nullptr;           // U_ij gradient weights, or nullptr
    bool want_tau = false;            // g_tsave given: dL/dtau of every exponential
    InjectSource inj;
    PauliInject pauli;                // what inj.pauli points to
    bool taped(int k) const { return full_tape() || (partial_tape() && k >= tmap.k0); }  // every factor input of interval k is on the tape
    const double2* state_at(int k) const { return tape + size_t(full_tape() ? fprefix[k] : k) * sv; }  // the state at tsave[k]
};

}  // namespace
