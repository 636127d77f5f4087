// chain_launch.hpp — chained tile passes (chain_kernels.hpp): launch schedule, argument fill, forward and adjoint chain drivers.
#pragma once

namespace {

// ---- launch schedule (the layouts themselves: runtime.hpp) ----------------------------------------------------------
// One launch of a chain: which layout, which index bits the partial already covers, which factor's partial it extends
// (`fin`, -1: none; `completes`: the factor is complete afterwards) and which factor it starts (`sta`, -1: none).
struct KernelStep {
    int layout;
    uint32_t covered;
    int fin;
    bool completes;
    int sta;
};

void chain_schedule(int N, const ChainGeom& geom, int F, std::vector<KernelStep>& ks) {
    ks.clear();
    if (geom.layouts == 2) {
        for (int k = 0; k <= F; ++k)
            ks.push_back({k & 1, k > 0 ? chain_layout(N, (k - 1) & 1, geom).bits : 0u, k - 1, true, k < F ? k : -1});
        return;
    }
    const uint32_t bbits = chain_layout(N, 1, geom).bits;
    auto end_layout = [](int m) { return (m & 1) ? 2 : 0; };  // factor m starts in A (even m) or C (odd m)
    for (int m = 0; m <= F; ++m) {
        const uint32_t cov = m > 0 ? (chain_layout(N, end_layout(m - 1), geom).bits | bbits) : 0u;
        ks.push_back({end_layout(m), cov, m - 1, true, m < F ? m : -1});
        if (m < F) ks.push_back({1, chain_layout(N, end_layout(m), geom).bits, m, false, -1});
    }
}

uint32_t to_tile_mask(const LayoutDesc& d, int lt, uint32_t index_mask) {
    uint32_t m = 0;
    for (int b = 0; b < lt; ++b) {
        const int gb = b < d.lo ? b : d.hs + (b - d.lo);
        if (index_mask >> gb & 1u) m |= 1u << b;
    }
    return m;
}

bool chain_enabled(const Runtime& rt) {
    const int N = rt.pl.NL;
    if (rt.variant == 1 || rt.pl.n_pair || rt.pl.xy_mode) return false;  // pair terms, the XY exchange: direct kernels
    // conditioned flips (three-level registers): measured (tools/time_three_level.py) the chained passes win up to 20 qubits (10 atoms:
    // 29.6 -> 20.6 us per pass, fwd+grad +23 %); beyond, the 2^12 tiles' short runs / third layout and the 512-thread signed-sum adjoint
    // lose to the generic direct kernels (22 qubits: 758 vs 687 steps/s fwd+grad).  Explicit chained variants still take them (tests).
    if (rt.pl.ga.flagged && N > 20 && rt.variant == 0) return false;
    if (rt.pl.shard_bits) return N > kTileBits && chain_geom(rt).layouts == 2;  // sharded: two-layout chains on the slab qubits (<= 22; wide tiles: <= 24)
    return N > kTileBits && N <= (chain_geom(rt).lt == kWideTileBits ? 30 : 28) && !rt.prefer_direct;
}

struct ChainStep {
    // kernel j finishes factor `fin` (if has_p) and starts factor `sta` (if has_q)
    const double2* u;
    const double2* p;
    double2* v_out;
    double2* q_out;
    int fin_stage, sta_stage;
    FactorScalars fin, sta;
    int has_p, has_q, write_v;
    bool completes = true;  // the finish stage yields the complete vector (false: middle pass of a three-layout chain)
    int layout;
    uint32_t covered_bits = 0;  // index bits whose flips the incoming partial already contains
    // backward mode
    bool bwd = false;
    const double2* x_fin = nullptr;
    const double2* x_sta = nullptr;
    double cb_fin_r = 0, cb_fin_i = 0, cb_sta_r = 0, cb_sta_i = 0;
    double* wtot = nullptr;
    // fused cotangent injection (adjoint): save point the vector completed by this launch belongs to, -1: none
    int inject_k = -1;
    // fused expectation (forward)
    const double* obs = nullptr;
    double* expect_slot = nullptr;
    int n_obs = 0;
    long exp_ostride = 0;
};

// What launch k of a schedule is whatever the direction: layout, the complete vector it works on, the partials it reads and writes
// (pp0 / pp1 alternately).  L2-resident placement: partials are rewritten IN PLACE (a workgroup reads and writes only its own tile
// elements), so the live set of a trajectory is one complete vector + one partial.
ChainStep chain_step(const Plan& pl, char* ws, const KernelStep& st, size_t k, const double2* cur, const BatchSlice& bs) {
    double2* pp[2] = {reinterpret_cast<double2*>(ws + pl.off_pp0), reinterpret_cast<double2*>(ws + pl.off_pp1)};
    auto ppsel = [&](size_t j) { return bs.xcd ? pp[0] : pp[j & 1]; };
    ChainStep cs{};
    cs.layout = st.layout;
    cs.covered_bits = st.covered;
    cs.u = cur;
    cs.has_p = st.fin >= 0;
    cs.has_q = st.sta >= 0;
    cs.p = cs.has_p ? ppsel(k - 1) : nullptr;
    cs.q_out = cs.has_q ? ppsel(k) : nullptr;
    cs.write_v = cs.has_p;
    cs.completes = st.completes;
    if (cs.has_p && !st.completes) cs.v_out = ppsel(k);  // a middle pass hands the extended partial on
    return cs;
}

template <int LT, int LGT, bool CPLX, bool BWD, bool FAST = false, bool RES = false>
int launch_chain_t(const ChainArgs& ca, unsigned tiles, hipStream_t stream) {
    static_assert(LT == kTileBits || (LT >= kSmallTileBits && LT <= kWideTileBits && LGT == 10 && !RES), "other tile sizes: 1024 threads, no L2-resident placement");
    if constexpr (!FAST) {  // one global drive, at most one detuning group: the loop-free instantiation
        if (ca.ga == 1 && ca.sta_mask[0] == (1u << LT) - 1u && !ca.cond)  // (any number of detuning groups)
            return launch_chain_t<LT, LGT, CPLX, BWD, true, RES>(ca, tiles, stream);
    }
    // tile + reduction scratch: one double per wave (forward), [4 ga + gd] slots per wave (adjoint: parked gradient partials)
    const size_t nw = (size_t(1) << LGT) / 64;
    const size_t max_lds = (size_t(1) << LT) * sizeof(double2) + 256 + (BWD ? size_t(5) * kMaxGroups * nw * sizeof(double) : 0);
    const size_t lds = (size_t(1) << LT) * sizeof(double2) + 256 + (BWD ? size_t(4 * ca.ga + ca.gd) * nw * sizeof(double) : 0);
    constexpr auto kern = [] {
        // register halves — quarters for the adjoint with signed sums (k_chain<13, ...> would spill)
        if constexpr (LT == kWideTileBits) return &k_chain_wide<LT, CPLX, BWD, FAST, (BWD && CPLX) ? 2 : 4>;
        else return &k_chain<LT, LGT, CPLX, BWD, FAST, RES>;
    }();
    if (int rc = set_max_dynamic_lds_once<kern>(max_lds)) return rc;
    const dim3 grid = ca.xcd_place ? dim3(tiles * 8u, unsigned(ca.b_count + 7) / 8u) : dim3(tiles, unsigned(ca.b_count));
    hipLaunchKernelGGL(kern, grid, dim3(1 << LGT), lds, stream, ca);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

template <int LT, int LGT, bool RES = false>
int launch_chain_l(const ChainArgs& ca, unsigned tiles, bool cplx, bool bwd, hipStream_t stream) {
    // the adjoint needs both partner sums (plain and signed) unless the coefficients are real AND the caller only uses the
    // real part of the amplitude gradients (RydProblem.real_amp_grad): then `cplx` arrives false here
    if (bwd) return cplx ? launch_chain_t<LT, LGT, true, true, false, RES>(ca, tiles, stream) : launch_chain_t<LT, LGT, false, true, false, RES>(ca, tiles, stream);
    return cplx ? launch_chain_t<LT, LGT, true, false, false, RES>(ca, tiles, stream) : launch_chain_t<LT, LGT, false, false, false, RES>(ca, tiles, stream);
}

int launch_chain(const Runtime& rt, char* ws, const ChainStep& cs, const BatchSlice& bs, const InjectSource& inj, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const ChainGeom geom = chain_geom(rt);
    const LayoutDesc X = chain_layout(pl.NL, cs.layout, geom);
    ChainArgs ca{};
    ca.u = cs.u;
    ca.p = cs.p ? cs.p : cs.u;  // (always loadable: the kernel requests u, p and the tape vectors outside of control flow)
    ca.v_out = cs.v_out;
    ca.q_out = cs.q_out;
    ca.utt = split_tables(pl, ws, geom.lt) + size_t(cs.layout) * rt.per_layout(geom.lt);
    ca.vr = ca.utt + (size_t(1) << geom.lt);
    ca.coef_fin = rt.coef(ws, std::max(cs.fin_stage, 0));
    ca.coef_sta = rt.coef(ws, std::max(cs.sta_stage, 0));
    ca.coef_bstride = rt.coef_bstride();
    ca.fb_r = cs.fin.br;
    ca.fb_i = cs.fin.bi;
    ca.fg_r = cs.fin.gr;
    ca.fg_i = cs.fin.gi;
    ca.completes = (cs.has_p && cs.completes) ? 1 : 0;
    ca.sg_r = cs.sta.gr;
    ca.sg_i = cs.sta.gi;
    ca.sb_r = cs.sta.br;
    ca.sb_i = cs.sta.bi;
    ca.lo = X.lo;
    ca.hs = X.hs;
    ca.hb = X.hb;
    ca.dim = uint32_t(pl.dim);
    ca.has_p = cs.has_p;
    ca.has_q = cs.has_q;
    ca.write_v = cs.write_v;
    ca.ga = pl.ga.n;
    ca.gd = pl.gd.n;
    ca.cond = pl.ga.flagged;
    ca.xcd_place = bs.xcd ? 1 : 0;
    ca.resident = bs.xcd ? 1 : 0;
    ca.b_first = bs.first;
    ca.b_count = bs.count;
    for (int g = 0; g < pl.ga.n; ++g) {
        ca.fin_mask[g] = to_tile_mask(X, geom.lt, pl.ga.amp_index_mask[g] & ~cs.covered_bits);
        ca.sta_mask[g] = to_tile_mask(X, geom.lt, pl.ga.amp_index_mask[g]);
    }
    fill_detuning(ca.dmask, ca.dcnt, pl);
    ca.obs = cs.obs;
    ca.expect_slot = cs.expect_slot;
    ca.n_obs = cs.n_obs;
    ca.exp_ostride = cs.exp_ostride;
    ca.obs_bstride = rt.obs_bstride();
    ca.obs_ostride = rt.obs_ostride();
    fill_shard(ca, rt);
    if (cs.bwd) {
        ca.x_fin = cs.x_fin ? cs.x_fin : cs.u;
        ca.x_sta = cs.x_sta ? cs.x_sta : cs.u;
        ca.ge_fin = rt.ge(ws, std::max(cs.fin_stage, 0));
        ca.ge_sta = rt.ge(ws, std::max(cs.sta_stage, 0));
        ca.ge_bstride = rt.ge_bstride();
        ca.ge_rstride = pl.NC + 1;
        ca.cb_fin_r = cs.cb_fin_r;
        ca.cb_fin_i = cs.cb_fin_i;
        ca.cb_sta_r = cs.cb_sta_r;
        ca.cb_sta_i = cs.cb_sta_i;
        ca.wtot = cs.wtot;
        // has_p adds nothing today (only completing launches, which all have it, carry an inject_k): kept as this launch's own guard
        if (cs.has_p) fill_inject(ca, inj, cs.inject_k, pl);
    }
    const unsigned tiles = unsigned(pl.dim >> geom.lt);
    if (X.lo < 3 && !bs.xcd && !rt.plain_tile_order && tiles % (8u << (3 - X.lo)) == 0) ca.tile_swz = 3 - X.lo;
    const bool cplx = (rt.flags & 1) != 0 || (cs.bwd && !rt.real_amp_grad);
    // auto: 1024 threads per tile for the forward passes, 512 for the (register-hungrier) adjoint passes
    // (the real-drive adjoint, without the signed sums, fits 1024 threads too: measured 2710 -> 2767 steps/s on C3)
    const int lgt = rt.variant == 0 ? ((cs.bwd && cplx) ? 9 : 10) : rt.chain_lgt;
    if (geom.lt == kWideTileBits) return launch_chain_l<kWideTileBits, 10>(ca, tiles, cplx, cs.bwd, stream);
    if (geom.lt == 11) return launch_chain_l<11, 10>(ca, tiles, cplx, cs.bwd, stream);
    if (geom.lt == 10) return launch_chain_l<10, 10>(ca, tiles, cplx, cs.bwd, stream);
    if (bs.xcd)  // L2-resident placement (automatic thread counts only: variant 10 decodes to 0)
        return lgt == 9 ? launch_chain_l<kTileBits, 9, true>(ca, tiles, cplx, cs.bwd, stream) : launch_chain_l<kTileBits, 10, true>(ca, tiles, cplx, cs.bwd, stream);
    switch (lgt) {
        case 8: return launch_chain_l<kTileBits, 8>(ca, tiles, cplx, cs.bwd, stream);
        case 10: return launch_chain_l<kTileBits, 10>(ca, tiles, cplx, cs.bwd, stream);
        default: return launch_chain_l<kTileBits, 9>(ca, tiles, cplx, cs.bwd, stream);
    }
}

// Run `items` (factors, in order) as a chain starting from the complete vector `start`.
//   dst(i)   : where the complete output of factor i (0-based) goes, or nullptr to skip storing it (only legal for the last)
//   on_done(i, ptr): called after the launch that completed factor i
// skip_last_finish: do not finish the last factor (its output is not needed) — used by the backward recompute.
template <class DstFn, class DoneFn, class ExpFn>
int run_chain(const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const double2* start, DstFn dst, DoneFn on_done,
              ExpFn exp_slot, bool skip_last_finish, const BatchSlice& bs, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int F = int(items.size()) - (skip_last_finish ? 1 : 0);  // the last factor is not even started then
    if (F <= 0) return RYDIFF_OK;
    std::vector<KernelStep> ks;
    chain_schedule(pl.NL, chain_geom(rt), F, ks);
    const double2* cur = start;
    int rcx = shard_signal(rt, 0, cur);  // partners need the chain's start vector for the first completing launch
    if (rcx) return rcx;
    const InjectSource no_inj{};
    for (size_t k = 0; k < ks.size(); ++k) {
        const KernelStep& st = ks[k];
        ChainStep cs = chain_step(pl, ws, st, k, cur, bs);
        if (cs.has_p) {
            if (st.completes) cs.v_out = dst(st.fin);
            cs.fin_stage = items[st.fin].stage;
            cs.fin = items[st.fin].s;
            if (!cs.v_out) return fail(RYDIFF_EINVAL, "internal: chain destination missing");
            if (st.completes) exp_slot(st.fin, cs);
        } else {
            cs.fin_stage = -1;
        }
        cs.sta_stage = cs.has_q ? items[st.sta].stage : -1;
        if (cs.has_q) cs.sta = items[st.sta].s;
        int rc = cs.has_p ? shard_signal(rt, 1, nullptr) : RYDIFF_OK;  // this launch reads the partners' copies of `cur`
        if (rc) return rc;
        rc = launch_chain(rt, ws, cs, bs, no_inj, stream);
        if (rc) return rc;
        if (cs.has_p && st.completes) {
            cur = cs.v_out;
            if (k + 1 < ks.size()) {  // the next launch completes the next factor from the partners' copies of this vector
                rc = shard_signal(rt, 0, cur);
                if (rc) return rc;
            }
            rc = on_done(st.fin, cs.v_out);
            if (rc) return rc;
        }
    }
    return RYDIFF_OK;
}

// Adjoint sweep of consecutive tsave intervals as ONE chain.  `items` are the forward factors (in forward order), xs[i] the
// input of factor i, `lam_in` the cotangent w.r.t. the output of the last one; the cotangent w.r.t. the first one's input ends
// up in lam_bufs[cl].  save_k[i] >= 0: the input of factor i is the state at save point save_k[i] — the launch that completes
// the cotangent there also adds the cotangent injected at that save point (fused).  on_stage_end(stage, lam, x_out) is called
// with the complete cotangent at every exponential's output.  stage_end_reads_partners (matters in sharded runs only): on_stage_end
// reads the partner ranks' copies of that cotangent too — the wait for them (shard_signal phase 1) then comes before the call instead
// of before the completing launch that follows it; still one wait per posted exchange.
template <class StageEndFn>
int run_chain_bwd(const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const std::vector<const double2*>& xs,
                  const std::vector<int>& save_k, const double2* lam_in, double2* lam_bufs[2], int& cl, double* wtot,
                  StageEndFn on_stage_end, bool stage_end_reads_partners, const BatchSlice& bs, const InjectSource& inj,
                  hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int M = int(items.size());
    std::vector<KernelStep> ks;
    chain_schedule(pl.NL, chain_geom(rt), M, ks);
    const double2* cur = lam_in;
    int rcx = shard_signal(rt, 0, cur);  // sharded: the partners need the incoming cotangent for the first completing launch
    if (rcx) return rcx;
    bool posted = true;  // the exchange of `cur` is posted and nobody has waited for it yet
    auto stage_end = [&](int stage, const double2* lam, const double2* x_out) -> int {
        if (stage_end_reads_partners && posted) {
            const int rc = shard_signal(rt, 1, nullptr);
            if (rc) return rc;
            posted = false;
        }
        return on_stage_end(stage, lam, x_out);
    };
    // adjoint factor index a = 0..M-1 corresponds to forward factor f = M-1-a
    for (size_t k = 0; k < ks.size(); ++k) {
        const KernelStep& st = ks[k];
        ChainStep cs = chain_step(pl, ws, st, k, cur, bs);
        cs.bwd = true;
        cs.wtot = wtot;
        if (cs.has_p) {
            const int f = M - 1 - st.fin;  // forward factor whose adjoint this launch extends / completes
            const ChainItem& it = items[f];
            cs.fin_stage = it.stage;
            cs.fin = {it.s.gr, -it.s.gi, it.s.br, -it.s.bi};
            cs.cb_fin_r = it.s.br;
            cs.cb_fin_i = it.s.bi;
            cs.x_fin = xs[f];
            if (st.completes) {
                if (!bs.xcd) cl ^= 1;  // L2-resident placement rewrites the cotangent in place
                cs.v_out = lam_bufs[cl];
                if (!bs.xcd && cs.v_out == cur) return fail(RYDIFF_EINVAL, "internal: cotangent ping-pong clash");
                cs.inject_k = save_k[f];
            }
        }
        if (cs.has_q) {
            const int f = M - 1 - st.sta;
            const ChainItem& it = items[f];
            cs.sta_stage = it.stage;
            cs.sta = {it.s.gr, -it.s.gi, it.s.br, -it.s.bi};
            cs.cb_sta_r = it.s.br;
            cs.cb_sta_i = it.s.bi;
            cs.x_sta = xs[f];
            // the cotangent `cur` at the output of the chain's last factor: exponential boundary for dL/dtau
            if (st.sta == 0) {
                int rc = stage_end(it.stage, cur, xs[M]);
                if (rc) return rc;
            }
        }
        // this launch reads the partners' copies of `cur` (a stage-end call in between may have waited for them already)
        int rc = (cs.has_p && st.completes && posted) ? shard_signal(rt, 1, nullptr) : RYDIFF_OK;
        if (rc) return rc;
        if (cs.has_p && st.completes) posted = false;
        rc = launch_chain(rt, ws, cs, bs, inj, stream);
        if (rc) return rc;
        if (cs.has_p && st.completes) {
            cur = cs.v_out;  // complete cotangent at the INPUT of forward factor f = output of forward factor f-1
            if (k + 1 < ks.size()) {  // the next completing launch needs the partners' copies of this cotangent
                rc = shard_signal(rt, 0, cur);
                if (rc) return rc;
                posted = true;
            }
            const int f = M - 1 - st.fin;
            if (f >= 1 && items[f].stage != items[f - 1].stage) {
                rc = stage_end(items[f - 1].stage, cur, xs[f]);
                if (rc) return rc;
            }
        }
    }
    return RYDIFF_OK;
}

// Trajectory-per-XCD placement of the chained tile passes ("Batches of L2-sized trajectories"): a launch
// covers a GROUP of 8 m trajectories, trajectory -> XCD by workgroup id % 8, vectors rewritten in place with plain loads and
// stores, so that the complete vector + partial of m trajectories (m * 32 * 2^N bytes) stay in each XCD's 4 MiB L2 from pass to
// pass and only the write-back crosses the fabric.  Every group runs its WHOLE sweep before the next one starts.  Returns the
// group size (0: off).  Placement changes speed only: results are the same as with the plain grid (A/B-tested).
int xcd_group_size(const Runtime& rt, bool adjoint) {
    const Plan& pl = rt.pl;
    if (!chain_enabled(rt) || chain_geom(rt).layouts != 2 || chain_geom(rt).lt != kTileBits || pl.shard_bits) return 0;
    const size_t live = size_t(32) << pl.N;    // complete vector + partial of one trajectory
    const size_t budget = size_t(3) << 20;     // of the 4 MiB L2 (the rest: tape lines on their way out, tables)
    const int m = int(std::max<size_t>(1, budget / live));
    if (rt.force_xcd) return 8 * m;
    // Measured (profiles/r02_xcd_placement.txt): a launch of <= 256 tiles is bound by the ~10 us one tile keeps its CU busy, not by
    // the fabric, so SEVERAL groups in sequence lose to one launch over the whole batch (16 qubits x 32: 38 vs 27 us per pass).
    // Where ONE group covers the batch the forward passes gain (16 qubits x 8: 14.2 -> 9.8 us; 13 qubits x 64: 12.1 -> 9.6 us);
    // the adjoint passes, which stream two tape vectors anyway, do not (17.1 vs 17.3 us).
    if (rt.variant != 0 || adjoint || pl.B < 8 || pl.B > 8 * m || live > budget) return 0;
    return 8 * m;
}

}  // namespace
