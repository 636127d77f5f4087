// pair_launch.hpp — chained passes in blocks of two factors (pair_kernels.hpp): where they run, forward and adjoint drivers.
#pragma once

namespace {

// ---- block-of-two forward passes (k_chain2, pair_kernels.hpp) ------------------------------------------------------
// Legal for one phase-free global drive and at most one detuning group on 13..20 qubits with the two-layout 2^12 tiles, un-sharded.
bool pair_legal(const Runtime& rt) {
    const Plan& pl = rt.pl;
    const uint32_t all = uint32_t(pl.dim) - 1u;
    const ChainGeom g = chain_geom(rt);
    return rt.pair_mode >= 0 && rt.variant == 0 && !rt.force_three && !rt.force_xcd && chain_enabled(rt) && !pl.shard_bits &&
           pl.N > kTileBits && pl.N <= 20 && g.lt == kTileBits && g.layouts == 2 && pl.ga.n == 1 && pl.gd.n <= 1 && !pl.ga.flagged &&
           (pl.ga.amp_index_mask[0] & all) == all && !(rt.flags & 1) && pl.off_pp2 && pl.off_pp3;
}

// Automatic only where it measured faster: the 20-qubit single trajectory (C3).  Variant 17: wherever legal.
bool pair_enabled(const Runtime& rt) {
    if (!pair_legal(rt)) return false;
    return rt.pair_mode == 1 || (rt.pl.N == 20 && rt.pl.B == 1);
}

// What launch j of a block chain fills whatever the direction (Chain2Args / Chain2BwdArgs): it finishes block j-1 and starts
// block j of `blk` (first factor, second factor or -1), in layout j & 1.  The w / t of a started block go to pp0 / pp1 and
// pp2 / pp3 alternately; `cur` is the complete vector the launch works on.
template <class Args>
void fill_chain2(Args& ca, const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const std::vector<std::pair<int, int>>& blk,
                 int j, const double2* cur, const BatchSlice& bs) {
    const Plan& pl = rt.pl;
    double2* wt[2][2] = {{reinterpret_cast<double2*>(ws + pl.off_pp0), reinterpret_cast<double2*>(ws + pl.off_pp1)},
                         {reinterpret_cast<double2*>(ws + pl.off_pp2), reinterpret_cast<double2*>(ws + pl.off_pp3)}};
    const ChainGeom geom{kTileBits, 2};
    const int nb = int(blk.size()), L = j & 1;
    const LayoutDesc Y = chain_layout(pl.NL, L, geom), X = chain_layout(pl.NL, L ^ 1, geom);
    ca.w = j ? wt[(j - 1) & 1][0] : cur;  // (always loadable: the kernels request their inputs outside of control flow)
    ca.t = j ? wt[(j - 1) & 1][1] : cur;
    ca.utt = split_tables(pl, ws, kTileBits) + size_t(L) * rt.per_layout(kTileBits);
    ca.vr = ca.utt + (size_t(1) << kTileBits);
    ca.coef_bstride = rt.coef_bstride();
    ca.coef_fin = rt.coef(ws, j ? items[blk[j - 1].first].stage : 0);
    ca.coef_sta = rt.coef(ws, j < nb ? items[blk[j].first].stage : 0);
    ca.lo = Y.lo;
    ca.hs = Y.hs;
    ca.hb = Y.hb;
    ca.dim = uint32_t(pl.dim);
    ca.has_p = j > 0;
    ca.has_q = j < nb;
    ca.gd = pl.gd.n;
    ca.b_first = bs.first;
    ca.b_count = bs.count;
    if (ca.has_p) ca.fin_mask = to_tile_mask(Y, kTileBits, uint32_t(pl.dim - 1) & ~X.bits);
    if (ca.has_q) {
        ca.w_out = wt[j & 1][0];
        ca.t_out = wt[j & 1][1];
    }
}

// Request order and store policy of the block kernels (template parameters ORD / WT of k_chain2 and k_chain2_bwd, pair_kernels.hpp).
// Automatic: vector-major requests and every output stored write-through, the combination that measured fastest on C3 (variant 28:
// +2.7 % on the bench line); variants 22..30 select the others for A/B runs, 30 the kernels before this choice.
constexpr bool kPairVecMajorDefault = true;
constexpr int kPairThroughDefault = 3;
bool pair_vec_major(const Runtime& rt) { return rt.pair_phases >= 0 ? (rt.pair_phases >> 2) != 0 : kPairVecMajorDefault; }
int pair_through(const Runtime& rt) { return rt.pair_phases >= 0 ? (rt.pair_phases & 3) : kPairThroughDefault; }

// Paced input requests of the block kernels (their template parameter PACE; variants 31..34).  They exist next to the automatic
// request order and store policy only (vector-major, everything written through), the adjoint one with register staging only.
// Automatic (C3, the only shape where the blocks are automatic): the paced ADJOINT kernel, +1.9 % on the bench
// line and past the bar of ten spreads; the paced forward kernels did not clear it (31: +0.5 %, 34: -0.6 %) and stay selectable.
constexpr int kPairPaceFwdDefault = 0;
constexpr int kPairPaceBwdDefault = 1;
int pair_pace_fwd(const Runtime& rt) {
    if (!pair_vec_major(rt) || pair_through(rt) != 3) return 0;
    return rt.pair_pace_fwd >= 0 ? rt.pair_pace_fwd : kPairPaceFwdDefault;
}

// f(bool_constant<ORD>, integral_constant<int, WT>) for the run-time pair (ord, wt): the instantiations that exist
template <class F>
int with_pair_phases(bool ord, int wt, F f) {
    using std::bool_constant;
    using std::integral_constant;
    switch ((ord ? 4 : 0) | wt) {
        case 0: return f(bool_constant<false>{}, integral_constant<int, 0>{});
        case 1: return f(bool_constant<false>{}, integral_constant<int, 1>{});
        case 2: return f(bool_constant<false>{}, integral_constant<int, 2>{});
        case 3: return f(bool_constant<false>{}, integral_constant<int, 3>{});
        case 4: return f(bool_constant<true>{}, integral_constant<int, 0>{});
        case 5: return f(bool_constant<true>{}, integral_constant<int, 1>{});
        case 6: return f(bool_constant<true>{}, integral_constant<int, 2>{});
        case 7: return f(bool_constant<true>{}, integral_constant<int, 3>{});
    }
    return fail(RYDIFF_EINVAL, "internal: no such block kernel");
}

template <int LGT, bool ORD, int WT, int PACE = 0>
int launch_chain2_t(const Chain2Args& ca, unsigned tiles, hipStream_t stream) {
    constexpr int LT = kTileBits;
    const size_t lds = 2 * (size_t(1) << LT) * sizeof(double2) + 256;  // two tile buffers + one double per wave
    if (int rc = set_max_dynamic_lds_once<&k_chain2<LT, LGT, ORD, WT, PACE>>(lds)) return rc;
    hipLaunchKernelGGL((k_chain2<LT, LGT, ORD, WT, PACE>), dim3(tiles, unsigned(ca.b_count)), dim3(1 << LGT), lds, stream, ca);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

int launch_chain2(const Runtime& rt, const Chain2Args& ca, unsigned tiles, hipStream_t stream) {
    switch (pair_pace_fwd(rt)) {
        case 1: return launch_chain2_t<10, true, 3, 1>(ca, tiles, stream);
        case 2: return launch_chain2_t<10, true, 3, 2>(ca, tiles, stream);
    }
    return with_pair_phases(pair_vec_major(rt), pair_through(rt), [&](auto ord, auto wt) {
        return launch_chain2_t<10, decltype(ord)::value, decltype(wt)::value>(ca, tiles, stream);
    });
}

// Forward chain in blocks of two factors of one exponential (an exponential of odd degree ends in a one-factor block).  Same
// contract as run_chain (no skip_last_finish); keep_mid: the output of a block's first factor is stored too (dst of that factor).
template <class DstFn, class DoneFn, class ExpFn>
int run_chain2(const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const double2* start, DstFn dst, bool keep_mid,
               DoneFn on_done, ExpFn exp_slot, const BatchSlice& bs, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int F = int(items.size());
    if (F <= 0) return RYDIFF_OK;
    std::vector<std::pair<int, int>> blk;  // (first factor, second factor or -1)
    for (int i = 0; i < F;) {
        if (i + 1 < F && items[i + 1].stage == items[i].stage) {
            blk.push_back({i, i + 1});
            i += 2;
        } else {
            blk.push_back({i, -1});
            ++i;
        }
    }
    const unsigned tiles = unsigned(pl.dim >> kTileBits);
    const int nb = int(blk.size());
    const double2* cur = start;
    for (int j = 0; j <= nb; ++j) {
        Chain2Args ca{};
        fill_chain2(ca, rt, ws, items, blk, j, cur, bs);
        ca.v = cur;
        fill_detuning(ca.dmask, ca.dcnt, pl);
        int f0 = -1, last = -1;
        if (ca.has_p) {
            f0 = blk[j - 1].first;
            const int f1 = blk[j - 1].second;
            last = f1 >= 0 ? f1 : f0;
            const FactorScalars& s1 = items[f0].s;
            const FactorScalars s2 = f1 >= 0 ? items[f1].s : FactorScalars{1.0, 0.0, 0.0, 0.0};
            const std::complex<double> g1(s1.gr, s1.gi), b1(s1.br, s1.bi), g2(s2.gr, s2.gi), b2(s2.br, s2.bi);
            const std::complex<double> qa = g1 * g2, qb = g1 * b2 + b1 * g2, qk = b1 * b2;
            ca.a_r = qa.real();
            ca.a_i = qa.imag();
            ca.b_r = qb.real();
            ca.b_i = qb.imag();
            ca.k_r = qk.real();
            ca.k_i = qk.imag();
            ca.g1_r = s1.gr;
            ca.g1_i = s1.gi;
            ca.b1_r = s1.br;
            ca.b1_i = s1.bi;
            ca.vmid_out = (f1 >= 0 && keep_mid) ? dst(f0) : nullptr;
            ca.y_out = dst(last);
            if (!ca.y_out) return fail(RYDIFF_EINVAL, "internal: chain destination missing");
            ChainStep cs{};
            exp_slot(last, cs);
            ca.obs = cs.obs;
            ca.expect_slot = cs.expect_slot;
            ca.n_obs = cs.n_obs;
            ca.exp_ostride = cs.exp_ostride;
        }
        int rc = launch_chain2(rt, ca, tiles, stream);
        if (rc) return rc;
        if (ca.has_p) {
            if (ca.vmid_out) {
                rc = on_done(f0, ca.vmid_out);
                if (rc) return rc;
            }
            rc = on_done(last, ca.y_out);
            if (rc) return rc;
            cur = ca.y_out;
        }
    }
    return RYDIFF_OK;
}

// ---- adjoint in blocks of two factors (k_chain2_bwd, pair_kernels.hpp) -------------------------------------------------
// Where the forward blocks are, for the real-drive adjoint (RydProblem.real_amp_grad: no signed sums) on the 2^12 two-layout
// tiles; variant 19 keeps the one-factor adjoint (k_chain) next to automatic forward blocks.  Variants 20 / 21: blocks wherever
// legal (as 17) with the tape vectors staged through registers / by LDS-DMA (k_chain2_bwd<.., false / true>).  Variants 22..30: as
// 20, with a request order and a store policy of their own (pair_vec_major, pair_through); 29 alone stages by LDS-DMA.
// Variants 31..34: as 20, with paced input requests (pair_pace_fwd, pair_pace_bwd).
bool pair_bwd_enabled(const Runtime& rt) {
    const ChainGeom g = chain_geom(rt);
    return !rt.pair_bwd_off && rt.real_amp_grad && pair_enabled(rt) && g.lt == kTileBits && g.layouts == 2;
}

// Tape staging of the adjoint block kernel.  Automatic stays with the registers: on C3 the LDS-DMA version measured the same per
// launch (26.3 us both) and within noise on the bench line; it remains selectable for A/B runs.
constexpr bool kPairBwdDmaDefault = false;
bool pair_bwd_dma(const Runtime& rt) { return rt.pair_bwd_stage ? rt.pair_bwd_stage > 0 : kPairBwdDmaDefault; }

int pair_pace_bwd(const Runtime& rt) {
    if (!pair_vec_major(rt) || pair_through(rt) != 3 || pair_bwd_dma(rt)) return 0;
    return rt.pair_pace_bwd >= 0 ? rt.pair_pace_bwd : kPairPaceBwdDefault;
}

template <int LGT, bool ORD, int WT, bool DMA, int PACE = 0>
int launch_chain2_bwd_t(const Chain2BwdArgs& ca, unsigned tiles, hipStream_t stream) {
    constexpr int LT = kTileBits;
    constexpr size_t lds = chain2_bwd_lds_bytes<LT, LGT, DMA>();
    static_assert(lds <= 160 * 1024, "k_chain2_bwd: more LDS than a gfx950 workgroup can have");
    if (int rc = set_max_dynamic_lds_once<&k_chain2_bwd<LT, LGT, ORD, WT, DMA, PACE>>(lds)) return rc;
    hipLaunchKernelGGL((k_chain2_bwd<LT, LGT, ORD, WT, DMA, PACE>), dim3(tiles, unsigned(ca.b_count)), dim3(1 << LGT), lds, stream, ca);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// The LDS-DMA staging exists with vector-major requests only: with the automatic store policy (variant 21) and with streaming
// stores (variant 29).
int launch_chain2_bwd(const Runtime& rt, const Chain2BwdArgs& ca, unsigned tiles, hipStream_t stream) {
    const bool ord = pair_vec_major(rt);
    if (pair_pace_bwd(rt)) return launch_chain2_bwd_t<10, true, 3, false, 1>(ca, tiles, stream);
    if (pair_bwd_dma(rt)) {
        if (ord && pair_through(rt) == 3) return launch_chain2_bwd_t<10, true, 3, true>(ca, tiles, stream);
        if (ord && pair_through(rt) == 0) return launch_chain2_bwd_t<10, true, 0, true>(ca, tiles, stream);
        return fail(RYDIFF_EINVAL, "internal: no such block kernel");
    }
    return with_pair_phases(ord, pair_through(rt), [&](auto o, auto wt) {
        return launch_chain2_bwd_t<10, decltype(o)::value, decltype(wt)::value, false>(ca, tiles, stream);
    });
}

// Same contract as run_chain_bwd (un-sharded, no trajectory-per-XCD placement), in blocks of two factors of one exponential.
// Factors are paired from the end of each exponential backwards (an exponential of odd degree starts with a one-factor block),
// so a block never spans two exponentials and only its first factor's input can be a save point.  Launch j finishes the adjoint
// of block j-1 and starts block j, in layout j & 1 (w / t of a started block: pp0 / pp1 and pp2 / pp3, alternately).
template <class StageEndFn>
int run_chain2_bwd(const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const std::vector<const double2*>& xs,
                   const std::vector<int>& save_k, const double2* lam_in, double2* lam_bufs[2], int& cl, double* wtot,
                   StageEndFn on_stage_end, const BatchSlice& bs, const InjectSource& inj, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int M = int(items.size());
    if (M <= 0) return RYDIFF_OK;
    std::vector<std::pair<int, int>> blk;  // adjoint order: (first forward factor b, second forward factor a or -1)
    for (int f = M - 1; f >= 0;) {
        if (f >= 1 && items[f - 1].stage == items[f].stage) {
            blk.push_back({f - 1, f});
            f -= 2;
        } else {
            blk.push_back({f, -1});
            --f;
        }
    }
    const unsigned tiles = unsigned(pl.dim >> kTileBits);
    const int nb = int(blk.size());
    const double2* cur = lam_in;
    int rc = on_stage_end(items[M - 1].stage, cur, xs[M]);  // the cotangent at the chain's output: exponential boundary for dL/dtau
    if (rc) return rc;
    for (int j = 0; j <= nb; ++j) {
        Chain2BwdArgs ca{};
        fill_chain2(ca, rt, ws, items, blk, j, cur, bs);
        ca.mu = cur;
        ca.xa = ca.xb = cur;  // (loadable, as w and t)
        if (pl.gd.n) {
            ca.dmask = pl.gd.amp_index_mask[0];
            ca.dcnt = pl.gd.count[0];
        }
        ca.ge_fin = rt.ge(ws, 0);
        ca.ge_bstride = rt.ge_bstride();
        ca.ge_rstride = pl.NC + 1;
        ca.det_slot = 2 * pl.ga.n;
        ca.wtot = wtot;
        int fb = -1;
        if (ca.has_p) {
            fb = blk[j - 1].first;
            const int fa = blk[j - 1].second;
            const FactorScalars& sb = items[fb].s;
            const FactorScalars sa = fa >= 0 ? items[fa].s : FactorScalars{1.0, 0.0, 0.0, 0.0};
            const std::complex<double> gb(sb.gr, -sb.gi), bb(sb.br, -sb.bi), ga(sa.gr, -sa.gi), ba(sa.br, -sa.bi);  // conjugated
            const std::complex<double> qk = ba * bb;
            ca.gb_r = gb.real();
            ca.gb_i = gb.imag();
            ca.bb_r = bb.real();
            ca.bb_i = bb.imag();
            ca.k_r = qk.real();
            ca.k_i = qk.imag();
            ca.ga_r = ga.real();
            ca.ga_i = ga.imag();
            ca.ba_r = ba.real();
            ca.ba_i = ba.imag();
            ca.cba_r = sa.br;
            ca.cba_i = sa.bi;
            ca.cbb_r = sb.br;
            ca.cbb_i = sb.bi;
            ca.xb = xs[fb];
            ca.xa = fa >= 0 ? xs[fa] : xs[fb];
            ca.ge_fin = rt.ge(ws, items[fb].stage);
            cl ^= 1;
            ca.mu_out = lam_bufs[cl];
            if (ca.mu_out == cur) return fail(RYDIFF_EINVAL, "internal: cotangent ping-pong clash");
            fill_inject(ca, inj, save_k[fb], pl);  // (inside has_p: every finishing launch completes a cotangent, mu_out)
        }
        rc = launch_chain2_bwd(rt, ca, tiles, stream);
        if (rc) return rc;
        if (ca.has_p) {
            cur = ca.mu_out;  // complete cotangent at the input of forward factor fb
            if (fb >= 1 && items[fb].stage != items[fb - 1].stage) {
                rc = on_stage_end(items[fb - 1].stage, cur, xs[fb]);
                if (rc) return rc;
            }
        }
    }
    return RYDIFF_OK;
}

}  // namespace
