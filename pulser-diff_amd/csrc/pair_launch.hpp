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

// The forward pass's blocks of a chain: factors paired from the start of each exponential (an exponential with an odd number of
// factors ends in a one-factor block).  (first factor, second factor or -1)
std::vector<std::pair<int, int>> forward_blocks(const std::vector<ChainItem>& items) {
    std::vector<std::pair<int, int>> blk;
    const int F = int(items.size());
    for (int i = 0; i < F;) {
        if (i + 1 < F && items[i + 1].stage == items[i].stage) {
            blk.push_back({i, i + 1});
            i += 2;
        } else {
            blk.push_back({i, -1});
            ++i;
        }
    }
    return blk;
}

// forward blocks in the factors of interval k (step_factor_count counts its factors)
int64_t step_block_count(const Runtime& rt, int k) {
    int64_t b = 0;
    for (int e = rt.pl.step_begin[k]; e < rt.pl.step_begin[k + 1]; ++e) b += (int64_t(rt.pl.stages[e].nsub) * rt.poly.degree + 1) / 2;
    return b;
}

// What launch j of a block chain fills whatever the direction (Chain2Args / Chain2BwdArgs): it finishes block j-1 and starts
// block j of `blk` (first factor, second factor or -1), in layout (j + par) & 1.  The w / t of a started block go to pp0 / pp1 and
// pp2 / pp3 alternately; `cur` is the complete vector the launch works on.  `par`: the layout of the chain's first launch (the
// layout, the split tables, the Y' mask and the w / t buffers all follow it).
template <class Args>
void fill_chain2(Args& ca, const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const std::vector<std::pair<int, int>>& blk,
                 int j, const double2* cur, const BatchSlice& bs, int par = 0) {
    const Plan& pl = rt.pl;
    double2* wt[2][2] = {{reinterpret_cast<double2*>(ws + pl.off_pp0), reinterpret_cast<double2*>(ws + pl.off_pp1)},
                         {reinterpret_cast<double2*>(ws + pl.off_pp2), reinterpret_cast<double2*>(ws + pl.off_pp3)}};
    const ChainGeom geom{kTileBits, 2};
    const int nb = int(blk.size()), jp = j + (par & 1), L = jp & 1;
    const LayoutDesc Y = chain_layout(pl.NL, L, geom), X = chain_layout(pl.NL, L ^ 1, geom);
    ca.w = j ? wt[(jp - 1) & 1][0] : cur;  // (always loadable: the kernels request their inputs outside of control flow)
    ca.t = j ? wt[(jp - 1) & 1][1] : cur;
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
        ca.w_out = wt[jp & 1][0];
        ca.t_out = wt[jp & 1][1];
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
// wtape (with keep_mid; pair_wtape): that slot takes the block's w = P_X v instead.  The launch that starts the block writes it there
// and not into the ping-pong buffers, the launch that finishes it reads it from there, and no v_mid is stored: 3R+3W per block.
// One-factor blocks keep w in the ping-pong buffers; t always stays there.  The kernel and its arithmetic are the same.
template <class DstFn, class DoneFn, class ExpFn>
int run_chain2(const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const double2* start, DstFn dst, bool keep_mid,
               bool wtape, DoneFn on_done, ExpFn exp_slot, const BatchSlice& bs, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int F = int(items.size());
    if (F <= 0) return RYDIFF_OK;
    if (wtape && !keep_mid) return fail(RYDIFF_EINVAL, "internal: P_X v is taped with the full tape only");
    const std::vector<std::pair<int, int>> blk = forward_blocks(items);
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
            ca.vmid_out = (f1 >= 0 && keep_mid && !wtape) ? dst(f0) : nullptr;
            if (f1 >= 0 && wtape) ca.w = dst(f0);
            ca.y_out = dst(last);
            if (!ca.y_out) return fail(RYDIFF_EINVAL, "internal: chain destination missing");
            ChainStep cs{};
            exp_slot(last, cs);
            ca.obs = cs.obs;
            ca.expect_slot = cs.expect_slot;
            ca.n_obs = cs.n_obs;
            ca.exp_ostride = cs.exp_ostride;
        }
        if (wtape && ca.has_q && blk[j].second >= 0) {
            ca.w_out = dst(blk[j].first);
            if (!ca.w_out) return fail(RYDIFF_EINVAL, "internal: chain destination missing");
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

// What the full tape holds between the two factors of a block.  v_mid, the first factor's output, has one reader, the adjoint block
// kernel, and v_mid = gamma_1 v + beta_1 (D v + c (P_X v + P_Y' v)) with w = P_X v written by the forward chain anyway.  With w in
// that slot ("w on the tape") the forward block is 3R+3W instead of 3R+4W, and the adjoint kernel (its XW instantiation) rebuilds
// v_mid from the two tape vectors it reads as before, with one more partner-sum round over the Y' bits.
// Only where the full tape's one reader is that kernel: the block adjoint is on and no pass is placed one trajectory per XCD.  The
// one-factor adjoint (variant 19, complex tables), the partial tape and the recomputed factor inputs keep v_mid.  The forward call
// records the format it wrote next to the workspace (tape_format_record, rydiff.hip); the backward call reads that record.
// Automatic (C3, the only shape where the blocks are automatic): on, +2.5 % on the bench line, 31 of the parent's spreads above the
// parent, and +1.6 %, 18 spreads, in a second session (profiles/r10_bench.jsonl); variant 35 selects it wherever the blocks are
// legal, 17 and 19..34 keep v_mid.
constexpr bool kPairWtapeDefault = true;
bool pair_wtape(const Runtime& rt) {
    const bool sel = rt.pair_wtape ? rt.pair_wtape > 0 : kPairWtapeDefault;
    return sel && rt.pl.tape_mode == 2 && pair_bwd_enabled(rt) && xcd_group_size(rt, false) == 0 && xcd_group_size(rt, true) == 0;
}

// Tape staging of the adjoint block kernel.  Automatic stays with the registers: on C3 the LDS-DMA version measured the same per
// launch (26.3 us both) and within noise on the bench line; it remains selectable for A/B runs.
constexpr bool kPairBwdDmaDefault = false;
bool pair_bwd_dma(const Runtime& rt) { return rt.pair_bwd_stage ? rt.pair_bwd_stage > 0 : kPairBwdDmaDefault; }

int pair_pace_bwd(const Runtime& rt) {
    if (!pair_vec_major(rt) || pair_through(rt) != 3 || pair_bwd_dma(rt)) return 0;
    return rt.pair_pace_bwd >= 0 ? rt.pair_pace_bwd : kPairPaceBwdDefault;
}

template <int LGT, bool ORD, int WT, bool DMA, int PACE = 0, bool XW = false>
int launch_chain2_bwd_t(const Chain2BwdArgs& ca, unsigned tiles, hipStream_t stream) {
    constexpr int LT = kTileBits;
    constexpr size_t lds = chain2_bwd_lds_bytes<LT, LGT, DMA>();
    static_assert(lds <= 160 * 1024, "k_chain2_bwd: more LDS than a gfx950 workgroup can have");
    if (int rc = set_max_dynamic_lds_once<&k_chain2_bwd<LT, LGT, ORD, WT, DMA, PACE, XW>>(lds)) return rc;
    hipLaunchKernelGGL((k_chain2_bwd<LT, LGT, ORD, WT, DMA, PACE, XW>), dim3(tiles, unsigned(ca.b_count)), dim3(1 << LGT), lds, stream, ca);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// The LDS-DMA staging exists with vector-major requests only: with the automatic store policy (variant 21) and with streaming
// stores (variant 29).
int launch_chain2_bwd(const Runtime& rt, const Chain2BwdArgs& ca, unsigned tiles, bool wtape, hipStream_t stream) {
    const bool ord = pair_vec_major(rt);
    if (wtape) {  // one instantiation: vector-major, register-staged, everything written through, with a pacing of its own
        if (!ord || pair_through(rt) != 3 || pair_bwd_dma(rt)) return fail(RYDIFF_EINVAL, "internal: no such block kernel");
        return launch_chain2_bwd_t<10, true, 3, false, 0, true>(ca, tiles, stream);
    }
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
// wtape (pair_wtape: xs holds P_X x_b where a two-factor block's x_a would be): the blocks are the FORWARD pass's, in reverse (an
// exponential of odd degree starts, in adjoint order, with its one-factor block), and each is finished in the layout in which the
// forward pass finished it: the taped P_X x_b covers the bits of the layout the forward block was started in, so only then are the
// bits it lacks (Y') local to the tile.  The forward pass finished its block g (counted over the whole run) in layout (g + 1) & 1;
// with g_hi the run-wide index of this chain's last block, launch j finishes block g_hi - (j - 1) and runs in layout (j + g_hi) & 1.
template <class StageEndFn>
int run_chain2_bwd(const Runtime& rt, char* ws, const std::vector<ChainItem>& items, const std::vector<const double2*>& xs,
                   const std::vector<int>& save_k, const double2* lam_in, double2* lam_bufs[2], int& cl, double* wtot,
                   StageEndFn on_stage_end, const BatchSlice& bs, const InjectSource& inj, bool wtape, int64_t g_hi, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int M = int(items.size());
    if (M <= 0) return RYDIFF_OK;
    std::vector<std::pair<int, int>> blk;  // adjoint order: (first forward factor b, second forward factor a or -1)
    if (wtape) {
        blk = forward_blocks(items);
        std::reverse(blk.begin(), blk.end());
    }
    for (int f = wtape ? -1 : M - 1; f >= 0;) {
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
    const int par = wtape ? int(g_hi & 1) : 0;
    const double2* cur = lam_in;
    int rc = on_stage_end(items[M - 1].stage, cur, xs[M]);  // the cotangent at the chain's output: exponential boundary for dL/dtau
    if (rc) return rc;
    for (int j = 0; j <= nb; ++j) {
        Chain2BwdArgs ca{};
        fill_chain2(ca, rt, ws, items, blk, j, cur, bs, par);
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
            ca.cgb_r = sb.gr;
            ca.cgb_i = sb.gi;
            ca.xb = xs[fb];
            ca.xa = fa >= 0 ? xs[fa] : xs[fb];  // (wtape: P_X x_b, in the slot of x_a)
            ca.ge_fin = rt.ge(ws, items[fb].stage);
            cl ^= 1;
            ca.mu_out = lam_bufs[cl];
            if (ca.mu_out == cur) return fail(RYDIFF_EINVAL, "internal: cotangent ping-pong clash");
            fill_inject(ca, inj, save_k[fb], pl);  // (inside has_p: every finishing launch completes a cotangent, mu_out)
        }
        rc = launch_chain2_bwd(rt, ca, tiles, wtape, stream);
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
