// pair_kernels.hpp — block-of-two chained pass (included by rydiff.hip after chain_kernels.hpp).
//
// Two consecutive factors of ONE exponential share H = D + c P (one phase-free global drive: real c, real diagonal D, P the plain
// sum of all flips), so together they are the quadratic  q(H) = (g1 + b1 H)(g2 + b2 H) = a + b H + k H^2.  In the two-layout chain
// of k_chain, with X the layout of the previous launch and Y the layout of this one, P = P_X + P_Y' (P_X: flips of every X tile
// bit, P_Y': flips of the Y tile bits X lacks; they commute).  The launch that STARTS a block in X writes, next to v itself,
//     w = P_X v,   t = P_X (D v + c w);
// the launch that FINISHES it in Y reads v, w, t (own elements) and, with two partner-sum rounds over the Y' bits,
//     s = P_Y' v,  h1 = D v + c (w + s)  (= H v),   e = h1 + c w,
//     y = a v + b h1 + k (D h1 + c t + c P_Y' e)    (= q(H) v exactly: H^2 v = D h1 + c [P_X (D v + c w) + P_Y' e], as P_X s = P_Y' w)
//     v_mid = g1 v + b1 h1                           (output of the first factor: the tape entry between the two)
// and then starts the next block in Y on y (two rounds over every Y tile bit).  Per factor that is 3R+3W / 2 (no tape) or
// 3R+4W / 2 (full tape) instead of 2R+2W, with the same LDS partner-sum work per factor.  A block with k = 0 (the last factor of
// an exponential of odd degree) skips the second finishing round.  The tile lives in two LDS buffers used alternately, so a
// round needs one barrier (a buffer is rewritten only after the barrier that follows the other buffer's write).
#pragma once

struct Chain2Args {
    const double2* v;  // complete input of the block being finished (this launch's layout; the start vector for the first launch)
    const double2* w;  // P_X v                                (unused when !has_p)
    const double2* t;  // P_X (D v + c w)                      (unused when !has_p)
    double2* vmid_out;  // output of the block's first factor, or nullptr
    double2* y_out;     // output of the block (written when has_p)
    double2* w_out;     // the next block's w, t (written when has_q)
    double2* t_out;
    const double* utt;  // split interaction diagonal of this layout (as ChainArgs)
    const double* vr;
    const double* coef_fin;  // coefficient record of the finished block's exponential (trajectory 0)
    const double* coef_sta;  // ... of the started block's exponential
    long coef_bstride;
    double a_r, a_i, b_r, b_i, k_r, k_i;  // q(H) = a + b H + k H^2 of the finished block
    double g1_r, g1_i, b1_r, b1_i;        // its first factor (v_mid)
    int lo, hs, hb;                       // layout of this launch (as ChainArgs)
    uint32_t dim;
    int has_p, has_q;
    int gd;
    uint32_t fin_mask;  // TILE-bit mask of the Y' bits (the bits of this layout that the previous one lacks)
    uint32_t dmask[kMaxGroups];
    int dcnt[kMaxGroups];
    int b_first, b_count;
    const double* obs;  // fused <y|O|y> (forward, step ends): [n_obs][dim] or nullptr
    double* expect_slot;
    int n_obs;
    long exp_ostride;
};

// ORD: the workgroup requests its inputs vector-major.  A CU's vector-memory path serves requests roughly in issue order, and each
// wave issues v, w, t back to back, so wave-major the last wave's v is requested behind almost all of w and t and round A's barrier
// waits for about the whole load phase.  With ORD every wave issues v, a bare execution barrier (s_barrier: no fence, no wait on
// the counter) lets the other waves issue theirs, and only then follow w and, behind another barrier, t.  Speed only: each wave
// still awaits each input where it uses it.  (The early return above the loads is workgroup-uniform.)
// WT: which outputs are stored write-through (through_store) instead of streaming (stream_store, dirty in L2 until the end of the
// kernel): 0 none | 1 v_mid and y, which have the whole start stage behind them | 2 also w' | 3 all, t' included.
// PACE (with ORD; replaces its two barriers): w and t are kept OUT of the memory system while v is wanted, so that the finishing
// rounds run inside the load phase.  Each wave requests v, waits (counted s_waitcnt) until half of its v is back and only then
// requests w; it awaits v alone for round A.  1: t is requested after round A's partner sums, once half of the wave's w is back,
// in program order ahead of the v_mid stores, and round B runs while it lands | 2: t is requested before round A's barrier, as
// soon as the wave's v is complete, without a look at w.  The four v_mid stores are issued whether there is a destination or not
// (without one the buffer has no records and the range check drops them), so that the wait for t is a counted one that leaves
// exactly these four outstanding: behind a branch around them it would be vmcnt(0), the counter retires in order, and t would wait
// for their acknowledgement.  A chain's first launch requests v and w only and takes y from w; a one-factor block retires t unused.
// No arithmetic statement differs: every stored value is bit-identical.
template <int LT, int LGT, bool ORD = false, int WT = 0, int PACE = 0>
__global__ __launch_bounds__(1 << LGT) void k_chain2(Chain2Args a) {
    constexpr int NT = 1 << LGT, R = 1 << (LT - LGT);
    static_assert(WT >= 0 && WT <= 3);
    static_assert(PACE >= 0 && PACE <= 2 && (!PACE || ORD) && (!PACE || R == 4), "pacing: vector-major kernels with four elements per thread");
    extern __shared__ __attribute__((aligned(16))) double2 tiles[];
    double* red = reinterpret_cast<double*>(tiles + 2 * (size_t(1) << LT));
    const unsigned tid = threadIdx.x;
    const unsigned t = blockIdx.x;
    const unsigned bl = blockIdx.y;
    if (bl >= unsigned(a.b_count)) return;
    const unsigned bt = unsigned(a.b_first) + bl;
    const size_t boff = size_t(bt) * a.dim;
    const unsigned lomask = (1u << a.lo) - 1u;
    const int midlow = a.hs - a.lo;
    const unsigned xbase = ((t & ((1u << midlow) - 1u)) << a.lo) | ((t >> midlow) << (a.hs + a.hb));
    RYDIFF_TL(0);
    // ORD: the diagonal's table entries and the coefficients of both stages (L2 hits, at most one detuning group where the blocks
    // are legal) are requested ahead of the streamed vectors, as in k_chain2_bwd.  Behind them, the wait for the table would retire
    // v, w and t together, and the start stage's coefficient reads would wait for the acknowledgement of the y stores.
    const double* __restrict__ vrow = a.vr + size_t(t) * 16;
    [[maybe_unused]] double ut[R], vtop[LT + 1], c_fin = 0.0, c_sta = 0.0, cdet_fin = 0.0, cdet_sta = 0.0;
    if constexpr (ORD) {
#pragma unroll
        for (int b2 = 0; b2 <= LT; ++b2) vtop[b2] = vrow[b2];  // (workgroup-uniform: scalar loads, as long as nothing is in their way)
#pragma unroll
        for (int r = 0; r < R; ++r) ut[r] = a.utt[unsigned(r) * NT + tid];
        c_fin = a.coef_fin[bt * a.coef_bstride];
        c_sta = a.coef_sta[bt * a.coef_bstride];
        if (a.gd) {  // (uniform)
            cdet_fin = a.coef_fin[bt * a.coef_bstride + 2];
            cdet_sta = a.coef_sta[bt * a.coef_bstride + 2];
        }
    }
    double2 uu[R], ww[R], tt[R];
    unsigned xg[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned i = unsigned(r) * NT + tid;
        xg[r] = xbase | (i & lomask) | ((i >> a.lo) << a.hs);
        uu[r] = stream_load(a.v + boff + xg[r]);
    }
    if constexpr (ORD && !PACE) __builtin_amdgcn_s_barrier();  // every wave's v is requested before any wave's w
    if constexpr (PACE) {  // ... PACE: not before half of this wave's own v is back (the table entries were requested ahead of v)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    // w and t requested with v, outside of control flow (the host passes valid pointers for the first launch too): each is awaited
    // where it is first used — w after the first round, t after the second
#pragma unroll
    for (int r = 0; r < R; ++r) ww[r] = stream_load(a.w + boff + xg[r]);
    if constexpr (ORD && !PACE) __builtin_amdgcn_s_barrier();  // ... and every wave's w before any wave's t
    if constexpr (!PACE) {
#pragma unroll
        for (int r = 0; r < R; ++r) tt[r] = stream_load(a.t + boff + xg[r]);
    } else {
        __builtin_amdgcn_sched_barrier(0);  // (w is requested before anything below is awaited)
    }
    // ORD: the amplitude indices are taken afresh for each stage's stores, from a copy of tid the compiler cannot see through (as in
    // k_chain2_bwd): otherwise the 64-bit addresses of the loads stay live up to the stores and spill
    auto reindex = [&]() {
        if constexpr (ORD) {
            unsigned tid_o = tid;
            asm volatile("" : "+v"(tid_o));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const unsigned i = unsigned(r) * NT + tid_o;
                xg[r] = xbase | (i & lomask) | ((i >> a.lo) << a.hs);
            }
        }
    };
    reindex();
    double du[R];  // interaction diagonal (as k_chain)
    {
        double vloc[LT];
#pragma unroll
        for (int b2 = 0; b2 < LT; ++b2) vloc[b2] = ORD ? vtop[b2] : vrow[b2];
        double dlane = ORD ? vtop[LT] : vrow[LT];
#pragma unroll
        for (int b2 = 0; b2 < LGT; ++b2)
            if (!(tid >> b2 & 1u)) dlane += vloc[b2];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double d;
            if constexpr (ORD) d = ut[r] + dlane;
            else d = a.utt[unsigned(r) * NT + tid] + dlane;
#pragma unroll
            for (int b2 = LGT; b2 < LT; ++b2)
                if (!(r >> (b2 - LGT) & 1)) d += vloc[b2];
            du[r] = d;
        }
    }
    // D(x) of one exponential: interaction + detuning groups (ORD: the one group's coefficient was fetched at the top, cdet)
    auto diag = [&](const double* cf, [[maybe_unused]] double cdet, int r) -> double {
        double d = du[r];
        if constexpr (ORD) {  // (the same loop, so that the compiler forms the same fused multiply-adds around it: bit-identical states)
            for (int g = 0; g < a.gd; ++g) d += cdet * double(a.dcnt[g] - popc_i(xg[r] & a.dmask[g]));
        } else {
            for (int g = 0; g < a.gd; ++g) d += cf[2 + g] * double(a.dcnt[g] - popc_i(xg[r] & a.dmask[g]));
        }
        return d;
    };
    int buf = 0;  // LDS buffer the next round writes
    auto put = [&](const double2 (&val)[R]) -> const double2* {
        double2* tile = tiles + (size_t(buf) << LT);
#pragma unroll
        for (int r = 0; r < R; ++r) tile[unsigned(r) * NT + tid] = val[r];
        __syncthreads();
        buf ^= 1;
        return tile;
    };
    auto cmul = [](double xr, double xi, const double2& z) { return make_double2(xr * z.x - xi * z.y, xr * z.y + xi * z.x); };
    auto request_t = [&]() {  // (PACE) nothing moves across the request: it stands where it is written
        __builtin_amdgcn_sched_barrier(0);
        // (uniform base + 32-bit byte offset, which the 2^20 amplitudes of the largest legal shape fit: no 64-bit address per element)
        const char* tbase = reinterpret_cast<const char*>(a.t + boff);
#pragma unroll
        for (int r = 0; r < R; ++r) tt[r] = stream_load(reinterpret_cast<const double2*>(tbase + xg[r] * unsigned(sizeof(double2))));
        __builtin_amdgcn_sched_barrier(0);
    };

    double2 y[R];
    if (a.has_p) {
        const double* __restrict__ cf = a.coef_fin + bt * a.coef_bstride;
        double c;
        if constexpr (ORD) c = c_fin;
        else c = cf[0];
        double2 s[R], h1[R], ds[R];
        const double2* vtile;
        if constexpr (PACE == 2) {  // put(uu), with t requested between the tile's write (v is complete) and round A's barrier
            double2* tile = tiles + (size_t(buf) << LT);
#pragma unroll
            for (int r = 0; r < R; ++r) tile[unsigned(r) * NT + tid] = uu[r];
            request_t();
            __syncthreads();
            buf ^= 1;
            vtile = tile;
        } else {
            vtile = put(uu);
        }
        RYDIFF_TL(1);
        partner_sums<LT, LGT, false>(vtile, uu, a.fin_mask, tid, s, ds);
        if constexpr (PACE == 1) {  // only w is outstanding here: t follows once half of it is back
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            request_t();
        }
#ifdef RYDIFF_TIMELINE
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" ::"v"(ww[r].x), "v"(ww[r].y));
        RYDIFF_TL(8);  // (tuning builds: w landed in this wave)
#endif
        double d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            d[r] = diag(cf, cdet_fin, r);
            h1[r].x = d[r] * uu[r].x + c * (ww[r].x + s[r].x);
            h1[r].y = d[r] * uu[r].y + c * (ww[r].y + s[r].y);
            const double2 p = cmul(a.a_r, a.a_i, uu[r]), q = cmul(a.b_r, a.b_i, h1[r]);
            y[r] = make_double2(p.x + q.x, p.y + q.y);
        }
        RYDIFF_TL(2);
        if constexpr (PACE) {
            // Always four stores, so that the wait for t is a counted one that leaves exactly these four outstanding: behind a
            // branch it would be vmcnt(0), the counter retires in order, and t would wait for their acknowledgement.  Without a
            // destination the buffer has no records, and the range check drops every element.
            static_assert(WT >= 1, "pacing: v_mid goes through through_store");
            double2* mid_base = a.vmid_out ? a.vmid_out + boff : nullptr;
            const uint32_t mid_n = a.vmid_out ? a.dim : 0u;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double2 p = cmul(a.g1_r, a.g1_i, uu[r]), q = cmul(a.b1_r, a.b1_i, h1[r]);
                through_store(mid_base, mid_n, xg[r], make_double2(p.x + q.x, p.y + q.y));
            }
        } else if (a.vmid_out) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double2 p = cmul(a.g1_r, a.g1_i, uu[r]), q = cmul(a.b1_r, a.b1_i, h1[r]);
                out_store<(WT >= 1)>(a.vmid_out + boff, a.dim, xg[r], make_double2(p.x + q.x, p.y + q.y));
            }
        }
        if (a.k_r != 0.0 || a.k_i != 0.0) {  // (uniform) second finishing round: P_Y' e
            double2 e[R], pe[R];
#pragma unroll
            for (int r = 0; r < R; ++r) e[r] = make_double2(h1[r].x + c * ww[r].x, h1[r].y + c * ww[r].y);
            partner_sums<LT, LGT, false>(put(e), e, a.fin_mask, tid, pe, ds);
#ifdef RYDIFF_TIMELINE
#pragma unroll
            for (int r = 0; r < R; ++r) asm volatile("" ::"v"(tt[r].x), "v"(tt[r].y));
            RYDIFF_TL(9);  // (tuning builds: t landed in this wave)
#endif
#pragma unroll
            for (int r = 0; r < R; ++r) {  // H^2 v = D h1 + c (t + P_Y' e)
                const double2 z = make_double2(d[r] * h1[r].x + c * (tt[r].x + pe[r].x), d[r] * h1[r].y + c * (tt[r].y + pe[r].y));
                const double2 k = cmul(a.k_r, a.k_i, z);
                y[r].x += k.x;
                y[r].y += k.y;
            }
        } else if constexpr (PACE) {
            // a one-factor block has no use for t: its request is retired here, not behind the y stores (see the first launch, below)
#pragma unroll
            for (int r = 0; r < R; ++r) asm volatile("" ::"v"(tt[r].x), "v"(tt[r].y));
        }
        RYDIFF_TL(3);
#pragma unroll
        for (int r = 0; r < R; ++r) out_store<(WT >= 1)>(a.y_out + boff, a.dim, xg[r], y[r]);
        RYDIFF_TL(4);
        if (a.obs) {  // <y|O|y> for diagonal observables, straight from the registers that hold y
            for (int o = 0; o < a.n_obs; ++o) {
                double ex = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) ex += a.obs[size_t(o) * a.dim + xg[r]] * (y[r].x * y[r].x + y[r].y * y[r].y);
                wg_atomic_add<NT>(ex, a.expect_slot + o * a.exp_ostride + bt, red);
            }
        }
    } else {
        // A chain's first launch has no block to finish, and the host passes v for w and t as well.  ORD: y is taken from the LAST of
        // the three requests, which retires all of them on this path.  Left pending, they would make the start stage of the OTHER
        // path wait for the acknowledgement of its y stores: the compiler places its waits after the join of the two paths.
        // PACE: t is requested inside the other path, so the last request here is w.
#pragma unroll
        for (int r = 0; r < R; ++r) y[r] = PACE ? ww[r] : (ORD ? tt[r] : uu[r]);
    }
    if (!a.has_q) return;

    // start the next block in this layout: w' = P_Y y, t' = P_Y (D' y + c' w')
    reindex();
    const double* __restrict__ cf = a.coef_sta + bt * a.coef_bstride;
    double c;
    if constexpr (ORD) c = c_sta;
    else c = cf[0];
    double2 w2[R], ds[R];
    partner_sums<LT, LGT, false, true>(put(y), y, ~0u, tid, w2, ds);
#pragma unroll
    for (int r = 0; r < R; ++r) out_store<(WT >= 2)>(a.w_out + boff, a.dim, xg[r], w2[r]);
    RYDIFF_TL(5);
    double2 z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double d = diag(cf, cdet_sta, r);
        z[r] = make_double2(d * y[r].x + c * w2[r].x, d * y[r].y + c * w2[r].y);
    }
    double2 t2[R];
    partner_sums<LT, LGT, false, true>(put(z), z, ~0u, tid, t2, ds);
#pragma unroll
    for (int r = 0; r < R; ++r) out_store<(WT >= 3)>(a.t_out + boff, a.dim, xg[r], t2[r]);
    RYDIFF_TL(6);
#ifdef RYDIFF_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (tuning builds: the last stamp is taken once this wave's stores are acknowledged)
    RYDIFF_TL(7);
#endif
}

// ---- adjoint of a block (k_chain2_bwd) -------------------------------------------------------------------------------------
// The cotangent runs through the same quadratic with conjugated scalars (H real symmetric).  A block holds the factors b then a of
// one exponential (forward order; a one-factor block: b alone, a = identity), so the adjoint meets a first.  The launch that
// STARTS a block in X writes, next to the complete cotangent mu at a's output, w = P_X mu and t = P_X (D mu + c w) (k_chain2's start
// stage).  The launch that FINISHES it in Y reads mu, w, t and the tape vectors x_a, x_b (the inputs of a and b): 5R.  Round A gives
//     s = P_Y' mu,  h1 = H mu = D mu + c (w + s),  e = h1 + c w,   P mu = w + s;
// round B (skipped when k = 0) gives pe = P_Y' e, and P H mu = t + pe (as in k_chain2), so with tp = t + pe
//     mu_mid = ga~ mu + ba~ h1                  (cotangent between the two factors; never written)
//     P mu_mid = ga~ (w + s) + ba~ tp
//     mu_out = q~(H) mu = (gb~ + bb~ H) mu_mid = (gb~ + bb~ D) mu_mid + bb~ c (ga~ (w + s) + ba~ tp)
// (~: conjugate).  Both factors' gradients are exact contractions, with no further partner sums:
//     dL/dc  += Re(beta_a <P mu, x_a>) + Re(beta_b <P mu_mid, x_b>)
//     weight of d(x) (detuning group, U_ij accumulator) += Re(beta_a conj(mu) x_a) + Re(beta_b conj(mu_mid) x_b)
// Both factors belong to one exponential, so both go to the same gradient record: one wtot atomic per amplitude, one parked
// partial per quantity.  Registers (1024 threads: at most 128): mu, w, x_a are requested first, and x_a waits out round A in
// this thread's own slots of the idle LDS buffer, where e replaces it.  After round A only mu_mid, P mu and factor a's weights
// are kept; x_b and t are requested then.  x_b is consumed (factor b's weights, the wtot atomics, the (w + s) part of
// <P mu_mid, x_b>, mu_out but its tp part) before round B, and t lands during it: t is only needed as tp.  Cotangent injection
// at a save point (the state there is x_b) as in k_chain; then the next block starts on mu_out: 5R + 3W per two factors.
// Nothing after the mu_out stores waits on the vector-memory counter: the diagonal of the layout is formed once and kept for the
// start stage, both stages' coefficients are fetched at the top, and every request of the top is retired before the has_p branch,
// so the start stage's rounds run while the mu_out stores drain (they used to wait for their acknowledgement).
struct Chain2BwdArgs {
    const double2* mu;  // complete cotangent at the output of the block being finished (the start vector for the first launch)
    const double2* w;   // P_X mu                              (unused when !has_p)
    const double2* t;   // P_X (D mu + c w)                    (unused when !has_p)
    const double2* xa;  // input of factor a (one-factor block: = xb)
    const double2* xb;  // input of factor b
    double2* mu_out;    // cotangent at the block's input (written when has_p)
    double2* w_out;     // the next block's w, t (written when has_q)
    double2* t_out;
    const double* utt;  // split interaction diagonal of this layout (as ChainArgs)
    const double* vr;
    const double* coef_fin;  // coefficient record of the finished block's exponential (trajectory 0)
    const double* coef_sta;  // ... of the started block's exponential
    long coef_bstride;
    double gb_r, gb_i, bb_r, bb_i;        // conj gamma_b, conj beta_b
    double k_r, k_i;                      // conj beta_a beta_b: the H^2 coefficient of the block (0: one factor)
    double ga_r, ga_i, ba_r, ba_i;        // conj gamma_a, conj beta_a (mu_mid)
    double cba_r, cba_i, cbb_r, cbb_i;    // beta_a, beta_b un-conjugated (contraction weights; one-factor block: beta_a = 0)
    double cgb_r, cgb_i;                  // gamma_b un-conjugated (XW: x_a is rebuilt with the forward pass's own scalars, no sign flipped on the way)
    int lo, hs, hb;                       // layout of this launch (as ChainArgs)
    uint32_t dim;
    int has_p, has_q;
    int gd;                               // 0 or 1 detuning group
    uint32_t fin_mask;                    // TILE-bit mask of the Y' bits
    uint32_t dmask;
    int dcnt;
    int b_first, b_count;
    double* ge_fin;  // gradient record of the finished block's exponential (trajectory 0, replica 0): [0] dL/dc, [det_slot] dL/ddelta
    long ge_bstride, ge_rstride;
    int det_slot;    // 2 * (number of amplitude groups)
    double* wtot;    // optional U_ij-gradient accumulator [dim]
    const double2* inj_gstate;  // fused cotangent injection at a save point (as ChainArgs)
    const double* inj_gexp;
    const double* inj_obs;      // [n_obs][dim]
    int inj_n_obs;
    long inj_ostride;
};

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4, streaming policy as stream_load): no VGPR
// destination.  `lds_wave` is the wave's destination base (wave-uniform); lane l lands at lds_wave + l.  Counted on vmcnt.
__device__ __forceinline__ void stream_load_lds(const double2* g, double2* lds_wave) {
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const __attribute__((address_space(1))) void*>(reinterpret_cast<uintptr_t>(g)),
                                     (__attribute__((address_space(3))) void*)lds_wave, 16, 0, /* nt */ 2);
}

constexpr int kChain2BwdXbLds = 1;  // elements of x_b per thread that the DMA instantiation stages in LDS (the rest: registers)

// bytes of dynamic LDS: two tile buffers, [2][waves] parked partials, and (DMA) the staging area of x_b
template <int LT, int LGT, bool DMA>
constexpr size_t chain2_bwd_lds_bytes() {
    return 2 * (size_t(1) << LT) * sizeof(double2) + 2 * ((size_t(1) << LGT) / 64) * sizeof(double) +
           (DMA ? size_t(kChain2BwdXbLds) * (size_t(1) << LGT) * sizeof(double2) : 0);
}

// DMA: the tape vectors are requested at the top of the kernel with mu and w.  They never take part in a partner sum (a thread
// needs its own elements only), so x_a goes by LDS-DMA straight into this thread's slots of the idle tile buffer (where the
// register instantiation parks it) and kChain2BwdXbLds elements of x_b into a staging area behind the parked partials, which no
// put() touches: it lives until the mu_out store.  The other elements of x_b wait in registers.  Every DMA is retired (vmcnt(0))
// before round A's barrier and read after it, by the wave that issued it.  !DMA: the register-staged kernel described above.
// ORD, WT: as in k_chain2.  ORD: every wave requests mu, then (behind a bare execution barrier) w, then (behind another) the tape
// vectors.  WT: 1 mu_out, which has the whole start stage behind it | 2 also w' | 3 all.
// PACE (with ORD, !DMA; replaces the two barriers): as in k_chain2.  Each wave requests mu, waits (counted s_waitcnt) until half of
// its mu is back, and only then requests w and x_a.  Round A awaits mu alone and runs while the two land; x_a is not parked in LDS
// at all: it waits out round A's partner sums in registers (x_b and t are not live yet) and is consumed straight from them where P mu
// is formed, which is also where w is awaited.  Not on the LDS-DMA staging: with a global_load_lds pending next to ordinary loads
// the compiler treats the counter as retiring out of order and awaits mu with vmcnt(0), x_a and w included (seen in the gfx950 ISA).
// A chain's first launch retires w and x_a where it takes y.
// XW (vector-major, register-staged, everything written through; a pacing of its own, PACE = 0): the tape holds w_x = P_X x_b, the
// forward block's own w, where x_a would be (pair_wtape, pair_launch.hpp), and the kernel rebuilds x_a, the forward pass's v_mid:
//     s_x = P_Y' x_b,   x_a = gamma_b x_b + beta_b ((D x_b) + c (w_x + s_x))
// in the statement order of k_chain2, so to the last bit.  The host runs the launch in the layout in which the forward pass finished
// the block, so the Y' bits are those of this launch's fin_mask.  Requests: x_b; once half of it is back, w_x and mu; w when x_b is
// complete.  x_b goes as a tile into the idle LDS buffer (this thread's slots are where x_a is parked by the unpaced kernel), one
// barrier, the x-round's partner sums, x_a in registers; then round A on mu as in the paced kernel.  Round A's barrier retires every
// partner read of the x_b tile, and x_b's own elements are read back from this thread's slots just before e replaces them: x_b has
// no second load phase and only t is requested behind round A.  A one-factor block (x_a is not used: beta_a = 0) skips the x-round.
template <int LT, int LGT, bool ORD, int WT, bool DMA, int PACE = 0, bool XW = false>
__global__ __launch_bounds__(1 << LGT) void k_chain2_bwd(Chain2BwdArgs a) {
    constexpr int NT = 1 << LGT, R = 1 << (LT - LGT), NW = NT / 64;
    static_assert(WT >= 0 && WT <= 3);
    static_assert(!XW || (ORD && WT == 3 && !DMA && !PACE && R == 4), "P_X x_b on the tape: one instantiation");
    static_assert(PACE >= 0 && PACE <= 1 && (!PACE || (ORD && !DMA && R == 4)), "pacing: the vector-major register-staged kernel, four elements per thread");
    constexpr int XBL = DMA ? kChain2BwdXbLds : 0;
    static_assert(XBL <= R && (2 * NW * sizeof(double)) % sizeof(double2) == 0);
    extern __shared__ __attribute__((aligned(16))) double2 tiles[];
    double* red = reinterpret_cast<double*>(tiles + 2 * (size_t(1) << LT));  // [2][NW] parked gradient partials: dL/dc, dL/ddelta
    double2* xbs = tiles + 2 * (size_t(1) << LT) + 2 * NW * sizeof(double) / sizeof(double2);  // (DMA) [XBL][NT] staged x_b
    const unsigned tid = threadIdx.x;
    const unsigned t = blockIdx.x;
    const unsigned bl = blockIdx.y;
    if (bl >= unsigned(a.b_count)) return;
    const unsigned bt = unsigned(a.b_first) + bl;
    const size_t boff = size_t(bt) * a.dim;
    const unsigned lomask = (1u << a.lo) - 1u;
    const int midlow = a.hs - a.lo;
    const unsigned xbase = ((t & ((1u << midlow) - 1u)) << a.lo) | ((t >> midlow) << (a.hs + a.hb));
    if (tid < 2 * NW) red[tid] = 0.0;  // published by the barrier of the first round
    RYDIFF_TL(0);
    double2 uu[R], ww[R], xb[R], tp[R];
    unsigned xg[R];
    // the amplitude indices (and the 64-bit offsets derived from them) are taken afresh for each stage's stores, from a copy of
    // tid the compiler cannot see through: otherwise they stay live from the first loads to the last stores and spill
    auto reindex = [&]() {
        unsigned tid_o = tid;
        asm volatile("" : "+v"(tid_o));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned i = unsigned(r) * NT + tid_o;
            xg[r] = xbase | (i & lomask) | ((i >> a.lo) << a.hs);
        }
    };
    // interaction diagonal (as k_chain): its table entries (L2 hits) are requested ahead of the streamed vectors, branch-free, so that
    // they neither wait for those nor cost a round trip of their own once those have landed
    double vloc[LT + 1], ut[R];
    {
        const double* __restrict__ vrow = a.vr + size_t(t) * 16;
#pragma unroll
        for (int b2 = 0; b2 <= LT; ++b2) vloc[b2] = vrow[b2];
#pragma unroll
        for (int r = 0; r < R; ++r) ut[r] = a.utt[unsigned(r) * NT + tid];
    }
    // ... and so are the drive and detuning coefficients of both stages (the host passes loadable records for the first and the
    // last launch too)
    double c_fin = a.coef_fin[bt * a.coef_bstride], c_sta = a.coef_sta[bt * a.coef_bstride], cdet_fin = 0.0, cdet_sta = 0.0;
    if (a.gd) {  // (uniform)
        cdet_fin = a.coef_fin[bt * a.coef_bstride + 2];
        cdet_sta = a.coef_sta[bt * a.coef_bstride + 2];
    }
    [[maybe_unused]] double2 xa[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned i = unsigned(r) * NT + tid;
        xg[r] = xbase | (i & lomask) | ((i >> a.lo) << a.hs);
        if constexpr (XW) xb[r] = stream_load(a.xb + boff + xg[r]);
        else uu[r] = stream_load(a.mu + boff + xg[r]);
    }
    if constexpr (ORD && !PACE && !XW) __builtin_amdgcn_s_barrier();  // every wave's mu is requested before any wave's w
    if constexpr (PACE || XW) {  // ... PACE: not before half of this wave's own mu is back (the table entries were requested ahead of mu)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    // w and x_a requested with mu, outside of control flow (the host passes valid pointers for the first launch too)
    // (XW: w_x, in the slot of x_a, and mu behind half of x_b; w follows inside the has_p path, once x_b is complete)
    if constexpr (!XW) {
#pragma unroll
        for (int r = 0; r < R; ++r) ww[r] = stream_load(a.w + boff + xg[r]);
    }
    if constexpr (ORD && !PACE && !XW) __builtin_amdgcn_s_barrier();  // ... and every wave's w before any wave's tape vector
    if constexpr (XW) {
#pragma unroll
        for (int r = 0; r < R; ++r) xa[r] = stream_load(a.xa + boff + xg[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) uu[r] = stream_load(a.mu + boff + xg[r]);
    } else if constexpr (DMA) {
        const unsigned wv = __builtin_amdgcn_readfirstlane(tid & ~63u);  // a wave's 64 slots of one r are 1 KiB of contiguous LDS
        double2* xat = tiles + (size_t(1) << LT);                        // the idle buffer of round A (buf ^ 1)
#pragma unroll
        for (int r = 0; r < R; ++r) stream_load_lds(a.xa + boff + xg[r], xat + unsigned(r) * NT + wv);
#pragma unroll
        for (int r = 0; r < XBL; ++r) stream_load_lds(a.xb + boff + xg[r], xbs + unsigned(r) * NT + wv);
#pragma unroll
        for (int r = XBL; r < R; ++r) xb[r] = stream_load(a.xb + boff + xg[r]);
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) xa[r] = stream_load(a.xa + boff + xg[r]);
    }
    __builtin_amdgcn_sched_barrier(0);  // (every request above is issued before the first wait)
    auto uniform = [](double v) {  // (workgroup-uniform values: scalar registers)
        return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    };
    c_fin = uniform(c_fin);
    c_sta = uniform(c_sta);
    cdet_fin = uniform(cdet_fin);
    cdet_sta = uniform(cdet_sta);
    double du[R];  // kept for both stages: the finish and the start stage work in the same layout
    {
        double dlane = vloc[LT];
#pragma unroll
        for (int b2 = 0; b2 < LGT; ++b2) dlane = (tid >> b2 & 1u) ? dlane : dlane + vloc[b2];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double d = ut[r] + dlane;
#pragma unroll
            for (int b2 = LGT; b2 < LT; ++b2)
                if (!(r >> (b2 - LGT) & 1)) d += vloc[b2];
            du[r] = d;
        }
    }
    auto cnt = [&](int r) -> double { return a.gd ? double(a.dcnt - popc_i(xg[r] & a.dmask)) : 0.0; };
    int buf = 0;  // LDS buffer the next round writes
    auto put = [&](const double2 (&val)[R]) -> const double2* {
        double2* tile = tiles + (size_t(buf) << LT);
#pragma unroll
        for (int r = 0; r < R; ++r) tile[unsigned(r) * NT + tid] = val[r];
        __syncthreads();
        buf ^= 1;
        return tile;
    };
    auto cmul = [](double xr, double xi, const double2& z) { return make_double2(xr * z.x - xi * z.y, xr * z.y + xi * z.x); };
    auto cdot = [](const double2& p, const double2& x) { return make_double2(p.x * x.x + p.y * x.y, p.x * x.y - p.y * x.x); };  // conj(p) x
    auto xbv = [&](int r) -> double2 { return r < XBL ? xbs[unsigned(r) * NT + tid] : xb[r]; };  // x_b: staged in LDS or in registers

    // Every request of the top is retired here, on both paths (round A's barrier needs all of them anyway: x_a sits in LDS before it).
    // Left pending on the path of a chain's first launch, which does not use them, they would make the start stage of the OTHER path
    // wait for the acknowledgement of its mu_out stores: the compiler places its waits after the join of the two paths.
#ifdef RYDIFF_TIMELINE
#pragma unroll
    for (int r = 0; r < R; ++r) asm volatile("" ::"v"(uu[r].x), "v"(uu[r].y));
    RYDIFF_TL(8);  // (tuning builds: mu landed in this wave, apart from w and x_a)
#endif
    // PACE: mu alone is awaited here; w and x_a are retired behind round A's partner sums, or on the first launch's path
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if constexpr (XW) {
            asm volatile("" ::"v"(xb[r].x), "v"(xb[r].y));  // (x_b alone: w_x and mu are retired where they are used, or on the first launch's path)
        } else if constexpr (PACE) {
            asm volatile("" ::"v"(uu[r].x), "v"(uu[r].y));
        } else {
            asm volatile("" ::"v"(uu[r].x), "v"(uu[r].y), "v"(ww[r].x), "v"(ww[r].y));
            if constexpr (!DMA) asm volatile("" ::"v"(xa[r].x), "v"(xa[r].y));
            if (DMA && r >= XBL) asm volatile("" ::"v"(xb[r].x), "v"(xb[r].y));
        }
    }
    double2 y[R];
    if (a.has_p) {
        const double c = c_fin, cdet = cdet_fin;
        double2 pm[R], mid[R];  // P mu, mu_mid: kept until x_b arrives (mu_out is formed from them, not from mu and H mu)
        double wx[R];           // Re(beta_a conj(mu) x_a): factor a's weight of d(x) (factor b's, Re(beta_b conj(mu_mid) x_b), joins it)
        double zc = 0.0;  // Re(beta_a <P mu, x_a>) + Re(beta_b <P mu_mid, x_b>): dL/dc
        const bool two = a.k_r != 0.0 || a.k_i != 0.0;  // (uniform) a second finishing round: P_Y' e
        {
            // x_a waits out round A in this thread's own slots of the other LDS buffer (not in registers); e replaces it there
            // (DMA: it is there already, retired by the vmcnt(0) in front of round A's barrier)
            double2* etile = tiles + (size_t(buf ^ 1) << LT);
            if constexpr (XW) {
                __builtin_amdgcn_sched_barrier(0);  // w is requested now that x_b is complete: it lands under the x-round and round A
                {
                    const char* wbase = reinterpret_cast<const char*>(a.w + boff);
#pragma unroll
                    for (int r = 0; r < R; ++r) ww[r] = stream_load(reinterpret_cast<const double2*>(wbase + xg[r] * unsigned(sizeof(double2))));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < R; ++r) etile[unsigned(r) * NT + tid] = xb[r];
                if (two) {  // the x-round: x_a = v_mid of the forward block, statement for statement as in k_chain2
                    __syncthreads();
                    RYDIFF_TL(11);
                    double2 sx[R], dsx[R];
                    partner_sums<LT, LGT, false>(etile, xb, a.fin_mask, tid, sx, dsx);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double d = du[r];
                        if (a.gd) d += cdet * double(a.dcnt - popc_i(xg[r] & a.dmask));
                        double2 h1;
                        h1.x = d * xb[r].x + c * (xa[r].x + sx[r].x);
                        h1.y = d * xb[r].y + c * (xa[r].y + sx[r].y);
                        const double2 p = cmul(a.cgb_r, a.cgb_i, xb[r]), q = cmul(a.cbb_r, a.cbb_i, h1);
                        xa[r] = make_double2(p.x + q.x, p.y + q.y);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        asm volatile("" ::"v"(xa[r].x), "v"(xa[r].y));  // (its request retired)
                        xa[r] = xb[r];
                    }
                }
            } else if constexpr (PACE) {
                // (nothing: x_a stays in registers and is awaited behind the partner sums)
            } else if constexpr (DMA) {
#ifdef RYDIFF_TIMELINE
                RYDIFF_TL(9);  // (tuning builds: w landed in this wave, retired above)
#endif
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
#ifdef RYDIFF_TIMELINE
                RYDIFF_TL(9);
#endif
#pragma unroll
                for (int r = 0; r < R; ++r) etile[unsigned(r) * NT + tid] = xa[r];
            }
#ifdef RYDIFF_TIMELINE
            if constexpr (!PACE && !XW) RYDIFF_TL(10);  // (tuning builds: x_a landed in this wave)
#endif
            double2 s[R], ds[R];
            const double2* mtile = put(uu);
            RYDIFF_TL(1);
            partner_sums<LT, LGT, false>(mtile, uu, a.fin_mask, tid, s, ds);
#ifdef RYDIFF_TIMELINE
            if constexpr (PACE || XW) {
#pragma unroll
                for (int r = 0; r < R; ++r) asm volatile("" ::"v"(ww[r].x), "v"(ww[r].y));
                RYDIFF_TL(9);
#pragma unroll
                for (int r = 0; r < R; ++r) asm volatile("" ::"v"(xa[r].x), "v"(xa[r].y));
                RYDIFF_TL(10);
            }
#endif
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double2 xav;
                if constexpr (PACE || XW) xav = xa[r];
                else xav = etile[unsigned(r) * NT + tid];
                if constexpr (XW) xb[r] = etile[unsigned(r) * NT + tid];  // x_b's own element, before e replaces it
                const double d = du[r] + cdet * cnt(r);
                pm[r] = make_double2(ww[r].x + s[r].x, ww[r].y + s[r].y);
                const double2 h1 = make_double2(d * uu[r].x + c * pm[r].x, d * uu[r].y + c * pm[r].y);  // H mu
                if (two) etile[unsigned(r) * NT + tid] = make_double2(h1.x + c * ww[r].x, h1.y + c * ww[r].y);  // e = h1 + c w
                const double2 q1 = cdot(pm[r], xav);
                zc += a.cba_r * q1.x - a.cba_i * q1.y;
                const double2 wa = cdot(uu[r], xav);
                wx[r] = a.cba_r * wa.x - a.cba_i * wa.y;
                const double2 mm = cmul(a.ga_r, a.ga_i, uu[r]), mh = cmul(a.ba_r, a.ba_i, h1);
                mid[r] = make_double2(mm.x + mh.x, mm.y + mh.y);
            }
        }
        park1<NW>(zc, red, 0);  // factor a's drive contraction is complete: parked now, not kept through round B
        zc = 0.0;
        RYDIFF_TL(2);
        // the second tape vector (!DMA) and t (needed as tp = t + P_Y' e only) are requested once round A is done
        if constexpr (!DMA && !XW) {
#pragma unroll
            for (int r = 0; r < R; ++r) xb[r] = stream_load(a.xb + boff + xg[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) tp[r] = stream_load(a.t + boff + xg[r]);
        reindex();  // (the indices of round A are not kept through the second load)
        double sgd = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double2 xbr = xbv(r);
            const double2 wb = cdot(mid[r], xbr);
            const double wr = wx[r] + (a.cbb_r * wb.x - a.cbb_i * wb.y);
            if (a.wtot) unsafeAtomicAdd(a.wtot + xg[r], wr);  // both factors: one atomic
            sgd += wr * cnt(r);
            const double2 gpm = cmul(a.ga_r, a.ga_i, pm[r]);
            const double2 q = cdot(gpm, xbr);
            zc += a.cbb_r * q.x - a.cbb_i * q.y;
            // mu_out = (gb~ + bb~ H) mu_mid, H mu_mid = d mu_mid + c (ga~ P mu + ba~ tp): all but the tp part now
            const double d = du[r] + cdet * cnt(r);
            const double2 y1 = cmul(a.gb_r + a.bb_r * d, a.gb_i + a.bb_i * d, mid[r]), y2 = cmul(a.bb_r * c, a.bb_i * c, gpm);
            y[r] = make_double2(y1.x + y2.x, y1.y + y2.y);
        }
        // x_b is consumed before round B starts: its partner reads must not be scheduled while P mu and mu_mid are still live
        __builtin_amdgcn_sched_barrier(0);
        RYDIFF_TL(3);
        if (two) {
            __syncthreads();  // e published
            buf ^= 1;
        }
        if (two) {  // second finishing round, partners from LDS only: tp += P_Y' e
            const double2* tile = tiles + (size_t(buf ^ 1) << LT);
#pragma unroll
            for (int b = 0; b < LT; ++b) {
                if (a.fin_mask >> b & 1u) {  // wave-uniform
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double2 q = tile[(unsigned(r) * NT + tid) ^ (1u << b)];
                        tp[r].x += q.x;
                        tp[r].y += q.y;
                    }
                }
            }
        }
        const double kc_r = a.k_r * c, kc_i = a.k_i * c;  // bb~ c ba~
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double2 kt = cmul(kc_r, kc_i, tp[r]);
            y[r].x += kt.x;
            y[r].y += kt.y;
            const double2 q = cdot(cmul(a.ba_r, a.ba_i, tp[r]), xbv(r));  // (one-factor block: ba~ = 0)
            zc += a.cbb_r * q.x - a.cbb_i * q.y;
        }
        RYDIFF_TL(4);
        park2<NW>(zc, sgd, red, 0, 1);
        reindex();
        if (a.inj_gexp || a.inj_gstate) {  // wave-uniform: the completed cotangent sits at a save point whose state is x_b
            if (a.inj_gexp) {
                bool any = false;
                for (int o = 0; o < a.inj_n_obs; ++o) any |= a.inj_gexp[o * a.inj_ostride + bt] != 0.0;
                if (any) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double wsum = 0.0;
                        for (int o = 0; o < a.inj_n_obs; ++o) wsum += a.inj_gexp[o * a.inj_ostride + bt] * a.inj_obs[size_t(o) * a.dim + xg[r]];
                        const double2 xbr = xbv(r);
                        y[r].x += 2.0 * wsum * xbr.x;
                        y[r].y += 2.0 * wsum * xbr.y;
                    }
                }
            }
            if (a.inj_gstate) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double2 gs = stream_load(a.inj_gstate + boff + xg[r]);
                    y[r].x += gs.x;
                    y[r].y += gs.y;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) out_store<(WT >= 1)>(a.mu_out + boff, a.dim, xg[r], y[r]);
        RYDIFF_TL(5);
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            y[r] = uu[r];
            if constexpr (PACE) asm volatile("" ::"v"(ww[r].x), "v"(ww[r].y), "v"(xa[r].x), "v"(xa[r].y));  // (every request of the top retired)
            if constexpr (XW) asm volatile("" ::"v"(xa[r].x), "v"(xa[r].y));
        }
    }
    auto flush = [&]() {  // after the barrier that follows the parks: one atomic per quantity and workgroup
        if (a.has_p && tid < 2) {
            double sum = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) sum += red[tid * NW + w];
            double* ge = a.ge_fin + bt * a.ge_bstride + (blockIdx.x % kGradReplicas) * a.ge_rstride;
            if (sum != 0.0) unsafeAtomicAdd(ge + (tid ? a.det_slot : 0), sum);
        }
    };
    if (!a.has_q) {
        __syncthreads();
        flush();
        return;
    }

    // start the next block in this layout: w' = P_Y mu_out, t' = P_Y (D' mu_out + c' w')
    const double c = c_sta, cdet = cdet_sta;
    reindex();
    double2 w2[R], ds[R];
    partner_sums<LT, LGT, false, true>(put(y), y, ~0u, tid, w2, ds);
#pragma unroll
    for (int r = 0; r < R; ++r) out_store<(WT >= 2)>(a.w_out + boff, a.dim, xg[r], w2[r]);
    RYDIFF_TL(6);
    double2 z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double d = du[r] + cdet * cnt(r);
        z[r] = make_double2(d * y[r].x + c * w2[r].x, d * y[r].y + c * w2[r].y);
    }
    double2 t2[R];
    partner_sums<LT, LGT, false, true>(put(z), z, ~0u, tid, t2, ds);
#pragma unroll
    for (int r = 0; r < R; ++r) out_store<(WT >= 3)>(a.t_out + boff, a.dim, xg[r], t2[r]);
    RYDIFF_TL(7);
    flush();  // (the barriers of the start rounds published the parked partials)
}
