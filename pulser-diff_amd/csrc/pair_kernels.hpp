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

template <int LT, int LGT>
__global__ __launch_bounds__(1 << LGT) void k_chain2(Chain2Args a) {
    constexpr int NT = 1 << LGT, R = 1 << (LT - LGT);
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
    double2 uu[R], ww[R], tt[R];
    unsigned xg[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned i = unsigned(r) * NT + tid;
        xg[r] = xbase | (i & lomask) | ((i >> a.lo) << a.hs);
        uu[r] = stream_load(a.v + boff + xg[r]);
    }
    // w and t requested with v, outside of control flow (the host passes valid pointers for the first launch too): each is awaited
    // where it is first used — w after the first round, t after the second
#pragma unroll
    for (int r = 0; r < R; ++r) ww[r] = stream_load(a.w + boff + xg[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) tt[r] = stream_load(a.t + boff + xg[r]);
    double du[R];  // interaction diagonal (as k_chain)
    {
        const double* __restrict__ vrow = a.vr + size_t(t) * 16;
        double vloc[LT];
#pragma unroll
        for (int b2 = 0; b2 < LT; ++b2) vloc[b2] = vrow[b2];
        double dlane = vrow[LT];
#pragma unroll
        for (int b2 = 0; b2 < LGT; ++b2)
            if (!(tid >> b2 & 1u)) dlane += vloc[b2];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double d = a.utt[unsigned(r) * NT + tid] + dlane;
#pragma unroll
            for (int b2 = LGT; b2 < LT; ++b2)
                if (!(r >> (b2 - LGT) & 1)) d += vloc[b2];
            du[r] = d;
        }
    }
    auto diag = [&](const double* cf, int r) -> double {  // D(x) of one exponential: interaction + detuning groups
        double d = du[r];
        for (int g = 0; g < a.gd; ++g) d += cf[2 + g] * double(a.dcnt[g] - popc_i(xg[r] & a.dmask[g]));
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

    double2 y[R];
    if (a.has_p) {
        const double* __restrict__ cf = a.coef_fin + bt * a.coef_bstride;
        const double c = cf[0];
        double2 s[R], h1[R], ds[R];
        partner_sums<LT, LGT, false>(put(uu), uu, a.fin_mask, tid, s, ds);
        double d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            d[r] = diag(cf, r);
            h1[r].x = d[r] * uu[r].x + c * (ww[r].x + s[r].x);
            h1[r].y = d[r] * uu[r].y + c * (ww[r].y + s[r].y);
            const double2 p = cmul(a.a_r, a.a_i, uu[r]), q = cmul(a.b_r, a.b_i, h1[r]);
            y[r] = make_double2(p.x + q.x, p.y + q.y);
        }
        if (a.vmid_out) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double2 p = cmul(a.g1_r, a.g1_i, uu[r]), q = cmul(a.b1_r, a.b1_i, h1[r]);
                stream_store(a.vmid_out + boff + xg[r], make_double2(p.x + q.x, p.y + q.y));
            }
        }
        if (a.k_r != 0.0 || a.k_i != 0.0) {  // (uniform) second finishing round: P_Y' e
            double2 e[R], pe[R];
#pragma unroll
            for (int r = 0; r < R; ++r) e[r] = make_double2(h1[r].x + c * ww[r].x, h1[r].y + c * ww[r].y);
            partner_sums<LT, LGT, false>(put(e), e, a.fin_mask, tid, pe, ds);
#pragma unroll
            for (int r = 0; r < R; ++r) {  // H^2 v = D h1 + c (t + P_Y' e)
                const double2 z = make_double2(d[r] * h1[r].x + c * (tt[r].x + pe[r].x), d[r] * h1[r].y + c * (tt[r].y + pe[r].y));
                const double2 k = cmul(a.k_r, a.k_i, z);
                y[r].x += k.x;
                y[r].y += k.y;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) stream_store(a.y_out + boff + xg[r], y[r]);
        if (a.obs) {  // <y|O|y> for diagonal observables, straight from the registers that hold y
            for (int o = 0; o < a.n_obs; ++o) {
                double ex = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) ex += a.obs[size_t(o) * a.dim + xg[r]] * (y[r].x * y[r].x + y[r].y * y[r].y);
                wg_atomic_add<NT>(ex, a.expect_slot + o * a.exp_ostride + bt, red);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) y[r] = uu[r];
    }
    if (!a.has_q) return;

    // start the next block in this layout: w' = P_Y y, t' = P_Y (D' y + c' w')
    const double* __restrict__ cf = a.coef_sta + bt * a.coef_bstride;
    const double c = cf[0];
    double2 w2[R], ds[R];
    partner_sums<LT, LGT, false, true>(put(y), y, ~0u, tid, w2, ds);
#pragma unroll
    for (int r = 0; r < R; ++r) stream_store(a.w_out + boff + xg[r], w2[r]);
    double2 z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double d = diag(cf, r);
        z[r] = make_double2(d * y[r].x + c * w2[r].x, d * y[r].y + c * w2[r].y);
    }
    double2 t2[R];
    partner_sums<LT, LGT, false, true>(put(z), z, ~0u, tid, t2, ds);
#pragma unroll
    for (int r = 0; r < R; ++r) stream_store(a.t_out + boff + xg[r], t2[r]);
}
