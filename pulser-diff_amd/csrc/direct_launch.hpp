// direct_launch.hpp — launches of the one-amplitude-per-thread kernels (direct_kernels.hpp): forward factor, adjoint factor, dL/dtau.
#pragma once

namespace {

// the XY exchange family (xy_launch.hpp): every launch below hands over to it when the problem carries the exchange
int launch_factor_xy(const Runtime& rt, char* ws, const double2* xin, double2* xout, int stage, const FactorScalars& s, hipStream_t stream);
int launch_factor_bwd_xy(const Runtime& rt, char* ws, const double2* gin, const double2* xin, double2* gout, int stage,
                         const FactorScalars& s, double* wtot, const InjectSource& inj, int save_k, hipStream_t stream);
int launch_dot_h_xy(const Runtime& rt, char* ws, int stage, const double2* g, const double2* xout, const BatchSlice& bs, hipStream_t stream);

// one global drive on a 12..20-qubit register without pair terms: the unrolled direct kernels (k_factor_direct_global)
bool direct_global_ok(const Runtime& rt) {
    const Plan& pl = rt.pl;
    return !rt.generic_direct && !pl.shard_bits && !pl.xy_mode && pl.N >= 12 && pl.N <= 20 && pl.n_pair == 0 && pl.ga.n == 1 &&
           pl.ga.amp_index_mask[0] == (1u << pl.N) - 1u;
}

// Launch KERNEL<N, ONEXCD> for the register size at hand, or GENERIC where direct_global_ok() says no (uses `rt` and `stream` of
// the calling function).  One XCD has the CUs for <= 32 workgroups (12, 13 qubits: ONEXCD instantiations on an 8x oversubscribed
// grid); beyond, spreading wins (measured).
#define RYDIFF_CASE(KERNEL, NQ, ONEXCD, GRID, ARGS) case NQ: hipLaunchKernelGGL((KERNEL<NQ, ONEXCD>), GRID, dim3(256), 0, stream, ARGS); break;
#define RYDIFF_LAUNCH_DIRECT(KERNEL, GENERIC, ARGS)                                                                          \
    do {                                                                                                                     \
        const dim3 grid_(unsigned((rt.pl.dim + 255) / 256), rt.pl.B), grid8_(grid_.x * 8, grid_.y);                          \
        if (!direct_global_ok(rt)) hipLaunchKernelGGL(GENERIC, grid_, dim3(256), 0, stream, ARGS);                           \
        else switch (rt.pl.N) {                                                                                              \
            RYDIFF_CASE(KERNEL, 12, true, grid8_, ARGS) RYDIFF_CASE(KERNEL, 13, true, grid8_, ARGS)                          \
            RYDIFF_CASE(KERNEL, 14, false, grid_, ARGS) RYDIFF_CASE(KERNEL, 15, false, grid_, ARGS)                          \
            RYDIFF_CASE(KERNEL, 16, false, grid_, ARGS) RYDIFF_CASE(KERNEL, 17, false, grid_, ARGS)                          \
            RYDIFF_CASE(KERNEL, 18, false, grid_, ARGS) RYDIFF_CASE(KERNEL, 19, false, grid_, ARGS)                          \
            RYDIFF_CASE(KERNEL, 20, false, grid_, ARGS)                                                                      \
        }                                                                                                                    \
        LAUNCH_CHECK();                                                                                                      \
    } while (0)

// what FactorArgs and FactorBwdArgs have in common: tables, the exponential's coefficient record, the factor's scalars, groups
template <class Args>
void fill_factor(Args& a, const Runtime& rt, char* ws, int stage, const FactorScalars& s) {
    const Plan& pl = rt.pl;
    a.udiag = reinterpret_cast<const double*>(ws + pl.off_udiag);
    a.coef = rt.coef(ws, stage);
    a.coef_bstride = rt.coef_bstride();
    a.dim = uint32_t(pl.dim);
    a.gr = s.gr;
    a.gi = s.gi;
    a.br = s.br;
    a.bi = s.bi;
    a.g = rt.garg;
    a.pair = rt.parg;
    fill_shard(a, rt);  // (forward: the partner ranks' state slabs; adjoint: their cotangent slabs)
    if (pl.shard_bits)  // in-slab flips only; the rank bits are the partner slabs
        for (int q = 0; q < a.g.ga; ++q) a.g.amask[q] &= uint32_t(pl.dim - 1);
}

// obs / expect_slot: fuse <y|O|y> into this launch where the kernel can (returns *fused = true then)
int launch_factor(const Runtime& rt, char* ws, const double2* xin, double2* xout, int stage, const FactorScalars& s, hipStream_t stream,
                  const double* obs = nullptr, double* expect_slot = nullptr, bool* fused = nullptr) {
    const Plan& pl = rt.pl;
    if (fused) *fused = false;
    if (pl.xy_mode) return launch_factor_xy(rt, ws, xin, xout, stage, s, stream);
    FactorArgs fa{};
    fill_factor(fa, rt, ws, stage, s);
    fa.xin = xin;
    fa.xout = xout;
    if (direct_global_ok(rt) && obs && expect_slot) {
        fa.obs = obs;
        fa.expect_slot = expect_slot;
        fa.n_obs = pl.n_obs;
        fa.exp_ostride = long(pl.T + 1) * pl.B;
        if (fused) *fused = true;
    }
    RYDIFF_LAUNCH_DIRECT(k_factor_direct_global, k_factor_direct, fa);
    return RYDIFF_OK;
}

// Adjoint of one factor: gout = cotangent w.r.t. the factor's input xin, gradient contractions into the exponential's record.
// save_k >= 0: gout is the cotangent at save point save_k — add what is injected there (fused).
int launch_factor_bwd(const Runtime& rt, char* ws, const double2* gin, const double2* xin, double2* gout, int stage,
                      const FactorScalars& s, double* wtot, const InjectSource& inj, int save_k, hipStream_t stream) {
    const Plan& pl = rt.pl;
    if (pl.xy_mode) return launch_factor_bwd_xy(rt, ws, gin, xin, gout, stage, s, wtot, inj, save_k, stream);
    FactorBwdArgs ba{};
    fill_factor(ba, rt, ws, stage, s);
    ba.gin = gin;
    ba.xin = xin;
    ba.gout = gout;
    ba.ge = rt.ge(ws, stage);
    ba.ge_bstride = rt.ge_bstride();
    ba.ge_rstride = pl.NC + 1;
    ba.wtot = wtot;
    ba.obs_bstride = rt.obs_bstride();
    ba.obs_ostride = rt.obs_ostride();
    fill_inject(ba, inj, save_k, pl);  // every launch finishes its factor: no further condition
    RYDIFF_LAUNCH_DIRECT(k_factor_bwd_direct_global, k_factor_bwd_direct, ba);
    return RYDIFF_OK;
}

// dL/dtau of exponential `stage`, taken at its output xout with the cotangent g there (k_dot_hx), for the trajectories of `bs`.
// State-sharded runs apply H to g instead (DotHArgs); with ranks elsewhere shard_recv[] must hold the partners' copies of g by now.
int launch_dot_h(const Runtime& rt, char* ws, int stage, const double2* g, const double2* xout, const BatchSlice& bs, hipStream_t stream) {
    const Plan& pl = rt.pl;
    if (pl.xy_mode) return launch_dot_h_xy(rt, ws, stage, g, xout, bs, stream);
    DotHArgs da{};
    da.g = g;
    da.x = xout;
    da.udiag = reinterpret_cast<const double*>(ws + pl.off_udiag);
    da.coef = rt.coef(ws, stage);
    da.coef_bstride = rt.coef_bstride();
    da.out = rt.ge(ws, stage) + pl.NC;
    da.out_bstride = rt.ge_bstride();
    da.out_rstride = pl.NC + 1;
    da.dim = uint32_t(pl.dim);
    da.b_first = bs.first;
    da.gr = rt.garg;
    da.pair = rt.parg;
    fill_shard(da, rt);  // (the partner ranks' cotangent slabs: the caller has waited for them, shard_signal phase 1)
    if (pl.shard_bits)   // in-slab flips only; the rank bits are the partner slabs
        for (int q = 0; q < da.gr.ga; ++q) da.gr.amask[q] &= uint32_t(pl.dim - 1);
    hipLaunchKernelGGL(k_dot_hx, dim3(unsigned((pl.dim + 255) / 256), unsigned(bs.count)), dim3(256), 0, stream, da);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

#undef RYDIFF_LAUNCH_DIRECT
#undef RYDIFF_CASE

}  // namespace
