// xy_launch.hpp — launches of the XY exchange family (xy_kernels.hpp).  launch_factor / launch_factor_bwd / launch_dot_h
// (direct_launch.hpp) hand over to these whenever the problem carries the exchange (Plan::xy_mode != 0); with xy_mode == 0 nothing
// here is reached.
#pragma once

namespace {

int launch_factor_xy(const Runtime& rt, char* ws, const double2* xin, double2* xout, int stage, const FactorScalars& s, hipStream_t stream) {
    const Plan& pl = rt.pl;
    FactorArgs fa{};
    fill_factor(fa, rt, ws, stage, s);
    fa.xin = xin;
    fa.xout = xout;
    hipLaunchKernelGGL(k_factor_xy, dim3(unsigned((pl.dim + 255) / 256), pl.B), dim3(256), 0, stream, fa, rt.xarg);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// rt.xy_ge: the gradient replicas of this backward call (nullptr: g_xy not asked for — the contractions are skipped)
int launch_factor_bwd_xy(const Runtime& rt, char* ws, const double2* gin, const double2* xin, double2* gout, int stage,
                         const FactorScalars& s, double* wtot, const InjectSource& inj, int save_k, hipStream_t stream) {
    const Plan& pl = rt.pl;
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
    fill_inject(ba, inj, save_k, pl);
    hipLaunchKernelGGL(k_factor_bwd_xy, dim3(unsigned((pl.dim + 255) / 256), pl.B), dim3(256), 0, stream, ba, rt.xarg, rt.xy_ge);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

int launch_dot_h_xy(const Runtime& rt, char* ws, int stage, const double2* g, const double2* xout, const BatchSlice& bs, hipStream_t stream) {
    const Plan& pl = rt.pl;
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
    hipLaunchKernelGGL(k_dot_hx_xy, dim3(unsigned((pl.dim + 255) / 256), unsigned(bs.count)), dim3(256), 0, stream, da, rt.xarg);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// the replicas -> g_xy (overwritten), once per backward call
int xy_contract(const Runtime& rt, double* g_xy, hipStream_t stream) {
    const int P = rt.pl.N * (rt.pl.N - 1) / 2;
    if (!g_xy || !rt.xy_ge || P == 0) return RYDIFF_OK;
    hipLaunchKernelGGL(k_xy_contract, dim3(unsigned((P + 127) / 128)), dim3(128), 0, stream, g_xy, rt.xy_ge, P);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

}  // namespace
