// moments_launch.hpp — occupation correlations (moments_kernels.hpp): the evaluation launches of the forward sweeps, the moment
// tangents of the tangent sweep (tangent_launch.hpp: launch_expect_tangent) and the moments part of the observable cotangent
// (overlap_launch.hpp: launch_observable_cotangent).
#pragma once

namespace {

// the rows of save points k0 .. k0 + nk - 1 from the tile records `rec` ([n_dir][nk][B][79][tiles], n_dir = 1: the values)
void launch_moments_finish(const ForwardCtx& c, const double* rec, double* out, int k0, int nk, const BatchSlice& bs, int n_dir,
                           size_t rec_dstride, size_t out_dstride) {
    const Plan& pl = c.rt.pl;
    MomentsFinishArgs f{};
    f.rec = rec;
    f.out = out;
    f.N = pl.N;
    f.n_tsave = pl.T + 1;
    f.k0 = k0;
    f.B = pl.B;
    f.b_first = bs.first;
    f.b_count = bs.count;
    f.tiles = uint32_t(pl.dim >> kMomTileBits);
    f.rec_dstride = rec_dstride;
    f.out_dstride = out_dstride;
    const int H = pl.N - kMomTileBits;
    hipLaunchKernelGGL(k_moments_finish, dim3(unsigned(kMomEntries + H + kMomTileBits * H + H * (H - 1) / 2), unsigned(bs.count * nk), unsigned(n_dir)),
                       dim3(64), 0, c.stream, f);
}

// S, B_q, B_qr of the states of save points k0 .. k0 + nk - 1 (kstride amplitudes apart; `psi` is the one at k0, trajectory 0),
// trajectories of `bs`.  Up to 12 qubits one launch covers every state; beyond, the tile records of one save point at a time go
// through the workspace (plan.hpp: off_moments holds [B][79][tiles] doubles) and a second launch turns them into the rows.
int launch_moments_expect(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.moments_out) return RYDIFF_OK;
    const uint32_t tiles = uint32_t(std::max<size_t>(pl.dim >> kMomTileBits, 1));
    const int kmax = tiles > 1u ? 1 : std::max(1, 65535 / bs.count);  // grid.y; the workspace region holds one save point
    for (int k = 0; k < nk; k += kmax) {
        const int n = std::min(kmax, nk - k);
        MomentsTileArgs a{};
        a.psi = psi + size_t(k) * kstride;
        a.kstride = kstride;
        a.out = c.moments_out;
        a.rec = tiles > 1u ? reinterpret_cast<double*>(c.ws + pl.off_moments) : nullptr;
        a.N = pl.N;
        a.n_tsave = pl.T + 1;
        a.k0 = k0 + k;
        a.B = pl.B;
        a.b_first = bs.first;
        a.b_count = bs.count;
        a.dim = uint32_t(pl.dim);
        a.tiles = tiles;
        hipLaunchKernelGGL(k_moments_tile, dim3(tiles, unsigned(bs.count * n)), dim3(256), 0, c.stream, a);
        LAUNCH_CHECK();
        if (tiles > 1u) launch_moments_finish(c, a.rec, c.moments_out, k0 + k, n, bs, 1, 0, 0);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

// The tangents of S, B_q, B_qr in every direction at save point k: vec = [1 + n_dir][B][dim] with the state first; `out`: the first
// Moments row of direction 0 in dexpect_out, dstride doubles between directions.  One launch over all directions (grid.z); past 12
// qubits their tile records go to the tangent sweep's own region (c.moments_drec: [n_dir][B][79][tiles]) and a second launch turns
// them into the rows.  Every entry is written.
int launch_moments_tangent(const ForwardCtx& c, const double2* vec, int n_dir, int k, double* out, size_t dstride) {
    const Plan& pl = c.rt.pl;
    if (!out) return RYDIFF_OK;
    const uint32_t tiles = uint32_t(std::max<size_t>(pl.dim >> kMomTileBits, 1));
    if (tiles > 1u && !c.moments_drec) return fail(RYDIFF_EINVAL, "internal: no workspace region for the moment tangents' tile records");
    const BatchSlice bs{0, pl.B, false};
    MomentsTangentArgs a{};
    a.t.psi = vec;
    a.t.kstride = 0;
    a.t.out = out;
    a.t.rec = tiles > 1u ? c.moments_drec : nullptr;
    a.t.N = pl.N;
    a.t.n_tsave = pl.T + 1;
    a.t.k0 = k;
    a.t.B = pl.B;
    a.t.b_first = 0;
    a.t.b_count = pl.B;
    a.t.dim = uint32_t(pl.dim);
    a.t.tiles = tiles;
    a.vstride = size_t(pl.B) * pl.dim;
    a.out_dstride = dstride;
    a.rec_dstride = tiles > 1u ? size_t(pl.B) * kMomEntries * tiles : 0;
    hipLaunchKernelGGL(k_moments_tangent, dim3(tiles, unsigned(pl.B), unsigned(n_dir)), dim3(256), 0, c.stream, a);
    LAUNCH_CHECK();
    if (tiles > 1u) launch_moments_finish(c, a.t.rec, out, k, 1, bs, n_dir, a.rec_dstride, dstride);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// out[kk] = base[kk] + 2 q_k psi_{k0 + kk},  kk < nk; base: [nk][B][dim] or nullptr, may be `out` (the state at save point k as
// launch_pauli_apply takes it: psi / entry / kmul)
void launch_moments_apply(const PauliInject& pi, const double2* psi, const int32_t* entry, int kmul, int k0, int nk, const double2* base,
                          double2* out) {
    const Plan& pl = pi.rt->pl;
    MomentsApplyArgs a{};
    a.psi = psi;
    a.entry = entry;
    a.kmul = kmul;
    a.base = base;
    a.out = out;
    a.gexp = pi.moments_gexp;
    a.N = pl.N;
    a.n_tsave = pl.T + 1;
    a.k0 = k0;
    a.B = pl.B;
    a.dim = uint32_t(pl.dim);
    hipLaunchKernelGGL(k_moments_apply, dim3(unsigned(std::max<size_t>(pl.dim >> kMomTileBits, 1)), unsigned(pl.B), unsigned(nk)), dim3(256), 0,
                       pi.stream, a);
}

}  // namespace
