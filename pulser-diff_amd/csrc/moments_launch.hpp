// moments_launch.hpp — occupation correlations (moments_kernels.hpp): the evaluation launches of the forward sweeps and the moments
// part of the observable cotangent (overlap_launch.hpp: launch_observable_cotangent).
#pragma once

namespace {

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
        if (tiles == 1u) continue;
        MomentsFinishArgs f{};
        f.rec = a.rec;
        f.out = c.moments_out;
        f.N = pl.N;
        f.n_tsave = pl.T + 1;
        f.k0 = k0 + k;
        f.B = pl.B;
        f.b_first = bs.first;
        f.b_count = bs.count;
        f.tiles = tiles;
        const int H = pl.N - kMomTileBits;
        hipLaunchKernelGGL(k_moments_finish, dim3(unsigned(kMomEntries + H + kMomTileBits * H + H * (H - 1) / 2), unsigned(bs.count * n)),
                           dim3(64), 0, c.stream, f);
        LAUNCH_CHECK();
    }
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
