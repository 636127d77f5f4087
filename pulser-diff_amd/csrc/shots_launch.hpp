// shots_launch.hpp — measurement shots (shots_kernels.hpp): the launches behind launch_observables_expect (overlap_launch.hpp).
#pragma once

namespace {

// the shots of every SAMPLED save point among k0 .. k0 + nk - 1 (states kstride amplitudes apart; `psi` is the one at k0,
// trajectory 0), trajectories of `bs`: pass A, the scan of its chunk sums, pass B — the scratch is reused in stream order
int launch_shots(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.shots_out) return RYDIFF_OK;
    const uint32_t nch = uint32_t(pl.shot_chunks());
    double* sums = reinterpret_cast<double*>(c.ws + pl.off_shot_sums);
    double* prefix = reinterpret_cast<double*>(c.ws + pl.off_shot_prefix);
    for (size_t si = 0; si < pl.shot_times.size(); ++si) {
        const int k = pl.shot_times[si];
        if (k < k0 || k >= k0 + nk) continue;
        const double2* state = psi + size_t(k - k0) * kstride;
        const ShotSumArgs sa{state, sums, uint32_t(pl.dim), nch, bs.first};
        hipLaunchKernelGGL(k_shot_chunk_sums, dim3(nch, unsigned(bs.count)), dim3(256), 0, c.stream, sa);
        LAUNCH_CHECK();
        const ShotScanArgs sc{sums, prefix, nch, bs.first};
        hipLaunchKernelGGL(k_shot_scan, dim3(unsigned(bs.count)), dim3(256), 0, c.stream, sc);
        LAUNCH_CHECK();
        const size_t at = si * size_t(pl.B) * size_t(pl.n_shots);
        const ShotResolveArgs ra{state, sums, prefix, c.shot_u + at, c.shots_out + at, uint32_t(pl.dim), nch, pl.n_shots, bs.first};
        hipLaunchKernelGGL(k_shot_resolve, dim3(unsigned(pl.n_shots), unsigned(bs.count)), dim3(64), 0, c.stream, ra);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

}  // namespace
