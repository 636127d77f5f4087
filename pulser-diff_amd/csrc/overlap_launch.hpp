// overlap_launch.hpp — state-overlap observables (overlap_kernels.hpp): the evaluation launches of the forward sweeps, and the
// observable cotangent (Pauli part, then overlap part, then the reduced-density-matrix part, then the density-matrix rows, in one workspace buffer) the adjoint sweeps inject at a save point.
#pragma once

namespace {

template <int NO>
void launch_overlap_expect_n(const OverlapExpectArgs& a, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((k_overlap_expect<NO>), grid, dim3(256), 0, stream, a);
}

// Re / Im <phi_o|psi> for every target on the states of save points k0 .. k0 + nk - 1 (kstride amplitudes apart; `psi` is the one
// at k0, trajectory 0), trajectories of `bs`
int launch_overlap_expect(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.overlap_out) return RYDIFF_OK;
    const unsigned red_blocks = unsigned(std::min<size_t>((pl.dim + 255) / 256, 1024));
    const int kmax = std::max(1, 65535 / bs.count);  // grid.y
    for (int k = 0; k < nk; k += kmax) {
        OverlapExpectArgs a{};
        a.psi = psi + size_t(k) * kstride;
        a.kstride = kstride;
        a.phi = static_cast<const double2*>(c.p->overlap_targets);
        a.out = c.overlap_out;
        a.n_ov = pl.n_ov;
        a.ov_batch = pl.ov_batch;
        a.n_tsave = pl.T + 1;
        a.k0 = k0 + k;
        a.B = pl.B;
        a.b_first = bs.first;
        a.b_count = bs.count;
        a.dim = uint32_t(pl.dim);
        const dim3 grid(red_blocks, unsigned(bs.count * std::min(kmax, nk - k)));
        if (pl.n_ov <= 1) launch_overlap_expect_n<1>(a, grid, c.stream);
        else if (pl.n_ov <= 2) launch_overlap_expect_n<2>(a, grid, c.stream);
        else if (pl.n_ov <= 4) launch_overlap_expect_n<4>(a, grid, c.stream);
        else if (pl.n_ov <= 8) launch_overlap_expect_n<8>(a, grid, c.stream);
        else launch_overlap_expect_n<RYDIFF_MAX_OVERLAPS>(a, grid, c.stream);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

// every native observable that is evaluated by a launch of its own (Pauli strings, overlaps, reduced density matrices, density-matrix rows) on the states of k0 .. k0 + nk - 1,
// and the measurement shots of the sampled save points among them
int launch_observables_expect(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    if (const int rc = launch_pauli_expect(c, psi, kstride, k0, nk, bs)) return rc;
    if (const int rc = launch_overlap_expect(c, psi, kstride, k0, nk, bs)) return rc;
    if (const int rc = launch_rdm_expect(c, psi, kstride, k0, nk, bs)) return rc;
    if (const int rc = launch_moments_expect(c, psi, kstride, k0, nk, bs)) return rc;
    if (const int rc = launch_energy_expect(c, psi, kstride, k0, nk, bs)) return rc;
    if (const int rc = launch_dm_expect(c, psi, kstride, k0, nk, bs)) return rc;
    return c.rt.pl.dm_shots ? launch_dm_shots(c, psi, kstride, k0, nk, bs) : launch_shots(c, psi, kstride, k0, nk, bs);
}

// out[kk] = grad_states[k0 + kk] + 2 sum_o g_o O_o psi_{k0 + kk} + sum_o (gRe + i gIm)_o phi_o + sum_o ((G + G^dagger)_{A_o} (x) 1) psi_{k0 + kk},
// kk < nk  (the state at save point k as launch_pauli_apply takes it: psi / entry / kmul)
void launch_observable_cotangent(const PauliInject& pi, const double2* psi, const int32_t* entry, int kmul, int k0, int nk, double2* out) {
    const Plan& pl = pi.rt->pl;
    const size_t sv = size_t(pl.B) * pl.dim;
    const double2* base = pi.gstate ? pi.gstate + size_t(k0) * sv : nullptr;
    if (pi.gexp) {
        launch_pauli_apply(pi, psi, entry, kmul, k0, nk, out);
        base = out;
    }
    if (pi.ov_gexp) {
        OverlapApplyArgs a{};
        a.base = base;
        a.out = out;
        a.phi = pi.ov_targets;
        a.gexp = pi.ov_gexp;
        a.n_ov = pl.n_ov;
        a.ov_batch = pl.ov_batch;
        a.n_tsave = pl.T + 1;
        a.k0 = k0;
        a.B = pl.B;
        a.dim = uint32_t(pl.dim);
        hipLaunchKernelGGL(k_overlap_apply, dim3(unsigned((pl.dim + 255) / 256), unsigned(pl.B), unsigned(nk)), dim3(256), 0, pi.stream, a);
        base = out;
    }
    if (pi.rdm_gexp) {
        launch_rdm_apply(pi, psi, entry, kmul, k0, nk, base, out);
        base = out;
    }
    if (pi.moments_gexp) {
        launch_moments_apply(pi, psi, entry, kmul, k0, nk, base, out);
        base = out;
    }
    if (pi.energy_gexp) {  // (a failed launch is kept for rydiff_backward to report: PauliInject::rc)
        if (const int rc = launch_energy_apply(pi, psi, entry, kmul, k0, nk, base, out)) pi.rc = rc;
        base = out;
    }
    if (pi.dm_gexp) launch_dm_apply(pi, psi, entry, kmul, k0, nk, base, out);
}

// launch-per-factor adjoint sweeps: the cotangent injected at save point k, written into the one reused workspace buffer right
// before the launch that reads it (stream order keeps the previous reader ahead of this write)
const double2* observable_cotangent(const PauliInject& pi, int k) {
    launch_observable_cotangent(pi, (pi.gexp || pi.rdm_gexp || pi.moments_gexp || pi.energy_gexp || (pi.dm_gexp && pi.rt->pl.dm_purity)) ? pi.state_at(k) : nullptr, nullptr, 0, k, 1, pi.buf);
    return pi.buf;
}

}  // namespace
