// energy_launch.hpp — energy observables (energy_kernels.hpp): the coefficient records of the save points (prepare), the evaluation
// launches of the forward sweeps, the energy part of the observable cotangent (overlap_launch.hpp: launch_observable_cotangent) and
// the table gradients at the end of rydiff_backward.
#pragma once

namespace {

// One coefficient record per save point: k_expand_coeffs with a "stage" per save point that takes column k with weight 1 from tables
// of n_tsave samples.  Enqueued by prepare(); nothing waits.
int energy_prepare(const Runtime& rt, const RydProblem* p, char* ws, hipStream_t stream) {
    const Plan& pl = rt.pl;
    if (!pl.energy) return RYDIFF_OK;
    std::vector<StageDev> sd(pl.T + 1);
    for (int k = 0; k <= pl.T; ++k) sd[k] = {1.0, 0.0, k, 0};
    if (const int rc = upload_words(stream, ws + pl.off_energy_meta, sd.data(), sd.size() * sizeof(StageDev))) return rc;
    if (pl.NC == 0) return RYDIFF_OK;
    return launch_expand_at(pl, reinterpret_cast<const StageDev*>(ws + pl.off_energy_meta), pl.T + 1, pl.T + 1, static_cast<const double2*>(p->energy_amp),
                            p->energy_det, reinterpret_cast<double*>(ws + pl.off_energy_coef), stream);
}

// what every launch of the block shares
void fill_energy(EnergyArgs& a, const Runtime& rt, char* ws) {
    const Plan& pl = rt.pl;
    a.udiag = reinterpret_cast<const double*>(ws + pl.off_udiag);
    a.coef = reinterpret_cast<const double*>(ws + pl.off_energy_coef);
    a.coef_bstride = pl.Bc > 1 ? long(pl.T + 1) * pl.NC : 0;
    a.NC = pl.NC;
    a.n_tsave = pl.T + 1;
    a.B = pl.B;
    a.dim = uint32_t(pl.dim);
    a.g = rt.garg;
    a.xy = rt.xarg;
    a.rows = pl.energy;
}

// Which version runs (RydProblem.energy_kernel; Plan::energy_tile_legal): forced, or the one that measured faster
// (profiles/energy_observables.txt, per save point, direct / LDS-tile): the FORWARD reduction 55 / 48 us at 20 qubits and 787 / 718 us
// at 24, but -0.4 (hidden behind the launches) / 26 us at 16, where 16 tiles leave most of the chip idle -> the tile version from 20
// qubits; the COTANGENT passes 14 / 66 us at 16, 88 / 97 us at 20, 1477 / 1641 us at 24 -> the direct version everywhere.
bool energy_use_tile(const Plan& pl, bool forward) {
    if (pl.energy_kernel) return pl.energy_kernel == 2;
    return forward && pl.energy_tile_legal() && pl.N >= 20;
}

template <int MODE>
int launch_energy_tile(const EnergyArgs& a, dim3 grid, hipStream_t stream) {
    if (const int rc = set_max_dynamic_lds_once<k_energy_tile<MODE>>(kEnergyTileLds)) return rc;
    hipLaunchKernelGGL(k_energy_tile<MODE>, grid, dim3(256), kEnergyTileLds, stream, a);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// E (and M2) of the states of save points k0 .. k0 + nk - 1 (kstride amplitudes apart; `psi` is the one at k0, trajectory 0),
// trajectories of `bs`.  Up to 12 qubits one launch covers every state; beyond, one save point at a time goes through the
// workspace region of the partial sums (plan.hpp: off_energy_part).
int launch_energy_expect(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.energy_out) return RYDIFF_OK;
    const bool tile = energy_use_tile(pl, true);
    const unsigned blocks = tile ? unsigned(pl.dim >> kEnergyTileBits) : unsigned(pl.energy_blocks());
    const int kmax = pl.N <= 12 ? std::min(pl.T + 1, 65535) : 1;  // grid.z; what the region holds
    for (int k = 0; k < nk; k += kmax) {
        const int n = std::min(kmax, nk - k);
        EnergyArgs a{};
        fill_energy(a, c.rt, c.ws);
        a.psi = psi + size_t(k) * kstride;
        a.kstride = kstride;
        a.k0 = k0 + k;
        a.b_first = bs.first;
        a.iters = int(std::max<size_t>(pl.dim / (size_t(256) * blocks), 1));
        a.part = reinterpret_cast<double*>(c.ws + pl.off_energy_part);
        const dim3 grid(blocks, unsigned(bs.count), unsigned(n));
        if (tile) {
            if (const int rc = launch_energy_tile<0>(a, grid, c.stream)) return rc;
        } else if (pl.xy_mode) hipLaunchKernelGGL(k_energy_expect<true>, grid, dim3(256), 0, c.stream, a);
        else hipLaunchKernelGGL(k_energy_expect<false>, grid, dim3(256), 0, c.stream, a);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_energy_finish, dim3(unsigned(bs.count), unsigned(n)), dim3(64), 0, c.stream, a.part, c.energy_out, int(blocks), pl.energy,
                           pl.T + 1, k0 + k, pl.B, bs.first);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

// out[kk] = base[kk] + 2 H_k (g_E psi + g_M H_k psi),  k = k0 + kk, kk < nk; base: [nk][B][dim] or nullptr, may be `out` (the state
// at save point k as launch_pauli_apply takes it: psi / entry / kmul).  On the way: the explicit coefficient gradients of H_k into
// the block's records, wtot and the exchange replicas.
int launch_energy_apply(const PauliInject& pi, const double2* psi, const int32_t* entry, int kmul, int k0, int nk, const double2* base,
                         double2* out) {
    const Runtime& rt = *pi.rt;
    const Plan& pl = rt.pl;
    const int kmax = std::min(pl.N <= 12 ? pl.T + 1 : 1, 65535);  // grid.z; the scratch states z the workspace holds
    const size_t sv = size_t(pl.B) * pl.dim;
    for (int k = 0; k < nk; k += kmax) {
        const int n = std::min(kmax, nk - k);
        EnergyArgs a{};
        fill_energy(a, rt, pi.ws);
        a.psi = entry ? psi : psi + size_t(k0 + k) * kmul * sv;
        a.entry = entry;
        a.kstride = size_t(kmul) * sv;
        a.k0 = k0 + k;
        a.gexp = pi.energy_gexp;
        a.z = reinterpret_cast<double2*>(pi.ws + pl.off_energy_z);
        a.base = base ? base + size_t(k) * sv : nullptr;
        a.out = out + size_t(k) * sv;
        a.ge = reinterpret_cast<double*>(pi.ws + pl.off_energy_ge);
        a.ge_bstride = pl.Bc > 1 ? long(pl.T + 1) * kEnergyReplicas * pl.NC : 0;
        a.wtot = pi.wtot;
        a.xy_ge = rt.xy_ge;
        const dim3 grid(unsigned((pl.dim + 255) / 256), unsigned(pl.B), unsigned(n));
        if (energy_use_tile(pl, false)) {
            const dim3 tgrid(unsigned(pl.dim >> kEnergyTileBits), unsigned(pl.B), unsigned(n));
            if (const int rc = launch_energy_tile<1>(a, tgrid, pi.stream)) return rc;
            if (const int rc = launch_energy_tile<2>(a, tgrid, pi.stream)) return rc;
        } else if (pl.xy_mode) {
            hipLaunchKernelGGL(k_energy_bwd1<true>, grid, dim3(256), 0, pi.stream, a);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(k_energy_bwd2<true>, grid, dim3(256), 0, pi.stream, a);
            LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(k_energy_bwd1<false>, grid, dim3(256), 0, pi.stream, a);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(k_energy_bwd2<false>, grid, dim3(256), 0, pi.stream, a);
            LAUNCH_CHECK();
        }
    }
    return RYDIFF_OK;
}

// rydiff_backward, before the sweep: the block's gradient records start at zero
int energy_clear_gradients(const Runtime& rt, char* ws, hipStream_t stream) {
    const Plan& pl = rt.pl;
    if (!pl.energy) return RYDIFF_OK;
    HIP_TRY(hipMemsetAsync(ws + pl.off_energy_ge, 0, size_t(pl.Bc) * (pl.T + 1) * kEnergyReplicas * std::max(pl.NC, 1) * sizeof(double), stream));
    return RYDIFF_OK;
}

// rydiff_backward, after the sweep: the records -> g_energy_amp / g_energy_det (overwritten; zero where no cotangent came in)
int energy_scatter(const Runtime& rt, const RydProblem* p, char* ws, hipStream_t stream) {
    const Plan& pl = rt.pl;
    if (!pl.energy) return RYDIFF_OK;  // (the fields are ignored)
    double2* g_amp = pl.Ka ? static_cast<double2*>(p->g_energy_amp) : nullptr;
    double* g_det = pl.Kd ? p->g_energy_det : nullptr;
    if (!g_amp && !g_det) return RYDIFF_OK;
    EnergyScatterArgs sa{};
    sa.ge = reinterpret_cast<const double*>(ws + pl.off_energy_ge);
    sa.g_amp = g_amp;
    sa.g_det = g_det;
    sa.n_tsave = pl.T + 1;
    sa.Ka = pl.Ka;
    sa.Kd = pl.Kd;
    sa.NC = pl.NC;
    sa.ga = pl.ga.n;
    sa.gd = pl.gd.n;
    for (int g = 0; g < pl.ga.n; ++g) sa.amem[g] = pl.ga.members[g];
    for (int g = 0; g < pl.gd.n; ++g) sa.dmem[g] = pl.gd.members[g];
    hipLaunchKernelGGL(k_energy_scatter, dim3(unsigned(pl.T + 1 + 63) / 64, pl.Bc), dim3(64), 0, stream, sa);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

}  // namespace
