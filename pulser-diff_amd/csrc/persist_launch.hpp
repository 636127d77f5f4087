// persist_launch.hpp — one-launch sweeps of small registers (persist_kernels.hpp, lane_kernels.hpp): kernel choice, factor table,
// forward and adjoint launches.
#pragma once

namespace {

// ---- persistent small-N forward (k_persist) ------------------------------------------------------------------------
bool persist_enabled(const Runtime& rt) { return rt.variant != 1 && rt.pl.N <= kTileBits && !rt.pl.shard_bits && !rt.pl.xy_mode; }

// every amplitude and every detuning group is ONE qubit and there are more than two of either (stochastic-noise runs, several local
// channels): the per-bit form of the forward sweep (k_persist<..., PERBIT>) instead of the generic group loops
bool per_bit_terms(const PersistArgs& pa) {
    auto single = [](uint32_t m) { return m != 0 && (m & (m - 1)) == 0; };
    if (pa.pair.n || pa.cond || (pa.ga <= 2 && pa.gd <= 2)) return false;
    uint32_t seen = 0;
    for (int g = 0; g < pa.ga; ++g) {
        if (!single(pa.amask[g]) || (seen & pa.amask[g])) return false;
        seen |= pa.amask[g];
    }
    seen = 0;
    for (int g = 0; g < pa.gd; ++g) {
        if (!single(pa.dmask[g]) || (seen & pa.dmask[g]) || pa.dcnt[g] != 1) return false;
        seen |= pa.dmask[g];
    }
    return true;
}

// one global drive, at most one detuning group, no pair terms, no conditioned flips: the loop-free instantiations
template <int LT, class Args>
bool global_drive_only(const Args& pa) {
    return pa.ga == 1 && pa.gd <= 1 && pa.amask[0] == (1u << LT) - 1u && pa.pair.n == 0 && pa.cond == 0;
}

// f(std::integral_constant<int, LT>{}) with LT = N clamped to [1, MAX]: the register size as a template argument
template <int MAX, class F>
int with_tile_bits(int N, F&& f) {
    if constexpr (MAX > 1) {
        if (N < MAX) return with_tile_bits<MAX - 1>(N, f);
    }
    return f(std::integral_constant<int, MAX>{});
}

// KERNEL<..., FAST, GLMAX> by the problem's groups: loop-free / up to two amplitude and detuning groups / general
// (uses LT, pa, B and stream of the calling function)
#define RYDIFF_LAUNCH_BY_GROUPS(BLOCK, KERNEL, ...)                                                                                \
    do {                                                                                                                           \
        if (global_drive_only<LT>(pa)) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, true>), dim3(B), BLOCK, 0, stream, pa);             \
        else if (pa.ga <= 2 && pa.gd <= 2) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, false, 2>), dim3(B), BLOCK, 0, stream, pa);     \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__, false>), dim3(B), BLOCK, 0, stream, pa);                                      \
        LAUNCH_CHECK();                                                                                                            \
    } while (0)

template <int LT, bool CPLX>
int launch_persist_t(const PersistArgs& pa, int B, hipStream_t stream) {
    constexpr int LGT = LT < 10 ? LT : 10;
    const dim3 block(LGT < 6 ? 64 : (1 << LGT));
    if (per_bit_terms(pa) && pa.NC <= 3 * LT)
        hipLaunchKernelGGL((k_persist<LT, LGT, CPLX, false, false, kPersistGroups, true>), dim3(B), block, 0, stream, pa);
    else if (global_drive_only<LT>(pa))
        hipLaunchKernelGGL((k_persist<LT, LGT, CPLX, true, true>), dim3(B), block, 0, stream, pa);
    else if (pa.ga <= 2 && pa.gd <= 2)
        hipLaunchKernelGGL((k_persist<LT, LGT, CPLX, true, false, 2>), dim3(B), block, 0, stream, pa);
    else if (pa.ga <= kPersistGroups && pa.gd <= kPersistGroups)
        hipLaunchKernelGGL((k_persist<LT, LGT, CPLX, true>), dim3(B), block, 0, stream, pa);
    else
        hipLaunchKernelGGL((k_persist<LT, LGT, CPLX, false>), dim3(B), block, 0, stream, pa);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

template <int LT, bool CPLX>
int launch_lanes_fwd_t(const PersistArgs& pa, int B, hipStream_t stream) {
    RYDIFF_LAUNCH_BY_GROUPS(dim3(64), k_lanes_fwd, LT, CPLX);
    return RYDIFF_OK;
}

// one amplitude per lane of one wave (lane_kernels.hpp); variant 8 keeps the LDS-tile kernels for A/B tests
bool lanes_enabled(const Runtime& rt) {
    const Plan& pl = rt.pl;
    return rt.variant != 8 && pl.N <= kLaneMaxQubits && pl.n_pair <= kLanePairMax && pl.ga.n <= kPersistGroups && pl.gd.n <= kPersistGroups;
}

template <bool CPLX>
int launch_persist(const Runtime& rt, const PersistArgs& pa, hipStream_t stream) {
    const int N = rt.pl.N, B = rt.pl.B;
    if (lanes_enabled(rt) && pa.n_factors > 0)  // (up to 4 groups: also ahead of the per-bit sweep, 0.83 vs 0.90 us per factor at 4 qubits)
        return with_tile_bits<kLaneMaxQubits>(N, [&](auto lt) { return launch_lanes_fwd_t<decltype(lt)::value, CPLX>(pa, B, stream); });
    return with_tile_bits<kTileBits>(N, [&](auto lt) { return launch_persist_t<decltype(lt)::value, CPLX>(pa, B, stream); });
}

template <int LT, bool CPLX>
int launch_persist_bwd_t(const PersistBwdArgs& pa, int B, hipStream_t stream) {
    constexpr int LGT = LT < 10 ? LT : 9;  // 1024+ amplitudes: 512 threads, so the accumulators stay in registers
    RYDIFF_LAUNCH_BY_GROUPS(dim3(LGT < 6 ? 64 : (1 << LGT)), k_persist_bwd, LT, LGT, CPLX);
    return RYDIFF_OK;
}

template <int LT, bool CPLX>
int launch_lanes_bwd_t(const PersistBwdArgs& pa, int B, hipStream_t stream) {
    if (pa.tape_full)  // every factor input is on the tape: one descending walk, nothing recomputed
        RYDIFF_LAUNCH_BY_GROUPS(dim3(64), k_lanes_bwd_tape, LT, CPLX);
    else
        RYDIFF_LAUNCH_BY_GROUPS(dim3(64), k_lanes_bwd, LT, CPLX);
    return RYDIFF_OK;
}

template <bool CPLX>
int launch_persist_bwd(const Runtime& rt, const PersistBwdArgs& pa, hipStream_t stream) {
    const int N = rt.pl.N, B = rt.pl.B;
    if (lanes_enabled(rt) && pa.n_factors > 0)
        return with_tile_bits<kLaneMaxQubits>(N, [&](auto lt) { return launch_lanes_bwd_t<decltype(lt)::value, CPLX>(pa, B, stream); });
    return with_tile_bits<kPersistBwdMaxQubits>(N, [&](auto lt) { return launch_persist_bwd_t<decltype(lt)::value, CPLX>(pa, B, stream); });
}

// Factor table of the one-launch sweeps: every factor of the run, in order, with the save point its output belongs to (0 = none).
// Built ON THE DEVICE (k_build_ptable) from four small per-interval / per-exponential arrays that travel as kernel arguments.
int build_persist_table_device(const Runtime& rt, char* ws, hipStream_t stream, int* n_factors) {
    const Plan& pl = rt.pl;
    const size_t E = pl.stages.size();
    if (rt.poly.degree > kMaxDegreeDev) return fail(RYDIFF_ENOTIMPL, "polynomial degree beyond the on-device factor table builder");
    if (size_t(rt.total_factors) * sizeof(PersistFactor) > pl.ptable_bytes) return fail(RYDIFF_EWORKSPACE, "internal: factor table does not fit");
    std::vector<int32_t> begin(pl.step_begin.begin(), pl.step_begin.end()), first(pl.T + 1, 0), nsub(E);
    std::vector<double> tau(E);
    for (size_t e = 0; e < E; ++e) {
        nsub[e] = pl.stages[e].nsub;
        tau[e] = pl.stages[e].tau / pl.stages[e].nsub;
    }
    for (int k = 0; k < pl.T; ++k) {
        first[k + 1] = int32_t(first[k] + step_factor_count(rt, k));
    }
    int rc = upload_words(stream, ws + pl.off_pm_begin, begin.data(), begin.size() * sizeof(int32_t));
    if (!rc) rc = upload_words(stream, ws + pl.off_pm_first, first.data(), first.size() * sizeof(int32_t));
    if (!rc) rc = upload_words(stream, ws + pl.off_pm_tau, tau.data(), tau.size() * sizeof(double));
    if (!rc) rc = upload_words(stream, ws + pl.off_pm_nsub, nsub.data(), nsub.size() * sizeof(int32_t));
    if (rc) return rc;
    PTableArgs ta{};
    ta.out = reinterpret_cast<PersistFactor*>(ws + pl.off_ptable);
    ta.tau_sub = reinterpret_cast<const double*>(ws + pl.off_pm_tau);
    ta.nsub = reinterpret_cast<const int32_t*>(ws + pl.off_pm_nsub);
    ta.step_begin = reinterpret_cast<const int32_t*>(ws + pl.off_pm_begin);
    ta.step_first = reinterpret_cast<const int32_t*>(ws + pl.off_pm_first);
    ta.T = pl.T;
    ta.degree = rt.poly.degree;
    ta.sigma = rt.sigma;
    ta.rho_design = rt.rho_design;
    ta.p0r = rt.poly.p0.real();
    ta.p0i = rt.poly.p0.imag();
    for (int f = 0; f < rt.poly.degree; ++f) {
        ta.roots[2 * f] = rt.poly.roots[f].real();
        ta.roots[2 * f + 1] = rt.poly.roots[f].imag();
    }
    hipLaunchKernelGGL(k_build_ptable, dim3(unsigned(pl.T + 63) / 64), dim3(64), 0, stream, ta);
    LAUNCH_CHECK();
    *n_factors = int(rt.total_factors);
    return RYDIFF_OK;
}

// the fields PersistArgs and PersistBwdArgs have in common
template <class Args>
int fill_persist(Args& pa, const Runtime& rt, char* ws, hipStream_t stream) {
    const Plan& pl = rt.pl;
    int rc = build_persist_table_device(rt, ws, stream, &pa.n_factors);
    if (rc) return rc;
    pa.factors = reinterpret_cast<const PersistFactor*>(ws + pl.off_ptable);
    pa.udiag = reinterpret_cast<const double*>(ws + pl.off_udiag);
    pa.coef = rt.coef(ws, 0);
    pa.coef_bstride = rt.coef_bstride();
    pa.NC = pl.NC;
    pa.n_tsave = pl.T + 1;
    pa.B = pl.B;
    pa.dim = uint32_t(pl.dim);
    pa.ga = pl.ga.n;
    pa.gd = pl.gd.n;
    pa.pair = rt.parg;
    for (int g = 0; g < pl.ga.n; ++g) pa.amask[g] = pl.ga.amp_index_mask[g];
    pa.cond = pl.ga.flagged;
    fill_detuning(pa.dmask, pa.dcnt, pl);
    return RYDIFF_OK;
}

// whole trajectory in one launch, from a factor table built on the device
int forward_persist(const ForwardCtx& c) {
    const Runtime& rt = c.rt;
    PersistArgs pa{};
    int rc = fill_persist(pa, rt, c.ws, c.stream);
    if (rc) return rc;
    pa.psi0 = c.psi0;
    pa.states = c.full_tape() ? c.copy_out : c.tape;
    pa.tape_all = c.full_tape() ? c.tape : nullptr;
    pa.obs = c.want_exp ? c.obs : nullptr;
    pa.expect = c.expect_out;
    pa.n_obs = c.want_exp ? rt.pl.n_obs : 0;
    const Plan& pl = rt.pl;
    if ((c.pauli_out || c.overlap_out || c.rdm_out || c.moments_out || c.energy_out || c.dm_out || c.shots_out) && !pa.states) {  // the caller keeps no trajectory: the Pauli / overlap observables and the shots read one in the workspace
        pa.states = reinterpret_cast<double2*>(c.ws + pl.off_pauli_traj);
        HIP_TRY(hipMemcpyAsync(pa.states, c.psi0, pl.state_bytes, hipMemcpyDeviceToDevice, c.stream));
    }
    rc = (rt.flags & 1) ? launch_persist<true>(rt, pa, c.stream) : launch_persist<false>(rt, pa, c.stream);
    if (rc) return rc;
    return launch_observables_expect(c, pa.states, c.sv, 0, pl.T + 1, BatchSlice{0, pl.B, false});  // one launch over the stored trajectory
}

// The whole reverse sweep in one launch (k_persist_bwd / k_lanes_bwd); the cotangent w.r.t. psi0 ends up in c.lam[0].
// (4096 amplitudes would need 8 per thread plus the accumulators: past the register file, so N = 12 keeps the launch-per-factor sweep;
// with the full tape both one-launch adjoints — one wave up to 6 qubits, one workgroup up to 11 — walk the tape)
bool persist_bwd_enabled(const Runtime& rt) {
    const Plan& pl = rt.pl;
    const bool lanes_tape = pl.tape_mode == 2 && lanes_enabled(rt);
    return persist_enabled(rt) && pl.N <= kPersistBwdMaxQubits && pl.ga.n <= kPersistGroups && pl.gd.n <= kPersistGroups &&
           (rt.max_step_factors <= kStageChunk || lanes_tape);
}

int backward_persist(const BackwardCtx& c) {
    const Runtime& rt = c.rt;
    const Plan& pl = rt.pl;
    if (!c.full_tape() && rt.max_step_factors - 1 > pl.chain_slots) return fail(RYDIFF_EWORKSPACE, "internal: chain buffers too small");
    PersistBwdArgs pa{};
    int rc = fill_persist(pa, rt, c.ws, c.stream);
    if (rc) return rc;
    if (c.inj.gexp) {  // stays on the device: the sweep skips save points without an expectation cotangent
        int32_t* dflags = reinterpret_cast<int32_t*>(c.ws + pl.off_meta2);
        hipLaunchKernelGGL(k_cotangent_flags, dim3(unsigned(pl.T + 1 + 255) / 256), dim3(256), 0, c.stream, c.inj.gexp, pl.n_obs, pl.T + 1,
                           pl.B, dflags);
        LAUNCH_CHECK();
        pa.gflags = dflags;
    }
    pa.tape = c.tape;
    pa.tape_full = c.full_tape() ? 1 : 0;
    pa.save_entry = reinterpret_cast<const int32_t*>(c.ws + pl.off_pm_first);
    pa.chainbuf = c.chainbuf;
    pa.gstate = c.inj.gstate;
    if (c.inj.pauli) {  // grad_states[k] + 2 sum_o g_o O_o psi_k + sum_o (gRe + i gIm)_o phi_o for every save point, one launch per kind
        launch_observable_cotangent(c.pauli, c.tape, c.full_tape() ? pa.save_entry : nullptr, 1, 0, pl.T + 1, c.pauli.buf);
        LAUNCH_CHECK();
        pa.gstate = c.pauli.buf;
    }
    pa.gexp = c.inj.gexp;
    pa.obs = c.inj.obs;
    pa.n_obs = c.inj.n_obs;
    pa.ge = c.ge;
    pa.ge_bstride = rt.ge_bstride();
    pa.ge_sstride = rt.ge_rec();
    pa.wtot = c.wtot;
    pa.mu_out = c.lam[0];
    pa.want_tau = c.want_tau ? 1 : 0;
    return (rt.flags & 1) ? launch_persist_bwd<true>(rt, pa, c.stream) : launch_persist_bwd<false>(rt, pa, c.stream);
}

#undef RYDIFF_LAUNCH_BY_GROUPS

}  // namespace
