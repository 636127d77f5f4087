// tangent_launch.hpp — forward-mode (tangent) sweep (tangent_kernels.hpp): argument validation, the workspace regions behind the
// forward plan's, the tangent coefficient records / interaction diagonals, and the launches of one factor pass and of the
// observable tangents at one save point.
#pragma once

namespace {

// Everything rydiff_forward_tangent refuses, checked on the host before anything touches a device.
int tangent_validate(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags) {
    if (!p) return fail(RYDIFF_EINVAL, "null problem");
    if (n_dir < 1 || n_dir > RYDIFF_MAX_TANGENTS)
        return fail(RYDIFF_EINVAL, "n_dir must be in [1, " + std::to_string(RYDIFF_MAX_TANGENTS) + "], got " + std::to_string(n_dir));
    if (!info) return fail(RYDIFF_EINVAL, "the tangent sweep needs the plan of rydiff_plan(p, 0, 0, ...): null info");
    if (p->xy_mode < 0 || p->xy_mode > 2) return fail(RYDIFF_EINVAL, "xy_mode must be 0 (none), 1 (Hermitian exchange) or 2 (one-directional)");
    // the exchange runs only where the caller asks for it, like the pair terms below: a caller that does not know the flag keeps its refusal
    if (p->xy_mode != 0 && !(flags & RYDIFF_TANGENT_XY))
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: not implemented with the XY exchange (xy_mode != 0) unless RydTangent.flags has "
                                     "RYDIFF_TANGENT_XY");
    if (p->shard_bits > 0) return fail(RYDIFF_ENOTIMPL, "tangent sweep: not implemented for state-sharded runs (shard_bits > 0)");
    if (flags & ~(RYDIFF_TANGENT_PAIR_TERMS | RYDIFF_TANGENT_DENSITY_MATRIX | RYDIFF_TANGENT_RDMS | RYDIFF_TANGENT_MOMENTS | RYDIFF_TANGENT_XY))
        return fail(RYDIFF_EINVAL, "RydTangent.flags: unknown bits " + std::to_string(flags));
    if (p->xy_mode == 0 && (flags & RYDIFF_TANGENT_XY))  // (the flag asks for a term the problem does not have)
        return fail(RYDIFF_EINVAL, "RydTangent.flags: RYDIFF_TANGENT_XY (16) on a problem without the XY exchange (xy_mode = 0)");
    // the moments flag is valid only on a problem that has the block: callers written before it existed probe bit 8 as an unknown one on
    // problems without bit moments and keep their RYDIFF_EINVAL
    if ((flags & RYDIFF_TANGENT_MOMENTS) && p->bit_moments == 0)
        return fail(RYDIFF_EINVAL, "RydTangent.flags: RYDIFF_TANGENT_MOMENTS (8) asks for the Moments block of a problem that has none "
                                   "(bit_moments = 0)");
    // dense pair terms, density-matrix registers, reduced density matrices and bit moments run only where the caller asks for them (RydTangent.flags): a caller that does
    // not know of them keeps the refusals it was written against
    if (p->n_pair_terms > 0 && !(flags & RYDIFF_TANGENT_PAIR_TERMS))
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: not implemented with dense pair terms (n_pair_terms > 0) unless RydTangent.flags "
                                     "has RYDIFF_TANGENT_PAIR_TERMS");
    if (p->amp_conditioned_terms || p->det_ones_terms)
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: not implemented with conditioned flips / ones-counting terms (three-level registers)");
    if (p->energy_rows != 0)
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: energy observables are not implemented (energy_rows > 0): request them from rydiff_forward");
    if (p->n_shots > 0) return fail(RYDIFF_ENOTIMPL, "tangent sweep: measurement shots are not implemented (n_shots > 0): draw them in rydiff_forward");
    if (p->bit_moments != 0 && (!(flags & RYDIFF_TANGENT_MOMENTS) || p->dm_atoms != 0))  // (the ket block; a density-matrix register asks with dm_moments)
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: bit moments are not implemented (bit_moments != 0) unless RydTangent.flags has "
                                     "RYDIFF_TANGENT_MOMENTS (kets only, dm_atoms = 0): request them from rydiff_forward");
    if (p->n_rdms > 0 && !(flags & RYDIFF_TANGENT_RDMS))
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: reduced density matrices are not implemented (n_rdms > 0) unless RydTangent.flags "
                                     "has RYDIFF_TANGENT_RDMS");
    if (p->dm_atoms != 0 && !(flags & RYDIFF_TANGENT_DENSITY_MATRIX))
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: density-matrix registers are not implemented (dm_atoms > 0) unless RydTangent.flags "
                                     "has RYDIFF_TANGENT_DENSITY_MATRIX");
    if (p->dm_atoms != 0 && p->n_dm_rdms > 0)
        return fail(RYDIFF_ENOTIMPL, "tangent sweep: reduced density matrices of density-matrix registers are not implemented (n_dm_rdms > 0)");
    return RYDIFF_OK;
}

// What rydiff_forward_geometry refuses on top of that: the Gram matrix of vec(rho) and its tangents is not the mixed-state quantum
// Fisher information
int geometry_validate(const RydProblem* p) {
    if (p && p->dm_atoms != 0)
        return fail(RYDIFF_ENOTIMPL, "geometry sweep: density-matrix registers are not implemented (dm_atoms > 0): the Gram matrix of "
                                     "vec(rho) is not the mixed-state quantum Fisher information");
    return RYDIFF_OK;
}

// Workspace of the tangent sweep: the forward plan's regions (udiag, coefficient records, Pauli tables ...) and behind them
struct TangentLayout {
    size_t off_vec[2] = {0, 0};  // ping-pong: [1 + D][B][dim] amplitudes each
    size_t off_dcoef = 0;        // [D][Bc][E][NC] doubles
    size_t off_dudiag = 0;       // [D][dim] doubles
    size_t off_dxy = 0;          // XY exchange: [D][N(N-1)/2] doubles, the tangents of the couplings (padded directions zero)
    size_t off_dmoments = 0;     // bit moments past 12 qubits: the tile records of the moment tangents, [n_dir][B][79][dim >> 12] doubles
    size_t total = 0;
    long dcoef_dstride = 0;      // doubles
};

// k_factor_tangent is instantiated for 1, 2, 3, 4, 6 and 8 directions; 5 and 7 run the next one with a zero direction (zero tangent
// vector, zero records: it stays zero and nothing reads it)
int tangent_padded(int n_dir) { return n_dir == 5 ? 6 : (n_dir == 7 ? 8 : n_dir); }

TangentLayout tangent_layout(const Plan& pl, size_t base, int n_real) {
    const int n_dir = tangent_padded(n_real);
    TangentLayout t;
    size_t off = align_up(base);
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes);
        return o;
    };
    const size_t vecs = size_t(1 + n_dir) * pl.state_bytes;
    t.off_vec[0] = take(vecs);
    t.off_vec[1] = take(vecs);
    t.dcoef_dstride = long(pl.Bc) * long(pl.stages.size()) * pl.NC;
    t.off_dcoef = take(size_t(n_dir) * size_t(std::max<long>(t.dcoef_dstride, 1)) * sizeof(double));
    t.off_dudiag = take(size_t(n_dir) * pl.dim * sizeof(double));
    // (only the real directions' moments are evaluated; the values' records go through the plan's own region, off_moments)
    t.off_dmoments = take((pl.moments && pl.moment_tiles() > 1) ? size_t(n_real) * pl.B * kMomEntries * pl.moment_tiles() * sizeof(double) : 0);
    t.off_dxy = take(pl.xy_mode ? size_t(n_dir) * (pl.N * (pl.N - 1) / 2) * sizeof(double) : 0);
    t.total = off;
    return t;
}

// host-only planning of a tangent call: validation, the forward plan from `info`, the layout
int tangent_plan(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags, Runtime& rt, TangentLayout& lay) {
    int rc = tangent_validate(p, info, n_dir, flags);
    if (rc) return rc;
    RydProblem q = *p;
    q.kernel_variant = 0;  // ignored: one kernel family
    double lo, hi, dummy_scratch = 0.0;
    size_t need = 0;
    int need_tape = 0;
    rc = plan_runtime(&q, info, &dummy_scratch, sizeof(dummy_scratch), need_tape, false, nullptr, rt, lo, hi, need);  // (with info: host only)
    if (rc) return rc;
    lay = tangent_layout(rt.pl, need, n_dir);
    return RYDIFF_OK;
}

// tangent coefficient records (k_expand_coeffs on the tangent tables, same StageDev records) and tangent interaction diagonals
int tangent_tables(const Runtime& rt, const RydProblem* p, const RydTangent* tg, char* ws, const TangentLayout& lay, hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int Dp = tangent_padded(tg->n_dir);
    if (pl.NC > 0) {
        for (int d = 0; d < tg->n_dir; ++d) {
            const int rc = launch_expand(pl, ws, tg->d_amp ? static_cast<const double2*>(tg->d_amp) + size_t(d) * pl.Bc * pl.Ka * pl.n_samples : nullptr,
                                         tg->d_det ? tg->d_det + size_t(d) * pl.Bc * pl.Kd * pl.n_samples : nullptr,
                                         reinterpret_cast<double*>(ws + lay.off_dcoef) + size_t(d) * lay.dcoef_dstride, stream);
            if (rc) return rc;
        }
        if (Dp > tg->n_dir)  // padded directions: zero records
            HIP_TRY(hipMemsetAsync(reinterpret_cast<double*>(ws + lay.off_dcoef) + size_t(tg->n_dir) * lay.dcoef_dstride, 0,
                                   size_t(Dp - tg->n_dir) * lay.dcoef_dstride * sizeof(double), stream));
    }
    if (tg->d_u && pl.N > 1) {
        const int npairs = pl.N * (pl.N - 1) / 2;
        double* dud = reinterpret_cast<double*>(ws + lay.off_dudiag);
        for (int d = 0; d < tg->n_dir; ++d) {
            hipLaunchKernelGGL(k_build_udiag, dim3(unsigned((pl.dim + 255) / 256)), dim3(256), 0, stream, dud + size_t(d) * pl.dim,
                               tg->d_u + size_t(d) * npairs, pl.N, uint32_t(pl.dim));
            LAUNCH_CHECK();
        }
        if (Dp > tg->n_dir) HIP_TRY(hipMemsetAsync(dud + size_t(tg->n_dir) * pl.dim, 0, size_t(Dp - tg->n_dir) * pl.dim * sizeof(double), stream));
    }
    if (tg->d_xy && pl.xy_mode && pl.N > 1) {  // the caller's [n_dir][P] into the sweep's [Dp][P]: a padded direction reads zeros
        const size_t P = size_t(pl.N) * (pl.N - 1) / 2;
        double* dxy = reinterpret_cast<double*>(ws + lay.off_dxy);
        HIP_TRY(hipMemcpyAsync(dxy, tg->d_xy, size_t(tg->n_dir) * P * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (Dp > tg->n_dir) HIP_TRY(hipMemsetAsync(dxy + size_t(tg->n_dir) * P, 0, size_t(Dp - tg->n_dir) * P * sizeof(double), stream));
    }
    return RYDIFF_OK;
}

template <int D>
void launch_factor_tangent_n(const TangentFactorArgs& a, dim3 grid, hipStream_t stream) {
    if (a.xyt.xy.mode) hipLaunchKernelGGL((k_factor_tangent<D, false, true>), grid, dim3(256), 0, stream, a);
    else if (a.pair.n) hipLaunchKernelGGL((k_factor_tangent<D, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((k_factor_tangent<D, false>), grid, dim3(256), 0, stream, a);
}

// what every factor launch of one call shares
void fill_tangent_factor(TangentFactorArgs& a, const Runtime& rt, char* ws, const TangentLayout& lay, bool have_du, bool have_dxy) {
    const Plan& pl = rt.pl;
    a.vstride = size_t(pl.B) * pl.dim;
    a.udiag = reinterpret_cast<const double*>(ws + pl.off_udiag);
    a.dudiag = (have_du && pl.N > 1) ? reinterpret_cast<const double*>(ws + lay.off_dudiag) : nullptr;
    a.coef_bstride = rt.coef_bstride();
    a.dcoef_dstride = lay.dcoef_dstride;
    a.dim = uint32_t(pl.dim);
    a.ga = pl.ga.n;
    a.gd = pl.gd.n;
    fill_detuning(a.dmask, a.dcnt, pl);
    a.pair = rt.parg;  // (tables uploaded by prepare)
    a.xyt.xy = rt.xarg;
    a.xyt.P = pl.N * (pl.N - 1) / 2;
    a.xyt.dJ = (have_dxy && pl.xy_mode && pl.N > 1) ? reinterpret_cast<const double*>(ws + lay.off_dxy) : nullptr;
    a.nflip = 0;
    for (int q = 0; q < pl.ga.n; ++q)
        for (uint32_t m = pl.ga.amp_index_mask[q]; m; m &= m - 1) {
            a.fbg[a.nflip++] = uint32_t(__builtin_ctz(m)) | (uint32_t(q) << 8);
        }
}

int launch_factor_tangent(TangentFactorArgs& a, const Runtime& rt, char* ws, const TangentLayout& lay, int n_dir, const double2* xin,
                          double2* xout, int stage, const FactorScalars& s, hipStream_t stream) {
    const Plan& pl = rt.pl;
    a.xin = xin;
    a.xout = xout;
    a.coef = rt.coef(ws, stage);
    a.dcoef = reinterpret_cast<const double*>(ws + lay.off_dcoef) + size_t(stage) * pl.NC;
    a.gr = s.gr;
    a.gi = s.gi;
    a.br = s.br;
    a.bi = s.bi;
    const dim3 grid(unsigned((pl.dim + 255) / 256), unsigned(pl.B));
    switch (tangent_padded(n_dir)) {
        case 1: launch_factor_tangent_n<1>(a, grid, stream); break;
        case 2: launch_factor_tangent_n<2>(a, grid, stream); break;
        case 3: launch_factor_tangent_n<3>(a, grid, stream); break;
        case 4: launch_factor_tangent_n<4>(a, grid, stream); break;
        case 6: launch_factor_tangent_n<6>(a, grid, stream); break;
        case 8: launch_factor_tangent_n<8>(a, grid, stream); break;
        default: return fail(RYDIFF_EINVAL, "internal: n_dir out of range");
    }
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// observable tangents of every row at save point k: vec = [1 + D][B][dim] with the state first; dexp = dexpect_out
int launch_expect_tangent(const ForwardCtx& c, const double2* vec, int n_dir, int k, double* dexp) {
    const Plan& pl = c.rt.pl;
    const size_t vstride = size_t(pl.B) * pl.dim;
    const ExpectRows rows(pl);
    const size_t dstride = rows.size();
    const unsigned red_blocks = unsigned(std::min<size_t>((pl.dim + 255) / 256, 1024));
    if (pl.n_obs > 0) {
        hipLaunchKernelGGL(k_expect_tangent, dim3(red_blocks, unsigned(pl.B), unsigned(n_dir)), dim3(256), 0, c.stream, vec, vec + vstride, vstride,
                           c.p->obs_diag, dexp, dstride, pl.n_obs, pl.T + 1, k, pl.B, uint32_t(pl.dim));
        LAUNCH_CHECK();
    }
    if (pl.n_pobs > 0) {
        PauliTangentArgs a{};
        a.psi = vec;
        a.dpsi = vec + vstride;
        a.vstride = vstride;
        a.t = pauli_tables(pl, c.ws);
        a.out = rows.at(dexp, ExpectRows::Pauli);
        a.out_dstride = dstride;
        a.n_pobs = pl.n_pobs;
        a.n_tsave = pl.T + 1;
        a.k = k;
        a.B = pl.B;
        a.dim = uint32_t(pl.dim);
        hipLaunchKernelGGL(k_pauli_expect_tangent, dim3(red_blocks, unsigned(pl.B), unsigned(pl.n_pobs * n_dir)), dim3(256), 0, c.stream, a);
        LAUNCH_CHECK();
    }
    if (pl.n_ov > 0) {  // Re / Im <phi_o|dpsi_d>: k_overlap_expect as it is, on the tangent, into direction d's overlap rows
        for (int d = 0; d < n_dir; ++d) {
            ForwardCtx t = c;
            t.overlap_out = rows.at(dexp + size_t(d) * dstride, ExpectRows::Overlap);
            if (const int rc = launch_overlap_expect(t, vec + size_t(1 + d) * vstride, 0, k, 1, BatchSlice{0, pl.B, false})) return rc;
        }
    }
    if (pl.n_rdm > 0)  // d rho_A = Tr_E(|dpsi_d><psi| + |psi><dpsi_d|): k_rdm_tangent, one launch per RDM over all directions
        if (const int rc = launch_rdm_tangent(c, vec, n_dir, k, rows.at(dexp, ExpectRows::Rdm), dstride)) return rc;
    if (pl.moments)  // d S, d B_q, d B_qr: the moments of 2 Re(conj psi . dpsi_d), k_moments_tangent over all directions
        if (const int rc = launch_moments_tangent(c, vec, n_dir, k, rows.at(dexp, ExpectRows::Moments), dstride)) return rc;
    if (pl.dm_rows()) {
        // diagonal, Pauli, fidelity and moment rows are linear in vec(rho): k_dm_trace / k_dm_fidelity / k_dm_moments as they are, on d rho_d, into direction
        // d's density-matrix rows; the purity |v|^2 has the tangent 2 Re <v|dv_d>
        double* first = rows.at(dexp, ExpectRows::DmTrace, ExpectRows::End);
        for (int d = 0; d < n_dir; ++d) {
            ForwardCtx t = c;
            t.dm_out = first + size_t(d) * dstride;
            if (const int rc = launch_dm_expect(t, vec + size_t(1 + d) * vstride, 0, k, 1, BatchSlice{0, pl.B, false}, true)) return rc;
        }
        if (pl.dm_purity) {
            if (const int rc = launch_dm_purity_tangent(c, vec, n_dir, k, rows.at(dexp, ExpectRows::DmPurity), dstride)) return rc;
        }
    }
    return RYDIFF_OK;
}

}  // namespace
