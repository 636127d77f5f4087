// dm_launch.hpp — density-matrix observables (dm_kernels.hpp): where the string tables live, the evaluation launches and the shots
// behind launch_observables_expect, and the density-matrix part of the observable cotangent (overlap_launch.hpp).
#pragma once

namespace {

DmTables dm_tables(const Plan& pl, const char* ws) {
    DmTables t;
    const char* base = ws + pl.off_dm;
    t.gfirst = reinterpret_cast<const int32_t*>(base);
    base += pl.dm_gfirst_bytes();
    t.groups = reinterpret_cast<const PauliGroup*>(base);
    base += pl.dm_groups.size() * sizeof(PauliGroup);
    t.agroups = reinterpret_cast<const PauliGroup*>(base);
    base += pl.dm_agroups.size() * sizeof(PauliGroup);
    t.strings = reinterpret_cast<const PauliString*>(base);
    base += pl.dm_strings.size() * sizeof(PauliString);
    t.astrings = reinterpret_cast<const PauliString*>(base);
    return t;
}

// tables -> workspace as kernel arguments (like every other piece of host metadata)
int upload_dm_tables(const Plan& pl, char* ws, hipStream_t stream) {
    if (!pl.dm_n || !pl.dm_bytes()) return RYDIFF_OK;
    std::vector<unsigned char> img(pl.dm_bytes(), 0);
    size_t off = 0;
    auto put = [&](const void* src, size_t bytes, size_t padded) {
        if (bytes) memcpy(img.data() + off, src, bytes);
        off += padded;
    };
    put(pl.dm_gfirst.data(), pl.dm_gfirst.size() * sizeof(int32_t), pl.dm_gfirst_bytes());
    put(pl.dm_groups.data(), pl.dm_groups.size() * sizeof(PauliGroup), pl.dm_groups.size() * sizeof(PauliGroup));
    put(pl.dm_agroups.data(), pl.dm_agroups.size() * sizeof(PauliGroup), pl.dm_agroups.size() * sizeof(PauliGroup));
    put(pl.dm_strings.data(), pl.dm_strings.size() * sizeof(PauliString), pl.dm_strings.size() * sizeof(PauliString));
    put(pl.dm_astrings.data(), pl.dm_astrings.size() * sizeof(PauliString), pl.dm_astrings.size() * sizeof(PauliString));
    return upload_words(stream, ws + pl.off_dm, img.data(), img.size());
}

template <int NO>
void launch_dm_fidelity_n(const DmFidArgs& a, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((k_dm_fidelity<NO>), grid, dim3(256), 0, stream, a);
}

// every density-matrix row on the states of save points k0 .. k0 + nk - 1 (kstride amplitudes apart; `v` is the one at k0,
// trajectory 0), trajectories of `bs`.  `linear_only`: the rows that are linear in vec(rho) — diagonal, Pauli, fidelity, moments — and nothing
// else: what the tangent sweep runs on a tangent vector d rho_d, with c.dm_out redirected to direction d's rows of dexpect_out (the
// purity row, quadratic, is k_dm_purity_tangent's)
int launch_dm_expect(const ForwardCtx& c, const double2* v, size_t kstride, int k0, int nk, const BatchSlice& bs, bool linear_only = false) {
    const Plan& pl = c.rt.pl;
    if (!c.dm_out) return RYDIFF_OK;
    const ExpectRows rows(pl);  // (c.dm_out is the first density-matrix row: offsets from DmTrace)
    const size_t D = size_t(1) << pl.dm_n;
    const int kmax = std::max(1, 65535 / bs.count);  // grid.y
    const int n_trace = rows.count(ExpectRows::DmTrace);
    for (int k = 0; k < nk; k += kmax) {
        const unsigned gy = unsigned(bs.count * std::min(kmax, nk - k));
        if (n_trace) {
            DmTraceArgs a{};
            a.v = v + size_t(k) * kstride;
            a.kstride = kstride;
            a.t = dm_tables(pl, c.ws);
            a.diag = c.p->dm_diag;
            a.out = c.dm_out;
            a.n_diag = pl.n_dm_diag;
            a.n_tsave = pl.T + 1;
            a.k0 = k0 + k;
            a.B = pl.B;
            a.b_first = bs.first;
            a.b_count = bs.count;
            a.n = pl.dm_n;
            hipLaunchKernelGGL(k_dm_trace, dim3(unsigned((D + 255) / 256), gy, unsigned(n_trace)), dim3(256), 0, c.stream, a);
            LAUNCH_CHECK();
        }
        const int purity = linear_only ? 0 : pl.dm_purity;
        if (pl.n_dm_fid || purity) {
            DmFidArgs a{};
            a.v = v + size_t(k) * kstride;
            a.kstride = kstride;
            a.phi = static_cast<const double2*>(c.p->dm_fid_targets);
            a.out = c.dm_out + rows.offset(ExpectRows::DmFid, ExpectRows::DmTrace);
            a.n_fid = pl.n_dm_fid;
            a.fid_batch = pl.dm_fid_batch;
            a.purity = purity;
            a.n_tsave = pl.T + 1;
            a.k0 = k0 + k;
            a.B = pl.B;
            a.b_first = bs.first;
            a.b_count = bs.count;
            a.n = pl.dm_n;
            const dim3 grid(unsigned(std::min<size_t>((D * D + 255) / 256, 1024)), gy);
            if (pl.n_dm_fid <= 1) launch_dm_fidelity_n<1>(a, grid, c.stream);  // (also the purity alone: zero targets)
            else if (pl.n_dm_fid <= 2) launch_dm_fidelity_n<2>(a, grid, c.stream);
            else if (pl.n_dm_fid <= 4) launch_dm_fidelity_n<4>(a, grid, c.stream);
            else if (pl.n_dm_fid <= 8) launch_dm_fidelity_n<8>(a, grid, c.stream);
            else launch_dm_fidelity_n<RYDIFF_MAX_OVERLAPS>(a, grid, c.stream);
            LAUNCH_CHECK();
        }
        if (pl.n_dm_rdm && !linear_only) {
            DmRdmArgs a{};
            a.v = v + size_t(k) * kstride;
            a.kstride = kstride;
            a.out = c.dm_out + rows.offset(ExpectRows::DmRdm, ExpectRows::DmTrace);
            a.n_tsave = pl.T + 1;
            a.k0 = k0 + k;
            a.B = pl.B;
            a.b_first = bs.first;
            a.b_count = bs.count;
            a.n = pl.dm_n;
            int m_max = 0;
            for (int o = 0; o < pl.n_dm_rdm; ++o) {
                a.am[o] = pl.dm_rdm_am[o];
                a.m[o] = pl.dm_rdm_m[o];
                a.row[o] = pl.dm_rdm_row[o];
                m_max = std::max(m_max, pl.dm_rdm_m[o]);
            }
            hipLaunchKernelGGL(k_dm_rdm, dim3(1u << m_max, gy, unsigned(pl.n_dm_rdm)), dim3(256), 0, c.stream, a);
            LAUNCH_CHECK();
        }
        if (pl.dm_moments) {  // linear in vec(rho): also what the tangent sweep runs on d rho_d
            DmMomentsArgs a{};
            a.v = v + size_t(k) * kstride;
            a.kstride = kstride;
            a.out = c.dm_out + rows.offset(ExpectRows::DmMoments, ExpectRows::DmTrace);
            a.n_tsave = pl.T + 1;
            a.k0 = k0 + k;
            a.B = pl.B;
            a.b_first = bs.first;
            a.b_count = bs.count;
            a.n = pl.dm_n;
            hipLaunchKernelGGL(k_dm_moments, dim3(1, gy), dim3(256), 0, c.stream, a);
            LAUNCH_CHECK();
        }
    }
    return RYDIFF_OK;
}

// tangent of the purity row at save point k: vec = [1 + D][B][4^n] with vec(rho) first; slot = &dexpect_out[0][purity row][0][0]
int launch_dm_purity_tangent(const ForwardCtx& c, const double2* vec, int n_dir, int k, double* slot, size_t dstride) {
    const Plan& pl = c.rt.pl;
    DmPurityTangentArgs a{};
    a.v = vec;
    a.dv = vec + size_t(pl.B) * pl.dim;
    a.vstride = size_t(pl.B) * pl.dim;
    a.out = slot;
    a.out_dstride = dstride;
    a.k = k;
    a.B = pl.B;
    a.total = uint32_t(pl.dim);
    const unsigned blocks = unsigned(std::min<size_t>((pl.dim + 255) / 256, 1024));
    hipLaunchKernelGGL(k_dm_purity_tangent, dim3(blocks, unsigned(pl.B), unsigned(n_dir)), dim3(256), 0, c.stream, a);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// dm_shots: the shots of every SAMPLED save point among k0 .. k0 + nk - 1, drawn from the diagonal of rho
int launch_dm_shots(const ForwardCtx& c, const double2* v, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.shots_out) return RYDIFF_OK;
    for (size_t si = 0; si < pl.shot_times.size(); ++si) {
        const int k = pl.shot_times[si];
        if (k < k0 || k >= k0 + nk) continue;
        const size_t at = si * size_t(pl.B) * size_t(pl.n_shots);
        const DmShotArgs a{v + size_t(k - k0) * kstride, c.shot_u + at, c.shots_out + at, pl.dm_n, pl.n_shots, bs.first};
        hipLaunchKernelGGL(k_dm_shots, dim3(unsigned(bs.count)), dim3(256), 0, c.stream, a);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

// out[kk] = base[kk] + the cotangents of the density-matrix rows at save point k0 + kk,  kk < nk; base: [nk][B][4^n] or nullptr, may
// be `out` (the state at save point k as launch_pauli_apply takes it: psi / entry / kmul)
void launch_dm_apply(const PauliInject& pi, const double2* psi, const int32_t* entry, int kmul, int k0, int nk, const double2* base,
                     double2* out) {
    const Plan& pl = pi.rt->pl;
    const ExpectRows rows(pl);  // (pi.dm_gexp is the first density-matrix row: offsets from DmTrace)
    const size_t D = size_t(1) << pl.dm_n;
    if (pl.n_dm_fid || pl.dm_purity || base != out) {  // the dense pass (also what copies or clears where nothing has written `out` yet)
        DmApplyArgs a{};
        a.psi = psi;
        a.entry = entry;
        a.kmul = kmul;
        a.base = base;
        a.out = out;
        a.phi = pi.dm_phi;
        a.g_fid = pi.dm_gexp + rows.offset(ExpectRows::DmFid, ExpectRows::DmTrace);
        a.g_pur = pl.dm_purity ? pi.dm_gexp + rows.offset(ExpectRows::DmPurity, ExpectRows::DmTrace) : nullptr;
        a.n_fid = pl.n_dm_fid;
        a.fid_batch = pl.dm_fid_batch;
        a.n_tsave = pl.T + 1;
        a.k0 = k0;
        a.B = pl.B;
        a.n = pl.dm_n;
        hipLaunchKernelGGL(k_dm_apply, dim3(unsigned((D * D + 255) / 256), unsigned(pl.B), unsigned(nk)), dim3(256), 0, pi.stream, a);
    }
    if (!pl.dm_agroups.empty()) {
        DmScatterArgs a{};
        a.out = out;
        a.t = dm_tables(pl, pi.ws);
        a.diag = pi.dm_diag;
        a.gexp = pi.dm_gexp;
        a.n_diag = pl.n_dm_diag;
        a.n_tsave = pl.T + 1;
        a.k0 = k0;
        a.B = pl.B;
        a.n = pl.dm_n;
        a.xblocks = uint32_t((D + 255) / 256);
        hipLaunchKernelGGL(k_dm_scatter, dim3(a.xblocks * unsigned(pl.dm_agroups.size()), unsigned(pl.B), unsigned(nk)), dim3(256), 0,
                           pi.stream, a);
    }
    // one launch per RDM, in stream order: two RDMs (or an RDM and a row above) may own the same entry
    for (int o = 0; o < pl.n_dm_rdm; ++o) {
        DmRdmScatterArgs a{};
        a.out = out;
        a.gexp = pi.dm_gexp + rows.offset(ExpectRows::DmRdm, ExpectRows::DmTrace) + size_t(pl.dm_rdm_row[o]) * rows.stride;
        a.n_tsave = pl.T + 1;
        a.k0 = k0;
        a.B = pl.B;
        a.n = pl.dm_n;
        a.m = pl.dm_rdm_m[o];
        a.am = pl.dm_rdm_am[o];
        hipLaunchKernelGGL(k_dm_rdm_scatter, dim3(unsigned(((D << a.m) + 255) / 256), unsigned(pl.B), unsigned(nk)), dim3(256), 0, pi.stream, a);
    }
    if (pl.dm_moments) {  // behind them all: the diagonal rows, the xm = 0 strings and the RDMs own the same entries
        DmMomentsScatterArgs a{};
        a.out = out;
        a.gexp = pi.dm_gexp + rows.offset(ExpectRows::DmMoments, ExpectRows::DmTrace);
        a.n_tsave = pl.T + 1;
        a.k0 = k0;
        a.B = pl.B;
        a.n = pl.dm_n;
        hipLaunchKernelGGL(k_dm_moments_scatter, dim3(unsigned((D + 255) / 256), unsigned(pl.B), unsigned(nk)), dim3(256), 0, pi.stream, a);
    }
}

}  // namespace
