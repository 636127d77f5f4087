// rdm_launch.hpp — reduced density matrices (rdm_kernels.hpp): the tile geometry of one RDM, the evaluation launches of the forward
// sweeps, the RDM tangents of the tangent sweep (tangent_launch.hpp: launch_expect_tangent) and the RDM part of the observable
// cotangent (overlap_launch.hpp: launch_observable_cotangent).  One launch per RDM.
#pragma once

namespace {

// The staged bit set of RDM o: A plus the lowest t - m environment bits, t = min(N, tmax); staged index bits in the order of the
// global ones, so a and e keep the order of the index bits (lowest-numbered qubit = highest index bit = most significant in a).
RdmTile rdm_tile(const Plan& pl, int o, int tmax) {
    RdmTile g{};
    const uint32_t am = pl.rdm_am[o];
    g.m = pl.rdm_m[o];
    g.t = std::min(pl.NL, tmax);
    uint32_t staged = am;
    for (int bit = 0, need = g.t - g.m; need > 0; ++bit)
        if (!(am >> bit & 1u)) {
            staged |= 1u << bit;
            --need;
        }
    int i = 0, ai = 0, ei = 0;
    for (int bit = 0; bit < pl.NL; ++bit) {
        if (!(staged >> bit & 1u)) {
            g.hbit[g.nh++] = 1u << bit;
            continue;
        }
        g.ybit[i] = 1u << bit;
        if (am >> bit & 1u) g.abit[i] = 1u << ai++;
        else g.ebit[i] = 1u << ei++;
        ++i;
    }
    g.stride = (1u << (g.t - g.m)) + 1u;
    return g;
}

size_t rdm_tile_bytes(int m, int t) { return (size_t(1) << m) * ((size_t(1) << (t - m)) + 1) * sizeof(double2); }

// dynamic LDS of k_rdm_expect<M>: the tile, or the reduction scratch that reuses its place where that is larger (tiny registers)
size_t rdm_expect_lds(int m, int t) {
    const size_t d = size_t(1) << m;
    const size_t red = m <= 3 ? size_t(kRdmThreads / 64) * d * (d + 1) * sizeof(double) : size_t(136) * (d / 16) * (d / 16) * 2 * sizeof(double);
    return std::max(rdm_tile_bytes(m, t), red);
}

template <int M>
int launch_rdm_expect_m(const RdmExpectArgs& a, dim3 grid, hipStream_t stream) {
    if (int rc = set_max_dynamic_lds_once<&k_rdm_expect<M>>(rdm_expect_lds(M, kRdmTileBits))) return rc;
    hipLaunchKernelGGL((k_rdm_expect<M>), grid, dim3(kRdmThreads), rdm_expect_lds(M, a.g.t), stream, a);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// rho_A of every RDM on the states of save points k0 .. k0 + nk - 1 (kstride amplitudes apart; `psi` is the one at k0,
// trajectory 0), trajectories of `bs`
int launch_rdm_expect(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.rdm_out) return RYDIFF_OK;
    const size_t row = size_t(pl.T + 1) * pl.B;
    const int kmax = std::max(1, 65535 / bs.count);  // grid.y
    for (int o = 0; o < pl.n_rdm; ++o) {
        RdmExpectArgs a{};
        a.g = rdm_tile(pl, o, kRdmTileBits);
        a.kstride = kstride;
        a.out = c.rdm_out + size_t(pl.rdm_row[o]) * row;
        a.n_tsave = pl.T + 1;
        a.B = pl.B;
        a.b_first = bs.first;
        a.b_count = bs.count;
        a.dim = uint32_t(pl.dim);
        a.nblocks = uint32_t(pl.dim >> a.g.t);
        for (int k = 0; k < nk; k += kmax) {
            a.psi = psi + size_t(k) * kstride;
            a.k0 = k0 + k;
            const dim3 grid(std::min<unsigned>(a.nblocks, kRdmMaxBlocks), unsigned(bs.count * std::min(kmax, nk - k)));
            int rc = RYDIFF_OK;
            switch (a.g.m) {
                case 1: rc = launch_rdm_expect_m<1>(a, grid, c.stream); break;
                case 2: rc = launch_rdm_expect_m<2>(a, grid, c.stream); break;
                case 3: rc = launch_rdm_expect_m<3>(a, grid, c.stream); break;
                case 4: rc = launch_rdm_expect_m<4>(a, grid, c.stream); break;
                case 5: rc = launch_rdm_expect_m<5>(a, grid, c.stream); break;
                default: rc = launch_rdm_expect_m<6>(a, grid, c.stream); break;
            }
            if (rc) return rc;
        }
    }
    return RYDIFF_OK;
}

// dynamic LDS of k_rdm_tangent<M>: the Psi tile and the dPsi tile (the reduction scratch reuses their place)
size_t rdm_tangent_lds(int m, int t) { return std::max(2 * rdm_tile_bytes(m, t), rdm_expect_lds(m, t)); }

template <int M>
int launch_rdm_tangent_m(const RdmTangentArgs& a, dim3 grid, hipStream_t stream) {
    if (int rc = set_max_dynamic_lds_once<&k_rdm_tangent<M>>(rdm_tangent_lds(M, kRdmTileBits))) return rc;
    hipLaunchKernelGGL((k_rdm_tangent<M>), grid, dim3(kRdmThreads), rdm_tangent_lds(M, a.g.t), stream, a);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// d rho_A of every RDM and direction at save point k: vec = [1 + n_dir][B][dim] with the state first; `out`: the first RDM row of
// direction 0 in dexpect_out (zeroed by the caller of the sweep's launches: the kernel adds), dstride doubles between directions
int launch_rdm_tangent(const ForwardCtx& c, const double2* vec, int n_dir, int k, double* out, size_t dstride) {
    const Plan& pl = c.rt.pl;
    const size_t row = size_t(pl.T + 1) * pl.B;
    for (int o = 0; o < pl.n_rdm; ++o) {
        RdmTangentArgs a{};
        a.g = rdm_tile(pl, o, kRdmTileBits);
        a.vec = vec;
        a.vstride = size_t(pl.B) * pl.dim;
        a.out = out + size_t(pl.rdm_row[o]) * row;
        a.out_dstride = dstride;
        a.n_tsave = pl.T + 1;
        a.k = k;
        a.B = pl.B;
        a.dim = uint32_t(pl.dim);
        a.nblocks = uint32_t(pl.dim >> a.g.t);
        const dim3 grid(std::min<unsigned>(a.nblocks, kRdmMaxBlocks), unsigned(pl.B), unsigned(n_dir));
        int rc = RYDIFF_OK;
        switch (a.g.m) {
            case 1: rc = launch_rdm_tangent_m<1>(a, grid, c.stream); break;
            case 2: rc = launch_rdm_tangent_m<2>(a, grid, c.stream); break;
            case 3: rc = launch_rdm_tangent_m<3>(a, grid, c.stream); break;
            case 4: rc = launch_rdm_tangent_m<4>(a, grid, c.stream); break;
            case 5: rc = launch_rdm_tangent_m<5>(a, grid, c.stream); break;
            default: rc = launch_rdm_tangent_m<6>(a, grid, c.stream); break;
        }
        if (rc) return rc;
    }
    return RYDIFF_OK;
}

constexpr int rdm_apply_tile_bits(int m) { return m == RYDIFF_MAX_RDM_QUBITS ? kRdmTileBits - 1 : kRdmTileBits; }

size_t rdm_apply_lds(int m, int t) { return (size_t(1) << (2 * m)) * sizeof(double2) + rdm_tile_bytes(m, t); }

// k_rdm_apply's dynamic LDS goes beyond 64 KiB: raised once, by rydiff_backward, ahead of the sweep (whose cotangent launches
// report no status of their own)
int rdm_apply_prepare() {
    return set_max_dynamic_lds_once<&k_rdm_apply>(rdm_apply_lds(RYDIFF_MAX_RDM_QUBITS, rdm_apply_tile_bits(RYDIFF_MAX_RDM_QUBITS)));
}

// out[kk] = base[kk] + sum_o ((G + G^dagger)_{A_o} (x) 1) psi_{k0 + kk},  kk < nk; base: [nk][B][dim] or nullptr, may be `out`
// (the state at save point k as launch_pauli_apply takes it: psi / entry / kmul)
void launch_rdm_apply(const PauliInject& pi, const double2* psi, const int32_t* entry, int kmul, int k0, int nk, const double2* base,
                      double2* out) {
    const Plan& pl = pi.rt->pl;
    const size_t row = size_t(pl.T + 1) * pl.B;
    for (int o = 0; o < pl.n_rdm; ++o) {
        RdmApplyArgs a{};
        a.g = rdm_tile(pl, o, rdm_apply_tile_bits(pl.rdm_m[o]));
        a.psi = psi;
        a.entry = entry;
        a.kmul = kmul;
        a.base = base;
        a.out = out;
        a.gexp = pi.rdm_gexp + size_t(pl.rdm_row[o]) * row;
        a.n_tsave = pl.T + 1;
        a.k0 = k0;
        a.B = pl.B;
        a.dim = uint32_t(pl.dim);
        a.nblocks = uint32_t(pl.dim >> a.g.t);
        hipLaunchKernelGGL(k_rdm_apply, dim3(std::min<unsigned>(a.nblocks, kRdmMaxBlocks), unsigned(pl.B), unsigned(nk)), dim3(kRdmThreads),
                           rdm_apply_lds(a.g.m, a.g.t), pi.stream, a);
        base = out;
    }
}

}  // namespace
