// pauli_launch.hpp — Pauli-string observables (pauli_kernels.hpp): where the tables live, the evaluation launches of the forward
// sweeps and the Pauli part of the cotangent the adjoint sweeps inject at a save point (overlap_launch.hpp: observable_cotangent).
#pragma once

namespace {

PauliTables pauli_tables(const Plan& pl, const char* ws) {
    PauliTables t;
    const char* base = ws + pl.off_pauli;
    t.gfirst = reinterpret_cast<const int32_t*>(base);
    t.groups = reinterpret_cast<const PauliGroup*>(base + pl.pauli_gfirst_bytes());
    t.strings = reinterpret_cast<const PauliString*>(base + pl.pauli_gfirst_bytes() + pl.pauli_groups.size() * sizeof(PauliGroup));
    return t;
}

// tables -> workspace as kernel arguments (like every other piece of host metadata: no copy engine, no synchronisation)
int upload_pauli_tables(const Plan& pl, char* ws, hipStream_t stream) {
    if (!pl.n_pobs) return RYDIFF_OK;
    std::vector<unsigned char> img(pl.pauli_bytes(), 0);
    memcpy(img.data(), pl.pauli_gfirst.data(), pl.pauli_gfirst.size() * sizeof(int32_t));
    size_t off = pl.pauli_gfirst_bytes();
    if (!pl.pauli_groups.empty()) memcpy(img.data() + off, pl.pauli_groups.data(), pl.pauli_groups.size() * sizeof(PauliGroup));
    off += pl.pauli_groups.size() * sizeof(PauliGroup);
    if (!pl.pauli_strings.empty()) memcpy(img.data() + off, pl.pauli_strings.data(), pl.pauli_strings.size() * sizeof(PauliString));
    return upload_words(stream, ws + pl.off_pauli, img.data(), img.size());
}

// Tile size of k_pauli_expect_tile: the chained passes' (2^12 amplitudes, the wide 2^13 where the chain uses them), two layouts;
// 0: this problem is evaluated by the direct kernel alone (up to 12 qubits: cache-resident; from 25 on; direct kernels forced)
int pauli_tile_bits(const Runtime& rt) {
    const Plan& pl = rt.pl;
    if (rt.variant == 1 || pl.shard_bits || !pl.n_pobs) return 0;
    const int lt = chain_geom(rt).lt == kWideTileBits ? kWideTileBits : kTileBits;
    return (pl.NL > lt && pl.NL <= 24) ? lt : 0;
}

// Every distinct flip mask goes to the first tile layout whose bits contain it (diagonal strings ride the first pass); masks that
// straddle the layouts stay with the direct kernel.
void assign_pauli_layouts(Runtime& rt) {
    Plan& pl = rt.pl;
    const int lt = pauli_tile_bits(rt);
    pl.pauli_work[0] = pl.pauli_work[1] = pl.pauli_work[2] = false;
    for (PauliGroup& g : pl.pauli_groups) {
        g.layout = kPauliDirect;
        for (int l = 0; lt && l < 2; ++l)
            if ((g.xm & ~chain_layout(pl.NL, l, ChainGeom{lt, 2}).bits) == 0u) {
                g.layout = uint32_t(l);
                break;
            }
        pl.pauli_work[g.layout == kPauliDirect ? 2 : g.layout] = true;
    }
}

template <int LT>
int launch_pauli_tile(const PauliTileArgs& a, unsigned tiles, unsigned b_count, hipStream_t stream) {
    const size_t lds = (size_t(1) << LT) * sizeof(double2) + 32 * sizeof(double);
    if (int rc = set_max_dynamic_lds_once<&k_pauli_expect_tile<LT>>(lds)) return rc;
    hipLaunchKernelGGL((k_pauli_expect_tile<LT>), dim3(tiles, b_count), dim3(1024), lds, stream, a);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// <psi|O_o|psi> for every Pauli observable on the states of save points k0 .. k0 + nk - 1 (kstride amplitudes apart; `psi` is the
// one at k0, trajectory 0), trajectories of `bs`
int launch_pauli_expect(const ForwardCtx& c, const double2* psi, size_t kstride, int k0, int nk, const BatchSlice& bs) {
    const Plan& pl = c.rt.pl;
    if (!c.pauli_out) return RYDIFF_OK;
    const int lt = pauli_tile_bits(c.rt);
    for (int l = 0; lt && l < 2; ++l) {  // one pass per tile layout that has work (lt != 0: launch-per-factor sweeps, nk == 1)
        if (!pl.pauli_work[l]) continue;
        const LayoutDesc d = chain_layout(pl.NL, l, ChainGeom{lt, 2});
        for (int k = 0; k < nk; ++k) {
            PauliTileArgs a{};
            a.psi = psi + size_t(k) * kstride;
            a.t = pauli_tables(pl, c.ws);
            a.out = c.pauli_out;
            a.n_pobs = pl.n_pobs;
            a.n_tsave = pl.T + 1;
            a.k = k0 + k;
            a.B = pl.B;
            a.b_first = bs.first;
            a.dim = uint32_t(pl.dim);
            a.lo = d.lo;
            a.hs = d.hs;
            a.hb = d.hb;
            a.layout = uint32_t(l);
            const int rc = lt == kWideTileBits ? launch_pauli_tile<kWideTileBits>(a, unsigned(pl.dim >> lt), unsigned(bs.count), c.stream)
                                               : launch_pauli_tile<kTileBits>(a, unsigned(pl.dim >> lt), unsigned(bs.count), c.stream);
            if (rc) return rc;
        }
    }
    if (!pl.pauli_work[2]) return RYDIFF_OK;  // no group left for the direct kernel
    const unsigned red_blocks = unsigned(std::min<size_t>((pl.dim + 255) / 256, 1024));
    const int kmax = std::max(1, 65535 / bs.count);  // grid.y
    for (int k = 0; k < nk; k += kmax) {
        PauliExpectArgs a{};
        a.psi = psi + size_t(k) * kstride;
        a.kstride = kstride;
        a.t = pauli_tables(pl, c.ws);
        a.out = c.pauli_out;
        a.n_tsave = pl.T + 1;
        a.k0 = k0 + k;
        a.B = pl.B;
        a.b_first = bs.first;
        a.b_count = bs.count;
        a.dim = uint32_t(pl.dim);
        hipLaunchKernelGGL(k_pauli_expect_direct, dim3(red_blocks, unsigned(bs.count * std::min(kmax, nk - k)), unsigned(pl.n_pobs)), dim3(256), 0,
                           c.stream, a);
        LAUNCH_CHECK();
    }
    return RYDIFF_OK;
}

// out[kk] = grad_states[k0 + kk] + 2 sum_o grad_expect[n_obs + o][k0 + kk] O_o psi_{k0 + kk},  kk < nk
void launch_pauli_apply(const PauliInject& pi, const double2* psi, const int32_t* entry, int kmul, int k0, int nk, double2* out) {
    const Plan& pl = pi.rt->pl;
    PauliApplyArgs a{};
    a.psi = psi;
    a.entry = entry;
    a.kmul = kmul;
    a.base = pi.gstate;
    a.out = out;
    a.gexp = pi.gexp;
    a.t = pauli_tables(pl, pi.ws);
    a.n_pobs = pl.n_pobs;
    a.n_tsave = pl.T + 1;
    a.k0 = k0;
    a.B = pl.B;
    a.dim = uint32_t(pl.dim);
    hipLaunchKernelGGL(k_pauli_apply, dim3(unsigned((pl.dim + 255) / 256), unsigned(pl.B), unsigned(nk)), dim3(256), 0, pi.stream, a);
}

}  // namespace
