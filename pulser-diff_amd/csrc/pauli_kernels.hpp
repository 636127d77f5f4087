// pauli_kernels.hpp — Pauli-string observables (include/rydiff.h: RydProblem.pauli_*), matrix-free:
//   (P psi)[y] = i^ny * (-1)^popcount((y ^ xm) & zm) * psi[y ^ xm]
// k_pauli_expect_direct   <psi|O_o|psi> of one or many stored states, one amplitude per thread, partners by global loads
// k_pauli_expect_tile     the same sums for 13..24 qubits: a workgroup stages one tile of the state in LDS once and takes every
//                         partner from there, one pass per tile layout that has work
// k_pauli_apply           the cotangent  base + 2 * sum_o g_o * O_o psi  (a gather: no atomics), g read on the device
// The tables (plan.hpp: PauliGroup / PauliString) hold every observable's strings grouped by flip mask: one partner load per
// distinct mask, all strings that share it applied to the same pair of registers.  y ^ xm maps an aligned run of amplitudes to an
// aligned run, so the partner loads stay coalesced (flips below the line size permute inside a line).
#pragma once

struct PauliTables {
    const int32_t* gfirst = nullptr;       // [n_pobs + 1]
    const PauliGroup* groups = nullptr;    // [gfirst[n_pobs]]
    const PauliString* strings = nullptr;  // by group
};

struct PauliExpectArgs {
    const double2* psi;  // state at save point k0, trajectory 0
    size_t kstride;      // amplitudes between consecutive save points (grid.y covers b_count * n_k states)
    PauliTables t;
    double* out;         // &expect_out[n_obs][0][0]: [n_pobs][n_tsave][B]
    int n_tsave, k0, B, b_first, b_count;
    uint32_t dim;
};

// grid (blocks, b_count * n_k, n_pobs); one atomic per block into the observable's slot
__global__ __launch_bounds__(256) void k_pauli_expect_direct(PauliExpectArgs a) {
    __shared__ double lds[8];
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const int o = blockIdx.z;
    const double2* __restrict__ psi = a.psi + size_t(kk) * a.kstride + size_t(b) * a.dim;
    const int g0 = a.t.gfirst[o], g1 = a.t.gfirst[o + 1];
    bool mine = false;  // (uniform) tile passes may have taken every group of this observable
    for (int g = g0; g < g1; ++g) mine |= a.t.groups[g].layout == kPauliDirect;
    if (!mine) return;
    double acc = 0.0;
    for (uint32_t y = blockIdx.x * 256u + threadIdx.x; y < a.dim; y += gridDim.x * 256u) {
        const double2 v = psi[y];
        for (int g = g0; g < g1; ++g) {  // uniform
            const PauliGroup gr = a.t.groups[g];
            if (gr.layout != kPauliDirect) continue;  // evaluated by a tile pass
            const uint32_t yp = y ^ gr.xm;
            const double2 q = gr.xm ? psi[yp] : v;
            const double tr = v.x * q.x + v.y * q.y, ti = v.x * q.y - v.y * q.x;  // conj(psi[y]) * psi[y ^ xm]
            for (uint32_t s = gr.first; s < gr.first + gr.count; ++s) {
                const PauliString st = a.t.strings[s];
                const double val = st.wr * tr - st.wi * ti;
                acc += (__popc(yp & st.zm) & 1u) ? -val : val;
            }
        }
    }
    block_atomic_add(acc, a.out + (size_t(o) * a.n_tsave + a.k0 + kk) * a.B + b, lds);
}

struct PauliTileArgs {
    const double2* psi;  // the state at save point k, trajectory 0
    PauliTables t;
    double* out;         // &expect_out[n_obs][0][0]
    int n_pobs, n_tsave, k, B, b_first;
    uint32_t dim;
    int lo, hs, hb;      // the tile layout (runtime.hpp: LayoutDesc): tile bit b <-> index bit b (b < lo) or hs + b - lo
    uint32_t layout;     // which groups this pass evaluates (PauliGroup.layout)
};

// grid (tiles, b_count), 1024 threads, LDS: the tile in index order (2^LT amplitudes) + 32 doubles.  Staged with one 16-byte load
// per amplitude (consecutive threads: consecutive amplitudes of a run); partner reads y ^ xm permute the 16-byte slots: a flip
// below tile bit 4 is a bijection on (slot mod 16), a higher one leaves it unchanged — no padding, no swizzle.
template <int LT>
__global__ __launch_bounds__(1024) void k_pauli_expect_tile(PauliTileArgs a) {
    extern __shared__ double2 pauli_tile[];
    constexpr uint32_t NT = 1024, R = (1u << LT) / NT;
    double* red = reinterpret_cast<double*>(pauli_tile + (1u << LT));
    const int b = a.b_first + int(blockIdx.y);
    const uint32_t tau = blockIdx.x, lomask = (1u << a.lo) - 1u;
    const int mid = a.hs - a.lo;
    const uint32_t x0 = ((tau & ((1u << mid) - 1u)) << a.lo) | ((tau >> mid) << (a.hs + a.hb));  // index bits outside the tile
    auto index_of = [&](uint32_t t) { return x0 | (t & lomask) | ((t >> a.lo) << a.hs); };
    const double2* __restrict__ psi = a.psi + size_t(b) * a.dim;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t t = r * NT + threadIdx.x;
        pauli_tile[t] = psi[index_of(t)];
    }
    __syncthreads();
    for (int o = 0; o < a.n_pobs; ++o) {
        double acc = 0.0;
        for (int g = a.t.gfirst[o]; g < a.t.gfirst[o + 1]; ++g) {  // uniform
            const PauliGroup gr = a.t.groups[g];
            if (gr.layout != a.layout) continue;
            const uint32_t xmt = (gr.xm & lomask) | ((gr.xm >> a.hs) << a.lo);  // the flip mask in tile bits (no bit outside the tile)
#pragma unroll
            for (uint32_t r = 0; r < R; ++r) {
                const uint32_t t = r * NT + threadIdx.x, tp = t ^ xmt;
                const double2 v = pauli_tile[t], q = pauli_tile[tp];
                const uint32_t yp = index_of(tp);
                const double tr = v.x * q.x + v.y * q.y, ti = v.x * q.y - v.y * q.x;
                for (uint32_t s = gr.first; s < gr.first + gr.count; ++s) {
                    const PauliString st = a.t.strings[s];
                    const double val = st.wr * tr - st.wi * ti;
                    acc += (__popc(yp & st.zm) & 1u) ? -val : val;
                }
            }
        }
        block_atomic_add(acc, a.out + (size_t(o) * a.n_tsave + a.k) * a.B + b, red);
    }
}

struct PauliApplyArgs {
    const double2* psi;    // trajectory: the state at save point k is psi + index(k) * B * dim, index(k) = entry ? entry[k] : k * kmul
    const int32_t* entry;  // full tape of the one-launch sweeps: tape entry of every save point; else nullptr
    int kmul;              // 0: psi IS the state at the one save point of this launch
    const double2* base;   // grad_states [n_tsave][B][dim] or nullptr
    double2* out;          // [n_k][B][dim]
    const double* gexp;    // &grad_expect[n_obs][0][0]: [n_pobs][n_tsave][B]
    PauliTables t;
    int n_pobs, n_tsave, k0, B;
    uint32_t dim;
};

// grid (dim / 256, B, n_k): out[kk][b][y] = base[k][b][y] + 2 * sum_o g[o][k][b] * (O_o psi_k)[y],  k = k0 + kk
__global__ __launch_bounds__(256) void k_pauli_apply(PauliApplyArgs a) {
    const uint32_t y = blockIdx.x * 256u + threadIdx.x;
    if (y >= a.dim) return;
    const int b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t sv = size_t(a.B) * a.dim;
    const double2* __restrict__ psi = a.psi + size_t(a.entry ? a.entry[k] : k * a.kmul) * sv + size_t(b) * a.dim;
    double ar = 0.0, ai = 0.0;
    for (int o = 0; o < a.n_pobs; ++o) {
        const double g = a.gexp[(size_t(o) * a.n_tsave + k) * a.B + b];
        if (g == 0.0) continue;  // uniform: cotangents usually sit at one or a few save points
        double sr = 0.0, si = 0.0;
        for (int gi = a.t.gfirst[o]; gi < a.t.gfirst[o + 1]; ++gi) {
            const PauliGroup gr = a.t.groups[gi];
            const uint32_t yp = y ^ gr.xm;
            const double2 q = psi[yp];
            for (uint32_t s = gr.first; s < gr.first + gr.count; ++s) {
                const PauliString st = a.t.strings[s];
                const double vr = st.wr * q.x - st.wi * q.y, vi = st.wr * q.y + st.wi * q.x;
                const bool neg = (__popc(yp & st.zm) & 1u) != 0u;
                sr += neg ? -vr : vr;
                si += neg ? -vi : vi;
            }
        }
        ar = fma(2.0 * g, sr, ar);
        ai = fma(2.0 * g, si, ai);
    }
    if (a.base) {
        const double2 g = a.base[size_t(k) * sv + size_t(b) * a.dim + y];
        ar += g.x;
        ai += g.y;
    }
    a.out[size_t(blockIdx.z) * sv + size_t(b) * a.dim + y] = make_double2(ar, ai);
}
