// overlap_kernels.hpp — state-overlap observables (include/rydiff.h: RydProblem.overlap_*):
//   c_o[k][b] = sum_y conj(phi_{o,b}[y]) psi_b(t_k)[y],   rows Re c_o, Im c_o of expect_out behind the Pauli rows
// k_overlap_expect   the complex dot products of one or many stored states with every target: each amplitude of psi is loaded
//                    once (16 bytes, consecutive lanes on consecutive amplitudes) and used against all targets, the accumulator
//                    pairs stay in registers (NO = compile-time bound on the targets, so nothing is indexed dynamically)
// k_overlap_apply    the cotangent  base + sum_o (gRe + i gIm)_o phi_o  (streaming: no atomics), g read on the device
// The targets are read where the caller has them: [n_ov][ov_batch][dim], ov_batch = 1 (shared by the trajectories) or B.
#pragma once

struct OverlapExpectArgs {
    const double2* psi;  // state at save point k0, trajectory 0
    size_t kstride;      // amplitudes between consecutive save points (grid.y covers b_count * n_k states)
    const double2* phi;  // targets
    double* out;         // the Overlap block of expect_out (ExpectRows, plan.hpp): [2 * n_ov][n_tsave][B]
    int n_ov, ov_batch, n_tsave, k0, B, b_first, b_count;
    uint32_t dim;
};

// grid (blocks, b_count * n_k); one atomic per block and row
template <int NO>
__global__ __launch_bounds__(256) void k_overlap_expect(OverlapExpectArgs a) {
    __shared__ double lds[8];
    const int b = a.b_first + int(blockIdx.y) % a.b_count;
    const int kk = int(blockIdx.y) / a.b_count;
    const double2* __restrict__ psi = a.psi + size_t(kk) * a.kstride + size_t(b) * a.dim;
    const double2* __restrict__ phi = a.phi + (a.ov_batch > 1 ? size_t(b) * a.dim : size_t(0));
    const size_t ostride = size_t(a.ov_batch) * a.dim;
    double re[NO], im[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) re[o] = im[o] = 0.0;
    for (uint32_t y = blockIdx.x * 256u + threadIdx.x; y < a.dim; y += gridDim.x * 256u) {
        const double2 v = psi[y];
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (o < a.n_ov) {  // uniform
                const double2 t = phi[size_t(o) * ostride + y];
                re[o] = fma(t.x, v.x, fma(t.y, v.y, re[o]));   // conj(phi) * psi
                im[o] = fma(t.x, v.y, fma(-t.y, v.x, im[o]));
            }
        }
    }
    double* out = a.out + size_t(a.k0 + kk) * a.B + b;
    const size_t row = size_t(a.n_tsave) * a.B;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        if (o < a.n_ov) {
            block_atomic_add(re[o], out + size_t(2 * o) * row, lds);
            block_atomic_add(im[o], out + size_t(2 * o + 1) * row, lds);
        }
    }
}

struct OverlapApplyArgs {
    const double2* base;  // [n_k][B][dim]: what the overlap cotangent is added to (the Pauli cotangent, grad_states from k0 on), or nullptr
    double2* out;         // [n_k][B][dim]; may be `base`
    const double2* phi;   // targets
    const double* gexp;   // the Overlap block of grad_expect (ExpectRows, plan.hpp): [2 * n_ov][n_tsave][B]
    int n_ov, ov_batch, n_tsave, k0, B;
    uint32_t dim;
};

// grid (dim / 256, B, n_k): out[kk][b][y] = base[kk][b][y] + sum_o (g[2o][k][b] + i g[2o+1][k][b]) * phi_{o,b}[y],  k = k0 + kk
__global__ __launch_bounds__(256) void k_overlap_apply(OverlapApplyArgs a) {
    const uint32_t y = blockIdx.x * 256u + threadIdx.x;
    if (y >= a.dim) return;
    const int b = blockIdx.y, k = a.k0 + int(blockIdx.z);
    const size_t off = (size_t(blockIdx.z) * a.B + b) * a.dim + y;
    const size_t row = size_t(a.n_tsave) * a.B;
    const double* g = a.gexp + size_t(k) * a.B + b;
    const double2* phi = a.phi + (a.ov_batch > 1 ? size_t(b) * a.dim : size_t(0)) + y;
    const size_t ostride = size_t(a.ov_batch) * a.dim;
    double2 acc = a.base ? a.base[off] : make_double2(0.0, 0.0);
    bool any = false;
    for (int o = 0; o < a.n_ov; ++o) {
        const double gr = g[size_t(2 * o) * row], gi = g[size_t(2 * o + 1) * row];
        if (gr == 0.0 && gi == 0.0) continue;  // uniform: cotangents usually sit at one or a few save points
        const double2 t = phi[size_t(o) * ostride];
        acc.x = fma(gr, t.x, fma(-gi, t.y, acc.x));
        acc.y = fma(gr, t.y, fma(gi, t.x, acc.y));
        any = true;
    }
    if (!any && a.base == a.out) return;  // (uniform) nothing to add in place
    a.out[off] = acc;
}
