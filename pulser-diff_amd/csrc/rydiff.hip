// rydiff.hip — MI355X (gfx950, wave64) kernels + the C ABI declared in include/rydiff.h.
//
// The hot path of pulser_diff.backend.TorchEmulator (pulser_diff/backend.py:488-494 calling
// pulser_diff/hamiltonian.py:526-546 on every solver sub-step) re-designed matrix-free:
//
//   K0 k_expand_coeffs   per-exponential effective coefficients from the sampled tables (hamiltonian.py:532-542)
//   K1 k_factor_*        y = gamma*x + beta*H(t)x : one factor of the product-form propagator (never builds H)
//   K2 k_expect_diag     <psi|O|psi> for diagonal O (utils.py:79-81), wave-shuffle + LDS reduction
//   K3 k_factor_bwd_*    adjoint of K1 fused with the gradient contractions (replaces the autograd tape, derivative.py:40,76)
//   K4 k_inject          cotangent injection  lambda += grad_states + 2*ge*O*psi
//   K5 k_scatter_grads   per-exponential coefficient gradients -> table / tsave gradients
//   K6 k_build_udiag / k_ugrad   static interaction diagonal (hamiltonian.py:333-344,368-404) and its gradient
//
// No H matrix, no sparse algebra, no accumulator vectors: every factor pass reads the state once and writes it once.
//
// This file: the C ABI and the forward / adjoint sweeps that choose between the kernel families; the kernels (*_kernels.hpp) and
// each family's launch code (*_launch.hpp, runtime.hpp for what they share) are included below (file map: README.md).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/rydiff.h"
#include "plan.hpp"
#include "poly.hpp"

using namespace rydiff;

#include "common.hpp"
#include "direct_kernels.hpp"
#include "xy_kernels.hpp"
#include "chain_kernels.hpp"
#include "pair_kernels.hpp"
#include "persist_kernels.hpp"
#include "lane_kernels.hpp"
#include "pauli_kernels.hpp"
#include "overlap_kernels.hpp"
#include "rdm_kernels.hpp"
#include "moments_kernels.hpp"
#include "energy_kernels.hpp"
#include "shots_kernels.hpp"
#include "dm_kernels.hpp"
#include "tangent_kernels.hpp"
#include "gram_kernels.hpp"
#include "fisher_kernels.hpp"
static_assert(sizeof(PersistFactor) == 48, "plan.hpp sizes the factor table with 48 bytes per entry");

#include "runtime.hpp"
#include "pauli_launch.hpp"
#include "direct_launch.hpp"
#include "xy_launch.hpp"
#include "chain_launch.hpp"
#include "pair_launch.hpp"
#include "shots_launch.hpp"
#include "rdm_launch.hpp"
#include "moments_launch.hpp"
#include "energy_launch.hpp"
#include "dm_launch.hpp"
#include "overlap_launch.hpp"
#include "tangent_launch.hpp"
#include "gram_launch.hpp"
#include "fisher_launch.hpp"
#include "persist_launch.hpp"

namespace {

// RydPlanInfo.kernel_fwd / kernel_bwd: the instantiations launch_chain / launch_factor / the one-launch sweeps will pick for this
// problem (same tests as there), spelled the way rocprofv3 prints them.  Reporting only.
void describe_kernels(const Runtime& rt, const RydProblem* p, bool backward, RydPlanInfo* info) {
    const Plan& pl = rt.pl;
    auto b = [](bool v) { return v ? "true" : "false"; };
    info->kernel_fwd[0] = info->kernel_bwd[0] = 0;
    if (info->kernel_family == 3) {
        const bool pairs = pl.tape_mode != 3 && xcd_group_size(rt, false) == 0 && pair_enabled(rt);
        const bool pairs_bwd = xcd_group_size(rt, true) == 0 && pair_bwd_enabled(rt);
        const bool fast = pl.ga.n == 1 && (pl.ga.amp_index_mask[0] & ((1u << pl.NL) - 1u)) == (1u << pl.NL) - 1u && !pl.ga.flagged;
        for (int bwd = 0; bwd <= (backward ? 1 : 0); ++bwd) {
            const bool cplx = (rt.flags & 1) != 0 || (bwd && !p->real_amp_grad);
            const int lgt = rt.variant == 0 ? ((bwd && cplx) ? 9 : 10) : rt.chain_lgt;
            const bool res = xcd_group_size(rt, bwd != 0) > 0;
            if (!bwd && pairs && pair_pace_fwd(rt))
                std::snprintf(info->kernel_fwd, sizeof(info->kernel_fwd), "k_chain2<%d,10,true,3,%d>", kTileBits, pair_pace_fwd(rt));
            else if (!bwd && pairs)
                std::snprintf(info->kernel_fwd, sizeof(info->kernel_fwd), "k_chain2<%d,10,%s,%d>", kTileBits, b(pair_vec_major(rt)), pair_through(rt));
            else if (bwd && pairs_bwd && pair_wtape(rt))
                std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_chain2_bwd<%d,10,true,3,false,0,true>", kTileBits);
            else if (bwd && pairs_bwd && pair_pace_bwd(rt))
                std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_chain2_bwd<%d,10,true,3,false,%d>", kTileBits, pair_pace_bwd(rt));
            else if (bwd && pairs_bwd)
                std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_chain2_bwd<%d,10,%s,%d,%s>", kTileBits, b(pair_vec_major(rt)),
                              pair_through(rt), b(pair_bwd_dma(rt)));
            else if (chain_geom(rt).lt == kWideTileBits)
                std::snprintf(bwd ? info->kernel_bwd : info->kernel_fwd, sizeof(info->kernel_fwd), "k_chain_wide<%d,%s,%s,%s>", kWideTileBits,
                              b(cplx), b(bwd != 0), b(fast));
            else
                std::snprintf(bwd ? info->kernel_bwd : info->kernel_fwd, sizeof(info->kernel_fwd), "k_chain<%d,%d,%s,%s,%s,%s>", chain_geom(rt).lt,
                              chain_geom(rt).lt == kTileBits ? lgt : 10, b(cplx), b(bwd != 0), b(fast), b(res));
        }
    } else if (info->kernel_family == 2) {
        if (pl.xy_mode) {
            std::snprintf(info->kernel_fwd, sizeof(info->kernel_fwd), "k_factor_xy");
            if (backward) std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_factor_bwd_xy");
        } else if (direct_global_ok(rt)) {
            std::snprintf(info->kernel_fwd, sizeof(info->kernel_fwd), "k_factor_direct_global<%d,%s>", pl.N, b(pl.N <= 13));
            if (backward) std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_factor_bwd_direct_global<%d,%s>", pl.N, b(pl.N <= 13));
        } else {
            std::snprintf(info->kernel_fwd, sizeof(info->kernel_fwd), "k_factor_direct");
            if (backward) std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_factor_bwd_direct");
        }
    } else {
        std::snprintf(info->kernel_fwd, sizeof(info->kernel_fwd), info->kernel_family == 0 ? "k_lanes_fwd (N=%d)" : "k_persist<%d,...>", pl.N);
        // (12 qubits, more than kPersistGroups groups, or an interval of more than kStageChunk factors without the lanes' full tape:
        // the launch-per-factor adjoint reads what the one-launch forward sweep left)
        if (backward && persist_bwd_enabled(rt))
            std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), info->kernel_family == 0 ? "k_lanes_bwd (N=%d)" : "k_persist_bwd<%d,...>", pl.N);
        else if (backward && direct_global_ok(rt))
            std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_factor_bwd_direct_global<%d,%s>", pl.N, b(pl.N <= 13));
        else if (backward)
            std::snprintf(info->kernel_bwd, sizeof(info->kernel_bwd), "k_factor_bwd_direct");
    }
}

// ---- format of the full workspace tape -------------------------------------------------------------------------------------
// Which of the two mid-block entries (pair_wtape, pair_launch.hpp) the last rydiff_forward call wrote into the full tape of a
// workspace: kept here, by workspace address, and not among the bytes of the workspace, which the library never reads back on
// the host.  Only the workspaces that hold P_X v are listed; every forward call that writes a full tape updates its entry.
std::mutex g_tape_format_mutex;
std::vector<const void*> g_wtape_workspaces;

void tape_format_record(const void* workspace, bool wtape) {
    std::lock_guard<std::mutex> lk(g_tape_format_mutex);
    auto it = std::find(g_wtape_workspaces.begin(), g_wtape_workspaces.end(), workspace);
    if (wtape && it == g_wtape_workspaces.end()) g_wtape_workspaces.push_back(workspace);
    else if (!wtape && it != g_wtape_workspaces.end()) g_wtape_workspaces.erase(it);
}

bool tape_format_wtape(const void* workspace) {
    std::lock_guard<std::mutex> lk(g_tape_format_mutex);
    return std::find(g_wtape_workspaces.begin(), g_wtape_workspaces.end(), workspace) != g_wtape_workspaces.end();
}

// ---- forward sweeps (launch per factor; the one-launch sweep: persist_launch.hpp) ------------------------------------------
// <psi|O|psi> of the state at save point k, where no factor launch reduces it on the way
int launch_expect(const ForwardCtx& c, const double2* psi, int k) {
    const Plan& pl = c.rt.pl;
    const unsigned red_blocks = unsigned(std::min<size_t>((pl.dim + 255) / 256, 1024));
    hipLaunchKernelGGL(k_expect_diag, dim3(red_blocks, pl.B), dim3(256), 0, c.stream, psi, c.obs, c.expect_out, pl.n_obs, pl.T + 1, k, pl.B,
                       uint32_t(pl.dim), c.rt.obs_bstride());
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

// where the value rows of a sweep go (ExpectRows, plan.hpp), cleared: the reductions add into them
int bind_expect_rows(ForwardCtx& c, double* expect_out) {
    const Plan& pl = c.rt.pl;
    const ExpectRows rows(pl);
    c.obs = c.p->obs_diag;
    c.expect_out = expect_out;
    c.want_exp = expect_out && pl.n_obs > 0;
    c.pauli_out = rows.at(expect_out, ExpectRows::Pauli);
    c.overlap_out = rows.at(expect_out, ExpectRows::Overlap);
    c.rdm_out = rows.at(expect_out, ExpectRows::Rdm);
    c.moments_out = rows.at(expect_out, ExpectRows::Moments);
    c.energy_out = rows.at(expect_out, ExpectRows::Energy);
    c.dm_out = rows.at(expect_out, ExpectRows::DmTrace, ExpectRows::End);
    if (expect_out && rows.total()) HIP_TRY(hipMemsetAsync(expect_out, 0, rows.size() * sizeof(double), c.stream));
    return RYDIFF_OK;
}

// chained tile passes: one chain over the whole run: factor i of step k; complete outputs at step ends go to the tape
int forward_chained(const ForwardCtx& c) {
    const Runtime& rt = c.rt;
    const Plan& pl = rt.pl;
    const size_t sv = c.sv;
    hipStream_t stream = c.stream;
    std::vector<ChainItem> all, chain;
    std::vector<int> step_of_end;  // for factor i: k+1 if it ends step k, else 0
    std::vector<int64_t> b_entry;  // partial tape: region-B entry of factor i's output, -1: not kept
    for (int k = 0; k < pl.T; ++k) {
        build_step_chain(rt, k, chain);
        for (size_t i = 0; i < chain.size(); ++i) {
            all.push_back(chain[i]);
            step_of_end.push_back(i + 1 == chain.size() ? k + 1 : 0);
            if (c.partial_tape()) b_entry.push_back((k >= c.tmap.k0 && i + 1 < chain.size()) ? c.tmap.bprefix[k] + int64_t(i) : -1);
        }
    }
    const int grp = xcd_group_size(rt, false);
    for (int b0 = 0; b0 < pl.B; b0 += (grp ? grp : pl.B)) {
        const BatchSlice bs{b0, std::min(grp ? grp : pl.B, pl.B - b0), grp > 0};
        int flip = 0;
        auto dst = [&](int i) -> double2* {
            if (c.full_tape()) return c.tape + size_t(i + 1) * sv;  // entry g = output of global factor g (entry 0 = psi0)
            if (step_of_end[i] && c.tape) return c.tape + size_t(step_of_end[i]) * sv;
            if (c.partial_tape() && b_entry[i] >= 0) return c.tape_b + size_t(b_entry[i]) * sv;
            if (bs.xcd) return c.buf[0];  // rewritten in place: the trajectory's lines stay in its XCD's L2
            flip ^= 1;
            return c.buf[flip];
        };
        auto done = [&](int i, const double2* out) -> int {
            if (c.final_dst && step_of_end[i] == pl.T)
                HIP_TRY(hipMemcpyAsync(c.final_dst + size_t(bs.first) * pl.dim, out + size_t(bs.first) * pl.dim,
                                       size_t(bs.count) * pl.dim * sizeof(double2), hipMemcpyDeviceToDevice, stream));
            if (c.copy_out && step_of_end[i])
                HIP_TRY(hipMemcpyAsync(c.copy_out + size_t(step_of_end[i]) * sv + size_t(bs.first) * pl.dim, out + size_t(bs.first) * pl.dim,
                                       size_t(bs.count) * pl.dim * sizeof(double2), hipMemcpyDeviceToDevice, stream));
            if (step_of_end[i]) return launch_observables_expect(c, out, 0, step_of_end[i], 1, bs);
            return RYDIFF_OK;
        };
        auto exp_slot = [&](int i, ChainStep& cs) {
            if (c.want_exp && step_of_end[i]) {  // the pass that completes a step's last factor also reduces <O>
                cs.obs = c.obs;
                cs.n_obs = pl.n_obs;
                cs.exp_ostride = long(pl.T + 1) * pl.B;
                cs.expect_slot = c.expect_out + size_t(step_of_end[i]) * pl.B;
            }
        };
        const int rc = (!c.partial_tape() && !bs.xcd && pair_enabled(rt))
                           ? run_chain2(rt, c.ws, all, c.start, dst, c.full_tape(), c.wtape, done, exp_slot, bs, stream)
                           : run_chain(rt, c.ws, all, c.start, dst, done, exp_slot, false, bs, stream);
        if (rc) return rc;
    }
    return RYDIFF_OK;
}

// one launch per factor of the one-amplitude-per-thread kernels
int forward_direct(const ForwardCtx& c) {
    const Runtime& rt = c.rt;
    const Plan& pl = rt.pl;
    const size_t sv = c.sv;
    std::vector<ChainItem> chain;
    const double2* cur = c.start;
    int pp = 0;
    bool exp_fused = false;
    size_t gfac = 0;  // global factor index: with the full tape entry g + 1 = output of factor g (entry 0 = psi0)
    for (int k = 0; k < pl.T; ++k) {
        build_step_chain(rt, k, chain);
        for (size_t i = 0; i < chain.size(); ++i, ++gfac) {
            const bool last = (i + 1 == chain.size());
            double2* dst;
            if (c.full_tape() && c.tape) dst = c.tape + (gfac + 1) * sv;
            else if (last && c.tape) dst = c.tape + size_t(k + 1) * sv;
            else if (c.partial_tape() && k >= c.tmap.k0) dst = c.tape_b + size_t(c.tmap.bprefix[k] + int64_t(i)) * sv;
            else {
                dst = c.buf[pp];
                if (dst == cur) dst = c.buf[pp ^ 1];
                pp ^= 1;
            }
            const bool want_here = c.want_exp && last;  // the launch that completes the step also reduces <O> where it can
            int rc = shard_signal(rt, 0, cur);  // sharded: partners need `cur` ...
            if (!rc) rc = shard_signal(rt, 1, nullptr);  // ... and this launch reads theirs
            if (rc) return rc;
            rc = launch_factor(rt, c.ws, cur, dst, chain[i].stage, chain[i].s, c.stream, want_here ? c.obs : nullptr,
                               want_here ? c.expect_out + size_t(k + 1) * pl.B : nullptr, &exp_fused);
            if (rc) return rc;
            cur = dst;
        }
        if (c.copy_out) HIP_TRY(hipMemcpyAsync(c.copy_out + size_t(k + 1) * sv, cur, pl.state_bytes, hipMemcpyDeviceToDevice, c.stream));
        if (c.want_exp && !exp_fused) {
            const int rc = launch_expect(c, cur, k + 1);
            if (rc) return rc;
        }
        if (const int rc = launch_observables_expect(c, cur, 0, k + 1, 1, BatchSlice{0, pl.B, false})) return rc;
    }
    if (c.final_dst) HIP_TRY(hipMemcpyAsync(c.final_dst, cur, pl.state_bytes, hipMemcpyDeviceToDevice, c.stream));
    return RYDIFF_OK;
}

// ---- adjoint sweep, launch per factor (the one-launch sweep: persist_launch.hpp) ------------------------------------------
// The inputs x_0 .. x_{M-1} of the factors `chain` of intervals k .. k_hi: on the tape, or recomputed into the chain buffers.
int gather_factor_inputs(const BackwardCtx& c, const BatchSlice& bs, int k, int k_hi, const std::vector<ChainItem>& chain,
                         std::vector<const double2*>& xs) {
    const Runtime& rt = c.rt;
    const int M = int(chain.size());
    const size_t sv = c.sv;
    xs.assign(M + 1, nullptr);
    xs[0] = c.state_at(k);
    xs[M] = c.state_at(k_hi + 1);
    if (c.full_tape()) {
        for (int i = 1; i < M; ++i) xs[i] = c.tape + size_t(c.fprefix[k] + i) * sv;  // every factor input is on the tape
    } else if (c.taped(k_hi)) {  // partial tape: interval kk's first input is its save-point state, the others sit in region B
        int i = 0;
        for (int kk = k; kk <= k_hi; ++kk) {
            const int mk = int(c.fprefix[kk + 1] - c.fprefix[kk]);
            for (int j = 0; j < mk; ++j, ++i) xs[i] = j == 0 ? c.state_at(kk) : c.tape_b + size_t(c.tmap.bprefix[kk] + j - 1) * sv;
        }
    } else if (M - 1 > rt.pl.chain_slots) {
        return fail(RYDIFF_EWORKSPACE, "internal: chain buffers too small");
    } else if (chain_enabled(rt) && M > 1) {
        for (int i = 1; i < M; ++i) xs[i] = c.chainbuf + size_t(i - 1) * sv;
        auto dst = [&](int i) -> double2* { return c.chainbuf + size_t(i) * sv; };
        auto done = [&](int, const double2*) -> int { return RYDIFF_OK; };
        auto no_exp = [&](int, ChainStep&) {};
        return run_chain(rt, c.ws, chain, xs[0], dst, done, no_exp, true, bs, c.stream);
    } else {
        for (int i = 1; i < M; ++i) {
            double2* dst = c.chainbuf + size_t(i - 1) * sv;
            int rc = shard_signal(rt, 0, xs[i - 1]);  // (sharded recompute: the partners need this factor input, this launch theirs)
            if (!rc) rc = shard_signal(rt, 1, nullptr);
            if (rc) return rc;
            rc = launch_factor(rt, c.ws, xs[i - 1], dst, chain[i - 1].stage, chain[i - 1].s, c.stream);
            if (rc) return rc;
            xs[i] = dst;
        }
    }
    return RYDIFF_OK;
}

// g_hi: the run-wide index of the last forward block of `chain` (read with P_X v on the tape only, run_chain2_bwd)
int adjoint_chained(const BackwardCtx& c, const BatchSlice& bs, const std::vector<ChainItem>& chain, const std::vector<const double2*>& xs,
                    const std::vector<int>& save_k, int64_t g_hi, int& cl) {
    const Runtime& rt = c.rt;
    double2* lam[2] = {c.lam[0], c.lam[1]};
    auto dot_h = [&](int stage, const double2* g, const double2* xout) -> int {
        return c.want_tau ? launch_dot_h(rt, c.ws, stage, g, xout, bs, c.stream) : RYDIFF_OK;
    };
    // sharded: dot_h reads the partners' copies of the cotangent it is handed, like the completing launch that follows it
    if (c.wtape && (bs.xcd || !pair_bwd_enabled(rt))) return fail(RYDIFF_EINVAL, "internal: P_X v on the tape without the block adjoint");
    return (!bs.xcd && pair_bwd_enabled(rt)) ? run_chain2_bwd(rt, c.ws, chain, xs, save_k, lam[cl], lam, cl, c.wtot, dot_h, bs, c.inj, c.wtape, g_hi, c.stream)
                                             : run_chain_bwd(rt, c.ws, chain, xs, save_k, lam[cl], lam, cl, c.wtot, dot_h, c.want_tau, bs, c.inj, c.stream);
}

int adjoint_direct(const BackwardCtx& c, const BatchSlice& bs, const std::vector<ChainItem>& chain, const std::vector<const double2*>& xs,
                   const std::vector<int>& save_k, int& cl) {
    const Runtime& rt = c.rt;
    const int M = int(chain.size());
    for (int i = M; i >= 1; --i) {
        const ChainItem& it = chain[i - 1];
        int rc = shard_signal(rt, 0, c.lam[cl]);  // sharded: the partners need this rank's cotangent ...
        if (!rc) rc = shard_signal(rt, 1, nullptr);  // ... and the launches below read theirs
        if (rc) return rc;
        // dL/dtau of an exponential is taken at its output (end of its last factor); sharded: with the partners' cotangent slabs
        if (c.want_tau && (i == M || chain[i].stage != it.stage)) {
            rc = launch_dot_h(rt, c.ws, it.stage, c.lam[cl], xs[i], bs, c.stream);
            if (rc) return rc;
        }
        rc = launch_factor_bwd(rt, c.ws, c.lam[cl], xs[i - 1], c.lam[cl ^ 1], it.stage, it.s, c.wtot, c.inj, save_k[i - 1], c.stream);
        if (rc) return rc;
        cl ^= 1;
    }
    return RYDIFF_OK;
}

// The reverse sweep over the trajectories of `bs`, from the cotangent at the final time in c.lam[0]; the cotangent w.r.t. psi0 ends
// up in c.lam[cl].  The cotangents of the earlier save points are added by the launch that completes the adjoint state there.
int adjoint_sweep(const BackwardCtx& c, const BatchSlice& bs, int& cl) {
    const Runtime& rt = c.rt;
    const Plan& pl = rt.pl;
    const bool chained = chain_enabled(rt);
    std::vector<ChainItem> chain, part;
    std::vector<const double2*> xs;
    std::vector<int> save_k;
    std::vector<int64_t> bprefix(pl.T + 1, 0);  // forward blocks before interval k (as fprefix counts factors)
    if (c.wtape)
        for (int k = 0; k < pl.T; ++k) bprefix[k + 1] = bprefix[k] + step_block_count(rt, k);
    cl = 0;
    for (int k = pl.T - 1; k >= 0; --k) {
        // With every factor input on the tape, consecutive intervals run as ONE chain: the launch that finishes the adjoint
        // of interval k's first factor (and adds the cotangent injected at save point k) also starts interval k-1's last one.
        const int k_hi = k;
        if (c.taped(k_hi) && chained) {
            while (k > 0 && c.taped(k - 1) && c.fprefix[k_hi + 1] - c.fprefix[k - 1] < (int64_t(1) << 16)) --k;
        }
        chain.clear();
        save_k.clear();
        for (int kk = k; kk <= k_hi; ++kk) {
            build_step_chain(rt, kk, part);
            for (size_t i = 0; i < part.size(); ++i) save_k.push_back(i == 0 ? kk : -1);
            chain.insert(chain.end(), part.begin(), part.end());
        }
        int rc = gather_factor_inputs(c, bs, k, k_hi, chain, xs);
        if (!rc) rc = chained ? adjoint_chained(c, bs, chain, xs, save_k, bprefix[k_hi + 1] - 1, cl) : adjoint_direct(c, bs, chain, xs, save_k, cl);
        if (rc) return rc;
    }
    return RYDIFF_OK;
}

// per-exponential gradient records -> table / tsave gradients; interaction weights -> g_u
int scatter_gradients(const BackwardCtx& c, void* g_amp, double* g_det, double* g_u, double* g_tsave) {
    const Plan& pl = c.rt.pl;
    hipStream_t stream = c.stream;
    const size_t E = pl.stages.size();
    if (g_amp) HIP_TRY(hipMemsetAsync(g_amp, 0, size_t(pl.Bc) * pl.Ka * pl.n_samples * 16, stream));
    if (g_det) HIP_TRY(hipMemsetAsync(g_det, 0, size_t(pl.Bc) * pl.Kd * pl.n_samples * 8, stream));
    if (g_tsave) HIP_TRY(hipMemsetAsync(g_tsave, 0, size_t(pl.T + 1) * 8, stream));
    if ((g_amp && pl.Ka) || (g_det && pl.Kd) || g_tsave) {
        char* m = c.ws + pl.off_meta2;  // (the save-point flags of the one-launch adjoint, which share the region, are dead by now)
        if (g_tsave) {
            std::vector<StageBwdDev> sb(E);
            for (size_t e = 0; e < E; ++e) {
                const Stage& st = pl.stages[e];
                sb[e] = {st.tau_scale, st.tnw[0], st.tnw[1], st.tn[0], st.tn[1], st.t_hi, st.t_lo};
            }
            const int rc = upload_words(stream, m, sb.data(), E * sizeof(StageBwdDev));
            if (rc) return rc;
        }
        ScatterArgs sa{};
        sa.ge = c.ge;
        sa.st = reinterpret_cast<const StageDev*>(c.ws + pl.off_meta_idx);
        sa.sb = reinterpret_cast<const StageBwdDev*>(m);
        sa.inv_dt = pl.dt > 0.0 ? 1.0 / pl.dt : 0.0;
        sa.amp = static_cast<const double2*>(c.p->amp_tables);
        sa.det = c.p->det_tables;
        sa.g_amp = static_cast<double2*>(g_amp);
        sa.g_det = g_det;
        sa.g_tsave = g_tsave;
        sa.E = int(E);
        sa.n_samples = pl.n_samples;
        sa.Ka = pl.Ka;
        sa.Kd = pl.Kd;
        sa.NC = pl.NC;
        sa.ga = pl.ga.n;
        sa.gd = pl.gd.n;
        for (int g = 0; g < pl.ga.n; ++g) sa.amem[g] = pl.ga.members[g];
        for (int g = 0; g < pl.gd.n; ++g) sa.dmem[g] = pl.gd.members[g];
        hipLaunchKernelGGL(k_scatter_grads, dim3((unsigned(E) + 63) / 64, pl.Bc), dim3(64), 0, stream, sa);
        LAUNCH_CHECK();
    }
    const int npairs = pl.N * (pl.N - 1) / 2;
    if (g_u && npairs > 0) {
        HIP_TRY(hipMemsetAsync(g_u, 0, size_t(npairs) * 8, stream));
        const unsigned nb = unsigned(std::min<size_t>((pl.dim + 255) / 256, 256));
        hipLaunchKernelGGL(k_ugrad, dim3(nb, npairs), dim3(256), 0, stream, g_u, c.wtot, pl.N, uint32_t(pl.dim), pl.shard_bits ? pl.B : 0, pl.NL,
                           pl.rank_first);
        LAUNCH_CHECK();
    }
    return xy_contract(c.rt, c.p->g_xy, stream);  // (the exchange gradient: its replicas -> g_xy)
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* rydiff_last_error(void) { return g_last_error.c_str(); }
const char* rydiff_version(void) { return "rydiff 0.4 (gfx950)"; }
size_t rydiff_sizeof_problem(void) { return sizeof(RydProblem); }
size_t rydiff_sizeof_plan_info(void) { return sizeof(RydPlanInfo); }
size_t rydiff_sizeof_tangent(void) { return sizeof(RydTangent); }

#ifdef RYDIFF_TIMELINE
int rydiff_debug_timeline(unsigned long long* host_buf, int n_entries) {  // tuning builds only
    return hipMemcpyFromSymbol(host_buf, HIP_SYMBOL(g_timeline), size_t(n_entries) * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

int rydiff_design_polynomial(double rho, double tol, int max_degree, int* degree, double* roots_reim, double* p0_reim, double* max_err) {
    if (!(rho > 0.0) || !degree || !roots_reim || max_degree < 1) return fail(RYDIFF_EINVAL, "bad arguments");
    PolyDesign d = design_polynomial(rho, tol, max_degree);
    if (d.degree < 1) return fail(RYDIFF_EINVAL, "polynomial design failed");
    *degree = d.degree;
    for (int i = 0; i < d.degree; ++i) {
        roots_reim[2 * i] = d.roots[i].real();
        roots_reim[2 * i + 1] = d.roots[i].imag();
    }
    if (p0_reim) {
        p0_reim[0] = d.p0.real();
        p0_reim[1] = d.p0.imag();
    }
    if (max_err) *max_err = d.max_err;
    return RYDIFF_OK;
}

int rydiff_plan(const RydProblem* p, int need_tape, int need_backward, void* scratch, void* stream_, RydPlanInfo* info) {
    if (!p) return fail(RYDIFF_EINVAL, "null problem");
    if (!info || !scratch) return fail(RYDIFF_EINVAL, "null info or scratch");
    if (need_tape < 0 || need_tape > 3) return fail(RYDIFF_EINVAL, "need_tape must be 0..3");
    Runtime rt;
    double lo, hi;
    size_t ws;
    const int rc = plan_runtime(p, nullptr, scratch, RYDIFF_PLAN_SCRATCH_BYTES, need_tape, need_backward != 0, static_cast<hipStream_t>(stream_),
                                rt, lo, hi, ws);
    if (rc) return rc;
    info->spectral_lo = lo;
    info->spectral_hi = hi;
    info->rho_design = rt.rho_design;
    info->degree = rt.poly.degree;
    info->n_stages = int(rt.pl.stages.size());
    info->max_step_factors = rt.max_step_factors;
    info->flags = rt.flags;
    info->total_factors = rt.total_factors;
    info->workspace_bytes = ws;
    info->tape_mode = need_tape;  // (as granted)
    if (persist_enabled(rt)) info->kernel_family = lanes_enabled(rt) ? 0 : 1;
    else info->kernel_family = chain_enabled(rt) ? 3 : 2;
    describe_kernels(rt, p, need_backward != 0, info);
    return RYDIFF_OK;
}

int rydiff_forward(const RydProblem* p, const RydPlanInfo* info, const void* psi0, void* states_out, double* expect_out,
                   void* workspace, size_t workspace_bytes, int need_tape, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!psi0) return fail(RYDIFF_EINVAL, "null psi0");
    Runtime rt;
    // need_tape = 2 together with states_out: the caller wants the stored states AND a gradient later — where the full tape is
    // granted the factor outputs go to the workspace tape and the states at the save points are copied out of it
    int rc = prepare(p, info, workspace, workspace_bytes, need_tape >= 2 ? need_tape : (states_out ? 0 : need_tape), false, stream, rt);
    if (rc) return rc;
    const Plan& pl = rt.pl;
    ForwardCtx c{{rt, p, static_cast<char*>(workspace), stream, size_t(pl.B) * pl.dim}};
    c.psi0 = c.start = static_cast<const double2*>(psi0);
    c.buf[0] = reinterpret_cast<double2*>(c.ws + pl.off_buf0);
    c.buf[1] = reinterpret_cast<double2*>(c.ws + pl.off_buf1);
    if (c.partial_tape()) c.tmap = partial_tape_map(rt, p->tape_steps);
    const bool ws_tape = c.full_tape() || c.partial_tape();  // (prepare downgrades the request where such a tape is not possible)
    if (c.full_tape()) {  // the mid-block entries of the tape this call writes: chosen here, recorded for the backward call
        c.wtape = pair_wtape(rt);
        tape_format_record(workspace, c.wtape);
    }
    double2* sout = static_cast<double2*>(states_out);
    // final_state_only: no per-step states; the state at the last evaluation time is copied to states_out at the end
    if (p->final_state_only && sout) {
        if (need_tape || persist_enabled(rt))
            return fail(RYDIFF_EINVAL, "final_state_only needs the launch-per-factor kernels (more than 12 qubits or a sharded run) and no tape");
        c.final_dst = sout;
        sout = nullptr;
    }
    c.tape = (sout && !ws_tape) ? sout : (pl.tape_mode ? reinterpret_cast<double2*>(c.ws + pl.off_tape) : nullptr);
    c.copy_out = ws_tape ? sout : nullptr;  // states at the save points, copied from the workspace tape
    c.tape_b = c.partial_tape() ? c.tape + size_t(pl.T + 1) * c.sv : nullptr;
    if (c.tape) {
        HIP_TRY(hipMemcpyAsync(c.tape, psi0, pl.state_bytes, hipMemcpyDeviceToDevice, stream));
        c.start = c.tape;
    }
    if (c.copy_out) HIP_TRY(hipMemcpyAsync(c.copy_out, psi0, pl.state_bytes, hipMemcpyDeviceToDevice, stream));
    if (pl.n_shots) {  // drawn wherever launch_observables_expect sees a sampled save point
        c.shot_u = p->shot_uniforms;
        c.shots_out = p->shots_out;
    }
    rc = bind_expect_rows(c, expect_out);
    if (rc) return rc;
    if (c.want_exp) {
        rc = launch_expect(c, c.start, 0);
        if (rc) return rc;
    }
    if (persist_enabled(rt)) return forward_persist(c);  // (evaluates the Pauli / overlap / reduced-density-matrix observables and draws the shots on the whole trajectory afterwards)
    rc = launch_observables_expect(c, c.start, 0, 0, 1, BatchSlice{0, pl.B, false});
    if (rc) return rc;
    return chain_enabled(rt) ? forward_chained(c) : forward_direct(c);
}

int rydiff_backward(const RydProblem* p, const RydPlanInfo* info, const void* states, const void* grad_states,
                    const double* grad_expect, void* g_amp, double* g_det, double* g_u, double* g_tsave, void* g_psi0,
                    void* workspace, size_t workspace_bytes, int need_tape, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!states && !need_tape) return fail(RYDIFF_EINVAL, "backward needs the trajectory: pass states or use the workspace tape");
    Runtime rt;
    int rc = prepare(p, info, workspace, workspace_bytes, need_tape >= 2 ? need_tape : (states ? 0 : need_tape), true, stream, rt);
    if (rc) return rc;
    const Plan& pl = rt.pl;
    if (!states && !pl.tape_mode) return fail(RYDIFF_EINVAL, "backward needs the trajectory: pass states or use the workspace tape");
    if (pl.xy_mode && p->g_xy && pl.N > 1) {  // dL/dJ: replicas in the workspace, zeroed here, contracted by scatter_gradients
        rt.xy_ge = reinterpret_cast<double*>(static_cast<char*>(workspace) + pl.off_xy_ge);
        HIP_TRY(hipMemsetAsync(rt.xy_ge, 0, size_t(kXyReplicas) * (pl.N * (pl.N - 1) / 2) * sizeof(double), stream));
    }
    BackwardCtx c{{rt, p, static_cast<char*>(workspace), stream, size_t(pl.B) * pl.dim}};
    // the full workspace tape (written by a forward call with need_tape = 2) is preferred over `states`
    c.tape = (pl.tape_mode >= 2 || !states) ? reinterpret_cast<const double2*>(c.ws + pl.off_tape) : static_cast<const double2*>(states);
    if (c.partial_tape()) {
        c.tmap = partial_tape_map(rt, p->tape_steps);
        c.tape_b = c.tape + size_t(pl.T + 1) * c.sv;
    }
    // the mid-block entries of a full tape are what the forward call recorded, and this call's kernels have to be the ones that read them
    c.wtape = c.full_tape() && tape_format_wtape(workspace);
    if (c.full_tape() && c.wtape != pair_wtape(rt))
        return fail(RYDIFF_EINVAL, c.wtape ? "the full tape in this workspace holds P_X v between the factors of a block (written by a forward call with the "
                                             "block adjoint in view), and this backward call would read it as the mid-block state: use the forward call's kernel_variant and real_amp_grad"
                                           : "the full tape in this workspace holds the mid-block state between the factors of a block, and this backward call "
                                             "expects P_X v there: use the forward call's kernel_variant and real_amp_grad");
    c.fprefix.assign(pl.T + 1, 0);
    for (int k = 0; k < pl.T; ++k) c.fprefix[k + 1] = c.fprefix[k] + step_factor_count(rt, k);
    c.lam[0] = reinterpret_cast<double2*>(c.ws + pl.off_buf0);
    c.lam[1] = reinterpret_cast<double2*>(c.ws + pl.off_buf1);
    c.chainbuf = reinterpret_cast<double2*>(c.ws + pl.off_chain);
    c.ge = rt.ge(c.ws, 0);
    c.wtot = g_u ? reinterpret_cast<double*>(c.ws + pl.off_wtot) : nullptr;
    c.want_tau = g_tsave != nullptr;
    const bool have_gexp = grad_expect && pl.n_obs > 0;
    c.inj.gstate = static_cast<const double2*>(grad_states);
    c.inj.gexp = have_gexp ? grad_expect : nullptr;
    c.inj.obs = p->obs_diag;
    c.inj.n_obs = have_gexp ? pl.n_obs : 0;
    const ExpectRows rows(pl);
    if (grad_expect && rows.total() > rows.count(ExpectRows::Diag)) {  // some row that is not a diagonal observable's
        c.pauli.rt = &rt;
        c.pauli.ws = c.ws;
        c.pauli.stream = stream;
        c.pauli.gstate = c.inj.gstate;
        c.pauli.gexp = rows.at(grad_expect, ExpectRows::Pauli);
        c.pauli.ov_gexp = rows.at(grad_expect, ExpectRows::Overlap);
        c.pauli.ov_targets = static_cast<const double2*>(p->overlap_targets);
        c.pauli.rdm_gexp = rows.at(grad_expect, ExpectRows::Rdm);
        c.pauli.moments_gexp = rows.at(grad_expect, ExpectRows::Moments);
        c.pauli.energy_gexp = rows.at(grad_expect, ExpectRows::Energy);
        c.pauli.wtot = c.wtot;
        c.pauli.dm_gexp = rows.at(grad_expect, ExpectRows::DmTrace, ExpectRows::End);
        c.pauli.dm_diag = p->dm_diag;
        c.pauli.dm_phi = static_cast<const double2*>(p->dm_fid_targets);
        if (pl.n_rdm && (rc = rdm_apply_prepare())) return rc;
        c.pauli.buf = reinterpret_cast<double2*>(c.ws + pl.off_pauli_cot);
        c.pauli.state_at = [&c](int k) { return c.state_at(k); };
        c.inj.pauli = &c.pauli;
    }

    HIP_TRY(hipMemsetAsync(c.ge, 0, size_t(pl.Bc) * pl.stages.size() * rt.ge_rec() * sizeof(double), stream));
    if (c.wtot) HIP_TRY(hipMemsetAsync(c.wtot, 0, pl.dim * (pl.shard_bits ? size_t(pl.B) : 1) * sizeof(double), stream));
    rc = energy_clear_gradients(rt, c.ws, stream);
    if (rc) return rc;
    int cl = 0;  // c.lam[cl]: the cotangent w.r.t. psi0 once the sweep is through
    if (persist_bwd_enabled(rt)) {
        rc = backward_persist(c);
        if (rc) return rc;
    } else {
        // cotangent at the final time; the cotangents of the earlier save points are added by the launch that completes the
        // adjoint state there (fused injection: no separate launches, and no host-side look at grad_expect)
        hipLaunchKernelGGL(k_inject, dim3(unsigned((pl.dim + 255) / 256), pl.B), dim3(256), 0, stream, c.lam[0],
                           c.inj.pauli ? observable_cotangent(c.pauli, pl.T) : (c.inj.gstate ? c.inj.gstate + size_t(pl.T) * c.sv : nullptr), c.state_at(pl.T), c.inj.obs, c.inj.gexp, pl.n_obs,
                           pl.T + 1, pl.T, pl.B, uint32_t(pl.dim), 1, rt.obs_ostride(), rt.obs_bstride());
        LAUNCH_CHECK();
        // chained passes in trajectory-per-XCD placement: every group of trajectories runs its whole sweep before the next one starts
        const int grp = chain_enabled(rt) ? xcd_group_size(rt, true) : 0;
        for (int b0 = 0; b0 < pl.B; b0 += (grp ? grp : pl.B)) {
            rc = adjoint_sweep(c, BatchSlice{b0, std::min(grp ? grp : pl.B, pl.B - b0), grp > 0}, cl);
            if (rc) return rc;
        }
    }
    if (c.pauli.rc) return c.pauli.rc;  // (a cotangent launch failed: rydiff_last_error names it)
    if (g_psi0) HIP_TRY(hipMemcpyAsync(g_psi0, c.lam[cl], pl.state_bytes, hipMemcpyDeviceToDevice, stream));
    rc = scatter_gradients(c, g_amp, g_det, g_u, g_tsave);
    return rc ? rc : energy_scatter(rt, p, c.ws, stream);  // (the explicit dL/d(energy tables); dL/dU and dL/dJ went into wtot / the exchange replicas)
}

size_t rydiff_tangent_workspace_bytes_flags(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags) {
    Runtime rt;
    TangentLayout lay;
    return tangent_plan(p, info, n_dir, flags, rt, lay) ? 0 : lay.total;
}

size_t rydiff_tangent_workspace_bytes(const RydProblem* p, const RydPlanInfo* info, int n_dir) {
    return rydiff_tangent_workspace_bytes_flags(p, info, n_dir, 0);
}

size_t rydiff_geometry_workspace_bytes_flags(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags) {
    Runtime rt;
    TangentLayout lay;
    if (tangent_plan(p, info, n_dir, flags, rt, lay)) return 0;  // (the sweep's refusals first, as in rydiff_forward_geometry)
    if (geometry_validate(p)) return 0;
    return geometry_layout(rt.pl, lay, n_dir).total;
}

size_t rydiff_geometry_workspace_bytes(const RydProblem* p, const RydPlanInfo* info, int n_dir) {
    return rydiff_geometry_workspace_bytes_flags(p, info, n_dir, 0);
}

size_t rydiff_fisher_workspace_bytes_flags(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags) {
    Runtime rt;
    TangentLayout lay;
    if (tangent_plan(p, info, n_dir, flags, rt, lay)) return 0;  // (the refusals of rydiff_forward_geometry, in its order)
    if (geometry_validate(p)) return 0;
    return fisher_layout(rt.pl, geometry_layout(rt.pl, lay, n_dir), n_dir).total;
}

}  // extern "C"

namespace {

// The forward-mode sweep behind rydiff_forward_tangent, rydiff_forward_geometry and rydiff_forward_fisher: the state and n_dir tangents
// through every factor once (tangent_kernels.hpp); at every save point the observable values, their tangents (dexpect_out, skipped when
// NULL), with `geometry` the Gram matrix of the (1 + n_dir) vectors (gram_kernels.hpp) and with `fisher` (which implies `geometry`: its
// refusals and its workspace; gram_out is optional then) their classical Gram matrix (fisher_kernels.hpp).  One kernel family: launch per factor, one amplitude
// per thread; dense pair terms (the dissipator of a master-equation run, the XY exchange) ride in the same pass.  On the doubled
// register of a density matrix (dm_atoms > 0) the vectors are vec(rho) and vec(d rho_d), and the density-matrix rows follow the ket rows.
int tangent_sweep(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tg, const void* psi0, double* expect_out,
                  double* dexpect_out, bool geometry, void* gram_out, bool fisher, double* cgram_out, void* workspace, size_t workspace_bytes,
                  hipStream_t stream) {
    // ---- host-only validation: nothing below this block runs unless all of it passes ----
    if (!p) return fail(RYDIFF_EINVAL, "null problem");
    if (!tg) return fail(RYDIFF_EINVAL, "null tangent");
    int rc = tangent_validate(p, info, tg->n_dir, tg->flags);  // n_dir, the plan, what the sweep does not implement
    if (rc) return rc;
    if (geometry && (rc = geometry_validate(p))) return rc;
    if (tg->d_xy && p->xy_mode == 0) return fail(RYDIFF_EINVAL, "tangent: d_xy given on a problem without the XY exchange (xy_mode = 0)");
    if (!tg->d_amp && !tg->d_det && !tg->d_u && !tg->d_psi0 && !tg->d_xy)
        return fail(RYDIFF_EINVAL, "tangent: all of d_amp, d_det, d_u, d_psi0 are NULL, and so is d_xy (nothing to differentiate)");
    if (!geometry && !dexpect_out) return fail(RYDIFF_EINVAL, "null dexpect_out");
    if (geometry && !fisher && !gram_out) return fail(RYDIFF_EINVAL, "null gram_out");
    if (fisher && !cgram_out) return fail(RYDIFF_EINVAL, "null cgram_out");
    if (!psi0) return fail(RYDIFF_EINVAL, "null psi0");
    Runtime rt0;
    TangentLayout lay;
    rc = tangent_plan(p, info, tg->n_dir, tg->flags, rt0, lay);
    if (rc) return rc;
    GeometryLayout glay;
    if (geometry) glay = geometry_layout(rt0.pl, lay, tg->n_dir);
    FisherLayout flay;
    if (fisher) flay = fisher_layout(rt0.pl, glay, tg->n_dir);
    const size_t need = fisher ? flay.total : (geometry ? glay.total : lay.total);
    if (!workspace) return fail(RYDIFF_EINVAL, "null workspace");
    if (workspace_bytes < need)
        return fail(RYDIFF_EWORKSPACE, std::string(fisher ? "fisher" : (geometry ? "geometry" : "tangent")) + " workspace too small: need " + std::to_string(need) +
                                           " bytes, got " + std::to_string(workspace_bytes));
    // ---- device work ----
    RydProblem q = *p;
    q.kernel_variant = 0;
    Runtime rt;
    rc = prepare(&q, info, workspace, workspace_bytes, 0, false, stream, rt);  // metadata, coefficient records, udiag, Pauli tables
    if (rc) return rc;
    const Plan& pl = rt.pl;
    const int D = tg->n_dir;
    char* ws = static_cast<char*>(workspace);
    rc = tangent_tables(rt, &q, tg, ws, lay, stream);
    if (rc) return rc;
    const size_t sv = size_t(pl.B) * pl.dim;
    double2* vec[2] = {reinterpret_cast<double2*>(ws + lay.off_vec[0]), reinterpret_cast<double2*>(ws + lay.off_vec[1])};
    HIP_TRY(hipMemcpyAsync(vec[0], psi0, pl.state_bytes, hipMemcpyDeviceToDevice, stream));
    const int Dp = tangent_padded(D);  // the kernel's direction count: a padded direction starts at zero and stays there
    if (tg->d_psi0) {
        HIP_TRY(hipMemcpyAsync(vec[0] + sv, tg->d_psi0, size_t(D) * pl.state_bytes, hipMemcpyDeviceToDevice, stream));
        if (Dp > D) HIP_TRY(hipMemsetAsync(vec[0] + size_t(1 + D) * sv, 0, size_t(Dp - D) * pl.state_bytes, stream));
    } else {
        HIP_TRY(hipMemsetAsync(vec[0] + sv, 0, size_t(Dp) * pl.state_bytes, stream));
    }
    const ExpectRows rows(pl);
    if (rows.total() && dexpect_out) HIP_TRY(hipMemsetAsync(dexpect_out, 0, size_t(D) * rows.size() * sizeof(double), stream));
    ForwardCtx c{{rt, &q, ws, stream, sv}};
    c.psi0 = c.start = vec[0];
    rc = bind_expect_rows(c, expect_out);
    if (rc) return rc;
    if (pl.moments && pl.moment_tiles() > 1) c.moments_drec = reinterpret_cast<double*>(ws + lay.off_dmoments);
    auto save_point = [&](const double2* v, int k) -> int {  // values (the existing reductions on psi) and tangents of every row
        if (c.want_exp)
            if (const int r = launch_expect(c, v, k)) return r;
        if (const int r = launch_observables_expect(c, v, 0, k, 1, BatchSlice{0, pl.B, false})) return r;
        if (dexpect_out)
            if (const int r = launch_expect_tangent(c, v, D, k, dexpect_out)) return r;
        if (geometry && gram_out)
            if (const int r = launch_gram(rt, ws, glay, v, D, k, static_cast<double2*>(gram_out), stream)) return r;
        return fisher ? launch_cfi(rt, ws, flay, v, D, k, cgram_out, stream) : RYDIFF_OK;
    };
    rc = save_point(vec[0], 0);
    if (rc) return rc;
    TangentFactorArgs fa{};
    fill_tangent_factor(fa, rt, ws, lay, tg->d_u != nullptr, tg->d_xy != nullptr);
    std::vector<ChainItem> chain;
    int cur = 0;
    for (int k = 0; k < pl.T; ++k) {
        build_step_chain(rt, k, chain);
        for (const ChainItem& it : chain) {
            rc = launch_factor_tangent(fa, rt, ws, lay, D, vec[cur], vec[cur ^ 1], it.stage, it.s, stream);
            if (rc) return rc;
            cur ^= 1;
        }
        rc = save_point(vec[cur], k + 1);
        if (rc) return rc;
    }
    return RYDIFF_OK;
}

}  // namespace

extern "C" {

int rydiff_forward_tangent(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tg, const void* psi0, double* expect_out,
                           double* dexpect_out, void* workspace, size_t workspace_bytes, void* stream_) {
    return tangent_sweep(p, info, tg, psi0, expect_out, dexpect_out, false, nullptr, false, nullptr, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream_));
}

// The same sweep with the Gram matrix of (psi, dpsi_0 .. dpsi_{n_dir - 1}) at every save point; the row tangents are optional here.
int rydiff_forward_geometry(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tg, const void* psi0, double* expect_out,
                            double* dexpect_out, void* gram_out, void* workspace, size_t workspace_bytes, void* stream_) {
    return tangent_sweep(p, info, tg, psi0, expect_out, dexpect_out, true, gram_out, false, nullptr, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream_));
}

// The geometry sweep with the classical Gram matrix of the same vectors (the occupation-basis measurement) at every save point; the
// Gram matrix itself is optional here.
int rydiff_forward_fisher(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tg, const void* psi0, double* expect_out,
                          double* dexpect_out, void* gram_out, double* cgram_out, void* workspace, size_t workspace_bytes, void* stream_) {
    return tangent_sweep(p, info, tg, psi0, expect_out, dexpect_out, true, gram_out, true, cgram_out, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream_));
}

int rydiff_apply_factor(const RydProblem* p, const double* c_amp_reim, const double* c_det, const double* gamma_reim,
                        const double* beta_reim, const void* x, void* y, int n_remote, const void* const* remote,
                        const double* remote_coef_reim, int reuse_diag, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!p) return fail(RYDIFF_EINVAL, "null problem");
    if (!x || !y || !workspace || !gamma_reim || !beta_reim) return fail(RYDIFF_EINVAL, "null buffer");
    if (p->xy_mode != 0) return fail(RYDIFF_ENOTIMPL, "rydiff_apply_factor: not implemented with the XY exchange (xy_mode != 0)");
    if ((p->n_amp_terms > 0 && !c_amp_reim) || (p->n_det_terms > 0 && !c_det))
        return fail(RYDIFF_EINVAL, "missing coefficient values (c_amp_reim / c_det) for the problem's terms");
    if (n_remote < 0 || n_remote > kMaxRemote || (n_remote > 0 && (!remote || !remote_coef_reim)))
        return fail(RYDIFF_EINVAL, "bad remote vector list");
    RydProblem q = *p;
    double dummy_t[2] = {0.0, 1.0};
    if (q.n_tsave < 2 || !q.tsave) {
        q.n_tsave = 2;
        q.tsave = dummy_t;
    }
    q.solver = RYDIFF_SOLVER_KRYLOV_SE;
    Runtime rt;
    std::string err;
    if (!build_plan(&q, rt.pl, err)) return fail(RYDIFF_EINVAL, err);
    Plan& pl = rt.pl;
    if (pl.n_pair) return fail(RYDIFF_ENOTIMPL, "rydiff_apply_factor does not take pair terms");
    fill_group_args(pl, rt.garg);
    const size_t need = align_up(pl.dim * sizeof(double));
    if (workspace_bytes < need) return fail(RYDIFF_EWORKSPACE, "workspace too small: need " + std::to_string(need));
    FactorArgs fa{};
    fa.use_inline = 1;
    for (int g = 0; g < pl.ga.n; ++g)
        for (int k = 0; k < pl.Ka; ++k)
            if (pl.ga.members[g] >> k & 1ull) {
                fa.coef_inline[g] += c_amp_reim[2 * k];
                fa.coef_inline[pl.ga.n + g] += c_amp_reim[2 * k + 1];
            }
    for (int g = 0; g < pl.gd.n; ++g)
        for (int k = 0; k < pl.Kd; ++k)
            if (pl.gd.members[g] >> k & 1ull) fa.coef_inline[2 * pl.ga.n + g] += 2.0 * c_det[k];
    double* udiag = static_cast<double*>(workspace);
    if (!reuse_diag) {
        if (pl.N > 1) {
            hipLaunchKernelGGL(k_build_udiag, dim3((pl.dim + 255) / 256), dim3(256), 0, stream, udiag, p->u_pairs, pl.N, uint32_t(pl.dim));
            LAUNCH_CHECK();
        } else {
            HIP_TRY(hipMemsetAsync(udiag, 0, pl.dim * sizeof(double), stream));
        }
    }
    fa.xin = static_cast<const double2*>(x);
    fa.xout = static_cast<double2*>(y);
    fa.udiag = udiag;
    fa.coef = nullptr;
    fa.coef_bstride = 0;
    fa.dim = uint32_t(pl.dim);
    fa.gr = gamma_reim[0];
    fa.gi = gamma_reim[1];
    fa.br = beta_reim[0];
    fa.bi = beta_reim[1];
    fa.g = rt.garg;
    fa.n_remote = n_remote;
    for (int k = 0; k < n_remote; ++k) {
        fa.remote[k] = static_cast<const double2*>(remote[k]);
        fa.rc[2 * k] = remote_coef_reim[2 * k];
        fa.rc[2 * k + 1] = remote_coef_reim[2 * k + 1];
    }
    hipLaunchKernelGGL(k_factor_direct, dim3(unsigned((pl.dim + 255) / 256), pl.B), dim3(256), 0, stream, fa);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

int rydiff_apply_hamiltonian(const RydProblem* p, const double* c_amp_reim, const double* c_det, const void* x, void* y,
                             void* workspace, size_t workspace_bytes, void* stream_) {
    const double zero[2] = {0.0, 0.0}, one[2] = {1.0, 0.0};
    return rydiff_apply_factor(p, c_amp_reim, c_det, zero, one, x, y, 0, nullptr, nullptr, 0, workspace, workspace_bytes, stream_);
}

}  // extern "C"
