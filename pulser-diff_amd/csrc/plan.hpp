// Host-side planning: validates a RydProblem, groups qubits that share coefficients, builds the list
// of exponential "stages" (one per tsave interval for KRYLOV_SE) and carves the device workspace.
//
// Reference semantics restated here:
//   interpolation indices / weights      pulser_diff/hamiltonian.py:532-542
//   KRYLOV_SE right-endpoint H freezing  SURVEY.md section 8 a-4 (pinned by notebook outputs KA-2..4)
//   term -> qubit maps                   pulser_diff/hamiltonian.py:419-452, backend.py:102-112
#pragma once
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rydiff.h"

namespace rydiff {

constexpr int kMaxGroups = RYDIFF_MAX_QUBITS;  // at most one coefficient group per qubit
constexpr double kRhoCap = 6.0;                // per-exponential spectral radius*tau cap (sub-steps above it)
constexpr size_t kAlign = 256;

struct Stage {
    double tau;        // duration of this exponential
    int step;          // tsave interval it belongs to
    int nsub;          // sub-steps (set once the spectral width is known)
    int idx[4];        // sample indices entering the coefficient combination
    double w[4];       // their weights
    double dwdt[4];    // d w / d (interpolation time)
    int tn[2];         // tsave indices the interpolation time depends on (-1: none) ...
    double tnw[2];     // ... with d(time)/d(tsave[tn[i]]) = tnw[i]
    int t_hi, t_lo;    // tau = tau_scale * (P_hi - P_lo); P = tsave[index] or a fixed sample-grid point (index -1)
    double tau_scale;
};

struct Groups {
    int n = 0;
    uint32_t amp_index_mask[kMaxGroups];  // bits of the AMPLITUDE index (qubit j <-> bit N-1-j)
    uint64_t members[kMaxGroups];         // which terms contribute to this group's coefficient
    int count[kMaxGroups];                // qubits in the group
    uint32_t flagged = 0;                 // groups whose member terms carry the flag (amp: conditioned flips, det: ones-counting)
    int nq[kMaxGroups] = {0};             // detuning groups: qubits in the group (count is 0 for a ones-counting group)
};

// Pauli-string observables as the kernels read them (pauli_kernels.hpp): the strings of every observable grouped by flip mask
struct PauliGroup {
    uint32_t xm;            // flip mask in amplitude-index bits
    uint32_t first, count;  // its strings in the string table
    uint32_t layout;        // who evaluates it: tile layout 0 / 1 (k_pauli_expect_tile) or kPauliDirect (k_pauli_expect_direct)
};
constexpr uint32_t kPauliDirect = 255;
struct PauliString {
    double wr, wi;  // w_s * i^ny
    uint32_t zm;    // sign mask in amplitude-index bits
    uint32_t pad;
};

struct Plan {
    int N = 0;       // qubits of the whole register
    int NL = 0;      // qubits that index a vector of this call: N, or N - shard_bits for a state-sharded run (slabs)
    int shard_bits = 0, rank_first = 0;
    bool shard_self = false;  // every rank's slab is part of this call (partners are read in place)
    size_t dim = 0;  // 2^NL
    int B = 1, Bc = 1, T = 0, n_samples = 0, Ka = 0, Kd = 0, n_obs = 0, solver = 0;
    double dt = 0.0, tol = 1e-13, ode_tol = 1e-9;
    Groups ga, gd;
    int NC = 0;  // doubles per (trajectory, stage) coefficient record: c_re[Ga], c_im[Ga], dcoef[Gd]
    std::vector<Stage> stages;
    std::vector<int> step_begin;  // stages of step k are [step_begin[k], step_begin[k+1])
    std::vector<double> tsave;
    // dense two-qubit terms (master equation on the doubled register): index-bit masks, tables [p][fwd | adjoint][16] (re, im)
    int n_pair = 0;
    uint32_t pair_ma[RYDIFF_MAX_PAIR_TERMS] = {0}, pair_mb[RYDIFF_MAX_PAIR_TERMS] = {0};
    std::vector<double> pair_tab;
    double pair_radius = 0.0;  // Gershgorin radius of the pair terms (sum over terms of the largest absolute row sum)
    size_t off_pair = 0;
    // XY exchange (RydProblem.xy_mode, xy_kernels.hpp): 0 none | 1 Hermitian | 2 one-directional; gradient replicas [kXyReplicas][N(N-1)/2]
    int xy_mode = 0;
    size_t off_xy_ge = 0;
    // Pauli-string observables: groups of observable o are [pauli_gfirst[o], pauli_gfirst[o + 1])
    int n_pobs = 0;
    std::vector<int32_t> pauli_gfirst;
    std::vector<PauliGroup> pauli_groups;
    std::vector<PauliString> pauli_strings;
    bool pauli_work[3] = {false, false, false};  // some group is evaluated in tile layout 0 / in tile layout 1 / by the direct kernel
    size_t off_pauli = 0, off_pauli_traj = 0, off_pauli_cot = 0;  // (the trajectory and the cotangent buffer serve the overlaps too)
    // state-overlap observables (overlap_kernels.hpp): targets stay where the caller has them
    int n_ov = 0, ov_batch = 1;
    // reduced density matrices (rdm_kernels.hpp): subsystem masks over amplitude-index bits, qubits, first row (behind the overlap rows)
    int n_rdm = 0, rdm_rows = 0;
    uint32_t rdm_am[RYDIFF_MAX_RDMS] = {0};
    int rdm_m[RYDIFF_MAX_RDMS] = {0}, rdm_row[RYDIFF_MAX_RDMS] = {0};
    // occupation correlations (moments_kernels.hpp): S, B_q, B_qr of |psi|^2 over the index bits, 1 + N + N(N-1)/2 rows behind the RDM
    // rows; past one tile of 2^12 amplitudes the tile records of one save point go through the workspace: [B][79][tiles] doubles
    int moments = 0;
    int moment_rows() const { return moments ? 1 + N + N * (N - 1) / 2 : 0; }
    size_t moment_tiles() const { return dim >> 12; }  // (kMomTileBits)
    size_t off_moments = 0;
    // energy observables (RydProblem.energy_rows, energy_kernels.hpp): E (and M2) behind the moment rows.  Workspace: one StageDev and
    // one coefficient record per save point, the workgroups' partial sums; backward: the scratch state(s) z and the gradient records
    int energy = 0;
    int energy_kernel = 0;  // RydProblem.energy_kernel: 0 automatic | 1 direct | 2 LDS-tile
    bool energy_tile_legal() const { return !xy_mode && N >= 13 && N <= 24; }  // (2^(N-12) <= energy_blocks() partial sums per state)
    size_t energy_blocks() const { return std::min<size_t>(std::max<size_t>(dim >> 8, 1), 4096); }  // workgroups of one (save point, trajectory)
    size_t off_energy_meta = 0, off_energy_coef = 0, off_energy_part = 0, off_energy_z = 0, off_energy_ge = 0;
    // measurement shots (shots_kernels.hpp): the sampled save points; scratch = chunk sums and their prefix, [B][shot_chunks()] doubles each
    int n_shots = 0;
    std::vector<int32_t> shot_times;
    size_t off_shot_sums = 0, off_shot_prefix = 0;
    // density-matrix observables (dm_kernels.hpp): n atoms (0: none); Pauli strings over the atoms grouped by flip mask per observable
    // (the evaluation) and over ALL observables (the cotangent scatter: one owner per entry; PauliString.pad = the observable)
    int dm_n = 0, n_dm_diag = 0, n_dm_pobs = 0, n_dm_fid = 0, dm_fid_batch = 1, dm_purity = 0, dm_shots = 0;
    std::vector<int32_t> dm_gfirst;
    std::vector<PauliGroup> dm_groups, dm_agroups;
    std::vector<PauliString> dm_strings, dm_astrings;
    size_t off_dm = 0;
    // reduced density matrices of the density-matrix register: subsystem masks over atom-index bits, atoms, first row (behind the purity row)
    int n_dm_rdm = 0, dm_rdm_rows = 0;
    uint32_t dm_rdm_am[RYDIFF_MAX_RDMS] = {0};
    int dm_rdm_m[RYDIFF_MAX_RDMS] = {0}, dm_rdm_row[RYDIFF_MAX_RDMS] = {0};
    // occupation correlations of the diagonal of rho (RydProblem.dm_moments): S, B_q, B_qr over the n atoms, the last density-matrix rows
    int dm_moments = 0;
    int dm_moment_rows() const { return dm_moments ? 1 + dm_n + dm_n * (dm_n - 1) / 2 : 0; }
    int dm_rows() const { return n_dm_diag + n_dm_pobs + n_dm_fid + dm_purity + dm_rdm_rows + dm_moment_rows(); }
    size_t dm_gfirst_bytes() const { return (dm_gfirst.size() * sizeof(int32_t) + 7) / 8 * 8; }
    size_t dm_bytes() const {
        return dm_gfirst_bytes() + (dm_groups.size() + dm_agroups.size()) * sizeof(PauliGroup) +
               (dm_strings.size() + dm_astrings.size()) * sizeof(PauliString);
    }
    size_t shot_chunks() const { return std::max<size_t>(dim >> 10, 1); }  // 2^10 amplitudes per chunk (kShotChunkBits)
    size_t pauli_gfirst_bytes() const { return (pauli_gfirst.size() * sizeof(int32_t) + 7) / 8 * 8; }
    size_t pauli_bytes() const {
        return n_pobs ? pauli_gfirst_bytes() + pauli_groups.size() * sizeof(PauliGroup) + pauli_strings.size() * sizeof(PauliString) : 0;
    }

    // workspace offsets (bytes)
    size_t off_meta_idx = 0, off_coef = 0, off_stats = 0, off_udiag = 0, off_buf0 = 0, off_buf1 = 0;
    size_t off_tape = 0, off_chain = 0, off_ge = 0, off_wtot = 0, off_members = 0, off_meta2 = 0, off_pp0 = 0, off_pp1 = 0, off_pp2 = 0, off_pp3 = 0, off_split = 0, off_ptable = 0, ptable_bytes = 0;
    size_t split_off_doubles[4] = {0, 0, 0, 0};  // where the split-diagonal table set of tile size 2^(10 + i) starts inside off_split
    size_t off_pm_begin = 0, off_pm_first = 0, off_pm_tau = 0, off_pm_nsub = 0;  // inputs of the on-device factor table build
    size_t state_bytes = 0;  // B * dim * 16
    size_t total_fwd = 0;
    int chain_slots = 0;
    int tape_mode = 0;
};

// The row order of expect_out / grad_expect / dexpect_out ([rows][n_tsave][B] each, dexpect_out one such array per direction):
// the blocks of the enumeration, in its order.  The only place that adds row counts up; every launch takes its pointers from at().
struct ExpectRows {
    // Moments: S, B_q, B_qr of the occupation correlations (empty unless bit_moments); Energy: E, M2 (empty unless energy_rows), the
    // last block of a ket's rows;
    // DmTrace (dm_diag rows, then the density-matrix Pauli rows) .. DmMoments (S, B_q, B_qr of diag rho; empty unless dm_moments):
    // the density-matrix rows
    enum Block { Diag, Pauli, Overlap, Rdm, Moments, Energy, DmTrace, DmFid, DmPurity, DmRdm, DmMoments, End };
    size_t stride = 0;        // doubles per row: (T + 1) * B
    int first[End + 1] = {};  // first row of each block; first[End]: all rows
    explicit ExpectRows(const Plan& pl) : stride(size_t(pl.T + 1) * pl.B) {
        const int count[End] = {pl.n_obs, pl.n_pobs, 2 * pl.n_ov, pl.rdm_rows, pl.moment_rows(), pl.energy, pl.n_dm_diag + pl.n_dm_pobs, pl.n_dm_fid, pl.dm_purity, pl.dm_rdm_rows, pl.dm_moment_rows()};
        for (int b = 0; b < End; ++b) first[b + 1] = first[b] + count[b];
    }
    int count(Block b) const { return first[b + 1] - first[b]; }
    int total() const { return first[End]; }
    size_t size() const { return size_t(total()) * stride; }  // doubles of one such array: the direction stride of dexpect_out
    // doubles from the first row of block `from` to the first row of block b (a launch that is handed the density-matrix rows
    // alone counts from DmTrace)
    size_t offset(Block b, Block from = Diag) const { return size_t(first[b] - first[from]) * stride; }
    // the first row of block b in the array that starts at `base`; nullptr: no such array, or no row in the blocks [b, end)
    template <class T>
    T* at(T* base, Block b, Block end) const {
        return (base && first[end] > first[b]) ? base + offset(b) : nullptr;
    }
    template <class T>
    T* at(T* base, Block b) const {
        return at(base, b, Block(b + 1));
    }
};

inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

inline bool build_groups(int N, int n_terms, const uint32_t* masks, Groups& g, std::string& err, uint64_t term_flags = 0) {
    g.n = 0;
    g.flagged = 0;
    if (n_terms > RYDIFF_MAX_TERMS) {
        err = "too many terms (max " + std::to_string(RYDIFF_MAX_TERMS) + ")";
        return false;
    }
    for (int j = 0; j < N; ++j) {
        uint64_t sig = 0;
        for (int k = 0; k < n_terms; ++k)
            if (masks[k] >> j & 1u) sig |= (1ull << k);
        if (!sig) continue;
        int found = -1;
        for (int q = 0; q < g.n; ++q)
            if (g.members[q] == sig) found = q;
        if (found < 0) {
            found = g.n++;
            g.members[found] = sig;
            g.amp_index_mask[found] = 0;
            g.count[found] = 0;
        }
        g.amp_index_mask[found] |= (1u << (N - 1 - j));
        g.count[found] += 1;
        if (sig & term_flags) {
            if ((sig & term_flags) != sig) {
                err = "terms that address qubit " + std::to_string(j) + " disagree on amp_conditioned_terms / det_ones_terms";
                return false;
            }
            g.flagged |= 1u << found;
        }
    }
    for (int k = 0; k < n_terms; ++k) {
        if (masks[k] == 0 || (N < 32 && (masks[k] >> N) != 0)) {
            err = "term mask " + std::to_string(k) + " is empty or addresses a qubit >= n_qubits";
            return false;
        }
    }
    return true;
}

inline uint32_t to_index_mask(uint32_t qubit_mask, int N) {
    uint32_t m = 0;
    for (int j = 0; j < N; ++j)
        if (qubit_mask >> j & 1u) m |= 1u << (N - 1 - j);
    return m;
}

// RydProblem.pauli_* -> per-observable groups of strings that share a flip mask (one partner load per group)
inline bool build_pauli(const RydProblem* p, Plan& pl, std::string& err) {
    pl.n_pobs = 0;
    pl.pauli_gfirst.clear();
    pl.pauli_groups.clear();
    pl.pauli_strings.clear();
    if (p->n_pauli_obs < 0 || p->n_pauli_strings < 0) {
        err = "negative Pauli observable / string count";
        return false;
    }
    if (p->n_pauli_obs == 0) {
        if (p->n_pauli_strings != 0) {
            err = "Pauli strings without a Pauli observable";
            return false;
        }
        return true;
    }
    const int no = p->n_pauli_obs, ns = p->n_pauli_strings;
    if (ns > RYDIFF_MAX_PAULI_STRINGS || no > RYDIFF_MAX_PAULI_STRINGS) {
        err = "too many Pauli strings / observables (max " + std::to_string(RYDIFF_MAX_PAULI_STRINGS) + ")";
        return false;
    }
    if (!p->pauli_first || (ns > 0 && (!p->pauli_x || !p->pauli_z || !p->pauli_w))) {
        err = "missing Pauli observable arrays (pauli_first / pauli_x / pauli_z / pauli_w)";
        return false;
    }
    if (p->pauli_first[0] != 0 || p->pauli_first[no] != ns) {
        err = "pauli_first must start at 0 and end at n_pauli_strings";
        return false;
    }
    for (int o = 0; o < no; ++o)
        if (p->pauli_first[o + 1] < p->pauli_first[o]) {
            err = "pauli_first must be non-decreasing";
            return false;
        }
    if (p->shard_bits > 0) {
        err = "Pauli-string observables: not implemented together with state sharding";
        return false;
    }
    const int N = p->n_qubits;
    for (int s = 0; s < ns; ++s) {
        if (N < 32 && (((p->pauli_x[s] | p->pauli_z[s]) >> N) != 0)) {
            err = "Pauli string " + std::to_string(s) + " addresses a qubit >= n_qubits";
            return false;
        }
        if (!std::isfinite(p->pauli_w[s])) {
            err = "Pauli string " + std::to_string(s) + " has a non-finite weight";
            return false;
        }
    }
    pl.n_pobs = no;
    pl.pauli_gfirst.assign(no + 1, 0);
    for (int o = 0; o < no; ++o) {
        pl.pauli_gfirst[o] = int32_t(pl.pauli_groups.size());
        std::vector<int> order;
        for (int s = p->pauli_first[o]; s < p->pauli_first[o + 1]; ++s) order.push_back(s);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p->pauli_x[a] < p->pauli_x[b]; });
        for (size_t i = 0; i < order.size(); ++i) {
            const int s = order[i];
            if (i == 0 || p->pauli_x[s] != p->pauli_x[order[i - 1]])
                pl.pauli_groups.push_back({to_index_mask(p->pauli_x[s], N), uint32_t(pl.pauli_strings.size()), 0u, kPauliDirect});
            pl.pauli_groups.back().count += 1;
            static const double ph[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};  // i^ny
            const int ny = __builtin_popcount(p->pauli_x[s] & p->pauli_z[s]) & 3;
            pl.pauli_strings.push_back({p->pauli_w[s] * ph[ny][0], p->pauli_w[s] * ph[ny][1], to_index_mask(p->pauli_z[s], N), 0u});
        }
    }
    pl.pauli_gfirst[no] = int32_t(pl.pauli_groups.size());
    return true;
}

// RydProblem.overlap_*: counts, target batch (1 or B), pointer
inline bool build_overlaps(const RydProblem* p, Plan& pl, std::string& err) {
    pl.n_ov = 0;
    pl.ov_batch = 1;
    if (p->n_overlaps < 0 || p->n_overlaps > RYDIFF_MAX_OVERLAPS) {
        err = "n_overlaps must be in [0, " + std::to_string(RYDIFF_MAX_OVERLAPS) + "]";
        return false;
    }
    if (p->n_overlaps == 0) return true;
    if (p->overlap_batch != 1 && p->overlap_batch != p->batch) {
        err = "overlap_batch must be 1 or batch";
        return false;
    }
    if (!p->overlap_targets) {
        err = "missing overlap_targets";
        return false;
    }
    if (p->shard_bits > 0) {
        err = "state-overlap observables: not implemented together with state sharding";
        return false;
    }
    pl.n_ov = p->n_overlaps;
    pl.ov_batch = p->overlap_batch;
    return true;
}

// RydProblem.n_rdms / rdm_masks: count, every mask non-empty, at most RYDIFF_MAX_RDM_QUBITS qubits, all inside the register
inline bool build_rdms(const RydProblem* p, Plan& pl, std::string& err) {
    pl.n_rdm = pl.rdm_rows = 0;
    if (p->n_rdms < 0 || p->n_rdms > RYDIFF_MAX_RDMS) {
        err = "n_rdms must be in [0, " + std::to_string(RYDIFF_MAX_RDMS) + "]";
        return false;
    }
    if (p->n_rdms == 0) return true;
    if (!p->rdm_masks) {
        err = "missing rdm_masks";
        return false;
    }
    int rows = 0;
    for (int o = 0; o < p->n_rdms; ++o) {
        const uint32_t qm = p->rdm_masks[o];
        int m = 0;
        uint32_t am = 0;
        for (int j = 0; j < 32; ++j)
            if (qm >> j & 1u) {
                if (j >= p->n_qubits) {
                    err = "rdm_masks[" + std::to_string(o) + "] addresses a qubit outside the register";
                    return false;
                }
                am |= 1u << (p->n_qubits - 1 - j);
                ++m;
            }
        if (m == 0) {
            err = "rdm_masks[" + std::to_string(o) + "] is empty";
            return false;
        }
        if (m > RYDIFF_MAX_RDM_QUBITS) {
            err = "rdm_masks[" + std::to_string(o) + "] holds more than " + std::to_string(RYDIFF_MAX_RDM_QUBITS) + " qubits";
            return false;
        }
        pl.rdm_am[o] = am;
        pl.rdm_m[o] = m;
        pl.rdm_row[o] = rows;
        rows += 2 << (2 * m);
    }
    if (p->shard_bits > 0) {
        err = "reduced density matrices: not implemented together with state sharding";
        return false;
    }
    pl.n_rdm = p->n_rdms;
    pl.rdm_rows = rows;
    return true;
}

// RydProblem.n_shots / shot_*: counts against the caps, pointers, the list of sampled save points
inline bool build_shots(const RydProblem* p, Plan& pl, std::string& err) {
    pl.n_shots = 0;
    pl.shot_times.clear();
    if (p->n_shots < 0 || p->n_shots > RYDIFF_MAX_SHOTS) {
        err = "n_shots must be in [0, " + std::to_string(RYDIFF_MAX_SHOTS) + "]";
        return false;
    }
    if (p->n_shots == 0) return true;
    if (p->n_shot_times < 1 || p->n_shot_times > p->n_tsave) {
        err = "n_shot_times must be in [1, n_tsave]";
        return false;
    }
    if (!p->shot_times || !p->shot_uniforms || !p->shots_out) {
        err = "missing shot arrays (shot_times / shot_uniforms / shots_out)";
        return false;
    }
    for (int i = 0; i < p->n_shot_times; ++i)
        if (p->shot_times[i] < 0 || p->shot_times[i] >= p->n_tsave || (i > 0 && p->shot_times[i] <= p->shot_times[i - 1])) {
            err = "shot_times must be strictly increasing save-point indices in [0, n_tsave)";
            return false;
        }
    if (p->shard_bits > 0) {
        err = "measurement shots: not implemented together with state sharding";
        return false;
    }
    pl.n_shots = p->n_shots;
    pl.shot_times.assign(p->shot_times, p->shot_times + p->n_shot_times);
    return true;
}

// RydProblem.dm_*: the doubled register, counts, masks, tables; the string groups of the evaluation and of the cotangent scatter
inline bool build_dm(const RydProblem* p, Plan& pl, std::string& err) {
    pl.dm_n = pl.n_dm_diag = pl.n_dm_pobs = pl.n_dm_fid = pl.dm_purity = pl.dm_shots = 0;
    pl.n_dm_rdm = pl.dm_rdm_rows = pl.dm_moments = 0;
    pl.dm_fid_batch = 1;
    pl.dm_gfirst.clear();
    pl.dm_groups.clear();
    pl.dm_agroups.clear();
    pl.dm_strings.clear();
    pl.dm_astrings.clear();
    if (p->dm_atoms == 0) return true;
    const int n = p->dm_atoms;
    if (n < 0 || n > RYDIFF_MAX_DM_ATOMS) {
        err = "dm_atoms must be in [0, " + std::to_string(RYDIFF_MAX_DM_ATOMS) + "]";
        return false;
    }
    if (p->n_qubits != 2 * n) {
        err = "dm_atoms = n declares a doubled register: n_qubits must be 2 * dm_atoms";
        return false;
    }
    if (p->n_dm_diag < 0 || p->n_dm_diag > RYDIFF_MAX_DM_DIAG) {
        err = "n_dm_diag must be in [0, " + std::to_string(RYDIFF_MAX_DM_DIAG) + "]";
        return false;
    }
    if (p->n_dm_diag > 0 && !p->dm_diag) {
        err = "missing dm_diag";
        return false;
    }
    const int no = p->n_dm_pauli_obs, ns = p->n_dm_pauli_strings;
    if (no < 0 || ns < 0 || no > RYDIFF_MAX_PAULI_STRINGS || ns > RYDIFF_MAX_PAULI_STRINGS) {
        err = "n_dm_pauli_obs / n_dm_pauli_strings must be in [0, " + std::to_string(RYDIFF_MAX_PAULI_STRINGS) + "]";
        return false;
    }
    if (no == 0 && ns != 0) {
        err = "density-matrix Pauli strings without a Pauli observable";
        return false;
    }
    if (no > 0) {
        if (!p->dm_pauli_first || (ns > 0 && (!p->dm_pauli_x || !p->dm_pauli_z || !p->dm_pauli_w))) {
            err = "missing density-matrix Pauli arrays (dm_pauli_first / dm_pauli_x / dm_pauli_z / dm_pauli_w)";
            return false;
        }
        if (p->dm_pauli_first[0] != 0 || p->dm_pauli_first[no] != ns) {
            err = "dm_pauli_first must start at 0 and end at n_dm_pauli_strings";
            return false;
        }
        for (int o = 0; o < no; ++o)
            if (p->dm_pauli_first[o + 1] < p->dm_pauli_first[o]) {
                err = "dm_pauli_first must be non-decreasing";
                return false;
            }
        for (int s = 0; s < ns; ++s) {
            if (((p->dm_pauli_x[s] | p->dm_pauli_z[s]) >> n) != 0) {
                err = "density-matrix Pauli string " + std::to_string(s) + " addresses an atom >= dm_atoms";
                return false;
            }
            if (!std::isfinite(p->dm_pauli_w[s])) {
                err = "density-matrix Pauli string " + std::to_string(s) + " has a non-finite weight";
                return false;
            }
        }
    }
    if (p->n_dm_fid < 0 || p->n_dm_fid > RYDIFF_MAX_OVERLAPS) {
        err = "n_dm_fid must be in [0, " + std::to_string(RYDIFF_MAX_OVERLAPS) + "]";
        return false;
    }
    if (p->n_dm_fid > 0) {
        if (p->dm_fid_batch != 1 && p->dm_fid_batch != p->batch) {
            err = "dm_fid_batch must be 1 or batch";
            return false;
        }
        if (!p->dm_fid_targets) {
            err = "missing dm_fid_targets";
            return false;
        }
    }
    if ((p->dm_purity != 0 && p->dm_purity != 1) || (p->dm_shots != 0 && p->dm_shots != 1)) {
        err = "dm_purity and dm_shots must be 0 or 1";
        return false;
    }
    if (p->dm_moments != 0 && p->dm_moments != 1) {
        err = "dm_moments must be 0 or 1";
        return false;
    }
    if (p->dm_shots && p->n_shots <= 0) {
        err = "dm_shots needs n_shots > 0 (and the shot arrays)";
        return false;
    }
    if (p->n_dm_rdms < 0 || p->n_dm_rdms > RYDIFF_MAX_RDMS) {
        err = "n_dm_rdms must be in [0, " + std::to_string(RYDIFF_MAX_RDMS) + "]";
        return false;
    }
    if (p->n_dm_rdms > 0 && !p->dm_rdm_masks) {
        err = "missing dm_rdm_masks";
        return false;
    }
    int rdm_rows = 0;
    for (int o = 0; o < p->n_dm_rdms; ++o) {
        const uint32_t qm = p->dm_rdm_masks[o];
        if (n < 32 && (qm >> n) != 0) {
            err = "dm_rdm_masks[" + std::to_string(o) + "] addresses an atom >= dm_atoms";
            return false;
        }
        const int m = __builtin_popcount(qm);
        if (m == 0) {
            err = "dm_rdm_masks[" + std::to_string(o) + "] is empty";
            return false;
        }
        if (m > RYDIFF_MAX_RDM_QUBITS) {
            err = "dm_rdm_masks[" + std::to_string(o) + "] holds more than " + std::to_string(RYDIFF_MAX_RDM_QUBITS) + " atoms";
            return false;
        }
        pl.dm_rdm_am[o] = to_index_mask(qm, n);
        pl.dm_rdm_m[o] = m;
        pl.dm_rdm_row[o] = rdm_rows;
        rdm_rows += 2 << (2 * m);
    }
    if (p->shard_bits > 0) {
        err = "density-matrix observables: not implemented together with state sharding";
        return false;
    }
    pl.dm_n = n;
    pl.n_dm_rdm = p->n_dm_rdms;
    pl.dm_rdm_rows = rdm_rows;
    pl.n_dm_diag = p->n_dm_diag;
    pl.n_dm_pobs = no;
    pl.n_dm_fid = p->n_dm_fid;
    pl.dm_fid_batch = p->n_dm_fid ? p->dm_fid_batch : 1;
    pl.dm_purity = p->dm_purity;
    pl.dm_shots = p->dm_shots;
    pl.dm_moments = p->dm_moments;
    static const double ph[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};  // i^ny
    auto make_string = [&](int s, uint32_t row) {
        const int ny = __builtin_popcount(p->dm_pauli_x[s] & p->dm_pauli_z[s]) & 3;
        return PauliString{p->dm_pauli_w[s] * ph[ny][0], p->dm_pauli_w[s] * ph[ny][1], to_index_mask(p->dm_pauli_z[s], n), row};
    };
    // grouped by flip mask: per observable (evaluation), over all of them (cotangent scatter)
    auto group_strings = [&](std::vector<int>& order, std::vector<PauliGroup>& groups, std::vector<PauliString>& strings,
                             const std::vector<uint32_t>& row_of) {
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p->dm_pauli_x[a] < p->dm_pauli_x[b]; });
        for (size_t i = 0; i < order.size(); ++i) {
            const int s = order[i];
            if (i == 0 || p->dm_pauli_x[s] != p->dm_pauli_x[order[i - 1]])
                groups.push_back({to_index_mask(p->dm_pauli_x[s], n), uint32_t(strings.size()), 0u, kPauliDirect});
            groups.back().count += 1;
            strings.push_back(make_string(s, row_of[s]));
        }
    };
    std::vector<uint32_t> row_of(ns, 0u);
    for (int o = 0; o < no; ++o)
        for (int s = p->dm_pauli_first[o]; s < p->dm_pauli_first[o + 1]; ++s) row_of[s] = uint32_t(o);
    pl.dm_gfirst.assign(no + 1, 0);
    for (int o = 0; o < no; ++o) {
        pl.dm_gfirst[o] = int32_t(pl.dm_groups.size());
        std::vector<int> order;
        for (int s = p->dm_pauli_first[o]; s < p->dm_pauli_first[o + 1]; ++s) order.push_back(s);
        group_strings(order, pl.dm_groups, pl.dm_strings, row_of);
    }
    pl.dm_gfirst[no] = int32_t(pl.dm_groups.size());
    if (pl.n_dm_diag) pl.dm_agroups.push_back({0u, 0u, 0u, kPauliDirect});  // the diagonal tables ride the xm = 0 group
    {
        std::vector<int> order(ns);
        for (int s = 0; s < ns; ++s) order[s] = s;
        std::vector<PauliGroup> g;
        group_strings(order, g, pl.dm_astrings, row_of);
        for (const PauliGroup& q : g) {
            if (q.xm == 0u && pl.n_dm_diag) pl.dm_agroups[0] = q;  // (sorted by mask: the strings of xm = 0 come first)
            else pl.dm_agroups.push_back(q);
        }
    }
    return true;
}

// RydProblem.xy_*: what the exchange term is refused with (host only; "not implemented" in the message -> RYDIFF_ENOTIMPL)
inline bool xy_validate(const RydProblem* p, std::string& err) {
    if (p->xy_mode < 0 || p->xy_mode > 2) {
        err = "xy_mode must be 0 (none), 1 (Hermitian exchange) or 2 (one-directional)";
        return false;
    }
    if (p->xy_mode == 0) return true;
    if (p->n_qubits > 1 && !p->xy_pairs) {
        err = "xy_pairs is required with xy_mode != 0 on more than one qubit";
        return false;
    }
    const char* with = nullptr;
    if (p->n_pair_terms > 0) with = "dense pair terms (n_pair_terms > 0)";
    else if (p->shard_bits > 0) with = "state sharding (shard_bits > 0)";
    else if (p->dm_atoms > 0) with = "density-matrix registers (dm_atoms > 0)";
    else if (p->amp_conditioned_terms || p->det_ones_terms) with = "conditioned flips / ones-counting terms";
    else if (p->kernel_variant != 0 && p->kernel_variant != 1 && p->kernel_variant != 9)
        with = "this kernel_variant (the exchange runs on the direct family: 0, 1 or 9)";
    if (with) {
        err = std::string("XY exchange (xy_mode != 0): not implemented together with ") + with;
        return false;
    }
    return true;
}

// RydProblem.energy_*: the range, the tables, and what the block is refused with (host only; "not implemented" -> RYDIFF_ENOTIMPL)
inline bool energy_validate(const RydProblem* p, std::string& err) {
    if (p->energy_rows < 0 || p->energy_rows > 2) {
        err = "energy_rows must be 0 (off), 1 (E) or 2 (E and M2)";
        return false;
    }
    if (p->energy_rows == 0) return true;
    if (p->energy_kernel < 0 || p->energy_kernel > 2) {
        err = "energy_kernel must be 0 (automatic), 1 (direct) or 2 (LDS-tile)";
        return false;
    }
    if ((p->n_amp_terms > 0 && !p->energy_amp) || (p->n_det_terms > 0 && !p->energy_det)) {
        err = "energy_rows > 0 needs energy_amp / energy_det (the coefficients at the save points) for the problem's terms";
        return false;
    }
    const char* with = nullptr;
    if (p->n_pair_terms > 0) with = "dense pair terms (n_pair_terms > 0)";
    else if (p->dm_atoms > 0) with = "density-matrix registers (dm_atoms > 0: the Tr(rho H) rows are a follow-up)";
    else if (p->shard_bits > 0) with = "state sharding (shard_bits > 0)";
    else if (p->amp_conditioned_terms || p->det_ones_terms) with = "conditioned flips / ones-counting terms";
    else if (p->xy_mode == 2) with = "the one-directional exchange (xy_mode = 2: the expectation of a non-Hermitian generator is not an energy)";
    if (with) {
        err = std::string("energy observables (energy_rows > 0): not implemented together with ") + with;
        return false;
    }
    if (p->energy_kernel == 2 && (p->xy_mode != 0 || p->n_qubits < 13 || p->n_qubits > 24)) {
        err = "energy_kernel = 2: the LDS-tile version is not implemented outside 13 .. 24 qubits or with the XY exchange";
        return false;
    }
    return true;
}

// number of gradient replicas of the energy block's coefficient records (energy_kernels.hpp)
constexpr int kEnergyReplicas = 16;

// number of XY gradient replicas in the workspace (xy_kernels.hpp)
constexpr int kXyReplicas = 32;

// `width`: half spectral width of the generator when it is already known (<= 0: not yet) — the continuous solver's
// sub-step shrinks with it.
inline bool build_plan(const RydProblem* p, Plan& pl, std::string& err, double width = -1.0) {
    if (!p) {
        err = "null problem";
        return false;
    }
    if (p->n_qubits < 1 || p->n_qubits > RYDIFF_MAX_QUBITS) {
        err = "n_qubits out of range";
        return false;
    }
    if (p->batch < 1 || (p->coeff_batch != 1 && p->coeff_batch != p->batch)) {
        err = "coeff_batch must be 1 or batch";
        return false;
    }
    if (p->batch > 65535) {  // the trajectory index is the y dimension of every launch grid
        err = "batch must be <= 65535 (split the columns / trajectories into several calls)";
        return false;
    }
    if (p->n_tsave < 2 || !p->tsave) {
        err = "need at least two evaluation times";
        return false;
    }
    if (p->n_amp_terms < 0 || p->n_det_terms < 0) {
        err = "negative term count";
        return false;
    }
    if ((p->n_amp_terms + p->n_det_terms) > 0 && (p->n_samples < 2 || !(p->dt > 0.0))) {
        err = "coefficient tables need n_samples >= 2 and dt > 0";
        return false;
    }
    if ((p->n_amp_terms > 0 && (!p->amp_tables || !p->amp_masks)) || (p->n_det_terms > 0 && (!p->det_tables || !p->det_masks))) {
        err = "missing coefficient tables or masks";
        return false;
    }
    if (p->n_qubits > 1 && !p->u_pairs) {
        err = "u_pairs is required for more than one qubit";
        return false;
    }
    if (p->n_obs < 0 || (p->n_obs > 0 && !p->obs_diag)) {
        err = "obs_diag missing";
        return false;
    }
    if (p->solver != RYDIFF_SOLVER_KRYLOV_SE && p->solver != RYDIFF_SOLVER_DP5_SE) {
        err = "unknown solver";
        return false;
    }
    if (p->n_pair_terms < 0 || p->n_pair_terms > RYDIFF_MAX_PAIR_TERMS || (p->n_pair_terms > 0 && (!p->pair_qubits || !p->pair_tables))) {
        err = "bad pair terms";
        return false;
    }
    if (!xy_validate(p, err)) return false;
    pl.xy_mode = p->xy_mode;
    if (!energy_validate(p, err)) return false;
    pl.energy = p->energy_rows;
    pl.energy_kernel = p->energy_rows ? p->energy_kernel : 0;
    pl.n_pair = p->n_pair_terms;
    pl.pair_tab.assign(size_t(pl.n_pair) * 64, 0.0);
    pl.pair_radius = 0.0;
    for (int t = 0; t < pl.n_pair; ++t) {
        const uint32_t qa = p->pair_qubits[2 * t], qb = p->pair_qubits[2 * t + 1];
        if (qa >= uint32_t(p->n_qubits) || qb >= uint32_t(p->n_qubits) || qa == qb) {
            err = "pair term addresses qubits outside the register";
            return false;
        }
        pl.pair_ma[t] = 1u << (p->n_qubits - 1 - qa);
        pl.pair_mb[t] = 1u << (p->n_qubits - 1 - qb);
        const double* src = p->pair_tables + size_t(t) * 32;
        double* fwd = pl.pair_tab.data() + size_t(t) * 64;
        double* adj = fwd + 32;
        double worst = 0.0;
        for (int r = 0; r < 4; ++r) {
            double row = 0.0;
            for (int c = 0; c < 4; ++c) {
                const double re = src[2 * (4 * r + c)], im = src[2 * (4 * r + c) + 1];
                fwd[2 * (4 * r + c)] = re;
                fwd[2 * (4 * r + c) + 1] = im;
                adj[2 * (4 * c + r)] = re;  // conjugate transpose
                adj[2 * (4 * c + r) + 1] = -im;
                row += std::sqrt(re * re + im * im);
            }
            worst = std::max(worst, row);
        }
        pl.pair_radius += worst;
    }
    pl.N = p->n_qubits;
    if (!build_pauli(p, pl, err)) return false;
    if (!build_overlaps(p, pl, err)) return false;
    if (!build_rdms(p, pl, err)) return false;
    if (!build_shots(p, pl, err)) return false;
    if (!build_dm(p, pl, err)) return false;
    pl.moments = 0;
    if (p->bit_moments != 0 && p->bit_moments != 1) {
        err = "bit_moments must be 0 or 1";
        return false;
    }
    if (p->bit_moments && p->shard_bits > 0) {
        err = "bit moments (occupation correlations): not implemented together with state sharding";
        return false;
    }
    if (p->bit_moments && p->dm_atoms != 0) {
        err = "bit moments (occupation correlations): not implemented for density-matrix registers (dm_atoms > 0)";
        return false;
    }
    pl.moments = p->bit_moments;
    pl.shard_bits = p->shard_bits;
    if (pl.shard_bits < 0 || pl.shard_bits > 6 || pl.shard_bits >= pl.N) {
        err = "shard_bits must be in [0, min(6, n_qubits - 1)]";
        return false;
    }
    pl.NL = pl.N - pl.shard_bits;
    pl.rank_first = p->shard_rank_first;
    if (pl.shard_bits) {
        const int world = 1 << pl.shard_bits;
        if (p->coeff_batch != 1 || p->n_pair_terms != 0) {
            err = "state-sharded runs take shared coefficient tables (coeff_batch = 1) and no pair terms";
            return false;
        }
        if (pl.rank_first < 0 || pl.rank_first + p->batch > world) {
            err = "shard_rank_first + batch exceeds 2^shard_bits";
            return false;
        }
        pl.shard_self = p->batch == world;
        if (!pl.shard_self && (!p->shard_recv || !p->shard_exchange || p->batch != 1)) {
            err = "state-sharded run with ranks elsewhere: one slab per call (batch = 1), shard_recv and shard_exchange required";
            return false;
        }
    }
    pl.dim = size_t(1) << pl.NL;
    pl.B = p->batch;
    pl.Bc = p->coeff_batch;
    pl.T = p->n_tsave - 1;
    pl.n_samples = p->n_samples;
    pl.Ka = p->n_amp_terms;
    pl.Kd = p->n_det_terms;
    pl.n_obs = p->n_obs;
    pl.dt = p->dt;
    pl.solver = p->solver;
    if (p->solver == RYDIFF_SOLVER_KRYLOV_SE) {
        pl.tol = (p->tol > 0.0) ? p->tol : 1e-13;
    } else {
        // continuous-time solver: `tol` is the target accuracy of the solution; the exponentials are kept well below it
        pl.ode_tol = (p->tol > 0.0) ? p->tol : 1e-9;
        pl.tol = std::min(1e-13, std::max(pl.ode_tol * 1e-3, 1e-15));
    }
    pl.tsave.assign(p->tsave, p->tsave + p->n_tsave);
    for (int k = 0; k < pl.T; ++k) {
        if (!(pl.tsave[k + 1] > pl.tsave[k]) || !std::isfinite(pl.tsave[k + 1])) {
            err = "tsave must be finite and strictly increasing";
            return false;
        }
    }
    if (!build_groups(pl.N, pl.Ka, p->amp_masks, pl.ga, err, p->amp_conditioned_terms)) return false;
    if (!build_groups(pl.N, pl.Kd, p->det_masks, pl.gd, err, p->det_ones_terms)) return false;
    if (pl.ga.flagged && (pl.N & 1)) {
        err = "conditioned flips pair the qubits (2i, 2i+1): n_qubits must be even";
        return false;
    }
    if ((pl.ga.flagged || pl.gd.flagged) && (p->shard_bits || p->n_pair_terms)) {
        err = "conditioned flips / ones-counting terms: not implemented together with state sharding or pair terms";
        return false;
    }
    // ones-counting detuning groups contribute dcoef * (0 - #ones): the kernels' (count - popcount) with count = 0
    for (int g = 0; g < pl.gd.n; ++g) {
        pl.gd.nq[g] = pl.gd.count[g];
        if (pl.gd.flagged >> g & 1u) pl.gd.count[g] = 0;
    }
    pl.NC = 2 * pl.ga.n + pl.gd.n;

    pl.stages.clear();
    pl.step_begin.assign(pl.T + 1, 0);
    const int n = pl.n_samples;
    auto node = [&](double t, int tnode, Stage& s, double weight, int slot) {
        // hamiltonian.py:532-533 / :538,542
        int i1 = 0, i2 = 0;
        double frac = 0.0;
        if (pl.Ka + pl.Kd > 0) {
            double q = std::floor(t / pl.dt);
            double lim = double(n - 2);
            double qq = q < lim ? q : lim;
            i1 = int(qq) > 0 ? int(qq) : 0;
            i2 = (i1 + 1 < n - 2) ? i1 + 1 : n - 2;
            if (i2 < 0) i2 = 0;
            frac = (t - i1 * pl.dt) / pl.dt;
        }
        s.idx[slot] = i1;
        s.idx[slot + 1] = i2;
        s.w[slot] = weight * (1.0 - frac);
        s.w[slot + 1] = weight * frac;
        s.dwdt[slot] = -weight / pl.dt;
        s.dwdt[slot + 1] = weight / pl.dt;
        (void)tnode;
    };
    // continuous-time solver: largest sub-step of the 4th-order commutator-free Magnus scheme.  Calibrated on the
    // reference's own workloads (tests/test_gpu_dp5.py): 2.5 ns keeps the global error below ~2e-10; error ~ h^4.
    // The leading error term carries two powers of the generator's size ([A,[A,A']]), so beyond the calibrated range
    // (half width ~1e2 rad/us) the step shrinks like width^-1/2 — this is what keeps strongly dissipative master-equation
    // runs (large pair terms) and strongly interacting registers at the same accuracy.
    constexpr double kMagnusWidthRef = 128.0;
    const double h_max = 2.5e-3 * std::pow(std::min(std::max(pl.ode_tol, 1e-14), 1e-4) / 1e-10, 0.25) *
                         (width > kMagnusWidthRef ? std::sqrt(kMagnusWidthRef / width) : 1.0);
    for (int k = 0; k < pl.T; ++k) {
        pl.step_begin[k] = int(pl.stages.size());
        if (pl.solver == RYDIFF_SOLVER_KRYLOV_SE) {
            Stage s{};
            s.step = k;
            s.tau = pl.tsave[k + 1] - pl.tsave[k];
            s.nsub = 1;
            s.tn[0] = k + 1;
            s.tn[1] = -1;
            s.tnw[0] = 1.0;
            s.tnw[1] = 0.0;
            s.t_hi = k + 1;
            s.t_lo = k;
            s.tau_scale = 1.0;
            node(pl.tsave[k + 1], k + 1, s, 1.0, 0);
            s.idx[2] = s.idx[3] = 0;
            s.w[2] = s.w[3] = 0.0;
            s.dwdt[2] = s.dwdt[3] = 0.0;
            pl.stages.push_back(s);
        } else {
            // DP5_SE semantics = the continuous-time solution.  H(t) is piecewise LINEAR in t between sample points
            // (hamiltonian.py:532-542), so the interval is cut at the sample grid and every linear piece is advanced by
            // CF4 Magnus steps: for linear H the two exponentials are exp(-i h/2 H(t0+5h/6)) exp(-i h/2 H(t0+h/6)).
            const double a = pl.tsave[k], b = pl.tsave[k + 1];
            std::vector<double> pts{a};
            if (pl.Ka + pl.Kd > 0) {
                long i = long(std::floor(a / pl.dt)) + 1;
                while (i <= long(n) - 2 && double(i) * pl.dt < b - 1e-13) {
                    if (double(i) * pl.dt > a + 1e-13) pts.push_back(double(i) * pl.dt);
                    ++i;
                }
            }
            pts.push_back(b);
            const int np = int(pts.size()) - 1;
            for (int q = 0; q < np; ++q) {
                const double p0 = pts[q], p1 = pts[q + 1], hf = p1 - p0;
                const int lo_owner = (q == 0) ? k : -1, hi_owner = (q == np - 1) ? k + 1 : -1;
                int S = std::max(1, int(std::ceil(hf / h_max - 1e-9)));
                if (p->dp5_piece_refine && n >= 2) {  // caller's hint: pieces across which the coefficient tables jump
                    const long si = std::min(std::max(long(std::floor(0.5 * (p0 + p1) / pl.dt)), 0L), long(n) - 2);
                    S *= std::max(1, int(p->dp5_piece_refine[si]));
                }
                for (int sub = 0; sub < S; ++sub)
                    for (double theta : {1.0 / 6.0, 5.0 / 6.0}) {
                        Stage s{};
                        s.step = k;
                        const double mu = (sub + theta) / S;
                        s.tau = hf / (2.0 * S);
                        s.nsub = 1;
                        s.tn[0] = lo_owner;
                        s.tn[1] = hi_owner;
                        s.tnw[0] = 1.0 - mu;
                        s.tnw[1] = mu;
                        s.t_hi = hi_owner;
                        s.t_lo = lo_owner;
                        s.tau_scale = 1.0 / (2.0 * S);
                        node(p0 + mu * hf, -1, s, 1.0, 0);
                        s.idx[2] = s.idx[3] = 0;
                        s.w[2] = s.w[3] = 0.0;
                        s.dwdt[2] = s.dwdt[3] = 0.0;
                        pl.stages.push_back(s);
                    }
            }
        }
    }
    pl.step_begin[pl.T] = int(pl.stages.size());
    pl.state_bytes = size_t(pl.B) * pl.dim * 16;
    return true;
}

// Carve the workspace. `chain_slots` = number of intermediate state buffers the backward recompute needs.
// tape_mode: 0 none | 1 one state per tsave | 2 FULL: the output of every factor pass (no recompute in the adjoint sweep;
// needs total_factors+1 states of HBM — e.g. 156 GiB for N=20, T=1000, which an MI355X's 288 GB holds) | 3 PARTIAL: one state per
// tsave + the intermediate factor outputs of the trailing intervals (`tape_entries` states in all, counted by the caller)
inline size_t carve(Plan& pl, int tape_mode, bool need_backward, int chain_slots, int64_t total_factors = 0, int64_t tape_entries = 0) {
    // factor table of the persistent small-N kernel: 40 bytes per factor pass
    pl.ptable_bytes = (pl.N <= 12 && !pl.shard_bits) ? size_t(total_factors) * 48 + 64 : 0;  // sizeof(PersistFactor)
    const size_t E = pl.stages.size();
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes);
        return o;
    };
    pl.off_stats = take(64 * sizeof(double));
    pl.off_meta_idx = take(E * 24);  // StageDev records (rydiff.hip)
    pl.off_members = take(2 * kMaxGroups * sizeof(uint64_t));
    pl.off_coef = take(size_t(pl.Bc) * E * std::max(pl.NC, 1) * sizeof(double));
    pl.off_udiag = take(pl.dim * sizeof(double) * (pl.shard_bits ? size_t(pl.B) : 1));  // sharded: one table per slab
    pl.off_buf0 = take(pl.state_bytes);
    pl.off_buf1 = take(pl.state_bytes);
    pl.off_pp0 = take(pl.state_bytes);  // partial vectors of the chained passes
    pl.off_pp1 = take(pl.state_bytes);
    if (!pl.shard_bits && pl.N > 12 && pl.N <= 20) {  // the w / t pair of the block-of-two passes (pair_kernels.hpp): pp0..pp3
        pl.off_pp2 = take(pl.state_bytes);
        pl.off_pp3 = take(pl.state_bytes);
    }
    // split interaction diagonal for the tile layouts: utt[3][2^LT] + vr[3][tiles][16] per tile size; one set per tile size
    // (LT = 10 .. 13: the forward and the adjoint chains pick their tile size independently)
    {   // (sharded runs index the table by the GLOBAL tile: 2^(N-LT) rows)
        const size_t gdim = size_t(1) << pl.N;
        size_t tot = 0;
        for (int lt = 10; lt <= 13; ++lt) {  // tile sizes 2^10 .. 2^13 amplitudes, up to three tile layouts each
            pl.split_off_doubles[lt - 10] = tot;
            tot += 3 * ((size_t(1) << lt) + ((gdim >> lt) ? (gdim >> lt) : 1) * 16);
        }
        pl.off_split = take(tot * sizeof(double));
    }
    pl.off_ptable = take(pl.ptable_bytes);
    if (pl.ptable_bytes) {
        pl.off_pm_begin = take(size_t(pl.T + 1) * sizeof(int32_t));
        pl.off_pm_first = take(size_t(pl.T + 1) * sizeof(int32_t));
        pl.off_pm_tau = take(E * sizeof(double));
        pl.off_pm_nsub = take(E * sizeof(int32_t));
    }
    pl.off_pair = take(size_t(pl.n_pair) * 64 * sizeof(double));
    pl.off_pauli = take(pl.pauli_bytes());
    // one-launch sweeps: the trajectory the Pauli and overlap observables are evaluated on (and the shots drawn from) where the
    // caller keeps none
    pl.off_pauli_traj = take(((pl.n_pobs || pl.n_ov || pl.n_rdm || pl.moments || pl.energy || pl.n_shots || pl.dm_rows()) && pl.N <= 12) ? size_t(pl.T + 1) * pl.state_bytes : 0);
    pl.off_dm = take(pl.dm_n ? pl.dm_bytes() : 0);  // string tables of the density-matrix observables
    pl.off_shot_sums = take(pl.n_shots ? size_t(pl.B) * pl.shot_chunks() * sizeof(double) : 0);
    pl.off_shot_prefix = take(pl.n_shots ? size_t(pl.B) * pl.shot_chunks() * sizeof(double) : 0);
    pl.off_moments = take((pl.moments && pl.moment_tiles() > 1) ? size_t(pl.B) * 79 * pl.moment_tiles() * sizeof(double) : 0);  // kMomEntries per tile
    if (pl.energy) {  // (nothing is taken with the block off: every other offset stays where it was)
        pl.off_energy_meta = take(size_t(pl.T + 1) * 24);  // StageDev records: column k with weight 1
        pl.off_energy_coef = take(size_t(pl.Bc) * (pl.T + 1) * std::max(pl.NC, 1) * sizeof(double));
        // partial sums [save points of one launch][B][workgroups][2]: up to 12 qubits one launch covers the whole trajectory
        pl.off_energy_part = take(size_t(pl.N <= 12 ? pl.T + 1 : 1) * pl.B * pl.energy_blocks() * 2 * sizeof(double));
    }
    pl.total_fwd = off;
    pl.tape_mode = tape_mode;
    if (tape_mode == 2) pl.off_tape = take(size_t(total_factors + 1) * pl.state_bytes);
    else if (tape_mode == 3) pl.off_tape = take(size_t(tape_entries) * pl.state_bytes);
    else pl.off_tape = tape_mode ? take(size_t(pl.T + 1) * pl.state_bytes) : 0;
    pl.chain_slots = chain_slots;
    if (need_backward) {
        pl.off_chain = take(size_t(chain_slots > 0 ? chain_slots : 1) * pl.state_bytes);
        pl.off_ge = take(size_t(pl.Bc) * E * 64 /* kGradReplicas */ * (pl.NC + 1) * sizeof(double));
        pl.off_wtot = take(pl.dim * (pl.shard_bits ? size_t(pl.B) : 1) * sizeof(double));  // sharded: one weight slab per rank of the call
        // observable cotangent grad_states[k] + 2 sum_o g_o O_o psi_k + sum_o (gRe + i gIm)_o phi_o: one state, reused in stream order
        // (one-launch adjoints: every k)
        pl.off_pauli_cot = take((pl.n_pobs || pl.n_ov || pl.n_rdm || pl.moments || pl.energy || pl.dm_rows()) ? size_t(pl.N <= 12 ? pl.T + 1 : 1) * pl.state_bytes : 0);
        pl.off_meta2 = take(std::max(E * 40, size_t(pl.T + 1) * sizeof(int32_t)));  // StageBwdDev records, or the save-point flags of the one-launch adjoint
        if (pl.energy) {  // z = g_E psi + g_M H_k psi (one state; one-launch adjoints: every k) and the records [Bc][n_tsave][replica][NC]
            pl.off_energy_z = take(size_t(pl.N <= 12 ? pl.T + 1 : 1) * pl.state_bytes);
            pl.off_energy_ge = take(size_t(pl.Bc) * (pl.T + 1) * kEnergyReplicas * std::max(pl.NC, 1) * sizeof(double));
        }
        pl.off_xy_ge = take(pl.xy_mode ? size_t(kXyReplicas) * (pl.N * (pl.N - 1) / 2) * sizeof(double) : 0);  // XY gradient replicas (zeroed by rydiff_backward)
    }
    return off;
}

}  // namespace rydiff
