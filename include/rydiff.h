/*
 * rydiff.h — C ABI of the MI355X-native differentiable Rydberg time-evolution library.
 *
 * This is the drop-in boundary for ONE hot path of pasqal-io/pulser-diff: the solver seam
 *
 *     pulser_diff/backend.py:488-494      result = sesolve(H=H_t, psi0, tsave, solver, options)
 *
 * together with the Hamiltonian closure it calls on every sub-step
 *
 *     pulser_diff/hamiltonian.py:499-548  build_ham_tensor(qobj_list) -> H_t(t)
 *
 * and the observable / autograd legs that hang off it
 *
 *     pulser_diff/utils.py:68-86          expect(obs, states)        (ket branch :79-81)
 *     pulser_diff/derivative.py:40,76     torch.autograd.grad(f, x, v, retain_graph=True)
 *
 * The reference hands the solver an opaque Python callable H_t that re-assembles a sparse
 * 2^N x 2^N matrix per call.  This library replaces seam + closure by a STRUCTURED problem:
 * the coefficient arrays the reference captures in `build_ham_tensor` (amp_values /
 * det_values, hamiltonian.py:507-520), the qubits each operator acts on, the pair
 * interaction strengths (hamiltonian.py:343, :536), dt and n_samples (hamiltonian.py:523-524),
 * tsave and psi0 (backend.py:490-491).  H is never materialised.
 *
 * Conventions (fixed by the reference):
 *   - basis r=0, g=1 per qubit; qubit 0 is the MOST significant bit of the amplitude index
 *     (hamiltonian.py:299, utils.py:127-129);  n_j(x) = 1 - bit_j(x).
 *   - (H psi)[x] = [sum_{i<j} U_ij n_i n_j + sum_terms 2*det_k(t) * sum_{j in mask_k} n_j] psi[x]
 *                  + sum_terms sum_{j in mask_k} ( amp_k(t) if bit_j(x)=1 else conj(amp_k(t)) ) psi[x ^ m_j]
 *     where amp_k = 0.5*Omega*exp(-i*phi) and det_k = -0.5*delta are the reference's own
 *     coefficient arrays (hamiltonian.py:420-423, 439-442) and the factor 2 is its
 *     `ham_mat + ham_mat.adjoint()` on a diagonal operator (hamiltonian.py:539-540).
 *   - coefficient at time t: linear interpolation between samples i1 = max(min(floor(t/dt), n-2), 0)
 *     and i2 = min(i1+1, n-2) (hamiltonian.py:532-542).
 *   - states are complex128, laid out (n_tsave, batch, 2^N) with the amplitude index fastest;
 *     the reference's (n_t, dim, B) (simresults.py:398-401) is the permuted view.
 *
 * Ownership: every pointer marked DEVICE is device memory owned by the caller (torch);
 * pointers marked HOST are host memory.  The library allocates nothing on the device: the
 * caller passes a workspace sized by rydiff_plan().  All work is enqueued on `stream`.
 * Functions return 0 on success, a negative RYDIFF_E* code otherwise; rydiff_last_error()
 * gives the message (thread-local).  The library never aborts.
 *
 * Threads and streams: the library keeps NO mutable process state besides the thread-local error string (and a
 * mutex-protected cache of polynomial designs, which only saves host time).  Every choice that steers a call — including
 * the kernel family (RydProblem.kernel_variant) — travels in the RydProblem, so concurrent calls from different threads on
 * different streams with distinct workspaces are independent.  rydiff_forward / rydiff_backward given a RydPlanInfo are
 * fully ASYNCHRONOUS: they only enqueue work (host-side metadata reaches the device as kernel arguments, never through
 * pageable-memory copies) and never synchronise the stream.  rydiff_plan is the one call that waits: the spectral bounds it
 * computes on the device decide the polynomial degree, i.e. how many launches the host has to enqueue.
 */
#ifndef RYDIFF_H
#define RYDIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RYDIFF_MAX_QUBITS 30
#define RYDIFF_MAX_PAIR_TERMS 28
#define RYDIFF_MAX_TERMS 64
#define RYDIFF_MAX_PAULI_STRINGS 1024 /* Pauli strings of one call, over all Pauli observables (after any frame rotation) */
#define RYDIFF_MAX_OVERLAPS 16 /* state-overlap observables (target states) of one call */
#define RYDIFF_MAX_RDMS 8        /* reduced density matrices of one call */
#define RYDIFF_MAX_RDM_QUBITS 6  /* qubits of one reduced density matrix */
#define RYDIFF_MAX_DM_ATOMS 12   /* atoms of a density-matrix register (RydProblem.dm_atoms): 4^12 amplitudes */
#define RYDIFF_MAX_DM_DIAG 64    /* diagonal observables of a density-matrix register */

enum { RYDIFF_OK = 0, RYDIFF_EINVAL = -1, RYDIFF_EWORKSPACE = -2, RYDIFF_EHIP = -3, RYDIFF_ENOTIMPL = -4 };

/* SolverType member names mirror pyqtorch.utils.SolverType as used at backend.py:434,487. */
enum { RYDIFF_SOLVER_KRYLOV_SE = 0, RYDIFF_SOLVER_DP5_SE = 1 };

typedef struct RydProblem {
    int32_t n_qubits;      /* N, 1..RYDIFF_MAX_QUBITS */
    int32_t batch;         /* B: number of state columns / trajectories (backend.py:266-280: psi0 is (dim, B)) */
    int32_t coeff_batch;   /* 1: all trajectories share the coefficient tables; B: one table set per trajectory */
    int32_t n_samples;     /* n: length of every coefficient array (hamiltonian.py:524) */
    double dt;             /* 0.001 / sampling_rate, in us (hamiltonian.py:523) */

    int32_t n_amp_terms;   /* off-diagonal terms ("amp_matrices", hamiltonian.py:517-520) */
    int32_t n_det_terms;   /* diagonal terms ("det_matrices", hamiltonian.py:513-516) */
    const uint32_t* amp_masks;  /* HOST [n_amp_terms]; bit j set = term acts on qubit j (global = all qubits, backend.py:102-112) */
    const uint32_t* det_masks;  /* HOST [n_det_terms] */
    const void* amp_tables;     /* DEVICE complex128 [coeff_batch][n_amp_terms][n_samples] = 0.5*amp*exp(-i*phase) */
    const double* det_tables;   /* DEVICE float64    [coeff_batch][n_det_terms][n_samples] = -0.5*det */
    const double* u_pairs;      /* DEVICE float64 [N(N-1)/2], U_ij = C6/r_ij^6 in itertools.combinations order (hamiltonian.py:385) */

    int32_t n_tsave;       /* number of evaluation times (backend.py:364-373), >= 2 */
    const double* tsave;   /* HOST float64 [n_tsave], strictly increasing, in us */

    int32_t solver;        /* RYDIFF_SOLVER_* */
    double tol;            /* per-exponential truncation target (<=0: default 1e-13) */

    int32_t n_obs;         /* diagonal observables evaluated at every tsave (utils.py:79-81 for diagonal O) */
    const double* obs_diag;/* DEVICE float64 [n_obs][2^N] */

    /* Optional dense two-qubit terms of the generator M in d/dt v = -i M(t) v — how the master-equation path
     * (backend.py:495-509, SolverType.DP5_ME) runs on this library: rho is the state of a DOUBLED register (row qubits,
     * column qubits), the commutator is an ordinary structured "Hamiltonian" on it, and every collapse operator acting
     * on qubit j contributes a constant 4x4 block on the pair (row qubit j, column qubit j):
     *   (M v)[x] += sum_{s=0..3} T_p[4*own + s] * v[x with the bits of qubits (a_p, b_p) set to s],
     * own / s = 2*bit(a_p) + bit(b_p).  M need not be Hermitian.  Problems with pair terms run on the persistent (N <= 12)
     * or direct kernels. */
    int32_t n_pair_terms;          /* 0..RYDIFF_MAX_PAIR_TERMS */
    const uint32_t* pair_qubits;   /* HOST [n_pair_terms][2]: (a_p, b_p), a_p != b_p */
    const double* pair_tables;     /* HOST complex128 as (re, im) [n_pair_terms][16] */

    /* rydiff_backward only.  != 0: the caller uses only the REAL part of g_amp — its amplitude tables were built from
     * real-valued data (a drive without phase; the reference's 0.5*amp*exp(-1j*phase), hamiltonian.py:420, with phase 0).
     * When in addition every table entry is real (RydPlanInfo.flags bit 0 clear) the chained adjoint passes skip the signed
     * partner sums and the contractions for dL/dIm(amp); the imaginary parts of g_amp are then not computed (zero). */
    int32_t real_amp_grad;

    /* Kernel family, 0 = automatic (what production callers pass).  Non-zero values force one implementation so that
     * parity tests can compare the families with each other and with the oracle, and tuning scripts can time them:
     *   1 direct (one amplitude per thread, global partner loads)       9 direct, always the generic kernels
     *   2 / 3 / 4 LDS-tiled chained passes with 512 / 256 / 1024 threads per tile (13 <= N <= 28; two tile layouts up to
     *             N = 22, three from N = 23)
     *   7 automatic, but three tile layouts wherever they are legal (21 <= N <= 28)
     *   8 automatic, but the LDS-tile persistent kernels also up to 6 qubits (instead of the one-wave lane kernels)
     *  10 chained passes with trajectory-per-XCD placement forced (L2-resident trajectories)
     *  11 automatic, but TWO tile layouts up to 24 qubits (32- / 16-byte runs in the second layout at 23 / 24 qubits)
     *  12 automatic, but tiles in plain workgroup order (no line-sharing swizzle where a layout's runs are shorter than 128 bytes)
     *  13 automatic, but 2^12-amplitude tiles everywhere (automatic takes 2^13-amplitude "wide" tiles — k_chain_wide, DESIGN.md
     *     section 3 — with two layouts at 21..24 qubits and with three at 29 and 30, where variant 13 falls back to the direct kernels)
     *  14 chained passes with wide tiles wherever they are legal (14 <= N <= 30; three layouts from 25)
     *  15 / 16 chained passes with tiles of 2^11 / 2^10 amplitudes where two layouts of them are legal (12 <= N <= 20 / 11 <= N <= 18;
     *     automatic takes the 2^11 tiles around 2^19 amplitudes in flight: 256 tiles, one per CU)
     *  17 chains in blocks of two factors per launch (k_chain2 forward, k_chain2_bwd adjoint) wherever they are
     *     legal: one phase-free global drive, at most one detuning group, 13 <= N <= 20, un-sharded; forward with no tape or the full
     *     tape, adjoint with real_amp_grad (automatic: one 20-qubit trajectory)
     *  18 automatic, but one factor per launch (k_chain) everywhere
     *  19 automatic, but one factor per adjoint launch (forward blocks as automatic)
     *  20 / 21 as 17, with the adjoint block kernel's tape vectors staged through registers / by LDS-DMA (DESIGN.md section 3;
     *     17 and automatic take the one that measured faster)
     *  22..30 as 20, with a request order and a store policy of the block kernels' own: inputs requested vector-major (v of every wave,
     *     then w, then t / the tape) and / or some outputs stored write-through (level 1: v_mid and y, adjoint mu_out; 2: also w';
     *     3: all).  22 vector-major | 23 / 24 / 25 write-through level 1 / 2 / 3 | 26 / 27 / 28 both | 29 vector-major with LDS-DMA
     *     staging and streaming stores | 30 neither (wave-major requests, streaming stores).  DESIGN.md section 3; automatic, 17, 20
     *     and 21 take the combination that measured fastest (that of 28)
     *  31..34 as 20, with PACED input requests: a wave requests w (adjoint: w and x_a) only once half of its v
     *     (mu) is back, awaits v alone for the first finishing round, and requests t behind that round once half of its w is back.
     *     31 forward | 32 adjoint | 33 both | 34 forward, with t requested before the first round instead.  17 and 20..30 never pace;
     *     automatic takes the paced adjoint kernel (that of 32) and the unpaced forward kernel
     *  35 as 20, with "w on the tape" (DESIGN.md section 3): where the full tape is read by the adjoint block kernel alone, the slot
     *     between the two factors of a block holds the forward block's own partial sum P_X v and not the mid-block state, which the
     *     adjoint kernel rebuilds with one more partner-sum round (forward 3R+3W instead of 3R+4W per block).  The backward call must
     *     be made with the kernel_variant and real_amp_grad of the forward call that wrote the tape: a tape of the other format is
     *     refused (RYDIFF_EINVAL).  17 and 19..34 keep the mid-block state on the tape
     * "automatic" takes the one-launch sweeps up to 12 qubits, the direct kernels while few tiles are in flight
     * (B * 2^N <= 2^18, with gradients 2^19) and the chained passes beyond.  Results do not depend on the variant beyond rounding. */
    int32_t kernel_variant;

    /* STATE-SHARDED runs (BASELINE config 5; the reference has no counterpart: it keeps the whole
     * state in one process).  shard_bits = g > 0: the top g qubits (qubits 0..g-1 = the top g bits of the amplitude index)
     * select the RANK; every rank owns a contiguous slab of 2^(N-g) amplitudes.  n_qubits, the masks and u_pairs describe the
     * WHOLE register; `batch` = number of ranks whose slabs are part of THIS call, rank ids shard_rank_first ... + batch - 1,
     * and psi0 / states_out / obs_diag are laid out per slab: [batch][2^(N-g)] (obs_diag: [n_obs][batch][2^(N-g)]).
     * expect_out [n_obs][n_tsave][batch] receives every slab's PARTIAL sum (the caller adds them / all-reduces them).
     * One factor pass = the local pass on the N-g slab qubits (same kernels, diagonal evaluated at the global index) plus
     * beta * (c or conj c) * the partner rank's slab for each of the g rank qubits (partner of rank bit k: rank ^ (1 << k)):
     *   - batch == 2^g (every rank in this call, e.g. all of them on one device): partners are read in place;
     *   - otherwise shard_recv[k] (HOST array of g DEVICE buffers of 2^(N-g) amplitudes) must hold the partner's current slab
     *     whenever a pass needs it, and shard_exchange says when: it is called (on the calling thread) with phase 0 right
     *     after the launch that produced the slab `src` (nbytes) which the partners need next — post the sends of `src` and
     *     the receives into shard_recv[] there, ordered after the work enqueued on `stream` so far — and with phase 1 before
     *     the first launch that reads shard_recv[] — make `stream` wait for those receives there.  Every phase 0 is followed by
     *     exactly ONE phase 1 before the next phase 0; more than one launch may read shard_recv[] after it (with g_tsave the
     *     dL/dtau pass at an exponential's output and the completing adjoint launch read the same received slabs).  The library runs the whole
     *     trajectory (every step, every factor) in ONE call and never touches the transport itself (torch.distributed /
     *     RCCL stay with the caller).  A non-zero return aborts the run with RYDIFF_EHIP.
     * GRADIENTS (round 3): rydiff_forward with need_tape (the slabs' trajectory in the workspace tape) followed by rydiff_backward runs
     * the whole reverse sweep natively as well.  The cotangent slabs take the SAME exchange (shard_exchange is called for them exactly as
     * for the state slabs, phase 0 / phase 1), the drive gradients of the rank qubits are contracted with the partner slabs inside the
     * completing launch, grad_expect is [n_obs][n_tsave][batch] (the cotangent of every slab's partial sum: normally the same number for
     * all slabs) and g_amp / g_det / g_u / g_tsave receive this call's PARTIAL sums (the caller adds them over the ranks: one
     * all-reduce of the tiny arrays); g_psi0 is [batch][2^(N-g)].  g_tsave costs one pass per exponential and NO slab exchange:
     * Im<mu, H x_out> is taken as Im<H mu, x_out> (H is Hermitian: no pair terms here), and the partners' copies of the cotangent
     * mu are the ones the next adjoint launch needs anyway.
     * No pair terms, 1 <= N-g, N <= RYDIFF_MAX_QUBITS. */
    int32_t shard_bits;
    int32_t shard_rank_first;
    void* const* shard_recv;
    int (*shard_exchange)(void* user, int phase, const void* src, size_t nbytes);
    void* shard_user;

    /* rydiff_forward: != 0: states_out is [1][B][2^N] and receives only the state at the LAST evaluation time (a 24-qubit
     * trajectory would otherwise need n_tsave x 256 MiB).  Launch-per-factor kernels only (more than 12 qubits, or a
     * state-sharded run); not together with need_tape. */
    int32_t final_state_only;

    /* Three-level registers (the reference's basis "all": r, g, h, hamiltonian.py:306-310) run as TWO qubits per atom — atom i =
     * qubits (2i, 2i+1) = (a_i, b_i) with r = (0,1), g = (1,1), h = (1,0); the code (0,0) is never populated — with two
     * generalisations of the terms above, both bit masks over TERM indices (bit k = term k):
     *   amp_conditioned_terms: the flip of qubit j by term k acts only on amplitudes whose SIBLING qubit (j ^ 1) is in state 1:
     *       g <-> r flips a_i where b_i = 1, g <-> h flips b_i where a_i = 1, and neither leaves the three valid codes;
     *   det_ones_terms: term k weights the qubits of its mask that are in state 1 with MINUS its coefficient, i.e. contributes
     *       2*det_k(t) * (0 - #ones) instead of 2*det_k(t) * (#zeros): on the valid codes n_g = a_i + b_i - 1, so the reference's
     *       detuning on sigma_gg (hamiltonian.py:413) is an ordinary term on the a qubits plus a ones-counting term on the b qubits.
     * All terms that address one qubit must agree on these flags; n_qubits must be even when any term is conditioned.  Such
     * problems run on the one-launch kernels up to 12 qubits, beyond that on the generic one-amplitude-per-thread kernels and — with
     * enough tiles in flight, up to 20 qubits — on the chained passes over 2^12-amplitude tiles (forward, adjoint, every gradient). */
    uint64_t amp_conditioned_terms;
    uint64_t det_ones_terms;

    /* ENERGY OBSERVABLES: the expectation of the run's own Hamiltonian and its second moment at every tsave, from the state while
     * it is on the device — the score of a state-preparation or annealing sequence that needs no target state, and (as the variance
     * M2 - E^2) the distance from any eigenstate.  H_k is the Hamiltonian the factor passes apply (same groups, masks, diagonal rule,
     * u_pairs, and with xy_mode = 1 the Hermitian exchange with xy_pairs), built from COLUMN k of two tables the caller interpolates
     * to the save points itself:
     *   E[k][b]  = Re sum_x conj(psi[x]) (H_k psi)[x]        M2[k][b] = sum_x |(H_k psi)[x]|^2        (psi = psi_b(t_k), not normalised)
     * energy_rows = 1 adds the row E, 2 the rows E then M2, to expect_out / grad_expect BEHIND the bit_moments block (the last block
     * of a ket's rows, in front of the density-matrix rows).  Every workgroup writes its two partial sums to the workspace and a
     * second launch adds them in index order (no atomics): two calls on the same input give bit-identical rows, and every row is
     * written.  rydiff_plan adds the scratch to workspace_bytes: the (n_tsave) coefficient records and the partial sums, for
     * rydiff_backward one more state per trajectory (n_tsave of them up to 12 qubits) and the gradient records.
     * rydiff_backward, with g_E, g_M the rows of grad_expect at (k, b) (g_M = 0 with one row): the cotangent added to psi_b(t_k) is
     *   2 H_k (g_E psi + g_M H_k psi)                                       (the factor-2 convention of the diagonal rows)
     * formed in two passes (z = g_E psi + g_M H_k psi into the scratch state, then 2 H_k z) in the workspace buffer of the Pauli /
     * overlap / RDM / moment cotangents (after them) and injected through the grad_states route.  The EXPLICIT derivative w.r.t. a
     * coefficient c of H_k, Re<g_E psi + 2 g_M H_k psi| dH_k/dc |psi>, goes for the drive and detuning coefficients to column k of
     * g_energy_amp / g_energy_det (members of a group as in g_amp / g_det; both parts of g_energy_amp whatever real_amp_grad says),
     * for u_pairs into g_u and for xy_pairs into g_xy, in their plain units dL/dU_p, dL/dJ_p, next to what the factor passes put there.
     * Honoured wherever bit_moments is: every kernel family and kernel_variant (the block reads save-point states only: up to 12
     * qubits the trajectory the one-launch sweeps leave in the workspace), every tape mode, final_state_only, states_out == NULL
     * without a tape, batch / coeff_batch, next to every other ket row and the shots, N = 1 .. RYDIFF_MAX_QUBITS.  One kernel family
     * of its own (energy_kernels.hpp) in two versions, energy_kernel: direct (one amplitude per thread, partners from global memory,
     * as k_dot_hx; every N, and the only one with the exchange) and LDS-tile (13 .. 24 qubits).
     * RYDIFF_EINVAL: energy_rows outside 0..2; energy_amp == NULL with n_amp_terms > 0; energy_det == NULL with n_det_terms > 0.
     * RYDIFF_ENOTIMPL, before anything touches a device: energy_rows > 0 together with n_pair_terms > 0, dm_atoms > 0, shard_bits > 0,
     * conditioned or ones-counting terms, xy_mode = 2 (the expectation of a non-Hermitian generator is not an energy), and in
     * rydiff_forward_tangent / rydiff_forward_geometry / rydiff_forward_fisher.  Follow-ups, not built: the Tr(rho H) rows of
     * master-equation runs (dm_atoms > 0) and the tangents of the rows in the tangent sweep.
     * energy_rows = 0: the other five fields are ignored and nothing changes.  (The fields sit in front of xy_mode: every later block
     * keeps its neighbours, and the Pauli block stays the tail of the struct.) */
    int32_t energy_rows;       /* 0: off; 1: E; 2: E then M2 */
    const void* energy_amp;    /* DEVICE complex128 [coeff_batch][n_amp_terms][n_tsave]: 0.5*amp*exp(-i*phase) AT the save points */
    const double* energy_det;  /* DEVICE float64    [coeff_batch][n_det_terms][n_tsave]: -0.5*det AT the save points */
    void* g_energy_amp;        /* rydiff_backward: DEVICE complex128, the shape of energy_amp, or NULL; overwritten */
    double* g_energy_det;      /* rydiff_backward: DEVICE float64, the shape of energy_det, or NULL; overwritten */
    int32_t energy_kernel;     /* 0: automatic (what production callers pass); 1: the direct version (one amplitude per thread, every N);
                                * 2: the LDS-tile version (2^12 amplitudes staged per workgroup; 13 <= N <= 24, xy_mode = 0: elsewhere
                                * RYDIFF_ENOTIMPL) — for parity tests and timing, like kernel_variant.  Results do not depend on it
                                * beyond rounding.  RYDIFF_EINVAL outside 0..2 (with energy_rows > 0; ignored with energy_rows = 0) */

    /* XY EXCHANGE (the reference's microwave / "XY" interaction mode, hamiltonian.py:346-366) as a term of its own: one real number
     * per pair of qubits and one partner amplitude, instead of a dense 4x4 pair term.  With b_q(x) the index bit of qubit q (bit
     * N-1-q of the amplitude index x) and m_q = 1 << (N-1-q):
     *   xy_mode = 1 (Hermitian):  (H v)[x] += sum_{i<j, b_i(x) != b_j(x)} J_ij * v[x ^ m_i ^ m_j]
     *   xy_mode = 2 (one-directional, as the reference writes it: its 2 * int_mat without the adjoint): only the rows with
     *               b_i(x) = 0 and b_j(x) = 1 for i < j are kept — source |d_i u_j>, target |u_i d_j>, the pair-term block[1][2] = J.
     * J_ij is the full coefficient of the generator (the reference's 2 U); real, any sign, zero allowed; shared by the trajectories
     * like u_pairs, next to which it may be used (u_pairs != 0 is fine).  Runs on the direct family (launch per factor, kernels of its
     * own: xy_kernels.hpp) at every N from 1 to RYDIFF_MAX_QUBITS, RydPlanInfo.kernel_family = 2; kernel_variant 0, 1 and 9 only.
     * need_tape = 2 / 3 are downgraded to 1 as for pair terms.  batch / coeff_batch, every ket observable row and the shots are
     * honoured (they read states at save points only).  rydiff_plan reads xy_pairs in the kernel that inspects the tables (still
     * one synchronisation) and widens the spectral interval by sum |J_ij| on either side — a Gershgorin bound on the exchange rows;
     * in mode 2 (H not Hermitian) it bounds the numerical range, as the radius of non-Hermitian pair terms does.
     * rydiff_backward delivers g_amp, g_det, g_u, g_tsave, g_psi0 as usual (the Im<mu, H x> pass carries the exchange on x: no side
     * swap, H need not be Hermitian) and g_xy[p] = dL/dJ_p through every factor pass with the plan constants frozen — the discrete
     * map that g_u differentiates, scaled like it under KRYLOV_SE, DP5_SE and sub-stepped exponentials.  It sits in the struct so
     * that the signature of rydiff_backward stays.  Every workgroup reduces its N(N-1)/2 contributions and adds them with one atomic
     * per pair into a few replicas in the workspace (zeroed by the call; rydiff_plan sizes them), summed in a fixed order at the end:
     * g_xy is overwritten, and two calls agree up to the rounding of the order in which the atomics land.
     * RYDIFF_EINVAL: xy_mode outside 0..2; xy_pairs == NULL with xy_mode != 0 and N > 1.  RYDIFF_ENOTIMPL, before anything touches a
     * device: xy_mode != 0 together with n_pair_terms > 0, shard_bits > 0, dm_atoms > 0, conditioned or ones-counting terms, a
     * kernel_variant other than 0, 1, 9, in rydiff_apply_factor, and in rydiff_forward_tangent / rydiff_forward_geometry /
     * rydiff_forward_fisher unless RydTangent.flags has RYDIFF_TANGENT_XY (the tangent sweep with the exchange stencil; the tangents of
     * xy_pairs are RydTangent.d_xy).  Follow-up: the one-launch sweeps up to 12 qubits.
     * xy_mode = 0: the other two fields are ignored and nothing changes.  (The fields sit in front of dp5_piece_refine: every later
     * block keeps its neighbours, and the Pauli block stays the tail of the struct.) */
    int32_t xy_mode;          /* 0: none; 1: Hermitian exchange; 2: one-directional, as the reference writes it */
    const double* xy_pairs;   /* DEVICE float64 [N(N-1)/2], J_ij in itertools.combinations order (the order of u_pairs) */
    double* g_xy;             /* rydiff_backward: DEVICE float64 [N(N-1)/2] or NULL; overwritten */

    /* RYDIFF_SOLVER_DP5_SE only, optional (NULL: none).  HOST uint8 [n_samples - 1]: entry i multiplies the number of Magnus
     * sub-steps taken on the linear piece between samples i and i + 1 (0 and 1: unchanged).  The sub-step is sized from the
     * generator's width; the error constant also carries dH/dt, so a piece across which a table JUMPS (the edge of a constant
     * pulse inside one sample interval) wants a finer step than the smooth pieces — a caller that builds the tables on the host
     * knows where that is (pulser-diff_amd/hamiltonian.py: piece_refinement) and the library does not have to read them back. */
    const uint8_t* dp5_piece_refine;

    /* OCCUPATION CORRELATIONS OF A DENSITY-MATRIX REGISTER (dm_atoms = n > 0, below): the bit moments of the diagonal of rho.  With
     * v = vec(rho), p[x] = Re v[x (2^n + 1)] (x < 2^n) and x_q the index bit of atom q (atom q <-> bit n-1-q of x):
     *   S = sum_x p[x],   B_q = sum_x p[x] x_q  (q = 0..n-1),   B_qr = sum_x p[x] x_q x_r  (0 <= q < r < n)
     * dm_moments = 1 adds 1 + n + n(n-1)/2 rows to expect_out / grad_expect BEHIND the dm_rdm rows (the last block of all): S, then
     * B_q in ascending q, then B_qr in lexicographic (q, r) — the order of the ket block of bit_moments with N = n.  p is NOT clamped
     * (the shots clamp, these rows do not): every row is linear in rho, and rho is assumed neither Hermitian nor normalised.  One
     * workgroup per (save point, trajectory) forms all rows in float64 in one fixed order (no atomics): two calls on the same input
     * give bit-identical rows, and every row is written.  rydiff_backward: with g the rows of grad_expect at (k, b), the cotangent
     * added to Re v[x (2^n + 1)] is q(x) = g_S + sum_q g_q x_q + sum_{q<r} g_qr x_q x_r (factor 1, the convention of the dm_diag
     * rows), added behind the other density-matrix cotangents in the same workspace buffer.  Honoured wherever the other dm_* rows
     * are: every kernel family, every tape mode, states_out == NULL without a tape.  rydiff_forward_tangent (with
     * RYDIFF_TANGENT_DENSITY_MATRIX): the rows are linear, so the rows of dexpect_out are the same kernel on d rho_d.  RYDIFF_EINVAL:
     * a value other than 0 or 1 (with dm_atoms > 0).  bit_moments keeps its meaning (kets) and stays RYDIFF_ENOTIMPL with
     * dm_atoms > 0.  Traffic per state: the 2^n real parts of the diagonal (2^n * 8 B); nothing of size 2^n or 4^n is written.
     * dm_atoms = 0: the field is ignored, like the other dm_* fields.  dm_moments = 0: nothing changes.  (The field sits in front of
     * n_shots: the shot block, the 14 fields dm_atoms .. dm_shots, the overlap block and the Pauli block keep their neighbours.) */
    int32_t dm_moments;           /* 0: off; 1: all atoms */

    /* MEASUREMENT SHOTS: amplitude indices sampled from |psi_b(t_k)|^2 at chosen save points by rydiff_forward, while the state is
     * on the device — no stored trajectory, no 2^N probabilities on the host.  The caller supplies the uniforms (its own generator and
     * seeding), which makes the rule deterministic.  For sampled save point k, trajectory b, shot s with uniform u:
     *   p[y] = |psi_b(t_k)[y]|^2,   C[x] = sum_{y <= x} p[y],   S = C[2^N - 1];   result = the smallest x with C[x] > u * S
     * with u clamped into [0, 1) (anything not > 0, NaN included, counts as 0).  Where rounding leaves no such x the result is the
     * largest x with p[x] > 0; an x with p[x] == 0 is never returned; S == 0 gives RYDIFF_SHOT_NONE.  The state need not be
     * normalised; result s belongs to uniform s (no sorting asked of the caller).  The cumulative sums are formed in float64 in a fixed
     * order (bit-reproducible; within (2^N - 1) * 2^-53 * S of the exact ones).
     * Honoured by rydiff_forward in every kernel family and with every tape mode — final_state_only, states_out == NULL without a
     * tape, next to diagonal / Pauli / overlap observables, pair terms, conditioned and ones-counting terms.  rydiff_backward ignores
     * the values (shots carry no gradient) but must be given the same counts as the forward call: rydiff_plan adds the scratch they
     * need to workspace_bytes (two doubles per 2^10 amplitudes and trajectory, and up to 12 qubits the trajectory the one-launch sweeps
     * are sampled from where the caller keeps none).  Not together with shard_bits > 0 and not in rydiff_forward_tangent
     * (RYDIFF_ENOTIMPL).  Traffic per sampled save point and trajectory: one read of the state plus at most n_shots * 16 KiB; the state
     * is never written.  n_shots = 0: nothing changes.  (The fields sit in front of tape_steps and the overlap block, so the Pauli block
     * stays the tail of the struct.) */
#define RYDIFF_MAX_SHOTS (1 << 20)   /* shots per (sampled save point, trajectory) */
#define RYDIFF_SHOT_NONE 0xFFFFFFFFu /* the sampled state was identically zero */
    int32_t n_shots;              /* 0: none */
    int32_t n_shot_times;         /* 1 .. n_tsave */
    const int32_t* shot_times;    /* HOST [n_shot_times]: save-point indices, strictly increasing, 0 .. n_tsave-1 */
    const double* shot_uniforms;  /* DEVICE float64 [n_shot_times][B][n_shots], in any order */
    uint32_t* shots_out;          /* DEVICE [n_shot_times][B][n_shots]: amplitude indices */

    /* OCCUPATION CORRELATIONS (bit moments): with p[y] = |psi_b(t_k)[y]|^2 and y_q the index bit of qubit q (qubit q <-> index bit
     * N-1-q), evaluated at every tsave from ONE read of the state and differentiated by rydiff_backward:
     *   S = sum_y p[y],   B_q = sum_y p[y] y_q  (q = 0..N-1),   B_qr = sum_y p[y] y_q y_r  (0 <= q < r < N)
     * bit_moments = 1 adds 1 + N + N(N-1)/2 rows to expect_out / grad_expect BEHIND the reduced-density-matrix rows (the last
     * block of a ket's rows): S, then B_q in ascending q, then B_qr in lexicographic (q, r) — pair (q, r) at offset
     * 1 + N + q(2N-q-1)/2 + (r-q-1).  S is a row of its own because the state need not be normalised.  Every sum is formed in
     * float64 in one fixed order (no atomics): two calls on the same input give bit-identical rows.  rydiff_backward: with g the
     * rows of grad_expect at (k, b), the cotangent added to psi_b(t_k) is 2 q(y) psi[y], q(y) = g_S + sum_q g_q y_q +
     * sum_{q<r} g_qr y_q y_r, formed per save point in the workspace buffer of the Pauli / overlap / RDM cotangents (after them)
     * and injected through the grad_states route.  Honoured by rydiff_forward in every kernel family and with every tape mode
     * next to every other ket row, shots, pair terms, conditioned and ones-counting terms (plain bits at this level).  Beyond 12
     * qubits rydiff_plan adds 79 doubles per 2^12 amplitudes and trajectory to workspace_bytes.  RYDIFF_EINVAL: a value other
     * than 0 or 1.  RYDIFF_ENOTIMPL: together with shard_bits > 0, with dm_atoms > 0, and in rydiff_forward_tangent /
     * rydiff_forward_geometry without RYDIFF_TANGENT_MOMENTS in RydTangent.flags (with it: values and tangents at every save
     * point).  Traffic per state: one read; nothing of size 2^N is written.  bit_moments = 0: nothing changes.
     * (The field sits in front of n_rdms, so every later block keeps its place relative to its neighbours.) */
    int32_t bit_moments;          /* 0: off; 1: all qubits */

    /* REDUCED DENSITY MATRICES: the state of a subsystem A of m distinct qubits (1 <= m <= RYDIFF_MAX_RDM_QUBITS), the rest E traced out,
     * evaluated at every tsave behind the overlap rows and differentiated by rydiff_backward:
     *   rho_o[a][a'] = sum_e psi[idx(a, e)] conj(psi[idx(a', e)])          (= Tr_E |psi><psi|, not normalised by the library)
     * rdm_masks[o]: the qubits of A in the convention of amp_masks (bit j = qubit j); a enumerates their settings with the
     * lowest-numbered qubit most significant.  expect_out and grad_expect become
     *   [n_obs + n_pauli_obs + 2 * n_overlaps + 2 * sum_o 4^{m_o}][n_tsave][B]:
     * RDM o owns 2 * 4^{m_o} consecutive rows behind the overlap rows, entry (a, a') at offset 2 * (a * 2^m + a'), Re then Im.  All
     * entries are written: the lower triangle is the conjugate of the upper one and Im rho[a][a] is an exact 0.  Every entry is an
     * independent output for rydiff_backward: with G = gRe + i gIm (2^m x 2^m, the RDM's rows of grad_expect at (k, b)) the
     * cotangent added to psi_b(t_k) is ((G + G^dagger)_A (x) 1_E) psi_b(t_k), formed per save point in the workspace buffer of the
     * Pauli and overlap cotangents (after them) and injected through the grad_states route.  Honoured by rydiff_forward in every
     * kernel family and with every tape mode — final_state_only, states_out == NULL without a tape — next to diagonal, Pauli and
     * overlap observables, shots, pair terms and conditioned terms.  Not together with shard_bits > 0 and not in
     * rydiff_forward_tangent (RYDIFF_ENOTIMPL).  RYDIFF_EINVAL: a count outside [0, RYDIFF_MAX_RDMS], an empty mask, more than
     * RYDIFF_MAX_RDM_QUBITS bits in a mask, bits at or above N.  Cost per RDM and state: one read of the state, 8 * 2^(N+m) flops.
     * n_rdms = 0: nothing changes.  (The fields sit in front of tape_steps and the overlap block, so the Pauli block stays the tail of the struct.) */
    int32_t n_rdms;                 /* 0: none; at most RYDIFF_MAX_RDMS */
    const uint32_t* rdm_masks;      /* HOST [n_rdms] */

    /* REDUCED DENSITY MATRICES OF A DENSITY-MATRIX REGISTER (dm_atoms = n > 0, below): the state of a subsystem A of m distinct ATOMS
     * (1 <= m <= min(n, RYDIFF_MAX_RDM_QUBITS)), the other atoms E traced out, evaluated at every tsave and differentiated by
     * rydiff_backward.  With v = vec(rho), v[x * 2^n + y] = rho[x][y], atom j <-> bit n-1-j of an atom index:
     *   rho_o[a][a'] = sum_e v[idx(a, e) * 2^n + idx(a', e)]                                (= Tr_E rho)
     * dm_rdm_masks[o]: the atoms of A (bit j = ATOM j, all below n); a enumerates their settings with the lowest-numbered atom most
     * significant — the convention of the ket block above.  rho is assumed neither Hermitian nor normalised: all 4^m complex entries
     * are computed independently, each a float64 sum of its 2^(n-m) terms in a fixed order (bit-reproducible, no atomics); the lower
     * triangle is NOT filled by conjugation.  RDM o owns 2 * 4^{m_o} consecutive rows of expect_out / grad_expect BEHIND the dm_purity
     * row (order: diag, Pauli, fidelity, purity, RDMs), entry (a, a') at offset 2 * (a * 2^m + a'), Re then Im.  rydiff_backward:
     * with G = gRe + i gIm (the RDM's rows of grad_expect at (k, b)) the cotangent added to v is G[a][a'] at every entry
     * (idx(a, e), idx(a', e)) — the map is linear in v, so there is no G + G^dagger as on kets — formed in the workspace buffer of
     * the other density-matrix cotangents (after them) and injected through the grad_states route.  Honoured wherever the other
     * dm_* rows are: every kernel family, every tape mode, states_out == NULL without a tape, next to ket-style rows on the doubled
     * register.  Not together with shard_bits > 0 and not in rydiff_forward_tangent (RYDIFF_ENOTIMPL: the other dm_* rows have tangents there).
     * RYDIFF_EINVAL, before anything touches a device: a count outside [0, RYDIFF_MAX_RDMS], NULL masks with a non-zero count, an
     * empty mask, more than RYDIFF_MAX_RDM_QUBITS bits in a mask, a bit at or above n.  Traffic per RDM and state: 2^(n+m) * 16 B,
     * never the 4^n matrix.  dm_atoms = 0: the fields are ignored, like the other dm_* fields.  n_dm_rdms = 0: nothing changes.  (The
     * fields sit in front of dm_atoms: the 14 fields dm_atoms .. dm_shots stay contiguous and directly in front of tape_steps.) */
    int32_t n_dm_rdms;              /* 0: none; at most RYDIFF_MAX_RDMS */
    const uint32_t* dm_rdm_masks;   /* HOST [n_dm_rdms]: bit j = ATOM j, 1 .. min(n, RYDIFF_MAX_RDM_QUBITS) bits, all below n = dm_atoms */

    /* DENSITY-MATRIX observables: dm_atoms = n > 0 declares the register to be the DOUBLED register of a density matrix (the
     * master-equation path, see the pair terms above): n_qubits == 2n, row qubits 0..n-1, column qubits n..2n-1,
     *   vec(rho)[x * 2^n + y] = rho[x][y],
     * and asks for functionals of v = vec(rho_b(t_k)) at every tsave, evaluated while the state is on the device.  Their rows follow
     * ALL the rows above in expect_out / grad_expect ([n_tsave][B] each), in this order:
     *   n_dm_diag rows       sum_x o[x] Re v[x (2^n + 1)]                                  (Tr(rho O) for diagonal O)
     *   n_dm_pauli_obs rows  sum_s w_s Re sum_x i^ny (-1)^popcount((x ^ xm) & zm) v[(x ^ xm) 2^n + x]      (sum_s w_s Re Tr(P_s rho);
     *                        strings over the n ATOMS in the conventions and limits of the ket Pauli block, xm / zm the masks
     *                        moved to index bits of an atom index: atom j <-> bit n-1-j)
     *   n_dm_fid rows        Re sum_{x,y} conj(phi[x]) v[x 2^n + y] phi[y]                  (<phi|rho|phi>; targets are constants, not
     *                        normalised by the library; dm_fid_batch = 1: shared by the trajectories, B: one per trajectory)
     *   dm_purity row        sum_i |v_i|^2                                                  (Tr rho^2 for Hermitian rho)
 *   n_dm_rdms blocks     2 * 4^{m_o} rows each: the reduced density matrices above
     *   dm_moments block     1 + n + n(n-1)/2 rows: the occupation correlations of the diagonal (dm_moments, above)
     * None of them assumes a Hermitian or normalised rho.  rydiff_backward differentiates every row: with g the row's entry of
     * grad_expect at (k, b), the cotangent added to v (torch's dL/dRe + i dL/dIm) is  g o[x] on the diagonal entries;
     * g w_s conj(phase_s(x)) at entry (x ^ xm, x);  g phi[x] conj(phi[y]);  2 g v — formed per save point in the workspace buffer of the
     * Pauli / overlap / RDM cotangents (after them) and injected through the grad_states route.
     * dm_shots = 1 (needs n_shots > 0): the measurement shots above are drawn from p[x] = max(Re v[x (2^n + 1)], 0), x < 2^n — the
     * diagonal of rho — instead of |psi|^2; every other word of the shot rule holds (float64 cumulative sums in a fixed order, the
     * smallest x with C[x] > u * S, the clamping of u, RYDIFF_SHOT_NONE when S == 0, never an x with p[x] == 0).
     * The ket-style fields keep their meaning on the doubled register.  Honoured by rydiff_forward in every kernel family and with
     * every tape mode (states_out == NULL without a tape included: rydiff_plan adds the trajectory the one-launch sweeps are
     * evaluated from).  Not together with shard_bits > 0 (RYDIFF_ENOTIMPL).  rydiff_forward_tangent evaluates the diag / Pauli /
     * fidelity / purity / moment rows and their tangents (not the RDMs, not the shots); rydiff_forward_geometry refuses dm_atoms > 0.  RYDIFF_EINVAL:
     * n_qubits != 2 * dm_atoms, dm_atoms outside [0, RYDIFF_MAX_DM_ATOMS], a count out of range (n_dm_diag <= RYDIFF_MAX_DM_DIAG,
     * strings <= RYDIFF_MAX_PAULI_STRINGS, n_dm_fid <= RYDIFF_MAX_OVERLAPS, dm_purity / dm_shots 0 or 1), a mask bit at or above n,
     * a NULL table with a non-zero count, dm_shots without n_shots.  Traffic per save point and trajectory: 2^n * 16 B per distinct
     * flip mask for the diagonal and Pauli rows, ONE read of the 4^n amplitudes for all fidelities and the purity, 2^n * 16 B for
     * the shots.  dm_atoms = 0: nothing changes, the other dm_* fields are ignored.  (The fields sit in front of tape_steps.) */
    int32_t dm_atoms;               /* n; 0: none */
    int32_t n_dm_diag;
    const double* dm_diag;          /* DEVICE float64 [n_dm_diag][2^n] */
    int32_t n_dm_pauli_obs;
    int32_t n_dm_pauli_strings;
    const int32_t* dm_pauli_first;  /* HOST [n_dm_pauli_obs + 1] */
    const uint32_t* dm_pauli_x;     /* HOST [n_dm_pauli_strings]: bit j = atom j */
    const uint32_t* dm_pauli_z;     /* HOST [n_dm_pauli_strings] */
    const double* dm_pauli_w;       /* HOST [n_dm_pauli_strings] */
    int32_t n_dm_fid;               /* 0 .. RYDIFF_MAX_OVERLAPS */
    int32_t dm_fid_batch;           /* 1 or B */
    const void* dm_fid_targets;     /* DEVICE complex128 [n_dm_fid][dm_fid_batch][2^n] */
    int32_t dm_purity;              /* 0 or 1 */
    int32_t dm_shots;               /* 0 or 1 */

    /* need_tape = 3 (PARTIAL tape) only: the number of TRAILING tsave intervals whose factor outputs are all kept in the workspace
     * tape (1 .. n_tsave - 1); the earlier intervals keep their save-point states only and are recomputed by the adjoint sweep.  The
     * caller sizes it to the HBM that is free (rydiff_plan reports the workspace for the value given): what the full tape of
     * need_tape = 2 does for a run that fits, this does for the part of a run that fits. */
    int32_t tape_steps;

    /* STATE-OVERLAP observables: the complex overlaps with given target states, evaluated at every tsave behind the Pauli
     * observables (below) and differentiated by rydiff_backward:
     *   c_o[k][b] = sum_y conj(phi_{o,b}[y]) psi_b(t_k)[y]          (state fidelity |c|^2, gate fidelity |sum_b c_b| / dim)
     * expect_out and grad_expect become [n_obs + n_pauli_obs + 2 * n_overlaps][n_tsave][B]: overlap o owns two consecutive rows
     * behind the Pauli rows, Re c_o then Im c_o.  The cotangent added to psi_b(t_k) is (gRe + i gIm) * phi_{o,b} (gRe, gIm: the two
     * rows of grad_expect), formed per save point in the workspace next to the Pauli one and injected through the grad_states route.
     * The targets are constants (no gradient) and need not be normalised.  Allowed with final_state_only, with states_out == NULL
     * and no tape, and next to diagonal observables, Pauli observables and pair terms; not together with shard_bits > 0
     * (RYDIFF_ENOTIMPL).  n_overlaps = 0: nothing changes.  (The fields sit in front of the Pauli block, which stays the tail of the
     * struct; library and bindings are built from one header and rydiff_sizeof_problem() guards against a stale pair.) */
    int32_t n_overlaps;             /* 0: none; at most RYDIFF_MAX_OVERLAPS */
    int32_t overlap_batch;          /* 1: all trajectories share each target; B (= batch): one target per trajectory */
    const void* overlap_targets;    /* DEVICE complex128 [n_overlaps][overlap_batch][2^N] */

    /* PAULI-STRING observables, evaluated at every tsave next to the diagonal ones and differentiated by rydiff_backward:
     *   O_o = sum_{s = pauli_first[o]}^{pauli_first[o+1]-1} w_s P_s,   w_s real,   P_s = (x)_j sigma_j,  sigma_j in {I, X, Y, Z}
     * in the basis order of the register (index bit 0 = first basis state r, bit 1 = g): X = [[0,1],[1,0]], Y = [[0,-i],[i,0]],
     * Z = diag(+1,-1).  A string is two qubit masks in the convention of amp_masks (bit j = qubit j; qubit 0 = most significant
     * bit of the amplitude index): pauli_x = the qubits carrying X or Y, pauli_z = the qubits carrying Z or Y.  With xm, zm the
     * same masks moved to amplitude-index bits (qubit j <-> bit N-1-j) and ny = popcount(x & z), since Y = i X Z:
     *   (P psi)[y] = i^ny * (-1)^popcount((y ^ xm) & zm) * psi[y ^ xm],     <O> = sum_s w_s sum_y Re( conj(psi[y]) (P_s psi)[y] )
     * No 2^N table: strings with x = 0 are diagonal observables given by one integer.  expect_out and grad_expect become
     * [n_obs + n_pauli_obs][n_tsave][B], the diagonal observables first.  The arrays are HOST memory (the planner groups the strings by
     * flip mask); they reach the device as kernel arguments, so forward / backward with a RydPlanInfo stay asynchronous.
     * Values are produced while the state is on the device: allowed with final_state_only and with states_out == NULL and no tape.
     * The gradient rides the grad_states route of rydiff_backward (the cotangent 2 * sum_o g_o O_o psi_k is formed per save point
     * in the workspace).  Not together with shard_bits > 0 (RYDIFF_ENOTIMPL); pair terms are fine.  n_pauli_obs = 0: nothing changes. */
    int32_t n_pauli_obs;            /* 0: none */
    int32_t n_pauli_strings;        /* 0 .. RYDIFF_MAX_PAULI_STRINGS */
    const int32_t* pauli_first;     /* HOST [n_pauli_obs + 1], non-decreasing, pauli_first[0] = 0, pauli_first[n_pauli_obs] = n_pauli_strings */
    const uint32_t* pauli_x;        /* HOST [n_pauli_strings] */
    const uint32_t* pauli_z;        /* HOST [n_pauli_strings] */
    const double* pauli_w;          /* HOST [n_pauli_strings] */
} RydProblem;

/* Result of rydiff_plan(): everything that depends on the VALUES in the coefficient tables. */
typedef struct RydPlanInfo {
    double spectral_lo, spectral_hi; /* rigorous bounds on the spectrum of H(t) over the whole run (Gershgorin) */
    double rho_design;               /* max over exponentials of tau * (hi-lo)/2 after sub-stepping */
    int32_t degree;                  /* polynomial degree = matrix-free H applications per (sub-)exponential */
    int32_t n_stages;                /* exponentials in the run (KRYLOV_SE: one per tsave interval) */
    int32_t max_step_factors;        /* largest number of factor passes inside one tsave interval */
    int32_t flags;                   /* bit 0: some flip coefficient has a non-zero imaginary part */
    int64_t total_factors;           /* factor passes of one forward run = H applications per trajectory */
    size_t workspace_bytes;          /* device workspace needed by forward/backward for the flags given to rydiff_plan */
    int32_t tape_mode;               /* the tape the workspace was sized for: 0 none, 1 one state per tsave, 2 full, 3 partial (one state per
                                        tsave + every factor output of the last RydProblem.tape_steps intervals); need_tape = 2 / 3 are granted
                                        from 12 / 13 qubits on, without pair terms and without the XY exchange (xy_mode), otherwise downgraded to 1 */
    int32_t kernel_family;           /* which forward kernels the problem will run on (reporting only): 0 one-wave lane sweep
                                        (<= 6 qubits), 1 one-workgroup persistent sweep (<= 12 qubits), 2 direct launch per factor
                                        (always, at every N, with the XY exchange: xy_mode != 0), 3 chained LDS-tile launch per factor */
    char kernel_fwd[80];             /* reporting only: the instantiation the forward factor passes of THIS problem run on, as a profiler
                                        prints it, e.g. "k_chain<12,10,false,false,true,false>" (tile bits, log2 threads, complex tables,
                                        adjoint, loop-free, L2-resident) — bench.py names its roofline kernel from here */
    char kernel_bwd[80];             /* the same for the adjoint factor passes (empty when need_backward was 0); where a one-launch forward
                                        sweep is followed by the launch-per-factor adjoint (12 qubits, or a save interval of more than 64
                                        factors) this names that adjoint's kernel */
} RydPlanInfo;

#define RYDIFF_PLAN_SCRATCH_BYTES 1024

/* Inspect the coefficient tables (one tiny kernel + ONE stream synchronisation — the only one in the library), bound the spectrum,
 * choose sub-steps and polynomial degree, and size the workspace.
 *   need_tape      1: reserve room for the (n_tsave, B, 2^N) trajectory inside the workspace (caller passes
 *                        states_out == NULL but wants gradients);
 *                  2: FULL tape — the output of every factor pass is kept ((total_factors+1) states), so the adjoint
 *                        sweep recomputes nothing.  Sized for 288 GB of HBM: 156 GiB at N=20, T=1000.  Granted from 12
 *                        qubits on and without pair terms (below, the adjoint sweep is one launch and recomputes on chip);
 *                        otherwise falls back to 1.  RydPlanInfo.tape_mode reports what was granted.
 *                  3: PARTIAL tape — one state per tsave plus the output of every factor pass of the LAST RydProblem.tape_steps
 *                        tsave intervals: the adjoint sweep recomputes the earlier intervals only.  For runs whose full tape does
 *                        not fit (22 qubits x 600 steps, a batch of two 20-qubit trajectories x 1000 steps ...): the caller sizes
 *                        tape_steps to the free HBM.  Granted from 13 qubits on, without pair terms, not for state-sharded runs;
 *                        otherwise falls back to 1.
 *   need_backward  != 0: reserve the backward-sweep buffers too
 *   scratch        DEVICE, >= RYDIFF_PLAN_SCRATCH_BYTES */
int rydiff_plan(const RydProblem* p, int need_tape, int need_backward, void* scratch, void* stream, RydPlanInfo* info);

/* Forward: replaces sesolve(H_t, psi0, tsave, solver, options).states (backend.py:488-494,513-521)
 * and SimulationResults.expect for diagonal observables (simresults.py:81-129).
 *   info        HOST: result of rydiff_plan for the SAME table values (the call is then asynchronous: it enqueues and
 *               returns), or NULL to plan internally (one synchronisation; workspace must then be large enough, see
 *               RYDIFF_EWORKSPACE)
 *   psi0        DEVICE complex128 [B][2^N]
 *   states_out  DEVICE complex128 [n_tsave][B][2^N], or NULL (trajectory kept in the workspace tape if need_tape).
 *               With need_tape = 2 / 3 AND states_out the factor outputs go to the (granted) workspace tape and the states at the
 *               save points are copied out of it — stored states plus a later gradient without (or with less) recomputation.
 *   expect_out  DEVICE float64 [n_obs + n_pauli_obs + 2 * n_overlaps + 2 * sum_o 4^{m_o} + moment rows + dm rows][n_tsave][B] (diagonal observables
 *               first, then the Pauli ones, then Re / Im of every overlap, then Re / Im of every reduced-density-matrix entry, then with
 *               bit_moments the 1 + N + N(N-1)/2 moment rows S, B_q, B_qr, then with energy_rows the rows E (and M2), then the
 *               density-matrix rows n_dm_diag + n_dm_pauli_obs + n_dm_fid + dm_purity + 2 * sum_o 4^{m_o} over dm_rdm_masks
 *               + with dm_moments the 1 + n + n(n-1)/2 rows S, B_q, B_qr of the diagonal of rho), or NULL
 * With RydProblem.n_shots > 0 the measurement shots of the save points in shot_times go to RydProblem.shots_out on the way. */
int rydiff_forward(const RydProblem* p, const RydPlanInfo* info, const void* psi0, void* states_out, double* expect_out,
                   void* workspace, size_t workspace_bytes, int need_tape, void* stream);

/* Backward (vector-Jacobian product): replaces torch autograd's tape through every solver
 * sub-step (derivative.py:40,76).  Cotangents use torch's convention for complex tensors
 * (grad = dL/dRe + i dL/dIm).  The workspace must be the one the forward call used when the
 * trajectory lives in its tape (states == NULL).
 *   states       DEVICE: the states_out of the forward call, or NULL to use the workspace tape (with need_tape = 2 / 3 the
 *                granted workspace tape is used even when states is given)
 *   grad_states  DEVICE complex128 [n_tsave][B][2^N] or NULL
 *   grad_expect  DEVICE float64 [n_obs + n_pauli_obs + 2 * n_overlaps + 2 * sum_o 4^{m_o} + moment rows + energy rows + dm rows][n_tsave][B] or NULL
 *   g_amp        DEVICE complex128 [coeff_batch][n_amp_terms][n_samples] or NULL   (overwritten)
 *   g_det        DEVICE float64    [coeff_batch][n_det_terms][n_samples] or NULL   (overwritten)
 *   g_u          DEVICE float64 [N(N-1)/2] or NULL  (dist_grad, backend.py:456-460 / hamiltonian.py:341-344)
 *   g_tsave      DEVICE float64 [n_tsave] or NULL   (time_grad, backend.py:453-455; state-sharded runs: this call's partial
 *                sum, to be added over the ranks like g_amp / g_det / g_u)
 *   g_psi0       DEVICE complex128 [B][2^N] or NULL */
int rydiff_backward(const RydProblem* p, const RydPlanInfo* info, const void* states, const void* grad_states,
                    const double* grad_expect, void* g_amp, double* g_det, double* g_u, double* g_tsave, void* g_psi0,
                    void* workspace, size_t workspace_bytes, int need_tape, void* stream);

/* Forward-mode (tangent) sweep: the Jacobian-vector twin of rydiff_backward.  One sweep carries the state AND n_dir tangent
 * states through every factor pass and emits d<O>(t_k)/d(theta_d) for every evaluation time, every observable row and every
 * direction d, at roughly (1 + n_dir) forward passes instead of one reverse sweep per evaluation time.  A direction is given by
 * the tangents of the problem's inputs: tables laid out like the tables themselves with the direction as the outermost index.
 * The plan constants (polynomial roots, spectral shift, sub-steps) are frozen — the discrete map that rydiff_backward
 * differentiates:   y = (gamma + beta H) x   =>   dy_d = (gamma + beta H) dx_d + beta dH_d x,   dH_d = H built from the tangent
 * coefficients (same groups, masks, conjugation and diagonal rules).  Tangents w.r.t. tsave are not part of it (g_tsave of
 * rydiff_backward delivers all of them in one reverse sweep). */
#define RYDIFF_MAX_TANGENTS 8
typedef struct RydTangent {
    int32_t n_dir;          /* 1..RYDIFF_MAX_TANGENTS */
    const void*   d_amp;    /* DEVICE complex128 [n_dir][coeff_batch][n_amp_terms][n_samples] or NULL (zero) */
    const double* d_det;    /* DEVICE float64    [n_dir][coeff_batch][n_det_terms][n_samples] or NULL */
    const double* d_u;      /* DEVICE float64    [n_dir][N(N-1)/2] or NULL */
    const void*   d_psi0;   /* DEVICE complex128 [n_dir][B][2^N] or NULL */
    int32_t flags;          /* 0, or RYDIFF_TANGENT_* ored: what the caller asks the sweep to take beyond plain Ising kets */
    const double* d_xy;     /* DEVICE float64    [n_dir][N(N-1)/2] or NULL: tangents of xy_pairs (RYDIFF_TANGENT_XY); RYDIFF_EINVAL when
                             * given with xy_mode = 0.  A valid tangent input on its own.  (Last: the fields before it keep their offsets.) */
} RydTangent;
/* Without its flag a problem with dense pair terms / a density-matrix register / reduced density matrices / bit moments is
 * RYDIFF_ENOTIMPL, as before the sweep took them. */
#define RYDIFF_TANGENT_PAIR_TERMS 1      /* n_pair_terms > 0: the pair terms ride in the pass as constants of every direction */
#define RYDIFF_TANGENT_DENSITY_MATRIX 2  /* dm_atoms > 0: the vectors are vec(rho) and its tangents; the dm_* rows get tangents */
#define RYDIFF_TANGENT_RDMS 4            /* n_rdms > 0: the RDM block of rydiff_forward joins expect_out and dexpect_out */
#define RYDIFF_TANGENT_MOMENTS 8         /* bit_moments = 1 (kets): the Moments block of rydiff_forward joins expect_out and dexpect_out;
                                          * RYDIFF_EINVAL with bit_moments = 0 */
#define RYDIFF_TANGENT_XY 16             /* xy_mode != 0: the exchange stencil rides in the pass (k_factor_tangent<D, false, true>) and its
                                          * couplings have tangents, RydTangent.d_xy; RYDIFF_EINVAL with xy_mode = 0 */

/* sizeof(RydTangent) as this library was compiled (see rydiff_sizeof_problem). */
size_t rydiff_sizeof_tangent(void);

/* Device workspace of rydiff_forward_tangent for n_dir directions (sized as if every tangent pointer were given); 0 on an
 * error (rydiff_last_error).  `info`: from rydiff_plan(p, 0, 0, ...).  Host only.  The regions, each rounded up to 256 bytes: the
 * forward plan's (info->workspace_bytes; with bit_moments beyond 12 qubits that holds B * 79 * 2^(N-12) doubles for the values' tile
 * records), two vector sets of (1 + D') * B * 2^N * 16 bytes (D' = n_dir, 5 -> 6, 7 -> 8), D' coefficient-record sets, D' * 2^N
 * doubles of tangent interaction diagonals and, with RYDIFF_TANGENT_MOMENTS and bit_moments beyond 12 qubits, n_dir * B * 79 * 2^(N-12)
 * doubles for the tile records of the moment tangents (nothing up to 12 qubits). */
size_t rydiff_tangent_workspace_bytes(const RydProblem* p, const RydPlanInfo* info, int n_dir);
/* The same for a call with RydTangent.flags = flags (rydiff_tangent_workspace_bytes is flags = 0). */
size_t rydiff_tangent_workspace_bytes_flags(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags);

/* The tangent sweep.  Asynchronous like rydiff_forward with a plan: it only enqueues work on `stream`.
 *   info         HOST: result of rydiff_plan(p, 0, 0, ...) for the SAME table values (required)
 *   psi0         DEVICE complex128 [B][2^N]  (dm_atoms > 0: vec(rho_0), and d_psi0 = vec(d rho_0))
 *   expect_out   DEVICE float64 [rows][n_tsave][B] or NULL: the values, rows = n_obs + n_pauli_obs + 2 * n_overlaps in the order
 *                of rydiff_forward; with RYDIFF_TANGENT_RDMS followed by the RDM block (2 * 4^{m_o} rows per reduced density matrix,
 *                entry (a, a') at 2 (a 2^m + a'), Re then Im); with RYDIFF_TANGENT_MOMENTS and bit_moments = 1 followed by the
 *                Moments block behind the RDM block, as in rydiff_forward (1 + N + N(N-1)/2 rows: S, B_q in ascending q, B_qr at
 *                1 + N + q(2N-q-1)/2 + (r-q-1)); with dm_atoms > 0 followed by n_dm_diag + n_dm_pauli_obs + n_dm_fid + dm_purity
 *                rows and, with dm_moments, the 1 + n + n(n-1)/2 rows of the DmMoments block, as there
 *   dexpect_out  DEVICE float64 [n_dir][rows][n_tsave][B] (required): diagonal rows 2 sum_y o[y] Re(conj psi[y] dpsi_d[y]), Pauli
 *                rows 2 sum_s w_s Re<psi|P_s|dpsi_d>, overlap rows Re / Im <phi_o|dpsi_d>, RDM rows the entries of
 *                d rho_A = Tr_E(|dpsi_d><psi| + |psi><dpsi_d|) (the mirror entry is the exact conjugate, Im of the diagonal an exact
 *                0; summed with atomics: not bit-reproducible), Moments rows the same moments of the signed weight
 *                dp_d[y] = 2 Re(conj psi[y] dpsi_d[y]): dS_d = sum_y dp_d[y], dB_q = sum_y dp_d[y] y_q, dB_qr = sum_y dp_d[y] y_q y_r
 *                (no atomics, one fixed order: two calls give the same bits; only the n_dir real directions are evaluated); every
 *                save point, k = 0 included.  Need not be cleared.
 *                Density-matrix rows (dm_atoms > 0; v = vec(rho), dv_d its tangent): the diagonal, Pauli, fidelity and moment rows
 *                (dm_moments: k_dm_moments on dv_d, fixed order, no atomics) are linear in v — the row's functional of dv_d — and
 *                the purity row is 2 Re sum_i conj(v_i) dv_d,i
 *   workspace    DEVICE, >= rydiff_tangent_workspace_bytes(p, info, n_dir)
 * Both solvers, coeff_batch 1 or B, dp5_piece_refine honoured (same plan); kernel_variant is ignored: the sweep has one kernel
 * family (launch per factor, one amplitude per thread).  With RYDIFF_TANGENT_PAIR_TERMS in tangent->flags dense pair terms
 * (n_pair_terms > 0: the XY exchange, the dissipator of a master-equation run on the doubled register) ride in the same pass as
 * constants of every direction; with RYDIFF_TANGENT_DENSITY_MATRIX a register with dm_atoms > 0 is taken; with RYDIFF_TANGENT_RDMS
 * the reduced density matrices of a ket (n_rdms > 0) get values and tangents (one k_rdm_tangent launch per RDM and save point); with
 * RYDIFF_TANGENT_MOMENTS the bit moments of a ket (bit_moments = 1) get values and tangents (one k_moments_tangent launch per save
 * point over all directions, beyond 12 qubits followed by k_moments_finish).  The flags combine.
 * With RYDIFF_TANGENT_XY a problem with the XY exchange (xy_mode != 0) is taken, on the forward plan (whose spectral interval already
 * holds sum |J|): the stencil of xy_kernels.hpp rides in the factor pass over the state and all tangent states,
 *   y = (gamma + beta (H + X(J))) x,   dy_d = (gamma + beta (H + X(J))) dx_d + beta (dH_d + X(dJ_d)) x,
 * with dJ_d = tangent->d_xy[d] (NULL: zero).  All ket rows, RYDIFF_TANGENT_RDMS / _MOMENTS, batches and coeff_batch as for Ising kets.
 * xy_mode != 0 without the flag: RYDIFF_ENOTIMPL; the flag or a non-NULL d_xy with xy_mode = 0: RYDIFF_EINVAL.  What the exchange
 * is refused with in rydiff_forward stays refused: pair terms together with it, sharding, dm_atoms > 0, conditioned terms.
 * Not implemented (RYDIFF_ENOTIMPL): pair terms / dm_atoms > 0 / n_rdms > 0 / bit_moments without their flag, state-sharded runs,
 * conditioned / ones-counting terms, shots, partial traces of a density matrix (n_dm_rdms > 0), bit_moments with dm_atoms > 0 whatever
 * the flags.  RYDIFF_EINVAL: flag bits from 32 up, and RYDIFF_TANGENT_MOMENTS on a problem with bit_moments = 0 (the flag asks for a
 * block the problem does not have; callers that predate it and probe bit 8 as an unknown one keep their answer).  Every argument is validated
 * before anything touches a device. */
int rydiff_forward_tangent(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tangent, const void* psi0,
                           double* expect_out, double* dexpect_out, void* workspace, size_t workspace_bytes, void* stream);

/* Quantum geometry from the tangent sweep: the same sweep as rydiff_forward_tangent, which at every save point also takes the inner
 * products of the vectors it carries with each other.  With v_0 = psi(t_k) and v_{1+d} = d psi(t_k) / d theta_d,
 *   G_ij(t_k) = <v_i|v_j> = sum_y conj(v_i[y]) v_j[y]          (conjugate on the LEFT index, so G_ji = conj(G_ij))
 * from which the caller forms, with N = G_00 (valid for unnormalised states),
 *   quantum geometric tensor   Q_de = G_{1+d,1+e} / N - G_{1+d,0} G_{0,1+e} / N^2
 *   quantum Fisher information F = 4 Re Q,       Berry curvature  -2 Im Q
 * and, together with the overlap rows <phi|dpsi_d>, Gauss-Newton terms of fidelity losses.
 *   gram_out     DEVICE complex128 [n_tsave][B][1 + n_dir][1 + n_dir] (required): the FULL Hermitian matrix per save point and
 *                trajectory — the lower triangle is the exact conjugate of the upper one, Im G_ii is an exact 0.  Every entry is
 *                written, k = 0 included (there G is the Gram matrix of psi0 and d_psi0); neither gram_out nor the workspace needs
 *                to be cleared.  A direction padded to the kernel's width (n_dir 5, 7) leaves no trace in the output.
 *   dexpect_out  as in rydiff_forward_tangent, or NULL: the row tangents are skipped
 *   workspace    DEVICE, >= rydiff_geometry_workspace_bytes(p, info, n_dir): the tangent sweep's regions and, behind them, one
 *                partial sum per block, trajectory and entry
 * Fixed order: the sums are formed without atomics — per thread ascending, a fixed wave64 shuffle tree, the block's four waves in
 * order, the blocks in a fixed tree — so two calls on the same inputs return bit-identical matrices (F subtracts numbers of equal
 * size and is inverted in natural-gradient solves).  Traffic: one read of (1 + n_dir) * B * 2^N * 16 bytes per save point on top of
 * the sweep's; nothing of size 2^N is written.  Everything else — expect_out, the solvers, the validation before anything touches
 * a device, what is RYDIFF_ENOTIMPL (state-sharded runs, conditioned / ones-counting terms, shots, reduced density matrices
 * without RYDIFF_TANGENT_RDMS, bit moments without RYDIFF_TANGENT_MOMENTS) — is rydiff_forward_tangent's; pair terms on kets are taken
 * with RYDIFF_TANGENT_PAIR_TERMS, reduced density matrices with RYDIFF_TANGENT_RDMS (the same sweep, the RDM rows are not part of the
 * fixed-order guarantee) and bit moments with RYDIFF_TANGENT_MOMENTS (fixed order; the Gram matrix does not change).  On top of that
 * dm_atoms > 0 is RYDIFF_ENOTIMPL here whatever the flags (and the workspace functions return 0): the Gram matrix of vec(rho) and its
 * tangents is not the mixed-state quantum Fisher information.  RYDIFF_EINVAL also for a NULL gram_out. */
size_t rydiff_geometry_workspace_bytes(const RydProblem* p, const RydPlanInfo* info, int n_dir);
size_t rydiff_geometry_workspace_bytes_flags(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags);
int rydiff_forward_geometry(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tangent, const void* psi0,
                            double* expect_out, double* dexpect_out /* may be NULL */,
                            void* gram_out /* DEVICE complex128 [n_tsave][B][1+n_dir][1+n_dir], required */,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Classical Fisher information of the occupation-basis measurement (bitstrings) from the tangent sweep: the same sweep as
 * rydiff_forward_geometry, which at every save point also forms the "classical Gram matrix" of the vectors it carries.  With
 * u[y] = psi[y] / |psi[y]| the phase of the amplitude, the REAL vectors
 *   w_0[y] = |psi[y]|  (= sqrt p[y]),     w_{1+d}[y] = 2 Re(conj(u[y]) dpsi_d[y])  (= dp_d[y] / sqrt p[y])
 * and C_ij(t_k) = sum_y w_i[y] w_j[y], real symmetric.  C_00 = S = <psi|psi>, C_{0,1+d} = dS / d theta_d, and the caller forms
 *   classical Fisher information   F_C,de = C_{1+d,1+e} / S - C_{0,1+d} C_{0,1+e} / S^2      (valid for unnormalised states)
 * of p(y) = |psi[y]|^2 / S, to hold against the quantum one of gram_out (F_C <= F_Q as matrices).  An amplitude that is exactly zero
 * contributes nothing (w_i[y] = 0 for every i: the sum over the support).  The phase is formed without |psi[y]|^2: amplitudes whose
 * square would overflow or underflow (1e-170, denormals) are legitimate input.
 *   cgram_out    DEVICE float64 [n_tsave][B][1 + n_dir][1 + n_dir] (required): the FULL symmetric matrix per save point and
 *                trajectory, the lower triangle an exact copy of the upper one.  Every entry is written, k = 0 included (there C is
 *                the matrix of psi0 and d_psi0 as given); neither cgram_out nor the workspace needs to be cleared.  A direction
 *                padded to the kernel's width (n_dir 5, 7) leaves no trace in the output.
 *   gram_out     as in rydiff_forward_geometry (the same launches, the same bits), or NULL: the Gram matrix is skipped
 *   dexpect_out  as in rydiff_forward_tangent, or NULL: the row tangents are skipped
 *   workspace    DEVICE, >= rydiff_fisher_workspace_bytes_flags(p, info, n_dir, flags): the geometry sweep's regions and, behind
 *                them, gram_blocks * B * (1 + n_pad)(2 + n_pad) / 2 doubles rounded up to 256 bytes — one upper triangle per block
 *                and trajectory, gram_blocks = min(ceil(2^N / 256), 1024), n_pad = n_dir padded (5 -> 6, 7 -> 8).  Sized as if every
 *                pointer were given.
 * Fixed order, like the Gram matrix: no atomics, two calls on the same inputs return bit-identical matrices.  Traffic: one more read
 * of (1 + n_dir) * B * 2^N * 16 bytes per save point; nothing of size 2^N is written.  Validation happens before anything touches a
 * device; everything rydiff_forward_geometry refuses is refused here with the same codes (dm_atoms > 0 included: RYDIFF_ENOTIMPL
 * whatever the flags, and the workspace function returns 0), and the flags mean what they mean there.  RYDIFF_EINVAL also for a NULL
 * cgram_out; RYDIFF_EWORKSPACE: "fisher workspace too small: need ...". */
size_t rydiff_fisher_workspace_bytes_flags(const RydProblem* p, const RydPlanInfo* info, int n_dir, int flags);
int rydiff_forward_fisher(const RydProblem* p, const RydPlanInfo* info, const RydTangent* tangent, const void* psi0,
                          double* expect_out, double* dexpect_out /* may be NULL */,
                          void* gram_out /* DEVICE complex128 [n_tsave][B][1+n_dir][1+n_dir], may be NULL */,
                          double* cgram_out /* DEVICE float64 [n_tsave][B][1+n_dir][1+n_dir], required */,
                          void* workspace, size_t workspace_bytes, void* stream);

/* One matrix-free application y = H(coefficients) x on DEVICE buffers, for get_hamiltonian-style
 * checks (backend.py:401-427) and micro-benchmarks.  c_amp: HOST complex (re,im) per amp term,
 * c_det: HOST value per det term (already interpolated, reference units as above). */
int rydiff_apply_hamiltonian(const RydProblem* p, const double* c_amp_reim, const double* c_det,
                             const void* x, void* y, void* workspace, size_t workspace_bytes, void* stream);

/* One factor pass  y = gamma*x + beta*H x + sum_k rc_k * remote_k  on DEVICE buffers, coefficients given per term on the
 * HOST like rydiff_apply_hamiltonian.  `remote` (HOST array of n_remote DEVICE pointers, each [B][2^N]) carries the vectors
 * of other GPUs in a state-sharded run: the flip terms of the qubits that select the GPU (pulser-diff_amd/sharded.py;
 * SURVEY.md section 8e, BASELINE config 5).  reuse_diag != 0 skips rebuilding the interaction diagonal kept at the start
 * of `workspace` (>= 8 * 2^N bytes) by a previous call with the same u_pairs. */
int rydiff_apply_factor(const RydProblem* p, const double* c_amp_reim, const double* c_det, const double* gamma_reim,
                        const double* beta_reim, const void* x, void* y, int n_remote, const void* const* remote,
                        const double* remote_coef_reim, int reuse_diag, void* workspace, size_t workspace_bytes, void* stream);

/* Host-only helper (no GPU needed): design the product-form polynomial used for exp(-i*rho*x), x in [-1,1].
 * Writes the degree to *degree and roots (re,im interleaved) to roots_reim[2*max_degree]; returns the
 * measured max |p(x) - exp(-i rho x)| on a test grid in *max_err.  Exposed so the host logic is testable on CPU. */
int rydiff_design_polynomial(double rho, double tol, int max_degree, int* degree, double* roots_reim,
                             double* p0_reim, double* max_err);


const char* rydiff_last_error(void);
const char* rydiff_version(void);

/* sizeof(RydProblem) / sizeof(RydPlanInfo) as this library was compiled: lets a foreign-language binding (ctypes, cgo, JNI)
 * assert that its mirror of the two structs has the same layout before it passes one in. */
size_t rydiff_sizeof_problem(void);
size_t rydiff_sizeof_plan_info(void);

#ifdef __cplusplus
}
#endif
#endif /* RYDIFF_H */
