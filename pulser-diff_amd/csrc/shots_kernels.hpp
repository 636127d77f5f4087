// shots_kernels.hpp — measurement shots (include/rydiff.h: RydProblem.n_shots / shot_*): amplitude indices sampled from
// |psi_b(t_k)|^2 by inverse transform of the caller's uniforms, on the state where it lies — it is read, never written.
//   k_shot_chunk_sums  pass A: p = |psi|^2 summed per chunk of 2^10 amplitudes, 16 bytes per lane and load, consecutive lanes on
//                      consecutive amplitudes; wave shuffle + one LDS step in a fixed order, no atomics: bit-reproducible
//   k_shot_scan        inclusive prefix of the chunk sums of every trajectory (2^N / 2^10 doubles: 8 KiB at 20 qubits), monotone
//                      by construction: every entry is offset + running sum of non-negative terms
//   k_shot_resolve     pass B, one wave per shot: binary search of the chunk prefix for u * S, then that one chunk again (16 KiB):
//                      p through LDS into 16 consecutive amplitudes per lane, serial sums per lane, wave scan of the lane totals,
//                      first amplitude whose cumulative value exceeds the target
// The rule of the header holds exactly where rounding does not decide: a returned x always has p[x] > 0; where the within-chunk
// sums (another order than pass A's) leave no amplitude above the target, or the target is not below S, the last amplitude with
// p > 0 of the chunk (of the state) is taken.  Registers below one chunk (N < 10) are one partial chunk: same kernels.
#pragma once

constexpr int kShotChunkBits = 10;
constexpr uint32_t kShotChunk = 1u << kShotChunkBits;

// one expression for p in both passes (the compiler is free to contract a * a + b * b either way)
__device__ __forceinline__ double shot_prob(const double2& v) { return fma(v.x, v.x, v.y * v.y); }

struct ShotSumArgs {
    const double2* psi;  // the sampled state, trajectory 0
    double* sums;        // [B][nch]
    uint32_t dim, nch;
    int b_first;
};

// grid (nch, b_count)
__global__ __launch_bounds__(256) void k_shot_chunk_sums(ShotSumArgs a) {
    __shared__ double lds[4];
    const int b = a.b_first + int(blockIdx.y);
    const double2* __restrict__ psi = a.psi + size_t(b) * a.dim;
    const uint32_t base = blockIdx.x << kShotChunkBits;
    double s = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < kShotChunk / 256u; ++j) {
        const uint32_t y = base + j * 256u + threadIdx.x;
        if (y < a.dim) s += shot_prob(psi[y]);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.sums[size_t(b) * a.nch + blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

struct ShotScanArgs {
    const double* sums;  // [B][nch]
    double* prefix;      // [B][nch]: prefix[c] = sums[0] + ... + sums[c]
    uint32_t nch;
    int b_first;
};

// grid (b_count): thread t owns a contiguous segment; segment totals are scanned serially by thread 0, so the last entry of a
// segment and the offset of the next one are the same number
__global__ __launch_bounds__(256) void k_shot_scan(ShotScanArgs a) {
    __shared__ double part[256];
    const int b = a.b_first + int(blockIdx.x);
    const double* __restrict__ s = a.sums + size_t(b) * a.nch;
    double* __restrict__ p = a.prefix + size_t(b) * a.nch;
    const uint32_t seg = (a.nch + 255u) / 256u;
    const uint32_t lo = min(threadIdx.x * seg, a.nch), hi = min(lo + seg, a.nch);
    double run = 0.0;
    for (uint32_t i = lo; i < hi; ++i) run += s[i];
    part[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int w = 0; w < 256; ++w) {
            const double v = part[w];
            part[w] = acc;
            acc += v;
        }
    }
    __syncthreads();
    const double off = part[threadIdx.x];
    run = 0.0;
    for (uint32_t i = lo; i < hi; ++i) {
        run += s[i];
        p[i] = off + run;
    }
}

struct ShotResolveArgs {
    const double2* psi;    // the sampled state, trajectory 0
    const double* sums;    // [B][nch]
    const double* prefix;  // [B][nch]
    const double* u;       // [B][n_shots] of this sampled save point
    uint32_t* out;         // [B][n_shots]
    uint32_t dim, nch;
    int n_shots, b_first;
};

// grid (n_shots, b_count), one wave each.  LDS: the chunk's p, one double of padding per 16 so that the lanes' runs of 16
// (stride 17 doubles) fall on distinct banks.
__global__ __launch_bounds__(64) void k_shot_resolve(ShotResolveArgs a) {
    __shared__ double pl[kShotChunk + kShotChunk / 16];
    const int lane = threadIdx.x;
    const int b = a.b_first + int(blockIdx.y);
    const size_t slot = size_t(b) * a.n_shots + blockIdx.x;
    const double* __restrict__ prefix = a.prefix + size_t(b) * a.nch;
    const double* __restrict__ sums = a.sums + size_t(b) * a.nch;
    const double S = prefix[a.nch - 1];
    if (!(S > 0.0)) {  // (uniform) nothing to sample from
        if (lane == 0) a.out[slot] = RYDIFF_SHOT_NONE;
        return;
    }
    double u = a.u[slot];
    u = u > 0.0 ? fmin(u, 1.0 - 0x1p-53) : 0.0;  // [0, 1); NaN -> 0
    const double tau = u * S;
    // first chunk whose prefix exceeds the target (every lane walks the same path)
    uint32_t lo = 0, hi = a.nch;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] > tau) hi = mid;
        else lo = mid + 1;
    }
    const bool tail = lo == a.nch;  // rounding left no cumulative value above the target: the last populated amplitude
    uint32_t c = lo;
    if (tail) {
        bool found = false;
        for (int64_t base = int64_t((a.nch - 1) / 64u) * 64; base >= 0 && !found; base -= 64) {
            const int64_t i = base + lane;
            const unsigned long long m = __ballot(i < int64_t(a.nch) && sums[i] > 0.0);
            if (m) {
                c = uint32_t(base) + 63u - uint32_t(__clzll(m));
                found = true;
            }
        }
        if (!found) {  // (S > 0 rules it out)
            if (lane == 0) a.out[slot] = RYDIFF_SHOT_NONE;
            return;
        }
    }
    const uint32_t cbase = c << kShotChunkBits;
    const double2* __restrict__ psi = a.psi + size_t(b) * a.dim;
#pragma unroll
    for (uint32_t j = 0; j < kShotChunk / 64u; ++j) {
        const uint32_t i = j * 64u + lane, y = cbase + i;
        pl[i + (i >> 4)] = y < a.dim ? shot_prob(psi[y]) : 0.0;
    }
    __syncthreads();
    double v[16], tot = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        v[q] = pl[lane * 17 + q];
        tot += v[q];
    }
    double inc = tot;  // inclusive scan of the lane totals
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    const double below = c ? prefix[c - 1] : 0.0;
    int hit = -1, last = -1;
    double run = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        run += v[q];
        if (v[q] > 0.0) {
            last = q;
            if (hit < 0 && !tail && below + (exc + run) > tau) hit = q;
        }
    }
    uint32_t x = RYDIFF_SHOT_NONE;
    const unsigned long long mh = __ballot(hit >= 0);
    if (mh) {
        const int src = __ffsll(mh) - 1;
        x = cbase + uint32_t(src) * 16u + uint32_t(__shfl(hit, src, 64));
    } else {
        const unsigned long long ml = __ballot(last >= 0);
        if (ml) {
            const int src = 63 - __clzll(ml);
            x = cbase + uint32_t(src) * 16u + uint32_t(__shfl(last, src, 64));
        }
    }
    if (lane == 0) a.out[slot] = x;
}
