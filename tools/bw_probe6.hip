// Probe 6: the exchange patterns of a block-of-two chained pass (two factors per launch, 3 vectors per layout change) against
// the one-factor pass, on 16 MiB vectors at N = 20 with 256 tiles of 2^12 amplitudes (1024 threads x 4 amplitudes).
//   2R+2W, 2 rounds   one factor per launch (today's k_chain: finish + start)
//   3R+3W, 4 rounds   block of two, forward without tape        (v, w, t in;  y, w', t' out)
//   3R+4W, 4 rounds   block of two, forward with the full tape  (+ v_mid)
//   5R+3W, 4 rounds   block of two, adjoint with the full tape  (mu, w, t + two tape vectors in)
//   5R+3W, 5 rounds   ... with P_X x on the tape: one more finishing round (8 bits) on a tape vector, in a second tile buffer,
//                     with a barrier of its own, ahead of the other four (it rebuilds the mid-block state from x and P_X x)
// A round is: tile write, barrier, partner sums over the tile bits of the stage (8 Y' bits in the finishing rounds, all 12 in
// the starting rounds: 10 through LDS, 2 register renaming), barrier — the LDS work of the real passes.  Back-to-back
// launches alternating the two tile layouts; the tape vectors cycle through a pool larger than the Infinity Cache.
//   hipcc --offload-arch=gfx950 -O3 -o bw_probe6 bw_probe6.hip && ./bw_probe6
#include <hip/hip_runtime.h>
#include <cstdio>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %d\n",hipGetErrorString(e),__LINE__); return 1;}}while(0)

constexpr int LGT = 10, NT = 1 << LGT, R = 4, TILE = NT * R;
constexpr int kMaxVec = 5;

// layout A: tile = contiguous 2^12 run; layout B: 256-byte runs (16 amplitudes) strided by 2^12 amplitudes (N = 20)
__device__ __forceinline__ size_t addr(int layout, unsigned t, unsigned i) {
  if (layout == 0) return (size_t)t * TILE + i;
  return ((size_t)(i >> 4) << 12) | ((size_t)t << 4) | (i & 15u);
}

struct Vecs {
  const double2* in[kMaxVec];
  double2* out[kMaxVec];
};

// partner sum over tile bits [b0, 12): LDS for bits < LGT, register renaming above
__device__ __forceinline__ void round_sum(const double2* sh, const double2 (&own)[R], int b0, double2 (&ts)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) ts[r] = make_double2(0.0, 0.0);
#pragma unroll
  for (int b = 0; b < 12; ++b) {
    if (b < b0) continue;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double2 q = b < LGT ? sh[(unsigned(r) * NT + threadIdx.x) ^ (1u << b)] : own[r ^ (1 << (b - LGT))];
      ts[r].x += q.x;
      ts[r].y += q.y;
    }
  }
}

// LIGHT: one LDS partner read per round instead of the partner sums (the exchange of tools/bw_probe5.hip: bandwidth + barriers only)
// XR: the extra finishing round on the tape vector x[NR - 2], folded into the tape vector x[NR - 1]
template <int NR, int NW, int ROUNDS, bool LIGHT, bool XR = false>
__global__ __launch_bounds__(NT) void k_probe(int layout, Vecs v) {
  extern __shared__ __attribute__((aligned(16))) double2 sh[];
  const unsigned t = blockIdx.x;
  double2 x[NR][R];
#pragma unroll
  for (int k = 0; k < NR; ++k)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t g = addr(layout, t, r * NT + threadIdx.x);
      x[k][r].x = __builtin_nontemporal_load(&v.in[k][g].x);
      x[k][r].y = __builtin_nontemporal_load(&v.in[k][g].y);
    }
  if constexpr (XR) {
    double2* sh2 = sh + TILE;
#pragma unroll
    for (int r = 0; r < R; ++r) sh2[r * NT + threadIdx.x] = x[NR - 2][r];
    __syncthreads();
    double2 ts[R];
    round_sum(sh2, x[NR - 2], 4, ts);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      x[NR - 1][r].x = 0.5 * x[NR - 2][r].x + 1e-3 * ts[r].x + 0.25 * x[NR - 1][r].x;
      x[NR - 1][r].y = 0.5 * x[NR - 2][r].y + 1e-3 * ts[r].y + 0.25 * x[NR - 1][r].y;
    }
  }
  double2 cur[R];
#pragma unroll
  for (int r = 0; r < R; ++r) cur[r] = x[0][r];
  int stored = 0;
  auto store = [&](const double2 (&val)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t g = addr(layout, t, r * NT + threadIdx.x);
      __builtin_nontemporal_store(val[r].x, &v.out[stored][g].x);
      __builtin_nontemporal_store(val[r].y, &v.out[stored][g].y);
    }
    ++stored;
  };
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    if (k) __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) sh[r * NT + threadIdx.x] = cur[r];
    __syncthreads();
    double2 ts[R];
    if (LIGHT) {
#pragma unroll
      for (int r = 0; r < R; ++r) ts[r] = sh[(unsigned(r) * NT + threadIdx.x) ^ (64u << (k & 1))];
    } else {
      round_sum(sh, cur, k < ROUNDS / 2 ? 4 : 0, ts);  // finishing rounds: the 8 bits the previous layout lacked
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {  // fold in the next loaded vector (as w, t, tape are folded in by the real passes)
      const double2 o = x[(k + 1) % NR][r];
      cur[r].x = 0.5 * cur[r].x + 1e-3 * ts[r].x + 0.25 * o.x;
      cur[r].y = 0.5 * cur[r].y + 1e-3 * ts[r].y + 0.25 * o.y;
    }
    // stores: everything but one per later round after the finishing rounds, then one per starting round
    const int due = k < ROUNDS / 2 - 1 ? 0 : (k == ROUNDS / 2 - 1 ? NW - ROUNDS / 2 : NW - (ROUNDS - 1 - k));
    while (stored < due) store(cur);
  }
}

template <int NR, int NW, int ROUNDS, bool LIGHT, bool XR = false>
static int run(const char* name, double2** pool, int npool, int iters, double per_factor_div, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  const size_t lds = (XR ? 2 : 1) * TILE * sizeof(double2);
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_probe<NR, NW, ROUNDS, LIGHT, XR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // buffers 0..4: set A, 5..9: set B (the chained vectors ping-pong); 10..npool-1: tape pool
  auto launch = [&](int i) {
    Vecs v{};
    const int src = (i & 1) ? 5 : 0, dst = (i & 1) ? 0 : 5;
    const int chained = NW < NR ? NW : NR;
    for (int k = 0; k < NR; ++k) v.in[k] = k < chained ? pool[src + k] : pool[10 + (i * 2 + k) % (npool - 10)];
    for (int k = 0; k < NW; ++k) v.out[k] = pool[dst + k];
    hipLaunchKernelGGL((k_probe<NR, NW, ROUNDS, LIGHT, XR>), dim3(256), dim3(NT), lds, s, i & 1, v);
  };
  for (int i = 0; i < 4; ++i) launch(i);
  CK(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) launch(i);
  CK(hipEventRecord(e1, s));
  CK(hipEventSynchronize(e1));
  CK(hipGetLastError());
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  const double us = ms * 1e3 / iters;
  const double mb = (NR + NW) * 16.777216;
  printf("%-30s %7.2f us per launch  %7.2f us per factor  (%.1f MB moved, %.2f TB/s)\n", name, us, us / per_factor_div, mb, mb / us);  // MB per us = TB/s
  return 0;
}

int main() {
  hipStream_t s;
  CK(hipStreamCreate(&s));
  const size_t n = (size_t)1 << 20;  // 16 MiB of double2
  constexpr int kPool = 10 + 24;     // 10 chained + 24 tape vectors (384 MiB: more than the Infinity Cache)
  double2* pool[kPool];
  for (int i = 0; i < kPool; ++i) {
    CK(hipMalloc(&pool[i], n * sizeof(double2)));
    CK(hipMemset(pool[i], 0, n * sizeof(double2)));
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int it = 2000;
  for (int rep = 0; rep < 3; ++rep) {  // interleaved repeats: the spread is the noise
    printf("-- repeat %d\n", rep);
    if (run<2, 2, 2, true>("2R+2W light, 1 factor", pool, kPool, it, 1.0, s, e0, e1)) return 1;
    if (run<3, 3, 4, true>("3R+3W light, 2 factors", pool, kPool, it, 2.0, s, e0, e1)) return 1;
    if (run<2, 2, 2, false>("2R+2W, 1 factor (today)", pool, kPool, it, 1.0, s, e0, e1)) return 1;
    if (run<3, 3, 4, false>("3R+3W, 2 factors (no tape)", pool, kPool, it, 2.0, s, e0, e1)) return 1;
    if (run<3, 4, 4, false>("3R+4W, 2 factors (tape)", pool, kPool, it, 2.0, s, e0, e1)) return 1;
    if (run<5, 3, 4, false>("5R+3W, 2 factors (adjoint)", pool, kPool, it, 2.0, s, e0, e1)) return 1;
    if (run<5, 3, 4, false, true>("5R+3W, 5 rounds (adjoint, w tape)", pool, kPool, it, 2.0, s, e0, e1)) return 1;
  }
  for (int i = 0; i < kPool; ++i) CK(hipFree(pool[i]));
  return 0;
}
