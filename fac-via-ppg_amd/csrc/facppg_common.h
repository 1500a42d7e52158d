// Internal helpers shared by the translation units of libfacppg_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "facppg.h"

namespace facppg {

void set_error(const char* fmt, ...);

#define FACPPG_HIP_CHECK(expr)                                                          \
  do {                                                                                  \
    hipError_t e__ = (expr);                                                            \
    if (e__ != hipSuccess) {                                                            \
      ::facppg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return FACPPG_EHIP;                                                               \
    }                                                                                   \
  } while (0)

#define FACPPG_REQUIRE(cond, code, ...)  \
  do {                                   \
    if (!(cond)) {                       \
      ::facppg::set_error(__VA_ARGS__);  \
      return (code);                     \
    }                                    \
  } while (0)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;  // CDNA wavefront

__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// The cooperating kernels (decoder, BiLSTM) need all their workgroups co-resident; hipLaunchCooperativeKernel checks that the
// grid fits, and the callers size their grids from the occupancy calculator.  (The persistent vocoder's launch in
// facppg_wgp.hip and the vocoder handles' poll limit still carry their own copies of these two helpers.)
// FACPPG_COOP_PLAIN=1 launches the SAME kernels with the same grids as ordinary launches (read per call): rocprofv3 on this
// stack dies on cooperative launches, and an ordinary launch of a grid that fits an otherwise idle GPU is co-resident all the
// same (every poll is bounded in wall-clock time: a launch that did not fit traps instead of hanging) -- the profiling mode of
// tools/profile_coop.sh, not a production setting.
inline hipError_t launch_coop(const void* fn, dim3 grid, dim3 block, void** args, size_t smem, hipStream_t s) {
  const char* plain = getenv("FACPPG_COOP_PLAIN");
  if (plain && atoi(plain) != 0) return hipLaunchKernel(fn, grid, block, args, smem, s);
  return hipLaunchCooperativeKernel(fn, grid, block, args, smem, s);
}

// FACPPG_POLL_LIMIT (seconds a cooperative kernel may wait on one exchange word before it traps; default 20, 0 = never) in
// ticks of the device's constant-rate clock; 0 = unbounded (also when the clock rate is unknown).
inline unsigned long long poll_limit_ticks(int device) {
  const char* pl = getenv("FACPPG_POLL_LIMIT");
  const double seconds = pl ? strtod(pl, nullptr) : 20.0;
  int khz = 0;
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
  return seconds > 0 && khz > 0 ? (unsigned long long)(seconds * 1e3 * khz) : 0ull;
}

// A kernel that asks for more than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize once on EVERY device it
// runs on.  `devices` is the call site's (or the kernel's) own static, one bit per device: a set bit means no HIP call beyond
// hipGetDevice (so nothing but that query runs while a stream is being captured, once the eager warm-up has set the bit); a
// second thread setting the attribute again is harmless; devices >= 64 set it on every call.  fn2: a second instantiation
// launched from the same site (the stamped debugging build), set together with the first.
inline int ensure_dynamic_lds(std::atomic<unsigned long long>& devices, size_t bytes, const void* fn, const void* fn2 = nullptr) {
  int dev = 0;
  FACPPG_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 64 && ((devices.load(std::memory_order_relaxed) >> dev) & 1ull)) return FACPPG_OK;
  FACPPG_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (fn2) FACPPG_HIP_CHECK(hipFuncSetAttribute(fn2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (dev < 64) devices.fetch_or(1ull << dev, std::memory_order_relaxed);
  return FACPPG_OK;
}

// Frame / sample offsets of a batch of utterances laid end to end (host copy): B + 1 values, off[0] = 0, strictly increasing
// (every utterance holds at least one element).
inline int check_offsets(const int32_t* off, int B, const char* what) {
  FACPPG_REQUIRE(off && B > 0, FACPPG_EINVAL, "%s: NULL offsets or no utterance", what);
  FACPPG_REQUIRE(off[0] == 0, FACPPG_EINVAL, "%s: offsets must start at 0 (got %d)", what, off[0]);
  for (int b = 0; b < B; ++b)
    FACPPG_REQUIRE(off[b + 1] > off[b], FACPPG_EINVAL, "%s: offsets must increase (utterance %d: %d -> %d)", what, b, off[b], off[b + 1]);
  return FACPPG_OK;
}

// largest b in [0, B) with off[b] <= g  (off strictly increasing, off[0] <= g)
__device__ __forceinline__ int seg_of(const int* __restrict__ off, int B, int g) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One exact-fp32 MFMA: D[32x32] += A[32x2] * B[2x32]; lane l holds A[l&31][l>>5], B[l>>5][l&31].
__device__ __forceinline__ f32x16 mfma32x32x2(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// v_mfma_f32_16x16x4_f32: D[16x16] += A[16x4] * B[4x16].  Lane l supplies A[l % 16][l / 16] and
// B[l / 16][l % 16]; it holds D[4 * (l / 16) + r][l % 16] in c[r].
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// log det W and W^-T of one small mixing matrix (c <= 8) by LU with partial pivoting, one thread: (called by ONE wave of 64 lanes; uses 528 bytes of LDS.)  What torch.logdet and its
// backward do through rocSOLVER in ~22 tiny launches per flow and direction (glow.py:100: log_det_W = B * L * logdet(W)).
// det <= 0 follows torch.logdet: NaN for a negative determinant, -inf for a singular matrix.
__device__ inline void logdet_wave(const float* __restrict__ W, int c, float* __restrict__ logdet, float* __restrict__ winv_t) {
  // one wave; lane (i, j) owns element [i][j] of the matrix and of the accumulating inverse (Gauss-Jordan on [A | I] with
  // partial pivoting).  (A one-thread version with the two 8 x 8 arrays in scratch took 72 us per call.)
  __shared__ float A[8][8], Iv[8][8];
  __shared__ int s_piv, s_singular;
  __shared__ float s_sign, s_log;
  const int tid = threadIdx.x, i = tid >> 3, j = tid & 7;
  const bool in = i < c && j < c;
  A[i][j] = in ? W[i * c + j] : (i == j ? 1.0f : 0.0f);
  Iv[i][j] = i == j ? 1.0f : 0.0f;
  if (tid == 0) { s_sign = 1.0f; s_log = 0.0f; s_singular = 0; }
  __syncthreads();
  for (int k = 0; k < c; ++k) {
    if (tid == 0) {
      int piv = k;
      float best = fabsf(A[k][k]);
      for (int r = k + 1; r < c; ++r)
        if (fabsf(A[r][k]) > best) { best = fabsf(A[r][k]); piv = r; }
      s_piv = piv;
      if (best == 0.0f) s_singular = 1;
    }
    __syncthreads();
    if (s_singular) break;
    const int piv = s_piv;
    if (piv != k && i == k) {   // row k's lanes exchange rows k and piv
      float t = A[k][j]; A[k][j] = A[piv][j]; A[piv][j] = t;
      t = Iv[k][j]; Iv[k][j] = Iv[piv][j]; Iv[piv][j] = t;
    }
    __syncthreads();
    const float d = A[k][k];
    __syncthreads();
    if (tid == 0) {
      if (piv != k) s_sign = -s_sign;
      if (d < 0.0f) s_sign = -s_sign;
      s_log += logf(fabsf(d));
    }
    if (i == k) { const float r = 1.0f / d; A[k][j] *= r; Iv[k][j] *= r; }
    __syncthreads();
    const float f = A[i][k], akj = A[k][j], ikj = Iv[k][j];
    __syncthreads();
    if (i != k) { A[i][j] = fmaf(-f, akj, A[i][j]); Iv[i][j] = fmaf(-f, ikj, Iv[i][j]); }
    __syncthreads();
  }
  if (s_singular) {
    if (tid == 0) *logdet = -INFINITY;
    if (in) winv_t[i * c + j] = NAN;
    return;
  }
  if (tid == 0) *logdet = s_sign > 0.0f ? s_log : NAN;
  if (in) winv_t[i * c + j] = Iv[j][i];
}

}  // namespace facppg
