// Free-running validation (facppg.score.mel_dtw / attention_path): the mel-cepstral DTW of two padded log-mel batches, and what
// the attention of a free-running decode did.  The reference has no counterpart -- its validate() is teacher-forced only
// (train_ppg2mel.py:152-177).  include/facppg.h states both definitions.
//
// facppg_mel_dtw, per pair p: a [M][Ta] against b [M][Tb] (frames contiguous), three kinds of launch:
//   k_mcd_project  one thread per (coefficient k, frame t): c[k][t] = sum_m basis[k][m] x[m][t], one fp32 fma chain from 0 with m
//                  increasing; frames < length only (what lies behind a length is neither read nor written)
//   k_mcd_dist     one workgroup per 64 x 64 tile of one pair, the two tiles of cepstra staged in LDS (zeros past the lengths: they
//                  only feed cells that are not written).  d(i,j) = sqrtf(sum_k (ca[k][i] - cb[k][j])^2) by DIRECT differences, one
//                  fp32 fma chain from 0 with k increasing -- |a|^2 + |b|^2 - 2 a.b would lose eps |a|^2 exactly where two frames
//                  are close.  Lane l sits on row i0 + l and walks the columns j0 + ((c - l) & 63): in one step a wave's cells lie
//                  on two anti-diagonals, i.e. in two contiguous runs of the SKEWED image dist[i + j][i] that the sweep reads, and
//                  both LDS reads are conflict-free.  Tiles that the band or the lengths leave empty return at once; only
//                  admissible cells are written.  d >= 0 with a clear sign bit: the sweep's flag count M stays 0
//   k_dtw_sweep    facppg_dtw_sweep.h, the sweep facppg_ppg_dtw runs: band, recurrence, tie order and N(i,j) are its own
// facppg_attention_path, per utterance p: two launches:
//   k_attn_argmax  one wave per decoder step t < T: pos[t] = arg max_{j < L} A[t][j] (the lowest j on a tie), w[t] = that maximum
//   k_attn_stats   one workgroup per utterance: every thread summarises a contiguous chunk of pos (backward jumps, largest jump,
//                  its first / last value, the runs at its head and tail, the longest run inside, the float64 sum of w) and marks
//                  the visited inputs in a byte map (plain stores of 1); thread 0 joins the 256 summaries in order
// Plain bounds-checked grid launches on the caller's stream; no cooperative launch, no waiting on memory, no atomics; every loop
// is bounded by the lengths.
#include <climits>
#include <cmath>
#include <cstdint>

#include "facppg_common.h"
#include "facppg_dtw_sweep.h"

namespace facppg {
namespace {

constexpr int kProjThreads = 256;
constexpr int kTile = 64;            // k_mcd_dist: rows and columns of a tile; one lane per row
constexpr int kDistThreads = 256;    // 4 waves, 16 columns each
constexpr int kColsPerWave = kTile / (kDistThreads / kWave);
constexpr int kMaxCep = 64;
constexpr int kMaxMel = 256;
constexpr int kArgWaves = 4;
constexpr int kStatThreads = 256;

struct MelLayout {                   // byte offsets into the workspace, each a multiple of 256
  size_t ca, cb, dist, bnd_c, bnd_n, bnd_m, flags, inf, total;
  size_t dist_pair;                  // floats of one pair's skewed image: (Ta_max + Tb_max - 1) * Ta_max
};

struct Taker {                       // hands out 256-byte aligned pieces; ok = false: the sizes do not fit a size_t
  typedef unsigned __int128 u128;
  u128 off = 0;
  bool ok = true;
  size_t take(u128 bytes) {
    const u128 at = off;
    off += (bytes + 255) / 256 * 256;
    if (off > ((u128)1 << 62)) ok = false;
    return (size_t)at;
  }
};

bool make_mel_layout(int B, int K, int Ta_max, int Tb_max, MelLayout* out) {
  typedef unsigned __int128 u128;
  const u128 pair = (u128)((size_t)Ta_max + (size_t)Tb_max - 1) * (u128)Ta_max;
  if (pair > ((u128)1 << 62)) return false;
  Taker t;
  out->dist_pair = (size_t)pair;
  out->ca = t.take((u128)B * K * Ta_max * 4);
  out->cb = t.take((u128)B * K * Tb_max * 4);
  out->dist = t.take((u128)B * pair * 4);
  out->bnd_c = t.take((u128)B * 2 * Tb_max * 4);
  out->bnd_n = t.take((u128)B * 2 * Tb_max * 4);
  out->bnd_m = t.take((u128)B * 2 * Tb_max * 4);
  out->flags = t.take((u128)B * 4);           // the sweep's M(Ta-1, Tb-1): no cell sets the flag, nobody reads it
  out->inf = t.take(4);
  out->total = (size_t)t.off;
  return t.ok;
}

// c[p][k][t] = sum_m basis[k][m] x[p][m][t] for t < len[p]: grid (frames / 256, K, B); a wave reads consecutive frames of every mel
// row and one basis value (uniform over the workgroup) per step.
__global__ void __launch_bounds__(kProjThreads) k_mcd_project(const float* __restrict__ x, const int* __restrict__ len, const float* __restrict__ basis,
                                                            int M, int K, int Tmax, float* __restrict__ c, float* __restrict__ inf_cell) {
  const int p = blockIdx.z, k = blockIdx.y;
  const int t = blockIdx.x * kProjThreads + threadIdx.x;
  if (p == 0 && k == 0 && t == 0) *inf_cell = INFINITY;      // what the sweep reads where there is no cell
  if (t >= Tmax || t >= len[p]) return;
  const float* xp = x + (size_t)p * M * Tmax + t;
  const float* bk = basis + (size_t)k * M;
  float acc = 0.0f;
  for (int m = 0; m < M; ++m) acc = fmaf(bk[m], xp[(size_t)m * Tmax], acc);
  c[((size_t)p * K + k) * Tmax + t] = acc;
}

__global__ void __launch_bounds__(kDistThreads) k_mcd_dist(const float* __restrict__ ca, const float* __restrict__ cb, const int* __restrict__ la,
                                                         const int* __restrict__ lb, int K, int Ta_max, int Tb_max, int band,
                                                         float* __restrict__ dist, size_t dist_pair) {
  __shared__ float s_a[kMaxCep * kTile], s_b[kMaxCep * kTile];
  const int p = blockIdx.z;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int Ta = la[p], Tb = lb[p];
  if (i0 >= Ta || j0 >= Tb) return;          // (the whole workgroup, ahead of its only barrier)
  const long ea = Ta - 1, eb = Tb - 1;
  const long width = (long)band * (ea > eb ? (ea > 1 ? ea : 1) : (eb > 1 ? eb : 1));
  if (band != 0) {   // f is linear in (i, j): over the tile it peaks at (i1, j0) and bottoms out at (i0, j1)
    const long i1 = (i0 + kTile - 1 < Ta ? i0 + kTile - 1 : Ta - 1), j1 = (j0 + kTile - 1 < Tb ? j0 + kTile - 1 : Tb - 1);
    if (i1 * eb - (long)j0 * ea < -width || (long)i0 * eb - j1 * ea > width) return;
  }
  const float* pa = ca + (size_t)p * K * Ta_max;
  const float* pb = cb + (size_t)p * K * Tb_max;
  for (int e = threadIdx.x; e < K * kTile; e += kDistThreads) {
    const int k = e / kTile, x = e % kTile;
    s_a[e] = i0 + x < Ta ? pa[(size_t)k * Ta_max + i0 + x] : 0.0f;
    s_b[e] = j0 + x < Tb ? pb[(size_t)k * Tb_max + j0 + x] : 0.0f;
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), c0 = (threadIdx.x / kWave) * kColsPerWave;
  float s[kColsPerWave];
#pragma unroll
  for (int c = 0; c < kColsPerWave; ++c) s[c] = 0.0f;
  for (int k = 0; k < K; ++k) {
    const float av = s_a[k * kTile + lane];
#pragma unroll
    for (int c = 0; c < kColsPerWave; ++c) {
      const float diff = av - s_b[k * kTile + ((c0 + c - lane) & (kTile - 1))];
      s[c] = fmaf(diff, diff, s[c]);
    }
  }
  const int i = i0 + lane;
  if (i >= Ta) return;
  float* dp = dist + (size_t)p * dist_pair;
#pragma unroll
  for (int c = 0; c < kColsPerWave; ++c) {
    const int j = j0 + ((c0 + c - lane) & (kTile - 1));
    if (j < Tb && admissible(i, j, ea, eb, width, band)) dp[((size_t)i + j) * Ta_max + i] = sqrtf(s[c]);
  }
}

struct AttnLayout {
  size_t pos, w, seen, total;
};

bool make_attn_layout(int B, int Tout_max, int Tin_max, AttnLayout* out) {
  typedef unsigned __int128 u128;
  Taker t;
  out->pos = t.take((u128)B * Tout_max * 4);
  out->w = t.take((u128)B * Tout_max * 4);
  out->seen = t.take((u128)B * Tin_max);
  out->total = (size_t)t.off;
  return t.ok;
}

// One wave per row t < T of utterance p: lane l looks at j = l, l + 64, ... < L (a strict > keeps its lowest j), then the lanes
// are joined pairwise: the larger value, on a tie the lower j.  A lane without a column holds (-inf, INT_MAX) and loses.
__global__ void __launch_bounds__(kWave * kArgWaves) k_attn_argmax(const float* __restrict__ align, const int* __restrict__ tout,
                                                                  const int* __restrict__ tin, int Tout_max, int Tin_max,
                                                                  int* __restrict__ pos, float* __restrict__ w) {
  const int p = blockIdx.y;
  const long t = (long)blockIdx.x * kArgWaves + threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int L = tin[p];
  if (t >= Tout_max || t >= tout[p]) return;
  const float* row = align + ((size_t)p * Tout_max + t) * Tin_max;
  float best = -INFINITY;
  int arg = INT_MAX;
  for (int j = lane; j < L; j += kWave) {
    const float v = row[j];
    if (v > best || arg == INT_MAX) { best = v; arg = j; }
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(best, d, kWave);
    const int oj = __shfl_xor(arg, d, kWave);
    if (oj != INT_MAX && (arg == INT_MAX || ov > best || (ov == best && oj < arg))) { best = ov; arg = oj; }
  }
  if (lane == 0) {
    pos[(size_t)p * Tout_max + t] = arg;
    w[(size_t)p * Tout_max + t] = best;
  }
}

// What a thread knows of its chunk of pos, joined in order by thread 0.
struct Chunk {
  int len, first, last, head, tail, best, back, jump;
};

__global__ void __launch_bounds__(kStatThreads) k_attn_stats(const int* __restrict__ pos, const float* __restrict__ w, const int* __restrict__ tout,
                                                           const int* __restrict__ tin, int Tout_max, int Tin_max, unsigned char* seen,
                                                           int* __restrict__ stats, float* __restrict__ focus) {
  __shared__ Chunk s_chunk[kStatThreads];
  __shared__ double s_sum[kStatThreads];
  __shared__ int s_seen[kStatThreads];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int T = tout[p], L = tin[p];
  const int* pp = pos + (size_t)p * Tout_max;
  const float* wp = w + (size_t)p * Tout_max;
  unsigned char* sp = seen + (size_t)p * Tin_max;
  for (int j = tid; j < L; j += kStatThreads) sp[j] = 0;
  __syncthreads();
  const long per = ((long)T + kStatThreads - 1) / kStatThreads;
  const long t0 = tid * per < T ? tid * per : T, t1 = t0 + per < T ? t0 + per : T;
  Chunk c = {(int)(t1 - t0), 0, 0, 0, 0, 0, 0, 0};
  double sum = 0.0;
  int run = 0, prev = 0;
  for (long t = t0; t < t1; ++t) {
    const int v = pp[t];
    sp[v] = 1;                               // (v < L: k_attn_argmax looked at columns < L only)
    sum += (double)wp[t];
    if (t == t0) {
      c.first = v;
      run = 1;
      if (t > 0) prev = pp[t - 1];           // the chunk before: a backward jump or a skip across the seam counts here
    } else if (v == prev) {
      run += 1;
    } else {
      if (c.head == 0) c.head = run;
      c.best = run > c.best ? run : c.best;
      run = 1;
    }
    if (t > 0) {
      c.back += v < prev;
      c.jump = v - prev > c.jump ? v - prev : c.jump;
    }
    prev = v;
  }
  if (c.len > 0) {
    c.last = prev;
    c.tail = run;
    if (c.head == 0) c.head = run;           // one run: head == tail == len
    c.best = run > c.best ? run : c.best;
  }
  s_chunk[tid] = c;
  s_sum[tid] = sum;
  __syncthreads();                           // (and every mark in ``seen`` is visible to the workgroup)
  int n = 0;
  for (int j = tid; j < L; j += kStatThreads) n += sp[j];
  s_seen[tid] = n;
  __syncthreads();
  if (tid != 0) return;
  int back = 0, jump = 0, best = 0, carry = 0, carry_val = 0, visited = 0;
  double total = 0.0;
  for (int k = 0; k < kStatThreads; ++k) {
    visited += s_seen[k];
    const Chunk& q = s_chunk[k];
    if (q.len == 0) continue;
    total += s_sum[k];
    back += q.back;
    jump = q.jump > jump ? q.jump : jump;
    best = q.best > best ? q.best : best;
    if (carry > 0 && carry_val == q.first) {   // the run at the end of the chunks so far goes on into this one
      const int joined = carry + q.head;
      best = joined > best ? joined : best;
      carry = q.head == q.len ? joined : q.tail;
    } else {
      carry = q.tail;
    }
    carry_val = q.last;
  }
  int* out = stats + (size_t)p * 6;
  out[0] = pp[0];
  out[1] = pp[T - 1];
  out[2] = back;
  out[3] = jump;
  out[4] = best;
  out[5] = visited;
  focus[p] = (float)(total / (double)T);
}

// ``what`` names the first NULL pointer of a call, or is NULL
const char* first_null(const void* const* ptrs, const char* const* names, int n) {
  for (int k = 0; k < n; ++k)
    if (!ptrs[k]) return names[k];
  return nullptr;
}

}  // namespace
}  // namespace facppg

using namespace facppg;

extern "C" size_t facppg_mel_dtw_workspace_bytes(int B, int M, int K, int Ta_max, int Tb_max, int band) {
  (void)band;
  if (B < 1 || M < 1 || K < 1 || Ta_max < 1 || Tb_max < 1) {
    set_error("facppg_mel_dtw_workspace_bytes: B, M, K, Ta_max, Tb_max must be positive (got %d, %d, %d, %d, %d)", B, M, K, Ta_max, Tb_max);
    return 0;
  }
  MelLayout lay;
  if (!make_mel_layout(B, K, Ta_max, Tb_max, &lay)) {
    set_error("facppg_mel_dtw_workspace_bytes: %d pairs of %d x %d frames need more memory than a size_t counts", B, Ta_max, Tb_max);
    return 0;
  }
  return lay.total;
}

extern "C" int facppg_mel_dtw(const float* a_dev, const int32_t* la_dev, const int32_t* la_host, int Ta_max, const float* b_dev,
                              const int32_t* lb_dev, const int32_t* lb_host, int Tb_max, int B, int M, const float* basis_dev, int K, int band,
                              float* cost_dev, int32_t* steps_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
  const void* const ptrs[] = {a_dev, la_dev, la_host, b_dev, lb_dev, lb_host, basis_dev, cost_dev, steps_dev, ws_dev};
  const char* const names[] = {"a_dev", "la_dev", "la_host", "b_dev", "lb_dev", "lb_host", "basis_dev", "cost_dev", "steps_dev", "ws_dev"};
  const char* null = first_null(ptrs, names, 10);
  FACPPG_REQUIRE(!null, FACPPG_EINVAL, "facppg_mel_dtw: NULL argument: %s", null);
  FACPPG_REQUIRE(B >= 1 && M >= 1 && K >= 1 && Ta_max >= 1 && Tb_max >= 1, FACPPG_EINVAL,
                 "facppg_mel_dtw: B, M, K, Ta_max, Tb_max must be positive (got %d, %d, %d, %d, %d)", B, M, K, Ta_max, Tb_max);
  FACPPG_REQUIRE(band == 0 || band >= 2, FACPPG_EINVAL,
                 "facppg_mel_dtw: band must be 0 (no band) or at least 2 (got %d): a narrower band may leave no path", band);
  FACPPG_REQUIRE(M <= kMaxMel, FACPPG_EUNSUPPORTED, "facppg_mel_dtw: at most %d mel channels M per frame (got %d)", kMaxMel, M);
  FACPPG_REQUIRE(K <= kMaxCep, FACPPG_EUNSUPPORTED, "facppg_mel_dtw: at most %d cepstral coefficients K (got %d): a tile of them is staged in LDS",
                 kMaxCep, K);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "facppg_mel_dtw: at most 65535 pairs B per call (got %d)", B);
  int longest_a = 0, longest_b = 0;
  for (int p = 0; p < B; ++p) {
    FACPPG_REQUIRE(la_host[p] >= 1 && la_host[p] <= Ta_max, FACPPG_EINVAL, "facppg_mel_dtw: pair %d: a has %d frames (1 <= la <= Ta_max = %d)", p,
                   la_host[p], Ta_max);
    FACPPG_REQUIRE(lb_host[p] >= 1 && lb_host[p] <= Tb_max, FACPPG_EINVAL, "facppg_mel_dtw: pair %d: b has %d frames (1 <= lb <= Tb_max = %d)", p,
                   lb_host[p], Tb_max);
    longest_a = la_host[p] > longest_a ? la_host[p] : longest_a;
    longest_b = lb_host[p] > longest_b ? lb_host[p] : longest_b;
  }
  MelLayout lay;
  FACPPG_REQUIRE(make_mel_layout(B, K, Ta_max, Tb_max, &lay), FACPPG_EUNSUPPORTED,
                 "facppg_mel_dtw: %d pairs of %d x %d frames need more memory than a size_t counts", B, Ta_max, Tb_max);
  FACPPG_REQUIRE(ws_bytes >= lay.total, FACPPG_EWORKSPACE, "facppg_mel_dtw: workspace ws_bytes of %zu bytes, facppg_mel_dtw_workspace_bytes asks for %zu",
                 ws_bytes, lay.total);
  const long tiles_a = ((long)longest_a + kTile - 1) / kTile, tiles_b = ((long)longest_b + kTile - 1) / kTile;
  FACPPG_REQUIRE(tiles_a <= 65535, FACPPG_EUNSUPPORTED, "facppg_mel_dtw: %d frames of a are too many rows for one launch", longest_a);

  hipStream_t st = (hipStream_t)stream_;
  char* ws = (char*)ws_dev;
  float* ca = (float*)(ws + lay.ca);
  float* cb = (float*)(ws + lay.cb);
  float* dist = (float*)(ws + lay.dist);
  float* inf_cell = (float*)(ws + lay.inf);

  k_mcd_project<<<dim3((longest_a + kProjThreads - 1) / kProjThreads, K, B), kProjThreads, 0, st>>>(a_dev, la_dev, basis_dev, M, K, Ta_max, ca, inf_cell);
  FACPPG_HIP_CHECK(hipGetLastError());
  k_mcd_project<<<dim3((longest_b + kProjThreads - 1) / kProjThreads, K, B), kProjThreads, 0, st>>>(b_dev, lb_dev, basis_dev, M, K, Tb_max, cb, inf_cell);
  FACPPG_HIP_CHECK(hipGetLastError());
  k_mcd_dist<<<dim3((unsigned)tiles_b, (unsigned)tiles_a, B), kDistThreads, 0, st>>>(ca, cb, la_dev, lb_dev, K, Ta_max, Tb_max, band, dist, lay.dist_pair);
  FACPPG_HIP_CHECK(hipGetLastError());
  const SweepBuffers sweep = {dist, lay.dist_pair, inf_cell, (float*)(ws + lay.bnd_c), (int*)(ws + lay.bnd_n), (int*)(ws + lay.bnd_m)};
  return launch_dtw_sweep(sweep, la_dev, lb_dev, Ta_max, Tb_max, band, B, longest_a, cost_dev, steps_dev, (int*)(ws + lay.flags), st);
}

extern "C" size_t facppg_attention_path_workspace_bytes(int B, int Tout_max, int Tin_max) {
  if (B < 1 || Tout_max < 1 || Tin_max < 1) {
    set_error("facppg_attention_path_workspace_bytes: B, Tout_max, Tin_max must be positive (got %d, %d, %d)", B, Tout_max, Tin_max);
    return 0;
  }
  AttnLayout lay;
  if (!make_attn_layout(B, Tout_max, Tin_max, &lay)) {
    set_error("facppg_attention_path_workspace_bytes: %d utterances of %d x %d need more memory than a size_t counts", B, Tout_max, Tin_max);
    return 0;
  }
  return lay.total;
}

extern "C" int facppg_attention_path(const float* align_dev, const int32_t* tout_dev, const int32_t* tout_host, int Tout_max, const int32_t* tin_dev,
                                     const int32_t* tin_host, int Tin_max, int B, int32_t* stats_dev, float* focus_dev, void* ws_dev, size_t ws_bytes,
                                     void* stream_) {
  const void* const ptrs[] = {align_dev, tout_dev, tout_host, tin_dev, tin_host, stats_dev, focus_dev, ws_dev};
  const char* const names[] = {"align_dev", "tout_dev", "tout_host", "tin_dev", "tin_host", "stats_dev", "focus_dev", "ws_dev"};
  const char* null = first_null(ptrs, names, 8);
  FACPPG_REQUIRE(!null, FACPPG_EINVAL, "facppg_attention_path: NULL argument: %s", null);
  FACPPG_REQUIRE(B >= 1 && Tout_max >= 1 && Tin_max >= 1, FACPPG_EINVAL,
                 "facppg_attention_path: B, Tout_max, Tin_max must be positive (got %d, %d, %d)", B, Tout_max, Tin_max);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "facppg_attention_path: at most 65535 utterances B per call (got %d)", B);
  int longest = 0;
  for (int p = 0; p < B; ++p) {
    FACPPG_REQUIRE(tout_host[p] >= 1 && tout_host[p] <= Tout_max, FACPPG_EINVAL,
                   "facppg_attention_path: utterance %d: %d decoder steps (1 <= tout <= Tout_max = %d)", p, tout_host[p], Tout_max);
    FACPPG_REQUIRE(tin_host[p] >= 1 && tin_host[p] <= Tin_max, FACPPG_EINVAL,
                   "facppg_attention_path: utterance %d: %d input frames (1 <= tin <= Tin_max = %d)", p, tin_host[p], Tin_max);
    longest = tout_host[p] > longest ? tout_host[p] : longest;
  }
  AttnLayout lay;
  FACPPG_REQUIRE(make_attn_layout(B, Tout_max, Tin_max, &lay), FACPPG_EUNSUPPORTED,
                 "facppg_attention_path: %d utterances of %d x %d need more memory than a size_t counts", B, Tout_max, Tin_max);
  FACPPG_REQUIRE(ws_bytes >= lay.total, FACPPG_EWORKSPACE,
                 "facppg_attention_path: workspace ws_bytes of %zu bytes, facppg_attention_path_workspace_bytes asks for %zu", ws_bytes, lay.total);

  hipStream_t st = (hipStream_t)stream_;
  char* ws = (char*)ws_dev;
  int* pos = (int*)(ws + lay.pos);
  float* w = (float*)(ws + lay.w);
  k_attn_argmax<<<dim3((longest + kArgWaves - 1) / kArgWaves, B), kWave * kArgWaves, 0, st>>>(align_dev, tout_dev, tin_dev, Tout_max, Tin_max, pos, w);
  FACPPG_HIP_CHECK(hipGetLastError());
  k_attn_stats<<<B, kStatThreads, 0, st>>>(pos, w, tout_dev, tin_dev, Tout_max, Tin_max, (unsigned char*)(ws + lay.seen), stats_dev, focus_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
