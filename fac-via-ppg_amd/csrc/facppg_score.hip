// Round-trip scoring (facppg.score): batched dynamic time warping of two padded PPG batches.  The reference has no counterpart --
// it writes the converted wav and never looks at it again (generate_synthesis.py:86-98).
//
// Per pair p: a [D][Ta] against b [D][Tb] (frames contiguous, the front end's layout), local distance the squared Hellinger
// distance d(i,j) = max(0, 1 - sum_k sqrt(a[k][i]) sqrt(b[k][j])), the three-predecessor recurrence over the cells of a slanted band,
// and -- carried along the chosen predecessor -- the path's length and the number of its cells whose top classes agree, so there
// is no back-pointer matrix and no backtrace.  include/facppg.h states the definition; three kinds of launch:
//   k_dtw_prep   one thread per frame: the square roots [D][T] and the arg max (lowest class on a tie), frames < length only
//   k_dtw_dist   one wave per 32 x 32 tile of one pair: the D inner products on the exact-fp32 MFMA (a k-ordered fma chain from
//                0), then 1 - sum clamped at 0; tiles that the band or the lengths leave empty return at once, and only
//                admissible cells are written -- into the SKEWED image dist[i + j][i], whose rows are the anti-diagonals.  The
//                sign bit of a cell says whether the two frames' top classes agree (d >= 0, so it is free)
//   k_dtw_sweep  one workgroup per pair, one thread per row i of a strip of blockDim rows, walking the strip's anti-diagonals:
//                at step s thread t is at column j = s - t.  It keeps "left" (its own last cell) and "diag" (what it read as
//                "up" a step ago) in registers and reads "up" -- thread t - 1's cell of the step before -- from LDS: one
//                ds_write, one ds_read and one barrier per step, and one float of dist per cell, read kAhead steps ahead of
//                its use (a row of the skewed image is one coalesced read of the workgroup).  A pair with more rows than one
//                workgroup has threads takes one launch per strip: the strip's last row leaves its (C, N, M) for every column
//                in the workspace and the next LAUNCH reads them as thread 0's "up" -- nothing crosses workgroups or waits on
//                memory inside a launch.
// Cells outside the band, outside the lengths or left of column 0 carry C = +inf: they lose every strict comparison against a
// finite cost and +inf + d stays +inf, so the recurrence needs no second case and no NaN can form (d is finite by the clamp).
// Plain bounds-checked grid launches on the caller's stream; no cooperative launch, no waiting on memory, no atomics; every loop
// is bounded by the lengths.
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "facppg_common.h"

namespace facppg {
namespace {

constexpr int kPrepThreads = 256;
constexpr int kDistWaves = 4;        // a workgroup of k_dtw_dist: 2 x 2 tiles of 32 x 32
constexpr int kSweepMax = 1024;      // rows of one strip at the most (threads of a k_dtw_sweep workgroup)
// steps the sweep reads dist ahead of their use.  8: 84 / 94 VGPRs; 12: 114 / 123; 16 spills at the 128 a workgroup of 1024 threads
// may hold, and a spilled value comes back through memory in every step
constexpr int kAhead = 8;
static_assert(kAhead % 2 == 0, "the unrolled step body takes the LDS parity from its position");

struct Layout {                      // byte offsets into the workspace, each a multiple of 256
  size_t ra, rb, ca, cb, dist, bnd_c, bnd_n, bnd_m, inf, total;
  size_t dist_pair;                  // floats of one pair's skewed image: (Ta_max + Tb_max - 1) * Ta_max
};

// false: the sizes do not fit a size_t
bool make_layout(int B, int D, int Ta_max, int Tb_max, Layout* out) {
  typedef unsigned __int128 u128;
  const u128 lim = (u128)1 << 62;
  u128 off = 0;
  bool ok = true;
  auto take = [&](u128 bytes) {
    const u128 at = off;
    off += (bytes + 255) / 256 * 256;
    if (off > lim) ok = false;
    return (size_t)at;
  };
  const u128 pair = (u128)((size_t)Ta_max + (size_t)Tb_max - 1) * (u128)Ta_max;
  if (pair > lim) return false;
  out->dist_pair = (size_t)pair;
  out->ra = take((u128)B * D * Ta_max * 4);
  out->rb = take((u128)B * D * Tb_max * 4);
  out->ca = take((u128)B * Ta_max);
  out->cb = take((u128)B * Tb_max);
  out->dist = take((u128)B * pair * 4);
  out->bnd_c = take((u128)B * 2 * Tb_max * 4);
  out->bnd_n = take((u128)B * 2 * Tb_max * 4);
  out->bnd_m = take((u128)B * 2 * Tb_max * 4);
  out->inf = take(4);
  out->total = (size_t)off;
  return ok;
}

// r[p][k][t] = sqrt(max(x[p][k][t], 0)), c[p][t] = arg max_k x[p][k][t] (the lowest k on a tie), for t < len[p] only: the padding
// behind a length is neither read nor written.  One thread per frame, a wave on consecutive frames of every class row.
__global__ void __launch_bounds__(kPrepThreads) k_dtw_prep(const float* __restrict__ x, const int* __restrict__ len, int D, int Tmax,
                                                          float* __restrict__ r, unsigned char* __restrict__ c, float* __restrict__ inf_cell) {
  const int p = blockIdx.y;
  const int t = blockIdx.x * kPrepThreads + threadIdx.x;
  if (p == 0 && t == 0) *inf_cell = INFINITY;      // what the sweep reads where there is no cell
  if (t >= Tmax || t >= len[p]) return;
  const float* xp = x + (size_t)p * D * Tmax + t;
  float* rp = r + (size_t)p * D * Tmax + t;
  float best = xp[0];
  int arg = 0;
  rp[0] = sqrtf(fmaxf(best, 0.0f));
  for (int k = 1; k < D; ++k) {
    const float v = xp[(size_t)k * Tmax];
    rp[(size_t)k * Tmax] = sqrtf(fmaxf(v, 0.0f));
    if (v > best) { best = v; arg = k; }
  }
  c[(size_t)p * Tmax + t] = (unsigned char)arg;
}

// |i (Tb - 1) - j (Ta - 1)| <= width, width = band * max(Ta - 1, Tb - 1, 1) (band 0: every cell)
__device__ __forceinline__ bool admissible(long i, long j, long ea, long eb, long width, int band) {
  const long f = i * eb - j * ea;
  return band == 0 || (f <= width && -f <= width);
}

// One wave per tile: rows i0 .. i0 + 31 of a against columns j0 .. j0 + 31 of b.  MFMA operands (facppg_common.h): lane l gives
// A[l & 31][l >> 5] = ra[k + (l >> 5)][i0 + (l & 31)] and B[l >> 5][l & 31] = rb[k + (l >> 5)][j0 + (l & 31)], zeros past the lengths
// and past D (fma(0, 0, acc) = acc); it receives D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] in acc[r].
// What it stores is d with the agreement of the top classes in the sign bit (d >= 0 by the clamp, -0.0f included): -d where
// ca[i] == cb[j], so that the sweep reads one float per cell and nothing else.
__global__ void __launch_bounds__(kWave * kDistWaves) k_dtw_dist(const float* __restrict__ ra, const float* __restrict__ rb,
                                                                 const unsigned char* __restrict__ ca, const unsigned char* __restrict__ cb,
                                                                 const int* __restrict__ la, const int* __restrict__ lb, int D, int Ta_max,
                                                                 int Tb_max, int band, float* __restrict__ dist, size_t dist_pair) {
  const int p = blockIdx.z;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i0 = (blockIdx.y * 2 + (w >> 1)) * 32, j0 = (blockIdx.x * 2 + (w & 1)) * 32;
  const int Ta = la[p], Tb = lb[p];
  if (i0 >= Ta || j0 >= Tb) return;
  const long ea = Ta - 1, eb = Tb - 1;
  const long width = (long)band * (ea > eb ? (ea > 1 ? ea : 1) : (eb > 1 ? eb : 1));
  if (band != 0) {   // f is linear in (i, j): over the tile it peaks at (i1, j0) and bottoms out at (i0, j1)
    const long i1 = (i0 + 31 < Ta ? i0 + 31 : Ta - 1), j1 = (j0 + 31 < Tb ? j0 + 31 : Tb - 1);
    if (i1 * eb - (long)j0 * ea < -width || (long)i0 * eb - j1 * ea > width) return;
  }
  const int li = i0 + (lane & 31), lj = j0 + (lane & 31), kh = lane >> 5;
  const float* pa = ra + (size_t)p * D * Ta_max + li;
  const float* pb = rb + (size_t)p * D * Tb_max + lj;
  const bool in_a = li < Ta, in_b = lj < Tb;
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int k = 0; k < D; k += 2) {
    const int kk = k + kh;
    const float va = (in_a && kk < D) ? pa[(size_t)kk * Ta_max] : 0.0f;
    const float vb = (in_b && kk < D) ? pb[(size_t)kk * Tb_max] : 0.0f;
    acc = mfma32x32x2(va, vb, acc);
  }
  if (!in_b) return;
  float* dp = dist + (size_t)p * dist_pair;
  const int top_b = cb[(size_t)p * Tb_max + lj];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (i < Ta && admissible(i, lj, ea, eb, width, band)) {
      const float d = fmaxf(0.0f, 1.0f - acc[r]);
      dp[((size_t)i + lj) * Ta_max + i] = (int)ca[(size_t)p * Ta_max + i] == top_b ? -d : d;
    }
  }
}

// What a cell hands on: its cost and, along its chosen predecessor, the path's length and agreeing cells.  16 bytes: one LDS access.
struct __attribute__((aligned(16))) Cell {
  float c;
  int n, m, pad;
};

// Strip q of every pair: rows q * blockDim .. of a, all columns.  See the file comment for the walk.  bnd_*: [B][2][Tb_max], half
// q & 1 written by this launch (the strip's last row), half (q - 1) & 1 read by it (q > 0).  FIRST: q == 0 -- no row above, thread
// 0's "up" is the +inf cell.  The step loop is unrolled kAhead times (its trip count rounded up: a step past the last one finds no
// cell), so the prefetched floats sit in named registers and the LDS parity is a constant of the unrolled body.
template <bool FIRST>
__global__ void __launch_bounds__(kSweepMax) k_dtw_sweep(const float* __restrict__ dist, size_t dist_pair, const float* __restrict__ inf_cell,
                                                        const int* __restrict__ la, const int* __restrict__ lb, int Ta_max, int Tb_max, int band, int q,
                                                        float* __restrict__ bnd_c, int* __restrict__ bnd_n, int* __restrict__ bnd_m,
                                                        float* __restrict__ cost, int* __restrict__ steps, int* __restrict__ agree) {
  // [0], [1]: the cells of the even / odd steps; [2]: the previous strip's last row, columns step .. step + blockDim - 1 (FIRST:
  // [2][0] = +inf).  One array, so that "up" is one read at a computed index.
  __shared__ Cell s_cell[3][kSweepMax];
  const int p = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const int Ta = la[p], Tb = lb[p];
  const long row0 = (long)q * nt;
  if (row0 >= Ta) return;                    // (the whole workgroup: nothing below waits for it)
  const int rows = Ta - row0 < nt ? (int)(Ta - row0) : nt;
  const long i = row0 + t;
  const bool mine = t < rows;
  const long ea = Ta - 1, eb = Tb - 1;
  const long width = (long)band * (ea > eb ? (ea > 1 ? ea : 1) : (eb > 1 ? eb : 1));
  const int n_steps = Tb + rows - 1;
  const float inf = INFINITY;
  const Cell none = {inf, 0, 0, 0};
  const size_t half_r = ((size_t)p * 2 + ((q + 1) & 1)) * Tb_max, half_w = ((size_t)p * 2 + (q & 1)) * Tb_max;

  s_cell[0][t] = none;
  s_cell[1][t] = none;
  if (FIRST) s_cell[2][t] = none;
  __syncthreads();

  // The image's float of the next step for this thread, the +inf cell where there is no admissible one: row (row0 + s) of the skewed
  // image holds this strip's cells of step s, thread t's at column i.  The address is chosen, the load unconditional and its value
  // used kAhead steps later: no step waits for memory.  f = i (Tb - 1) - j (Ta - 1) goes along (64-bit).  (Offsets from the +inf
  // cell and a mask, not a choice between two pointers: that the compiler turns into a table in scratch.)
  long next_off = (dist + (size_t)p * dist_pair + (size_t)row0 * Ta_max + i) - inf_cell;
  int next_j = -t;
  long next_f = i * eb + (long)t * ea;
  auto fetch = [&]() -> float {
    const bool ok = mine && (unsigned)next_j < (unsigned)Tb && (band == 0 || (next_f <= width && -next_f <= width));
    const float v = inf_cell[next_off & -(long)ok];
    next_off += Ta_max;
    next_j += 1;
    next_f -= ea;
    return v;
  };
  float cur[kAhead], nxt[kAhead];
#pragma unroll
  for (int u = 0; u < kAhead; ++u) cur[u] = fetch();

  // (0, 0) has no predecessor: its "diagonal" is a path of cost 0 and no cells
  Cell left = none, diag = {(FIRST && t == 0) ? 0.0f : inf, 0, 0, 0};
  const bool last_row = t == rows - 1, final_row = last_row && i == Ta - 1;
  int sb = 0;                                // step modulo blockDim (strips behind the first)
  int j = -t;
  for (int s0 = 0; s0 < n_steps; s0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) nxt[u] = fetch();
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (!FIRST) {
        if (sb == 0) {                       // thread 0's "up" of the next blockDim steps (uniform over the workgroup)
          const int jb = s0 + u + t;
          Cell b = none;
          if (jb < Tb) { b.c = bnd_c[half_r + jb]; b.n = bnd_n[half_r + jb]; b.m = bnd_m[half_r + jb]; }
          s_cell[2][t] = b;
          __syncthreads();
        }
      }
      // "up": thread t - 1's cell of the step before; thread 0: the row above the strip
      const Cell up = (&s_cell[0][0])[t > 0 ? ((u + 1) & 1) * kSweepMax + t - 1 : 2 * kSweepMax + (FIRST ? 0 : sb)];
      // predecessors in the order (i-1, j-1), (i-1, j), (i, j-1); a strict < keeps the earlier one on a tie
      Cell best = diag;
      if (up.c < best.c) best = up;
      if (left.c < best.c) best = left;
      // no cell here (cur = +inf: outside the band or the lengths): +inf, which no later comparison picks
      Cell me;
      me.c = fabsf(cur[u]) + best.c;
      me.n = best.n + 1;
      me.m = best.m + (int)(__float_as_uint(cur[u]) >> 31);
      me.pad = 0;
      s_cell[u & 1][t] = me;
      if (last_row && (unsigned)j < (unsigned)Tb) {
        if (final_row) {
          if (j == Tb - 1) { cost[p] = me.c; steps[p] = me.n; agree[p] = me.m; }
        } else {
          bnd_c[half_w + j] = me.c; bnd_n[half_w + j] = me.n; bnd_m[half_w + j] = me.m;
        }
      }
      left = me;
      diag = up;
      j += 1;
      if (!FIRST) sb = sb + 1 == nt ? 0 : sb + 1;
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
  }
}

}  // namespace
}  // namespace facppg

using namespace facppg;

extern "C" size_t facppg_ppg_dtw_workspace_bytes(int B, int D, int Ta_max, int Tb_max, int band) {
  (void)band;
  if (B < 1 || D < 1 || Ta_max < 1 || Tb_max < 1) {
    set_error("facppg_ppg_dtw_workspace_bytes: B, D, Ta_max, Tb_max must be positive (got %d, %d, %d, %d)", B, D, Ta_max, Tb_max);
    return 0;
  }
  Layout lay;
  if (!make_layout(B, D, Ta_max, Tb_max, &lay)) {
    set_error("facppg_ppg_dtw_workspace_bytes: %d pairs of %d x %d frames need more memory than a size_t counts", B, Ta_max, Tb_max);
    return 0;
  }
  return lay.total;
}

extern "C" int facppg_ppg_dtw(const float* a_dev, const int32_t* la_dev, const int32_t* la_host, int Ta_max, const float* b_dev,
                              const int32_t* lb_dev, const int32_t* lb_host, int Tb_max, int B, int D, int band, float* cost_dev,
                              int32_t* steps_dev, int32_t* agree_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(a_dev && la_dev && la_host && b_dev && lb_dev && lb_host && cost_dev && steps_dev && agree_dev && ws_dev, FACPPG_EINVAL,
                 "facppg_ppg_dtw: NULL argument");
  FACPPG_REQUIRE(B >= 1 && D >= 1 && Ta_max >= 1 && Tb_max >= 1, FACPPG_EINVAL,
                 "facppg_ppg_dtw: B, D, Ta_max, Tb_max must be positive (got %d, %d, %d, %d)", B, D, Ta_max, Tb_max);
  FACPPG_REQUIRE(band == 0 || band >= 2, FACPPG_EINVAL,
                 "facppg_ppg_dtw: band must be 0 (no band) or at least 2 (got %d): a narrower band may leave no path", band);
  FACPPG_REQUIRE(D <= 256, FACPPG_EUNSUPPORTED,
                 "facppg_ppg_dtw: at most 256 classes per frame (got %d): reduce senone posteriors to monophone classes first", D);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "facppg_ppg_dtw: at most 65535 pairs per call (got %d)", B);
  int longest_a = 0, longest_b = 0;
  for (int p = 0; p < B; ++p) {
    FACPPG_REQUIRE(la_host[p] >= 1 && la_host[p] <= Ta_max, FACPPG_EINVAL, "facppg_ppg_dtw: pair %d: a has %d frames (1 <= frames <= Ta_max = %d)", p,
                   la_host[p], Ta_max);
    FACPPG_REQUIRE(lb_host[p] >= 1 && lb_host[p] <= Tb_max, FACPPG_EINVAL, "facppg_ppg_dtw: pair %d: b has %d frames (1 <= frames <= Tb_max = %d)", p,
                   lb_host[p], Tb_max);
    longest_a = la_host[p] > longest_a ? la_host[p] : longest_a;
    longest_b = lb_host[p] > longest_b ? lb_host[p] : longest_b;
  }
  Layout lay;
  FACPPG_REQUIRE(make_layout(B, D, Ta_max, Tb_max, &lay), FACPPG_EUNSUPPORTED,
                 "facppg_ppg_dtw: %d pairs of %d x %d frames need more memory than a size_t counts", B, Ta_max, Tb_max);
  FACPPG_REQUIRE(ws_bytes >= lay.total, FACPPG_EWORKSPACE, "facppg_ppg_dtw: workspace of %zu bytes, facppg_ppg_dtw_workspace_bytes asks for %zu",
                 ws_bytes, lay.total);
  const long tiles_a = ((long)longest_a + 63) / 64, tiles_b = ((long)longest_b + 63) / 64;
  FACPPG_REQUIRE(tiles_a <= 65535, FACPPG_EUNSUPPORTED, "facppg_ppg_dtw: %d frames of a are too many rows for one launch", longest_a);

  hipStream_t st = (hipStream_t)stream_;
  char* ws = (char*)ws_dev;
  float* ra = (float*)(ws + lay.ra);
  float* rb = (float*)(ws + lay.rb);
  unsigned char* ca = (unsigned char*)(ws + lay.ca);
  unsigned char* cb = (unsigned char*)(ws + lay.cb);
  float* dist = (float*)(ws + lay.dist);
  float* bnd_c = (float*)(ws + lay.bnd_c);
  int* bnd_n = (int*)(ws + lay.bnd_n);
  int* bnd_m = (int*)(ws + lay.bnd_m);
  float* inf_cell = (float*)(ws + lay.inf);

  k_dtw_prep<<<dim3((longest_a + kPrepThreads - 1) / kPrepThreads, B), kPrepThreads, 0, st>>>(a_dev, la_dev, D, Ta_max, ra, ca, inf_cell);
  FACPPG_HIP_CHECK(hipGetLastError());
  k_dtw_prep<<<dim3((longest_b + kPrepThreads - 1) / kPrepThreads, B), kPrepThreads, 0, st>>>(b_dev, lb_dev, D, Tb_max, rb, cb, inf_cell);
  FACPPG_HIP_CHECK(hipGetLastError());
  k_dtw_dist<<<dim3((unsigned)tiles_b, (unsigned)tiles_a, B), kWave * kDistWaves, 0, st>>>(ra, rb, ca, cb, la_dev, lb_dev, D, Ta_max, Tb_max, band, dist,
                                                                                         lay.dist_pair);
  FACPPG_HIP_CHECK(hipGetLastError());
  // rows per strip = threads per workgroup: the longest a rounded up to whole waves, kSweepMax at the most (FACPPG_DTW_ROWS:
  // a smaller strip, for measurements)
  int nt = round_up(longest_a, kWave);
  nt = nt < kSweepMax ? nt : kSweepMax;
  if (const char* e = getenv("FACPPG_DTW_ROWS")) {
    const int v = atoi(e) / kWave * kWave;
    if (v >= kWave && v < nt) nt = v;
  }
  for (int q = 0; (long)q * nt < longest_a; ++q) {
    if (q == 0)
      k_dtw_sweep<true><<<B, nt, 0, st>>>(dist, lay.dist_pair, inf_cell, la_dev, lb_dev, Ta_max, Tb_max, band, q, bnd_c, bnd_n, bnd_m, cost_dev,
                                          steps_dev, agree_dev);
    else
      k_dtw_sweep<false><<<B, nt, 0, st>>>(dist, lay.dist_pair, inf_cell, la_dev, lb_dev, Ta_max, Tb_max, band, q, bnd_c, bnd_n, bnd_m, cost_dev,
                                           steps_dev, agree_dev);
    FACPPG_HIP_CHECK(hipGetLastError());
  }
  return FACPPG_OK;
}
