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
//   k_dtw_sweep  the sweep over that image, shared with facppg_mel_dtw: facppg_dtw_sweep.h (one workgroup per pair, one launch per
//                strip of 1024 rows)
// Cells outside the band, outside the lengths or left of column 0 carry C = +inf: they lose every strict comparison against a
// finite cost and +inf + d stays +inf, so the recurrence needs no second case and no NaN can form (d is finite by the clamp).
// Plain bounds-checked grid launches on the caller's stream; no cooperative launch, no waiting on memory, no atomics; every loop
// is bounded by the lengths.
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "facppg_common.h"
#include "facppg_dtw_sweep.h"

namespace facppg {
namespace {

constexpr int kPrepThreads = 256;
constexpr int kDistWaves = 4;        // a workgroup of k_dtw_dist: 2 x 2 tiles of 32 x 32

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
  const SweepBuffers sweep = {dist, lay.dist_pair, inf_cell, bnd_c, bnd_n, bnd_m};
  return launch_dtw_sweep(sweep, la_dev, lb_dev, Ta_max, Tb_max, band, B, longest_a, cost_dev, steps_dev, agree_dev, st);
}
