// The DTW sweep shared by facppg_score.hip (facppg_ppg_dtw) and facppg_mcd.hip (facppg_mel_dtw): the band, the recurrence, the tie
// order and what is carried along the chosen predecessor do not depend on the local distance, so both entry points write the same
// skewed image of distances and run the same kernel over it (not part of the ABI).  include/facppg.h states the definition.
//
//   the image    dist[i + j][i], Ta_max floats per row: the rows are the anti-diagonals.  Only admissible cells (inside the lengths
//                and the band) are written and read.  A cell holds d >= 0; its SIGN BIT is a flag that the sweep counts along the
//                path into M (ppg_dtw: the two frames' top classes agree; mel_dtw: never set)
//   k_dtw_sweep  one workgroup per pair, one thread per row i of a strip of blockDim rows, walking the strip's anti-diagonals:
//                at step s thread t is at column j = s - t.  It keeps "left" (its own last cell) and "diag" (what it read as
//                "up" a step ago) in registers and reads "up" -- thread t - 1's cell of the step before -- from LDS: one
//                ds_write, one ds_read and one barrier per step, and one float of dist per cell, read kAhead steps ahead of
//                its use (a row of the skewed image is one coalesced read of the workgroup).  A pair with more rows than one
//                workgroup has threads takes one launch per strip: the strip's last row leaves its (C, N, M) for every column
//                in the workspace and the next LAUNCH reads them as thread 0's "up" -- nothing crosses workgroups or waits on
//                memory inside a launch.
// Cells outside the band, outside the lengths or left of column 0 carry C = +inf: they lose every strict comparison against a
// finite cost and +inf + d stays +inf, so the recurrence needs no second case and no NaN can form (d is finite).
// Plain bounds-checked grid launches on the caller's stream; no cooperative launch, no waiting on memory, no atomics; every loop
// is bounded by the lengths.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "facppg_common.h"

namespace facppg {
namespace {

constexpr int kSweepMax = 1024;      // rows of one strip at the most (threads of a k_dtw_sweep workgroup)
// steps the sweep reads dist ahead of their use.  8: 84 / 94 VGPRs; 12: 114 / 123; 16 spills at the 128 a workgroup of 1024 threads
// may hold, and a spilled value comes back through memory in every step
constexpr int kAhead = 8;
static_assert(kAhead % 2 == 0, "the unrolled step body takes the LDS parity from its position");

// |i (Tb - 1) - j (Ta - 1)| <= width, width = band * max(Ta - 1, Tb - 1, 1) (band 0: every cell)
__device__ __forceinline__ bool admissible(long i, long j, long ea, long eb, long width, int band) {
  const long f = i * eb - j * ea;
  return band == 0 || (f <= width && -f <= width);
}

// What a cell hands on: its cost and, along its chosen predecessor, the path's length and flagged cells.  16 bytes: one LDS access.
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

// What the sweep needs of a workspace: the image, the strips' hand-over rows and the +inf cell (device pointers).
struct SweepBuffers {
  const float* dist;
  size_t dist_pair;                  // floats of one pair's skewed image: (Ta_max + Tb_max - 1) * Ta_max
  const float* inf_cell;             // one float holding +inf, written by an earlier launch on the same stream
  float* bnd_c;                      // [B][2][Tb_max] each
  int* bnd_n;
  int* bnd_m;
};

// The sweep over an image that earlier launches on ``st`` wrote: one launch per strip of the longest a.  Rows per strip = threads
// per workgroup: the longest a rounded up to whole waves, kSweepMax at the most (FACPPG_DTW_ROWS: a smaller strip, for
// measurements).
inline int launch_dtw_sweep(const SweepBuffers& w, const int* la_dev, const int* lb_dev, int Ta_max, int Tb_max, int band, int B, int longest_a,
                            float* cost_dev, int* steps_dev, int* agree_dev, hipStream_t st) {
  int nt = round_up(longest_a, kWave);
  nt = nt < kSweepMax ? nt : kSweepMax;
  if (const char* e = getenv("FACPPG_DTW_ROWS")) {
    const int v = atoi(e) / kWave * kWave;
    if (v >= kWave && v < nt) nt = v;
  }
  for (int q = 0; (long)q * nt < longest_a; ++q) {
    if (q == 0)
      k_dtw_sweep<true><<<B, nt, 0, st>>>(w.dist, w.dist_pair, w.inf_cell, la_dev, lb_dev, Ta_max, Tb_max, band, q, w.bnd_c, w.bnd_n, w.bnd_m, cost_dev,
                                          steps_dev, agree_dev);
    else
      k_dtw_sweep<false><<<B, nt, 0, st>>>(w.dist, w.dist_pair, w.inf_cell, la_dev, lb_dev, Ta_max, Tb_max, band, q, w.bnd_c, w.bnd_n, w.bnd_m, cost_dev,
                                           steps_dev, agree_dev);
    FACPPG_HIP_CHECK(hipGetLastError());
  }
  return FACPPG_OK;
}

}  // namespace
}  // namespace facppg
