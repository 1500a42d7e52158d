// F0 track on the device (ppg.compute_f0, ppg.compute_ppg_padded(append_f0=True)): a normalised cross-correlation over the front
// end's own samples, one Viterbi pass per utterance over its peaks, and the reference's log-F0 / delta / delta-delta rows
// (append_ppg, src/common/data_utils.py:142-160) written into the padded batch the encoder reads.  The reference takes its F0 from
// WORLD through pyworld (utterance.py:33-38); this tracker is defined in include/facppg.h instead and held to a float64 restatement.
//
//   k_f0_nccf    one workgroup per (utterance, 8 frames), the frames' sample span staged once in LDS (zeros outside the
//                utterance's own [0, n)), one thread per lag column: per frame W steps of three fma chains -- the product, E(a) and
//                E(a + l), the last two from the very values the product reads, so the kernel is bound by its two LDS reads per
//                step and the energies cost nothing (a running sum over l would carry its rounding from a loud stretch into a
//                quiet one).  Each chain is 8 partial sums (j mod 8) added pairwise: the order depends on nothing but W, so a
//                frame has the same bits in any batch
//   k_f0_local   one wave per frame: the peaks, dv (+inf off a peak) and du of the definition, [sum T][L + 1] with du in column 0
//   k_f0_track   one workgroup per utterance, one thread per state.  A state whose cost is +inf can never win the strict < against
//                the always-finite unvoiced predecessor, so after every frame the finite voiced states are compacted IN STATE ORDER
//                (ballot + popcount per wave, wave counts through LDS) into (cost, log2 lag, state) lists and the next frame's
//                predecessor loop walks that list: a few tens of entries on speech, not L.  Three barriers per frame; the local
//                costs are read a frame ahead.  Then thread 0 finds the first minimum and walks the back-pointers, and the
//                workgroup refines the lags into Hz
//   k_lf0_rows   one thread per (utterance, frame of the padded batch): log, delta and delta-delta, zeros behind the utterance
// Every multiply and add of the tracker is rounded on its own (contraction is off in this file; the NCCF's fma are explicit).
// Plain bounds-checked grid launches on the caller's stream; no atomics; every loop is bounded by the lengths.
#include <cmath>
#include <cstdint>

#include "facppg_common.h"

#pragma clang fp contract(off)

namespace facppg {
namespace {

constexpr int kNccfFrames = 8;       // frames of one k_f0_nccf workgroup
constexpr int kNccfLdsFloats = 15360;  // 60 KB of the 64 KB a workgroup may take without asking
constexpr int kTrackMax = 1024;      // states of one utterance at the most (threads of a k_f0_track workgroup)

struct F0Ws { size_t local, bp, nccf, total; };
F0Ws f0_ws(const facppg_f0_config* c, int total_frames) {
  const size_t L = (size_t)(c->lag_max - c->lag_min + 1), T = (size_t)total_frames;
  F0Ws w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.local = take(T * (L + 1) * 4);
  w.bp = take(T * (L + 1) * 2);
  w.nccf = take(T * (L + 2) * 4);
  w.total = off;
  return w;
}

int check_config(const facppg_f0_config* c, const char* what) {
  FACPPG_REQUIRE(c, FACPPG_EINVAL, "%s: NULL argument", what);
  FACPPG_REQUIRE(c->sample_rate >= 1 && c->frame_shift >= 1, FACPPG_EINVAL, "%s: sample_rate and frame_shift must be positive (got %d, %d)", what,
                 c->sample_rate, c->frame_shift);
  FACPPG_REQUIRE(c->window >= 1, FACPPG_EINVAL, "%s: window must be at least 1 (got %d)", what, c->window);
  FACPPG_REQUIRE(c->lag_min >= 2, FACPPG_EINVAL, "%s: lag_min must be at least 2 (got %d): the column below it is lag_min - 1", what, c->lag_min);
  FACPPG_REQUIRE(c->lag_max < 2048, FACPPG_EINVAL, "%s: lag_max must be below 2048 (got %d)", what, c->lag_max);
  FACPPG_REQUIRE(c->lag_max >= c->lag_min, FACPPG_EINVAL, "%s: lag_max %d is below lag_min %d", what, c->lag_max, c->lag_min);
  FACPPG_REQUIRE(c->ballast >= 0.0f && c->ballast < 1e6f && c->voicing_cost >= 0.0f && c->freq_weight >= 0.0f, FACPPG_EINVAL,
                 "%s: ballast, voicing_cost and freq_weight must be finite and not negative (got %g, %g, %g)", what, c->ballast, c->voicing_cost,
                 c->freq_weight);
  FACPPG_REQUIRE(c->lag_max - c->lag_min + 2 <= kTrackMax, FACPPG_EUNSUPPORTED, "%s: at most %d candidate lags (got %d .. %d)", what, kTrackMax - 1,
                 c->lag_min, c->lag_max);
  const long span = (long)(kNccfFrames - 1) * c->frame_shift + c->window + c->lag_max + 1;
  FACPPG_REQUIRE(span <= kNccfLdsFloats, FACPPG_EUNSUPPORTED,
                 "%s: %d frames at shift %d with window %d and lag_max %d span %ld samples, a workgroup stages %d at the most", what, kNccfFrames,
                 c->frame_shift, c->window, c->lag_max, span, kNccfLdsFloats);
  return FACPPG_OK;
}

// frame offsets (host): off[0] = 0, increasing; with sample offsets: T_b = (n_b + S / 2) / S
int check_frames(const facppg_f0_config* c, const int32_t* s_off, const int32_t* f_off, int B, const char* what) {
  FACPPG_REQUIRE(B >= 1, FACPPG_EINVAL, "%s: B must be at least 1 (got %d)", what, B);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "%s: at most 65535 utterances per call (got %d)", what, B);
  if (int rc = check_offsets(f_off, B, what)) return rc;
  if (!s_off) return FACPPG_OK;
  if (int rc = check_offsets(s_off, B, what)) return rc;
  for (int b = 0; b < B; ++b) {
    const int n = s_off[b + 1] - s_off[b];
    const long T = ((long)n + c->frame_shift / 2) / c->frame_shift;
    FACPPG_REQUIRE(T > 0, FACPPG_EINVAL, "no frames in %d samples", n);      // (facppg_mfcc_compute's refusal)
    FACPPG_REQUIRE(f_off[b + 1] - f_off[b] == T, FACPPG_EINVAL, "utterance %d: %d samples are %ld frames, the frame offsets say %d", b, n, T,
                   f_off[b + 1] - f_off[b]);
  }
  return FACPPG_OK;
}

__device__ __forceinline__ float sum8(const float* s) { return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])); }

// Frames t0 .. t0 + 7 of utterance blockIdx.y.  s_x[i] = x[a0 + i], a0 = a(t0): frame t0 + f reads s_x[f S + j] and s_x[f S + l + j],
// j < W, l <= lag_max + 1: the last index is (nf - 1) S + lag_max + W, below the (nf - 1) S + W + lag_max + 1 floats staged.
__global__ void __launch_bounds__(1024) k_f0_nccf(const float* __restrict__ wav, const int* __restrict__ soff, const int* __restrict__ foff, int S, int W,
                                                  int lag_min, int lag_max, float ballast2, float* __restrict__ nccf) {
  extern __shared__ float s_x[];
  const int b = blockIdx.y, t0 = blockIdx.x * kNccfFrames, tid = threadIdx.x;
  const int T = foff[b + 1] - foff[b];
  if (t0 >= T) return;                       // (the whole workgroup)
  const int n = soff[b + 1] - soff[b];
  const float* x = wav + soff[b];
  const int nf = T - t0 < kNccfFrames ? T - t0 : kNccfFrames;
  const long a0 = (long)t0 * S + S / 2 - (W + lag_max + 1) / 2;
  const int used = (nf - 1) * S + W + lag_max + 1;
  for (int i = tid; i < used; i += blockDim.x) {
    const long p = a0 + i;
    s_x[i] = (p >= 0 && p < n) ? x[p] : 0.0f;
  }
  __syncthreads();
  const int ncol = lag_max - lag_min + 3;
  for (int c = tid; c < ncol; c += blockDim.x) {
    const int l = lag_min - 1 + c;
    for (int f = 0; f < nf; ++f) {
      const float* u = s_x + f * S;
      const float* v = u + l;
      float d[8], e0[8], el[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) d[q] = e0[q] = el[q] = 0.0f;
      int j = 0;
      for (; j + 8 <= W; j += 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float p = u[j + q], r = v[j + q];
          d[q] = fmaf(p, r, d[q]);
          e0[q] = fmaf(p, p, e0[q]);
          el[q] = fmaf(r, r, el[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (j + q < W) {
          const float p = u[j + q], r = v[j + q];
          d[q] = fmaf(p, r, d[q]);
          e0[q] = fmaf(p, p, e0[q]);
          el[q] = fmaf(r, r, el[q]);
        }
      nccf[((size_t)foff[b] + t0 + f) * ncol + c] = sum8(d) / sqrtf(sum8(e0) * sum8(el) + ballast2);
    }
  }
}

// local[g][0] = du = max of phi over lag_min .. lag_max; local[g][s] = dv of state s (column s of the row), +inf off a peak.
// tables: wl [L], then g [L].  One wave per frame: no barrier, so a wave past the last frame just leaves.
__global__ void __launch_bounds__(256) k_f0_local(const float* __restrict__ nccf, int total, int L, const float* __restrict__ tables,
                                                  float* __restrict__ local) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= total) return;
  const float* row = nccf + (size_t)g * (L + 2);
  float* out = local + (size_t)g * (L + 1);
  float mx = -INFINITY;
  for (int s = 1 + lane; s <= L; s += 64) {
    const float p = row[s - 1], q = row[s], r = row[s + 1];
    mx = fmaxf(mx, q);
    out[s] = (q >= p && q > r) ? 1.0f - q * tables[s - 1] : INFINITY;
  }
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
  if (lane == 0) out[0] = mx;
}

// One utterance: the Viterbi pass, the backtrace and the refinement.  blockDim.x >= L + 1, a multiple of 64.
__global__ void __launch_bounds__(kTrackMax) k_f0_track(const float* __restrict__ nccf, const float* __restrict__ local, const int* __restrict__ foff,
                                                        int L, int lag_min, float sample_rate, float vuv, float omega,
                                                        const float* __restrict__ tables, uint16_t* __restrict__ bp, int* __restrict__ lag_out,
                                                        float* __restrict__ f0_out) {
  // the finite voiced states of the frame before, in state order: cost, log2 of the lag, state; later: the last frame's costs
  __shared__ float s_pc[kTrackMax], s_pg[kTrackMax];
  __shared__ int s_ps[kTrackMax];
  __shared__ int s_wcount[kTrackMax / kWave];
  __shared__ float s_c0;
  __shared__ int s_n;
  const int b = blockIdx.x, s = threadIdx.x, lane = s & 63, w = s >> 6;
  const int base = foff[b], T = foff[b + 1] - base, NS = L + 1;
  const bool active = s < NS;
  const float inf = INFINITY;
  const float* loc = local + (size_t)base * NS;
  uint16_t* bpu = bp + (size_t)base * NS;
  const float g_l = (active && s >= 1) ? tables[L + s - 1] : 0.0f;
  float c = inf;
  float nxt = active ? loc[s] : inf;
  for (int t = 0; t < T; ++t) {
    const float mine = nxt;
    if (t + 1 < T) nxt = active ? loc[(size_t)(t + 1) * NS + s] : inf;
    if (t == 0) {
      c = mine;
    } else {
      int arg = 0;
      c = inf;
      if (mine < inf) {                      // state 0 (du is finite) and the peaks of this frame
        const int n = s_n;
        const float c0 = s_c0;
        float best = s == 0 ? c0 : c0 + vuv;
        for (int i = 0; i < n; ++i) {
          const float trans = s == 0 ? vuv : omega * fabsf(g_l - s_pg[i]);
          const float cand = s_pc[i] + trans;
          if (cand < best) { best = cand; arg = s_ps[i]; }
        }
        c = best + mine;
      }
      if (active) bpu[(size_t)t * NS + s] = (uint16_t)arg;
    }
    __syncthreads();                         // (every thread has read the lists of the frame before)
    const bool flag = active && s >= 1 && c < inf;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_wcount[w] = __popcll(m);
    if (s == 0) s_c0 = c;
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) pos += s_wcount[k];
    if (flag) { s_pc[pos] = c; s_pg[pos] = g_l; s_ps[pos] = s; }
    if (s == (int)blockDim.x - 1) s_n = pos + (flag ? 1 : 0);
    __syncthreads();
  }
  // the first minimum of C(T - 1, .), then the back-pointers
  s_pc[s] = active ? c : inf;
  __threadfence_block();
  __syncthreads();
  if (s == 0) {
    int at = 0;
    float best = s_pc[0];
    for (int k = 1; k < NS; ++k)
      if (s_pc[k] < best) { best = s_pc[k]; at = k; }
    for (int t = T - 1; t >= 0; --t) {
      lag_out[base + t] = at ? lag_min + at - 1 : 0;
      if (t > 0) at = bpu[(size_t)t * NS + at];
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int t = s; t < T; t += blockDim.x) {
    const int l = lag_out[base + t];
    float f0 = 0.0f;
    if (l) {
      const float* row = nccf + ((size_t)base + t) * (L + 2) + (l - lag_min);   // columns of l - 1, l, l + 1
      const float p = row[0], q = row[1], r = row[2];
      const float den = (p - (q + q)) + r;
      const float delta = den < 0.0f ? 0.5f * (p - r) / den : 0.0f;
      f0 = sample_rate / ((float)l + delta);
    }
    f0_out[base + t] = f0;
  }
}

// out[b * bstride + r * Tmax + t], r = 0 .. 2: log F0, delta, delta-delta of frame t of utterance b; 0 for T_b <= t < Tmax.
__global__ void __launch_bounds__(256) k_lf0_rows(const float* __restrict__ f0, const int* __restrict__ foff, int Tmax, size_t bstride,
                                                  float* __restrict__ out) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tmax) return;
  const int T = foff[b + 1] - foff[b];
  float* o = out + (size_t)b * bstride + t;
  if (t >= T) {
    o[0] = 0.0f; o[Tmax] = 0.0f; o[(size_t)2 * Tmax] = 0.0f;
    return;
  }
  const float* f = f0 + foff[b];
  auto x0 = [&](int i) { return logf(f[i < 0 ? 0 : i > T - 1 ? T - 1 : i] + 2.220446e-16f); };
  const float m2 = x0(t - 2), m1 = x0(t - 1), z = x0(t), p1 = x0(t + 1), p2 = x0(t + 2);
  o[0] = z;
  o[Tmax] = 0.5f * (p1 - m1);
  o[(size_t)2 * Tmax] = (0.25f * m2 - 0.5f * z) + 0.25f * p2;
}

int launch_nccf(const facppg_f0_config* c, const float* wav_dev, const int32_t* s_off_dev, const int32_t* f_off_dev, const int32_t* f_off_host, int B,
                float* nccf_dev, hipStream_t st) {
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = f_off_host[b + 1] - f_off_host[b] > longest ? f_off_host[b + 1] - f_off_host[b] : longest;
  const int ncol = c->lag_max - c->lag_min + 3;
  const int nt = round_up(ncol, kWave) < 1024 ? round_up(ncol, kWave) : 1024;
  const size_t lds = ((size_t)(kNccfFrames - 1) * c->frame_shift + c->window + c->lag_max + 1) * 4;
  const float wb = (float)c->window * c->ballast * c->ballast;
  k_f0_nccf<<<dim3((longest + kNccfFrames - 1) / kNccfFrames, B), nt, lds, st>>>(wav_dev, s_off_dev, f_off_dev, c->frame_shift, c->window, c->lag_min,
                                                                                c->lag_max, wb * wb, nccf_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

int launch_track(const facppg_f0_config* c, const float* nccf_dev, const int32_t* f_off_dev, const int32_t* f_off_host, int B, const float* tables_dev,
                 int32_t* lag_dev, float* f0_dev, char* ws, const F0Ws& lay, hipStream_t st) {
  const int L = c->lag_max - c->lag_min + 1, total = f_off_host[B];
  float* local = (float*)(ws + lay.local);
  k_f0_local<<<(total + 3) / 4, 256, 0, st>>>(nccf_dev, total, L, tables_dev, local);
  FACPPG_HIP_CHECK(hipGetLastError());
  k_f0_track<<<B, round_up(L + 1, kWave), 0, st>>>(nccf_dev, local, f_off_dev, L, c->lag_min, (float)c->sample_rate, c->voicing_cost, c->freq_weight,
                                                   tables_dev, (uint16_t*)(ws + lay.bp), lag_dev, f0_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

}  // namespace
}  // namespace facppg

using namespace facppg;

extern "C" size_t facppg_f0_workspace_bytes(const facppg_f0_config* cfg, int total_frames) {
  if (check_config(cfg, "facppg_f0_workspace_bytes")) return 0;
  if (total_frames < 1) {
    set_error("facppg_f0_workspace_bytes: total_frames must be positive (got %d)", total_frames);
    return 0;
  }
  return f0_ws(cfg, total_frames).total;
}

extern "C" int facppg_f0_nccf_batch(const facppg_f0_config* cfg, const float* wav_dev, const int32_t* sample_offsets_dev,
                                    const int32_t* sample_offsets_host, const int32_t* frame_offsets_dev, const int32_t* frame_offsets_host, int B,
                                    float* nccf_dev, void* stream_) {
  if (int rc = check_config(cfg, "facppg_f0_nccf_batch")) return rc;
  FACPPG_REQUIRE(wav_dev && sample_offsets_dev && sample_offsets_host && frame_offsets_dev && frame_offsets_host && nccf_dev, FACPPG_EINVAL,
                 "facppg_f0_nccf_batch: NULL argument");
  if (int rc = check_frames(cfg, sample_offsets_host, frame_offsets_host, B, "facppg_f0_nccf_batch")) return rc;
  return launch_nccf(cfg, wav_dev, sample_offsets_dev, frame_offsets_dev, frame_offsets_host, B, nccf_dev, (hipStream_t)stream_);
}

extern "C" int facppg_f0_track_batch(const facppg_f0_config* cfg, const float* nccf_dev, const int32_t* frame_offsets_dev,
                                     const int32_t* frame_offsets_host, int B, const float* tables_dev, int32_t* lag_dev, float* f0_dev, void* ws_dev,
                                     size_t ws_bytes, void* stream_) {
  if (int rc = check_config(cfg, "facppg_f0_track_batch")) return rc;
  FACPPG_REQUIRE(nccf_dev && frame_offsets_dev && frame_offsets_host && tables_dev && lag_dev && f0_dev && ws_dev, FACPPG_EINVAL,
                 "facppg_f0_track_batch: NULL argument");
  if (int rc = check_frames(cfg, nullptr, frame_offsets_host, B, "facppg_f0_track_batch")) return rc;
  const F0Ws lay = f0_ws(cfg, frame_offsets_host[B]);
  FACPPG_REQUIRE(ws_bytes >= lay.total, FACPPG_EWORKSPACE, "facppg_f0_track_batch: workspace of %zu bytes, facppg_f0_workspace_bytes asks for %zu",
                 ws_bytes, lay.total);
  return launch_track(cfg, nccf_dev, frame_offsets_dev, frame_offsets_host, B, tables_dev, lag_dev, f0_dev, (char*)ws_dev, lay, (hipStream_t)stream_);
}

extern "C" int facppg_f0_batch(const facppg_f0_config* cfg, const float* wav_dev, const int32_t* sample_offsets_dev, const int32_t* sample_offsets_host,
                               const int32_t* frame_offsets_dev, const int32_t* frame_offsets_host, int B, const float* tables_dev, int32_t* lag_dev,
                               float* f0_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
  if (int rc = check_config(cfg, "facppg_f0_batch")) return rc;
  FACPPG_REQUIRE(wav_dev && sample_offsets_dev && sample_offsets_host && frame_offsets_dev && frame_offsets_host && tables_dev && lag_dev && f0_dev &&
                     ws_dev,
                 FACPPG_EINVAL, "facppg_f0_batch: NULL argument");
  if (int rc = check_frames(cfg, sample_offsets_host, frame_offsets_host, B, "facppg_f0_batch")) return rc;
  const F0Ws lay = f0_ws(cfg, frame_offsets_host[B]);
  FACPPG_REQUIRE(ws_bytes >= lay.total, FACPPG_EWORKSPACE, "facppg_f0_batch: workspace of %zu bytes, facppg_f0_workspace_bytes asks for %zu", ws_bytes,
                 lay.total);
  hipStream_t st = (hipStream_t)stream_;
  float* nccf = (float*)((char*)ws_dev + lay.nccf);
  if (int rc = launch_nccf(cfg, wav_dev, sample_offsets_dev, frame_offsets_dev, frame_offsets_host, B, nccf, st)) return rc;
  return launch_track(cfg, nccf, frame_offsets_dev, frame_offsets_host, B, tables_dev, lag_dev, f0_dev, (char*)ws_dev, lay, st);
}

extern "C" int facppg_lf0_rows_padded(const float* f0_dev, const int32_t* frame_offsets_dev, const int32_t* frame_offsets_host, int B, int Tmax,
                                      size_t batch_stride, float* out_dev, void* stream_) {
  FACPPG_REQUIRE(f0_dev && frame_offsets_dev && frame_offsets_host && out_dev, FACPPG_EINVAL, "facppg_lf0_rows_padded: NULL argument");
  if (int rc = check_frames(nullptr, nullptr, frame_offsets_host, B, "facppg_lf0_rows_padded")) return rc;
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = frame_offsets_host[b + 1] - frame_offsets_host[b] > longest ? frame_offsets_host[b + 1] - frame_offsets_host[b] : longest;
  FACPPG_REQUIRE(Tmax >= longest, FACPPG_EINVAL, "facppg_lf0_rows_padded: Tmax %d is shorter than the longest utterance (%d frames)", Tmax, longest);
  FACPPG_REQUIRE(batch_stride >= (size_t)3 * Tmax, FACPPG_EINVAL, "facppg_lf0_rows_padded: a batch stride of %zu floats is shorter than 3 rows of %d",
                 batch_stride, Tmax);
  k_lf0_rows<<<dim3((Tmax + 255) / 256, B), 256, 0, (hipStream_t)stream_>>>(f0_dev, frame_offsets_dev, Tmax, batch_stride, out_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
