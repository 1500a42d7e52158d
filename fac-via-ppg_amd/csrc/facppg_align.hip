// Per-phone report of a conversion (facppg.align): emissions of a padded PPG batch, a phone-loop decode of the teacher's own phone
// sequence, and a forced alignment of the converted audio's PPG to that sequence.  The reference has no counterpart -- its
// DataUtterance carries phone tiers that an external aligner produced from a transcript, and the wav -> wav path has neither.
// include/facppg.h states the definition; three kinds of launch:
//   k_align_emit    one workgroup per (utterance, 64 frames): reads x [D][Tmax] along the frames, writes em [sum T][D] along the
//                   classes -- the transpose goes through an LDS tile of 64 classes x 64 frames (rows padded to 65 floats), so both
//                   sides are coalesced; the frame's minimum emission and top class are combined from the four waves' partial ones
//   k_align_decode  one workgroup per utterance, one thread per class.  Per frame the first minimum of the costs of the frame
//                   before: a wave reduction (shuffles, then a ballot for the lowest lane that holds it); D <= 64 is one wave and has
//                   no barrier in the frame loop, D <= 256 combines up to four waves' minima through a two-slot LDS exchange with
//                   one barrier per frame.  Then thread 0 walks the one-byte back-pointers
//   k_align_force   one workgroup per utterance, one thread per state.  A state needs the costs of its two left neighbours of the
//                   frame before: S <= 64 takes them by shuffles (no barrier in the frame loop), more states through a two-slot LDS
//                   exchange -- one write, two reads, one barrier per frame.  Then thread 0 walks the one-byte back-pointers into
//                   (start, frames) per state, and every state sums its own segment's hits and goodness of pronunciation
// Emission rows are read kAhead frames ahead of their use.  A state whose cost is +inf loses every strict comparison and
// +inf + em stays +inf (em is finite by the floor), so the recurrences need no second case and no NaN can form.
// Every add is rounded on its own (contraction is off in this file).  Plain bounds-checked grid launches on the caller's stream;
// no cooperative launch, no waiting on memory, no atomics; every loop is bounded by the lengths.
#include <cmath>
#include <cstdint>

#include "facppg_common.h"

#pragma clang fp contract(off)

namespace facppg {
namespace {

constexpr int kEmitThreads = 256;
constexpr int kEmitTile = 64;        // frames of one k_align_emit workgroup, and classes of one pass over its LDS tile
constexpr int kClassMax = 256;       // classes at the most (threads of a k_align_decode workgroup)
constexpr int kStateMax = 1024;      // states of one utterance at the most (threads of a k_align_force workgroup)
constexpr int kAhead = 4;            // frames the two DPs read their emissions ahead of their use

// em[base + t][k] = -logf(max(x[b][k][t], floor)), eb[base + t] = min_k em, top[base + t] = arg max_k x (the lowest k on a tie), t < T_b
__global__ void __launch_bounds__(kEmitThreads) k_align_emit(const float* __restrict__ x, const int* __restrict__ foff, int D, int Tmax, float floor,
                                                             float* __restrict__ em, float* __restrict__ eb, int* __restrict__ top) {
  __shared__ float s_tile[kEmitTile][kEmitTile + 1];
  __shared__ float s_best[kEmitThreads / kWave][kEmitTile], s_min[kEmitThreads / kWave][kEmitTile];
  __shared__ int s_arg[kEmitThreads / kWave][kEmitTile];
  const int b = blockIdx.y, t0 = blockIdx.x * kEmitTile, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int base = foff[b], T = foff[b + 1] - base;
  if (t0 >= T) return;                       // (the whole workgroup)
  const int nf = T - t0 < kEmitTile ? T - t0 : kEmitTile;
  const bool in = lane < nf;                 // nothing behind the length is read
  const float* xp = x + (size_t)b * D * Tmax + t0 + lane;
  float* out = em + ((size_t)base + t0) * D;
  float best = -INFINITY, lowest = INFINITY;
  int arg = 0;
  for (int k0 = 0; k0 < D; k0 += kEmitTile) {
    const int kc = D - k0 < kEmitTile ? D - k0 : kEmitTile;
    if (in) {
      for (int kl = w; kl < kc; kl += kEmitThreads / kWave) {   // k increases: a strict > keeps the lowest class of a tie
        const float v = xp[(size_t)(k0 + kl) * Tmax];
        const float e = -logf(fmaxf(v, floor));
        s_tile[kl][lane] = e;
        if (v > best) { best = v; arg = k0 + kl; }
        lowest = fminf(lowest, e);
      }
    }
    __syncthreads();
    for (int i = tid; i < nf * kc; i += kEmitThreads) {         // frame-major: kc == D (one pass) makes the tile one contiguous run
      const int f = i / kc, kl = i - f * kc;
      out[(size_t)f * D + k0 + kl] = s_tile[kl][f];
    }
    __syncthreads();
  }
  s_best[w][lane] = best;
  s_arg[w][lane] = arg;
  s_min[w][lane] = lowest;
  __syncthreads();
  if (w == 0 && in) {                        // wave q holds the classes q, q + 4, ...: a tie between waves goes to the lower class
    for (int q = 1; q < kEmitThreads / kWave; ++q) {
      const float v = s_best[q][lane];
      const int a = s_arg[q][lane];
      if (v > best || (v == best && a < arg)) { best = v; arg = a; }
      lowest = fminf(lowest, s_min[q][lane]);
    }
    eb[base + t0 + lane] = lowest;
    top[base + t0 + lane] = arg;
  }
}

// the first minimum of c over the lanes of a wave: its value and the lowest lane that holds it
__device__ __forceinline__ float wave_first_min(float c, int* at) {
  float m = c;
  for (int o = 32; o >= 1; o >>= 1) m = fminf(m, __shfl_xor(m, o));
  *at = __ffsll((unsigned long long)__ballot(c == m)) - 1;
  return m;
}

// One utterance of the phone-loop decode.  WAVE: blockDim.x == 64 >= D; else blockDim.x a multiple of 64 >= D, at most kClassMax.
// bp [sum T][D] bytes: the class of the frame before.
template <bool WAVE>
__global__ void __launch_bounds__(kClassMax) k_align_decode(const float* __restrict__ em, const int* __restrict__ foff, int D, float switch_cost,
                                                            unsigned char* __restrict__ bp, int* __restrict__ labels, float* __restrict__ cost) {
  __shared__ float s_m[2][kClassMax / kWave];
  __shared__ int s_j[2][kClassMax / kWave];
  const int b = blockIdx.x, k = threadIdx.x, w = k >> 6, nw = blockDim.x >> 6;
  const int base = foff[b], T = foff[b + 1] - base;
  const bool active = k < D;
  const float inf = INFINITY;
  const float* e = em + (size_t)base * D + (active ? k : 0);
  unsigned char* bpu = bp + (size_t)base * D;

  // the workgroup's first minimum from the waves' (p: the LDS slot, alternating, so one barrier per use is enough)
  auto first_min = [&](float c, int p, int* at) -> float {
    int j;
    float m = wave_first_min(c, &j);
    j += w * kWave;
    if (!WAVE) {
      if ((k & 63) == 0) { s_m[p][w] = m; s_j[p][w] = j; }
      __syncthreads();
      m = s_m[p][0];
      j = s_j[p][0];
      for (int q = 1; q < nw; ++q)
        if (s_m[p][q] < m) { m = s_m[p][q]; j = s_j[p][q]; }
    }
    *at = j;
    return m;
  };

  // the row of a frame past the last one is the last one's (read, not used)
  auto fetch = [&](int t) -> float { return e[(size_t)(t < T ? t : T - 1) * D]; };
  float c = active ? e[0] : inf;
  float cur[kAhead], nxt[kAhead];
#pragma unroll
  for (int u = 0; u < kAhead; ++u) cur[u] = fetch(1 + u);
  for (int t0 = 1; t0 < T; t0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) nxt[u] = fetch(t0 + kAhead + u);
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int t = t0 + u;
      if (t < T) {                           // (uniform over the workgroup)
        int j;
        const float m = first_min(c, t & 1, &j);
        const float sw = m + switch_cost;
        const bool leave = sw < c;           // strict: a tie stays
        if (active) {
          c = cur[u] + (leave ? sw : c);
          bpu[(size_t)t * D + k] = (unsigned char)(leave ? j : k);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
  }
  int at;
  const float m = first_min(c, T & 1, &at);
  __threadfence_block();
  __syncthreads();                           // (the back-pointers of every thread are written)
  if (k == 0) {
    cost[b] = m;
    for (int t = T - 1; t >= 0; --t) {
      labels[base + t] = at;
      if (t > 0) at = bpu[(size_t)t * D + at];
    }
  }
}

// One utterance of the forced alignment.  WAVE: blockDim.x == 64 >= S; else blockDim.x a multiple of 64 >= S, at most kStateMax.
// bp [sum T][stride] bytes: 0 stay, 1 advance, 2 skip.
template <bool WAVE>
__global__ void __launch_bounds__(kStateMax) k_align_force(const float* __restrict__ em, const float* __restrict__ eb, const int* __restrict__ top,
                                                           const int* __restrict__ foff, int D, const int* __restrict__ seq,
                                                           const unsigned char* __restrict__ opt, const int* __restrict__ soff,
                                                           unsigned char* __restrict__ bp, int stride, int* __restrict__ start,
                                                           int* __restrict__ frames, int* __restrict__ hits, float* __restrict__ gop,
                                                           float* __restrict__ cost, int* __restrict__ ok) {
  // [t & 1][s + 2]: the costs of frame t; [.][0] and [.][1] stay +inf, so that states 0 and 1 read their missing neighbours there
  __shared__ float s_c[2][kStateMax + 2];
  __shared__ float s_last[kStateMax];
  __shared__ int s_start[kStateMax], s_frames[kStateMax];
  const int b = blockIdx.x, s = threadIdx.x, lane = s & 63;
  const int base = foff[b], T = foff[b + 1] - base;
  const int sb = soff[b], S = soff[b + 1] - sb;
  const bool active = s < S;
  const float inf = INFINITY;
  const int cls = active ? seq[sb + s] : 0;
  const bool may_skip = active && s >= 2 && opt[sb + s - 1] != 0;
  const float* e = em + (size_t)base * D + cls;
  unsigned char* bpu = bp + (size_t)base * stride;

  float c = inf;
  if (active && (s == 0 || (s == 1 && opt[sb] != 0))) c = e[0];
  s_start[s] = -1;
  s_frames[s] = 0;
  if (!WAVE) {
    s_c[0][s + 2] = c;
    if (s < 2) { s_c[0][s] = inf; s_c[1][s] = inf; }
    __syncthreads();
  }
  auto fetch = [&](int t) -> float { return e[(size_t)(t < T ? t : T - 1) * D]; };
  float cur[kAhead], nxt[kAhead];
#pragma unroll
  for (int u = 0; u < kAhead; ++u) cur[u] = fetch(1 + u);
  for (int t0 = 1; t0 < T; t0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) nxt[u] = fetch(t0 + kAhead + u);
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int t = t0 + u;
      if (t < T) {                           // (uniform over the workgroup)
        float c1, c2;
        if (WAVE) {
          c1 = __shfl_up(c, 1);
          c2 = __shfl_up(c, 2);
          if (lane < 1) c1 = inf;
          if (lane < 2) c2 = inf;
        } else {
          c1 = s_c[(t - 1) & 1][s + 1];
          c2 = s_c[(t - 1) & 1][s];
        }
        // stay, advance, skip, in that order with a strict <
        float best = c;
        int from = 0;
        if (c1 < best) { best = c1; from = 1; }
        if (may_skip && c2 < best) { best = c2; from = 2; }
        c = active ? best + cur[u] : inf;
        if (active) bpu[(size_t)t * stride + s] = (unsigned char)from;
        if (!WAVE) {
          s_c[t & 1][s + 2] = c;
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
  }
  s_last[s] = c;
  __threadfence_block();
  __syncthreads();                           // (the last costs and every back-pointer are written)
  if (s == 0) {
    int at = S - 1;
    if (S >= 2 && opt[sb + S - 1] != 0 && s_last[S - 2] < s_last[S - 1]) at = S - 2;
    const float total = s_last[at];
    cost[b] = total;
    // a finite cost is a path: there is one iff the utterance has at least as many frames as mandatory states
    ok[b] = total < inf ? 1 : 0;
    if (total < inf) {
      int last = T - 1;                      // the last frame of the segment being walked
      for (int t = T - 1; t >= 1; --t) {
        const int from = bpu[(size_t)t * stride + at];
        if (from) {
          s_start[at] = t;
          s_frames[at] = last - t + 1;
          at -= from;
          last = t - 1;
        }
      }
      s_start[at] = 0;
      s_frames[at] = last + 1;
    }
  }
  __syncthreads();
  if (!active) return;
  const int first = s_start[s], n = s_frames[s];
  float sum = 0.0f;
  int h = 0;
  for (int i = 0; i < n; ++i) {              // in frame order
    const int t = first + i;
    sum = sum + (eb[base + t] - e[(size_t)t * D]);
    h += top[base + t] == cls ? 1 : 0;
  }
  start[sb + s] = first;
  frames[sb + s] = n;
  hits[sb + s] = h;
  gop[sb + s] = n > 0 ? sum / (float)n : 0.0f;
}

int check_config(const facppg_align_config* c, const char* what) {
  FACPPG_REQUIRE(c, FACPPG_EINVAL, "%s: NULL argument", what);
  FACPPG_REQUIRE(c->floor > 0.0f && c->floor <= 1.0f, FACPPG_EINVAL, "%s: floor must lie in (0, 1] (got %g)", what, c->floor);
  FACPPG_REQUIRE(c->switch_cost >= 0.0f && c->switch_cost < 1e30f, FACPPG_EINVAL, "%s: switch_cost must be finite and not negative (got %g)", what,
                 c->switch_cost);
  return FACPPG_OK;
}

int check_batch(const int32_t* f_off, int B, int D, const char* what) {
  FACPPG_REQUIRE(B >= 1 && D >= 1, FACPPG_EINVAL, "%s: B and D must be positive (got %d, %d)", what, B, D);
  FACPPG_REQUIRE(D <= kClassMax, FACPPG_EUNSUPPORTED, "%s: at most %d classes per frame (got %d): reduce senone posteriors to monophone classes first",
                 what, kClassMax, D);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "%s: at most 65535 utterances per call (got %d)", what, B);
  return check_offsets(f_off, B, what);
}

size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace
}  // namespace facppg

using namespace facppg;

extern "C" int facppg_ppg_emissions(const facppg_align_config* cfg, const float* x_dev, int B, int D, int Tmax, const int32_t* frame_offsets_dev,
                                    const int32_t* frame_offsets_host, float* em_dev, float* eb_dev, int32_t* top_dev, void* stream_) {
  if (int rc = check_config(cfg, "facppg_ppg_emissions")) return rc;
  FACPPG_REQUIRE(x_dev && frame_offsets_dev && frame_offsets_host && em_dev && eb_dev && top_dev, FACPPG_EINVAL, "facppg_ppg_emissions: NULL argument");
  if (int rc = check_batch(frame_offsets_host, B, D, "facppg_ppg_emissions")) return rc;
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    const int T = frame_offsets_host[b + 1] - frame_offsets_host[b];
    FACPPG_REQUIRE(T <= Tmax, FACPPG_EINVAL, "facppg_ppg_emissions: utterance %d has %d frames, the batch is padded to Tmax = %d", b, T, Tmax);
    longest = T > longest ? T : longest;
  }
  k_align_emit<<<dim3((longest + kEmitTile - 1) / kEmitTile, B), kEmitThreads, 0, (hipStream_t)stream_>>>(x_dev, frame_offsets_dev, D, Tmax, cfg->floor,
                                                                                                     em_dev, eb_dev, top_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" size_t facppg_ppg_decode_phones_workspace_bytes(int total_frames, int D) {
  if (total_frames < 1 || D < 1 || D > kClassMax) {
    set_error("facppg_ppg_decode_phones_workspace_bytes: total_frames must be positive and D in [1, %d] (got %d, %d)", kClassMax, total_frames, D);
    return 0;
  }
  return round256((size_t)total_frames * D);
}

extern "C" int facppg_ppg_decode_phones(const facppg_align_config* cfg, const float* em_dev, const int32_t* frame_offsets_dev,
                                        const int32_t* frame_offsets_host, int B, int D, int32_t* labels_dev, float* cost_dev, void* ws_dev,
                                        size_t ws_bytes, void* stream_) {
  if (int rc = check_config(cfg, "facppg_ppg_decode_phones")) return rc;
  FACPPG_REQUIRE(em_dev && frame_offsets_dev && frame_offsets_host && labels_dev && cost_dev && ws_dev, FACPPG_EINVAL,
                 "facppg_ppg_decode_phones: NULL argument");
  if (int rc = check_batch(frame_offsets_host, B, D, "facppg_ppg_decode_phones")) return rc;
  const size_t need = round256((size_t)frame_offsets_host[B] * D);
  FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE,
                 "facppg_ppg_decode_phones: workspace of %zu bytes, facppg_ppg_decode_phones_workspace_bytes asks for %zu", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream_;
  if (D <= kWave)
    k_align_decode<true><<<B, kWave, 0, st>>>(em_dev, frame_offsets_dev, D, cfg->switch_cost, (unsigned char*)ws_dev, labels_dev, cost_dev);
  else
    k_align_decode<false><<<B, round_up(D, kWave), 0, st>>>(em_dev, frame_offsets_dev, D, cfg->switch_cost, (unsigned char*)ws_dev, labels_dev, cost_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" size_t facppg_ppg_force_align_workspace_bytes(int total_frames, int S_max) {
  if (total_frames < 1 || S_max < 1 || S_max > kStateMax) {
    set_error("facppg_ppg_force_align_workspace_bytes: total_frames must be positive and S_max in [1, %d] (got %d, %d)", kStateMax, total_frames, S_max);
    return 0;
  }
  return round256((size_t)total_frames * S_max);
}

extern "C" int facppg_ppg_force_align(const float* em_dev, const float* eb_dev, const int32_t* top_dev, const int32_t* frame_offsets_dev,
                                      const int32_t* frame_offsets_host, int B, int D, const int32_t* seq_dev, const int32_t* seq_host,
                                      const uint8_t* optional_dev, const uint8_t* optional_host, const int32_t* seq_offsets_dev,
                                      const int32_t* seq_offsets_host, int32_t* start_dev, int32_t* frames_dev, int32_t* hits_dev, float* gop_dev,
                                      float* cost_dev, int32_t* ok_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(em_dev && eb_dev && top_dev && frame_offsets_dev && frame_offsets_host && seq_dev && seq_host && optional_dev && optional_host &&
                     seq_offsets_dev && seq_offsets_host && start_dev && frames_dev && hits_dev && gop_dev && cost_dev && ok_dev && ws_dev,
                 FACPPG_EINVAL, "facppg_ppg_force_align: NULL argument");
  if (int rc = check_batch(frame_offsets_host, B, D, "facppg_ppg_force_align")) return rc;
  FACPPG_REQUIRE(seq_offsets_host[0] == 0, FACPPG_EINVAL, "facppg_ppg_force_align: sequence offsets must start at 0 (got %d)", seq_offsets_host[0]);
  int S_max = 0;
  for (int b = 0; b < B; ++b) {
    const int s0 = seq_offsets_host[b], S = seq_offsets_host[b + 1] - s0;
    FACPPG_REQUIRE(S >= 1, FACPPG_EINVAL, "facppg_ppg_force_align: utterance %d has %d states (at least 1)", b, S);
    FACPPG_REQUIRE(S <= kStateMax, FACPPG_EUNSUPPORTED, "facppg_ppg_force_align: utterance %d has %d states, a workgroup holds %d at the most", b, S,
                   kStateMax);
    for (int s = 0; s < S; ++s) {
      FACPPG_REQUIRE(seq_host[s0 + s] >= 0 && seq_host[s0 + s] < D, FACPPG_EINVAL,
                     "facppg_ppg_force_align: utterance %d, state %d: class %d is outside [0, %d)", b, s, seq_host[s0 + s], D);
      FACPPG_REQUIRE(s == 0 || !(optional_host[s0 + s] && optional_host[s0 + s - 1]), FACPPG_EINVAL,
                     "facppg_ppg_force_align: utterance %d: states %d and %d are both optional, the skip reaches over one state only", b, s - 1, s);
    }
    S_max = S > S_max ? S : S_max;
  }
  const size_t need = round256((size_t)frame_offsets_host[B] * S_max);
  FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE,
                 "facppg_ppg_force_align: workspace of %zu bytes, facppg_ppg_force_align_workspace_bytes asks for %zu", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream_;
  if (S_max <= kWave)
    k_align_force<true><<<B, kWave, 0, st>>>(em_dev, eb_dev, top_dev, frame_offsets_dev, D, seq_dev, optional_dev, seq_offsets_dev, (unsigned char*)ws_dev,
                                             S_max, start_dev, frames_dev, hits_dev, gop_dev, cost_dev, ok_dev);
  else
    k_align_force<false><<<B, round_up(S_max, kWave), 0, st>>>(em_dev, eb_dev, top_dev, frame_offsets_dev, D, seq_dev, optional_dev, seq_offsets_dev,
                                                               (unsigned char*)ws_dev, S_max, start_dev, frames_dev, hits_dev, gop_dev, cost_dev,
                                                               ok_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
