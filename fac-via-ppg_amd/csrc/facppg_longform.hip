// Long recordings (facppg.pipeline.synthesize_long): the three device steps around the cut planner.  The reference has no
// counterpart -- it decodes one utterance of at most max_decoder_steps frames and cuts a longer one off (model.py:527,
// generate_synthesis.py:90-93).
//   k_pause_flags      one byte per frame: does the mass of the pause rows of the PPG exceed the threshold (all the host reads)
//   k_gather_segments  segments of the padded PPG batch [B][K][Tmax] -> a fresh padded batch [S][K][Lmax], zeros behind each
//   k_join_segments    the segments' audio laid end to end, a linear fade on either side of every interior seam
// All three move frames / samples along the fast index of source and destination, a wave on consecutive addresses (flags and
// gather: four frames per lane; the join, whose seams fall on any sample, one); they are plain bounds-checked grid kernels
// (no cooperative launch, no waiting, no atomics).
#include <cstdint>

#include "facppg_common.h"

namespace facppg {
namespace {

// four floats from an address that is a multiple of 4 bytes only (a segment starts on any frame)
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kFlagThreads = 256;   // 4 frames per thread
constexpr int kRowsPerBlock = 4;    // gather: one wave per (segment, channel) row

// flags[b][t] = t < lengths[b] && x[b][rows[0]][t] + x[b][rows[1]][t] + ... > threshold.  The sum is ONE fp32 accumulator that
// takes the rows in the order given, additions only: the NumPy restatement that adds float32 rows in that order has the same bits.
__global__ void __launch_bounds__(kFlagThreads) k_pause_flags(const float* __restrict__ x, const int* __restrict__ lengths, int K, int Tmax,
                                                              const int* __restrict__ rows, int n_rows, float threshold,
                                                              unsigned char* __restrict__ flags) {
  const int b = blockIdx.y;
  const int t0 = (blockIdx.x * kFlagThreads + threadIdx.x) * 4;
  if (t0 >= Tmax) return;
  const int len = lengths[b];
  const int n = Tmax - t0 < 4 ? Tmax - t0 : 4;
  const float* xb = x + (size_t)b * K * Tmax;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (n == 4) {
    for (int r = 0; r < n_rows; ++r) {
      const f32x4_u v = *(const f32x4_u*)(xb + (size_t)rows[r] * Tmax + t0);
      if (r == 0) { acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w; }
      else { acc[0] = acc[0] + v.x; acc[1] = acc[1] + v.y; acc[2] = acc[2] + v.z; acc[3] = acc[3] + v.w; }
    }
  } else {
    for (int r = 0; r < n_rows; ++r)
      for (int i = 0; i < n; ++i) {
        const float v = xb[(size_t)rows[r] * Tmax + t0 + i];
        acc[i] = r == 0 ? v : acc[i] + v;
      }
  }
  unsigned char* f = flags + (size_t)b * Tmax + t0;
  for (int i = 0; i < n; ++i) f[i] = (t0 + i < len && acc[i] > threshold) ? 1 : 0;
}

// y[s][k][l] = l < frames_s ? x[b_s][k][start_s + l] : 0.  blockDim (64, kRowsPerBlock): a wave walks one row of y.
// VEC: Lmax % 4 == 0 and y 16-byte aligned -- every destination row then is, and is written as float4.
template <bool VEC>
__global__ void __launch_bounds__(kWave * kRowsPerBlock) k_gather_segments(const float* __restrict__ x, int K, int Tmax,
                                                                            const int* __restrict__ table, long rows_total, int Lmax,
                                                                            float* __restrict__ y) {
  const long row = (long)blockIdx.x * kRowsPerBlock + threadIdx.y;
  if (row >= rows_total) return;
  const int s = (int)(row / K), k = (int)(row % K);
  const int b = table[3 * s], start = table[3 * s + 1], frames = table[3 * s + 2];
  const float* src = x + ((size_t)b * K + k) * Tmax + start;
  float* dst = y + (size_t)row * Lmax;
  if (VEC) {
    for (int l = threadIdx.x * 4; l < Lmax; l += kWave * 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (l + 4 <= frames) {
        const f32x4_u u = *(const f32x4_u*)(src + l);
        v.x = u.x; v.y = u.y; v.z = u.z; v.w = u.w;
      } else {
        if (l < frames) v.x = src[l];
        if (l + 1 < frames) v.y = src[l + 1];
        if (l + 2 < frames) v.z = src[l + 2];
      }
      *(f32x4*)(dst + l) = v;
    }
  } else {
    for (int l = threadIdx.x; l < Lmax; l += kWave) dst[l] = l < frames ? src[l] : 0.f;
  }
}

// f_s = min(fade, n_s / 2) rounded down to a power of two (0: no fade)
__device__ __forceinline__ int seam_fade(int fade, int n) {
  int f = fade < n / 2 ? fade : n / 2;
  while (f & (f - 1)) f &= f - 1;
  return f;
}

// out[sum_{r < s} n_r + i] = gain_s(i) * audio[s][i], i < n_s.  gain: (2 i + 1) / (2 f_s) over the first f_s samples of a segment
// behind a seam, mirrored over the last f_s in front of one, 1 elsewhere: f_s is a power of two and 2 i + 1 < 2^24, so every
// gain is an fp32 number and the product rounds once.
__global__ void __launch_bounds__(256) k_join_segments(const float* __restrict__ audio, int Nmax, const int* __restrict__ n, int S, int fade,
                                                       float* __restrict__ out) {
  const int s = blockIdx.y;
  const int ns = n[s];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  size_t off = 0;
  for (int r = 0; r < s; ++r) off += (size_t)n[r];
  const int f = seam_fade(fade, ns);
  float v = audio[(size_t)s * Nmax + i];
  if (f > 0) {
    const float unit = 1.0f / (float)(2 * f);
    if (s > 0 && i < f) v = v * ((float)(2 * i + 1) * unit);
    if (s < S - 1 && i >= ns - f) v = v * ((float)(2 * (ns - 1 - i) + 1) * unit);
  }
  out[off + i] = v;
}

}  // namespace
}  // namespace facppg

using namespace facppg;

extern "C" int facppg_ppg_pause_flags(const float* x_dev, const int32_t* lengths_dev, int B, int K, int Tmax, const int32_t* rows_dev,
                                      const int32_t* rows_host, int n_rows, float threshold, uint8_t* flags_dev, void* stream_) {
  FACPPG_REQUIRE(x_dev && lengths_dev && rows_dev && rows_host && flags_dev, FACPPG_EINVAL, "facppg_ppg_pause_flags: NULL argument");
  FACPPG_REQUIRE(B >= 1 && K >= 1 && Tmax >= 1, FACPPG_EINVAL, "facppg_ppg_pause_flags: B, K, Tmax must be positive (got %d, %d, %d)", B, K, Tmax);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "facppg_ppg_pause_flags: at most 65535 recordings per call (got %d)", B);
  FACPPG_REQUIRE(n_rows >= 1, FACPPG_EINVAL, "facppg_ppg_pause_flags: n_rows must be at least 1 (got %d)", n_rows);
  for (int r = 0; r < n_rows; ++r)
    FACPPG_REQUIRE(rows_host[r] >= 0 && rows_host[r] < K, FACPPG_EINVAL, "facppg_ppg_pause_flags: row %d (%d) is outside [0, %d)", r, rows_host[r], K);
  FACPPG_REQUIRE(threshold > 0.0f && threshold < (float)n_rows, FACPPG_EINVAL,
                 "facppg_ppg_pause_flags: threshold %g is outside (0, %d), the range of a sum of %d posteriors", (double)threshold, n_rows, n_rows);
  const int per_block = kFlagThreads * 4;
  k_pause_flags<<<dim3((Tmax + per_block - 1) / per_block, B), kFlagThreads, 0, (hipStream_t)stream_>>>(x_dev, lengths_dev, K, Tmax, rows_dev,
                                                                                                        n_rows, threshold, flags_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_ppg_gather_segments(const float* x_dev, int B, int K, int Tmax, const int32_t* table_dev, const int32_t* table_host, int S,
                                          int Lmax, float* y_dev, void* stream_) {
  FACPPG_REQUIRE(x_dev && table_dev && table_host && y_dev, FACPPG_EINVAL, "facppg_ppg_gather_segments: NULL argument");
  FACPPG_REQUIRE(B >= 1 && K >= 1 && Tmax >= 1 && S >= 1 && Lmax >= 1, FACPPG_EINVAL,
                 "facppg_ppg_gather_segments: B, K, Tmax, S, Lmax must be positive (got %d, %d, %d, %d, %d)", B, K, Tmax, S, Lmax);
  for (int s = 0; s < S; ++s) {
    const int b = table_host[3 * s], start = table_host[3 * s + 1], frames = table_host[3 * s + 2];
    FACPPG_REQUIRE(b >= 0 && b < B, FACPPG_EINVAL, "facppg_ppg_gather_segments: segment %d names recording %d of %d", s, b, B);
    FACPPG_REQUIRE(start >= 0 && frames >= 1 && frames <= Lmax, FACPPG_EINVAL,
                   "facppg_ppg_gather_segments: segment %d: start %d, %d frames (start >= 0, 1 <= frames <= Lmax = %d)", s, start, frames, Lmax);
    FACPPG_REQUIRE((long)start + frames <= Tmax, FACPPG_EINVAL, "facppg_ppg_gather_segments: segment %d ends at frame %ld of %d", s,
                   (long)start + frames, Tmax);
  }
  const long rows_total = (long)S * K;
  const long blocks = (rows_total + kRowsPerBlock - 1) / kRowsPerBlock;
  FACPPG_REQUIRE(blocks <= 0x7fffffffl, FACPPG_EUNSUPPORTED, "facppg_ppg_gather_segments: %d segments of %d channels are too many rows for one launch", S, K);
  const dim3 block(kWave, kRowsPerBlock);
  hipStream_t st = (hipStream_t)stream_;
  if (Lmax % 4 == 0 && (uintptr_t)y_dev % 16 == 0)
    k_gather_segments<true><<<(unsigned)blocks, block, 0, st>>>(x_dev, K, Tmax, table_dev, rows_total, Lmax, y_dev);
  else
    k_gather_segments<false><<<(unsigned)blocks, block, 0, st>>>(x_dev, K, Tmax, table_dev, rows_total, Lmax, y_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_join_segments(const float* audio_dev, int Nmax, const int32_t* n_dev, const int32_t* n_host, int S, int fade, float* out_dev,
                                    void* stream_) {
  FACPPG_REQUIRE(audio_dev && n_dev && n_host && out_dev, FACPPG_EINVAL, "facppg_join_segments: NULL argument");
  FACPPG_REQUIRE(Nmax >= 1 && S >= 1, FACPPG_EINVAL, "facppg_join_segments: Nmax and S must be positive (got %d, %d)", Nmax, S);
  FACPPG_REQUIRE(S <= 65535, FACPPG_EUNSUPPORTED, "facppg_join_segments: at most 65535 segments per call (got %d)", S);
  FACPPG_REQUIRE(fade >= 0 && fade <= 4096 && (fade & (fade - 1)) == 0, FACPPG_EINVAL,
                 "facppg_join_segments: fade must be 0 or a power of two up to 4096 (got %d)", fade);
  int longest = 0;
  for (int s = 0; s < S; ++s) {
    FACPPG_REQUIRE(n_host[s] >= 0 && n_host[s] <= Nmax, FACPPG_EINVAL, "facppg_join_segments: segment %d has %d samples (0 <= n <= Nmax = %d)", s,
                   n_host[s], Nmax);
    longest = n_host[s] > longest ? n_host[s] : longest;
  }
  if (longest == 0) return FACPPG_OK;      // nothing to write
  k_join_segments<<<dim3((longest + 255) / 256, S), 256, 0, (hipStream_t)stream_>>>(audio_dev, Nmax, n_dev, S, fade, out_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
