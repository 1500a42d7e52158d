// nnet3 TDNN acoustic-model inference for MI355X (gfx950): feature frames -> senone posteriors (PPGs).
//
// Replaces the reference's compute_full_ppg (src/ppg/compute_ppg.py:42-70), which drives Kaldi's
// nnet3::DecodableNnetSimple through PyKaldi: set_batchnorm_test_mode / collapse_model, then the network output for
// every frame, with the input replicated at the utterance edges for the model's left / right context.
//
// The host side (common/nnet3.py plan_layers) hands over a chain of fused layers, each
//     y[:, t] = act(W . [x[:, t + first]; x[:, t + first + dil]; ...; x[:, t + first + (taps-1) dil]] + b)   (+ renorm)
// with test-mode BatchNorm already folded into the consuming layer.  Activations are channel-major [C][Tp],
// Tp = L + T + R frames (positions contiguous: coalesced loads, the layout k_gemm wants); every layer is the exact-fp32
// MFMA tapped GEMM of facppg_gemm.hip.  k_gemm reads columns n + tap*dil (pad = 0), so layer l stores true frame t at
// column t - s_l with s_l = s_{l-1} - first_l, s_0 = -L: the shifts telescope to s_last = 0, i.e. the last layer's
// columns 0..T-1 are frames 0..T-1, and the columns polluted by the zero fill past Tp lie outside every frame's
// dependency cone.  Bound: MFMA for the two big products (input splice x hidden, hidden x senones), latency otherwise.
#include <cmath>
#include <new>
#include <vector>

#include "facppg_gemm.h"

using namespace facppg;

struct facppg_tdnn {
  int device = 0, n_cu = 256;
  int n_layers = 0, final_op = 0, in_dim = 0, out_dim = 0, left = 0, right = 0, max_dim = 0;
  std::vector<facppg_tdnn_layer> layers;
  std::vector<float4*> A;
  std::vector<float*> bias;
  float* arena = nullptr;
};

namespace {

// feats [T][D] row-major -> x0 [D][Tp], x0[c][j] = feats[clamp(j - L, 0, T-1)][c]  (DecodableNnetSimple replicates the
// first / last frame for the context beyond the utterance)
__global__ void k_tdnn_input(const float* __restrict__ feats, float* __restrict__ x0, int T, int D, int L, int Tp) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (j >= Tp) return;
  const int t = min(max(j - L, 0), T - 1);
  x0[(size_t)c * Tp + j] = feats[(size_t)t * D + c];
}

// NormalizeComponent (nnet-normalize-component.cc): y = x * (max(sum x^2 / (C * rms^2), 2^-66))^(-1/2), per frame
__global__ void k_tdnn_renorm(float* __restrict__ x, int C, int Tp, float target_rms) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Tp) return;
  float ss = 0.0f;
  for (int c = 0; c < C; ++c) { const float v = x[(size_t)c * Tp + j]; ss = fmaf(v, v, ss); }
  const float floor_ = 1.3552527156068805e-20f;   // 2^-66 (kSquaredNormFloor)
  const float scale = 1.0f / sqrtf(fmaxf(ss / ((float)C * target_rms * target_rms), floor_));
  for (int c = 0; c < C; ++c) x[(size_t)c * Tp + j] *= scale;
}

// (Log)Softmax over the M channels of frames 0..T-1; writes out [T][M] row-major.  final_op: 0 copy, 1 softmax, 2 log-softmax
__global__ void k_tdnn_output(const float* __restrict__ y, int M, int Tp, int T, int final_op, float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  float mx = -INFINITY, sum = 0.0f;
  if (final_op != 0) {
    for (int m = 0; m < M; ++m) mx = fmaxf(mx, y[(size_t)m * Tp + t]);
    for (int m = 0; m < M; ++m) sum += expf(y[(size_t)m * Tp + t] - mx);
  }
  const float lse = logf(sum);
  for (int m = 0; m < M; ++m) {
    const float v = y[(size_t)m * Tp + t];
    out[(size_t)t * M + m] = final_op == 0 ? v : final_op == 1 ? expf(v - mx) / sum : v - mx - lse;
  }
}

// ---- batch form: B utterances laid end to end, one column space -------------------------------------------------------
// Utterance b owns the columns cs[b] .. cs[b+1]-1, cs[b+1] - cs[b] = round_up(L + T_b + R, 4) (the rounding keeps every
// segment's start on a 16-byte boundary of its row), laid out inside exactly as the single-utterance form lays out its
// Tp columns.  k_gemm reads columns n + tap*dil across a join, but only into columns outside every valid frame's
// dependency cone: by the telescoping shifts above, frame t of utterance b at the last layer depends on the segment's own
// columns t .. t + L + R alone.

// cs[b] = sum_{i < b} round_up(L + T_i + R, 4), b = 0..B  (B is small against the column count: each thread sums its own prefix)
__global__ void k_tdnn_colstart(const int* __restrict__ off, int B, int LR, int* __restrict__ cs) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > B) return;
  int c = 0;
  for (int i = 0; i < b; ++i) c += (LR + off[i + 1] - off[i] + 3) & ~3;
  cs[b] = c;
}

// ragged k_tdnn_input: x0[c][cs[b] + j] = feats[off[b] + clamp(j - L, 0, T_b - 1)][c] for every column j of segment b
__global__ void k_tdnn_input_batch(const float* __restrict__ feats, const int* __restrict__ off, const int* __restrict__ cs, int B,
                                   float* __restrict__ x0, int D, int L, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (n >= N) return;
  const int b = seg_of(cs, B, n), T = off[b + 1] - off[b];
  const int t = min(max(n - cs[b] - L, 0), T - 1);
  x0[(size_t)c * N + n] = feats[(size_t)(off[b] + t) * D + c];
}

// ragged k_tdnn_output: frame g of the batch (utterance b, frame g - off[b]) sits in column cs[b] + g - off[b]; same
// arithmetic per frame, in the same order, as k_tdnn_output
__global__ void k_tdnn_output_batch(const float* __restrict__ y, const int* __restrict__ off, const int* __restrict__ cs, int B, int M,
                                    int N, int final_op, float* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= off[B]) return;
  const int b = seg_of(off, B, g), t = cs[b] + g - off[b];
  float mx = -INFINITY, sum = 0.0f;
  if (final_op != 0) {
    for (int m = 0; m < M; ++m) mx = fmaxf(mx, y[(size_t)m * N + t]);
    for (int m = 0; m < M; ++m) sum += expf(y[(size_t)m * N + t] - mx);
  }
  const float lse = logf(sum);
  for (int m = 0; m < M; ++m) {
    const float v = y[(size_t)m * N + t];
    out[(size_t)g * M + m] = final_op == 0 ? v : final_op == 1 ? expf(v - mx) / sum : v - mx - lse;
  }
}

// Softmax fused with reduce_ppg_dim (compute_ppg.py:73-94): out[g][d] = sum_m softmax(y[:, col(g)])[m] * Rt[m][d], without
// the [frames][M] posterior matrix in between.  One workgroup = MONO_FT consecutive frames of the batch.
//  - logits are read as (frame f = tid % 16, channel row r = tid / 16): 16 neighbouring columns per channel row;
//  - max and sum of exp: per thread over its channel rows, then over the 4 rows of a wave by lane exchange and over the 4
//    waves through LDS;
//  - exp(y - max) goes through LDS in chunks of MONO_CH channels x 16 frames; thread (d = tid % 64, part = tid / 64) keeps
//    the 16 frames' sums of column d in registers and walks the chunk's channels part, part + 4, ..: one (coalesced) read of
//    Rt per 16 multiply-adds, the posteriors broadcast from LDS;
//  - the division by the sum of exp is applied once per output.
// PADDED = false stores out [sum T][Md] (frame g's row); PADDED = true stores the same values into out [B][Md][Tmax], the layout
// the encoder reads (frame t of utterance b at out[b * bstride + d * Tmax + t], bstride >= Md * Tmax floats from one utterance to
// the next; the columns T_b .. Tmax-1 are k_tdnn_zero_padding's):
// the 16 frames of the tile then lie along the lanes, so that the stores of a channel row are neighbours.
constexpr int MONO_FT = 16, MONO_CH = 256;
template <bool PADDED>
__global__ __launch_bounds__(256) void k_tdnn_mono(const float* __restrict__ y, const int* __restrict__ off, const int* __restrict__ cs,
                                                   int B, int M, int N, const float* __restrict__ Rt, int Md, float* __restrict__ out,
                                                   int Tmax, size_t bstride) {
  __shared__ __attribute__((aligned(16))) float pe[MONO_CH * MONO_FT];   // later: the 4 parts' sums [4][16][64]
  __shared__ float red[4][MONO_FT], mxs[MONO_FT], sums[MONO_FT];
  __shared__ int col[MONO_FT];
  __shared__ size_t dst[MONO_FT];      // PADDED: offset of out[b][0][t] for the tile's frames
  const int tid = threadIdx.x, f = tid & 15, r = tid >> 4, d = tid & 63, part = tid >> 6;
  const int g0 = blockIdx.x * MONO_FT, G = off[B];
  if (tid < MONO_FT) {
    const int g = min(g0 + tid, G - 1);      // a frame past the end repeats the last one (never stored)
    const int b = seg_of(off, B, g);
    col[tid] = cs[b] + g - off[b];
    if (PADDED) dst[tid] = (size_t)b * bstride + (g - off[b]);
  }
  __syncthreads();
  const float* yc = y + col[f];
  float mx = -INFINITY;
  for (int m = r; m < M; m += 16) mx = fmaxf(mx, yc[(size_t)m * N]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if ((tid & 63) < 16) red[part][f] = mx;
  __syncthreads();
  if (tid < MONO_FT) mxs[tid] = fmaxf(fmaxf(red[0][tid], red[1][tid]), fmaxf(red[2][tid], red[3][tid]));
  __syncthreads();
  mx = mxs[f];
  float se = 0.0f, acc[MONO_FT];
#pragma unroll
  for (int i = 0; i < MONO_FT; ++i) acc[i] = 0.0f;
  for (int c0 = 0; c0 < M; c0 += MONO_CH) {
#pragma unroll 4
    for (int i = 0; i < MONO_CH / 16; ++i) {
      const int m = c0 + r + 16 * i;
      const float e = m < M ? expf(yc[(size_t)m * N] - mx) : 0.0f;
      pe[(r + 16 * i) * MONO_FT + f] = e;
      se += e;
    }
    __syncthreads();
    const int kend = min(MONO_CH, M - c0);
    if (d < Md)
      for (int kk = part; kk < kend; kk += 4) {
        const float w = Rt[(size_t)(c0 + kk) * Md + d];
        const float4* p4 = (const float4*)(pe + kk * MONO_FT);
#pragma unroll
        for (int q = 0; q < MONO_FT / 4; ++q) {
          const float4 p = p4[q];
          acc[4 * q] = fmaf(p.x, w, acc[4 * q]); acc[4 * q + 1] = fmaf(p.y, w, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(p.z, w, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(p.w, w, acc[4 * q + 3]);
        }
      }
    __syncthreads();
  }
  se += __shfl_xor(se, 16);
  se += __shfl_xor(se, 32);
  if ((tid & 63) < 16) red[part][f] = se;
#pragma unroll
  for (int i = 0; i < MONO_FT; ++i) pe[(part * MONO_FT + i) * 64 + (PADDED ? (d + 4 * i) & 63 : d)] = acc[i];
  __syncthreads();
  if (tid < MONO_FT) sums[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  __syncthreads();
  if (PADDED) {      // (frame f, channels r, r + 16, ..): the same expression per output, stored along the frames
    // the sums of frame i sit rotated by 4 i within their row of 64: the 64 lanes (16 frames x 4 neighbouring channels) read 64 banks
    if (g0 + f < G)
      for (int dd = r; dd < Md; dd += 16) {
        const int c = (dd + 4 * f) & 63;
        out[dst[f] + (size_t)dd * Tmax] =
            ((pe[f * 64 + c] + pe[(MONO_FT + f) * 64 + c]) + (pe[(2 * MONO_FT + f) * 64 + c] + pe[(3 * MONO_FT + f) * 64 + c])) / sums[f];
      }
    return;
  }
  for (int i = part; i < MONO_FT; i += 4) {
    const int g = g0 + i;
    if (g < G && d < Md)
      out[(size_t)g * Md + d] = ((pe[i * 64 + d] + pe[(MONO_FT + i) * 64 + d]) + (pe[(2 * MONO_FT + i) * 64 + d] + pe[(3 * MONO_FT + i) * 64 + d])) / sums[i];
  }
}

// out [B][Md][Tmax]: the columns T_b .. Tmax-1 of every channel row, which k_tdnn_mono<true> does not visit, are set to 0
__global__ void k_tdnn_zero_padding(const int* __restrict__ off, int Tmax, size_t bstride, float* __restrict__ out) {
  const int b = blockIdx.z, d = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < Tmax && t >= off[b + 1] - off[b]) out[(size_t)b * bstride + (size_t)d * Tmax + t] = 0.0f;
}

// Softmax over the M channel rows of a column, written as out [B][M][Tmax] -- the layout the encoder reads (ppg_dev, channel-major
// with the frames contiguous), which is also the layout of the logits: no transpose.  One workgroup = POST_FT consecutive frames
// of ONE utterance (blockIdx.x, blockIdx.y) x the channel rows k0 .. k0 + kper - 1 it stores (blockIdx.z).
//  - threads are (frame f = tid % 16, channel row r = tid / 16): the 16 lanes of a channel row read 16 neighbouring logits and
//    store 16 neighbouring posteriors (scalar accesses: a segment starts on a multiple of 4 columns, an output row anywhere);
//  - max and sum of exp over ALL M rows in every workgroup, whatever rows it stores (the logits of a tile are 16 x M floats out
//    of the L2; splitting the stores over blockIdx.z is what fills the CUs when a batch has a few hundred columns): per thread
//    over its rows r, r + 16, .. in order, then over the 4 rows of a wave by lane exchange, then over the 4 waves through LDS,
//    pairwise -- k_tdnn_mono's order.  No atomics; a frame's posteriors depend on its own column alone, not on B, Tmax, the
//    segment's start or kper;
//  - the value is k_tdnn_output's expf(v - max) / sum;
//  - frames T_b .. Tmax-1 of an utterance are stored as 0: every element of the M rows of out is written; utterance b's rows start
//    at out + b * bstride (bstride >= M * Tmax: the rows behind them are the caller's).
constexpr int POST_FT = 16;
__global__ __launch_bounds__(256) void k_tdnn_post_padded(const float* __restrict__ y, const int* __restrict__ off, const int* __restrict__ cs,
                                                          int M, int N, int Tmax, int kper, size_t bstride, float* __restrict__ out) {
  __shared__ float red[4][POST_FT], stat[POST_FT];
  const int tid = threadIdx.x, f = tid & 15, r = tid >> 4, wave = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * POST_FT, t = t0 + f, T = off[b + 1] - off[b];
  const int k0 = blockIdx.z * kper, k1 = min(M, k0 + kper);
  float* ob = out + (size_t)b * bstride + t;
  if (t0 >= T) {      // (uniform over the workgroup) a tile of padding
    if (t < Tmax)
      for (int k = k0 + r; k < k1; k += 16) ob[(size_t)k * Tmax] = 0.0f;
    return;
  }
  const float* yc = y + cs[b] + min(t, T - 1);      // a frame past the utterance's end repeats its last one (stored as 0)
  float mx = -INFINITY;
#pragma unroll 8
  for (int m = r; m < M; m += 16) mx = fmaxf(mx, yc[(size_t)m * N]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if ((tid & 63) < 16) red[wave][f] = mx;
  __syncthreads();
  if (tid < POST_FT) stat[tid] = fmaxf(fmaxf(red[0][tid], red[1][tid]), fmaxf(red[2][tid], red[3][tid]));
  __syncthreads();
  mx = stat[f];
  float se = 0.0f;
#pragma unroll 8
  for (int m = r; m < M; m += 16) se += expf(yc[(size_t)m * N] - mx);
  se += __shfl_xor(se, 16);
  se += __shfl_xor(se, 32);
  __syncthreads();      // (every thread has read stat[] as the max)
  if ((tid & 63) < 16) red[wave][f] = se;
  __syncthreads();
  if (tid < POST_FT) stat[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  __syncthreads();
  const float sum = stat[f];
  if (t >= Tmax) return;
  const bool valid = t < T;
#pragma unroll 4
  for (int k = k0 + r; k < k1; k += 16) ob[(size_t)k * Tmax] = valid ? expf(yc[(size_t)k * N] - mx) / sum : 0.0f;
}

struct TdnnWs { size_t x[2], splitk, splitk_bytes, total; int Tp; };
TdnnWs tdnn_ws(const facppg_tdnn* h, int T) {
  TdnnWs w;
  w.Tp = h->left + T + h->right;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.x[0] = take((size_t)h->max_dim * w.Tp * 4);
  w.x[1] = take((size_t)h->max_dim * w.Tp * 4);
  w.splitk_bytes = (size_t)16 * h->max_dim * w.Tp * 4;
  w.splitk = take(w.splitk_bytes);
  w.total = off;
  return w;
}

struct TdnnBatchWs { size_t x[2], splitk, splitk_bytes, cs, total; long N; };
TdnnBatchWs tdnn_batch_ws(const facppg_tdnn* h, const int32_t* off, int B) {
  TdnnBatchWs w;
  w.N = 0;
  for (int b = 0; b < B; ++b) w.N += round_up(h->left + h->right + off[b + 1] - off[b], 4);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) / 256 * 256; return r; };
  w.x[0] = take((size_t)h->max_dim * w.N * 4);
  w.x[1] = take((size_t)h->max_dim * w.N * 4);
  size_t parts = 0;      // the largest layer's partial sums (the single form's 16 * max_dim bound costs GBs at a corpus's N)
  for (const facppg_tdnn_layer& l : h->layers) {
    const int sk = gemm_split_k(l.in_dim * l.taps);
    if (sk > 1 && (size_t)sk * l.out_dim > parts) parts = (size_t)sk * l.out_dim;
  }
  w.splitk_bytes = parts * w.N * 4;
  w.splitk = take(w.splitk_bytes);
  w.cs = take((size_t)(B + 1) * 4);
  w.total = o;
  return w;
}

// the layers of the batch form up to the last layer's output [out_dim][N]; *y_out = that buffer
int tdnn_batch_layers(facppg_tdnn* h, const float* feats_dev, const int32_t* off_dev, const int32_t* off_host, int B, void* ws_,
                      size_t ws_bytes, hipStream_t s, const float** y_out, const int** cs_out, int* N_out) {
  FACPPG_REQUIRE(h && feats_dev && off_dev && ws_, FACPPG_EINVAL, "NULL argument");
  const TdnnBatchWs w = tdnn_batch_ws(h, off_host, B);
  FACPPG_REQUIRE(w.N * (long)h->max_dim < (1l << 31), FACPPG_EUNSUPPORTED, "batch of %ld columns x %d channels exceeds 2^31 elements: split it", w.N,
                 h->max_dim);
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w.total);
  char* ws = (char*)ws_;
  float* x[2] = {(float*)(ws + w.x[0]), (float*)(ws + w.x[1])};
  int* cs = (int*)(ws + w.cs);
  const int N = (int)w.N;
  k_tdnn_colstart<<<(B + 256) / 256, 256, 0, s>>>(off_dev, B, h->left + h->right, cs);
  k_tdnn_input_batch<<<dim3((N + 255) / 256, h->in_dim), 256, 0, s>>>(feats_dev, off_dev, cs, B, x[0], h->in_dim, h->left, N);
  int cur = 0;
  for (int i = 0; i < h->n_layers; ++i) {
    const facppg_tdnn_layer& l = h->layers[i];
    GemmArgs g;
    g.A = h->A[i]; g.M = l.out_dim; g.Cin = l.in_dim; g.taps = l.taps; g.dil = l.dil; g.pad = 0;
    g.X = x[cur]; g.ldx = N; g.N = N; g.bias = h->bias[i]; g.act = l.relu ? ACT_RELU : ACT_NONE;
    g.C = x[cur ^ 1]; g.ldc = N; g.B = 1;
    g.splitk_ws = (float*)(ws + w.splitk); g.splitk_ws_bytes = w.splitk_bytes;
    const int rc = gemm_launch(g, s);
    if (rc != FACPPG_OK) return rc;
    cur ^= 1;
    if (l.renorm_target_rms > 0.0f) k_tdnn_renorm<<<(N + 255) / 256, 256, 0, s>>>(x[cur], l.out_dim, N, l.renorm_target_rms);
  }
  *y_out = x[cur]; *cs_out = cs; *N_out = N;
  return FACPPG_OK;
}

}  // namespace

extern "C" size_t facppg_tdnn_weight_count(const facppg_tdnn_layer* layers, int n_layers) {
  if (!layers || n_layers <= 0) return 0;
  size_t n = 0;
  for (int i = 0; i < n_layers; ++i) {
    const facppg_tdnn_layer& l = layers[i];
    if (l.out_dim <= 0 || l.in_dim <= 0 || l.taps <= 0 || l.dil <= 0) return 0;
    n += (size_t)l.out_dim * l.taps * l.in_dim + l.out_dim;
  }
  return n;
}

extern "C" int facppg_tdnn_create(const facppg_tdnn_layer* layers, int n_layers, int final_op, const float* weights_dev,
                                  size_t n_weights, int device, void* stream_, facppg_tdnn** out) {
  FACPPG_REQUIRE(layers && weights_dev && out && n_layers > 0, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(final_op >= 0 && final_op <= 2, FACPPG_EINVAL, "final_op must be 0 (none), 1 (softmax) or 2 (log-softmax)");
  FACPPG_REQUIRE(n_weights == facppg_tdnn_weight_count(layers, n_layers) && n_weights > 0, FACPPG_EINVAL,
                 "weight blob has %zu values, the layer table needs %zu", n_weights, facppg_tdnn_weight_count(layers, n_layers));
  hipStream_t s = (hipStream_t)stream_;
  facppg_tdnn* h = new (std::nothrow) facppg_tdnn;
  FACPPG_REQUIRE(h, FACPPG_EHIP, "out of host memory");
  h->device = device; h->n_layers = n_layers; h->final_op = final_op;
  if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cu < 1) h->n_cu = 256;
  h->layers.assign(layers, layers + n_layers);
  h->in_dim = layers[0].in_dim; h->out_dim = layers[n_layers - 1].out_dim; h->max_dim = h->in_dim;
  size_t a_f4 = 0, b_f = 0;
  for (int i = 0; i < n_layers; ++i) {
    const facppg_tdnn_layer& l = layers[i];
    if (i > 0 && l.in_dim != layers[i - 1].out_dim) {
      set_error("layer %d reads %d channels, layer %d writes %d", i, l.in_dim, i - 1, layers[i - 1].out_dim);
      delete h;
      return FACPPG_EINVAL;
    }
    // context of the chain: frame t of layer i needs frames t + first .. t + first + (taps-1) dil of layer i-1
    h->left += l.first < 0 ? -l.first : 0;
    const int hi = l.first + (l.taps - 1) * l.dil;
    h->right += hi > 0 ? hi : 0;
    if (l.first > 0 || hi < 0) {
      set_error("layer %d: a splice that excludes the current frame's side (first %d, last %d) is not supported", i, l.first, hi);
      delete h;
      return FACPPG_EUNSUPPORTED;
    }
    h->max_dim = l.out_dim > h->max_dim ? l.out_dim : h->max_dim;
    a_f4 += packed_a_float4s(l.out_dim, l.in_dim * l.taps);
    b_f += (size_t)round_up(l.out_dim, 64);
  }
  if (hipMalloc(&h->arena, a_f4 * 16 + b_f * 4) != hipSuccess) {
    set_error("hipMalloc of %zu bytes of packed TDNN weights failed", a_f4 * 16 + b_f * 4);
    delete h;
    return FACPPG_EHIP;
  }
  float4* ap = (float4*)h->arena;
  float* bp = (float*)(ap + a_f4);
  const float* src = weights_dev;
  for (int i = 0; i < n_layers; ++i) {
    const facppg_tdnn_layer& l = layers[i];
    const int K = l.taps * l.in_dim;
    // blob layout per layer: W [out][taps * in] (tap-major: Kaldi's Append order), then b [out]
    const int rc = pack_a_strided(src, l.out_dim, l.in_dim, l.taps, K, 1, l.in_dim, 0, ap, s);
    if (rc != FACPPG_OK || hipMemcpyAsync(bp, src + (size_t)l.out_dim * K, (size_t)l.out_dim * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      if (rc == FACPPG_OK) set_error("copy of the layer-%d bias failed", i);
      (void)hipFree(h->arena);
      delete h;
      return FACPPG_EHIP;
    }
    h->A.push_back(ap);
    h->bias.push_back(bp);
    ap += packed_a_float4s(l.out_dim, K);
    bp += round_up(l.out_dim, 64);
    src += (size_t)l.out_dim * K + l.out_dim;
  }
  if (hipStreamSynchronize(s) != hipSuccess) {   // the caller may free weights_dev when this returns
    set_error("packing the TDNN weights failed");
    (void)hipFree(h->arena);
    delete h;
    return FACPPG_EHIP;
  }
  *out = h;
  return FACPPG_OK;
}

extern "C" void facppg_tdnn_destroy(facppg_tdnn* h) {
  if (!h) return;
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

extern "C" int facppg_tdnn_context(const facppg_tdnn* h, int* left, int* right) {
  FACPPG_REQUIRE(h && left && right, FACPPG_EINVAL, "NULL argument");
  *left = h->left; *right = h->right;
  return FACPPG_OK;
}

extern "C" size_t facppg_tdnn_workspace_bytes(const facppg_tdnn* h, int T) {
  if (!h || T <= 0) return 0;
  return tdnn_ws(h, T).total;
}

extern "C" int facppg_tdnn_forward(facppg_tdnn* h, const float* feats_dev, int T, float* out_dev, void* ws_, size_t ws_bytes,
                                   void* stream_) {
  FACPPG_REQUIRE(h && feats_dev && out_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0, FACPPG_EINVAL, "T must be positive (got %d)", T);
  const TdnnWs w = tdnn_ws(h, T);
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  float* x[2] = {(float*)(ws + w.x[0]), (float*)(ws + w.x[1])};
  const int Tp = w.Tp;
  k_tdnn_input<<<dim3((Tp + 255) / 256, h->in_dim), 256, 0, s>>>(feats_dev, x[0], T, h->in_dim, h->left, Tp);
  int cur = 0;
  for (int i = 0; i < h->n_layers; ++i) {
    const facppg_tdnn_layer& l = h->layers[i];
    GemmArgs g;
    g.A = h->A[i]; g.M = l.out_dim; g.Cin = l.in_dim; g.taps = l.taps; g.dil = l.dil; g.pad = 0;
    g.X = x[cur]; g.ldx = Tp; g.N = Tp; g.bias = h->bias[i]; g.act = l.relu ? ACT_RELU : ACT_NONE;
    g.C = x[cur ^ 1]; g.ldc = Tp; g.B = 1;
    g.splitk_ws = (float*)(ws + w.splitk); g.splitk_ws_bytes = w.splitk_bytes;
    const int rc = gemm_launch(g, s);
    if (rc != FACPPG_OK) return rc;
    cur ^= 1;
    if (l.renorm_target_rms > 0.0f) k_tdnn_renorm<<<(Tp + 255) / 256, 256, 0, s>>>(x[cur], l.out_dim, Tp, l.renorm_target_rms);
  }
  k_tdnn_output<<<(T + 63) / 64, 64, 0, s>>>(x[cur], h->out_dim, Tp, T, h->final_op, out_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" size_t facppg_tdnn_batch_workspace_bytes(const facppg_tdnn* h, const int32_t* offsets_host, int B) {
  if (!h || check_offsets(offsets_host, B, "facppg_tdnn_batch_workspace_bytes")) return 0;
  return tdnn_batch_ws(h, offsets_host, B).total;
}

extern "C" int facppg_tdnn_forward_batch(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev, const int32_t* offsets_host,
                                         int B, float* out_dev, void* ws_, size_t ws_bytes, void* stream_) {
  if (int rc = check_offsets(offsets_host, B, "facppg_tdnn_forward_batch")) return rc;
  FACPPG_REQUIRE(out_dev, FACPPG_EINVAL, "NULL argument");
  hipStream_t s = (hipStream_t)stream_;
  const float* y; const int* cs; int N;
  if (int rc = tdnn_batch_layers(h, feats_dev, offsets_dev, offsets_host, B, ws_, ws_bytes, s, &y, &cs, &N)) return rc;
  k_tdnn_output_batch<<<(offsets_host[B] + 63) / 64, 64, 0, s>>>(y, offsets_dev, cs, B, h->out_dim, N, h->final_op, out_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_tdnn_forward_batch_reduced(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                                                 const int32_t* offsets_host, int B, const float* transform_t_dev, int M, float* out_dev,
                                                 void* ws_, size_t ws_bytes, void* stream_) {
  if (int rc = check_offsets(offsets_host, B, "facppg_tdnn_forward_batch_reduced")) return rc;
  FACPPG_REQUIRE(h && out_dev && transform_t_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(M > 0 && M <= 64, FACPPG_EINVAL, "bad M (1 <= M <= 64, got %d)", M);
  FACPPG_REQUIRE(h->final_op == 1, FACPPG_EUNSUPPORTED, "the fused reduction needs a model whose output is a softmax (final_op 1, got %d)",
                 h->final_op);
  hipStream_t s = (hipStream_t)stream_;
  const float* y; const int* cs; int N;
  if (int rc = tdnn_batch_layers(h, feats_dev, offsets_dev, offsets_host, B, ws_, ws_bytes, s, &y, &cs, &N)) return rc;
  k_tdnn_mono<false><<<(offsets_host[B] + MONO_FT - 1) / MONO_FT, 256, 0, s>>>(y, offsets_dev, cs, B, h->out_dim, N, transform_t_dev, M, out_dev, 0, 0);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_tdnn_forward_batch_padded_strided(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                                                        const int32_t* offsets_host, int B, const float* transform_t_dev, int M, int Tmax,
                                                        size_t batch_stride, float* out_dev, void* ws_, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(B >= 1, FACPPG_EINVAL, "facppg_tdnn_forward_batch_padded: B must be at least 1 (got %d)", B);
  if (int rc = check_offsets(offsets_host, B, "facppg_tdnn_forward_batch_padded")) return rc;
  FACPPG_REQUIRE(h && feats_dev && offsets_dev && out_dev && ws_, FACPPG_EINVAL, "facppg_tdnn_forward_batch_padded: NULL argument");
  FACPPG_REQUIRE(!transform_t_dev || (M > 0 && M <= 64), FACPPG_EINVAL, "facppg_tdnn_forward_batch_padded: bad M (1 <= M <= 64, got %d)", M);
  FACPPG_REQUIRE(h->final_op == 1, FACPPG_EUNSUPPORTED,
                 "facppg_tdnn_forward_batch_padded: the padded layout holds posteriors: the model's output must be a softmax (final_op 1, got %d)",
                 h->final_op);
  int Tlong = 0, Tshort = Tmax;
  for (int b = 0; b < B; ++b) {
    const int T = offsets_host[b + 1] - offsets_host[b];
    Tlong = T > Tlong ? T : Tlong;
    Tshort = T < Tshort ? T : Tshort;
  }
  FACPPG_REQUIRE(Tmax >= Tlong, FACPPG_EINVAL, "facppg_tdnn_forward_batch_padded: Tmax %d is shorter than the longest utterance (%d frames)", Tmax,
                 Tlong);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EUNSUPPORTED, "facppg_tdnn_forward_batch_padded: at most 65535 utterances per call (got %d)", B);
  const size_t rows = transform_t_dev ? (size_t)M : (size_t)h->out_dim;
  FACPPG_REQUIRE(batch_stride >= rows * (size_t)Tmax, FACPPG_EINVAL,
                 "facppg_tdnn_forward_batch_padded: a batch stride of %zu floats is shorter than the %zu x %d posteriors of one utterance", batch_stride,
                 rows, Tmax);
  hipStream_t s = (hipStream_t)stream_;
  const float* y; const int* cs; int N;
  if (int rc = tdnn_batch_layers(h, feats_dev, offsets_dev, offsets_host, B, ws_, ws_bytes, s, &y, &cs, &N)) return rc;
  if (transform_t_dev) {
    // k_tdnn_mono walks the valid frames only: the padding, where a batch has any, is zeroed next to it
    if (Tshort < Tmax) k_tdnn_zero_padding<<<dim3((Tmax + 255) / 256, M, B), 256, 0, s>>>(offsets_dev, Tmax, batch_stride, out_dev);
    k_tdnn_mono<true><<<(offsets_host[B] + MONO_FT - 1) / MONO_FT, 256, 0, s>>>(y, offsets_dev, cs, B, h->out_dim, N, transform_t_dev, M, out_dev, Tmax,
                                                                                batch_stride);
  } else {
    // channel rows per workgroup: whole tiles of 16 rows, split until the launch has about two workgroups per CU (at most 16 ways:
    // every split repeats the tile's max / sum passes; the values do not depend on the split)
    const int tiles = (Tmax + POST_FT - 1) / POST_FT;
    long want = 2l * h->n_cu / ((long)tiles * B);
    const int split = (int)(want < 1 ? 1 : want > 16 ? 16 : want);
    const int kper = round_up((h->out_dim + split - 1) / split, 16);
    k_tdnn_post_padded<<<dim3(tiles, B, (h->out_dim + kper - 1) / kper), 256, 0, s>>>(y, offsets_dev, cs, h->out_dim, N, Tmax, kper, batch_stride,
                                                                                      out_dev);
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_tdnn_forward_batch_padded(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                                                const int32_t* offsets_host, int B, const float* transform_t_dev, int M, int Tmax,
                                                float* out_dev, void* ws_, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(h, FACPPG_EINVAL, "facppg_tdnn_forward_batch_padded: NULL argument");
  const size_t rows = transform_t_dev ? (size_t)(M > 0 ? M : 0) : (size_t)h->out_dim;
  return facppg_tdnn_forward_batch_padded_strided(h, feats_dev, offsets_dev, offsets_host, B, transform_t_dev, M, Tmax,
                                                  rows * (size_t)(Tmax > 0 ? Tmax : 0), out_dev, ws_, ws_bytes, stream_);
}
