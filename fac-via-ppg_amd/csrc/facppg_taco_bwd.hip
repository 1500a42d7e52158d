// Backward pass of the teacher-forced Tacotron2.forward on gfx950: the recurrences.
//
// What is sequential in the backward pass of Decoder.forward (model.py:444-487) and of the encoder's BiLSTM
// (model.py:226-233) runs here; everything else -- every weight gradient, the prenets, the projection, the postnet, the
// encoder's convolutions -- is a dense product over all frames on the adjoints these kernels leave (common/taco_grad.py).
//
//   k_lstm_cell_scan     gate pre-activations of all frames (a GEMM on the saved hidden states) -> gate activations and cell
//                        states of all frames: what the forward pass did not keep
//   k_lstm_bwd_step      one frame of an LSTM's backward chain: dh(t) = seed(t) + W_hh^T dgates(t+1), the cell's pointwise
//                        backward -> dgates(t).  The decoder LSTM (its chain needs nothing of the attention's, so it runs
//                        first, model.py:427-428) and both directions of the encoder's BiLSTM
//   k_att_rec_step       [dctx(t) | dah(t)] = base(t) + [W_ih[:, P:] | W_hh]^T dgates_A(t+1)   (model.py:400-402)
//   k_att_bwd_step       one frame of the attention chain (model.py:408-424, 92-121): dw -> softmax backward -> dS = de v
//                        (1 - tanh^2) -> location layer transposed (dense, conv) -> the adjoints of frame t-1's weights and
//                        cumulative weights; query layer transposed -> dah(t); attention LSTMCell backward -> dgates_A(t)
//
// One launch per frame and kernel, in stream order: frame t reads what frame t+1's launch wrote, so there is no exchange
// between workgroups inside a launch and nothing to wait for.  Every sum has a fixed order (no atomics): two runs give the
// same bits.  Transposed products read W[k][j] with j across lanes, 16 columns x 64 K-parts per workgroup.
#include "facppg_common.h"

using namespace facppg;

namespace {

constexpr int NTB = 1024, JT = 16, KPARTS = NTB / JT;

__device__ __forceinline__ float sigm_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// sum_k W[k][j0 + j] x[k] for the workgroup's JT columns: thread (j = tid % JT, part = tid / JT) takes every KPARTS-th k;
// the column sums are returned to threads tid < JT (red: NTB floats of LDS; contains a barrier)
__device__ __forceinline__ float tmatvec16(const float* __restrict__ W, int ld, int K, int j0, int ncols, const float* xs, float* red,
                                           int tid) {
  const int j = tid % JT, kp = tid / JT;
  float acc = 0.0f;
  if (j0 + j < ncols) {
    const float* wp = W + j0 + j;
#pragma unroll 8
    for (int k = kp; k < K; k += KPARTS) acc = fmaf(wp[(size_t)k * ld], xs[k], acc);
  }
  red[tid] = acc;
  __syncthreads();
  float s = 0.0f;
  if (tid < JT)
    for (int q = 0; q < KPARTS; ++q) s += red[q * JT + tid];
  return s;
}

// LSTMCell pointwise backward of one unit (gate order i, f, g, o; activations, not pre-activations):
// dh, the carried dc(t+1) f(t+1) -> the four pre-activation gradients, and the carry for frame t-1
__device__ __forceinline__ float cell_backward(const float* __restrict__ act, const float* __restrict__ c, float* __restrict__ dg,
                                               int H, int T, int t, size_t row /* n * T + t */, int j, float dh, float dc_next) {
  const float* a = act + row * 4 * H;
  const float gi = a[j], gf = a[H + j], gg = a[2 * H + j], go = a[3 * H + j];
  const float ct = c[row * H + j], cp = t > 0 ? c[(row - 1) * H + j] : 0.0f;
  const float tc = tanhf(ct);
  const float dc = dc_next + dh * go * (1.0f - tc * tc);
  float* d = dg + row * 4 * H;
  d[j] = dc * gg * gi * (1.0f - gi);
  d[H + j] = dc * cp * gf * (1.0f - gf);
  d[2 * H + j] = dc * gi * (1.0f - gg * gg);
  d[3 * H + j] = dh * tc * go * (1.0f - go);
  return dc * gf;
}

// gates [N][T][4H]: pre-activations in, activations out; c [N][T][H].  Frames at or beyond an utterance's length: zeros.
__global__ void k_lstm_cell_scan(float* __restrict__ gates, float* __restrict__ c, const int32_t* __restrict__ lengths, int N, int T,
                                 int H) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * H) return;
  const int n = i / H, j = i % H;
  const int len = lengths ? min(max(lengths[n], 0), T) : T;
  float cs = 0.0f;
  for (int t = 0; t < T; ++t) {
    float* g = gates + ((size_t)n * T + t) * 4 * H;
    float gi = 0.0f, gf = 0.0f, gg = 0.0f, go = 0.0f;
    if (t < len) {
      gi = sigm_exact(g[j]); gf = sigm_exact(g[H + j]); gg = tanhf(g[2 * H + j]); go = sigm_exact(g[3 * H + j]);
      cs = gf * cs + gi * gg;
    }
    g[j] = gi; g[H + j] = gf; g[2 * H + j] = gg; g[3 * H + j] = go;
    c[((size_t)n * T + t) * H + j] = t < len ? cs : 0.0f;
  }
}

__global__ __launch_bounds__(NTB) void k_lstm_bwd_step(const float* __restrict__ w_hh /*[4H][H]*/, const float* __restrict__ act,
                                                       const float* __restrict__ c, const float* __restrict__ seed /*[N][T][H]*/,
                                                       const int32_t* __restrict__ lengths, float* __restrict__ dg /*[N][T][4H]*/,
                                                       float* __restrict__ carry /*[N][H]*/, int T, int H, int t) {
  extern __shared__ float xs[];   // dgates(t+1): 4H
  __shared__ float red[NTB];
  const int n = blockIdx.y, j0 = blockIdx.x * JT, tid = threadIdx.x, j = j0 + tid;
  const int len = lengths ? min(max(lengths[n], 0), T) : T;
  const size_t row = (size_t)n * T + t;
  const bool mine = tid < JT && j < H;
  if (t >= len) {   // (uniform per workgroup)
    if (mine) {
      for (int g = 0; g < 4; ++g) dg[row * 4 * H + g * H + j] = 0.0f;
      carry[(size_t)n * H + j] = 0.0f;
    }
    return;
  }
  const bool has_next = t + 1 < len;
  float rec = 0.0f;
  if (has_next) {
    const float* nx = dg + (row + 1) * 4 * H;
    for (int k = tid; k < 4 * H; k += NTB) xs[k] = nx[k];
    __syncthreads();
    rec = tmatvec16(w_hh, H, 4 * H, j0, H, xs, red, tid);
  }
  if (mine) {
    const float dcn = has_next ? carry[(size_t)n * H + j] : 0.0f;
    carry[(size_t)n * H + j] = cell_backward(act, c, dg, H, T, t, row, j, seed[row * H + j] + rec, dcn);
  }
}

struct AttBwd {
  facppg_taco_attention_backward_args a;
  float *dctx, *dah, *dw, *gprev, *gcum, *dfeat, *dc, *cpart;   // scratch: [B][E], [B][A], [B][Tin] x 3, [B][NFIL][Tin], [B][A], [B][CQ][2][Tin]
  int B, T, Tin, E, A, AD, NFIL, KSZ;
};

__global__ __launch_bounds__(NTB) void k_att_rec_step(AttBwd p, int t) {
  extern __shared__ float xs[];   // dgates_A(t+1): 4A
  __shared__ float red[NTB];
  const int b = blockIdx.y, j0 = blockIdx.x * JT, tid = threadIdx.x, j = j0 + tid, W = p.E + p.A;
  const size_t row = (size_t)b * p.T + t;
  float rec = 0.0f;
  if (t + 1 < p.T) {
    const float* nx = p.a.dgates_a + (row + 1) * 4 * p.A;
    for (int k = tid; k < 4 * p.A; k += NTB) xs[k] = nx[k];
    __syncthreads();
    rec = tmatvec16(p.a.w_cat, W, 4 * p.A, j0, W, xs, red, tid);
  }
  if (tid < JT && j < W) {
    if (j < p.E) {
      const float v = p.a.base_ctx[row * p.E + j] + rec;
      p.dctx[(size_t)b * p.E + j] = v;
      p.a.dctx[row * p.E + j] = v;
    } else {
      p.dah[(size_t)b * p.A + j - p.E] = p.a.base_ah[row * p.A + j - p.E] + rec;
    }
  }
}

constexpr int CQ = 8;   // the transposed location convolution sums its filters in CQ parts (then over the parts, in order)

__global__ __launch_bounds__(NTB) void k_att_bwd_step(AttBwd p, int t) {
  extern __shared__ float s_dq[];   // AD
  __shared__ float red[NTB];
  __shared__ int s_lo, s_hi;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tin = p.Tin, E = p.E, A = p.A, AD = p.AD, NFIL = p.NFIL, KSZ = p.KSZ;
  const size_t row = (size_t)b * p.T + t;
  const float* mem = p.a.memory + (size_t)b * Tin * E;
  const float* w = p.a.align + row * Tin;
  const float* dctx = p.dctx + (size_t)b * E;
  float* dw = p.dw + (size_t)b * Tin;
  float* gprev = p.gprev + (size_t)b * Tin;
  float* gcum = p.gcum + (size_t)b * Tin;
  float* dfeat = p.dfeat + (size_t)b * Tin * NFIL;   // [NFIL][Tin]
  float* cpart = p.cpart + (size_t)b * CQ * 2 * Tin;
  float* dS = p.a.ds + row * Tin * AD;
  // The stretch [lo, hi] of positions with non-zero weight (the attention window and the length mask, whatever rule made
  // them): everything below is zero outside it, and the caller zeroed dS.
  if (tid == 0) { s_lo = Tin; s_hi = -1; }
  __syncthreads();
  {
    int l = Tin, h = -1;
    for (int j = tid; j < Tin; j += NTB)
      if (w[j] != 0.0f) { l = min(l, j); h = max(h, j); }
    if (h >= 0) { atomicMin(&s_lo, l); atomicMax(&s_hi, h); }
  }
  __syncthreads();
  const int hi = s_hi, lo = hi < 0 ? 0 : s_lo, nw = hi - lo + 1;
  // dw(t)[j] = memory[j] . dctx(t) + dcum(t)[j] + (frame t+1's previous-weights input)[j]
  for (int j = lo + wave; j <= hi; j += NTB / 64) {
    float a = 0.0f;
    for (int e = lane; e < E; e += 64) a = fmaf(mem[(size_t)j * E + e], dctx[e], a);
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) dw[j] = a + gcum[j] + gprev[j];
  }
  __syncthreads();
  // softmax backward (masked positions carry weight 0, so gradient 0): de[j] = w[j] (dw[j] - sum_i w[i] dw[i])
  {
    float a = 0.0f;
    for (int j = lo + tid; j <= hi; j += NTB) a = fmaf(w[j], dw[j], a);
    red[tid] = a;
    __syncthreads();
    for (int o = NTB / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const float dot = red[0];
    __syncthreads();
    for (int j = tid; j < Tin; j += NTB) {
      const float de = j >= lo && j <= hi ? w[j] * (dw[j] - dot) : 0.0f;
      dw[j] = de;
      p.a.de[row * Tin + j] = de;
    }
  }
  __syncthreads();
  // dS[j][a] = de[j] v[a] (1 - tanh^2)
  {
    const float* th = p.a.tanh_s + row * Tin * AD;
    for (int i = lo * AD + tid; i < (hi + 1) * AD; i += NTB) {
      const float x = th[i];
      dS[i] = dw[i / AD] * p.a.v[i % AD] * (1.0f - x * x);
    }
  }
  __syncthreads();
  for (int a = tid; a < AD; a += NTB) {
    float s = 0.0f;
#pragma unroll 8
    for (int j = lo; j <= hi; ++j) s += dS[(size_t)j * AD + a];
    s_dq[a] = s;
  }
  if (t > 0) {   // frame 0's location input is the zero initial state
    // location_dense transposed: dfeat[f][j] = sum_a Wd[a][f] dS[j][a]
    for (int i = tid; i < nw * NFIL; i += NTB) {
      const int j = lo + i / NFIL, f = i % NFIL;
      float s = 0.0f;
#pragma unroll 8
      for (int a = 0; a < AD; ++a) s = fmaf(p.a.w_loc_dense[a * NFIL + f], dS[(size_t)j * AD + a], s);
      dfeat[(size_t)f * Tin + j] = s;
    }
    __syncthreads();
    // location_conv transposed: d in[c][i] = sum_f sum_k Wc[f][c][k] dfeat[f][i - k + pad], non-zero for i within pad of the
    // stretch; c = 0 previous weights, 1 cumulative weights.  Filters in CQ parts, then the parts in order.
    const int pad = (KSZ - 1) / 2, i_lo = max(0, lo - pad), i_hi = min(Tin - 1, hi + pad), ni = hi < 0 ? 0 : i_hi - i_lo + 1;
    const int fq = (NFIL + CQ - 1) / CQ;
    for (int it = tid; it < CQ * 2 * ni; it += NTB) {
      const int q = it / (2 * ni), c = it % (2 * ni) / ni, i = i_lo + it % ni;
      const int k0 = max(0, i + pad - hi), k1 = min(KSZ - 1, i + pad - lo);
      float s = 0.0f;
      for (int f = q * fq; f < min(NFIL, (q + 1) * fq); ++f) {
        const float* wc = p.a.w_loc_conv + ((size_t)f * 2 + c) * KSZ;
        const float* df = dfeat + (size_t)f * Tin + i + pad;
#pragma unroll 8
        for (int k = k0; k <= k1; ++k) s = fmaf(wc[k], df[-k], s);
      }
      cpart[(size_t)(q * 2 + c) * Tin + i] = s;
    }
    __syncthreads();
    for (int i2 = tid; i2 < 2 * Tin; i2 += NTB) {
      const int c = i2 / Tin, i = i2 % Tin;
      float s = 0.0f;
      if (ni > 0 && i >= i_lo && i <= i_hi)
        for (int q = 0; q < CQ; ++q) s += cpart[(size_t)(q * 2 + c) * Tin + i];
      if (c == 0) gprev[i] = s;
      else gcum[i] += s;
    }
  }
  __syncthreads();
  // query layer transposed + the attention LSTMCell's pointwise backward
  for (int i = tid; i < A; i += NTB) {
    float dh = p.dah[(size_t)b * A + i];
#pragma unroll 8
    for (int a = 0; a < AD; ++a) dh = fmaf(p.a.w_query[(size_t)a * A + i], s_dq[a], dh);
    const float dcn = t + 1 < p.T ? p.dc[(size_t)b * A + i] : 0.0f;
    p.dc[(size_t)b * A + i] = cell_backward(p.a.act_a, p.a.c_a, p.a.dgates_a, A, p.T, t, row, i, dh, dcn);
  }
}

struct AttWs { size_t dctx, dah, dw, gprev, gcum, dfeat, dc, cpart, total; };
AttWs att_ws(const facppg_taco_config& c, int B, int Tin) {
  AttWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.dctx = take((size_t)B * c.encoder_embedding_dim * 4);
  w.dah = take((size_t)B * c.attention_rnn_dim * 4);
  w.dw = take((size_t)B * Tin * 4);
  w.gprev = take((size_t)B * Tin * 4);
  w.gcum = take((size_t)B * Tin * 4);
  w.dfeat = take((size_t)B * Tin * c.attention_location_n_filters * 4);
  w.dc = take((size_t)B * c.attention_rnn_dim * 4);
  w.cpart = take((size_t)B * CQ * 2 * Tin * 4);
  w.total = off;
  return w;
}

bool dims_ok(const facppg_taco_config* c) {
  return c && c->encoder_embedding_dim > 0 && c->attention_rnn_dim > 0 && c->attention_dim > 0 && c->attention_location_n_filters > 0 &&
         c->attention_location_kernel_size > 0 && (c->attention_location_kernel_size & 1);
}

}  // namespace

extern "C" int facppg_lstm_cell_scan(float* gates_dev, float* c_dev, const int32_t* lengths_dev, int N, int T, int H, void* stream_) {
  FACPPG_REQUIRE(gates_dev && c_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(N > 0 && T > 0 && H > 0 && (long)N * H < (1l << 30), FACPPG_EINVAL, "bad N/T/H");
  k_lstm_cell_scan<<<(unsigned)(((long)N * H + 255) / 256), 256, 0, (hipStream_t)stream_>>>(gates_dev, c_dev, lengths_dev, N, T, H);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" size_t facppg_lstm_backward_workspace_bytes(int N, int H) {
  if (N <= 0 || H <= 0) return 0;
  return (size_t)N * H * 4;
}

extern "C" int facppg_lstm_backward(const float* w_hh_dev, const float* act_dev, const float* c_dev, const float* dh_seed_dev,
                                    const int32_t* lengths_dev, int N, int T, int H, float* dgates_dev, void* ws_, size_t ws_bytes,
                                    void* stream_) {
  FACPPG_REQUIRE(w_hh_dev && act_dev && c_dev && dh_seed_dev && dgates_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(N > 0 && N <= 65535 && T > 0 && H > 0, FACPPG_EINVAL, "bad N/T/H");
  FACPPG_REQUIRE(4 * H <= 8192, FACPPG_EUNSUPPORTED, "LSTM width %d: 4H floats must fit 32 KiB of LDS", H);
  FACPPG_REQUIRE(ws_bytes >= facppg_lstm_backward_workspace_bytes(N, H), FACPPG_EWORKSPACE, "LSTM backward workspace has %zu bytes, need %zu",
                 ws_bytes, facppg_lstm_backward_workspace_bytes(N, H));
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((unsigned)((H + JT - 1) / JT), (unsigned)N);
  for (int t = T - 1; t >= 0; --t)
    k_lstm_bwd_step<<<grid, NTB, (size_t)4 * H * 4, s>>>(w_hh_dev, act_dev, c_dev, dh_seed_dev, lengths_dev, dgates_dev, (float*)ws_, T, H, t);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" size_t facppg_taco_attention_backward_workspace_bytes(const facppg_taco_config* c, int B, int Tin) {
  if (!dims_ok(c) || B <= 0 || Tin <= 0) return 0;
  return att_ws(*c, B, Tin).total;
}

extern "C" int facppg_taco_attention_backward(const facppg_taco_config* c, const facppg_taco_attention_backward_args* a, int B, int Tin,
                                              int T_out, void* ws_, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(c && a && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(dims_ok(c), FACPPG_EINVAL, "bad configuration");
  FACPPG_REQUIRE(a->w_cat && a->w_query && a->v && a->w_loc_dense && a->w_loc_conv && a->memory && a->align && a->tanh_s && a->act_a &&
                     a->c_a && a->base_ctx && a->base_ah && a->dgates_a && a->dctx && a->ds && a->de,
                 FACPPG_EINVAL, "NULL pointer in the arguments");
  FACPPG_REQUIRE(B > 0 && B <= 65535 && Tin > 0 && T_out > 0, FACPPG_EINVAL, "bad B/Tin/T_out");
  FACPPG_REQUIRE(4 * c->attention_rnn_dim <= 8192 && c->attention_dim <= 8192, FACPPG_EUNSUPPORTED,
                 "attention LSTM width %d / attention_dim %d exceed the kernels' LDS stretch", c->attention_rnn_dim, c->attention_dim);
  const AttWs w = att_ws(*c, B, Tin);
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "attention backward workspace has %zu bytes, need %zu", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  FACPPG_HIP_CHECK(hipMemsetAsync(ws, 0, w.total, s));   // the adjoints carried into frame T - 1 are zero
  // (a frame writes dS on its stretch of non-zero weights only)
  FACPPG_HIP_CHECK(hipMemsetAsync(a->ds, 0, (size_t)B * T_out * Tin * c->attention_dim * 4, s));
  AttBwd p;
  p.a = *a;
  p.dctx = (float*)(ws + w.dctx); p.dah = (float*)(ws + w.dah); p.dw = (float*)(ws + w.dw); p.gprev = (float*)(ws + w.gprev);
  p.gcum = (float*)(ws + w.gcum); p.dfeat = (float*)(ws + w.dfeat); p.dc = (float*)(ws + w.dc); p.cpart = (float*)(ws + w.cpart);
  p.B = B; p.T = T_out; p.Tin = Tin; p.E = c->encoder_embedding_dim; p.A = c->attention_rnn_dim; p.AD = c->attention_dim;
  p.NFIL = c->attention_location_n_filters; p.KSZ = c->attention_location_kernel_size;
  const dim3 grid_rec((unsigned)((p.E + p.A + JT - 1) / JT), (unsigned)B);
  for (int t = T_out - 1; t >= 0; --t) {
    k_att_rec_step<<<grid_rec, NTB, (size_t)4 * p.A * 4, s>>>(p, t);
    k_att_bwd_step<<<B, NTB, (size_t)p.AD * 4, s>>>(p, t);
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
