// WaveGlow.infer for MI355X (gfx950): hand-written HIP kernels + their C ABI.
//
// Replaces the reference's src/waveglow/glow.py:252-293 (WaveGlow.infer) and everything it
// calls: WN.forward (:154-175), fused_add_tanh_sigmoid_multiply (:33-40),
// Invertible1x1Conv reverse (:88-97), the upsample ConvTranspose1d + regroup (:253-259).
//
// Two data layouts, both fp32 and channel-major with the time axis contiguous (a tile row of one
// channel is one 256-byte segment: coalesced global loads, conflict-free LDS image [k][64]):
//
// * inference (facppg_wg_infer): PHASE-MAJOR.  P = hop/8 group positions per mel frame; position
//   l = P*q + ph is stored at [ph][q], because the upsampler is folded into the conditioning convs and
//   the folded weights differ per phase (see k_wn_layer<PM>):
//     h0,h1 [B][256][P][16 + Tr + 16]  WN hidden state, ping-pong per layer; the zero margins of every
//                                      phase row ARE the dilated convolution's zero padding
//     skip  [B][256][P][Tr]            running sum of the skip outputs of a flow
//     melp  [B][80][16 + Tr + 16]      zero-margined mel frames (the conditioning operand)
//     aud0,aud1 [B][8][Lr]             the flow variable ("audio" in glow.py:272-290), natural order
// * training direction (facppg_wg_forward, facppg_wn_*) and FACPPG_WG_UNFOLDED=1: POSITION-MAJOR.
//   L = T*hop/8, Lr = round_up(L, 64), Lp = 128 + Lr + 128:
//     spect [B][640][Lr], h0,h1 [B][256][Lp] (128-wide zero margins), skip [B][256][Lr], aud [B][8][Lr]
//
// Kernels (one launch each):
//   k_mel_pad / k_upsample   mel -> melp (inference) / mel -> spect (training direction)
//   k_noise      Philox4x32-10 + Box-Muller -> z   (only when z is not injected)
//   k_begin      sigma*z -> aud, start conv of the last flow -> h
//   k_wn_layer   ONE fused WaveNet layer: dilated conv (3 taps) + conditioning as a single
//                [512 x 1088] x [1088 x 64] fp32 MFMA GEMM per tile (1408 unfolded), tanh*sigmoid gate,
//                res/skip 1x1 conv as a second [512 x 256] x [256 x 64] MFMA GEMM, residual and skip
//                updates in the epilogue.  >99 % of the FLOPs.  k_wn_layer8 is the
//                8-wave, 32-frame shape for launches smaller than the chip.
//   k_flow_end   end 1x1 conv, affine-coupling inverse, inverse 1x1 conv, early-z concat, then
//                either the next flow's start conv or the final group->time interleave.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "facppg_gemm.h"
#include "facppg_wg_internal.h"

namespace facppg {

thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

constexpr int TN = 64;        // positions per workgroup tile
constexpr int HALO = 128;     // zero margin = max dilation 2^7
constexpr int NCOND = 640;    // n_mel * n_group
constexpr int K1 = 3 * C + NCOND;  // 1408
constexpr int NG1 = K1 / 8;   // 176 k-groups of 8
constexpr int NG2 = C / 8;    // 32
constexpr int NCH1 = K1 / KCH;  // 22 chunks
#ifndef FACPPG_COST16_FULL
#define FACPPG_COST16_FULL 105   // microseconds per round of 16-frame tiles: full round / at most one workgroup per CU, on the scale of
#define FACPPG_COST16_HALF 57    // the other widths' constants (round 5's LDS image made these launches ~10 % faster -- 92 / 51 measured --
                                 // but the 32-frame constants are as stale, and with 92 the model picks 16-frame tiles at T = 200: 8.8 vs 7.7 ms)
#endif
#ifndef FACPPG_WN_W128_DEFAULT
#define FACPPG_WN_W128_DEFAULT 0
#endif
#ifndef FACPPG_WN_RING
#define FACPPG_WN_RING 3     // weight ring of the 64-frame phase-major tiles (3 or 4 register sets)
#endif
#ifndef FACPPG_NARROW_RING
#define FACPPG_NARROW_RING 8  // weight prefetch depth (k-groups) of the 32-column tiles, see k_wn_layer
#endif
// phase-major ("folded conditioning") inference layout, see k_wn_layer<.., PM = true>
constexpr int NGH = 3 * C / 8;   // 96 k-groups of the dilated convolution
constexpr int NCHH = 3 * C / KCH;  // its 12 chunks

// ------------------------------------------------------------------------------------------
// Weight packing (runs once in facppg_wg_create).
// MFMA A-operand image: float4 index ((w*4 + rb)*NG + g)*64 + lane holds, for output row
// rowmap(w, rb, lane&31) and kh = lane>>5, the four K entries 8g + 4kh + {0,1,2,3}.  A wave's
// load of one (rb, g) is therefore 1 KiB contiguous.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int rowmap(int w, int rb, int i) { return (rb >> 1) * C + w * 64 + (rb & 1) * 32 + i; }

__global__ void k_pack_w1(const float* __restrict__ in_w,    // [512][256][3]
                          const float* __restrict__ cond_w,  // [512][640]
                          float4* __restrict__ out) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
  int total = 16 * NG1 * 64;
  if (idx >= total) return;
  int lane = idx & 63, g = (idx >> 6) % NG1, wr = (idx >> 6) / NG1;
  int row = rowmap(wr >> 2, wr & 3, lane & 31);
  float v[4];
  for (int s = 0; s < 4; ++s) {
    int kk = 8 * g + 4 * (lane >> 5) + s;
    v[s] = kk < 3 * C ? in_w[(row * C + (kk % C)) * 3 + kk / C] : cond_w[row * NCOND + (kk - 3 * C)];
  }
  out[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

__global__ void k_pack_w2(const float* __restrict__ rs_w,  // [512 or 256][256]
                          float4* __restrict__ out, int last) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int nrb = last ? 2 : 4;
  int total = 4 * nrb * NG2 * 64;
  if (idx >= total) return;
  int lane = idx & 63, g = (idx >> 6) % NG2, wr = (idx >> 6) / NG2;
  int w = wr / nrb, rb = wr % nrb;
  int row = last ? w * 64 + rb * 32 + (lane & 31) : rowmap(w, rb, lane & 31);
  float v[4];
  for (int s = 0; s < 4; ++s) v[s] = rs_w[row * C + 8 * g + 4 * (lane >> 5) + s];
  out[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// Phase-major images: float4 index (g*16 + w*4 + rb)*64 + lane (k-group slowest), see k_wn_layer<PM>.
__global__ void k_pack_w1_pm(const float* __restrict__ in_w, float4* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NGH * 1024) return;
  const int lane = idx & 63, wr = (idx >> 6) & 15, g = idx >> 10;
  const int row = rowmap(wr >> 2, wr & 3, lane & 31);
  float v[4];
  for (int s = 0; s < 4; ++s) {
    const int kk = 8 * g + 4 * (lane >> 5) + s;
    v[s] = in_w[(row * C + (kk % C)) * 3 + kk / C];
  }
  out[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// U[8m+g][ph*kcp + j*80 + m'] = Wu[m'][m][hop*j + 8*ph + g]: the upsampling kernel laid out so that
// Wc[512 x 640] . U is every phase's folded conditioning matrix at once.
__global__ void k_fold_u(const float* __restrict__ up_w, float* __restrict__ U, int P, int kcp, int kc, int hop, int ksize) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t ncol = (size_t)P * kcp;
  if (idx >= NCOND * ncol) return;
  const int n = idx % ncol, mg = idx / ncol;
  const int ph = n / kcp, r = n % kcp, j = r / NMEL, mp = r % NMEL, m = mg >> 3, g = mg & 7;
  const int k = hop * j + 8 * ph + g;
  U[idx] = (r < kc && k < ksize) ? up_w[((size_t)mp * NMEL + m) * ksize + k] : 0.0f;
}

__global__ void k_pack_cond_pm(const float* __restrict__ F,   // [512][P*kcp] folded matrices
                               float4* __restrict__ out, int P, int kcp) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int ngc = kcp / 8;
  if (idx >= (size_t)P * ngc * 1024) return;
  const int lane = idx & 63, wr = (idx >> 6) & 15, g = (idx >> 10) % ngc, ph = (idx >> 10) / ngc;
  const int row = rowmap(wr >> 2, wr & 3, lane & 31);
  const float* src = F + (size_t)row * P * kcp + (size_t)ph * kcp + 8 * g + 4 * (lane >> 5);
  out[idx] = make_float4(src[0], src[1], src[2], src[3]);
}

// Images for the 16-frame tile kernel (k_wn_layer16, v_mfma_f32_16x16x4_f32): float4 index
// (g16*NB + blk)*64 + lane holds, for output row row16(blk, lane % 16) and kq = lane / 16, the K entries
// 16*g16 + 4*s + kq for s = 0..3 -- the A operands of the four MFMAs of one 16-wide K group.  blk orders the
// 16-row blocks wave by wave: blk = w8*4 + rbl -> rows (rbl>>1)*256 + 32*w8 + 16*(rbl&1) + i  (NB = 32), or
// for the 256-row last res_skip layer blk = w8*2 + rbl -> rows 32*w8 + 16*rbl + i  (NB = 16).
// K order inside a 16-wide group: MFMA s, lane quarter kq -> k16(s, kq).  It is chosen so that the running sum
// meets the K entries in the same sequence as the 32x32x2 kernels do (0,4,1,5,2,6,3,7 within each group of 8):
// a tile then gets the same bits from either kernel, and a batch equals its single runs whatever tile width
// each launch picks.
__device__ __forceinline__ int row16(int blk, int i) { return ((blk & 3) >> 1) * C + (blk >> 2) * 32 + (blk & 1) * 16 + i; }

__global__ void k_pack_w1_16(const float* __restrict__ in_w, float4* __restrict__ out) {   // [512][256][3] -> K = 768
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (3 * C / 16) * 32 * 64) return;
  const int lane = idx & 63, blk = (idx >> 6) & 31, g = idx >> 11;
  const int row = row16(blk, lane & 15);
  float v[4];
  for (int s = 0; s < 4; ++s) {
    const int kk = 16 * g + k16(s, lane >> 4);
    v[s] = in_w[(row * C + (kk % C)) * 3 + kk / C];
  }
  out[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

__global__ void k_pack_cond_16(const float* __restrict__ F,   // [512][P*kcp] folded matrices
                               float4* __restrict__ out, int P, int kcp) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int ng = kcp / 16;
  if (idx >= (size_t)P * ng * 32 * 64) return;
  const int lane = idx & 63, blk = (idx >> 6) & 31, g = (idx >> 11) % ng, ph = (idx >> 11) / ng;
  const float* src = F + (size_t)row16(blk, lane & 15) * P * kcp + (size_t)ph * kcp + 16 * g;
  const int kq = lane >> 4;
  out[idx] = make_float4(src[k16(0, kq)], src[k16(1, kq)], src[k16(2, kq)], src[k16(3, kq)]);
}

__global__ void k_pack_w2_16(const float* __restrict__ rs_w,  // [512 or 256][256]
                             float4* __restrict__ out, int last) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = last ? 16 : 32;
  if (idx >= (C / 16) * nb * 64) return;
  const int lane = idx & 63, blk = (idx >> 6) % nb, g = (idx >> 6) / nb;
  const int row = last ? (blk >> 1) * 32 + (blk & 1) * 16 + (lane & 15) : row16(blk, lane & 15);
  float v[4];
  for (int s = 0; s < 4; ++s) v[s] = rs_w[row * C + 16 * g + k16(s, lane >> 4)];
  out[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// b'[o] = in_b[o] + cond_b[o] + sum_{m,g} Wc[o][8m+g] * up_b[m]   (the upsample bias seen through the 1x1 conv)
__global__ void k_fold_bias(const float* in_b, const float* cond_b, const float* cond_w, const float* up_b, float* out) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= 2 * C) return;
  float v = 0.0f;
  for (int mg = 0; mg < NCOND; ++mg) v = fmaf(cond_w[o * NCOND + mg], up_b[mg >> 3], v);
  out[o] = in_b[o] + cond_b[o] + v;
}

// mel [B][80][T] -> [B][80][HQ + Tr + HQ], zero outside each utterance's valid frames
__global__ void k_mel_pad(const float* __restrict__ mel, float* __restrict__ melp, const int* __restrict__ t_valid, int T, int Tqp) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;   // row = b*80 + m
  if (x >= Tqp) return;
  const int q = x - HQ, Tb = t_valid ? t_valid[row / NMEL] : T;
  melp[(size_t)row * Tqp + x] = (q >= 0 && q < Tb) ? mel[(size_t)row * T + q] : 0.0f;
}

__global__ void k_add_bias(const float* a, const float* b, float* out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// ------------------------------------------------------------------------------------------
// Folded flow edges (inference, phase-major).  Both ends of a WN stack are linear maps next to linear maps:
//
// * glow.py:175 applies the `end` 1x1 conv (256 -> 2*n_half channels) to the SUM of the layers' skip outputs
//   (glow.py:167-174), so layer i's 256 skip rows are only ever seen through W_end:
//     end(sum_i (Ws_i a_i + bs_i)) = sum_i (W_end Ws_i) a_i + (W_end sum_i bs_i + b_end).
//   The res_skip GEMM of a layer therefore needs its 256 res rows plus 2*n_half <= 8 "end" rows, not 512 rows,
//   and the [B][256][L] skip accumulator becomes [B][8][L].  Image `we`: float index ((s*64 + lane)*8 + g) =
//   (W_end Ws_i)[lane % 16][32 s + 4 g + lane / 16]: the A operands of v_mfma_f32_16x16x4_f32, K slice s.
// * glow.py:156-160: the first layer's dilated conv is applied straight to start(x_a) = W_start x_a + b_start, a
//   1x1 conv of the n_half conditioning audio channels.  Composed: a 3-tap conv over n_half + 1 channels (the
//   extra one is 1 inside the utterance and 0 in the zero padding, carrying b_start exactly where the reference
//   pads h with zeros).  K = 24 instead of 768 for the first layer.  Matrix F0 [512][64]: column 8*tap + ch.
// The products are formed once in fp64 and rounded to fp32.
// ------------------------------------------------------------------------------------------
__global__ void k_fold_end_rows(const float* __restrict__ end_w,   // [cc][256]
                                const float* __restrict__ ws,      // [256][256] skip rows of res_skip_layers[i]
                                float* __restrict__ out, int cc) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // (s*64 + lane)*8 + g
  if (idx >= 8 * 64 * 8) return;
  const int g = idx & 7, lane = (idx >> 3) & 63, sl = idx >> 9;
  const int row = lane & 15, k = 32 * sl + 4 * g + (lane >> 4);
  double v = 0.0;
  if (row < cc)
    for (int c = 0; c < C; ++c) v += (double)end_w[row * C + c] * (double)ws[c * C + k];
  out[idx] = (float)v;
}

// endb[j] = end_b[j] + sum_c W_end[j][c] * sum_i bs_i[c];  bs_all = the layers' skip biases, [n_layers][256]
__global__ void k_fold_end_bias(const float* end_w, const float* end_b, const float* bs_all, int n_layers, float* out, int cc) {
  const int j = threadIdx.x;
  if (j >= 8) return;
  double v = 0.0;
  if (j < cc) {
    v = end_b[j];
    for (int c = 0; c < C; ++c) {
      double sb = 0.0;
      for (int i = 0; i < n_layers; ++i) sb += (double)bs_all[i * C + c];
      v += (double)end_w[j * C + c] * sb;
    }
  }
  out[j] = (float)v;
}

__global__ void k_fold_first(const float* __restrict__ in_w,      // [512][256][3]
                             const float* __restrict__ start_w,   // [256][hh]
                             const float* __restrict__ start_b,   // [256]
                             float* __restrict__ F0, int hh) {     // [512][64]
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C * 64) return;
  const int o = idx >> 6, kk = idx & 63, tap = kk >> 3, ch = kk & 7;
  double v = 0.0;
  if (tap < 3 && ch <= hh)
    for (int c = 0; c < C; ++c) v += (double)in_w[((size_t)o * C + c) * 3 + tap] * (double)(ch < hh ? start_w[c * hh + ch] : start_b[c]);
  F0[idx] = (float)v;
}

__global__ void k_copy_rows(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// Ragged batches: the tiles of a phase are cut from the utterances' valid frames laid end to end, each utterance rounded
// up to a multiple of 4 frames (a lane moves 4 frames at a time), instead of per utterance -- no half-empty last tile per
// utterance.  k_group_offsets: off[b] = sum_{b' < b} round_up(T_b', 4) / 4 (one block; chunked scan).  k_group_table:
// entry g = (b, first frame, live frames from there on, 0) for the g-th 4-frame group, zeros past the end.
__global__ __launch_bounds__(1024) void k_group_offsets(const int* __restrict__ t_valid, int B, int* __restrict__ off) {
  __shared__ int part[1024];
  const int t = threadIdx.x, per = (B + 1023) / 1024, b0 = t * per, b1 = min(B, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += (t_valid[b] + 3) / 4;
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;   // exclusive prefix of this thread's chunk
  for (int b = b0; b < b1; ++b) { off[b] = run; run += (t_valid[b] + 3) / 4; }
  if (t == 1023) off[B] = part[1023];
}

__global__ void k_group_table(const int* __restrict__ t_valid, const int* __restrict__ off, int B, int4* __restrict__ table, int n) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  int4 e = make_int4(0, 0, 0, 0);
  if (g < off[B]) {
    int lo = 0, hi = B - 1;   // the last b with off[b] <= g (utterances of zero frames own no group and are skipped)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int q = 4 * (g - off[lo]);
    e = make_int4(lo, q, t_valid[lo] - q, 0);
  }
  table[g] = e;
}

// ------------------------------------------------------------------------------------------
// k_wn_layer
// ------------------------------------------------------------------------------------------
struct WnArgs {
  const float* h_in;
  float* h_out;
  const float* spect;
  float* skip;
  const float4* w1;
  const float* b1;
  const float4* w2;
  const float* b2;
  const int* t_valid;  // may be null
  int T, hop8, Lp, Lr, dil, first;
  float* save_ts;      // training: [B][512][Lr] tanh / sigmoid halves of the gate (SAVE variant)
  // phase-major variant only
  const float* melp;   // [B][80][Tqp] zero-margined mel frames
  const float4* wc;    // folded conditioning weights of this layer: P images [ngc][16][64] float4
  int P, Tr, Tqp, ntq, nt, nch, ngc, kc, xcd_map;
  int hop, ksize;      // upsampler stride / kernel size: late phases reach fewer mel frames (pm_chunks)
  int flat_cols;       // > 0: uniform batch, tiles cut from the B*T frames of a phase laid end to end (no ragged last tile per utterance)
  const int4* groups;  // ragged batch: tiles cut from the utterances' valid frames laid end to end (each rounded up to 4 frames);
                       // entry per 4-frame group = (b, first frame, live frames from there on, -), dead groups have .z <= 0
  // folded flow edges (EF kernels): skip = the [B][8][P*Tr] end-row accumulator
  const float* xa;     // [B][8][P][Tqp] conditioning audio channels + the in-utterance indicator, zero margins (first layer's operand)
  const float* we;     // end-row image of this layer (k_fold_end_rows)
  const float* endb;   // [8] folded end bias (seeds the accumulator in the first layer)
  int nconv;           // K chunks before the conditioning rows: 12 (three taps of 256 channels) or 1 (folded first layer)
  // seeded tiles (k_wn_layer8<..., SEED>): the gate accumulators start from bias + conditioning sums formed ahead of time by
  // k_cond_seed (this layer's slice of its buffer), and the K loop is the convolution chunks alone
  const float4* seed;  // [P][seed_nt][8 waves][2 row blocks][4][64 lanes]
  int seed_nt;         // 32-frame tiles per phase in that buffer
  // fused flow edge (LAST tiles of one short utterance, wn_edge_tile): the tile runs k_flow_end's folded branch for its own
  // columns.  fe_mode = 0: off (the edge is a launch of its own), else 2 * n_half + (1 if the flow prepends early noise)
  int fe_mode, fe_swap, fe_swap_next, fe_L, fe_La;
  float fe_sigma;
  const float* fe_aud_in;    // [8][La]
  float* fe_aud_out;         // [8][La]
  const float* fe_z_early;   // [2][L] or null
  const float* fe_winv;      // [2H][2H]
  const float* fe_start_w;   // next flow: [256][Hn]
  const float* fe_start_b;   // [256]
  float* fe_xa_out;          // [8][Lp]
};

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at 4-byte alignment

template <int NRB>
__device__ __forceinline__ void load_a(float4 (&a)[4], const float4* __restrict__ p, int rb_stride, int g) {
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) a[rb] = p[rb * rb_stride + g * 64];
}

// B operand of one k-group (4 K-steps x NCB column blocks) from the LDS image [k][32*NCB].
// K4 (phase-major kernels): the image is [k/4][32*NCB][k%4] -- the four K-steps a lane feeds into one k-group's MFMAs
// (rows 8g + 4kh + 0..3 of its column) are 16 contiguous bytes, ONE ds_read_b128 per column block instead of four
// ds_read_b32.  With the row-major image hipcc, short of registers, sinks every 4-byte read next to its MFMAs and waits
// for each (lgkmcnt(0) every 8 MFMAs); lb = image + (kh * 32*NCB + li) * 4.
template <int NCB, bool K4 = false>
__device__ __forceinline__ void load_b(float (&bv)[4][NCB], const float* lb, int g) {
  if constexpr (K4) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const float4 v = *reinterpret_cast<const float4*>(lb + ((2 * g) * (32 * NCB) + 32 * cb) * 4);
      bv[0][cb] = v.x; bv[1][cb] = v.y; bv[2][cb] = v.z; bv[3][cb] = v.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) bv[s][cb] = lb[(8 * g + s) * (32 * NCB) + 32 * cb];
  }
}

// K4 image: float index of (k, col)
__device__ __forceinline__ int k4_index(int k, int col, int tnt) { return ((k >> 2) * tnt + col) * 4 + (k & 3); }

// 4 K-steps (one k-group of 8) for NRB row blocks x NCB column blocks.
template <int NRB, int NCB>
__device__ __forceinline__ void mfma_group(f32x16 (&acc)[4][NCB], const float4 (&a)[4], const float (&bv)[4][NCB]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      const float av = s == 0 ? a[rb].x : s == 1 ? a[rb].y : s == 2 ? a[rb].z : a[rb].w;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[rb][cb] = mfma32x32x2(av, bv[s][cb], acc[rb][cb]);
    }
  }
}

// PM = true is the phase-major inference variant.  The upsampling ConvTranspose1d (glow.py:253) is
// linear and the conditioning 1x1 conv (glow.py:160) is applied straight to its regrouped output, so
// the two compose: with P = hop/8 group positions per mel frame, position l = P*q + ph sees
//   cond[o][l] = b'[o] + sum_{j < NJ} sum_{m'} Wf[ph][o][j*80 + m'] * mel[m'][q - j],   NJ = ceil(K/hop)
//   Wf[ph][o][j*80+m'] = sum_{m,g} Wc[o][8m+g] * Wu[m'][m][hop*j + 8*ph + g]   (folded once, at create)
// i.e. K = NJ*80 = 320 rows instead of 640 (hop 256, K 1024), and the [B][640][L] spect tensor and
// the upsample kernel disappear.  The price is one weight image per phase, so a tile must hold
// positions of ONE phase: h and skip are stored phase-major, [B][C][P][frames], where a dilated tap
// l -+ d is simply another phase row ((ph -+ d) mod P) at a frame offset floor((ph -+ d) / P) --
// still one contiguous row per channel.  Workgroups of the same phase run together (and, with
// xcd_map, on the same XCD) so a phase's 655 KB image is fetched into an L2 once.
// K chunks of a phase-major tile: the convolution's 12 plus the folded conditioning rows that are not all
// zero for this phase -- sample hop*j + 8*ph + g exists in the upsampling kernel only for
// j <= (ksize - 1 - 8*ph) / hop, so late phases reach one mel frame less (hop 160: 8 chunks instead of 9
// for phases >= 8; hop 256: always 5).
__device__ __forceinline__ int pm_chunks(const WnArgs& p, int ph) {
  const int nj = (p.ksize - 1 - 8 * ph) / p.hop + 1;
  return min(p.nch, p.nconv + (nj * NMEL + KCH - 1) / KCH);
}

// EF (with PM): folded flow edges, see k_fold_end_rows -- the second GEMM has the 256 res rows only (none in the last
// layer), 8 end rows come from v_mfma_f32_16x16x4_f32 over the gated activations, and the first layer (p.nconv == 1)
// takes its taps from p.xa.
template <bool LAST, int NCB, bool SAVE = false, bool PM = false, bool EF = false>
__global__ __launch_bounds__(256, 2) void k_wn_layer(WnArgs p) {
  static_assert(!EF || PM, "folded flow edges exist on the phase-major layout only");
  // LDS: 2 staging buffers [64 k][TNt] then the gated activations [256][TNt] (aliased); EF: + end rows [8][TNt]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int TNt = 32 * NCB;          // positions per tile: 64 (throughput) or 32 (small problems)
  constexpr int RPL = 64 / TNt;          // k-rows covered by one wave-wide staging load
  constexpr int NSTG = 16 / RPL;         // staging loads per wave per chunk
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 31, kh = lane >> 5;
  const int srow = lane / TNt, scol = lane % TNt;   // this lane's slot inside a staging load
  // tile coordinates: batch b, first column t0 (position, or frame of phase ph), nvalid live columns,
  // in_off / sk_off = offset of column 0 inside a channel row of h / skip, tapo[] = same for the 3 taps
  // PM: tap0..2 are wave-uniform (three named scalars, NOT an array: hipcc turns the per-chunk select over an array into an
  // indexed scratch load behind a vmcnt(0)), the lane's column is lane_q
  int b, t0, nvalid, ph = 0, in_off, sk_off, tap0 = 0, tap1 = 0, tap2 = 0, lane_q = 0;
  if constexpr (PM) {
    const int lin = blockIdx.x;
    int tile;
    if (p.xcd_map == 1) { const int r = lin >> 3; ph = (r / p.nt) * 8 + (lin & 7); tile = r % p.nt; }
    else { ph = lin / p.nt; tile = lin % p.nt; }
    if (ph >= p.P) return;
    // this lane's four columns (staging loads and epilogue stores use the same lane -> column map):
    // batch b, first frame qcol, nvalid = live columns from qcol on (may be <= 0)
    int qcol;
    t0 = 0;
    if (p.groups) {
      const int4 e = p.groups[tile * (TNt / 4) + lane % (TNt / 4)];
      if (__builtin_amdgcn_readfirstlane(e.z) <= 0) return;   // lane 0 holds the tile's first group: the whole tile is past the end
      b = e.x; qcol = e.y; nvalid = e.z;
    } else if (p.flat_cols > 0) {
      const int c0 = tile * TNt + (lane % (TNt / 4)) * 4;
      const int cl = min(c0, p.flat_cols - 4);
      b = cl / p.T; qcol = cl - b * p.T; nvalid = p.flat_cols - c0;
    } else {
      b = tile / p.ntq;
      const int q0 = (tile % p.ntq) * TNt, Tb = p.t_valid ? p.t_valid[b] : p.T;
      if (q0 >= Tb) return;
      qcol = q0 + (lane % (TNt / 4)) * 4; nvalid = Tb - qcol;
    }
    in_off = ph * p.Tqp + HQ + qcol;
    sk_off = ph * p.Tr + qcol;
    lane_q = HQ + qcol;
    {
      const int pm = ph - p.dil, qm = pm >= 0 ? pm / p.P : -((p.P - 1 - pm) / p.P);   // floor((ph - d) / P)
      const int pq = ph + p.dil, qp = pq / p.P;
      tap0 = (pm - qm * p.P) * p.Tqp + qm;
      tap1 = ph * p.Tqp;
      tap2 = (pq - qp * p.P) * p.Tqp + qp;
    }
  } else {
    b = blockIdx.y; t0 = blockIdx.x * TNt;
    nvalid = (p.t_valid ? p.t_valid[b] : p.T) * p.hop8 - t0;
    in_off = HALO + t0;
    sk_off = t0;
  }
  if (!PM && nvalid <= 0) return;

  const float* hb = p.h_in + (size_t)b * C * p.Lp + scol;
  const float* sb = PM ? p.melp + (size_t)b * NMEL * p.Tqp + HQ + t0 + scol : p.spect + (size_t)b * NCOND * p.Lr + t0 + scol;

  // accumulators start at the bias (in_layer.bias + cond_layer.bias, summed at pack time)
  f32x16 acc[4][NCB];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int base = (rb >> 1) * C + w * 64 + (rb & 1) * 32 + 4 * kh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = *reinterpret_cast<const float4*>(p.b1 + base + 8 * q);
      acc[rb][0][4 * q + 0] = bv.x; acc[rb][0][4 * q + 1] = bv.y; acc[rb][0][4 * q + 2] = bv.z; acc[rb][0][4 * q + 3] = bv.w;
    }
#pragma unroll
    for (int cb = 1; cb < NCB; ++cb) acc[rb][cb] = acc[rb][0];
  }

  // PM images are [k-group][16 row blocks][64 lanes]: a k-group's four row blocks sit 1 KiB apart
  const float4* wave_a_ptr = PM ? p.w1 + w * 256 + lane : p.w1 + (size_t)(w * 4) * NG1 * 64 + lane;
  const float4* wave_c_ptr = PM ? p.wc + (size_t)ph * p.ngc * 1024 + w * 256 + lane : nullptr;
  const int nch = PM ? pm_chunks(p, ph) : NCH1;
  // PM: the K order is [conditioning rows | tap -d | tap 0 | tap +d] -- the conditioning chunks, which depend on nothing a
  // previous layer produced, come FIRST (the persistent small-launch path, facppg_wgp.hip, computes them while it waits for
  // the taps' operand; every kernel of the inference path sums in this one order, so a tile gets the same bits from any)
  const int ncc = nch - p.nconv;
  constexpr int F4R = TNt / 4, RPL4 = 64 / F4R, NSTG4 = 16 / RPL4;   // PM staging: float4 per row, rows per wave load, loads
  const int srow4 = lane / F4R, scol4 = (lane % F4R) * 4;
  const bool folded_first = EF && p.nconv == 1;
  const float* hb4 = folded_first ? p.xa + (size_t)b * 8 * p.Lp : p.h_in + (size_t)b * C * p.Lp;   // PM: tapo[] carry the lane's column
  const float* sb4 = PM ? p.melp + (size_t)b * NMEL * p.Tqp + in_off - ph * p.Tqp : nullptr;   // = HQ + qcol
  float stg[NSTG];
  auto stage_load = [&](int c) __attribute__((always_inline)) {
    if constexpr (PM) {
      // both kinds of chunk reduce to "base + per-row offset" so the loads themselves are branch-free.
      // Phase rows are contiguous in frames, so a lane fetches 4 columns at once (16-byte loads at
      // 4-byte alignment: tap offsets are arbitrary) -- 4 VMEM instructions per chunk instead of 16.
      // (a lane stages NSTG4 CONSECUTIVE k-rows of its 4 columns: they are neighbours in the K4 image)
      const bool conv = c >= ncc;
      const int cc = c - ncc;           // conv chunk: channels (cc % 4)*64.. of tap cc / 4
      const float* base = conv ? hb4 : sb4;
      const int tapc = tap0 + (int)(cc >= 4) * (tap1 - tap0) + (int)(cc >= 8) * (tap2 - tap1) + lane_q;
      int off[NSTG4];
#pragma unroll
      for (int jj = 0; jj < NSTG4; ++jj) {
        const int r0 = w * 16 + NSTG4 * srow4 + jj;
        // folded conditioning rows r = j*80 + m' <- mel[m'][q - j]; rows past kc (K padding) meet zero weights
        const int r = min(c * 64 + r0, p.kc - 1);
        const int j = r / NMEL, m = r - j * NMEL;
        // conv rows: channel (cc % 4)*64 + r0 of tap cc / 4; the folded first layer's only conv chunk: row r0 = 8*tap + ch of
        // p.xa (rows >= 24 meet zero weights)
        const int tp = min(r0 >> 3, 2);
        const int conv_off = folded_first ? (r0 & 7) * p.Lp + (tp == 0 ? tap0 : tp == 1 ? tap1 : tap2) + lane_q
                                          : ((cc & 3) * 64 + r0) * p.Lp + tapc;
        off[jj] = conv ? conv_off : m * p.Tqp - j;
      }
#pragma unroll
      for (int jj = 0; jj < NSTG4; ++jj) {
        const f4u v = *reinterpret_cast<const f4u*>(base + off[jj]);
        stg[4 * jj + 0] = v.x; stg[4 * jj + 1] = v.y; stg[4 * jj + 2] = v.z; stg[4 * jj + 3] = v.w;
      }
    } else {
      const float* src;
      int pitch;
      if (c < 12) {
        src = hb + (size_t)((c & 3) * 64 + w * 16 + srow) * p.Lp + in_off + ((c >> 2) - 1) * p.dil;
        pitch = p.Lp;
      } else {
        src = sb + (size_t)((c - 12) * 64 + w * 16 + srow) * p.Lr;
        pitch = p.Lr;
      }
#pragma unroll
      for (int j = 0; j < NSTG; ++j) stg[j] = src[(size_t)(j * RPL) * pitch];
    }
  };
  // A operand of k-group gg (PM: the convolution image, then this phase's conditioning image)
  auto load_a1 = [&](float4 (&a)[4], const float4* ap_, int gg) __attribute__((always_inline)) {
    if constexpr (PM) {
      const int ngc8 = 8 * ncc;
      const float4* src = gg < ngc8 ? wave_c_ptr + (size_t)gg * 1024 : ap_ + (size_t)(gg - ngc8) * 1024;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) a[rb] = src[rb * 64];
    } else {
      load_a<4>(a, ap_, NG1 * 64, gg);
    }
  };
  auto stage_write = [&](int buf) __attribute__((always_inline)) {
    if constexpr (PM) {
      // K4 image [k/4][TNt][k%4]: this lane's NSTG4 consecutive rows of column scol4 + cc are contiguous
      float* dst = smem + buf * (KCH * TNt) + k4_index(w * 16 + NSTG4 * srow4, scol4, TNt);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if constexpr (NSTG4 == 4) *reinterpret_cast<float4*>(dst + 4 * cc) = make_float4(stg[cc], stg[4 + cc], stg[8 + cc], stg[12 + cc]);
        else *reinterpret_cast<float2*>(dst + 4 * cc) = make_float2(stg[cc], stg[4 + cc]);
      }
    } else {
      float* dst = smem + buf * (KCH * TNt) + (w * 16) * TNt + lane;   // (row srow, col scol) = + lane
#pragma unroll
      for (int j = 0; j < NSTG; ++j) dst[j * 64] = stg[j];
    }
  };

  // A operand: a ring of RING register sets, prefetched PD = RING-1 k-groups ahead.  vmcnt retires
  // IN ORDER, so a wait on an A load also waits for every older load -- including the activation
  // staging loads, which come from HBM (2-3 us) while the weights come from L2.  With PD = 1 every
  // chunk stalled ~1 us on that; PD >= 2 gives the staging loads 3+ k-groups (>= 6144 cycles) to
  // land before the first younger A load is needed.  RING = 3 needs the group loop unrolled by
  // lcm(8, 3) = 24 groups = 3 chunks; 22 chunks = 7 x 3 + 1 and 168 % 3 == 0 keeps the phase static.
  constexpr int RING = NCB == 1 ? (PM ? FACPPG_NARROW_RING : 4) : (PM ? FACPPG_WN_RING : 3);
  constexpr int CPI = RING == 3 ? 3 : 1;   // chunks per unrolled iteration
  const float4* ap = wave_a_ptr;
  float4 ar[RING][4];
  stage_load(0);
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) load_a1(ar[i], ap, i);
  stage_write(0);
  __syncthreads();

  // One chunk = 64 K-rows = 8 k-groups.  No branch may sit between the staging loads and the
  // MFMAs that follow: hipcc's waitcnt pass merges the two paths and then waits for the staging
  // loads (vmcnt of the shorter path) at the very first A use -- an HBM round trip per chunk.
  // So the staging load is unconditional (the last chunk re-stages itself, harmlessly) and the
  // tail chunk is peeled instead of guarded.
  auto do_chunk = [&](int c, auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    stage_load(c + 1 < nch ? c + 1 : c);
    const float* lb = smem + (c & 1) * (KCH * TNt) + (PM ? (kh * TNt + li) * 4 : (4 * kh) * TNt + li);
    const int G = c * 8;
    if constexpr (NCB == 1) {
      // narrow tiles run ~1 wave/SIMD with registers to spare: read the B values one k-group ahead
      // (double-buffered) so no ds_read -> s_waitcnt -> MFMA chain is exposed
      float bq[2][4][NCB];
      load_b<NCB, PM>(bq[0], lb, 0);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int gi = j * 8 + g;
        load_a1(ar[(gi + RING - 1) % RING], ap, G + g + RING - 1);
        if (g + 1 < 8) load_b<NCB, PM>(bq[(g + 1) & 1], lb, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_group<4, NCB>(acc, ar[gi % RING], bq[g & 1]);
      }
    } else {
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int gi = j * 8 + g;   // position inside the unrolled iteration (ring phase is static)
        // padded groups exist past the end of the packed image (RING-1 of them)
        load_a1(ar[(gi + RING - 1) % RING], ap, G + g + RING - 1);
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch PD groups ahead (hipcc sinks it otherwise)
        float bq[4][NCB];
        load_b<NCB, PM>(bq, lb, g);
        mfma_group<4, NCB>(acc, ar[gi % RING], bq);
      }
    }
    stage_write((c + 1) & 1);
    __syncthreads();
  };
  if constexpr (CPI == 3 && PM) {
    int c0 = 0;
    for (; c0 + 3 <= nch; c0 += 3) {
      do_chunk(c0, std::integral_constant<int, 0>{});
      do_chunk(c0 + 1, std::integral_constant<int, 1>{});
      do_chunk(c0 + 2, std::integral_constant<int, 2>{});
    }
    if (c0 < nch) do_chunk(c0, std::integral_constant<int, 0>{});
    if (c0 + 1 < nch) do_chunk(c0 + 1, std::integral_constant<int, 1>{});
  } else if constexpr (CPI == 3) {
    static_assert(NCH1 % 3 == 1, "peeling below assumes 22 chunks");
    for (int c0 = 0; c0 + 3 <= NCH1; c0 += 3) {
      do_chunk(c0, std::integral_constant<int, 0>{});
      do_chunk(c0 + 1, std::integral_constant<int, 1>{});
      do_chunk(c0 + 2, std::integral_constant<int, 2>{});
    }
    do_chunk(NCH1 - 1, std::integral_constant<int, 0>{});
  } else {
    for (int c = 0; c < nch; ++c) do_chunk(c, std::integral_constant<int, 0>{});
  }

  // residual inputs h_in[ch][pos] for this lane's res rows are fetched BEFORE the gate so their
  // latency hides under its VALU work; they seed the second GEMM's accumulators (bias + h_in), which
  // makes the residual add free and takes the loads out of the epilogue.  Not in training (SAVE): a chain
  // that starts at h_in rounds each of its 128 steps at the magnitude of h instead of that of the small
  // residual -- h_{i+1} came out 8-10 x further from float64 than one rounded add -- so there
  // the chain starts at the bias and h_in is added once, in the epilogue (64-wide training tiles have no 64 registers to
  // carry it through the second GEMM: they fetch it again there, from L2).
  constexpr bool RES_EARLY = !LAST && !PM && !(SAVE && NCB == 2);
  float hres[(LAST || PM) ? 1 : 2][NCB][16];
  if constexpr (RES_EARLY) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const float* src = p.h_in + ((size_t)b * C + w * 64 + rb * 32 + 4 * kh) * p.Lp + in_off + cb * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) hres[rb][cb][r] = src[(size_t)(8 * (r >> 2) + (r & 3)) * p.Lp];
      }
  }

  // gate: acts = tanh(pre[0:256]) * sigmoid(pre[256:512])  (glow.py:33-40) -> LDS [256][TNt]
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v;
        const int ch = w * 64 + rb * 32 + 8 * (r >> 2) + (r & 3) + 4 * kh;
        if constexpr (SAVE) {   // training: keep tanh and sigmoid separately for the gate's backward
          const float ea = __expf(-2.0f * fminf(fmaxf(acc[rb][cb][r], -15.0f), 15.0f));
          const float T = __fdividef(1.0f - ea, 1.0f + ea), S = __fdividef(1.0f, 1.0f + __expf(-acc[rb + 2][cb][r]));
          v = T * S;
          const int col = cb * 32 + li;
          if (col < nvalid) {
            p.save_ts[((size_t)b * 2 * C + ch) * p.Lr + sk_off + col] = T;
            p.save_ts[((size_t)b * 2 * C + C + ch) * p.Lr + sk_off + col] = S;
          }
        } else {
          v = gate_tanh_sigmoid(acc[rb][cb][r], acc[rb + 2][cb][r]);
        }
        smem[PM ? k4_index(ch, cb * 32 + li, TNt) : ch * TNt + cb * 32 + li] = v;
      }
  __syncthreads();

  // res_skip 1x1 conv: [512 (256 if LAST)] x 256; accumulators start at bias (+ h_in for res rows).
  // EF: the 256 res rows only (image and bias laid out like a LAST layer's 256 rows), nothing in the last layer.
  constexpr int NRB2 = EF ? (LAST ? 0 : 2) : LAST ? 2 : 4;
  constexpr bool ROWS256 = LAST || EF;
#pragma unroll
  for (int rb = 0; rb < NRB2; ++rb) {
    const int base = (ROWS256 ? w * 64 + rb * 32 : (rb >> 1) * C + w * 64 + (rb & 1) * 32) + 4 * kh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = *reinterpret_cast<const float4*>(p.b2 + base + 8 * q);
      acc[rb][0][4 * q + 0] = bv.x; acc[rb][0][4 * q + 1] = bv.y; acc[rb][0][4 * q + 2] = bv.z; acc[rb][0][4 * q + 3] = bv.w;
    }
#pragma unroll
    for (int cb = 1; cb < NCB; ++cb) acc[rb][cb] = acc[rb][0];
    if constexpr (!LAST && !PM && !SAVE) {
      if (rb < 2) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[rb][cb][r] += hres[rb][cb][r];
      }
    }
  }
  if constexpr (NRB2 > 0) {
    const float4* ap2 = p.w2 + (size_t)(w * NRB2) * NG2 * 64 + lane;
    const float* lb = smem + (PM ? (kh * TNt + li) * 4 : (4 * kh) * TNt + li);
#pragma unroll
    for (int i = 0; i < RING - 1; ++i) load_a<NRB2>(ar[i], ap2, NG2 * 64, i);
    constexpr int NCH2 = NG2 / 8;
    auto do_chunk2 = [&](int c, auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int gi = j * 8 + g;
        load_a<NRB2>(ar[(gi + RING - 1) % RING], ap2, NG2 * 64, c * 8 + g + RING - 1);
        __builtin_amdgcn_sched_barrier(0);
        float bq[4][NCB];
        load_b<NCB, PM>(bq, lb, c * 8 + g);
        mfma_group<NRB2, NCB>(acc, ar[gi % RING], bq);
      }
    };
    if constexpr (CPI == 3) {
      static_assert(NCH2 == 4, "peeling below assumes 4 chunks");
      do_chunk2(0, std::integral_constant<int, 0>{});
      do_chunk2(1, std::integral_constant<int, 1>{});
      do_chunk2(2, std::integral_constant<int, 2>{});
      do_chunk2(3, std::integral_constant<int, 0>{});
    } else {
      for (int c = 0; c < NCH2; ++c) do_chunk2(c, std::integral_constant<int, 0>{});
    }
  }

  if constexpr (EF) {
    // end rows: (W_end Ws_i)[8 x 256] . gated[256 x TNt] on 16x16x4 MFMAs, one 16-column block per wave.  Eight K
    // slices of 32, each a chain of 8 MFMAs from zero, summed in slice order: every tile width does exactly this, so
    // a tile gets the same bits from k_wn_layer, k_wn_layer8 and k_wn_layer16.
    if (w < TNt / 16) {
      const int pl = lane & 15, kq = lane >> 4;
      const float4* wimg = reinterpret_cast<const float4*>(p.we) + lane * 2;
      const float* gb = smem + (16 * w + pl) * 4 + kq;   // K4 image: row 32 sl + 4 g + kq of column 16 w + pl
      float4 a0[8], a1[8];
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) { a0[sl] = wimg[sl * 128]; a1[sl] = wimg[sl * 128 + 1]; }
      f32x4 tot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) {
        const float av[8] = {a0[sl].x, a0[sl].y, a0[sl].z, a0[sl].w, a1[sl].x, a1[sl].y, a1[sl].z, a1[sl].w};
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 8; ++g) e = mfma16x16x4(av[g], gb[(8 * sl + g) * TNt * 4], e);
        if (sl == 0) tot = e;
        else { tot[0] += e[0]; tot[1] += e[1]; tot[2] += e[2]; tot[3] += e[3]; }
      }
      if (kq < 2) {
        float* endl = smem + C * TNt + (4 * kq) * TNt + 16 * w + pl;
#pragma unroll
        for (int r = 0; r < 4; ++r) endl[r * TNt] = tot[r];
      }
    }
  }

  if constexpr (PM) {
    // epilogue, phase-major: the MFMA result layout gives a lane one column of 16 rows, i.e. 4-byte
    // accesses.  Each wave transposes its 64 res rows, then its 64 skip rows, through a private
    // [64][TNt] LDS slab and touches HBM with 16-byte row segments instead (4x fewer VMEM instructions).
    __syncthreads();   // every wave is done reading the gated activations
    if constexpr (EF) {
      // end rows: 8 rows x TNt columns, accumulated over the layers of the flow (seeded with the folded end bias)
      const int row = w * RPL4 + srow4;
      if (row < 8 && nvalid > 0) {
        const float4 v4 = *reinterpret_cast<const float4*>(smem + C * TNt + row * TNt + scol4);
        float* g = p.skip + ((size_t)b * 8 + row) * p.Lr + sk_off;
        const float bias = p.endb[row];
        const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
        if (nvalid >= 4) {
          float4 x = make_float4(bias, bias, bias, bias);
          if (!p.first) x = *reinterpret_cast<const float4*>(g);
          *reinterpret_cast<float4*>(g) = make_float4(x.x + vv[0], x.y + vv[1], x.z + vv[2], x.w + vv[3]);
        } else {
          for (int k = 0; k < nvalid; ++k) g[k] = (p.first ? bias : g[k]) + vv[k];
        }
      }
    }
    float* slab = smem + w * (64 * TNt);
#pragma unroll
    for (int half = 0; half < NRB2 / 2; ++half) {
      const bool is_res = EF || (!LAST && half == 0);
#pragma unroll
      for (int rbh = 0; rbh < 2; ++rbh)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            slab[(rbh * 32 + 8 * (r >> 2) + (r & 3) + 4 * kh) * TNt + cb * 32 + li] = acc[half * 2 + rbh][cb][r];
      const int nv = nvalid;   // live columns among this lane's four
      if (nv <= 0) continue;
      float* gbase = is_res ? p.h_out + (size_t)b * C * p.Lp + in_off : p.skip + (size_t)b * C * p.Lr + sk_off;
      const float* rbase = is_res ? p.h_in + (size_t)b * C * p.Lp + in_off : gbase;
      const int pitch = is_res ? p.Lp : p.Lr;
      const bool add = is_res || !p.first;
#pragma unroll 4
      for (int i = 0; i < 64 / RPL4; ++i) {
        const int row = i * RPL4 + srow4;
        const size_t o = (size_t)(w * 64 + row) * pitch;
        float4 v = *reinterpret_cast<const float4*>(slab + row * TNt + scol4);
        if (nv >= 4) {
          if (add) {
            const float4 x = *reinterpret_cast<const float4*>(rbase + o);
            v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
          }
          *reinterpret_cast<float4*>(gbase + o) = v;
        } else {
          const float vv[4] = {v.x, v.y, v.z, v.w};
          for (int k = 0; k < nv; ++k) gbase[o + k] = vv[k] + (add ? rbase[o + k] : 0.0f);
        }
      }
    }
    return;
  }
  // epilogue: h_out = h_in + res (glow.py:165-166), skip (+)= skip part (glow.py:167-174)
#pragma unroll
  for (int rb = 0; rb < NRB2; ++rb) {
    const bool is_res = !LAST && rb < 2;
    const int chb = w * 64 + (rb & 1) * 32 + 4 * kh;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int col = cb * 32 + li;
      if (col < nvalid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ch = chb + 8 * (r >> 2) + (r & 3);
          if (is_res) {
            const size_t o = ((size_t)b * C + ch) * p.Lp + in_off + col;
            float v = acc[rb][cb][r];      // bias + h_in + res (h_in was folded into the accumulator; training: added here)
            if constexpr (SAVE && !LAST && !PM) v += RES_EARLY ? hres[rb & 1][cb][r] : p.h_in[o];
            p.h_out[o] = v;
          } else {
            const size_t o = ((size_t)b * C + ch) * p.Lr + sk_off + col;
            p.skip[o] = (p.first ? 0.0f : p.skip[o]) + acc[rb][cb][r];
          }
        }
      }
    }
  }
}

// FACPPG_WN8_PROF: phase stamps of the 8-wave layer tiles (wn_layer8_tile and wn_layer16_tile; thread 0 of one workgroup per
// launch and tile kind; ticks of the constant 100 MHz clock summed over launches), by tile kind and by the layer's place in
// its flow, read back with facppg_debug_wn_prof -- where a small launch spends its time outside the K loop
// (tools/prof_wn8.py).  A profiling build only: the stamps drain the memory queue at the end of the prologue and of the
// epilogue, so that the operand (seed) round trip and the stores' issue are counted where they belong.
#ifdef FACPPG_WN8_PROF
// [tile kind: 0 = 32-frame tile (workgroup 0), 1 = 16-frame tile (the first one of phase 0)][first, middle, last layer]
// [0-5: prologue, K loop, gate, second GEMM, end rows, epilogue; 6: fused flow edge; 7: launches]
__device__ unsigned long long g_wn_prof[2][3][8];
#define WN8_STAMP_DECL(TK, ON, KIND)                                  \
  long long wn8_t = wall_clock64();                                   \
  const bool wn8_on = (ON) && threadIdx.x == 0;                       \
  unsigned long long* const wn8_slot = g_wn_prof[TK][KIND]
#define WN8_STAMP(i)                                                                           \
  do {                                                                                         \
    if ((i) == 0 || (i) == 5) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 \
    const long long now__ = wall_clock64();                                                    \
    if (wn8_on) { atomicAdd(&wn8_slot[i], (unsigned long long)(now__ - wn8_t)); if ((i) == 5) atomicAdd(&wn8_slot[7], 1ull); } \
    wn8_t = now__;                                                                             \
  } while (0)
#else
#define WN8_STAMP_DECL(TK, ON, KIND)
#define WN8_STAMP(i)
#endif

// ------------------------------------------------------------------------------------------
// k_wn_layer8: the phase-major layer with EIGHT waves per tile.  Wave w8 owns one 32-channel block:
// its tanh rows and the matching sigmoid rows in the first GEMM (2 row blocks instead of 4), its res
// rows and skip rows in the second.  Same LDS footprint and weight traffic per tile as k_wn_layer,
// but twice the waves per SIMD: when a launch has fewer tiles than the chip has workgroup slots
// (one short utterance) a 4-wave tile leaves every SIMD with a single wave, and each barrier, LDS
// round trip and weight load is fully exposed.
// ------------------------------------------------------------------------------------------
// NCB = 4 (128-frame tiles, ONE workgroup per CU, 256 VGPRs): each weight load then feeds four column blocks -- 2 global
// loads per 32 MFMAs instead of k_wn_layer's 4.  tools/probes/mfma_probe.hip: with 2 waves per SIMD the fp32 MFMA stream
// runs at 0.95 of peak next to 2 global_load_dwordx4 per 32 MFMAs and at 0.85 next to 4.
typedef float f32x4s __attribute__((ext_vector_type(4)));
// a load that is a global_load whatever hipcc knows about the pointer: pointers that come out of a device table (k_cond_seed's
// per-layer operands) or out of integer arithmetic are "generic" to it, and every access through them a flat_load -- which
// counts on the LDS counter too, so that the K loop's ds_read waits would wait for the weight loads as well
// (built-in vector types only: a class type such as float4 is copied through a generic reference again)
#define FACPPG_AS1 __attribute__((address_space(1)))
typedef float f32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 gld(const float4* q) {
  const f32x4s v = *(const FACPPG_AS1 f32x4s*)q;
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ f4u gld(const f4u* q) { return *(const FACPPG_AS1 f4u*)q; }
__device__ __forceinline__ float gld(const float* q) { return *(const FACPPG_AS1 float*)q; }
__device__ __forceinline__ void store_f4(float* g, const float4 v) {
  const f32x4s x = {v.x, v.y, v.z, v.w};
  *(FACPPG_AS1 f32x4s*)g = x;
}
// WT: a write-through (sc0 sc1) store -- the line goes on to memory now and does not stay dirty in this XCD's L2 for the write-back
// at the end of the kernel to move.  (An asm store is not on hipcc's memory counters; nothing in a kernel here waits for a store.
// The s_nop keeps the next instruction off the data registers until the store has read them.)
template <bool WT>
__device__ __forceinline__ void store_f4(float* g, const float4 v) {
  if constexpr (WT) {
    const f32x4s x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"((FACPPG_AS1 f32x4s*)g), "v"(x));
  } else store_f4(g, v);
}
__device__ __forceinline__ void store_f1(float* g, const float v) { *(__attribute__((address_space(1))) float*)g = v; }

// ------------------------------------------------------------------------------------------
// wn_edge_tile: the flow edge of one LAST tile's own columns (one short utterance: B = 1), in place of a k_flow_end<QS>
// launch that is a latency chain alone on the chip.  The tile's final end rows are in LDS (fin[8][TW], written by the
// threads that added them into `skip`); one thread per column runs k_flow_end's folded branch on them -- the same
// operations in the same order, hence the same bits -- and leaves the next flow's conditioning channels in LDS, from
// where all eight waves form the start conv (32 channels each, the fmaf chain of start_conv) as 16-byte row segments.
// The start-conv rows go to p.h_out, NOT to the buffer the layer reads (where the separate launch puts them, after the
// whole layer has ended): neighbouring tiles still read these columns of h_in through their dilated taps.
// ------------------------------------------------------------------------------------------
template <int H, bool EARLY, int TW>
__device__ __forceinline__ void wn_edge_column(const WnArgs& p, const int ph, const int x, const int col, float* __restrict__ smem) {
  constexpr int CC = 2 * H, CN = EARLY ? CC + 2 : CC, HN = CN / 2;
  const int pos = x * p.P + ph;
  float a[CC], y[CN], o[CC];
#pragma unroll
  for (int j = 0; j < CC; ++j) a[j] = gld(p.fe_aud_in + (size_t)j * p.fe_La + pos);
  if constexpr (EARLY) {
#pragma unroll
    for (int j = 0; j < 2; ++j) y[j] = p.fe_sigma * gld(p.fe_z_early + (size_t)j * p.fe_L + pos);
  }
#pragma unroll
  for (int j = 0; j < CC; ++j) o[j] = smem[j * TW + col];
#pragma unroll
  for (int j = 0; j < H; ++j) {   // the transformed half: the second one, or (legacy layout, odd flows) the first
    const float t = ((p.fe_swap ? a[j] : a[H + j]) - o[j]) / expf(o[H + j]);
    if (p.fe_swap) a[j] = t;
    else a[H + j] = t;
  }
#pragma unroll
  for (int i = 0; i < CC; ++i) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < CC; ++j) v = fmaf(p.fe_winv[i * CC + j], a[j], v);
    y[(EARLY ? 2 : 0) + i] = v;
  }
#pragma unroll
  for (int j = 0; j < CN; ++j) store_f1(p.fe_aud_out + (size_t)j * p.fe_La + pos, y[j]);
  float* xd = p.fe_xa_out + ph * p.Tqp + HQ + x;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a0 = j < HN ? (p.fe_swap_next ? y[HN + (j < HN ? j : 0)] : y[j < HN ? j : 0]) : j == HN ? 1.0f : 0.0f;
    store_f1(xd + (size_t)j * p.Lp, a0);
    if (j < HN) smem[(8 + j) * TW + col] = a0;
  }
}

// q0: the tile's first frame, ncol: its live columns.  Every thread of the tile calls this (two barriers inside).
template <int TW, bool WT = false>
__device__ __forceinline__ void wn_edge_tile(const WnArgs& p, const int ph, const int q0, const int ncol, float* __restrict__ smem) {
  const int tid = threadIdx.x, lane = tid & 63, w8 = tid >> 6;
  const int hn = (p.fe_mode >> 1) + (p.fe_mode & 1);   // conditioning channels of the NEXT flow
  constexpr int F4 = TW / 4, RP = 64 / F4, NPASS = 32 / RP;
  const int srow = lane / F4, col4 = (lane % F4) * 4;
  // this thread's start-conv operands, requested ahead of the column chain
  float sb[NPASS], sw[NPASS][4];
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    const int ch = 32 * w8 + i * RP + srow;
    sb[i] = gld(p.fe_start_b + ch);
#pragma unroll
    for (int j = 0; j < 4; ++j) sw[i][j] = j < hn ? gld(p.fe_start_w + ch * hn + j) : 0.0f;
  }
  __syncthreads();   // fin is complete
  if (tid < ncol) {
    const int x = q0 + tid;
    switch (p.fe_mode) {
      case 2: wn_edge_column<1, false, TW>(p, ph, x, tid, smem); break;
      case 3: wn_edge_column<1, true, TW>(p, ph, x, tid, smem); break;
      case 4: wn_edge_column<2, false, TW>(p, ph, x, tid, smem); break;
      case 5: wn_edge_column<2, true, TW>(p, ph, x, tid, smem); break;
      case 6: wn_edge_column<3, false, TW>(p, ph, x, tid, smem); break;
      case 7: wn_edge_column<3, true, TW>(p, ph, x, tid, smem); break;
      default: wn_edge_column<4, false, TW>(p, ph, x, tid, smem); break;
    }
  }
  __syncthreads();   // the conditioning channels a0[hn][TW] are in LDS behind fin
  const int nv = ncol - col4;
  if (nv <= 0) return;
  float* hd = p.h_out + ph * p.Tqp + HQ + q0 + col4;
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    const int ch = 32 * w8 + i * RP + srow;
    float v[4] = {sb[i], sb[i], sb[i], sb[i]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < hn) {
        const float4 a0 = *reinterpret_cast<const float4*>(smem + (8 + j) * TW + col4);
        v[0] = fmaf(sw[i][j], a0.x, v[0]); v[1] = fmaf(sw[i][j], a0.y, v[1]);
        v[2] = fmaf(sw[i][j], a0.z, v[2]); v[3] = fmaf(sw[i][j], a0.w, v[3]);
      }
    }
    float* g = hd + (size_t)ch * p.Lp;
    if (nv >= 4) store_f4<WT>(g, make_float4(v[0], v[1], v[2], v[3]));
    else
      for (int k = 0; k < nv; ++k) store_f1(g + k, v[k]);
  }
}

// NS: the small-launch schedule (32-frame tiles; FACPPG_WN_SMALL=legacy runs NS = false).  Same operands, same MFMAs, same
// order of every sum -- only when things are requested and how stores leave the CU differ:
//   * the second GEMM's first operands (three ring sets of w2, its bias, the end-row image, the residual rows) are requested
//     in front of the gate, whose arithmetic covers their L2 round trip; behind the K loop the weight ring is dead, so the
//     requests take the registers it held
//   * every 16-byte row segment the epilogue publishes (h_out, the end rows in `skip`, the fused edge's start-conv rows) is
//     stored write-through, so the write-back at the end of the kernel finds nothing dirty
template <bool LAST, int NCB, bool EF, bool SEED = false, bool NS = false>
__device__ __forceinline__ void wn_layer8_tile(const WnArgs& p, const int lin, float* __restrict__ smem) {
  static_assert(!SEED || NCB == 1, "seeded tiles: 32 frames");
  static_assert(!NS || (NCB == 1 && EF), "small-launch schedule: 32 frames, folded flow edges");
  constexpr int TNt = 32 * NCB;
  WN8_STAMP_DECL(0, blockIdx.x == 0, p.first ? 0 : LAST ? 2 : 1);
  const int tid = threadIdx.x, lane = tid & 63, w8 = tid >> 6, wq = w8 >> 1, sub = w8 & 1;
  const int li = lane & 31, kh = lane >> 5;
  const int chb = wq * 64 + sub * 32;   // first channel of this wave's block
  int b, nvalid, ph, in_off, sk_off, tap0, tap1, tap2, lane_q;   // tap0..2 are wave-uniform, the lane's column is lane_q (see k_wn_layer)
  int tile;
  {
    if (p.xcd_map == 1) { const int r = lin >> 3; ph = (r / p.nt) * 8 + (lin & 7); tile = r % p.nt; }
    else { ph = lin / p.nt; tile = lin % p.nt; }
    if (ph >= p.P) return;
    int qcol;
    if (p.groups) {
      const int4 e = p.groups[tile * (TNt / 4) + lane % (TNt / 4)];
      if (__builtin_amdgcn_readfirstlane(e.z) <= 0) return;   // lane 0 holds the tile's first group: the whole tile is past the end
      b = e.x; qcol = e.y; nvalid = e.z;
    } else if (p.flat_cols > 0) {
      const int c0 = tile * TNt + (lane % (TNt / 4)) * 4;
      const int cl = min(c0, p.flat_cols - 4);
      b = cl / p.T; qcol = cl - b * p.T; nvalid = p.flat_cols - c0;
    } else {
      b = tile / p.ntq;
      const int q0 = (tile % p.ntq) * TNt, Tb = p.t_valid ? p.t_valid[b] : p.T;
      if (q0 >= Tb) return;
      qcol = q0 + (lane % (TNt / 4)) * 4; nvalid = Tb - qcol;
    }
    in_off = ph * p.Tqp + HQ + qcol;
    sk_off = ph * p.Tr + qcol;
    lane_q = HQ + qcol;
    {
      const int pm = ph - p.dil, qm = pm >= 0 ? pm / p.P : -((p.P - 1 - pm) / p.P);   // floor((ph - d) / P)
      const int pq = ph + p.dil, qp = pq / p.P;
      tap0 = (pm - qm * p.P) * p.Tqp + qm;
      tap1 = ph * p.Tqp;
      tap2 = (pq - qp * p.P) * p.Tqp + qp;
    }
  }
  f32x16 acc[2][NCB];   // [0] tanh rows / res rows, [1] sigmoid rows / skip rows of channels chb..chb+31
  // images are [k-group][16 row blocks][64 lanes]; row block index = wq*4 + sub (+2 for the second half)
  const float4* wave_a = p.w1 + (wq * 4 + sub) * 64 + lane;
  const float4* wave_c = p.wc + (size_t)ph * p.ngc * 1024 + (wq * 4 + sub) * 64 + lane;
  // SEED: the conditioning chunks (and the bias) are already in the accumulators' seed
  const int nch = SEED ? p.nconv : pm_chunks(p, ph);
  const int ncc = SEED ? 0 : nch - p.nconv;   // the conditioning chunks come first (see k_wn_layer)
  constexpr int F4R = TNt / 4, RPL4 = 64 / F4R, NSTG4 = 8 / RPL4;
  const int srow4 = lane / F4R, scol4 = (lane % F4R) * 4;
  const bool folded_first = EF && p.nconv == 1;
  const float* hb4 = folded_first ? p.xa + (size_t)b * 8 * p.Lp : p.h_in + (size_t)b * C * p.Lp;
  const float* sb4 = p.melp + (size_t)b * NMEL * p.Tqp + in_off - ph * p.Tqp;
  float4 stg[NSTG4];
  auto stage_load = [&](int c) __attribute__((always_inline)) {
    const bool conv = c >= ncc;
    const int cc = c - ncc;
    const float* base = conv ? hb4 : sb4;
    const int tapc = tap0 + (int)(cc >= 4) * (tap1 - tap0) + (int)(cc >= 8) * (tap2 - tap1) + lane_q;
#pragma unroll
    for (int jj = 0; jj < NSTG4; ++jj) {
      const int r0 = w8 * 8 + NSTG4 * srow4 + jj;   // consecutive k-rows per lane: neighbours in the K4 image (see load_b)
      const int r = min(c * 64 + r0, p.kc - 1);
      const int j = r / NMEL, m = r - j * NMEL;
      const int tp = min(r0 >> 3, 2);               // folded first layer: conv row r0 = 8*tap + ch of p.xa
      const int conv_off = folded_first ? (r0 & 7) * p.Lp + (tp == 0 ? tap0 : tp == 1 ? tap1 : tap2) + lane_q
                                        : ((cc & 3) * 64 + r0) * p.Lp + tapc;
      const int off = conv ? conv_off : m * p.Tqp - j;
      const f4u v = gld(reinterpret_cast<const f4u*>(base + off));
      stg[jj] = make_float4(v.x, v.y, v.z, v.w);
    }
  };
  auto stage_write = [&](int buf) __attribute__((always_inline)) {
    float* dst = smem + buf * (KCH * TNt) + k4_index(w8 * 8 + NSTG4 * srow4, scol4, TNt);
    if constexpr (NSTG4 == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(stg[0].x, stg[1].x, stg[2].x, stg[3].x);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(stg[0].y, stg[1].y, stg[2].y, stg[3].y);
      *reinterpret_cast<float4*>(dst + 8) = make_float4(stg[0].z, stg[1].z, stg[2].z, stg[3].z);
      *reinterpret_cast<float4*>(dst + 12) = make_float4(stg[0].w, stg[1].w, stg[2].w, stg[3].w);
    } else if constexpr (NSTG4 == 2) {
      dst[0] = stg[0].x; dst[1] = stg[1].x; dst[4] = stg[0].y; dst[5] = stg[1].y;
      dst[8] = stg[0].z; dst[9] = stg[1].z; dst[12] = stg[0].w; dst[13] = stg[1].w;
    } else {
      dst[0] = stg[0].x; dst[4] = stg[0].y; dst[8] = stg[0].z; dst[12] = stg[0].w;
    }
  };
  auto load_a1 = [&](float4 (&a)[2], int gg) __attribute__((always_inline)) {
    const int ngc8 = 8 * ncc;
    const float4* src = gg < ngc8 ? wave_c + (size_t)gg * 1024 : wave_a + (size_t)(gg - ngc8) * 1024;
    a[0] = gld(src);
    a[1] = gld(src + 128);
  };
  auto mfma2 = [&](const float4 (&a)[2], const float (&bv)[4][NCB], int nrb) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        if (rb >= nrb) continue;
        const float av = s == 0 ? a[rb].x : s == 1 ? a[rb].y : s == 2 ? a[rb].z : a[rb].w;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[rb][cb] = mfma32x32x2(av, bv[s][cb], acc[rb][cb]);
      }
  };
  constexpr int RING = 4;
  float4 ar[RING][2];
  stage_load(0);
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) load_a1(ar[i], i);
  // accumulators start at the bias (SEED: at bias + conditioning sums, k_cond_seed's registers as it left them); loaded behind
  // the first operand loads so the prologue is one memory round trip, not two
  const float4* seedp = SEED ? p.seed + ((((size_t)ph * p.seed_nt + tile) * 8 + w8) * 8) * 64 + lane : nullptr;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = SEED ? gld(seedp + (rb * 4 + q) * 64) : gld(reinterpret_cast<const float4*>(p.b1 + rb * C + chb + 4 * kh + 8 * q));
      acc[rb][0][4 * q + 0] = bv.x; acc[rb][0][4 * q + 1] = bv.y; acc[rb][0][4 * q + 2] = bv.z; acc[rb][0][4 * q + 3] = bv.w;
    }
#pragma unroll
    for (int cb = 1; cb < NCB; ++cb) acc[rb][cb] = acc[rb][0];
  }
  stage_write(0);
  __syncthreads();
  WN8_STAMP(0);   // prologue
  for (int c = 0; c < nch; ++c) {
    stage_load(c + 1 < nch ? c + 1 : c);
    const float* lb = smem + (c & 1) * (KCH * TNt) + (kh * TNt + li) * 4;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      load_a1(ar[(g + RING - 1) % RING], c * 8 + g + RING - 1);
      __builtin_amdgcn_sched_barrier(0);
      float bq[4][NCB];
      load_b<NCB, true>(bq, lb, g);
      mfma2(ar[g % RING], bq, 2);
    }
    stage_write((c + 1) & 1);
    __syncthreads();   // (ablation bit 1: no barrier per chunk -- racy, timing only)
  }
  WN8_STAMP(1);   // K loop
  // res_skip 1x1 conv
  constexpr int NRB2 = EF ? (LAST ? 0 : 1) : LAST ? 1 : 2;   // EF: res rows only (image laid out like a LAST layer's 256 rows)
  constexpr bool ROWS256 = LAST || EF;
  // narrow tiles run one workgroup per CU: nothing hides the epilogue's read of h_in (the residual), so fetch it here,
  // ahead of the second GEMM
  // NCB = 1 (one workgroup per CU, nothing to hide behind): the end rows are split by K slice over the eight waves, as in
  // k_wn_layer16 -- wave w8 forms slice w8 of both 16-column blocks; its 32 bytes of the image are fetched here, ahead of
  // the second GEMM.  (One wave per column block doing all eight slices cost 3.9 us of a 75 us launch, six waves idle.)
  constexpr bool ESPLIT = EF && NCB == 1;
  constexpr bool HPRE = !LAST && NCB == 1;
  float4 es0, es1;
  float4 hpre[HPRE ? 32 / RPL4 : 1];
  float4 b2v[NRB2 > 0 ? NRB2 : 1][4];
  // w2 image: float4 index ((wq*nrb + rb4)*NG2 + g)*64 + lane, nrb = 2 (LAST) or 4
  const float4* ap2 = p.w2 + (size_t)(ROWS256 ? wq * 2 + sub : wq * 4 + sub) * NG2 * 64 + lane;
  auto load_a2 = [&](float4 (&a)[2], int g) __attribute__((always_inline)) {
    a[0] = gld(ap2 + g * 64);
    if constexpr (!ROWS256) a[1] = gld(ap2 + (size_t)2 * NG2 * 64 + g * 64);
  };
  // everything the second GEMM, the end rows and the epilogue read from memory (the K loop's ring `ar` and `stg` are dead)
  auto request2 = [&]() __attribute__((always_inline)) {
    if constexpr (ESPLIT) {
      const float4* wimg = reinterpret_cast<const float4*>(p.we) + w8 * 128 + lane * 2;
      es0 = gld(wimg); es1 = gld(wimg + 1);
    }
    if constexpr (HPRE) {
      if (nvalid >= 4) {
        const float* rb0 = p.h_in + (size_t)b * C * p.Lp + in_off;
#pragma unroll
        for (int i = 0; i < 32 / RPL4; ++i) hpre[i] = gld(reinterpret_cast<const float4*>(rb0 + (size_t)(chb + i * RPL4 + srow4) * p.Lp));
      }
    }
#pragma unroll
    for (int rb = 0; rb < NRB2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) b2v[rb][q] = gld(reinterpret_cast<const float4*>(p.b2 + (ROWS256 ? 0 : rb * C) + chb + 4 * kh + 8 * q));
    if constexpr (NRB2 > 0) {
#pragma unroll
      for (int i = 0; i < RING - 1; ++i) load_a2(ar[i], i);
    }
  };
  if constexpr (NS) {   // in front of the gate: its arithmetic covers the round trip
    request2();
    __builtin_amdgcn_sched_barrier(0);
  }
  // gate -> LDS [256][TNt]
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      smem[k4_index(chb + 8 * (r >> 2) + (r & 3) + 4 * kh, cb * 32 + li, TNt)] = gate_tanh_sigmoid(acc[0][cb][r], acc[1][cb][r]);
  __syncthreads();
  WN8_STAMP(2);   // gate
  if constexpr (!NS) request2();
#pragma unroll
  for (int rb = 0; rb < NRB2; ++rb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = b2v[rb][q];
      acc[rb][0][4 * q + 0] = bv.x; acc[rb][0][4 * q + 1] = bv.y; acc[rb][0][4 * q + 2] = bv.z; acc[rb][0][4 * q + 3] = bv.w;
    }
#pragma unroll
    for (int cb = 1; cb < NCB; ++cb) acc[rb][cb] = acc[rb][0];
  }
  if constexpr (NRB2 > 0) {
    const float* lb = smem + (kh * TNt + li) * 4;
    for (int c = 0; c < NG2 / 8; ++c) {
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        load_a2(ar[(g + RING - 1) % RING], c * 8 + g + RING - 1);
        __builtin_amdgcn_sched_barrier(0);
        float bq[4][NCB];
        load_b<NCB, true>(bq, lb, c * 8 + g);
        mfma2(ar[g % RING], bq, NRB2);
      }
    }
  }
  WN8_STAMP(3);   // second GEMM
  if constexpr (ESPLIT) {
    const int pl = lane & 15, kq = lane >> 4;
    const float av[8] = {es0.x, es0.y, es0.z, es0.w, es1.x, es1.y, es1.z, es1.w};
#pragma unroll
    for (int blk = 0; blk < TNt / 16; ++blk) {
      const float* gb = smem + (16 * blk + pl) * 4 + kq + (8 * w8) * TNt * 4;   // K4 image, rows 32 w8 + 4 g + kq
      f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < 8; ++g) e = mfma16x16x4(av[g], gb[g * TNt * 4], e);
      if (kq < 2) {
        float* part = smem + C * TNt + (w8 * 8 + 4 * kq) * TNt + 16 * blk + pl;   // [slice][row][column]
#pragma unroll
        for (int r = 0; r < 4; ++r) part[r * TNt] = e[r];
      }
    }
  } else if constexpr (EF) {   // end rows, exactly as in k_wn_layer<EF>
    if (w8 < TNt / 16) {
      const int pl = lane & 15, kq = lane >> 4;
      const float4* wimg = reinterpret_cast<const float4*>(p.we) + lane * 2;
      const float* gb = smem + (16 * w8 + pl) * 4 + kq;   // K4 image
      float4 a0[8], a1[8];
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) { a0[sl] = gld(wimg + sl * 128); a1[sl] = gld(wimg + sl * 128 + 1); }
      f32x4 tot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) {
        const float av[8] = {a0[sl].x, a0[sl].y, a0[sl].z, a0[sl].w, a1[sl].x, a1[sl].y, a1[sl].z, a1[sl].w};
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 8; ++g) e = mfma16x16x4(av[g], gb[(8 * sl + g) * TNt * 4], e);
        if (sl == 0) tot = e;
        else { tot[0] += e[0]; tot[1] += e[1]; tot[2] += e[2]; tot[3] += e[3]; }
      }
      if (kq < 2) {
        float* endl = smem + C * TNt + (4 * kq) * TNt + 16 * w8 + pl;
#pragma unroll
        for (int r = 0; r < 4; ++r) endl[r * TNt] = tot[r];
      }
    }
  }
  // epilogue through a private [32][TNt] LDS slab per wave, 16-byte row segments to HBM
  __syncthreads();
  WN8_STAMP(4);   // end rows
  if constexpr (EF) {
    const int row = w8 * RPL4 + srow4;
    if (row < 8 && nvalid > 0) {
      float4 v4 = *reinterpret_cast<const float4*>(smem + C * TNt + row * TNt + scol4);
      if constexpr (ESPLIT) {   // the slices meet here, added in slice order (the order every tile width uses)
#pragma unroll
        for (int sl = 1; sl < 8; ++sl) {
          const float4 x = *reinterpret_cast<const float4*>(smem + C * TNt + (sl * 8 + row) * TNt + scol4);
          v4.x += x.x; v4.y += x.y; v4.z += x.z; v4.w += x.w;
        }
      }
      float* g = p.skip + ((size_t)b * 8 + row) * p.Lr + sk_off;
      const float bias = p.endb[row];
      const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
      float fs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (nvalid >= 4) {
        float4 x = make_float4(bias, bias, bias, bias);
        if (!p.first) x = *reinterpret_cast<const float4*>(g);
        fs[0] = x.x + vv[0]; fs[1] = x.y + vv[1]; fs[2] = x.z + vv[2]; fs[3] = x.w + vv[3];
        store_f4<NS>(g, make_float4(fs[0], fs[1], fs[2], fs[3]));
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < nvalid) { fs[k] = (p.first ? bias : g[k]) + vv[k]; store_f1(g + k, fs[k]); }
      }
      if constexpr (LAST && ESPLIT) {   // fused flow edge: the final rows go on to the column threads (the gate image is dead)
        if (p.fe_mode) *reinterpret_cast<float4*>(smem + row * TNt + scol4) = make_float4(fs[0], fs[1], fs[2], fs[3]);
      }
    }
  }
  if constexpr (LAST && ESPLIT) {
    if (p.fe_mode) {   // (B = 1: the tile's first frame follows from its index alone)
      const int q0 = (p.flat_cols > 0 ? tile : tile % p.ntq) * TNt;
      wn_edge_tile<TNt, NS>(p, ph, q0, min(TNt, (p.t_valid ? p.t_valid[0] : p.T) - q0), smem);
    }
  }
  WN8_STAMP(6);   // fused flow edge (with the add into skip)
  float* slab = smem + w8 * (32 * TNt);
#pragma unroll
  for (int half = 0; half < NRB2; ++half) {
    const bool is_res = EF || (!LAST && half == 0);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) slab[(8 * (r >> 2) + (r & 3) + 4 * kh) * TNt + cb * 32 + li] = acc[half][cb][r];
    const int nv = nvalid;
    if (nv <= 0) continue;
    float* gbase = is_res ? p.h_out + (size_t)b * C * p.Lp + in_off : p.skip + (size_t)b * C * p.Lr + sk_off;
    const float* rbase = is_res ? p.h_in + (size_t)b * C * p.Lp + in_off : gbase;
    const int pitch = is_res ? p.Lp : p.Lr;
    const bool add = is_res || !p.first;
#pragma unroll
    for (int i = 0; i < 32 / RPL4; ++i) {
      const int row = i * RPL4 + srow4;
      const size_t o = (size_t)(chb + row) * pitch;
      float4 v = *reinterpret_cast<const float4*>(slab + row * TNt + scol4);
      if (nv >= 4) {
        if (add) {
          float4 x;
          if (HPRE && is_res) x = hpre[i];
          else x = gld(reinterpret_cast<const float4*>(rbase + o));
          v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
        }
        store_f4<NS>(gbase + o, v);
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < nv; ++k) store_f1(gbase + o + k, vv[k] + (add ? gld(rbase + o + k) : 0.0f));
      }
    }
  }
  WN8_STAMP(5);   // epilogue
}

template <bool LAST, int NCB, bool EF = false, bool SEED = false, bool NS = false>
__global__ __launch_bounds__(512, NCB == 4 ? 2 : 4) void k_wn_layer8(WnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  wn_layer8_tile<LAST, NCB, EF, SEED, NS>(p, (int)blockIdx.x, smem);
}


struct WnLayerPtrs {   // the per-layer operands of one flow (device table, built once per handle)
  const float4* w1;
  const float4* wc;
  const float* b1;
  const float4* w2;
  const float* b2;
  const float* we;
};

// ------------------------------------------------------------------------------------------
// k_cond_seed: the conditioning part of every WN layer's gate GEMM, ahead of the layers themselves.
// A layer's accumulators are bias + sum over the conditioning chunks BEFORE any tap (the K order of k_wn_layer8 is
// conditioning first), and that part depends on the mel frames alone -- not on the flow variable.  For one utterance the
// decoder leaves most of the chip idle for milliseconds while the mel frames trickle out; this kernel forms, for a block of
// frames that are final, exactly the MFMA sequence k_wn_layer8 would run for its conditioning chunks (same operands, same
// order: same bits) for EVERY (flow, layer, phase), and parks the accumulator registers in HBM in the lane order the seeded
// layer kernel reads them back in (k_wn_layer8<..., SEED>: 12 K chunks instead of 17, first layers 1 instead of 6).
// Workgroup = (group of `lpw` layers, phase, block of NCB 32-frame tiles): the mel window of the block is staged into LDS
// once (all conditioning chunks: ncc * 8 KiB per 32 frames) and every layer streams its folded per-phase weight image past
// it -- no barrier inside the K loop.  One pass over a frame block reads every (layer, phase) image once (2 GB at hop 256):
// 16 * NCB FLOP per weight byte, so narrow blocks are HBM-bound and wide ones MFMA-bound.
// ------------------------------------------------------------------------------------------
struct SeedArgs {
  const float* melp;        // [80][Tqp] zero-margined mel frames of the ONE utterance
  float4* seeds;            // [layers_total][P][seed_nt][8][2][4][64]
  const void* ltab[MAXF];   // per flow: WnLayerPtrs[wn_layers] (device)
  int layers_total, wn_layers, lpw;
  int P, Tqp, seed_nt;
  int tile0, nblk;          // first 32-frame tile of this launch, NCB-tile blocks from there
  int ncmax, kc, ngc, hop, ksize;   // conditioning chunks at most (kcp / 64), rows, k-groups per phase image, upsampler stride / size
  const int* skip;          // optional (device): *skip != 0 -> the launch does nothing (the frames never became final)
  int items;                // work items = layer groups x phases x blocks (a bounded launch has fewer workgroups than that)
  int layer0, layer1;       // the layers of this launch: [layer0, layer1) of layers_total (flow-major: layer = flow * wn_layers + i)
  int* counter;             // bounded launch: the next item to hand out (zero at launch), or null: item = blockIdx, + gridDim, ...
};

template <bool NT>
__device__ __forceinline__ float4 gld_w(const float4* q) {   // NT: a stream that is read once -- do not keep it in the L2
  if constexpr (NT) {
    const f32x4s v = __builtin_nontemporal_load((const FACPPG_AS1 f32x4s*)q);
    return make_float4(v.x, v.y, v.z, v.w);
  } else return gld(q);
}

template <int NCB, bool NT>
__global__ __launch_bounds__(512, NCB <= 2 ? 4 : 2) void k_cond_seed(SeedArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [ncc][64 k][TNt] K4 images of the block's mel window
  constexpr int TNt = 32 * NCB;
  const int tid = threadIdx.x, lane = tid & 63, w8 = tid >> 6, wq = w8 >> 1, sub = w8 & 1;
  const int li = lane & 31, kh = lane >> 5;
  const int chb = wq * 64 + sub * 32;
  if (p.skip && *p.skip) return;
  // a launch may be bounded to fewer workgroups than it has work items (p.items): each then walks items blockIdx, + gridDim, ...
  // (gridDim a multiple of 8: an item stays on the XCD its index names)
  for (int lin = (int)blockIdx.x;;) {
  // (bounded launch with a counter: the first gridDim items are the workgroups' own, the counter hands out the rest -- no
  // workgroup idles while another still has a queue of its own)
  if (lin >= p.items) break;
  // workgroup i lands on XCD i % 8: the blocks that share a (layer, phase) image run back to back on one XCD
  int lg, ph, blk;
  {
    if (p.P % 8 == 0) {
      const int r = lin >> 3, rest = r / p.nblk;
      blk = r - rest * p.nblk; ph = (rest % (p.P / 8)) * 8 + (lin & 7); lg = rest / (p.P / 8);
    } else {
      blk = lin % p.nblk; const int rest = lin / p.nblk;
      ph = rest % p.P; lg = rest / p.P;
    }
  }
  const int l0 = p.layer0 + lg * p.lpw, l1 = min(l0 + p.lpw, p.layer1);
  // conditioning chunks of this phase (pm_chunks): late phases reach one mel frame less
  const int nj = (p.ksize - 1 - 8 * ph) / p.hop + 1;
  const int ncc = min(p.ncmax, (nj * NMEL + KCH - 1) / KCH);
  const int q0 = (p.tile0 + blk * NCB) * 32;   // first frame of the block
  constexpr int F4R = TNt / 4, RPL4 = 64 / F4R, NSTG4 = 8 / RPL4;
  const int srow4 = lane / F4R, scol4 = (lane % F4R) * 4;
  // stage every conditioning chunk, exactly as k_wn_layer8's stage_load / stage_write do for c < ncc
  {
    const float* sb4 = p.melp + HQ + q0 + scol4;
    for (int c = 0; c < ncc; ++c) {
      float4 stg[NSTG4];
#pragma unroll
      for (int jj = 0; jj < NSTG4; ++jj) {
        const int r0 = w8 * 8 + NSTG4 * srow4 + jj;
        const int r = min(c * 64 + r0, p.kc - 1);
        const int j = r / NMEL, m = r - j * NMEL;
        const f4u v = gld(reinterpret_cast<const f4u*>(sb4 + m * p.Tqp - j));
        stg[jj] = make_float4(v.x, v.y, v.z, v.w);
      }
      float* dst = smem + c * (KCH * TNt) + k4_index(w8 * 8 + NSTG4 * srow4, scol4, TNt);
      if constexpr (NSTG4 == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(stg[0].x, stg[1].x, stg[2].x, stg[3].x);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(stg[0].y, stg[1].y, stg[2].y, stg[3].y);
        *reinterpret_cast<float4*>(dst + 8) = make_float4(stg[0].z, stg[1].z, stg[2].z, stg[3].z);
        *reinterpret_cast<float4*>(dst + 12) = make_float4(stg[0].w, stg[1].w, stg[2].w, stg[3].w);
      } else if constexpr (NSTG4 == 2) {
        dst[0] = stg[0].x; dst[1] = stg[1].x; dst[4] = stg[0].y; dst[5] = stg[1].y;
        dst[8] = stg[0].z; dst[9] = stg[1].z; dst[12] = stg[0].w; dst[13] = stg[1].w;
      } else {
        dst[0] = stg[0].x; dst[4] = stg[0].y; dst[8] = stg[0].z; dst[12] = stg[0].w;
      }
    }
  }
  // the weight stream: k-group G of the workgroup = group G % ng of layer l0 + G / ng; ring of 4, as in k_wn_layer8
  const int ng = 8 * ncc;
  const size_t wave_off = (size_t)ph * p.ngc * 1024 + (wq * 4 + sub) * 64 + lane;
  auto layer_ptrs = [&](int l) __attribute__((always_inline)) {
    const WnLayerPtrs* t = reinterpret_cast<const WnLayerPtrs*>(p.ltab[l / p.wn_layers]) + (l % p.wn_layers);
    return t;
  };
  constexpr int RING = 4;
  float4 ar[RING][2];
  const float4* wc_cur = layer_ptrs(l0)->wc + wave_off;   // image of the layer the prefetch is in
  int g_in = 0, l_pre = l0;                             // its k-group inside that layer
  auto load_next = [&](float4 (&a)[2]) __attribute__((always_inline)) {
    const float4* src = wc_cur + (size_t)g_in * 1024;
    a[0] = gld_w<NT>(src);
    a[1] = gld_w<NT>(src + 128);
    if (++g_in == ng) {                                  // (wave-uniform) on to the next layer's image; past the last one: stay
      g_in = 0;
      if (l_pre + 1 < l1) { ++l_pre; wc_cur = layer_ptrs(l_pre)->wc + wave_off; }
      else g_in = ng - 1;
    }
  };
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) load_next(ar[i]);
  __syncthreads();
  const float* lb0 = smem + (kh * TNt + li) * 4;
  for (int l = l0; l < l1; ++l) {
    const float* b1 = layer_ptrs(l)->b1;
    f32x16 acc[2][NCB];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bv = gld(reinterpret_cast<const float4*>(b1 + rb * C + chb + 4 * kh + 8 * q));
        acc[rb][0][4 * q + 0] = bv.x; acc[rb][0][4 * q + 1] = bv.y; acc[rb][0][4 * q + 2] = bv.z; acc[rb][0][4 * q + 3] = bv.w;
      }
#pragma unroll
      for (int cb = 1; cb < NCB; ++cb) acc[rb][cb] = acc[rb][0];
    }
    for (int c = 0; c < ncc; ++c) {
      const float* lb = lb0 + c * (KCH * TNt);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        load_next(ar[(g + RING - 1) % RING]);
        __builtin_amdgcn_sched_barrier(0);
        float bq[4][NCB];
        load_b<NCB, true>(bq, lb, g);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
            const float4& a4 = ar[g % RING][rb];
            const float av = s4 == 0 ? a4.x : s4 == 1 ? a4.y : s4 == 2 ? a4.z : a4.w;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[rb][cb] = mfma32x32x2(av, bq[s4][cb], acc[rb][cb]);
          }
      }
    }
    // park the accumulators: one 32-frame tile per column block, in the seeded kernel's own register order
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int tile = p.tile0 + blk * NCB + cb;
      if (tile >= p.seed_nt) continue;
      float4* dst = p.seeds + (((((size_t)l * p.P + ph) * p.seed_nt + tile) * 8 + w8) * 8) * 64 + lane;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4s x = {acc[rb][cb][4 * q + 0], acc[rb][cb][4 * q + 1], acc[rb][cb][4 * q + 2], acc[rb][cb][4 * q + 3]};
          if constexpr (NT) __builtin_nontemporal_store(x, (FACPPG_AS1 f32x4s*)(dst + (rb * 4 + q) * 64));
          else *(FACPPG_AS1 f32x4s*)(dst + (rb * 4 + q) * 64) = x;
        }
    }
  }
  __syncthreads();   // (the next item restages the LDS image)
  if (p.counter) {   // (the image is dead: its first word carries the next item to every wave)
    if (tid == 0) reinterpret_cast<int*>(smem)[0] = (int)gridDim.x + atomicAdd(p.counter, 1);
    __syncthreads();
    lin = reinterpret_cast<const int*>(smem)[0];
    __syncthreads();
  } else lin += (int)gridDim.x;
  }
}

// ------------------------------------------------------------------------------------------
// k_wn_layer16: the phase-major layer on 16-frame tiles with v_mfma_f32_16x16x4_f32.  A launch smaller
// than the chip (one short utterance; anything at hop 160, whose 20 phases give few tiles) is bound by
// tile granularity: halving the tile doubles the workgroups that share the work.  Eight waves per tile,
// wave w8 owning channels 32*w8 .. 32*w8+31 as four 16-row blocks (two tanh, two sigmoid; then two res,
// two skip); ~115 VGPRs, 16 KiB of LDS: two workgroups per CU.  Tiles are per utterance (no flat cut).
// ------------------------------------------------------------------------------------------
constexpr int TN16 = 16;

// one 16-frame tile: phase ph, frames q0 .. q0 + 15 of utterance b
// WT: the epilogue's 16-byte row segments are stored write-through (the mixed launch's small-launch schedule, see wn_layer8_tile)
template <bool LAST, bool EF, bool WT = false>
__device__ __forceinline__ void wn_layer16_tile(const WnArgs& p, const int ph, const int b, const int q0, float* __restrict__ smem,
                                                const bool stamp = false) {   // stamp: FACPPG_WN8_PROF builds, this workgroup reports
  const int tid = threadIdx.x, lane = tid & 63, w8 = tid >> 6;
  const int pl = lane & 15, kq = lane >> 4;
  const int chb = w8 * 32;
  const int nvalid = (p.t_valid ? p.t_valid[b] : p.T) - q0;
  if (nvalid <= 0) return;
  WN8_STAMP_DECL(1, stamp, p.first ? 0 : LAST ? 2 : 1);
  const int in_off = ph * p.Tqp + HQ + q0, sk_off = ph * p.Tr + q0;
  int tapo[3];
#pragma unroll
  for (int tp = 0; tp < 3; ++tp) {
    const int pp = ph + (tp - 1) * p.dil;
    const int qsh = pp >= 0 ? pp / p.P : -((p.P - 1 - pp) / p.P);
    tapo[tp] = (pp - qsh * p.P) * p.Tqp + HQ + q0 + qsh;
  }
  f32x4 acc[4];
  const float4* wave_a = p.w1 + (w8 * 4) * 64 + lane;                                    // + g16 * 2048 + rbl * 64
  const float4* wave_c = p.wc + (size_t)ph * (p.ngc / 2) * 2048 + (w8 * 4) * 64 + lane;   // ngc counts 8-wide groups
  const int nch = pm_chunks(p, ph), ncc = nch - p.nconv, NGC16 = ncc * 4;   // the conditioning chunks come first (see k_wn_layer)
  // staging: a chunk is 64 k-rows x 16 frames = 1024 floats, two per thread
  const int srow = tid >> 3, scol = (tid & 7) * 2;
  const bool folded_first = EF && p.nconv == 1;
  const float* hb = (folded_first ? p.xa + (size_t)b * 8 * p.Lp : p.h_in + (size_t)b * C * p.Lp) + scol;
  const float* sb = p.melp + (size_t)b * NMEL * p.Tqp + HQ + q0 + scol;
  typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
  float2 stg;
  auto stage_load = [&](int c) __attribute__((always_inline)) {
    const bool conv = c >= ncc;
    const int cc = c - ncc;
    const int r = min(c * 64 + srow, p.kc - 1);
    const int j = r / NMEL, m = r - j * NMEL;
    const int tp = folded_first ? min(srow >> 3, 2) : cc >> 2;
    const int chn = folded_first ? (srow & 7) : (cc & 3) * 64 + srow;
    const float* src = conv ? hb + (size_t)chn * p.Lp + (tp == 0 ? tapo[0] : tp == 1 ? tapo[1] : tapo[2])
                            : sb + m * p.Tqp - j;
    const f2u v = *reinterpret_cast<const f2u*>(src);
    stg = make_float2(v.x, v.y);
  };
  // LDS image of a chunk: [16-wide k group g][lane quarter kq][column][s] -- the four k rows 16 g + k16(s, kq), s = 0..3, that
  // lane (column, kq) feeds into the group's four MFMAs are 16 contiguous bytes: ONE ds_read_b128 per group instead of four
  // ds_read_b32 with a wait each (the 32-frame kernels' K4 image, see load_b).  Row r16 = k16(s, kq) <-> s = 2 (r16 >> 3) +
  // ((r16 >> 1) & 1), kq = 2 (r16 & 1) + ((r16 >> 2) & 1).
  const int sw_r = srow & 15, sw_base = (((srow >> 4) * 4 + 2 * (sw_r & 1) + ((sw_r >> 2) & 1)) * TN16) * 4 + 2 * (sw_r >> 3) + ((sw_r >> 1) & 1);
  auto stage_write = [&](int buf) __attribute__((always_inline)) {
    float* dst = smem + buf * (KCH * TN16) + sw_base + scol * 4;
    dst[0] = stg.x; dst[4] = stg.y;
  };
  auto load_a = [&](float4 (&a)[4], int gg) __attribute__((always_inline)) {   // gg = 16-wide K group over [conv | cond]
    const float4* src = gg < NGC16 ? wave_c + (size_t)gg * 2048 : wave_a + (size_t)(gg - NGC16) * 2048;
#pragma unroll
    for (int rbl = 0; rbl < 4; ++rbl) a[rbl] = src[rbl * 64];
  };
  constexpr int RING = 4;
  float4 ar[RING][4];
  stage_load(0);
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) load_a(ar[i], i);
#pragma unroll
  for (int rbl = 0; rbl < 4; ++rbl) {
    const float4 bv = *reinterpret_cast<const float4*>(p.b1 + (rbl >> 1) * C + chb + (rbl & 1) * 16 + 4 * kq);
    acc[rbl][0] = bv.x; acc[rbl][1] = bv.y; acc[rbl][2] = bv.z; acc[rbl][3] = bv.w;
  }
  stage_write(0);
  __syncthreads();
  WN8_STAMP(0);   // prologue
  for (int c = 0; c < nch; ++c) {
    stage_load(c + 1 < nch ? c + 1 : c);
    const float* lb = smem + (c & 1) * (KCH * TN16) + (kq * TN16 + pl) * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      load_a(ar[(g + RING - 1) % RING], c * 4 + g + RING - 1);
      __builtin_amdgcn_sched_barrier(0);
      const float4 b4 = *reinterpret_cast<const float4*>(lb + g * (4 * TN16 * 4));
      const float bq[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rbl = 0; rbl < 4; ++rbl) {
          const float4& a4 = ar[g % RING][rbl];
          acc[rbl] = mfma16x16x4(s == 0 ? a4.x : s == 1 ? a4.y : s == 2 ? a4.z : a4.w, bq[s], acc[rbl]);
        }
    }
    stage_write((c + 1) & 1);
    __syncthreads();
  }
  WN8_STAMP(1);   // K loop
  // gate -> LDS [256][16]
#pragma unroll
  for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
    for (int r = 0; r < 4; ++r)   // channel chb + 16 rbl + 4 kq + r into the same [group][kq][column][s] image
      smem[(((2 * w8 + rbl) * 4 + 2 * (r & 1) + (kq & 1)) * TN16 + pl) * 4 + 2 * (kq >> 1) + ((r >> 1) & 1)] = gate_tanh_sigmoid(acc[rbl][r], acc[rbl + 2][r]);
  __syncthreads();
  WN8_STAMP(2);   // gate
  // res_skip 1x1 conv: blocks rbl 0,1 = res rows chb.., rbl 2,3 = skip rows 256+chb.. (LAST: rbl 0,1 = skip rows chb..)
  constexpr int NB2 = EF ? (LAST ? 0 : 2) : LAST ? 2 : 4;   // EF: res rows only (image laid out like a LAST layer's 256 rows)
  constexpr bool ROWS256 = LAST || EF;
  // the residual h_in of this wave's 32 res rows, fetched ahead of the second GEMM (see k_wn_layer8)
  float4 hpre[2];
  if constexpr (!LAST) {
    if (nvalid - (lane & 3) * 4 >= 4) {
#pragma unroll
      for (int it = 0; it < 2; ++it)
        hpre[it] = *reinterpret_cast<const float4*>(p.h_in + ((size_t)b * C + chb + it * 16 + (lane >> 2)) * p.Lp + in_off + (lane & 3) * 4);
    }
  }
#pragma unroll
  for (int rbl = 0; rbl < NB2; ++rbl) {
    const float4 bv = *reinterpret_cast<const float4*>(p.b2 + (ROWS256 ? 0 : (rbl >> 1) * C) + chb + (rbl & 1) * 16 + 4 * kq);
    acc[rbl][0] = bv.x; acc[rbl][1] = bv.y; acc[rbl][2] = bv.z; acc[rbl][3] = bv.w;
  }
  if constexpr (NB2 > 0) {
    const float4* ap2 = p.w2 + (w8 * NB2) * 64 + lane;   // [g16][NB2*8 blocks][64]
    const float* lb = smem + (kq * TN16 + pl) * 4;
    auto load_a2 = [&](float4 (&a)[4], int g) __attribute__((always_inline)) {
#pragma unroll
      for (int rbl = 0; rbl < NB2; ++rbl) a[rbl] = ap2[(size_t)g * (NB2 * 8 * 64) + rbl * 64];
    };
#pragma unroll
    for (int i = 0; i < RING - 1; ++i) load_a2(ar[i], i);
    for (int c = 0; c < C / 64; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        load_a2(ar[(g + RING - 1) % RING], c * 4 + g + RING - 1);
        __builtin_amdgcn_sched_barrier(0);
        const float4 b4 = *reinterpret_cast<const float4*>(lb + (4 * c + g) * (4 * TN16 * 4));
        const float bq[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int rbl = 0; rbl < NB2; ++rbl) {
            const float4& a4 = ar[g % RING][rbl];
            acc[rbl] = mfma16x16x4(s == 0 ? a4.x : s == 1 ? a4.y : s == 2 ? a4.z : a4.w, bq[s], acc[rbl]);
          }
      }
    }
  }
  WN8_STAMP(3);   // second GEMM
  if constexpr (EF) {
    // end rows (see k_wn_layer<EF>): wave w8 forms K slice w8 of the single 16-column block; the slices meet in LDS
    // and are summed in slice order below -- the same sums, in the same order, as the wider tiles
    const float4* wimg = reinterpret_cast<const float4*>(p.we) + w8 * 128 + lane * 2;
    const float4 a0 = wimg[0], a1 = wimg[1];
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    // (gated channel 32 w8 + 4 g + kq in the [group][kq][column][s] image)
    f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 8; ++g)
      e = mfma16x16x4(av[g], smem[(((2 * w8 + (g >> 2)) * 4 + 2 * (kq & 1) + (g & 1)) * TN16 + pl) * 4 + 2 * ((g & 3) >> 1) + (kq >> 1)], e);
    if (kq < 2) {
      float* part = smem + C * TN16 + (w8 * 8 + 4 * kq) * TN16 + pl;
#pragma unroll
      for (int r = 0; r < 4; ++r) part[r * TN16] = e[r];
    }
  }
  // epilogue through a private [32][16] LDS slab per wave, 16-byte row segments to HBM
  __syncthreads();
  WN8_STAMP(4);   // end rows
  if constexpr (EF) {
    if (tid < 32) {
      const int row = tid >> 2, c4 = (tid & 3) * 4, nv = nvalid - c4;
      if (nv > 0) {
        const float* part = smem + C * TN16 + row * TN16 + c4;
        float4 t = *reinterpret_cast<const float4*>(part);
#pragma unroll
        for (int sl = 1; sl < 8; ++sl) {
          const float4 x = *reinterpret_cast<const float4*>(part + sl * 8 * TN16);
          t.x += x.x; t.y += x.y; t.z += x.z; t.w += x.w;
        }
        float* g = p.skip + ((size_t)b * 8 + row) * p.Lr + sk_off + c4;
        const float bias = p.endb[row];
        const float vv[4] = {t.x, t.y, t.z, t.w};
        float fs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (nv >= 4) {
          float4 x = make_float4(bias, bias, bias, bias);
          if (!p.first) x = *reinterpret_cast<const float4*>(g);
          fs[0] = x.x + vv[0]; fs[1] = x.y + vv[1]; fs[2] = x.z + vv[2]; fs[3] = x.w + vv[3];
          store_f4<WT>(g, make_float4(fs[0], fs[1], fs[2], fs[3]));
        } else {
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (k < nv) { fs[k] = (p.first ? bias : g[k]) + vv[k]; g[k] = fs[k]; }
        }
        if constexpr (LAST) {   // fused flow edge: the final rows go on to the column threads (the gate image is dead)
          if (p.fe_mode) *reinterpret_cast<float4*>(smem + row * TN16 + c4) = make_float4(fs[0], fs[1], fs[2], fs[3]);
        }
      }
    }
    if constexpr (LAST) {
      if (p.fe_mode) wn_edge_tile<TN16, WT>(p, ph, q0, min(TN16, nvalid), smem);
    }
  }
  WN8_STAMP(6);   // fused flow edge (with the add into skip)
  float* slab = smem + w8 * (32 * TN16);
  const int erow = lane >> 2, ecol = (lane & 3) * 4;   // 16 rows x 4 float4 per pass, two passes
#pragma unroll
  for (int half = 0; half < NB2 / 2; ++half) {
    const bool is_res = EF || (!LAST && half == 0);
#pragma unroll
    for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(16 * rbl + 4 * kq + r) * TN16 + pl] = acc[half * 2 + rbl][r];
    const int nv = nvalid - ecol;
    if (nv <= 0) continue;
    float* gbase = is_res ? p.h_out + (size_t)b * C * p.Lp + in_off + ecol : p.skip + (size_t)b * C * p.Lr + sk_off + ecol;
    const float* rbase = is_res ? p.h_in + (size_t)b * C * p.Lp + in_off + ecol : gbase;
    const int pitch = is_res ? p.Lp : p.Lr;
    const bool add = is_res || !p.first;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = it * 16 + erow;
      const size_t o = (size_t)(chb + row) * pitch;
      float4 v = *reinterpret_cast<const float4*>(slab + row * TN16 + ecol);
      if (nv >= 4) {
        if (add) {
          float4 x;
          if (!LAST && is_res) x = hpre[it];
          else x = *reinterpret_cast<const float4*>(rbase + o);
          v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
        }
        store_f4<WT>(gbase + o, v);
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < nv; ++k) gbase[o + k] = vv[k] + (add ? rbase[o + k] : 0.0f);
      }
    }
  }
  WN8_STAMP(5);   // epilogue
}

template <bool LAST, bool EF = false>
__global__ __launch_bounds__(512, 4) void k_wn_layer16(WnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int ph, tile;
  {
    const int lin = blockIdx.x;
    if (p.xcd_map == 1) { const int r = lin >> 3; ph = (r / p.nt) * 8 + (lin & 7); tile = r % p.nt; }
    else { ph = lin / p.nt; tile = lin % p.nt; }
    if (ph >= p.P) return;
  }
  wn_layer16_tile<LAST, EF>(p, ph, tile / p.ntq, (tile % p.ntq) * TN16, smem, ph == 0 && tile == 0);
}

// ------------------------------------------------------------------------------------------
// k_wn_layer_mixed (one streamed utterance): the frames whose seeds k_cond_seed formed under the decoder run as seeded
// 32-frame tiles (12 K chunks), the frames behind them -- the ones that became final only when the decoder ended -- as
// UNSEEDED 16-frame tiles of the same launch (17 K chunks on half the columns: 57 us against the seeded tile's 56 with one
// workgroup per CU), instead of waiting for a seed pass over them (2 GB of weight images for a handful of frames) in front of
// the vocoder.  Per phase: n32 seeded tiles, then the 16-frame tiles from frame 32 * n32 on.  Both kinds of tile are the code of
// the single-kind launches (wn_layer8_tile<SEED>, wn_layer16_tile): same sums in the same order, same bits.
// ------------------------------------------------------------------------------------------
template <bool LAST, bool NS>
__global__ __launch_bounds__(512, 4) void k_wn_layer_mixed(WnArgs p32, WnArgs p16, int n32) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lin = (int)blockIdx.x, nt = p32.nt;   // tiles per phase of this launch: n32 + the 16-frame tiles
  int ph, tile;
  if (p32.xcd_map == 1) { const int r = lin >> 3; ph = (r / nt) * 8 + (lin & 7); tile = r % nt; }
  else { ph = lin / nt; tile = lin % nt; }
  if (ph >= p32.P) return;
  if (tile < n32) wn_layer8_tile<LAST, 1, true, true, NS>(p32, lin, smem);
  else wn_layer16_tile<LAST, true, NS>(p16, ph, 0, 32 * n32 + (tile - n32) * TN16, smem, ph == 0 && tile == n32);
}

// ------------------------------------------------------------------------------------------
// k_upsample: ConvTranspose1d(n_mel, n_mel, K, stride=hop) + trim + regroup (glow.py:253-259)
// out[m][n] = bias[m] + sum_{m'} sum_{t: 0 <= n - t*hop < K} mel[m'][t] * W[m'][m][n - t*hop]
// One workgroup = (batch b, output channel m, block of QB frames).  Thread p owns the `hop`-phase
// p: it keeps QB accumulators (one per frame q) so each weight it loads is reused QB times and
// the mel values come from LDS as broadcasts.
// ------------------------------------------------------------------------------------------
constexpr int UP_QB = 32;
constexpr int UP_MAXJ = 8;  // ceil(K / hop) <= 8  (hop >= 128 for K = 1024)

__global__ __launch_bounds__(256) void k_upsample(const float* __restrict__ mel, const float* __restrict__ W,
                                                  const float* __restrict__ bias, float* __restrict__ spect,
                                                  const int* __restrict__ t_valid, int T, int n_mel, int hop,
                                                  int ksize, int Lr, int n_limit) {
  extern __shared__ float smel[];  // [n_mel][UP_QB + UP_MAXJ]
  const int b = blockIdx.z, m = blockIdx.y, q0 = blockIdx.x * UP_QB;
  const int Tb = t_valid ? t_valid[b] : T;
  if (q0 >= Tb) return;
  const int nj = (ksize + hop - 1) / hop;
  const int SW = UP_QB + UP_MAXJ;
  for (int i = threadIdx.x; i < n_mel * SW; i += blockDim.x) {
    const int mp = i / SW, tt = i % SW;
    const int t = q0 - (UP_MAXJ - 1) + tt;  // column tt <-> frame q0 - 7 + tt
    smel[i] = (t >= 0 && t < Tb && tt < UP_QB + UP_MAXJ - 1) ? mel[((size_t)b * n_mel + mp) * T + t] : 0.0f;
  }
  __syncthreads();
  for (int pp = threadIdx.x; pp < hop; pp += blockDim.x) {
    float acc[UP_QB];
    const float bv = bias[m];
#pragma unroll
    for (int q = 0; q < UP_QB; ++q) acc[q] = bv;
    for (int j = 0; j < nj; ++j) {
      const int k = pp + j * hop;
      if (k < ksize) {
        for (int mp = 0; mp < n_mel; ++mp) {
          const float wv = W[((size_t)mp * n_mel + m) * ksize + k];
          const float* sm = smel + mp * SW + (UP_MAXJ - 1) - j;  // frame q0 + q - j
#pragma unroll
          for (int q = 0; q < UP_QB; ++q) acc[q] = fmaf(sm[q], wv, acc[q]);
        }
      }
    }
    // n = (q0+q)*hop + pp -> channel m*8 + n%8, position n/8 ; frames >= Tb are not produced
    const int hop8 = hop >> 3;
    float* dst = spect + ((size_t)b * n_mel * 8 + m * 8 + (pp & 7)) * Lr + (pp >> 3);
#pragma unroll
    for (int q = 0; q < UP_QB; ++q)
      if (q0 + q < Tb && (q0 + q) * hop + pp < n_limit) dst[(size_t)(q0 + q) * hop8] = acc[q];
  }
}

// ------------------------------------------------------------------------------------------
// k_noise: counter-based N(0,1) (Philox4x32-10, Box-Muller) replacing normal_() glow.py:266-289
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// four N(0,1) values from one Philox block (two Box-Muller pairs)
__device__ __forceinline__ void normal4(const uint32_t (&r)[4], float (&o)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(r[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
    const float u2 = ((float)(r[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.28318530717958647692f * u2, &sn, &cs);
    o[2 * h] = rad * cs; o[2 * h + 1] = rad * sn;
  }
}

__global__ void k_noise(float* __restrict__ z, size_t n, uint64_t seed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // produces z[4i .. 4i+3]
  if (4 * i >= n) return;
  uint32_t r[4];
  philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  float o[4];
  normal4(r, o);
  for (int j = 0; j < 4; ++j)
    if (4 * i + j < n) z[4 * i + j] = o[j];
}

// Per-utterance noise streams: value (segment, channel, position) of utterance b depends only on seeds[b] --
// not on the batch size, the utterance's slot in the batch or the padded length -- so a padded batch drawn with
// per-utterance seeds reproduces every utterance's own batch-1 draw (Philox key = seeds[b], counter =
// (position / 4, channel, segment)).  z: the flat injected-z layout of facppg_wg_infer.
__global__ void k_noise_utt(float* __restrict__ z, const uint64_t* __restrict__ seeds, int B, int L, int n_first, int n_early,
                            int n_seg) {
  const int l4 = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (4 * l4 >= L) return;
  const uint64_t seed = seeds[b];
  size_t seg_off = 0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int nch = sg == 0 ? n_first : n_early;
    for (int ch = 0; ch < nch; ++ch) {
      uint32_t r[4];
      philox4x32_10((uint32_t)l4, (uint32_t)ch, (uint32_t)sg, 0x7A5Eu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
      float o[4];
      normal4(r, o);
      float* dst = z + seg_off + ((size_t)b * nch + ch) * L + 4 * l4;
      for (int j = 0; j < 4; ++j)
        if (4 * l4 + j < L) dst[j] = o[j];
    }
    seg_off += (size_t)B * nch * L;
  }
}

// ------------------------------------------------------------------------------------------
// k_begin: audio = sigma * z0 (glow.py:261-270) and the start conv of the last flow (glow.py:156)
// ------------------------------------------------------------------------------------------
struct EdgeArgs {
  const float* skip;       // [B][256][Lr]
  const float* aud_in;     // [B][8][Lr]
  float* aud_out;          // [B][8][Lr]
  float* h_out;            // [B][256][Lp]
  float* final_audio;      // [B][T*hop]
  const float* z0;         // [B][c][L]  (k_begin)
  const float* z_early;    // [B][n_early][L] or null
  const float* end_w;      // [2H][256]
  const float* end_b;      // [2H]
  const float* winv;       // [2H][2H]
  const float* start_w;    // next flow: [256][Hn]
  const float* start_b;    // [256]
  const int* t_valid;
  float sigma;
  int T, hop8, Lp, Lr, L, n_early, final_flow;
  int swap, swap_next;     // legacy layout (glow_old.py:224-240): odd flows condition on the SECOND half
  int La;                  // channel pitch of aud_in / aud_out (always position-major)
  int P, Tr, Tqp;          // P > 0: h and skip are phase-major (k_wn_layer<PM>), grid = (frames/256, B, P)
  // folded flow edges (k_wn_layer<EF>): `skip` holds the end conv's output already, [B][8][Lr]; the next flow's
  // conditioning channels also go to xa_out [B][8][Lp] (+ the in-utterance indicator channel) for its folded first layer
  int folded;
  float* xa_out;
};

// rows 0..HN-1 = the conditioning audio channels, row HN = 1 (inside the utterance), rows above = 0
template <int HN>
__device__ __forceinline__ void write_xa(const EdgeArgs& p, int b, int h_off, const float* a0) {
  float* dst = p.xa_out + (size_t)b * 8 * p.Lp + h_off;
#pragma unroll
  for (int j = 0; j < 8; ++j) dst[(size_t)j * p.Lp] = j < HN ? a0[j] : j == HN ? 1.0f : 0.0f;
}

// This thread's position: natural index `pos` (into aud / z / the output audio) and the offsets of
// that position inside a channel row of h and of skip.
__device__ __forceinline__ bool edge_pos(const EdgeArgs& p, int b, int x, int& pos, int& h_off, int& sk_off) {
  const int Tb = p.t_valid ? p.t_valid[b] : p.T;
  if (p.P > 0) {
    const int ph = blockIdx.z;
    if (x >= Tb) return false;
    pos = x * p.P + ph; h_off = ph * p.Tqp + HQ + x; sk_off = ph * p.Tr + x;
  } else {
    if (x >= Tb * p.hop8) return false;
    pos = x; h_off = HALO + x; sk_off = x;
  }
  return true;
}

template <int HN>
__device__ __forceinline__ void start_conv(const EdgeArgs& p, int b, int h_off, const float* a0, int ch0 = 0, int nch = C) {
  float* dst = p.h_out + (size_t)b * C * p.Lp + h_off;
  for (int ch = ch0; ch < ch0 + nch; ++ch) {
    float v = p.start_b[ch];
#pragma unroll
    for (int j = 0; j < HN; ++j) v = fmaf(p.start_w[ch * HN + j], a0[j], v);
    dst[(size_t)ch * p.Lp] = v;
  }
}

// QS (few positions: one short utterance): 64 positions per workgroup, the four waves take 64 start-conv channels each -- a
// thread that walks all 256 channel rows alone is a chain of 256 dependent-address stores (38 us for 200 frames x 32 phases)
template <int HN, bool QS = false>
__global__ __launch_bounds__(256) void k_begin(EdgeArgs p) {
  const int b = blockIdx.y;
  const int pl = QS ? (int)(threadIdx.x & 63) : (int)threadIdx.x, wq = QS ? (int)(threadIdx.x >> 6) : 0;
  int pos, h_off, sk_off;
  if (!edge_pos(p, b, blockIdx.x * (QS ? 64 : 256) + pl, pos, h_off, sk_off)) return;
  float a[2 * HN];
#pragma unroll
  for (int j = 0; j < 2 * HN; ++j) {
    a[j] = p.sigma * p.z0[((size_t)b * 2 * HN + j) * p.L + pos];
    if (wq == 0) p.aud_out[((size_t)b * 8 + j) * p.La + pos] = a[j];
  }
  if constexpr (QS) start_conv<HN>(p, b, h_off, a + (p.swap_next ? HN : 0), 64 * wq, 64);
  else start_conv<HN>(p, b, h_off, a + (p.swap_next ? HN : 0));
  if (p.folded && wq == 0) write_xa<HN>(p, b, h_off, a + (p.swap_next ? HN : 0));
}

// ------------------------------------------------------------------------------------------
// k_flow_end<H, EARLY>: for a flow with n_half = H (glow.py:175, 278-290):
//   out = end(skip) ; b = out[:H], s = out[H:] ; a1 = (a1 - b)/exp(s) ; audio = W^-1 [a0; a1]
//   EARLY: audio = cat(sigma*z, audio) ; then next flow's start conv, or the final interleave
// ------------------------------------------------------------------------------------------
template <int H, bool EARLY, bool QS>
__global__ __launch_bounds__(256) void k_flow_end(EdgeArgs p) {
  // QS (launches with few positions -- one short utterance): 64 positions per workgroup; the four waves split
  // the 256 skip channels of the end conv (and later the 256 output channels of the next start conv), so the
  // launch still spreads over the chip and each thread's chain of L2 round trips is a quarter as long; the
  // partial sums meet in LDS in a fixed order.  !QS (large launches, HBM-bound): one thread per position.
  constexpr int CC = 2 * H;
  __shared__ float red[QS ? 4 : 1][CC][QS ? 64 : 1];
  const int b = blockIdx.y, pl = QS ? (threadIdx.x & 63) : threadIdx.x, qtr = QS ? (threadIdx.x >> 6) : 0;
  constexpr int CQ = QS ? C / 4 : C;   // channels per thread
  int pos = 0, h_off = 0, sk_off = 0;
  const bool valid = edge_pos(p, b, blockIdx.x * (QS ? 64 : 256) + pl, pos, h_off, sk_off);
  // Both shapes sum the same way -- four 64-channel chains, then bias + q0 + q1 + q2 + q3 -- so an utterance
  // gets the same bits whichever shape its batch selects.
  float o[CC];
  const float* sk = p.skip + (size_t)b * C * p.Lr + sk_off;
  auto quarter = [&](int q, float (&acc)[CC]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < CC; ++j) acc[j] = 0.0f;
    for (int c0 = q * 64; c0 < q * 64 + 64; c0 += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = sk[(size_t)(c0 + u) * p.Lr];
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int j = 0; j < CC; ++j) acc[j] = fmaf(p.end_w[j * C + c0 + u], v[u], acc[j]);
    }
  };
  if (p.folded) {
    if (!valid) return;
#pragma unroll
    for (int j = 0; j < CC; ++j) o[j] = p.skip[((size_t)b * 8 + j) * p.Lr + sk_off];
  } else if constexpr (QS) {
#pragma unroll
    for (int j = 0; j < CC; ++j) o[j] = 0.0f;
    if (valid) quarter(qtr, o);
#pragma unroll
    for (int j = 0; j < CC; ++j) red[qtr][j][pl] = o[j];
    __syncthreads();
    if (!valid) return;
#pragma unroll
    for (int j = 0; j < CC; ++j) o[j] = p.end_b[j] + red[0][j][pl] + red[1][j][pl] + red[2][j][pl] + red[3][j][pl];
  } else {
    if (!valid) return;
#pragma unroll
    for (int j = 0; j < CC; ++j) o[j] = p.end_b[j];
    for (int q = 0; q < 4; ++q) {
      float acc[CC];
      quarter(q, acc);
#pragma unroll
      for (int j = 0; j < CC; ++j) o[j] += acc[j];
    }
  }
  float a[CC];
#pragma unroll
  for (int j = 0; j < CC; ++j) a[j] = p.aud_in[((size_t)b * 8 + j) * p.La + pos];
  {
    const int tr = p.swap ? 0 : H;   // offset of the transformed half; the other half conditioned the WN
#pragma unroll
    for (int j = 0; j < H; ++j) a[tr + j] = (a[tr + j] - o[j]) / expf(o[H + j]);
  }
  constexpr int CN = EARLY ? CC + 2 : CC;
  float y[CN];
  if (EARLY) {
#pragma unroll
    for (int j = 0; j < 2; ++j) y[j] = p.sigma * p.z_early[((size_t)b * 2 + j) * p.L + pos];
  }
#pragma unroll
  for (int i = 0; i < CC; ++i) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < CC; ++j) v = fmaf(p.winv[i * CC + j], a[j], v);
    y[(EARLY ? 2 : 0) + i] = v;
  }
  if (p.final_flow) {
    // glow.py:292: [B, 8, L] -> permute -> [B, 8L]: sample n = 8*pos + channel
    if (qtr == 0) {
      float* dst = p.final_audio + (size_t)b * p.T * p.hop8 * 8 + (size_t)pos * CN;
#pragma unroll
      for (int j = 0; j < CN; ++j) dst[j] = y[j];
    }
  } else {
    if (qtr == 0) {
#pragma unroll
      for (int j = 0; j < CN; ++j) p.aud_out[((size_t)b * 8 + j) * p.La + pos] = y[j];
    }
    start_conv<CN / 2>(p, b, h_off, y + (p.swap_next ? CN / 2 : 0), qtr * CQ, CQ);
    if (p.folded && qtr == 0) write_xa<CN / 2>(p, b, h_off, y + (p.swap_next ? CN / 2 : 0));
  }
}


// k_flow_end4: the throughput shape of k_flow_end on the phase-major layout -- FOUR consecutive frames of one phase
// per thread, so the 256 skip rows are read and the 256 start-conv rows written as 16-byte accesses (a wave covers
// 1 KiB of a row per instruction instead of 256 B) and four independent FMA chains run per thread.  The arithmetic per
// position is exactly k_flow_end's (four 64-channel chains in channel order, then bias + q0 + q1 + q2 + q3; the same
// fmaf sequences for the 1x1 products), so an utterance gets the same bits from either kernel.
template <int H, bool EARLY>
__global__ __launch_bounds__(256) void k_flow_end4(EdgeArgs p) {
  constexpr int CC = 2 * H, CN = EARLY ? CC + 2 : CC, HN = CN / 2;
  const int b = blockIdx.y, ph = blockIdx.z, x0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  const int Tb = p.t_valid ? p.t_valid[b] : p.T;
  if (x0 >= Tb) return;
  const int nv = min(4, Tb - x0);                       // live frames among this thread's four
  const int h_off = ph * p.Tqp + HQ + x0, sk_off = ph * p.Tr + x0;
  const float* sk = p.skip + (size_t)b * C * p.Lr + sk_off;
  float o[4][CC];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int j = 0; j < CC; ++j) o[e][j] = p.end_b[j];
  if (p.folded) {
#pragma unroll
    for (int j = 0; j < CC; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(p.skip + ((size_t)b * 8 + j) * p.Lr + sk_off);
      o[0][j] = v.x; o[1][j] = v.y; o[2][j] = v.z; o[3][j] = v.w;
    }
  }
  for (int q = 0; q < (p.folded ? 0 : 4); ++q) {
    float acc[4][CC];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < CC; ++j) acc[e][j] = 0.0f;
    for (int c0 = q * 64; c0 < q * 64 + 64; c0 += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(sk + (size_t)(c0 + u) * p.Lr);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < CC; ++j) {
          const float wv = p.end_w[j * C + c0 + u];
          acc[0][j] = fmaf(wv, v[u].x, acc[0][j]); acc[1][j] = fmaf(wv, v[u].y, acc[1][j]);
          acc[2][j] = fmaf(wv, v[u].z, acc[2][j]); acc[3][j] = fmaf(wv, v[u].w, acc[3][j]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < CC; ++j) o[e][j] += acc[e][j];
  }
  float y[4][CN];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int pos = (x0 + (e < nv ? e : 0)) * p.P + ph;   // dead frames recompute frame 0 (never stored)
    float a[CC];
#pragma unroll
    for (int j = 0; j < CC; ++j) a[j] = p.aud_in[((size_t)b * 8 + j) * p.La + pos];
    const int tr = p.swap ? 0 : H;
#pragma unroll
    for (int j = 0; j < H; ++j) a[tr + j] = (a[tr + j] - o[e][j]) / expf(o[e][H + j]);
    if (EARLY) {
#pragma unroll
      for (int j = 0; j < 2; ++j) y[e][j] = p.sigma * p.z_early[((size_t)b * 2 + j) * p.L + pos];
    }
#pragma unroll
    for (int i = 0; i < CC; ++i) {
      float v = 0.0f;
#pragma unroll
      for (int j = 0; j < CC; ++j) v = fmaf(p.winv[i * CC + j], a[j], v);
      y[e][(EARLY ? 2 : 0) + i] = v;
    }
    if (e < nv) {
      if (p.final_flow) {
        float* dst = p.final_audio + (size_t)b * p.T * p.hop8 * 8 + (size_t)pos * CN;
#pragma unroll
        for (int j = 0; j < CN; ++j) dst[j] = y[e][j];
      } else {
#pragma unroll
        for (int j = 0; j < CN; ++j) p.aud_out[((size_t)b * 8 + j) * p.La + pos] = y[e][j];
      }
    }
  }
  if (p.final_flow) return;
  // next flow's start conv, four frames per row store
  const int a0 = p.swap_next ? HN : 0;
  float* dst = p.h_out + (size_t)b * C * p.Lp + h_off;
  for (int ch = 0; ch < C; ++ch) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = p.start_b[ch];
#pragma unroll
      for (int j = 0; j < HN; ++j) v[e] = fmaf(p.start_w[ch * HN + j], y[e][a0 + j], v[e]);
    }
    float* d = dst + (size_t)ch * p.Lp;
    if (nv == 4) *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int e = 0; e < nv; ++e) d[e] = v[e];
  }
  if (p.folded) {
    float* xd = p.xa_out + (size_t)b * 8 * p.Lp + h_off;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = j < HN ? y[e][a0 + j] : j == HN ? 1.0f : 0.0f;
      float* d = xd + (size_t)j * p.Lp;
      if (nv == 4) *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
      else for (int e = 0; e < nv; ++e) d[e] = v[e];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Training direction (WaveGlow.forward, glow.py:208-250): audio -> z.  The WN stacks are the same
// k_wn_layer launches; only the flow edges differ:
//   k_fwd_begin      regroup audio [B][N] -> 8 channels (glow.py:224), W_0 mix, start conv of flow 0
//   k_fwd_flow_end   end conv, log_s/b split, a1 = exp(log_s)*a1 + b (glow.py:241-246), then for
//                    the next flow: early-output split (glow.py:230-232), W mix, start conv
// ------------------------------------------------------------------------------------------
struct FwdArgs {
  const float* skip;
  const float* aud_in;
  float* aud_out;
  float* h_out;
  const float* audio;     // [B][N] (k_fwd_begin)
  float* z_out;           // [B][8][L]
  float* log_s_out;       // [B][H][L] of this flow
  const float* end_w;
  const float* end_b;
  const float* w_next;    // [CN][CN] mixing matrix of the next flow (or flow 0)
  const float* start_w;   // next flow's start conv
  const float* start_b;
  int N, hop8, Lp, Lr, L, z_row;   // z_row: first z channel the early / final outputs go to
};

__device__ __forceinline__ void fwd_start(const FwdArgs& p, int b, int pos, const float* a0, int HN) {
  float* dst = p.h_out + (size_t)b * C * p.Lp + HALO + pos;
  for (int ch = 0; ch < C; ++ch) {
    float v = p.start_b[ch];
    for (int j = 0; j < HN; ++j) v = fmaf(p.start_w[ch * HN + j], a0[j], v);
    dst[(size_t)ch * p.Lp] = v;
  }
}

__global__ __launch_bounds__(256) void k_fwd_begin(FwdArgs p) {
  const int pos = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (pos >= p.L) return;
  float a[8], y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = p.audio[(size_t)b * p.N + (size_t)pos * 8 + j];   // unfold(1, 8, 8)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v = fmaf(p.w_next[i * 8 + j], a[j], v);
    y[i] = v;
    p.aud_out[((size_t)b * 8 + i) * p.Lr + pos] = v;
  }
  fwd_start(p, b, pos, y, 4);
}

template <int H, bool EARLY_NEXT, bool LASTFLOW>
__global__ __launch_bounds__(256) void k_fwd_flow_end(FwdArgs p) {
  const int pos = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (pos >= p.L) return;
  constexpr int CC = 2 * H;
  float o[CC];
#pragma unroll
  for (int j = 0; j < CC; ++j) o[j] = p.end_b[j];
  const float* sk = p.skip + (size_t)b * C * p.Lr + pos;
  for (int ch = 0; ch < C; ++ch) {
    const float v = sk[(size_t)ch * p.Lr];
#pragma unroll
    for (int j = 0; j < CC; ++j) o[j] = fmaf(p.end_w[j * C + ch], v, o[j]);
  }
  float a[CC];
#pragma unroll
  for (int j = 0; j < CC; ++j) a[j] = p.aud_in[((size_t)b * 8 + j) * p.Lr + pos];
#pragma unroll
  for (int j = 0; j < H; ++j) {
    a[H + j] = expf(o[H + j]) * a[H + j] + o[j];
    p.log_s_out[((size_t)b * H + j) * p.L + pos] = o[H + j];
  }
  if constexpr (LASTFLOW) {
#pragma unroll
    for (int j = 0; j < CC; ++j) p.z_out[((size_t)b * 8 + p.z_row + j) * p.L + pos] = a[j];
  } else {
    constexpr int CN = EARLY_NEXT ? CC - 2 : CC;
    constexpr int OFF = EARLY_NEXT ? 2 : 0;
    if constexpr (EARLY_NEXT) {
#pragma unroll
      for (int j = 0; j < 2; ++j) p.z_out[((size_t)b * 8 + p.z_row + j) * p.L + pos] = a[j];
    }
    float y[CN > 0 ? CN : 1];
#pragma unroll
    for (int i = 0; i < CN; ++i) {
      float v = 0.0f;
#pragma unroll
      for (int j = 0; j < CN; ++j) v = fmaf(p.w_next[i * CN + j], a[OFF + j], v);
      y[i] = v;
      p.aud_out[((size_t)b * 8 + i) * p.Lr + pos] = v;
    }
    fwd_start(p, b, pos, y, CN / 2);
  }
}

}  // namespace

void wg_launch_noise(float* z, size_t n, uint64_t seed, hipStream_t s) {
  k_noise<<<(unsigned)((n / 4 + 255) / 256 + 1), 256, 0, s>>>(z, n, seed);
}
}  // namespace facppg

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace facppg;


// the fp32 entry points refuse a handle made by facppg_wg_create_f16 (facppg_wg16.hip)
#define WG_REQUIRE_FP32(h, fn)                                                                                    \
  FACPPG_REQUIRE(!(h) || !(h)->w16, FACPPG_EINVAL,                                                               \
                 fn ": the handle holds fp16 images (facppg_wg_create_f16); use facppg_wg_infer_f16, or make it with facppg_wg_create")

extern "C" int facppg_version(void) { return FACPPG_VERSION; }
extern "C" const char* facppg_last_error(void) { return g_err; }

static int wg_check_cfg(const facppg_wg_config* c) {
  FACPPG_REQUIRE(c != nullptr, FACPPG_EINVAL, "config is NULL");
  FACPPG_REQUIRE(c->wn_channels == C && c->wn_kernel_size == 3 && c->n_group == 8 && c->n_mel_channels * c->n_group == NCOND,
                 FACPPG_EUNSUPPORTED,
                 "kernels are built for WN n_channels=256, kernel_size=3, n_group=8, n_mel_channels=80 (got %d, %d, %d, %d)",
                 c->wn_channels, c->wn_kernel_size, c->n_group, c->n_mel_channels);
  FACPPG_REQUIRE(c->wn_layers >= 1 && c->wn_layers <= 8, FACPPG_EUNSUPPORTED, "wn_layers must be 1..8 (dilation <= 128)");
  FACPPG_REQUIRE(c->n_flows >= 1 && c->n_flows <= MAXF, FACPPG_EUNSUPPORTED, "n_flows must be 1..%d", MAXF);
  FACPPG_REQUIRE(c->hop_length > 0 && c->hop_length % c->n_group == 0, FACPPG_EUNSUPPORTED, "hop_length must be a positive multiple of n_group");
  FACPPG_REQUIRE(c->upsample_kernel >= c->hop_length && (c->upsample_kernel + c->hop_length - 1) / c->hop_length <= UP_MAXJ,
                 FACPPG_EUNSUPPORTED, "upsample kernel/hop ratio must be in [1, %d]", UP_MAXJ);
  FACPPG_REQUIRE(c->n_early_size == 2 && c->n_early_every >= 1, FACPPG_EUNSUPPORTED, "n_early_size must be 2");
  int n_half = c->n_group / 2;
  for (int k = 0; k < c->n_flows; ++k) {
    if (k % c->n_early_every == 0 && k > 0) n_half -= c->n_early_size / 2;
    FACPPG_REQUIRE(n_half >= 1, FACPPG_EUNSUPPORTED, "flow %d has no channels left", k);
  }
  return FACPPG_OK;
}

static void wg_flow_channels(const facppg_wg_config* c, int* n_rem, int* n_half, int* early) {
  int h = c->n_group / 2, r = c->n_group;
  for (int k = 0; k < c->n_flows; ++k) {
    early[k] = (k % c->n_early_every == 0 && k > 0);
    if (early[k]) { h -= c->n_early_size / 2; r -= c->n_early_size; }
    n_rem[k] = r; n_half[k] = h;
  }
}

extern "C" size_t facppg_wg_weight_count(const facppg_wg_config* c) {
  if (wg_check_cfg(c) != FACPPG_OK) return 0;
  int n_rem[MAXF], n_half[MAXF], early[MAXF];
  wg_flow_channels(c, n_rem, n_half, early);
  const size_t nm = c->n_mel_channels;
  size_t n = nm * nm * c->upsample_kernel + nm;
  for (int k = 0; k < c->n_flows; ++k) {
    const size_t h = n_half[k], cc = 2 * h;
    n += (size_t)C * h + C;
    for (int i = 0; i < c->wn_layers; ++i) {
      const size_t rs = i < c->wn_layers - 1 ? 2 * C : C;
      n += (size_t)2 * C * C * 3 + 2 * C + (size_t)2 * C * NCOND + 2 * C + rs * C + rs;
    }
    n += cc * C + cc + 2 * cc * cc;
  }
  return n;
}

extern "C" int facppg_wg_create(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats, int device,
                                void* stream_, facppg_wg** out) {
  if (int rc = wg_check_cfg(cfg)) return rc;
  FACPPG_REQUIRE(weights_dev && out, FACPPG_EINVAL, "weights_dev/out is NULL");
  FACPPG_REQUIRE(n_floats == facppg_wg_weight_count(cfg), FACPPG_EINVAL, "weight blob has %zu floats, expected %zu", n_floats,
                 facppg_wg_weight_count(cfg));
  hipStream_t stream = (hipStream_t)stream_;
  FACPPG_HIP_CHECK(hipSetDevice(device));
  facppg_wg* h = new (std::nothrow) facppg_wg();
  FACPPG_REQUIRE(h, FACPPG_EINVAL, "out of host memory");
  h->cfg = *cfg; h->device = device; h->profiling = 0; h->ev_used = 0; h->ev_layers = 1; h->poll_limit = 0; h->n_cu = 0; h->last_tile = h->last_waves = h->last_tiles = 0; h->last_schedule = 0; h->arena = nullptr;
  wg_flow_channels(cfg, h->n_rem, h->n_half, h->early);

  // arena layout (bytes, 256-aligned pieces)
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  const size_t nm = cfg->n_mel_channels;
  const size_t w1_bytes = (size_t)(16 * NG1 + 8) * 64 * sizeof(float4);
  auto w2_bytes = [&](int last) { return (size_t)(4 * (last ? 2 : 4) * NG2 + 8) * 64 * sizeof(float4); };
  struct Off { size_t start_w, start_b, end_w, end_b, winv, wfwd, w1[8], w2[8], b1[8], b2[8], w1pm[8], wcpm[8], b1pm[8], w1_16[8], wc_16[8], w2_16[8],
               we[8], endb, w1f, w1f_16, w2r[8], w2r_16[8], ltab; } fo[MAXF];
  h->P = cfg->hop_length / 8;
  h->nj = (cfg->upsample_kernel + cfg->hop_length - 1) / cfg->hop_length;
  h->kc = h->nj * NMEL;
  h->kcp = round_up(h->kc, KCH);
  const size_t w1pm_bytes = (size_t)(NGH + 8) * 1024 * sizeof(float4);   // + the A ring's look-ahead past the last K group
  const size_t wcpm_bytes = ((size_t)h->P * (h->kcp / 8) + 8) * 1024 * sizeof(float4);   // + RING look-ahead past the last phase
  const size_t o_up_w = take(nm * nm * cfg->upsample_kernel * 4), o_up_b = take(nm * 4);
  for (int k = 0; k < cfg->n_flows; ++k) {
    const size_t hh = h->n_half[k], cc = 2 * hh;
    fo[k].start_w = take(C * hh * 4); fo[k].start_b = take(C * 4);
    for (int i = 0; i < cfg->wn_layers; ++i) {
      const int last = i == cfg->wn_layers - 1;
      fo[k].w1[i] = take(w1_bytes); fo[k].b1[i] = take(2 * C * 4);
      fo[k].w2[i] = take(w2_bytes(last)); fo[k].b2[i] = take(2 * C * 4);
      fo[k].w1pm[i] = take(w1pm_bytes); fo[k].wcpm[i] = take(wcpm_bytes); fo[k].b1pm[i] = take(2 * C * 4);
      fo[k].w1_16[i] = take(w1pm_bytes);                      // same floats, other lane order
      fo[k].wc_16[i] = take(wcpm_bytes);                      // (the +8 groups of look-ahead padding cover 4 16-wide groups)
      fo[k].w2_16[i] = take((size_t)(C / 16 + 4) * (last ? 16 : 32) * 64 * sizeof(float4));   // 16 K groups + 4 of look-ahead
      fo[k].we[i] = take(8 * 64 * 8 * 4);
      fo[k].w2r[i] = last ? 0 : take(w2_bytes(1));
      fo[k].w2r_16[i] = last ? 0 : take((size_t)(C / 16 + 4) * 16 * 64 * sizeof(float4));
    }
    fo[k].endb = take(8 * 4);
    fo[k].ltab = take(8 * sizeof(WnLayerPtrs));
    fo[k].w1f = take((size_t)(8 + 8) * 1024 * sizeof(float4)); fo[k].w1f_16 = take((size_t)(4 + 4) * 2048 * sizeof(float4));   // + look-ahead
    fo[k].end_w = take(cc * C * 4); fo[k].end_b = take(cc * 4); fo[k].winv = take(cc * cc * 4); fo[k].wfwd = take(cc * cc * 4);
  }
  h->arena_bytes = off;
  if (hipMalloc((void**)&h->arena, off) != hipSuccess) {
    set_error("hipMalloc(%zu) for packed weights failed", off);
    delete h;
    return FACPPG_EHIP;
  }
  // scratch for folding the upsampler into the conditioning convs: U, one layer's folded matrices, packed Wc
  const size_t ncol = (size_t)h->P * h->kcp;
  const size_t t_u = 0, t_f = t_u + NCOND * ncol * 4, t_a = t_f + (size_t)2 * C * ncol * 4;
  const size_t t_f0 = t_a + packed_a_float4s(2 * C, NCOND) * sizeof(float4), t_bs = t_f0 + (size_t)2 * C * 64 * 4;
  const size_t tmp_bytes = t_bs + (size_t)8 * C * 4;
  char* tmp = nullptr;
  if (hipMalloc((void**)&tmp, tmp_bytes) != hipSuccess) {
    set_error("hipMalloc(%zu) for weight folding scratch failed", tmp_bytes);
    hipFree(h->arena);
    delete h;
    return FACPPG_EHIP;
  }
  h->wgp = nullptr;
  auto fail = [&](int rc) { wgp_destroy(h); hipFree(tmp); hipFree(h->arena); delete h; return rc; };
  if (int rc = wgp_create(h, h->arena, stream)) return fail(rc);   // the persistent small-launch path's own images (facppg_wgp.hip)
#define WG_TRY(expr)                                                                     \
  do {                                                                                   \
    hipError_t e__ = (expr);                                                             \
    if (e__ != hipSuccess) { set_error("%s failed: %s", #expr, hipGetErrorString(e__)); return fail(FACPPG_EHIP); } \
  } while (0)
  WG_TRY(hipMemsetAsync(h->arena, 0, off, stream));
  auto F = [&](size_t o) { return (float*)(h->arena + o); };
  auto cpy = [&](float* dst, const float* src, size_t n) { return hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, stream); };
  const float* src = weights_dev;
  h->up_w = F(o_up_w); h->up_b = F(o_up_b);
  WG_TRY(cpy(h->up_w, src, nm * nm * cfg->upsample_kernel)); src += nm * nm * cfg->upsample_kernel;
  WG_TRY(cpy(h->up_b, src, nm)); src += nm;
  {
    const size_t n = NCOND * ncol;
    k_fold_u<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(h->up_w, (float*)(tmp + t_u), h->P, h->kcp, h->kc, cfg->hop_length,
                                                             cfg->upsample_kernel);
  }
  for (int k = 0; k < cfg->n_flows; ++k) {
    const size_t hh = h->n_half[k], cc = 2 * hh;
    const float* h_flow_src = src;
    h->start_w[k] = F(fo[k].start_w); h->start_b[k] = F(fo[k].start_b);
    WG_TRY(cpy(h->start_w[k], src, C * hh)); src += C * hh;
    WG_TRY(cpy(h->start_b[k], src, C)); src += C;
    for (int i = 0; i < cfg->wn_layers; ++i) {
      const int last = i == cfg->wn_layers - 1;
      const float* in_w = src; src += (size_t)2 * C * C * 3;
      const float* in_b = src; src += 2 * C;
      const float* cond_w = src; src += (size_t)2 * C * NCOND;
      const float* cond_b = src; src += 2 * C;
      const size_t rs = last ? C : 2 * C;
      const float* rs_w = src; src += rs * C;
      const float* rs_b = src; src += rs;
      h->w1[k][i] = (float4*)(h->arena + fo[k].w1[i]); h->b1[k][i] = F(fo[k].b1[i]);
      h->w2[k][i] = (float4*)(h->arena + fo[k].w2[i]); h->b2[k][i] = F(fo[k].b2[i]);
      const int n1 = 16 * NG1 * 64, n2 = 4 * (last ? 2 : 4) * NG2 * 64;
      k_pack_w1<<<(n1 + 255) / 256, 256, 0, stream>>>(in_w, cond_w, h->w1[k][i]);
      k_pack_w2<<<(n2 + 255) / 256, 256, 0, stream>>>(rs_w, h->w2[k][i], last);
      k_add_bias<<<2, 256, 0, stream>>>(in_b, cond_b, h->b1[k][i], 2 * C);
      WG_TRY(cpy(h->b2[k][i], rs_b, rs));
      // phase-major images: Wf = Wc . U (fp32 MFMA GEMM), then the MFMA A-operand layout per phase
      h->w1pm[k][i] = (float4*)(h->arena + fo[k].w1pm[i]); h->wcpm[k][i] = (float4*)(h->arena + fo[k].wcpm[i]);
      h->b1pm[k][i] = F(fo[k].b1pm[i]);
      k_pack_w1_pm<<<(NGH * 1024 + 255) / 256, 256, 0, stream>>>(in_w, h->w1pm[k][i]);
      if (int rc = pack_a(cond_w, 2 * C, NCOND, 1, (float4*)(tmp + t_a), stream)) return fail(rc);
      GemmArgs ga;
      ga.A = (const float4*)(tmp + t_a); ga.M = 2 * C; ga.Cin = NCOND; ga.X = (const float*)(tmp + t_u); ga.ldx = (int)ncol;
      ga.N = (int)ncol; ga.C = (float*)(tmp + t_f); ga.ldc = (int)ncol;
      if (int rc = gemm_launch(ga, stream)) return fail(rc);
      {
        const size_t n = (size_t)h->P * (h->kcp / 8) * 1024;
        k_pack_cond_pm<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>((const float*)(tmp + t_f), h->wcpm[k][i], h->P, h->kcp);
      }
      k_fold_bias<<<2, 256, 0, stream>>>(in_b, cond_b, cond_w, h->up_b, h->b1pm[k][i]);
      h->w1_16[k][i] = (float4*)(h->arena + fo[k].w1_16[i]); h->wc_16[k][i] = (float4*)(h->arena + fo[k].wc_16[i]);
      h->w2_16[k][i] = (float4*)(h->arena + fo[k].w2_16[i]);
      k_pack_w1_16<<<(3 * C / 16 * 2048 + 255) / 256, 256, 0, stream>>>(in_w, h->w1_16[k][i]);
      {
        const size_t n = (size_t)h->P * (h->kcp / 16) * 2048;
        k_pack_cond_16<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>((const float*)(tmp + t_f), h->wc_16[k][i], h->P, h->kcp);
      }
      k_pack_w2_16<<<((C / 16) * (last ? 16 : 32) * 64 + 255) / 256, 256, 0, stream>>>(rs_w, h->w2_16[k][i], last);
      // folded flow edges: res rows alone (the first 256 rows of a non-last res_skip conv, packed like a last layer's
      // 256 rows); this layer's skip bias for the folded end bias; the first layer's taps through the start conv
      h->w2r[k][i] = last ? nullptr : (float4*)(h->arena + fo[k].w2r[i]);
      h->w2r_16[k][i] = last ? nullptr : (float4*)(h->arena + fo[k].w2r_16[i]);
      if (!last) {
        k_pack_w2<<<(4 * 2 * NG2 * 64 + 255) / 256, 256, 0, stream>>>(rs_w, h->w2r[k][i], 1);
        k_pack_w2_16<<<((C / 16) * 16 * 64 + 255) / 256, 256, 0, stream>>>(rs_w, h->w2r_16[k][i], 1);
      }
      k_copy_rows<<<1, 256, 0, stream>>>(rs_b + (last ? 0 : C), (float*)(tmp + t_bs) + i * C, C);
      if (i == 0) {
        h->w1f[k] = (float4*)(h->arena + fo[k].w1f); h->w1f_16[k] = (float4*)(h->arena + fo[k].w1f_16);
        k_fold_first<<<(2 * C * 64 + 255) / 256, 256, 0, stream>>>(in_w, h->start_w[k], h->start_b[k], (float*)(tmp + t_f0), (int)hh);
        k_pack_cond_pm<<<(8 * 1024 + 255) / 256, 256, 0, stream>>>((const float*)(tmp + t_f0), h->w1f[k], 1, 64);
        k_pack_cond_16<<<(4 * 2048 + 255) / 256, 256, 0, stream>>>((const float*)(tmp + t_f0), h->w1f_16[k], 1, 64);
      }
      {
        WgpLayerSrc ws;
        ws.in_w = in_w; ws.folded = (const float*)(tmp + t_f); ws.rs_w = rs_w; ws.b1pm = h->b1pm[k][i]; ws.b2 = h->b2[k][i];
        ws.f0 = (const float*)(tmp + t_f0);
        if (int rc = wgp_pack_layer(h, k, i, ws, stream)) return fail(rc);
      }
    }
    h->end_w[k] = F(fo[k].end_w); h->end_b[k] = F(fo[k].end_b); h->winv[k] = F(fo[k].winv);
    WG_TRY(cpy(h->end_w[k], src, cc * C)); src += cc * C;
    WG_TRY(cpy(h->end_b[k], src, cc)); src += cc;
    {
      // the skip rows of every layer of this flow seen through the end conv (src has moved past them: walk again)
      const float* q = h_flow_src;
      q += C * hh + C;
      for (int i = 0; i < cfg->wn_layers; ++i) {
        const int last = i == cfg->wn_layers - 1;
        q += (size_t)2 * C * C * 3 + 2 * C + (size_t)2 * C * NCOND + 2 * C;
        const float* rs_w = q; q += (last ? C : 2 * C) * C + (last ? C : 2 * C);
        h->we[k][i] = F(fo[k].we[i]);
        k_fold_end_rows<<<(8 * 64 * 8 + 255) / 256, 256, 0, stream>>>(h->end_w[k], rs_w + (last ? 0 : (size_t)C * C), h->we[k][i], (int)cc);
      }
      h->endb[k] = F(fo[k].endb);
      k_fold_end_bias<<<1, 64, 0, stream>>>(h->end_w[k], h->end_b[k], (const float*)(tmp + t_bs), cfg->wn_layers, h->endb[k], (int)cc);
    }
    WG_TRY(cpy(h->winv[k], src, cc * cc)); src += cc * cc;
    h->wfwd[k] = F(fo[k].wfwd);
    WG_TRY(cpy(h->wfwd[k], src, cc * cc)); src += cc * cc;
  }
  // per-layer operand tables of a flow (32-frame tiles, folded flow edges: k_cond_seed walks them), the poll limit of in-launch waits, the CU count
  for (int k = 0; k < cfg->n_flows; ++k) {
    WnLayerPtrs t[8];
    memset(t, 0, sizeof(t));
    for (int i = 0; i < cfg->wn_layers; ++i) {
      const bool last = i == cfg->wn_layers - 1;
      t[i].w1 = i == 0 ? h->w1f[k] : h->w1pm[k][i]; t[i].wc = h->wcpm[k][i]; t[i].b1 = h->b1pm[k][i];
      t[i].w2 = last ? h->w2[k][i] : h->w2r[k][i]; t[i].b2 = h->b2[k][i]; t[i].we = h->we[k][i];
    }
    h->ltab[k] = (WnLayerPtrs*)(h->arena + fo[k].ltab);
    WG_TRY(hipMemcpyAsync(h->ltab[k], t, sizeof(t), hipMemcpyHostToDevice, stream));
    WG_TRY(hipStreamSynchronize(stream));   // (t is a stack buffer)
  }
  {
    const char* pl = getenv("FACPPG_POLL_LIMIT");
    const double seconds = pl ? strtod(pl, nullptr) : 20.0;
    int khz = 0, ncu = 0;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
    h->poll_limit = seconds > 0 && khz > 0 ? (unsigned long long)(seconds * 1e3 * khz) : 0ull;
    h->n_cu = ncu;
  }
  WG_TRY(hipGetLastError());
  if (int rc = wgp_finish_create(h, stream)) return fail(rc);
  WG_TRY(hipStreamSynchronize(stream));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer<false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer<true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer<false, 2, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer<true, 2, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer8<false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer8<true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer<false, 2, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer<true, 2, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer8<false, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer8<true, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer8<false, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_wn_layer8<true, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<3, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  WG_TRY(hipFuncSetAttribute((const void*)k_cond_seed<4, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipFree(tmp);
#undef WG_TRY
  *out = h;
  return FACPPG_OK;
}

extern "C" void facppg_wg_destroy(facppg_wg* h) {
  if (!h) return;
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  wgp_destroy(h);
  if (h->w16) wg16_destroy(h);
  hipFree(h->arena);
  delete h;
}

namespace {
struct WsLayout {
  int L, Lr, Lp;
  size_t spect, h0, h1, skip, aud0, aud1, z, total;
};
WsLayout ws_layout(const facppg_wg_config& c, int B, int T) {
  WsLayout w;
  w.L = T * (c.hop_length / 8);
  w.Lr = round_up(w.L, TN);
  w.Lp = HALO + w.Lr + HALO;
  size_t off = 0;
  auto take = [&](size_t floats) { size_t o = off; off += (floats * 4 + 255) / 256 * 256; return o; };
  w.h0 = take((size_t)B * C * w.Lp);
  w.h1 = take((size_t)B * C * w.Lp);
  w.spect = take((size_t)B * NCOND * w.Lr);
  w.skip = take((size_t)B * C * w.Lr);
  w.aud0 = take((size_t)B * 8 * w.Lr);
  w.aud1 = take((size_t)B * 8 * w.Lr);
  w.z = take((size_t)B * 8 * w.L + 4);
  w.total = off;
  return w;
}

// phase-major layout (k_wn_layer<PM>): frames are the contiguous axis of every phase row
struct PmLayout {
  int L, La, Tr, Tqp, P;
  size_t h0, h1, xa, sync, skip, melp, aud0, aud1, z, goff, gtab, total;
  int ngroups;   // 4-frame groups a ragged batch can have at most (table entries; a multiple of 32 = one 128-frame tile)
};
PmLayout pm_layout(const facppg_wg_config& c, int B, int T) {
  PmLayout w;
  w.P = c.hop_length / 8;
  w.L = T * w.P;
  w.La = round_up(w.L, TN);
  w.Tr = round_up(T, TN);
  w.Tqp = HQ + w.Tr + HQ;
  size_t off = 0;
  auto take = [&](size_t floats) { size_t o = off; off += (floats * 4 + 255) / 256 * 256; return o; };
  w.h0 = take((size_t)B * C * w.P * w.Tqp);
  w.h1 = take((size_t)B * C * w.P * w.Tqp);
  w.xa = take((size_t)B * 8 * w.P * w.Tqp);     // right behind h0 | h1: one memset zeroes the margins of all three
  w.skip = take((size_t)B * C * w.P * w.Tr);
  w.melp = take((size_t)B * NMEL * w.Tqp);
  w.aud0 = take((size_t)B * 8 * w.La);
  w.aud1 = take((size_t)B * 8 * w.La);
  w.z = take((size_t)B * 8 * w.L + 4);
  w.ngroups = round_up(B * ((T + 3) / 4), 32);
  w.goff = take((size_t)B + 1);
  w.gtab = take((size_t)w.ngroups * 4);
  w.total = off;
  return w;
}
}  // namespace

extern "C" size_t facppg_wg_workspace_bytes(const facppg_wg* h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  if (h->w16) return wg16_workspace_bytes(h, B, T);
  const size_t a = ws_layout(h->cfg, B, T).total, b = pm_layout(h->cfg, B, T).total, c = wgp_workspace_bytes(h, B, T);
  return std::max(a, std::max(b, c));
}

#ifdef FACPPG_WN8_PROF
extern "C" int facppg_debug_wn_prof(unsigned long long* out48, int reset) {
  FACPPG_HIP_CHECK(hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_wn_prof), 48 * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[48];
    memset(z, 0, sizeof(z));
    FACPPG_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_wn_prof), z, sizeof(z)));
  }
  return FACPPG_OK;
}
#endif

// enable: 0 off, 1 the launches of the most recent infer, n > 1 accumulate over the next n infers (the events of n
// infers are created HERE, so that none is created inside a timed region)
extern "C" int facppg_wg_set_profiling(facppg_wg* h, int enable) {
  WG_REQUIRE_FP32(h, "facppg_wg_set_profiling");
  FACPPG_REQUIRE(h && enable >= 0, FACPPG_EINVAL, "handle is NULL or enable < 0");
  h->profiling = enable;
  h->ev_used = 0;
  if (enable > 1) {
    FACPPG_HIP_CHECK(hipSetDevice(h->device));
    const size_t need = (size_t)enable * 2 * h->cfg.n_flows * h->cfg.wn_layers;
    while (h->ev.size() < need) {
      hipEvent_t ev;
      FACPPG_HIP_CHECK(hipEventCreate(&ev));
      h->ev.push_back(ev);
    }
  }
  return FACPPG_OK;
}

extern "C" int facppg_wg_last_layer_ms(facppg_wg* h, float* avg_ms, int* n_launches) {
  WG_REQUIRE_FP32(h, "facppg_wg_last_layer_ms");
  FACPPG_REQUIRE(h && avg_ms && n_launches, FACPPG_EINVAL, "NULL argument");
  double tot = 0;
  for (int i = 0; i + 1 < h->ev_used; i += 2) {
    float ms = 0;
    FACPPG_HIP_CHECK(hipEventSynchronize(h->ev[i + 1]));
    FACPPG_HIP_CHECK(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
    tot += ms;
  }
  *n_launches = h->ev_used / 2 * std::max(1, h->ev_layers);
  *avg_ms = *n_launches ? (float)(tot / *n_launches) : 0.0f;
  return FACPPG_OK;
}

extern "C" int facppg_wg_last_launch_shape(const facppg_wg* h, int* tile_frames, int* waves, int* n_tiles) {
  FACPPG_REQUIRE(h && tile_frames && waves && n_tiles, FACPPG_EINVAL, "NULL argument");
  *tile_frames = h->last_tile; *waves = h->last_waves; *n_tiles = h->last_tiles;
  return FACPPG_OK;
}

extern "C" int facppg_wg_last_layer_schedule(const facppg_wg* h, int* schedule) {
  FACPPG_REQUIRE(h && schedule, FACPPG_EINVAL, "NULL argument");
  *schedule = h->last_schedule;
  return FACPPG_OK;
}

template <int H>
static void launch_flow_end(bool early, bool qs, dim3 grid, hipStream_t s, const EdgeArgs& a) {
  const char* no4 = getenv("FACPPG_FLOW_END_NO4");   // (read per call: the tests flip it)
  if (!qs && a.P > 0 && !no4) {   // phase-major, large launch: four frames per thread
    const dim3 g4((a.T + 1023) / 1024, grid.y, grid.z);
    if (early) k_flow_end4<H, true><<<g4, 256, 0, s>>>(a);
    else k_flow_end4<H, false><<<g4, 256, 0, s>>>(a);
    return;
  }
  if (qs) {
    if (early) k_flow_end<H, true, true><<<grid, 256, 0, s>>>(a);
    else k_flow_end<H, false, true><<<grid, 256, 0, s>>>(a);
  } else {
    if (early) k_flow_end<H, true, false><<<grid, 256, 0, s>>>(a);
    else k_flow_end<H, false, false><<<grid, 256, 0, s>>>(a);
  }
}

template <int HN>
static void launch_begin(dim3 grid, hipStream_t s, const EdgeArgs& a, bool qs = false) {
  if (qs) k_begin<HN, true><<<dim3((a.T + 63) / 64, grid.y, grid.z), 256, 0, s>>>(a);
  else k_begin<HN><<<grid, 256, 0, s>>>(a);
}

// WaveGlow.infer on the phase-major layout (folded conditioning): no spect tensor, no upsample kernel.
// seeds (B = 1): the gate accumulators of every layer start from k_cond_seed's buffer (facppg_wg_cond_seed) for the first
// `seeded_frames` frames; melp_ext is then the caller's zero-margined mel buffer the seeds were formed from
static int wg_infer_pm(facppg_wg* h, const float* mel_dev, const int32_t* T_valid_dev, const float* z_dev, uint64_t seed,
                       float sigma, int B, int T, float* audio_dev, char* ws, hipStream_t s, const float* melp_ext = nullptr,
                       const float4* seeds = nullptr, int seeded_frames = 0, int T_layout = 0, void* const* flow_events = nullptr) {
  const facppg_wg_config& c = h->cfg;
  // ONE short utterance: the persistent launch (facppg_wgp.hip) -- same bits, no kernel boundary per layer
  h->last_schedule = 0;
  if (!seeds && wgp_eligible(h, B, T, T_valid_dev)) return wgp_infer(h, mel_dev, z_dev, seed, sigma, T, audio_dev, ws, s);
  // T_layout >= T: the strides (frames per phase row) of buffers that were laid out before T was known -- the mel buffer and
  // the seeds of a streamed utterance -- while everything that is counted (positions, tiles, noise, samples) follows T itself
  PmLayout w = pm_layout(c, B, T_layout > T ? T_layout : T);
  w.L = T * w.P; w.La = round_up(w.L, TN);
  FACPPG_REQUIRE((double)C * w.P * w.Tqp < 2.0e9, FACPPG_EUNSUPPORTED, "T = %d frames is too long for 32-bit row offsets", T);
  float* hbuf[2] = {(float*)(ws + w.h0), (float*)(ws + w.h1)};
  float* skip = (float*)(ws + w.skip);
  const float* melp = melp_ext ? melp_ext : (const float*)(ws + w.melp);
  float* aud[2] = {(float*)(ws + w.aud0), (float*)(ws + w.aud1)};
  float* zbuf = (float*)(ws + w.z);
  const int nf = c.n_flows;
  // FACPPG_WG_EDGE_FOLD=0 runs the layers without the folded flow edges (512-row res_skip GEMM, 256-channel skip sum)
  const char* fold_env = getenv("FACPPG_WG_EDGE_FOLD");   // (read per call: the tests flip it)
  const bool fold = !fold_env || atoi(fold_env) != 0;
  float* xa = (float*)(ws + w.xa);
  // zero margins of h and xa (the convolution's zero padding) and the frames past each utterance's end
  FACPPG_HIP_CHECK(hipMemsetAsync(ws + w.h0, 0, w.skip - w.h0, s));
  if (!melp_ext) k_mel_pad<<<dim3((w.Tqp + 255) / 256, B * NMEL), 256, 0, s>>>(mel_dev, (float*)(ws + w.melp), T_valid_dev, T, w.Tqp);
  const float* z = z_dev;
  const size_t zn = (size_t)B * 8 * w.L;
  if (!z) {
    k_noise<<<(unsigned)((zn / 4 + 255) / 256 + 1), 256, 0, s>>>(zbuf, zn, seed);
    z = zbuf;
  }
  EdgeArgs e;
  memset(&e, 0, sizeof(e));
  e.skip = skip; e.t_valid = T_valid_dev; e.sigma = sigma; e.T = T; e.hop8 = w.P; e.Lp = w.P * w.Tqp; e.Lr = w.P * w.Tr; e.L = w.L;
  e.La = w.La; e.P = w.P; e.Tr = w.Tr; e.Tqp = w.Tqp;
  e.final_audio = audio_dev;
  e.folded = fold; e.xa_out = xa;
  const dim3 egrid((T + 255) / 256, B, w.P);
  const bool fqs = (long)B * w.L < 65536;   // k_flow_end: split channels over the waves when positions are few
  const dim3 fgrid(fqs ? (T + 63) / 64 : (T + 255) / 256, B, w.P);
  int ai = 0, hi = 0;
  {
    const int k = nf - 1;
    e.z0 = z; e.aud_out = aud[ai]; e.h_out = hbuf[hi]; e.start_w = h->start_w[k]; e.start_b = h->start_b[k];
    e.swap_next = c.alternate_halves && (k & 1);
    switch (h->n_half[k]) {
      case 1: launch_begin<1>(egrid, s, e, fqs); break;
      case 2: launch_begin<2>(egrid, s, e, fqs); break;
      case 3: launch_begin<3>(egrid, s, e, fqs); break;
      case 4: launch_begin<4>(egrid, s, e, fqs); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
  }
  size_t z_off = (size_t)B * h->n_rem[nf - 1] * w.L;
  if (h->profiling <= 1) h->ev_used = 0;   // (> 1: the launches of several infers accumulate, facppg_wg_set_profiling)
  if (h->profiling) {
    const size_t need = (size_t)h->ev_used + (size_t)2 * nf * c.wn_layers;
    while (h->ev.size() < need) {
      hipEvent_t ev;
      FACPPG_HIP_CHECK(hipEventCreate(&ev));
      h->ev.push_back(ev);
    }
  }
  // Tile width.  A launch runs in rounds of 512 workgroup slots (2 per CU); measured per-round times in microseconds for
  // a full round / a round that leaves every CU at most one workgroup: 64-frame tiles (4 waves, k_wn_layer) 331 / 185,
  // 32-frame tiles (8 waves, k_wn_layer8) 181 / 94, 16-frame tiles (k_wn_layer16) FACPPG_COST16_*.  Pick the cheapest.
  // 128-frame tiles (k_wn_layer8<NCB = 4>, one workgroup per CU, half the weight loads per MFMA) measure the same as the
  // 64-frame tiles on large launches and are never picked by cost.  FACPPG_WN_TILE = 16 | 32 | 64 | 128 forces a width
  // (tests / tuning; read per call): every width accumulates in the same K order, so a tile gets the same bits from any.
  auto launch_cost = [](long tiles, int full, int half) {
    const long rem = tiles % 512;
    return (tiles / 512) * full + (rem == 0 ? 0 : rem <= 256 ? half : full);
  };
  const bool uniform = !T_valid_dev && T % 4 == 0;
  const long cols = (long)B * T;
  const long tiles_w = uniform ? (long)w.P * ((cols + 63) / 64) : (long)w.P * B * ((T + 63) / 64);
  const long tiles_n = uniform ? (long)w.P * ((cols + 31) / 32) : (long)w.P * B * ((T + 31) / 32);
  const long tiles_16 = (long)w.P * B * ((T + 15) / 16);
  const long cost_w = launch_cost(tiles_w, 331, 185), cost_n = launch_cost(tiles_n, 181, 94);
  const long cost_16 = launch_cost(tiles_16, FACPPG_COST16_FULL, FACPPG_COST16_HALF);
  int tn = cost_16 < cost_w && cost_16 < cost_n ? TN16 : cost_n < cost_w ? 32 : TN;
  if (const char* tile_env = getenv("FACPPG_WN_TILE")) {
    const int v = atoi(tile_env);
    FACPPG_REQUIRE(v == 16 || v == 32 || v == 64 || (v == 128 && fold), FACPPG_EINVAL,
                   "FACPPG_WN_TILE=%s: expected 16, 32, 64 or (with folded flow edges) 128", tile_env);
    tn = v;
  }
  if (seeds) {
    FACPPG_REQUIRE(B == 1 && !T_valid_dev && fold, FACPPG_EUNSUPPORTED, "seeded inference: one utterance, folded flow edges");
    FACPPG_REQUIRE(seeded_frames % 32 == 0 && seeded_frames > 0, FACPPG_EUNSUPPORTED,
                   "seeded inference: %d seeded frames, expected a positive multiple of 32", seeded_frames);
    tn = 32;   // the seeds are 32-frame tiles of k_wn_layer8's accumulators
  }
  // frames behind the seeded ones run as unseeded 16-frame tiles of the same launches (k_wn_layer_mixed)
  const int n32 = seeds && seeded_frames < T ? seeded_frames / 32 : 0;
  const int n16 = n32 ? (T - seeded_frames + TN16 - 1) / TN16 : 0;
  const bool tile16 = tn == TN16, narrow = tn == 32, wide128 = tn == 128;
  WnArgs a;
  memset(&a, 0, sizeof(a));
  a.melp = melp; a.skip = skip; a.t_valid = T_valid_dev; a.T = T; a.hop8 = w.P; a.Lp = w.P * w.Tqp; a.Lr = w.P * w.Tr;
  a.P = w.P; a.Tr = w.Tr; a.Tqp = w.Tqp; a.ntq = (T + tn - 1) / tn; a.nt = a.ntq * B;
  // uniform batch: cut tiles from the B*T frames of a phase laid end to end, so only the very last tile is ragged
  const char* no_flat = getenv("FACPPG_WN_NO_FLAT");   // tests: per-utterance tiles instead of the flat / group-table cut
  if (!T_valid_dev && T % 4 == 0 && !no_flat && !tile16) { a.flat_cols = B * T; a.nt = (B * T + tn - 1) / tn; }
  if (T_valid_dev && B > 1 && !no_flat && !tile16) {
    // ragged batch: the group table maps every lane's 4 frames to (utterance, frame); tiles past the end exit at once
    int* goff = (int*)(ws + w.goff);
    int4* gtab = (int4*)(ws + w.gtab);
    k_group_offsets<<<1, 1024, 0, s>>>(T_valid_dev, B, goff);
    k_group_table<<<(w.ngroups + 255) / 256, 256, 0, s>>>(T_valid_dev, goff, B, gtab, w.ngroups);
    a.groups = gtab; a.nt = w.ngroups * 4 / tn;
  }
  a.ngc = h->kcp / 8; a.kc = h->kc; a.hop = c.hop_length; a.ksize = c.upsample_kernel;
  a.xa = xa;
  // workgroup i lands on XCD i % 8: give every XCD its own phases so a phase's weight image lives in one L2
  const char* no_xcd = getenv("FACPPG_WN_NO_XCD_MAP");   // tests: plain phase-major workgroup order
  a.xcd_map = ((w.P % 8 == 0) && !no_xcd) ? 1 : 0;
  if (n32) a.nt = n32 + n16;
  const unsigned lgrid = (unsigned)(w.P * a.nt);
  // 8 waves per tile for launches that cannot give every SIMD two 4-wave tiles (FACPPG_WN_8W: 0 never, 2 always)
  const char* w8env = getenv("FACPPG_WN_8W");
  const int w8mode = seeds ? 1 : w8env ? atoi(w8env) : 1;
  a.seed_nt = w.Tr / 32;
  h->last_tile = tn; h->last_tiles = (int)lgrid;
  h->last_waves = (wide128 || tile16 || (narrow && w8mode != 0) || (!narrow && w8mode == 2)) ? 8 : 4;
  h->ev_layers = c.wn_layers;
  // One short utterance on 16-frame or 8-wave 32-frame tiles (where the edge launch would take k_flow_end's QS shape): the
  // LAST layer's tiles run the inner flow edges themselves (wn_edge_tile).  FACPPG_WG_EDGE_FUSE=0: the separate launches.
  const char* fuse_env = getenv("FACPPG_WG_EDGE_FUSE");   // (read per call: the tests flip it)
  const bool fuse = fold && fqs && B == 1 && (tile16 || (narrow && w8mode != 0)) && (!fuse_env || atoi(fuse_env) != 0);
  // 8-wave 32-frame tiles with folded flow edges run the small-launch schedule (wn_layer8_tile<..., NS>).  FACPPG_WN_SMALL=legacy:
  // the schedule before it.  (Without the folded edges the second GEMM has twice the rows and its operands do not fit in front
  // of the gate: those launches, FACPPG_WG_EDGE_FOLD=0, keep the legacy schedule.)
  const char* small_env = getenv("FACPPG_WN_SMALL");   // (read per call: the tests flip it)
  FACPPG_REQUIRE(!small_env || !*small_env || !strcmp(small_env, "legacy"), FACPPG_EINVAL, "FACPPG_WN_SMALL=%s: expected legacy", small_env);
  const bool ns = !(small_env && *small_env);
  h->last_schedule = narrow && w8mode != 0 ? (ns && fold ? 2 : 1) : 0;
  for (int k = nf - 1; k >= 0; --k) {
    // (streamed utterance: the seeds of this flow come from a pass that may still be running on another stream)
    if (flow_events && flow_events[k]) FACPPG_HIP_CHECK(hipStreamWaitEvent(s, (hipEvent_t)flow_events[k], 0));
    e.aud_in = aud[ai]; e.aud_out = aud[ai ^ 1];
    e.end_w = h->end_w[k]; e.end_b = h->end_b[k]; e.winv = h->winv[k];
    e.final_flow = (k == 0);
    e.swap = c.alternate_halves && (k & 1);
    e.swap_next = c.alternate_halves && k > 0 && ((k - 1) & 1);
    e.z_early = nullptr;
    if (h->early[k]) { e.z_early = z + z_off; z_off += (size_t)B * c.n_early_size * w.L; }
    if (k > 0) { e.start_w = h->start_w[k - 1]; e.start_b = h->start_b[k - 1]; }
    const int cn = 2 * h->n_half[k] + (h->early[k] ? 2 : 0);
    if (k > 0) FACPPG_REQUIRE(cn == 2 * h->n_half[k - 1], FACPPG_EUNSUPPORTED, "flow %d channel mismatch", k);
    else FACPPG_REQUIRE(cn == 8, FACPPG_EUNSUPPORTED, "final flow must yield n_group channels");
    FACPPG_REQUIRE(h->n_half[k] >= 1 && h->n_half[k] <= 4, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    const bool fuse_k = fuse && k > 0;   // the final flow's edge (interleaved audio) stays a launch
    for (int i = 0; i < c.wn_layers; ++i) {
      a.h_in = hbuf[hi]; a.h_out = hbuf[hi ^ 1];
      a.fe_mode = 0;
      if (fuse_k && i == c.wn_layers - 1) {
        a.fe_mode = 2 * h->n_half[k] + (h->early[k] ? 1 : 0);
        a.fe_swap = e.swap; a.fe_swap_next = e.swap_next; a.fe_L = w.L; a.fe_La = w.La; a.fe_sigma = sigma;
        a.fe_aud_in = e.aud_in; a.fe_aud_out = e.aud_out; a.fe_z_early = e.z_early; a.fe_winv = e.winv;
        a.fe_start_w = e.start_w; a.fe_start_b = e.start_b; a.fe_xa_out = xa;
      }
      a.w1 = h->w1pm[k][i]; a.wc = h->wcpm[k][i]; a.b1 = h->b1pm[k][i]; a.w2 = h->w2[k][i]; a.b2 = h->b2[k][i];
      if (tile16) { a.w1 = h->w1_16[k][i]; a.wc = h->wc_16[k][i]; a.w2 = h->w2_16[k][i]; }
      a.dil = 1 << i; a.first = (i == 0);
      const bool last = i == c.wn_layers - 1;
      a.nconv = NCHH;
      if (fold) {
        a.we = h->we[k][i]; a.endb = h->endb[k];
        a.w2 = tile16 ? h->w2r_16[k][i] : h->w2r[k][i];
        if (i == 0) { a.nconv = 1; a.w1 = tile16 ? h->w1f_16[k] : h->w1f[k]; }
      }
      a.nch = a.nconv + h->kcp / KCH;
      if (h->profiling && i == 0) FACPPG_HIP_CHECK(hipEventRecord(h->ev[h->ev_used++], s));   // one pair per flow, see facppg_wg_last_layer_ms
      // folded flow edges need 8 more LDS rows per tile (the end rows; 16-frame tiles: their 8 K-slice partials)
#define WN_LAUNCH(KERNEL_LAST, KERNEL_MID, THREADS, LDS)              \
  do {                                                                 \
    if (last) KERNEL_LAST<<<lgrid, THREADS, LDS, s>>>(a);              \
    else KERNEL_MID<<<lgrid, THREADS, LDS, s>>>(a);                    \
  } while (0)
#define WN_LAUNCH_NS(SEED, LDS)   /* 8-wave 32-frame tiles, folded flow edges: small-launch or legacy schedule */                \
  do {                                                                                                                         \
    if (ns) WN_LAUNCH((k_wn_layer8<true, 1, true, SEED, true>), (k_wn_layer8<false, 1, true, SEED, true>), 512, LDS);         \
    else WN_LAUNCH((k_wn_layer8<true, 1, true, SEED>), (k_wn_layer8<false, 1, true, SEED>), 512, LDS);                        \
  } while (0)
      if (fold) {
        if (wide128) WN_LAUNCH((k_wn_layer8<true, 4, true>), (k_wn_layer8<false, 4, true>), 512, 131072 + 4096);
        else if (tile16) WN_LAUNCH((k_wn_layer16<true, true>), (k_wn_layer16<false, true>), 512, 16384 + 4096);
        else if (narrow) {
          if (seeds) {
            a.seed = seeds + (size_t)(k * c.wn_layers + i) * w.P * a.seed_nt * 8 * 8 * 64;
            if (n32) {
              WnArgs a16 = a;
              a16.w1 = i == 0 ? h->w1f_16[k] : h->w1_16[k][i]; a16.wc = h->wc_16[k][i]; a16.w2 = last ? h->w2_16[k][i] : h->w2r_16[k][i];
              a16.flat_cols = 0; a16.groups = nullptr;
              if (last && ns) k_wn_layer_mixed<true, true><<<lgrid, 512, 32768 + 8 * 1024, s>>>(a, a16, n32);
              else if (last) k_wn_layer_mixed<true, false><<<lgrid, 512, 32768 + 8 * 1024, s>>>(a, a16, n32);
              else if (ns) k_wn_layer_mixed<false, true><<<lgrid, 512, 32768 + 8 * 1024, s>>>(a, a16, n32);
              else k_wn_layer_mixed<false, false><<<lgrid, 512, 32768 + 8 * 1024, s>>>(a, a16, n32);
            } else WN_LAUNCH_NS(true, 32768 + 8 * 1024);
          } else if (w8mode == 0) WN_LAUNCH((k_wn_layer<true, 1, false, true, true>), (k_wn_layer<false, 1, false, true, true>), 256, 32768 + 1024);
          else WN_LAUNCH_NS(false, 32768 + 8 * 1024);   // + the end rows' 8 K-slice partials
        } else if (w8mode == 2) WN_LAUNCH((k_wn_layer8<true, 2, true>), (k_wn_layer8<false, 2, true>), 512, 65536 + 2048);
        else WN_LAUNCH((k_wn_layer<true, 2, false, true, true>), (k_wn_layer<false, 2, false, true, true>), 256, 65536 + 2048);
      } else {
        if (tile16) WN_LAUNCH((k_wn_layer16<true>), (k_wn_layer16<false>), 512, 16384);
        else if (narrow) {
          if (w8mode == 0) WN_LAUNCH((k_wn_layer<true, 1, false, true>), (k_wn_layer<false, 1, false, true>), 256, 32768);
          else WN_LAUNCH((k_wn_layer8<true, 1>), (k_wn_layer8<false, 1>), 512, 32768);
        } else if (w8mode == 2) WN_LAUNCH((k_wn_layer8<true, 2>), (k_wn_layer8<false, 2>), 512, 65536);
        else WN_LAUNCH((k_wn_layer<true, 2, false, true>), (k_wn_layer<false, 2, false, true>), 256, 65536);
      }
#undef WN_LAUNCH_NS
#undef WN_LAUNCH
      if (!last) hi ^= 1;
      if (h->profiling && last) FACPPG_HIP_CHECK(hipEventRecord(h->ev[h->ev_used++], s));
    }
    if (fuse_k) {
      // the last layer's tiles ran the edge and left the next flow's start-conv rows in the buffer they did not read
      hi ^= 1; ai ^= 1;
      continue;
    }
    e.h_out = hbuf[hi];
    switch (h->n_half[k]) {
      case 1: launch_flow_end<1>(h->early[k], fqs, fgrid, s, e); break;
      case 2: launch_flow_end<2>(h->early[k], fqs, fgrid, s, e); break;
      case 3: launch_flow_end<3>(h->early[k], fqs, fgrid, s, e); break;
      case 4: launch_flow_end<4>(h->early[k], fqs, fgrid, s, e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
    ai ^= 1;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_infer(facppg_wg* h, const float* mel_dev, const int32_t* T_valid_dev, const float* z_dev,
                               uint64_t seed, float sigma, int B, int T, float* audio_dev, void* ws_, size_t ws_bytes,
                               void* stream_) {
  WG_REQUIRE_FP32(h, "facppg_wg_infer");
  FACPPG_REQUIRE(h && mel_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && T > 0, FACPPG_EINVAL, "B and T must be positive (got %d, %d)", B, T);
  const facppg_wg_config& c = h->cfg;
  const WsLayout w = ws_layout(c, B, T);
  {
    const size_t need = facppg_wg_workspace_bytes(h, B, T);
    FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, need);
  }
  FACPPG_REQUIRE(B <= 65535, FACPPG_EINVAL, "B too large");
  {
    // total noise channels = n_remaining(last flow) + n_early_size * (#early flows) = n_group
    int tot = h->n_rem[c.n_flows - 1];
    for (int k = 0; k < c.n_flows; ++k) tot += h->early[k] ? c.n_early_size : 0;
    FACPPG_REQUIRE(tot == 8, FACPPG_EUNSUPPORTED, "noise channel count %d != n_group", tot);
  }
  const char* unfolded = getenv("FACPPG_WG_UNFOLDED");   // (read per call: the tests flip it)
  if (!unfolded || atoi(unfolded) == 0)
    return wg_infer_pm(h, mel_dev, T_valid_dev, z_dev, seed, sigma, B, T, audio_dev, (char*)ws_, (hipStream_t)stream_);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  float* hbuf[2] = {(float*)(ws + w.h0), (float*)(ws + w.h1)};
  float* spect = (float*)(ws + w.spect);
  float* skip = (float*)(ws + w.skip);
  float* aud[2] = {(float*)(ws + w.aud0), (float*)(ws + w.aud1)};
  float* zbuf = (float*)(ws + w.z);
  const int hop8 = c.hop_length / 8;
  const int nf = c.n_flows;

  // zero margins of h (the conv zero padding) and everything a ragged tile may read
  FACPPG_HIP_CHECK(hipMemsetAsync(ws + w.h0, 0, (size_t)B * C * w.Lp * 4 * 2, s));
  if (w.Lr != w.L || T_valid_dev) FACPPG_HIP_CHECK(hipMemsetAsync(spect, 0, (size_t)B * NCOND * w.Lr * 4, s));

  const float* z = z_dev;
  const size_t zn = (size_t)B * 8 * w.L;
  if (!z) {
    k_noise<<<(unsigned)((zn / 4 + 255) / 256 + 1), 256, 0, s>>>(zbuf, zn, seed);
    z = zbuf;
  }
  {
    dim3 g((T + UP_QB - 1) / UP_QB, c.n_mel_channels, B);
    const size_t sm = (size_t)c.n_mel_channels * (UP_QB + UP_MAXJ) * 4;
    k_upsample<<<g, 256, sm, s>>>(mel_dev, h->up_w, h->up_b, spect, T_valid_dev, T, c.n_mel_channels, c.hop_length,
                                  c.upsample_kernel, w.Lr, T * c.hop_length);
  }
  EdgeArgs e;
  memset(&e, 0, sizeof(e));
  e.skip = skip; e.t_valid = T_valid_dev; e.sigma = sigma; e.T = T; e.hop8 = hop8; e.Lp = w.Lp; e.Lr = w.Lr; e.L = w.L;
  e.La = w.Lr;
  e.final_audio = audio_dev;
  const dim3 egrid((w.L + 255) / 256, B);
  const bool fqs = (long)B * w.L < 65536;
  const dim3 fgrid(fqs ? (w.L + 63) / 64 : (w.L + 255) / 256, B);
  int ai = 0, hi = 0;  // current audio / h buffer
  {
    const int k = nf - 1;
    e.z0 = z; e.aud_out = aud[ai]; e.h_out = hbuf[hi]; e.start_w = h->start_w[k]; e.start_b = h->start_b[k];
    e.swap_next = c.alternate_halves && (k & 1);
    switch (h->n_half[k]) {
      case 1: k_begin<1><<<egrid, 256, 0, s>>>(e); break;
      case 2: k_begin<2><<<egrid, 256, 0, s>>>(e); break;
      case 3: k_begin<3><<<egrid, 256, 0, s>>>(e); break;
      case 4: k_begin<4><<<egrid, 256, 0, s>>>(e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
  }
  size_t z_off = (size_t)B * h->n_rem[nf - 1] * w.L;
  if (h->profiling <= 1) h->ev_used = 0;   // (> 1: the launches of several infers accumulate, facppg_wg_set_profiling)
  if (h->profiling) {
    const size_t need = (size_t)h->ev_used + (size_t)2 * nf * c.wn_layers;
    while (h->ev.size() < need) {
      hipEvent_t ev;
      FACPPG_HIP_CHECK(hipEventCreate(&ev));
      h->ev.push_back(ev);
    }
  }
  // tile width: 64 positions per workgroup for throughput; 32 when the launch would not fill
  // the chip's 512 workgroup slots 1.5 times (single short utterances), halving the per-layer latency
  const bool narrow = (long)(w.Lr / TN) * B < 768;
  const dim3 lgrid(narrow ? w.Lr / 32 : w.Lr / TN, B);
  h->last_tile = narrow ? 32 : TN; h->last_waves = 4; h->last_tiles = (int)(lgrid.x * lgrid.y); h->last_schedule = 0;
  h->ev_layers = c.wn_layers;
  for (int k = nf - 1; k >= 0; --k) {
    for (int i = 0; i < c.wn_layers; ++i) {
      WnArgs a;
      a.h_in = hbuf[hi]; a.h_out = hbuf[hi ^ 1]; a.spect = spect; a.skip = skip;
      a.w1 = h->w1[k][i]; a.b1 = h->b1[k][i]; a.w2 = h->w2[k][i]; a.b2 = h->b2[k][i];
      a.t_valid = T_valid_dev; a.T = T; a.hop8 = hop8; a.Lp = w.Lp; a.Lr = w.Lr; a.dil = 1 << i; a.first = (i == 0);
      a.save_ts = nullptr;
      const bool last = i == c.wn_layers - 1;
      if (h->profiling && i == 0) FACPPG_HIP_CHECK(hipEventRecord(h->ev[h->ev_used++], s));
      if (narrow) {
        if (last) k_wn_layer<true, 1><<<lgrid, 256, 32768, s>>>(a);
        else k_wn_layer<false, 1><<<lgrid, 256, 32768, s>>>(a);
      } else {
        static const int lds_bytes = getenv("FACPPG_WN_LDS") ? atoi(getenv("FACPPG_WN_LDS")) : 65536;   // tuning knob: > 80 KiB forces 1 workgroup/CU
        if (last) k_wn_layer<true, 2><<<lgrid, 256, lds_bytes, s>>>(a);
        else k_wn_layer<false, 2><<<lgrid, 256, lds_bytes, s>>>(a);
      }
      if (!last) hi ^= 1;
      if (h->profiling && last) FACPPG_HIP_CHECK(hipEventRecord(h->ev[h->ev_used++], s));
    }
    e.aud_in = aud[ai]; e.aud_out = aud[ai ^ 1]; e.h_out = hbuf[hi];
    e.end_w = h->end_w[k]; e.end_b = h->end_b[k]; e.winv = h->winv[k];
    e.final_flow = (k == 0);
    e.swap = c.alternate_halves && (k & 1);
    e.swap_next = c.alternate_halves && k > 0 && ((k - 1) & 1);
    e.z_early = nullptr;
    if (h->early[k]) { e.z_early = z + z_off; z_off += (size_t)B * c.n_early_size * w.L; }
    if (k > 0) { e.start_w = h->start_w[k - 1]; e.start_b = h->start_b[k - 1]; }
    const int cn = 2 * h->n_half[k] + (h->early[k] ? 2 : 0);
    if (k > 0) FACPPG_REQUIRE(cn == 2 * h->n_half[k - 1], FACPPG_EUNSUPPORTED, "flow %d channel mismatch", k);
    else FACPPG_REQUIRE(cn == 8, FACPPG_EUNSUPPORTED, "final flow must yield n_group channels");
    switch (h->n_half[k]) {
      case 1: launch_flow_end<1>(h->early[k], fqs, fgrid, s, e); break;
      case 2: launch_flow_end<2>(h->early[k], fqs, fgrid, s, e); break;
      case 3: launch_flow_end<3>(h->early[k], fqs, fgrid, s, e); break;
      case 4: launch_flow_end<4>(h->early[k], fqs, fgrid, s, e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
    ai ^= 1;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_seed_layout(const facppg_wg* h, int T, int* Tqp, int* margin, size_t* seed_bytes) {
  WG_REQUIRE_FP32(h, "facppg_wg_seed_layout");
  FACPPG_REQUIRE(h && T > 0 && Tqp && margin && seed_bytes, FACPPG_EINVAL, "NULL argument or T <= 0");
  const PmLayout w = pm_layout(h->cfg, 1, T);
  *Tqp = w.Tqp; *margin = HQ;
  *seed_bytes = (size_t)h->cfg.n_flows * h->cfg.wn_layers * w.P * (w.Tr / 32) * 8 * 8 * 64 * sizeof(float4);
  return FACPPG_OK;
}

extern "C" int facppg_wg_cond_seed(facppg_wg* h, const float* melp_dev, int T, int frame0, int nframes, int block_tiles,
                                   int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                                   const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream_) {
  WG_REQUIRE_FP32(h, "facppg_wg_cond_seed");
  FACPPG_REQUIRE(h && melp_dev && seeds_dev, FACPPG_EINVAL, "NULL argument");
  const facppg_wg_config& c = h->cfg;
  const PmLayout w = pm_layout(c, 1, T);
  size_t need = 0; int tqp = 0, mg = 0;
  facppg_wg_seed_layout(h, T, &tqp, &mg, &need);
  FACPPG_REQUIRE(seed_bytes >= need, FACPPG_EWORKSPACE, "seed buffer has %zu bytes, need %zu", seed_bytes, need);
  FACPPG_REQUIRE(frame0 >= 0 && frame0 % 32 == 0 && nframes > 0 && frame0 + nframes <= w.Tr, FACPPG_EINVAL,
                 "frames [%d, %d): the first must be a multiple of 32 and the range inside the %d padded frames", frame0, frame0 + nframes, w.Tr);
  FACPPG_REQUIRE(block_tiles >= 1 && block_tiles <= 4 && layers_per_workgroup >= 1, FACPPG_EINVAL, "block_tiles in 1..4, layers_per_workgroup >= 1");
  if (nflows <= 0) { flow0 = 0; nflows = c.n_flows; }
  FACPPG_REQUIRE(flow0 >= 0 && flow0 + nflows <= c.n_flows, FACPPG_EINVAL, "flows [%d, %d) of %d", flow0, flow0 + nflows, c.n_flows);
  SeedArgs a;
  memset(&a, 0, sizeof(a));
  a.melp = melp_dev; a.seeds = (float4*)seeds_dev; a.skip = skip_dev;
  for (int k = 0; k < c.n_flows; ++k) a.ltab[k] = h->ltab[k];
  a.layers_total = c.n_flows * c.wn_layers; a.wn_layers = c.wn_layers; a.lpw = layers_per_workgroup;
  a.P = w.P; a.Tqp = w.Tqp; a.seed_nt = w.Tr / 32;
  const int ntiles = (nframes + 31) / 32;
  a.tile0 = frame0 / 32; a.nblk = (ntiles + block_tiles - 1) / block_tiles;
  a.ncmax = h->kcp / KCH; a.kc = h->kc; a.ngc = h->kcp / 8; a.hop = c.hop_length; a.ksize = c.upsample_kernel;
  size_t lds = (size_t)a.ncmax * KCH * 32 * block_tiles * sizeof(float);
  FACPPG_REQUIRE(lds <= 160 * 1024, FACPPG_EUNSUPPORTED, "block_tiles = %d needs %zu bytes of LDS", block_tiles, lds);
  // A BOUNDED launch (max_workgroups > 0: the caller shares the GPU with other streams) asks for a CU's whole LDS per workgroup:
  // one workgroup per CU and nothing else next to it.  Measured (tools/postnet_under_seed_probe.py): the dispatcher places another
  // stream's small workgroups on the CUs a pass already runs on, where they share its LDS bandwidth and matrix pipe -- a chain of
  // ten 15 us launches took 0.4-0.7 ms next to a pass of 16-344 workgroups, 0.20-0.22 ms when the pass's workgroups own their CUs
  // (0.15 alone); a 32-frame pass is HBM-bound and no slower with one workgroup per CU than with two.  FACPPG_SEED_LDS (KiB)
  // overrides (0: what the kernel needs).
  {
    const char* le = getenv("FACPPG_SEED_LDS");
    const size_t want = le ? (size_t)atoi(le) * 1024 : (max_workgroups > 0 ? (size_t)160 * 1024 : 0);
    lds = std::max(lds, std::min((size_t)160 * 1024, want));
  }
  a.layer0 = flow0 * c.wn_layers; a.layer1 = (flow0 + nflows) * c.wn_layers;
  const int lgroups = (a.layer1 - a.layer0 + a.lpw - 1) / a.lpw;
  a.items = lgroups * w.P * a.nblk;
  // FACPPG_SEED_WGS bounds the workgroups of a launch (a multiple of 8; 0 = one per item): the kernel streams 2 GB of weight images
  // per pass, and next to a latency-bound decoder a slower stream can be the better neighbour.  FACPPG_SEED_NT=0: ordinary
  // (L2-allocating) loads and stores instead of non-temporal ones.  Both read per call: experiments.
  const char* wgs_env = getenv("FACPPG_SEED_WGS");
  const int max_wgs = (wgs_env ? atoi(wgs_env) : max_workgroups) / 8 * 8;
  a.counter = max_wgs > 0 && max_wgs < a.items ? counter_dev : nullptr;   // (a caller-zeroed word; without one the items are strided)
  const unsigned grid = (unsigned)(max_wgs > 0 && max_wgs < a.items ? max_wgs : a.items);
  const char* nt_env = getenv("FACPPG_SEED_NT");
  const bool nt = !nt_env || atoi(nt_env) != 0;
  hipStream_t s = (hipStream_t)stream_;
#define SEED_LAUNCH(N)                                         \
  do {                                                         \
    if (nt) k_cond_seed<N, true><<<grid, 512, lds, s>>>(a);    \
    else k_cond_seed<N, false><<<grid, 512, lds, s>>>(a);      \
  } while (0)
  switch (block_tiles) {
    case 1: SEED_LAUNCH(1); break;
    case 2: SEED_LAUNCH(2); break;
    case 3: SEED_LAUNCH(3); break;
    default: SEED_LAUNCH(4); break;
  }
#undef SEED_LAUNCH
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_mel_pad(const facppg_wg* h, const float* mel_dev, int T, int ld, float* melp_dev, void* stream_) {
  WG_REQUIRE_FP32(h, "facppg_wg_mel_pad");
  FACPPG_REQUIRE(h && mel_dev && melp_dev && T > 0 && ld >= T, FACPPG_EINVAL, "NULL argument or bad T / ld");
  const PmLayout w = pm_layout(h->cfg, 1, T);
  FACPPG_HIP_CHECK(hipMemsetAsync(melp_dev, 0, (size_t)NMEL * w.Tqp * 4, (hipStream_t)stream_));
  FACPPG_HIP_CHECK(hipMemcpy2DAsync(melp_dev + HQ, (size_t)w.Tqp * 4, mel_dev, (size_t)ld * 4, (size_t)T * 4, NMEL, hipMemcpyDeviceToDevice,
                                    (hipStream_t)stream_));
  return FACPPG_OK;
}

extern "C" int facppg_wg_infer_seeded(facppg_wg* h, const float* melp_dev, int T_layout, int T, const float* seeds_dev, int seeded_frames,
                                      const float* z_dev, uint64_t seed, float sigma, float* audio_dev, void* ws_, size_t ws_bytes,
                                      void* const* flow_events, void* stream_) {
  WG_REQUIRE_FP32(h, "facppg_wg_infer_seeded");
  FACPPG_REQUIRE(h && melp_dev && seeds_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0 && T_layout >= T, FACPPG_EINVAL, "need 0 < T <= T_layout (got %d, %d)", T, T_layout);
  const size_t need = facppg_wg_workspace_bytes(h, 1, T_layout);
  FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, need);
  return wg_infer_pm(h, nullptr, nullptr, z_dev, seed, sigma, 1, T, audio_dev, (char*)ws_, (hipStream_t)stream_, melp_dev,
                     (const float4*)seeds_dev, seeded_frames, T_layout, flow_events);
}

extern "C" int facppg_wg_draw_noise(const facppg_wg* h, const uint64_t* seeds_dev, int B, int T, float* z_dev, void* stream_) {
  FACPPG_REQUIRE(h && seeds_dev && z_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && T > 0 && B <= 65535, FACPPG_EINVAL, "bad B/T");
  const facppg_wg_config& c = h->cfg;
  const int nf = c.n_flows, L = T * (c.hop_length / c.n_group);
  int n_seg = 1;
  for (int k = 0; k < nf; ++k) n_seg += h->early[k] ? 1 : 0;
  k_noise_utt<<<dim3((L / 4 + 256) / 256, B), 256, 0, (hipStream_t)stream_>>>(z_dev, seeds_dev, B, L, h->n_rem[nf - 1], c.n_early_size, n_seg);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

template <int H>
static void launch_fwd_end(bool early_next, bool lastflow, dim3 grid, hipStream_t s, const FwdArgs& a) {
  if (lastflow) k_fwd_flow_end<H, false, true><<<grid, 256, 0, s>>>(a);
  else if (early_next) k_fwd_flow_end<H, true, false><<<grid, 256, 0, s>>>(a);
  else k_fwd_flow_end<H, false, false><<<grid, 256, 0, s>>>(a);
}

extern "C" size_t facppg_wg_log_s_count(const facppg_wg* h, int B, int N) {
  if (h && h->w16) return 0;   // (an fp16 handle has no training direction)
  if (!h || B <= 0 || N <= 0) return 0;
  size_t n = 0;
  for (int k = 0; k < h->cfg.n_flows; ++k) n += (size_t)B * h->n_half[k] * (N / 8);
  return n;
}

extern "C" int facppg_wg_forward(facppg_wg* h, const float* mel_dev, const float* audio_dev, int B, int F, int N, float* z_dev,
                                 float* log_s_dev, void* ws_, size_t ws_bytes, void* stream_) {
  WG_REQUIRE_FP32(h, "facppg_wg_forward");
  FACPPG_REQUIRE(h && mel_dev && audio_dev && z_dev && log_s_dev && ws_, FACPPG_EINVAL, "NULL argument");
  const facppg_wg_config& c = h->cfg;
  FACPPG_REQUIRE(B > 0 && F > 0 && N > 0 && N % 8 == 0, FACPPG_EINVAL, "need B, F > 0 and N a positive multiple of n_group");
  FACPPG_REQUIRE((F - 1) * c.hop_length + c.upsample_kernel >= N, FACPPG_EINVAL,
                 "upsampled mel (%d frames) is shorter than the audio (%d samples)  (glow.py:216)", F, N);
  FACPPG_REQUIRE(h->n_half[0] == 4, FACPPG_EUNSUPPORTED, "forward expects n_group = 8");
  FACPPG_REQUIRE(!c.alternate_halves, FACPPG_EUNSUPPORTED, "the legacy alternating-halves layout has no training direction (glow_old.py:150-151 returns None)");
  // workspace: same layout as infer for T' frames covering N samples
  const int Tq = (N + c.hop_length - 1) / c.hop_length;
  WsLayout w = ws_layout(c, B, Tq);
  const int L = N / 8;
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu (facppg_wg_workspace_bytes(B, ceil(N/hop)))",
                 ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  float* hbuf[2] = {(float*)(ws + w.h0), (float*)(ws + w.h1)};
  float* spect = (float*)(ws + w.spect);
  float* skip = (float*)(ws + w.skip);
  float* aud[2] = {(float*)(ws + w.aud0), (float*)(ws + w.aud1)};
  const int hop8 = c.hop_length / 8, nf = c.n_flows;
  FACPPG_HIP_CHECK(hipMemsetAsync(ws + w.h0, 0, (size_t)B * C * w.Lp * 4 * 2, s));
  FACPPG_HIP_CHECK(hipMemsetAsync(spect, 0, (size_t)B * NCOND * w.Lr * 4, s));
  {
    // spect = upsample(mel)[:, :, :N] regrouped (glow.py:214-222); mel frames beyond those that reach n < N add nothing
    dim3 g((F + UP_QB - 1) / UP_QB, c.n_mel_channels, B);
    const size_t sm = (size_t)c.n_mel_channels * (UP_QB + UP_MAXJ) * 4;
    // frames q >= Tq would write positions >= N: they are cut by n_limit; frames < F contribute via their taps
    k_upsample<<<g, 256, sm, s>>>(mel_dev, h->up_w, h->up_b, spect, nullptr, F, c.n_mel_channels, c.hop_length,
                                  c.upsample_kernel, w.Lr, N);
  }
  FwdArgs a;
  memset(&a, 0, sizeof(a));
  a.skip = skip; a.audio = audio_dev; a.z_out = z_dev; a.N = N; a.hop8 = hop8; a.Lp = w.Lp; a.Lr = w.Lr; a.L = L;
  const dim3 egrid((L + 255) / 256, B);
  int ai = 0, hi = 0;
  a.aud_out = aud[ai]; a.h_out = hbuf[hi]; a.w_next = h->wfwd[0]; a.start_w = h->start_w[0]; a.start_b = h->start_b[0];
  k_fwd_begin<<<egrid, 256, 0, s>>>(a);
  // layers see T = Tq frames; positions >= L are masked through t_valid-free Lb = Tq*hop8 >= L: use exact L via T/hop8
  const bool narrow = (long)(w.Lr / TN) * B < 768;
  const dim3 lgrid(narrow ? w.Lr / 32 : w.Lr / TN, B);
  size_t ls_off = 0;
  int z_row = 0;
  for (int k = 0; k < nf; ++k) {
    for (int i = 0; i < c.wn_layers; ++i) {
      WnArgs la;
      la.h_in = hbuf[hi]; la.h_out = hbuf[hi ^ 1]; la.spect = spect; la.skip = skip;
      la.w1 = h->w1[k][i]; la.b1 = h->b1[k][i]; la.w2 = h->w2[k][i]; la.b2 = h->b2[k][i];
      la.t_valid = nullptr; la.T = L; la.hop8 = 1;   // Lb = T * hop8 = L exactly
      la.Lp = w.Lp; la.Lr = w.Lr; la.dil = 1 << i; la.first = (i == 0); la.save_ts = nullptr;
      const bool last = i == c.wn_layers - 1;
      if (narrow) {
        if (last) k_wn_layer<true, 1><<<lgrid, 256, 32768, s>>>(la);
        else k_wn_layer<false, 1><<<lgrid, 256, 32768, s>>>(la);
      } else {
        if (last) k_wn_layer<true, 2><<<lgrid, 256, 65536, s>>>(la);
        else k_wn_layer<false, 2><<<lgrid, 256, 65536, s>>>(la);
      }
      if (!last) hi ^= 1;
    }
    const bool lastflow = k == nf - 1;
    const bool early_next = !lastflow && h->early[k + 1];
    a.aud_in = aud[ai]; a.aud_out = aud[ai ^ 1]; a.h_out = hbuf[hi];
    a.end_w = h->end_w[k]; a.end_b = h->end_b[k];
    a.log_s_out = log_s_dev + ls_off;
    ls_off += (size_t)B * h->n_half[k] * L;
    a.z_row = z_row;
    if (early_next) z_row += 2;
    if (!lastflow) { a.w_next = h->wfwd[k + 1]; a.start_w = h->start_w[k + 1]; a.start_b = h->start_b[k + 1]; }
    switch (h->n_half[k]) {
      case 2: launch_fwd_end<2>(early_next, lastflow, egrid, s, a); break;
      case 3: launch_fwd_end<3>(early_next, lastflow, egrid, s, a); break;
      case 4: launch_fwd_end<4>(early_next, lastflow, egrid, s, a); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
    ai ^= 1;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

// ==========================================================================================
// WN training primitives (WaveGlow training step): the WN stack of ONE flow
// with activations saved, and its backward w.r.t. data.  Weights change every optimiser step and
// are weight-normed on the host side, so these take PLAIN effective weights and pack them per call
// into the caller's workspace.  Weight gradients are plain [M x N].[N x K] matrix products over the
// saved tensors and are left to the caller's BLAS (rocBLAS through torch.matmul).
// ==========================================================================================
namespace {
using namespace facppg;

// The four 1x1 edge convs of a training WN stack.  256 threads = 64 positions x 4 channel quarters (wave q
// owns channels 64q..64q+63), so a 10 000-sample segment still spreads over ~60 workgroups per batch item
// and no thread walks all 256 channels; reductions over channels meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void k_wn_start(const float* __restrict__ a0, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ h0, int nh, int L, int Lp) {
  const int pos = blockIdx.x * 64 + (threadIdx.x & 63), qtr = threadIdx.x >> 6, b = blockIdx.y;
  if (pos >= L) return;
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = j < nh ? a0[((size_t)b * nh + j) * L + pos] : 0.0f;
  float* dst = h0 + (size_t)b * C * Lp + HALO + pos;
  for (int ch = qtr * 64; ch < qtr * 64 + 64; ++ch) {
    float v = bias[ch];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nh) v = fmaf(w[ch * nh + j], a[j], v);
    dst[(size_t)ch * Lp] = v;
  }
}

__global__ __launch_bounds__(256) void k_wn_end(const float* __restrict__ skip, const float* __restrict__ w,
                                                const float* __restrict__ bias, float* __restrict__ out, int nout, int L, int Lr) {
  __shared__ float red[4][8][64];
  const int pl = threadIdx.x & 63, pos = blockIdx.x * 64 + pl, qtr = threadIdx.x >> 6, b = blockIdx.y;
  const bool valid = pos < L;
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.0f;
  if (valid) {
    const float* sk = skip + (size_t)b * C * Lr + pos;
    for (int c0 = qtr * 64; c0 < qtr * 64 + 64; c0 += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = sk[(size_t)(c0 + u) * Lr];
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nout) o[j] = fmaf(w[j * C + c0 + u], v[u], o[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[qtr][j][pl] = o[j];
  __syncthreads();
  if (!valid) return;
  for (int j = qtr; j < nout; j += 4)   // outputs dealt to the four waves
    out[((size_t)b * nout + j) * L + pos] = bias[j] + red[0][j][pl] + red[1][j][pl] + red[2][j][pl] + red[3][j][pl];
}

// dskip[b][ch][pos] = sum_j Wend[j][ch] * dout[b][j][pos]
__global__ __launch_bounds__(256) void k_wn_end_bwd(const float* __restrict__ dout, const float* __restrict__ w,
                                                    float* __restrict__ dskip, int nout, int L, int Lr) {
  const int pos = blockIdx.x * 64 + (threadIdx.x & 63), qtr = threadIdx.x >> 6, b = blockIdx.y;
  if (pos >= L) return;
  float d[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = j < nout ? dout[((size_t)b * nout + j) * L + pos] : 0.0f;
  float* dst = dskip + (size_t)b * C * Lr + pos;
  for (int ch = qtr * 64; ch < qtr * 64 + 64; ++ch) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nout) v = fmaf(w[j * C + ch], d[j], v);
    dst[(size_t)ch * Lr] = v;
  }
}

// da0[b][j][pos] = sum_ch Wstart[ch][j] * dh0[b][ch][pos]
__global__ __launch_bounds__(256) void k_wn_start_bwd(const float* __restrict__ dh0, const float* __restrict__ w,
                                                      float* __restrict__ da0, int nh, int L, int Lr) {
  __shared__ float red[4][8][64];
  const int pl = threadIdx.x & 63, pos = blockIdx.x * 64 + pl, qtr = threadIdx.x >> 6, b = blockIdx.y;
  const bool valid = pos < L;
  float d[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = 0.0f;
  if (valid) {
    const float* src = dh0 + (size_t)b * C * Lr + pos;
    for (int c0 = qtr * 64; c0 < qtr * 64 + 64; c0 += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = src[(size_t)(c0 + u) * Lr];
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nh) d[j] = fmaf(w[(c0 + u) * nh + j], v[u], d[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[qtr][j][pl] = d[j];
  __syncthreads();
  if (!valid) return;
  for (int j = qtr; j < nh; j += 4)
    da0[((size_t)b * nh + j) * L + pos] = red[0][j][pl] + red[1][j][pl] + red[2][j][pl] + red[3][j][pl];
}

struct WnTrainWs {
  size_t w1[8], b1[8], w2[8], total;                     // forward operands
  size_t rs_a[8], rs_b[8], in_t[8], cond_t[8], tmp;      // backward operands ([K][M] transposes) + dacts temp
  size_t splitk, splitk_bytes;                            // split-K partial sums of the small-N backward GEMMs
};
WnTrainWs wn_train_ws(int n_layers, int B, int Lr) {
  WnTrainWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  for (int i = 0; i < n_layers; ++i) {
    w.w1[i] = take((size_t)(16 * NG1 + 8) * 64 * sizeof(float4));
    w.b1[i] = take(2 * C * 4);
    w.w2[i] = take((size_t)(16 * NG2 + 8) * 64 * sizeof(float4));
    w.rs_a[i] = take(packed_a_float4s(C, C) * 16);
    w.rs_b[i] = take(packed_a_float4s(C, C) * 16);
    w.in_t[i] = take(packed_a_float4s(C, 2 * C * 3) * 16);
    w.cond_t[i] = take(packed_a_float4s(NCOND, 2 * C) * 16);
  }
  w.tmp = take((size_t)B * C * Lr * 4);
  w.splitk_bytes = (size_t)8 * B * C * Lr * 4;   // <= 6 splits (K = 1536) of a [256 x L] product per batch item
  w.splitk = take(w.splitk_bytes);
  w.total = off;
  return w;
}
}  // namespace

extern "C" size_t facppg_wn_train_workspace_bytes(int n_layers, int B, int L) {
  if (n_layers < 1 || n_layers > 8 || B <= 0 || L <= 0) return 0;
  return wn_train_ws(n_layers, B, round_up(L, TN)).total;
}

static int wn_check(const facppg_wn_weights* w, int n_in, int n_layers, int B, int L) {
  FACPPG_REQUIRE(w && w->start_w && w->start_b && w->end_w && w->end_b, FACPPG_EINVAL, "NULL weight pointer");
  FACPPG_REQUIRE(n_in >= 1 && n_in <= 4 && n_layers >= 1 && n_layers <= 8 && B > 0 && B <= 65535 && L > 0, FACPPG_EINVAL,
                 "bad n_in/n_layers/B/L");
  for (int i = 0; i < n_layers; ++i)
    FACPPG_REQUIRE(w->in_w[i] && w->in_b[i] && w->cond_w[i] && w->cond_b[i] && w->rs_w[i] && w->rs_b[i], FACPPG_EINVAL,
                   "NULL weight pointer (layer %d)", i);
  return FACPPG_OK;
}

// Replaces: WN.forward (glow.py:154-175) in training, keeping what its backward needs:
//   h_all  [n_layers+1][B][256][Lp]  layer inputs (zero margins = conv padding), Lp = 128 + Lr + 128
//   ts_all [n_layers][B][512][Lr]    tanh / sigmoid halves of each gate
//   skip   [B][256][Lr]              total skip sum (input of the end conv)
// a0 [B][n_in][L], spect_pad [B][640][Lr], out [B][2*n_in][L].  Columns [L, Lr) of spect_pad must be readable and may hold
// anything, NaN included: they are B-operand columns of a tile's GEMMs, a column of the product depends on that column alone,
// and every store is masked to columns < L.  h_all comes back EXACTLY zero outside columns [128, 128 + L) of its first n_layers
// slabs and in the whole of h_all[n_layers] (the memset below; the taps of the next layer and of facppg_wn_weight_grads read
// up to 128 columns either side); columns [L, Lr) of ts_all and skip are not written.  tests/test_gpu_wn_train.py holds all
// of this with NaN-filled buffers.
extern "C" int facppg_wn_forward_save(const facppg_wn_weights* wts, int n_in, int n_layers, const float* a0_dev,
                                      const float* spect_pad_dev, int B, int L, float* out_dev, float* h_all_dev,
                                      float* ts_all_dev, float* skip_dev, void* ws_, size_t ws_bytes, void* stream_) {
  if (int rc = wn_check(wts, n_in, n_layers, B, L)) return rc;
  FACPPG_REQUIRE(a0_dev && spect_pad_dev && out_dev && h_all_dev && ts_all_dev && skip_dev && ws_, FACPPG_EINVAL, "NULL argument");
  const int Lr = round_up(L, TN), Lp = HALO + Lr + HALO;
  const WnTrainWs w = wn_train_ws(n_layers, B, Lr);
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  static bool attr_set = false;
  if (!attr_set) {
    FACPPG_HIP_CHECK(hipFuncSetAttribute((const void*)k_wn_layer<false, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    FACPPG_HIP_CHECK(hipFuncSetAttribute((const void*)k_wn_layer<true, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    attr_set = true;
  }
  const size_t hsz = (size_t)B * C * Lp;
  FACPPG_HIP_CHECK(hipMemsetAsync(h_all_dev, 0, hsz * (n_layers + 1) * 4, s));   // zero margins / tail columns
  for (int i = 0; i < n_layers; ++i) {
    const int last = i == n_layers - 1;
    const int n1 = 16 * NG1 * 64, n2 = 4 * (last ? 2 : 4) * NG2 * 64;
    k_pack_w1<<<(n1 + 255) / 256, 256, 0, s>>>(wts->in_w[i], wts->cond_w[i], (float4*)(ws + w.w1[i]));
    k_pack_w2<<<(n2 + 255) / 256, 256, 0, s>>>(wts->rs_w[i], (float4*)(ws + w.w2[i]), last);
    k_add_bias<<<2, 256, 0, s>>>(wts->in_b[i], wts->cond_b[i], (float*)(ws + w.b1[i]), 2 * C);
  }
  const dim3 egrid((L + 63) / 64, B);   // 64 positions x 4 channel quarters per workgroup
  k_wn_start<<<egrid, 256, 0, s>>>(a0_dev, wts->start_w, wts->start_b, h_all_dev, n_in, L, Lp);
  const bool narrow = (long)(Lr / TN) * B < 768;   // small batches: 32-wide tiles halve the per-layer latency
  const dim3 lgrid(narrow ? Lr / 32 : Lr / TN, B);
  for (int i = 0; i < n_layers; ++i) {
    WnArgs a;
    a.h_in = h_all_dev + hsz * i; a.h_out = h_all_dev + hsz * (i + 1); a.spect = spect_pad_dev; a.skip = skip_dev;
    a.w1 = (const float4*)(ws + w.w1[i]); a.b1 = (const float*)(ws + w.b1[i]); a.w2 = (const float4*)(ws + w.w2[i]);
    a.b2 = wts->rs_b[i]; a.t_valid = nullptr; a.T = L; a.hop8 = 1; a.Lp = Lp; a.Lr = Lr; a.dil = 1 << i; a.first = (i == 0);
    a.save_ts = ts_all_dev + (size_t)B * 2 * C * Lr * i;
    if (narrow) {
      if (i == n_layers - 1) k_wn_layer<true, 1, true><<<lgrid, 256, 32768, s>>>(a);
      else k_wn_layer<false, 1, true><<<lgrid, 256, 32768, s>>>(a);
    } else {
      if (i == n_layers - 1) k_wn_layer<true, 2, true><<<lgrid, 256, 65536, s>>>(a);
      else k_wn_layer<false, 2, true><<<lgrid, 256, 65536, s>>>(a);
    }
  }
  k_wn_end<<<egrid, 256, 0, s>>>(skip_dev, wts->end_w, wts->end_b, out_dev, 2 * n_in, L, Lr);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

// Backward of WN.forward w.r.t. data, layer by layer in reverse (all exact-fp32 MFMA GEMMs):
//   dskip = Wend^T dout
//   d(acts_i) = Wrs_i^T [dh_{i+1}; dskip]          (+ gate derivative in the GEMM epilogue -> dpre_i)
//   dh_i = dh_{i+1} + sum_taps Win_i[:, :, tap]^T dpre_i (shifted)   (transposed dilated conv)
//   dspect += Wcond_i^T dpre_i ;  da0 = Wstart^T dh_0
// Outputs kept for the caller's weight-gradient products: dpre_all [n_layers][B][512][Lr],
// dh_all [n_layers+1][B][256][Lr] (dh_all[n_layers] = 0), dskip [B][256][Lr]; dspect [B][640][Lr], da0 [B][n_in][L].
extern "C" int facppg_wn_backward_data(const facppg_wn_weights* wts, int n_in, int n_layers, const float* dout_dev,
                                       const float* ts_all_dev, int B, int L, float* dpre_all_dev, float* dh_all_dev,
                                       float* dskip_dev, float* dspect_dev, float* da0_dev, void* ws_, size_t ws_bytes,
                                       void* stream_) {
  if (int rc = wn_check(wts, n_in, n_layers, B, L)) return rc;
  FACPPG_REQUIRE(dout_dev && ts_all_dev && dpre_all_dev && dh_all_dev && dskip_dev && dspect_dev && da0_dev && ws_, FACPPG_EINVAL,
                 "NULL argument");
  const int Lr = round_up(L, TN);
  const WnTrainWs w = wn_train_ws(n_layers, B, Lr);
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  float* tmp = (float*)(ws + w.tmp);
  const size_t dh_sz = (size_t)B * C * Lr, dp_sz = (size_t)B * 2 * C * Lr;
  for (int i = 0; i < n_layers; ++i) {
    const int last = i == n_layers - 1;
    // Wrs_i [512 or 256][256]: A_a[m][c] = Wrs[c][m] (res rows), A_b[m][c] = Wrs[256 + c][m] (skip rows)
    if (!last) {
      if (int rc = pack_a_strided(wts->rs_w[i], C, C, 1, 1, C, 0, 0, (float4*)(ws + w.rs_a[i]), s)) return rc;
      if (int rc = pack_a_strided(wts->rs_w[i], C, C, 1, 1, C, 0, (long)C * C, (float4*)(ws + w.rs_b[i]), s)) return rc;
    } else {
      if (int rc = pack_a_strided(wts->rs_w[i], C, C, 1, 1, C, 0, 0, (float4*)(ws + w.rs_b[i]), s)) return rc;
    }
    // Win_i [512][256][3] -> A[m = cin][c = cout][tap'] = Win[c][m][2 - tap']
    if (int rc = pack_a_strided(wts->in_w[i], C, 2 * C, 3, 3, (long)C * 3, -1, 2, (float4*)(ws + w.in_t[i]), s)) return rc;
    // Wcond_i [512][640] -> A[m = cond channel][c = cout]
    if (int rc = pack_a_strided(wts->cond_w[i], NCOND, 2 * C, 1, 1, NCOND, 0, 0, (float4*)(ws + w.cond_t[i]), s)) return rc;
  }
  const dim3 egrid((L + 63) / 64, B);
  FACPPG_HIP_CHECK(hipMemsetAsync(dskip_dev, 0, dh_sz * 4, s));
  FACPPG_HIP_CHECK(hipMemsetAsync(dh_all_dev, 0, dh_sz * (n_layers + 1) * 4, s));
  k_wn_end_bwd<<<egrid, 256, 0, s>>>(dout_dev, wts->end_w, dskip_dev, 2 * n_in, L, Lr);
  for (int i = n_layers - 1; i >= 0; --i) {
    const int last = i == n_layers - 1;
    float* dpre = dpre_all_dev + dp_sz * i;
    const float* dh_next = dh_all_dev + dh_sz * (i + 1);
    float* dh = dh_all_dev + dh_sz * i;
    GemmArgs g;
    g.B = B; g.N = L; g.M = C; g.Cin = C; g.ldx = Lr; g.x_bs = (long)C * Lr;
    g.splitk_ws = (float*)(ws + w.splitk); g.splitk_ws_bytes = w.splitk_bytes;
    const float* res = nullptr;
    if (!last) {   // tmp = Wrs_res^T dh_{i+1}
      g.A = (const float4*)(ws + w.rs_a[i]); g.X = dh_next; g.C = tmp; g.c_bs = (long)C * Lr; g.ldc = Lr;
      if (int rc = gemm_launch(g, s)) return rc;
      res = tmp;
    }
    // dpre_i = gate'( Wrs_skip^T dskip (+ tmp) )
    g.A = (const float4*)(ws + w.rs_b[i]); g.X = dskip_dev; g.res = res; g.res_bs = (long)C * Lr; g.ldres = Lr;
    g.gate_ts = ts_all_dev + dp_sz * i; g.gate_bs = (long)2 * C * Lr; g.ldgate = Lr;
    g.C = dpre; g.c_bs = (long)2 * C * Lr; g.ldc = Lr;
    if (int rc = gemm_launch(g, s)) return rc;
    // dh_i = dh_{i+1} + Win^T (*) dpre_i   (taps reversed, same dilation)
    GemmArgs t;
    t.splitk_ws = g.splitk_ws; t.splitk_ws_bytes = g.splitk_ws_bytes;
    t.B = B; t.N = L; t.M = C; t.Cin = 2 * C; t.taps = 3; t.pad = 1; t.dil = 1 << i; t.A = (const float4*)(ws + w.in_t[i]);
    t.X = dpre; t.x_bs = (long)2 * C * Lr; t.ldx = Lr; t.res = last ? nullptr : dh_next; t.res_bs = (long)C * Lr; t.ldres = Lr;
    t.C = dh; t.c_bs = (long)C * Lr; t.ldc = Lr;
    if (int rc = gemm_launch(t, s)) return rc;
    // dspect (+)= Wcond^T dpre_i
    GemmArgs cgm;
    cgm.B = B; cgm.N = L; cgm.M = NCOND; cgm.Cin = 2 * C; cgm.A = (const float4*)(ws + w.cond_t[i]); cgm.X = dpre;
    cgm.x_bs = (long)2 * C * Lr; cgm.ldx = Lr; cgm.res = last ? nullptr : dspect_dev; cgm.res_bs = (long)NCOND * Lr; cgm.ldres = Lr;
    cgm.C = dspect_dev; cgm.c_bs = (long)NCOND * Lr; cgm.ldc = Lr;
    if (int rc = gemm_launch(cgm, s)) return rc;
  }
  k_wn_start_bwd<<<egrid, 256, 0, s>>>(dh_all_dev, wts->start_w, da0_dev, n_in, L, Lr);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
