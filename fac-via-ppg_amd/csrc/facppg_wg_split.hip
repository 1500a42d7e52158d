// WaveGlow.infer (glow.py:252-293) with fp32 operands SPLIT into two bf16 terms, for MI355X (gfx950): fp32-class accuracy on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The third inference arithmetic, next to facppg_wg.hip (exact fp32 on the
// fp32 MFMA) and facppg_wg16.hip (fp16 operands); fp32 module, fp32 mel, fp32 noise, fp32 audio.
//
// Every fp32 operand x of a WaveNet contraction is written as hi + lo with
//   hi = RNE_bf16(x),  lo = RNE_bf16(x - float(hi))      (the subtraction is exact in fp32)
// and a product A.B is formed as A_hi.B_hi + A_hi.B_lo + A_lo.B_hi in one fp32 accumulator: 16 of the operands' 24 significand
// bits, the fp32 exponent range.  A_lo.B_lo (2^-16 of the product) is left out.
//
// Same inference algebra as facppg_wg16.hip ("Folded conditioning" / "Folded flow edges"): the images are an fp32
// handle's (facppg_wg_create folds in fp32 / fp64), read back and split once; the fp32 handle is destroyed afterwards.
//
// What is split: every weight image (at create), and -- while they are staged into LDS -- the WN hidden state h, the conditioning
// audio channels xa of a first layer, the zero-margined mel, the gated activations fed to the res GEMM and the end rows.
// What stays fp32: h, xa and the mel IN MEMORY (the residual sum is exact fp32 and is rounded nowhere), every accumulator, biases,
// the gate, the running end-row (skip) sum, the 8-channel flow variable, all flow-edge arithmetic (affine inverse, W_inverse, early
// z, start conv), the noise (wg_launch_noise's Philox draw, unrounded) and the audio.
//
// Layout (B utterances of T frames, P = hop/8 phases, Tr = round_up(T, 64), Tqp = HQ + Tr + HQ), channel-contiguous:
//   h0,h1 [B][P][Tqp][256] fp32   zero margins / frames past T_valid[b] = the dilated conv's zero padding
//   xa    [B][P][Tqp][8]   fp32   first layer's input: n_half audio channels, 1 inside the utterance, zeros
//   melp  [B][Tqp][80]     fp32
//   skip  [B][8][P][Tr]    fp32   end rows of the flow, running over its layers (folded end conv + bias)
//   aud   [B][8][L]        fp32   flow variable, natural position order (L = T*P)
// Weight images: per A fragment of v_mfma_f32_32x32x16_bf16 (8 consecutive K entries per lane, one 16-byte load) the hi plane's
// 64 lanes, then the lo plane's.
//
// Kernels: ks_pack_gate / ks_pack_res / ks_pack_end (create), ks_mel_pad, ks_mel_cvt, ks_begin (sigma*z, start conv of the last
// flow), ks_wn_layer<LAST, NCB, SEED> (one fused WN layer per launch), ks_cond_seed<BT> (the conditioning chunks of every layer
// ahead of time), ks_flow_end (affine inverse, W^-1, early z, next start conv or the final interleave).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "facppg_wg_internal.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

struct facppg_wg_split {
  facppg_wg_config cfg;
  int device, n_cu;
  int n_rem[facppg::MAXF], n_half[facppg::MAXF], early[facppg::MAXF];
  int P, kc, kcp;
  char* arena;   // one device allocation holding everything below
  size_t arena_bytes;
  const u32x4* wconv[facppg::MAXF][8];   // gate GEMM, convolution part: [48 K steps][8 waves][2][hi, lo][64] (first layer: the folded taps, 4 K steps)
  const u32x4* wcond[facppg::MAXF][8];   // gate GEMM, folded conditioning: [P][kcp/16][8][2][hi, lo][64]
  const u32x4* wres[facppg::MAXF][8];    // res rows of a non-last res_skip conv: [16][8][hi, lo][64]; null for the last layer
  const u32x4* wend[facppg::MAXF][8];    // end rows (W_end . skip rows), padded to 32 rows: [16][hi, lo][64]
  const float *b1[facppg::MAXF][8], *b2[facppg::MAXF][8];
  const float *endb[facppg::MAXF], *start_w[facppg::MAXF], *start_b[facppg::MAXF], *winv[facppg::MAXF];
  int last_tile, last_waves, last_tiles;   // shape of the WN layer launches of the most recent infer
};

namespace facppg {
namespace {

constexpr int ZP = C + 8;     // gated-activation tile: bf16 per column and plane (16-byte pad)
constexpr int SP = 64 + 8;    // staged K chunk: bf16 per column and plane
constexpr int TWMAX = 64;     // widest tile; frame rows are padded to a multiple of it

// two fp32 -> two bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack2(float a, float b) {
  const f32x2v v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf_lo(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bf_hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }
// (a, b) -> packed hi terms, packed lo terms
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
  hi = pack2(a, b);
  lo = pack2(a - bf_lo(hi), b - bf_hi(hi));
}
__device__ __forceinline__ void split8(const float4& x0, const float4& x1, u32x4& hi, u32x4& lo) {
  unsigned h[4], l[4];
  split2(x0.x, x0.y, h[0], l[0]);
  split2(x0.z, x0.w, h[1], l[1]);
  split2(x1.x, x1.y, h[2], l[2]);
  split2(x1.z, x1.w, h[3], l[3]);
  hi = u32x4{h[0], h[1], h[2], h[3]};
  lo = u32x4{l[0], l[1], l[2], l[3]};
}
__device__ __forceinline__ f32x16 mfma_bf(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------
// Reading the fp32 handle's images (facppg_wg.hip's packers) back as matrices
// ------------------------------------------------------------------------------------------
// k_pack_w1_pm / k_pack_cond_pm layout: float4 ((G*16 + w*4 + rb)*64 + lane) holds row rowmap(w, rb, lane&31),
// K = 8G + 4(lane>>5) + s.  K runs over all phases of a conditioning image (kcp is a multiple of 8).
__device__ float pm_get(const float* img, int o, int K) {
  const int G = K >> 3, kh = (K >> 2) & 1, s = K & 3;
  const int r = o & 255, w = r >> 6, rb = 2 * (o >> 8) + ((r >> 5) & 1), i = r & 31;
  return img[(((size_t)G * 16 + w * 4 + rb) * 64 + i + 32 * kh) * 4 + s];
}
// k_pack_w2(last = 1) layout (w2r, 256 res rows): float4 (((w*2 + rb)*32 + g)*64 + lane), row w*64 + rb*32 + lane&31
__device__ float w2_get(const float* img, int o, int k) {
  const int w = o >> 6, rb = (o >> 5) & 1, i = o & 31, g = k >> 3, kh = (k >> 2) & 1, s = k & 3;
  return img[((((size_t)(w * 2 + rb)) * 32 + g) * 64 + i + 32 * kh) * 4 + s];
}
// k_fold_end_rows layout: float ((s*64 + lane)*8 + g) = E[lane%16][32s + 4g + lane/16]
__device__ float we_get(const float* img, int j, int k) {
  if (j >= 16) return 0.0f;
  const int s = k >> 5, r = k & 31;
  return img[((s * 64) + j + 16 * (r & 3)) * 8 + (r >> 2)];
}
__device__ __forceinline__ void store_split(u32x4* dst, const float (&x)[8]) {
  u32x4 hi, lo;
  split8(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]), hi, lo);
  dst[0] = hi;
  dst[64] = lo;
}

// Gate image: u32x4 (((KS*8 + w)*2 + m)*2 + plane)*64 + lane = 8 bf16 of row m*256 + 32w + lane&31, K = 16 KS + 8(lane>>5) + e
// (the A operand of v_mfma_f32_32x32x16_bf16 for wave w's tanh (m = 0) / sigmoid (m = 1) rows; plane 0 = hi, 1 = lo).
__global__ void ks_pack_gate(const float* __restrict__ src, u32x4* __restrict__ dst, int nks) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nks * 1024) return;
  const int lane = t & 63, m = (t >> 6) & 1, w = (t >> 7) & 7, KS = t >> 10;
  const int o = m * C + 32 * w + (lane & 31), K = 16 * KS + 8 * (lane >> 5);
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = pm_get(src, o, K + e);
  store_split(dst + (size_t)(t >> 6) * 128 + lane, x);
}
// res rows: u32x4 ((ks*8 + w)*2 + plane)*64 + lane = row 32w + lane&31, K = 16 ks + 8(lane>>5) + e
__global__ void ks_pack_res(const float* __restrict__ src, u32x4* __restrict__ dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 16 * 512) return;
  const int lane = t & 63, w = (t >> 6) & 7, ks = t >> 9;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = w2_get(src, 32 * w + (lane & 31), 16 * ks + 8 * (lane >> 5) + e);
  store_split(dst + (size_t)(t >> 6) * 128 + lane, x);
}
// end rows: u32x4 (ks*2 + plane)*64 + lane = row lane&31 (rows >= 2*n_half are zero), K = 16 ks + 8(lane>>5) + e
__global__ void ks_pack_end(const float* __restrict__ src, u32x4* __restrict__ dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 16 * 64) return;
  const int lane = t & 63, ks = t >> 6;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = we_get(src, lane & 31, 16 * ks + 8 * (lane >> 5) + e);
  store_split(dst + (size_t)ks * 128 + lane, x);
}

// mel [B][80][T] -> melp [B][Tqp][80], zero outside each utterance's valid frames
__global__ void ks_mel_pad(const float* __restrict__ mel, float* __restrict__ melp, const int* __restrict__ t_valid, int T, int Tqp) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (idx >= Tqp * NMEL) return;
  const int x = idx / NMEL, m = idx % NMEL, q = x - HQ, Tb = t_valid ? t_valid[b] : T;
  melp[(size_t)b * Tqp * NMEL + idx] = (q >= 0 && q < Tb) ? mel[((size_t)b * NMEL + m) * T + q] : 0.0f;
}

// ------------------------------------------------------------------------------------------
// ks_wn_layer<LAST, NCB>: one WN layer on a tile of TW = 32*NCB frames of one phase of one utterance, all 512 gate rows.
// 8 waves; wave w owns channels 32w..32w+31: their tanh and sigmoid rows of the gate GEMM (so the gate is formed in
// registers), then rows 32w..32w+31 of the res GEMM.
//   gate GEMM: [512 x K] x [K x TW], K = 3*256 taps (first layer: 64, the folded taps of xa) + kcp conditioning rows, in chunks
//              of 64 read as fp32, split and staged into LDS as two [column][k] bf16 planes (double-buffered, one barrier per
//              chunk); A fragments (hi, lo) straight from the packed image, one chunk ahead in registers.  Per K step of 16 and
//              accumulator three MFMAs in ONE order -- A_hi.B_hi, A_hi.B_lo, A_lo.B_hi --, consecutive MFMAs going to different
//              accumulators (tanh rows, sigmoid rows, column blocks) so that none waits for its predecessor's result
//   gate:      z = tanh(a) * sigmoid(b) in fp32, split once into two bf16 LDS tiles [column][256]
//   res GEMM:  [256 x 256] x [256 x TW] from those tiles; h_out = h_in + res + bias, all fp32
//   end rows:  wave w multiplies its own 32 channels by the folded end rows (32-row padded A), the eight partials are
//              summed in wave order and added to the running skip rows (first layer: + the folded end bias)
// Every output column is computed the same way in every tile width (same chunk order, same MFMA order, same wave-order sum), so
// an utterance gets the same bits in any batch and any tile width.
// SEED launches (32-frame tiles, one utterance) run CONDITIONING-FIRST: the ncond conditioning chunks in their own order from zero
// accumulators, then the tap chunks -- the order in which a tile may start from ks_cond_seed's accumulators instead of running the
// conditioning chunks itself (tiles [0, seed_tiles) do; seeded or not, a column gets the same bits).  Their samples differ from
// the tap-first launches' in the last bits (fp32 reassociation); the SEED = false instantiations are the code they were.
// ------------------------------------------------------------------------------------------
struct WnSplitArgs {
  const float* h_in;
  float* h_out;
  const float* xa;
  const float* melp;
  float* skip;
  const u32x4 *wconv, *wcond, *wres, *wend;
  const float *b1, *b2, *endb;
  const int* t_valid;
  int T, P, Tr, Tqp, dil, first, nconv, ncond, kc;
};

// the arguments of a SEED launch: the layer's own, and where its seeds are
struct WnSplitSeedArgs : WnSplitArgs {
  const float4* seeds;       // this (flow, layer)'s [P][seed_nt][8 waves][2][4][64 lanes] accumulators (ks_cond_seed)
  int seed_nt, seed_tiles;   // tiles per phase row of the seed buffer; tiles [0, seed_tiles) of the launch start from their seeds
};

template <int NCB>
constexpr int wns_lds_bytes() { return 32 * NCB * (2 * ZP + 4 * SP) * 2; }

template <bool LAST, int NCB, bool SEED = false>
__global__ __launch_bounds__(512, 1) void ks_wn_layer(std::conditional_t<SEED, WnSplitSeedArgs, WnSplitArgs> p) {
  static_assert(!SEED || NCB == 1, "seeds are kept per 32-frame tile");
  constexpr int TW = 32 * NCB;
  static_assert(8 * TW <= 512, "one staged 8-element vector per thread and chunk");
  extern __shared__ __align__(16) char smem[];
  unsigned short* zt = (unsigned short*)smem;   // [2 planes][TW][ZP]
  unsigned short* stg = zt + 2 * TW * ZP;       // [2 buffers][2 planes][TW][SP]
  float* ends = (float*)stg;                    // [8 waves][8 rows][TW], after the K loop
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 31, hf = lane >> 5;
  const int b = blockIdx.y, ph = blockIdx.z, q0 = blockIdx.x * TW;
  const int Tb = p.t_valid ? p.t_valid[b] : p.T;
  if (q0 >= Tb) return;
  const int P = p.P;
  // the three taps: position l + (t-1)*dil = P*(q + qs[t]) + php[t]
  int qs[3], php[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int s = ph + (t - 1) * p.dil;
    const int f = s >= 0 ? s / P : -((-s + P - 1) / P);
    qs[t] = f; php[t] = s - f * P;
  }
  const int nch = p.nconv + p.ncond;
  // SEED: step c of the loop runs chunk kmap(c) -- the conditioning chunks, then the taps --, and a seeded tile starts at step
  // ncond from ks_cond_seed's accumulators: the registers those first steps would have left
  bool seeded = false;
  if constexpr (SEED) seeded = (int)blockIdx.x < p.seed_tiles;
  const int c_lo = seeded ? p.ncond : 0;
  auto kmap = [&](int c) __attribute__((always_inline)) {
    if constexpr (SEED) return c < p.ncond ? c + p.nconv : c - p.ncond;
    else return c;
  };
  const size_t hrow = (size_t)b * P;   // (b, phase) row base of h / xa, in units of Tqp frames
  const bool stager = tid < 8 * TW;
  const int scol = tid >> 3, skv = tid & 7;
  auto load_stage = [&](int c, float4 (&sr)[2]) __attribute__((always_inline)) {
    sr[0] = sr[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!stager) return;
    const int q = q0 + scol;
    const float* src = nullptr;
    if (c < p.nconv) {
      if (p.first) {
        if (skv < 3) src = p.xa + ((hrow + php[skv]) * p.Tqp + HQ + q + qs[skv]) * 8;
      } else {
        const int t = c >> 2, c0 = 64 * (c & 3) + 8 * skv;
        src = p.h_in + ((hrow + php[t]) * p.Tqp + HQ + q + qs[t]) * C + c0;
      }
    } else {
      const int kk = 64 * (c - p.nconv) + 8 * skv;
      if (kk < p.kc) {
        const int j = kk / NMEL, m = kk % NMEL;
        src = p.melp + ((size_t)b * p.Tqp + HQ + q - j) * NMEL + m;
      }
    }
    if (src) { sr[0] = *(const float4*)src; sr[1] = *(const float4*)(src + 4); }
  };
  auto store_stage = [&](int buf, const float4 (&sr)[2]) __attribute__((always_inline)) {
    if (!stager) return;
    u32x4 hi, lo;
    split8(sr[0], sr[1], hi, lo);
    unsigned short* d = stg + ((size_t)(buf * 2) * TW + scol) * SP + 8 * skv;
    *(u32x4*)d = hi;
    *(u32x4*)(d + TW * SP) = lo;
  };
  const int ncks = 4 * p.ncond;
  // ar[kk][m][plane]
  auto load_a = [&](int c, u32x4 (&ar)[4][2][2]) __attribute__((always_inline)) {
    const u32x4* base = c < p.nconv ? p.wconv + (size_t)(4 * c) * 2048 : p.wcond + ((size_t)ph * ncks + 4 * (c - p.nconv)) * 2048;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) ar[kk][m][pl] = base[(((kk * 8 + w) * 2 + m) * 2 + pl) * 64 + lane];
  };

  f32x16 acc[2][NCB];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
  float4 sr[2];
  u32x4 ar[4][2][2], an[4][2][2];
  load_a(kmap(c_lo), ar);
  load_stage(kmap(c_lo), sr);
  if constexpr (SEED) {
    if (seeded) {
      const float4* sp = p.seeds + ((size_t)ph * p.seed_nt + blockIdx.x) * 4096 + w * 512 + lane;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4v v = __builtin_nontemporal_load((const f32x4v*)(sp + (m * 4 + g) * 64));   // read once
          acc[m][0][4 * g + 0] = v.x; acc[m][0][4 * g + 1] = v.y; acc[m][0][4 * g + 2] = v.z; acc[m][0][4 * g + 3] = v.w;
        }
    }
  }
  store_stage(0, sr);
  __syncthreads();
  for (int c = c_lo; c < nch; ++c) {
    const int cn = kmap(c + 1 < nch ? c + 1 : c);
    load_a(cn, an);
    load_stage(cn, sr);
    const unsigned short* sb = stg + (size_t)(((c - c_lo) & 1) * 2) * TW * SP;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      u32x4 bh[NCB], bl[NCB];
#pragma unroll
      for (int n = 0; n < NCB; ++n) {
        const unsigned short* bp = sb + (32 * n + lr) * SP + 16 * kk + 8 * hf;
        bh[n] = *(const u32x4*)bp;
        bl[n] = *(const u32x4*)(bp + TW * SP);
      }
#pragma unroll
      for (int n = 0; n < NCB; ++n)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf(ar[kk][m][0], bh[n], acc[m][n]);
#pragma unroll
      for (int n = 0; n < NCB; ++n)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf(ar[kk][m][0], bl[n], acc[m][n]);
#pragma unroll
      for (int n = 0; n < NCB; ++n)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf(ar[kk][m][1], bh[n], acc[m][n]);
    }
    if (c + 1 < nch) store_stage((c + 1 - c_lo) & 1, sr);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) ar[kk][m][pl] = an[kk][m][pl];
  }

  // gate (fp32) -> split bf16 tiles.  Accumulator register r of lane (lr, hf) is row (r&3) + 8(r>>2) + 4hf, column lr.
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int ch = 32 * w + 8 * g + 4 * hf;
    const float4 bt = *(const float4*)(p.b1 + ch), bs = *(const float4*)(p.b1 + C + ch);
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
      const float z0 = gate_tanh_sigmoid(acc[0][n][4 * g + 0] + bt.x, acc[1][n][4 * g + 0] + bs.x);
      const float z1 = gate_tanh_sigmoid(acc[0][n][4 * g + 1] + bt.y, acc[1][n][4 * g + 1] + bs.y);
      const float z2 = gate_tanh_sigmoid(acc[0][n][4 * g + 2] + bt.z, acc[1][n][4 * g + 2] + bs.z);
      const float z3 = gate_tanh_sigmoid(acc[0][n][4 * g + 3] + bt.w, acc[1][n][4 * g + 3] + bs.w);
      unsigned h0, l0, h1, l1;
      split2(z0, z1, h0, l0);
      split2(z2, z3, h1, l1);
      unsigned short* d = zt + (32 * n + lr) * ZP + ch;
      *(u32x2*)d = u32x2{h0, h1};
      *(u32x2*)(d + TW * ZP) = u32x2{l0, l1};
    }
  }
  __syncthreads();

  // end rows: this wave's 32 channels (K steps 2w, 2w+1) through the folded end rows; rows 0..7 are registers 0..3
  {
    f32x16 e[NCB];
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) e[n][r] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ks = 2 * w + kk;
      const u32x4 ah = p.wend[ks * 128 + lane], al = p.wend[ks * 128 + 64 + lane];
      u32x4 zh[NCB], zl[NCB];
#pragma unroll
      for (int n = 0; n < NCB; ++n) {
        const unsigned short* zp = zt + (32 * n + lr) * ZP + 16 * ks + 8 * hf;
        zh[n] = *(const u32x4*)zp;
        zl[n] = *(const u32x4*)(zp + TW * ZP);
      }
#pragma unroll
      for (int n = 0; n < NCB; ++n) e[n] = mfma_bf(ah, zh[n], e[n]);
#pragma unroll
      for (int n = 0; n < NCB; ++n) e[n] = mfma_bf(ah, zl[n], e[n]);
#pragma unroll
      for (int n = 0; n < NCB; ++n) e[n] = mfma_bf(al, zh[n], e[n]);
    }
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) ends[(w * 8 + r + 4 * hf) * TW + 32 * n + lr] = e[n][r];
  }

  if constexpr (!LAST) {
    f32x16 r2[NCB];
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) r2[n][r] = 0.0f;
    u32x4 ah = p.wres[(w * 2) * 64 + lane], al = p.wres[(w * 2 + 1) * 64 + lane];
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
      const u32x4* nx = p.wres + (size_t)((((ks + 1) & 15) * 8 + w) * 2) * 64 + lane;
      const u32x4 ah_next = nx[0], al_next = nx[64];
      u32x4 zh[NCB], zl[NCB];
#pragma unroll
      for (int n = 0; n < NCB; ++n) {
        const unsigned short* zp = zt + (32 * n + lr) * ZP + 16 * ks + 8 * hf;
        zh[n] = *(const u32x4*)zp;
        zl[n] = *(const u32x4*)(zp + TW * ZP);
      }
#pragma unroll
      for (int n = 0; n < NCB; ++n) r2[n] = mfma_bf(ah, zh[n], r2[n]);
#pragma unroll
      for (int n = 0; n < NCB; ++n) r2[n] = mfma_bf(ah, zl[n], r2[n]);
#pragma unroll
      for (int n = 0; n < NCB; ++n) r2[n] = mfma_bf(al, zh[n], r2[n]);
      ah = ah_next; al = al_next;
    }
    // residual: h_out = h_in + res + bias in fp32, four consecutive channels per access
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
      const int q = q0 + 32 * n + lr;
      if (q >= Tb) continue;
      const size_t off = ((hrow + ph) * p.Tqp + HQ + q) * C;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = 32 * w + 8 * g + 4 * hf;
        const float4 bb = *(const float4*)(p.b2 + ch);
        const float4 hi = *(const float4*)(p.h_in + off + ch);
        float4 ho;
        ho.x = hi.x + (r2[n][4 * g + 0] + bb.x);
        ho.y = hi.y + (r2[n][4 * g + 1] + bb.y);
        ho.z = hi.z + (r2[n][4 * g + 2] + bb.z);
        ho.w = hi.w + (r2[n][4 * g + 3] + bb.w);
        *(float4*)(p.h_out + off + ch) = ho;
      }
    }
  }
  __syncthreads();
  // the end rows' partials, summed in wave order, onto the flow's running skip rows
  for (int t = tid; t < 8 * TW; t += 512) {
    const int j = t / TW, col = t % TW, q = q0 + col;
    if (q >= Tb) continue;
    float s = ends[j * TW + col];
#pragma unroll
    for (int v = 1; v < 8; ++v) s += ends[(v * 8 + j) * TW + col];
    float* dst = p.skip + (((size_t)b * 8 + j) * P + ph) * p.Tr + q;
    *dst = p.first ? p.endb[j] + s : *dst + s;
  }
}

// ------------------------------------------------------------------------------------------
// ks_cond_seed<BT>: the conditioning chunks of every (flow, layer, phase) gate GEMM for a block of BT 32-frame tiles of ONE
// utterance, ahead of the layers (WN.forward's cond_layers, glow.py:154-175, on the upsampled mel, glow.py:253-259).
// The staged window is ks_wn_layer's load_stage for its conditioning chunks (fp32 melp, zeros for kk >= kc and for frames past the
// padded length), split ONCE by split8 into the hi / lo planes the layer kernel would stage; the A fragments are the same u32x4 of
// wcond, and per K step and accumulator the three MFMAs come in the layer kernel's order from zero accumulators: the registers
// parked in the seed buffer are those a SEED ks_wn_layer holds after its first ncond steps, bit for bit.  No bias (it stays at the
// gate).  The window depends on the frames alone: it is staged once per block ([ncond][hi, lo][32 BT][SP] bf16) and stays in LDS
// while the workgroup streams one 640 KiB (hop 256) weight image after the other past it -- 2.0 GB per pass.
// A fragments: four K steps (one chunk) in registers, each K step's refilled for the next chunk as soon as its MFMAs have
// issued -- no second buffer, so that BT = 3 (96 accumulator registers) fits the 256 registers of a 512-thread workgroup.
// Work item = (group of lpw layers, phase, block), block-major so that a workgroup restages only when its block changes.
// ------------------------------------------------------------------------------------------
struct SeedSplitArgs {
  const float* melp;                // [Tqp][80] zero-margined mel frames
  float4* seeds;                    // [layers_total][P][seed_nt][8][2][4][64]
  const u32x4* wcond[MAXF * 8];     // per (flow, layer): [P][4 ncond][8][2][hi, lo][64]
  int lpw, P, Tr, seed_nt;
  int tile0, tile1, nblk;           // tiles [tile0, tile1) in nblk blocks of BT
  int ncond, kc;
  int layer0, layer1, items;
  const int* skip;                  // optional (device): *skip != 0 -> the launch does nothing
  int* counter;                     // bounded launch: hands out the items past the first gridDim (zero at launch), or null: strided
};

constexpr int SEED_LDS_MAX = 160 * 1024 - 64;   // a CU's LDS less the kernel's own word
constexpr int SEED_BT_MAX = 3;
constexpr size_t seed_window_bytes(int ncond, int bt) { return (size_t)ncond * 2 * 32 * bt * SP * 2; }

template <int BT>
__global__ __launch_bounds__(512) void ks_cond_seed(SeedSplitArgs p) {
  constexpr int TW = 32 * BT;
  extern __shared__ __align__(16) char smem[];
  unsigned short* win = (unsigned short*)smem;   // [ncond][2 planes][TW][SP]
  __shared__ int next_item;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 31, hf = lane >> 5;
  if (p.skip && *p.skip) return;
  const int nlg = (p.layer1 - p.layer0 + p.lpw - 1) / p.lpw, per = nlg * p.P, ncks = 4 * p.ncond;
  int cur_blk = -1;
  for (int lin = (int)blockIdx.x; lin < p.items;) {
    const int blk = lin / per, rest = lin - blk * per, lg = rest / p.P, ph = rest - lg * p.P;
    const int t0 = p.tile0 + blk * BT;
    if (blk != cur_blk) {              // (uniform over the workgroup)
      __syncthreads();
      for (int v = tid; v < p.ncond * TW * 8; v += 512) {
        const int c = v / (TW * 8), r = v - c * (TW * 8), col = r >> 3, kv = r & 7;
        const int q = t0 * 32 + col, kk = 64 * c + 8 * kv;
        float4 x0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), x1 = x0;
        if (kk < p.kc && q < p.Tr) {
          const int j = kk / NMEL, m = kk % NMEL;
          const float* src = p.melp + ((size_t)HQ + q - j) * NMEL + m;
          x0 = *(const float4*)src; x1 = *(const float4*)(src + 4);
        }
        u32x4 hi, lo;
        split8(x0, x1, hi, lo);
        unsigned short* d = win + ((size_t)(c * 2) * TW + col) * SP + 8 * kv;
        *(u32x4*)d = hi;
        *(u32x4*)(d + TW * SP) = lo;
      }
      __syncthreads();
      cur_blk = blk;
    }
    const int l0 = p.layer0 + lg * p.lpw, l1 = min(l0 + p.lpw, p.layer1);
    for (int l = l0; l < l1; ++l) {
      // (((kk*8 + w)*2 + m)*2 + plane)*64 + lane of K step kk
      const u32x4* img = p.wcond[l] + (size_t)ph * ncks * 2048 + w * 256 + lane;
      f32x16 acc[2][BT];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < BT; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
      u32x4 ar[4][2][2];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) ar[kk][m][pl] = __builtin_nontemporal_load(img + kk * 2048 + (m * 2 + pl) * 64);
      for (int c = 0; c < p.ncond; ++c) {
        const int cn = c + 1 < p.ncond ? c + 1 : c;
        const unsigned short* sb = win + (size_t)(c * 2) * TW * SP;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          u32x4 bh[BT], bl[BT];
#pragma unroll
          for (int n = 0; n < BT; ++n) {
            const unsigned short* bp = sb + (32 * n + lr) * SP + 16 * kk + 8 * hf;
            bh[n] = *(const u32x4*)bp;
            bl[n] = *(const u32x4*)(bp + TW * SP);
          }
#pragma unroll
          for (int n = 0; n < BT; ++n)
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf(ar[kk][m][0], bh[n], acc[m][n]);
#pragma unroll
          for (int n = 0; n < BT; ++n)
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf(ar[kk][m][0], bl[n], acc[m][n]);
#pragma unroll
          for (int n = 0; n < BT; ++n)
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf(ar[kk][m][1], bh[n], acc[m][n]);
          // this K step's fragments of the next chunk, into the registers just read
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) ar[kk][m][pl] = __builtin_nontemporal_load(img + (size_t)(4 * cn + kk) * 2048 + (m * 2 + pl) * 64);
        }
      }
#pragma unroll
      for (int n = 0; n < BT; ++n) {
        if (t0 + n >= p.tile1) break;
        float4* dst = p.seeds + (((size_t)l * p.P + ph) * p.seed_nt + t0 + n) * 4096 + w * 512 + lane;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            __builtin_nontemporal_store(f32x4v{acc[m][n][4 * g + 0], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]},
                                        (f32x4v*)(dst + (m * 4 + g) * 64));   // read back milliseconds later: not through the L2
      }
    }
    if (p.counter) {
      __syncthreads();
      if (tid == 0) next_item = (int)gridDim.x + atomicAdd(p.counter, 1);
      __syncthreads();
      lin = next_item;
    } else {
      lin += (int)gridDim.x;
    }
  }
}

// frames [f0, f0 + n) of an fp32 mel [80][ld] (the streaming postnet's output) -> the zero-margined fp32 [Tqp][80] layout
__global__ void ks_mel_cvt(const float* __restrict__ mel, int ld, float* __restrict__ melp, int f0, int n, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * NMEL) return;
  const int m = idx / n, q = f0 + idx % n;
  melp[((size_t)HQ + q) * NMEL + m] = mel[(size_t)m * ld + q];
}

// ------------------------------------------------------------------------------------------
// Flow edges in fp32: 8 positions per 256-thread workgroup, 32 threads per position (8 start-conv channels each: two 16-byte
// stores, a position's 1 KiB h row written by 32 consecutive lanes).  grid = (ceil(T/8), B, P).
// ------------------------------------------------------------------------------------------
struct EdgeSplitArgs {
  const float* skip;
  const float* aud_in;
  float* aud_out;
  float* h_out;
  float* xa;
  float* audio;          // [B][T*hop]
  const float* z0;       // [B][2*HN][L]
  const float* z_early;  // [B][2][L] or null
  const float *winv, *start_w, *start_b;
  const int* t_valid;
  float sigma;
  int T, P, Tr, Tqp, L, swap, swap_next, final_flow;
};

__device__ __forceinline__ bool edges_pos(const EdgeSplitArgs& p, int& b, int& q, int& pos, int& cg) {
  b = blockIdx.y;
  q = blockIdx.x * 8 + (threadIdx.x >> 5);
  cg = threadIdx.x & 31;
  const int Tb = p.t_valid ? p.t_valid[b] : p.T;
  pos = q * p.P + blockIdx.z;
  return q < Tb;
}

// start conv (channels 8cg..8cg+7) of the flow whose conditioning channels are a0[0..HN), and (cg == 0) its xa row
template <int HN>
__device__ __forceinline__ void starts(const EdgeSplitArgs& p, int b, int q, int cg, const float* a0) {
  const size_t row = ((size_t)b * p.P + blockIdx.z) * p.Tqp + HQ + q;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ch = 8 * cg + e;
    float s = p.start_b[ch];
#pragma unroll
    for (int j = 0; j < HN; ++j) s = fmaf(p.start_w[ch * HN + j], a0[j], s);
    v[e] = s;
  }
  float* hd = p.h_out + row * C + 8 * cg;
  *(float4*)hd = make_float4(v[0], v[1], v[2], v[3]);
  *(float4*)(hd + 4) = make_float4(v[4], v[5], v[6], v[7]);
  if (cg == 0) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = j < HN ? a0[j] : j == HN ? 1.0f : 0.0f;
    float* xd = p.xa + row * 8;
    *(float4*)xd = make_float4(x[0], x[1], x[2], x[3]);
    *(float4*)(xd + 4) = make_float4(x[4], x[5], x[6], x[7]);
  }
}

template <int HN>
__global__ __launch_bounds__(256) void ks_begin(EdgeSplitArgs p) {
  int b, q, pos, cg;
  if (!edges_pos(p, b, q, pos, cg)) return;
  float a[2 * HN];
#pragma unroll
  for (int j = 0; j < 2 * HN; ++j) {
    a[j] = p.sigma * p.z0[((size_t)b * 2 * HN + j) * p.L + pos];
    if (cg == 0) p.aud_out[((size_t)b * 8 + j) * p.L + pos] = a[j];
  }
  starts<HN>(p, b, q, cg, a + (p.swap_next ? HN : 0));
}

template <int H, bool EARLY>
__global__ __launch_bounds__(256) void ks_flow_end(EdgeSplitArgs p) {
  constexpr int CC = 2 * H, CN = EARLY ? CC + 2 : CC;
  int b, q, pos, cg;
  if (!edges_pos(p, b, q, pos, cg)) return;
  float o[CC], a[CC], y[CN];
#pragma unroll
  for (int j = 0; j < CC; ++j) {
    o[j] = p.skip[(((size_t)b * 8 + j) * p.P + blockIdx.z) * p.Tr + q];
    a[j] = p.aud_in[((size_t)b * 8 + j) * p.L + pos];
  }
  const int tr = p.swap ? 0 : H;   // the transformed half; the other one conditioned the WN
#pragma unroll
  for (int j = 0; j < H; ++j) a[tr + j] = (a[tr + j] - o[j]) / expf(o[H + j]);
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
    if (cg < CN) p.audio[(size_t)b * p.T * p.P * 8 + (size_t)pos * CN + cg] = y[cg];   // glow.py:292 interleave
    return;
  }
  if (cg == 0) {
#pragma unroll
    for (int j = 0; j < CN; ++j) p.aud_out[((size_t)b * 8 + j) * p.L + pos] = y[j];
  }
  starts<CN / 2>(p, b, q, cg, y + (p.swap_next ? CN / 2 : 0));
}

struct WsSplit {
  int P, L, Tr, Tqp;
  size_t h0, h1, xa, melp, skip, aud0, aud1, z, total;
};
WsSplit wss_layout(const facppg_wg_config& c, int B, int T) {
  WsSplit w;
  w.P = c.hop_length / 8;
  w.L = T * w.P;
  w.Tr = round_up(T, TWMAX);
  w.Tqp = HQ + w.Tr + HQ;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.h0 = take((size_t)B * w.P * w.Tqp * C * 4);
  w.h1 = take((size_t)B * w.P * w.Tqp * C * 4);
  w.xa = take((size_t)B * w.P * w.Tqp * 8 * 4);   // right behind h0 | h1: one memset zeroes all three
  w.melp = take((size_t)B * w.Tqp * NMEL * 4);
  w.skip = take((size_t)B * 8 * w.P * w.Tr * 4);
  w.aud0 = take((size_t)B * 8 * w.L * 4);
  w.aud1 = take((size_t)B * 8 * w.L * 4);
  w.z = take(((size_t)B * 8 * w.L + 4) * 4);
  w.total = off;
  return w;
}

template <int H>
void launch_flow_end_s(bool early, dim3 grid, hipStream_t s, const EdgeSplitArgs& a) {
  if (early) ks_flow_end<H, true><<<grid, 256, 0, s>>>(a);
  else ks_flow_end<H, false><<<grid, 256, 0, s>>>(a);
}

}  // namespace
}  // namespace facppg

using namespace facppg;

extern "C" void facppg_wg_split_destroy(facppg_wg_split* h) {
  if (!h) return;
  if (h->arena) {
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != h->device && hipSetDevice(h->device) == hipSuccess;
    (void)hipFree(h->arena);
    if (sw) (void)hipSetDevice(prev);
  }
  delete h;
}

extern "C" int facppg_wg_split_create(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats, int device,
                                      void* stream_, facppg_wg_split** out) {
  FACPPG_REQUIRE(out, FACPPG_EINVAL, "out is NULL");
  // the fp32 handle folds the blob (upsampler into the conditioning, end conv through the skip rows, first taps through
  // start); its images are read back here and split into bf16 planes once
  facppg_wg* f = nullptr;
  if (int rc = facppg_wg_create(cfg, weights_dev, n_floats, device, stream_, &f)) return rc;
  hipStream_t s = (hipStream_t)stream_;
  const facppg_wg_config& c = f->cfg;
  const int P = f->P, kcp = f->kcp, nl = c.wn_layers, nf = c.n_flows;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  struct Off { size_t wconv[8], wcond[8], wres[8], wend[8], b1[8], b2[8], endb, start_w, start_b, winv; };
  Off* fo = new (std::nothrow) Off[MAXF];
  facppg_wg_split* h = new (std::nothrow) facppg_wg_split();
  if (fo && h) {
    for (int k = 0; k < nf; ++k) {
      const size_t hh = f->n_half[k], cc = 2 * hh;
      for (int i = 0; i < nl; ++i) {
        fo[k].wconv[i] = take((size_t)(i == 0 ? 4 : 48) * 2048 * 16);
        fo[k].wcond[i] = take((size_t)P * (kcp / 16) * 2048 * 16);
        fo[k].wres[i] = i == nl - 1 ? 0 : take((size_t)16 * 1024 * 16);
        fo[k].wend[i] = take((size_t)16 * 128 * 16);
        fo[k].b1[i] = take(2 * C * 4);
        fo[k].b2[i] = take(C * 4);
      }
      fo[k].endb = take(8 * 4); fo[k].start_w = take(C * hh * 4); fo[k].start_b = take(C * 4); fo[k].winv = take(cc * cc * 4);
    }
  }
  if (!fo || !h || hipMalloc((void**)&h->arena, off) != hipSuccess) {
    if (h) h->arena = nullptr;
    delete h; delete[] fo;
    facppg_wg_destroy(f);
    set_error("facppg_wg_split_create: allocating %zu bytes of split bf16 images failed", off);
    return FACPPG_EHIP;
  }
  h->cfg = c; h->device = f->device; h->arena_bytes = off; h->n_cu = f->n_cu;
  memcpy(h->n_rem, f->n_rem, sizeof(h->n_rem)); memcpy(h->n_half, f->n_half, sizeof(h->n_half)); memcpy(h->early, f->early, sizeof(h->early));
  h->P = P; h->kc = f->kc; h->kcp = kcp;
  auto U = [&](size_t o) { return (u32x4*)(h->arena + o); };
  auto F = [&](size_t o) { return (float*)(h->arena + o); };
  hipError_t e = hipSuccess;
  auto cpy = [&](size_t o, const float* src, size_t n) {
    if (e == hipSuccess) e = hipMemcpyAsync(F(o), src, n * 4, hipMemcpyDeviceToDevice, s);
  };
  for (int k = 0; k < nf && e == hipSuccess; ++k) {
    const size_t hh = f->n_half[k], cc = 2 * hh;
    for (int i = 0; i < nl; ++i) {
      const bool last = i == nl - 1;
      const int nks = i == 0 ? 4 : 48, ncks = P * (kcp / 16);
      ks_pack_gate<<<nks * 4, 256, 0, s>>>(i == 0 ? (const float*)f->w1f[k] : (const float*)f->w1pm[k][i], U(fo[k].wconv[i]), nks);
      ks_pack_gate<<<ncks * 4, 256, 0, s>>>((const float*)f->wcpm[k][i], U(fo[k].wcond[i]), ncks);
      if (!last) ks_pack_res<<<32, 256, 0, s>>>((const float*)f->w2r[k][i], U(fo[k].wres[i]));
      ks_pack_end<<<4, 256, 0, s>>>(f->we[k][i], U(fo[k].wend[i]));
      cpy(fo[k].b1[i], f->b1pm[k][i], 2 * C);
      cpy(fo[k].b2[i], f->b2[k][i], C);
      h->wconv[k][i] = U(fo[k].wconv[i]); h->wcond[k][i] = U(fo[k].wcond[i]);
      h->wres[k][i] = last ? nullptr : U(fo[k].wres[i]); h->wend[k][i] = U(fo[k].wend[i]);
      h->b1[k][i] = F(fo[k].b1[i]); h->b2[k][i] = F(fo[k].b2[i]);
    }
    cpy(fo[k].endb, f->endb[k], 8);
    cpy(fo[k].start_w, f->start_w[k], C * hh);
    cpy(fo[k].start_b, f->start_b[k], C);
    cpy(fo[k].winv, f->winv[k], cc * cc);
    h->endb[k] = F(fo[k].endb); h->start_w[k] = F(fo[k].start_w); h->start_b[k] = F(fo[k].start_b); h->winv[k] = F(fo[k].winv);
  }
  delete[] fo;
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // (the fp32 images are read by the packers above)
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)ks_wn_layer<false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, wns_lds_bytes<2>());
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)ks_wn_layer<true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, wns_lds_bytes<2>());
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)ks_cond_seed<1>, hipFuncAttributeMaxDynamicSharedMemorySize, SEED_LDS_MAX);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)ks_cond_seed<2>, hipFuncAttributeMaxDynamicSharedMemorySize, SEED_LDS_MAX);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)ks_cond_seed<3>, hipFuncAttributeMaxDynamicSharedMemorySize, SEED_LDS_MAX);
  facppg_wg_destroy(f);
  if (e != hipSuccess) {
    set_error("facppg_wg_split_create: %s", hipGetErrorString(e));
    facppg_wg_split_destroy(h);
    return FACPPG_EHIP;
  }
  *out = h;
  return FACPPG_OK;
}

extern "C" size_t facppg_wg_split_workspace_bytes(const facppg_wg_split* h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  return wss_layout(h->cfg, B, T).total;
}

extern "C" int facppg_wg_split_last_launch_shape(const facppg_wg_split* h, int* tile_frames, int* waves, int* n_tiles) {
  FACPPG_REQUIRE(h && tile_frames && waves && n_tiles, FACPPG_EINVAL, "NULL argument");
  *tile_frames = h->last_tile; *waves = h->last_waves; *n_tiles = h->last_tiles;
  return FACPPG_OK;
}

// WaveGlow.infer on a split handle.  melp_ext != null (B = 1): the caller's zero-margined fp32 mel buffer laid out, like `seeds`,
// for T_layout >= T frames; the layer launches are then the SEED ones (32-frame tiles, conditioning-first): tiles wholly inside
// [0, seeded_frames) start from their seeds, the others run full K in the same launches.  flow_events[k] (may be null): the
// launches of flow k wait for it on the stream.
static int wgs_infer(facppg_wg_split* h, const float* mel_dev, const int32_t* T_valid_dev, const float* z_dev, uint64_t seed,
                     float sigma, int B, int T, float* audio_dev, void* ws_, size_t ws_bytes, void* stream_,
                     const float* melp_ext = nullptr, const float* seeds_dev = nullptr, int seeded_frames = 0, int T_layout = 0,
                     void* const* flow_events = nullptr) {
  if (!melp_ext) T_layout = T;
  const size_t need = facppg_wg_split_workspace_bytes(h, B, T_layout);
  FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, need);
  const facppg_wg_config& c = h->cfg;
  {
    int tot = h->n_rem[c.n_flows - 1];
    for (int k = 0; k < c.n_flows; ++k) tot += h->early[k] ? c.n_early_size : 0;
    FACPPG_REQUIRE(tot == 8, FACPPG_EUNSUPPORTED, "noise channel count %d != n_group", tot);
  }
  WsSplit w = wss_layout(c, B, T_layout);   // rows (Tr, Tqp) of the layout; positions of the T frames that are there
  w.L = T * w.P;
  FACPPG_REQUIRE((1 << (c.wn_layers - 1)) / w.P + 1 <= HQ, FACPPG_EUNSUPPORTED, "hop %d: the dilated taps reach past the %d-frame margins",
                 c.hop_length, HQ);
  FACPPG_REQUIRE((double)B * w.P * w.Tqp * C < 2.0e9, FACPPG_EUNSUPPORTED, "B*T = %d*%d frames is too long", B, T);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  float* hbuf[2] = {(float*)(ws + w.h0), (float*)(ws + w.h1)};
  float* xa = (float*)(ws + w.xa);
  const float* melp = melp_ext ? melp_ext : (const float*)(ws + w.melp);
  float* skip = (float*)(ws + w.skip);
  float* aud[2] = {(float*)(ws + w.aud0), (float*)(ws + w.aud1)};
  const int nf = c.n_flows;
  // tile width: 64 frames when that still gives every CU a workgroup, else 32 (the B = 1 latency shape: narrow tiles spread one
  // short utterance over the chip); FACPPG_WG_SPLIT_TILE = 32 | 64 forces one
  const long tiles64 = (long)w.P * B * ((T + 63) / 64);
  const long ncu = h->n_cu > 0 ? h->n_cu : 256;
  int tw = tiles64 >= ncu ? 64 : 32;
  if (const char* env = getenv("FACPPG_WG_SPLIT_TILE")) {
    const int v = atoi(env);
    FACPPG_REQUIRE(v == 32 || v == 64, FACPPG_EINVAL, "FACPPG_WG_SPLIT_TILE=%s: expected 32 or 64", env);
    tw = v;
  }
  if (melp_ext) tw = 32;   // seeds are kept per 32-frame tile
  FACPPG_HIP_CHECK(hipMemsetAsync(ws + w.h0, 0, w.melp - w.h0, s));   // h0, h1, xa: margins and frames past each utterance
  if (!melp_ext) ks_mel_pad<<<dim3((w.Tqp * NMEL + 255) / 256, B), 256, 0, s>>>(mel_dev, (float*)(ws + w.melp), T_valid_dev, T, w.Tqp);
  const float* z = z_dev;
  if (!z) {
    wg_launch_noise((float*)(ws + w.z), (size_t)B * 8 * w.L, seed, s);
    z = (const float*)(ws + w.z);
  }
  const dim3 lgrid((T + tw - 1) / tw, B, w.P);
  h->last_tile = tw; h->last_waves = 8; h->last_tiles = (int)(lgrid.x * lgrid.y * lgrid.z);

  EdgeSplitArgs e;
  memset(&e, 0, sizeof(e));
  e.skip = skip; e.xa = xa; e.audio = audio_dev; e.t_valid = T_valid_dev; e.sigma = sigma;
  e.T = T; e.P = w.P; e.Tr = w.Tr; e.Tqp = w.Tqp; e.L = w.L;
  const dim3 egrid((T + 7) / 8, B, w.P);
  int ai = 0, hi = 0;
  {
    const int k = nf - 1;
    e.z0 = z; e.aud_out = aud[ai]; e.h_out = hbuf[hi]; e.start_w = h->start_w[k]; e.start_b = h->start_b[k];
    e.swap_next = c.alternate_halves && (k & 1);
    switch (h->n_half[k]) {
      case 1: ks_begin<1><<<egrid, 256, 0, s>>>(e); break;
      case 2: ks_begin<2><<<egrid, 256, 0, s>>>(e); break;
      case 3: ks_begin<3><<<egrid, 256, 0, s>>>(e); break;
      case 4: ks_begin<4><<<egrid, 256, 0, s>>>(e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
  }
  size_t z_off = (size_t)B * h->n_rem[nf - 1] * w.L;
  WnSplitSeedArgs a;   // (an unseeded launch takes its WnSplitArgs part)
  memset(&a, 0, sizeof(a));
  a.xa = xa; a.melp = melp; a.skip = skip; a.t_valid = T_valid_dev;
  a.T = T; a.P = w.P; a.Tr = w.Tr; a.Tqp = w.Tqp; a.kc = h->kc; a.ncond = h->kcp / 64;
  a.seed_nt = w.Tr / 32; a.seed_tiles = melp_ext ? std::min(seeded_frames, round_up(T, 32)) / 32 : 0;
  for (int k = nf - 1; k >= 0; --k) {
    if (flow_events && flow_events[k]) FACPPG_HIP_CHECK(hipStreamWaitEvent(s, (hipEvent_t)flow_events[k], 0));
    a.endb = h->endb[k];
    for (int i = 0; i < c.wn_layers; ++i) {
      if (melp_ext) a.seeds = (const float4*)seeds_dev + (size_t)(k * c.wn_layers + i) * w.P * a.seed_nt * 4096;
      const bool last = i == c.wn_layers - 1;
      a.h_in = hbuf[hi]; a.h_out = hbuf[hi ^ 1];
      a.wconv = h->wconv[k][i]; a.wcond = h->wcond[k][i]; a.wres = h->wres[k][i]; a.wend = h->wend[k][i];
      a.b1 = h->b1[k][i]; a.b2 = h->b2[k][i];
      a.dil = 1 << i; a.first = i == 0; a.nconv = i == 0 ? 1 : 12;
      if (melp_ext) {
        if (last) ks_wn_layer<true, 1, true><<<lgrid, 512, wns_lds_bytes<1>(), s>>>(a);
        else ks_wn_layer<false, 1, true><<<lgrid, 512, wns_lds_bytes<1>(), s>>>(a);
      } else if (tw == 64) {
        if (last) ks_wn_layer<true, 2><<<lgrid, 512, wns_lds_bytes<2>(), s>>>(a);
        else ks_wn_layer<false, 2><<<lgrid, 512, wns_lds_bytes<2>(), s>>>(a);
      } else {
        if (last) ks_wn_layer<true, 1><<<lgrid, 512, wns_lds_bytes<1>(), s>>>(a);
        else ks_wn_layer<false, 1><<<lgrid, 512, wns_lds_bytes<1>(), s>>>(a);
      }
      if (!last) hi ^= 1;
    }
    e.aud_in = aud[ai]; e.aud_out = aud[ai ^ 1]; e.h_out = hbuf[hi];
    e.winv = h->winv[k];
    e.final_flow = k == 0;
    e.swap = c.alternate_halves && (k & 1);
    e.swap_next = c.alternate_halves && k > 0 && ((k - 1) & 1);
    e.z_early = nullptr;
    if (h->early[k]) { e.z_early = z + z_off; z_off += (size_t)B * c.n_early_size * w.L; }
    if (k > 0) { e.start_w = h->start_w[k - 1]; e.start_b = h->start_b[k - 1]; }
    const int cn = 2 * h->n_half[k] + (h->early[k] ? 2 : 0);
    if (k > 0) FACPPG_REQUIRE(cn == 2 * h->n_half[k - 1], FACPPG_EUNSUPPORTED, "flow %d channel mismatch", k);
    else FACPPG_REQUIRE(cn == 8, FACPPG_EUNSUPPORTED, "final flow must yield n_group channels");
    switch (h->n_half[k]) {
      case 1: launch_flow_end_s<1>(h->early[k], egrid, s, e); break;
      case 2: launch_flow_end_s<2>(h->early[k], egrid, s, e); break;
      case 3: launch_flow_end_s<3>(h->early[k], egrid, s, e); break;
      case 4: launch_flow_end_s<4>(h->early[k], egrid, s, e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
    ai ^= 1;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_split_infer(facppg_wg_split* h, const float* mel_dev, const int32_t* T_valid_dev, const float* z_dev,
                                     uint64_t seed, float sigma, int B, int T, float* audio_dev, void* ws_, size_t ws_bytes,
                                     void* stream_) {
  FACPPG_REQUIRE(h && mel_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && T > 0, FACPPG_EINVAL, "B and T must be positive (got %d, %d)", B, T);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EINVAL, "B too large");
  return wgs_infer(h, mel_dev, T_valid_dev, z_dev, seed, sigma, B, T, audio_dev, ws_, ws_bytes, stream_);
}

extern "C" int facppg_wg_split_seed_layout(const facppg_wg_split* h, int T, int* Tqp, int* margin, size_t* seed_bytes,
                                           int* max_block_tiles) {
  FACPPG_REQUIRE(h && T > 0 && Tqp && margin && seed_bytes && max_block_tiles, FACPPG_EINVAL, "NULL argument or T <= 0");
  const WsSplit w = wss_layout(h->cfg, 1, T);
  *Tqp = w.Tqp; *margin = HQ;
  *seed_bytes = (size_t)h->cfg.n_flows * h->cfg.wn_layers * w.P * (w.Tr / 32) * 4096 * sizeof(float4);
  int bt = 0;
  while (bt < SEED_BT_MAX && seed_window_bytes(h->kcp / 64, bt + 1) <= (size_t)SEED_LDS_MAX) ++bt;
  *max_block_tiles = bt;
  return FACPPG_OK;
}

extern "C" int facppg_wg_split_mel_pad(const facppg_wg_split* h, const float* mel_dev, int T, int ld, int frame0, int nframes,
                                       float* melp_dev, const int32_t* skip_dev, void* stream_) {
  FACPPG_REQUIRE(h && mel_dev && melp_dev && T > 0, FACPPG_EINVAL, "NULL argument or T <= 0");
  const WsSplit w = wss_layout(h->cfg, 1, T);
  FACPPG_REQUIRE(frame0 >= 0 && nframes >= 0 && frame0 + nframes <= w.Tr && frame0 + nframes <= ld, FACPPG_EINVAL,
                 "frames [%d, %d) do not lie inside the %d padded frames and the row length %d", frame0, frame0 + nframes, w.Tr, ld);
  if (nframes == 0) return FACPPG_OK;
  ks_mel_cvt<<<(nframes * NMEL + 255) / 256, 256, 0, (hipStream_t)stream_>>>(mel_dev, ld, melp_dev, frame0, nframes, skip_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_split_cond_seed(facppg_wg_split* h, const float* melp_dev, int T, int frame0, int nframes, int block_tiles,
                                         int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                                         const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream_) {
  FACPPG_REQUIRE(h && melp_dev && seeds_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0, FACPPG_EINVAL, "T must be positive (got %d)", T);
  const facppg_wg_config& c = h->cfg;
  const WsSplit w = wss_layout(c, 1, T);
  size_t need = 0; int tqp = 0, mg = 0, bt_max = 0;
  facppg_wg_split_seed_layout(h, T, &tqp, &mg, &need, &bt_max);
  FACPPG_REQUIRE(seed_bytes >= need, FACPPG_EWORKSPACE, "seed buffer has %zu bytes, need %zu", seed_bytes, need);
  FACPPG_REQUIRE(frame0 >= 0 && frame0 % 32 == 0 && nframes > 0 && frame0 + nframes <= w.Tr, FACPPG_EINVAL,
                 "frames [%d, %d): the first must be a multiple of 32 and the range inside the %d padded frames", frame0, frame0 + nframes, w.Tr);
  FACPPG_REQUIRE(layers_per_workgroup >= 1, FACPPG_EINVAL, "layers_per_workgroup >= 1");
  FACPPG_REQUIRE(bt_max >= 1, FACPPG_EUNSUPPORTED, "hop %d: the conditioning window of one 32-frame tile (%zu bytes) does not fit the LDS",
                 c.hop_length, seed_window_bytes(h->kcp / 64, 1));
  FACPPG_REQUIRE(block_tiles >= 1 && block_tiles <= bt_max, FACPPG_EINVAL,
                 "block_tiles = %d: the window of %zu bytes per tile must fit %d bytes of LDS and %d accumulator tiles the registers: "
                 "the maximum is %d", block_tiles, seed_window_bytes(h->kcp / 64, 1), SEED_LDS_MAX, SEED_BT_MAX, bt_max);
  if (nflows <= 0) { flow0 = 0; nflows = c.n_flows; }
  FACPPG_REQUIRE(flow0 >= 0 && flow0 + nflows <= c.n_flows, FACPPG_EINVAL, "flows [%d, %d) of %d", flow0, flow0 + nflows, c.n_flows);
  FACPPG_REQUIRE(c.n_flows * c.wn_layers <= MAXF * 8, FACPPG_EUNSUPPORTED, "too many layers");
  SeedSplitArgs a;
  memset(&a, 0, sizeof(a));
  a.melp = melp_dev; a.seeds = (float4*)seeds_dev; a.skip = skip_dev;
  for (int k = 0; k < c.n_flows; ++k)
    for (int i = 0; i < c.wn_layers; ++i) a.wcond[k * c.wn_layers + i] = h->wcond[k][i];
  a.lpw = layers_per_workgroup; a.P = w.P; a.Tr = w.Tr; a.seed_nt = w.Tr / 32;
  const int ntiles = (nframes + 31) / 32;
  a.tile0 = frame0 / 32; a.tile1 = a.tile0 + ntiles; a.nblk = (ntiles + block_tiles - 1) / block_tiles;
  a.ncond = h->kcp / 64; a.kc = h->kc;
  a.layer0 = flow0 * c.wn_layers; a.layer1 = (flow0 + nflows) * c.wn_layers;
  a.items = (a.layer1 - a.layer0 + a.lpw - 1) / a.lpw * w.P * a.nblk;
  size_t lds = seed_window_bytes(a.ncond, block_tiles);
  // a BOUNDED launch (the caller shares the GPU with other streams) asks for a CU's whole LDS per workgroup, as
  // facppg_wg_cond_seed does: one workgroup per CU and no other stream's small workgroups next to it
  const int max_wgs = max_workgroups / 8 * 8;
  const bool bounded = max_wgs > 0 && max_wgs < a.items;
  if (max_workgroups > 0) lds = (size_t)SEED_LDS_MAX;
  a.counter = bounded ? counter_dev : nullptr;
  FACPPG_REQUIRE(!bounded || counter_dev, FACPPG_EINVAL, "a bounded launch needs counter_dev");
  const unsigned grid = (unsigned)(bounded ? max_wgs : a.items);
  hipStream_t s = (hipStream_t)stream_;
  switch (block_tiles) {
    case 1: ks_cond_seed<1><<<grid, 512, lds, s>>>(a); break;
    case 2: ks_cond_seed<2><<<grid, 512, lds, s>>>(a); break;
    default: ks_cond_seed<3><<<grid, 512, lds, s>>>(a); break;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_split_infer_seeded(facppg_wg_split* h, const float* melp_dev, int T_layout, int T, const float* seeds_dev,
                                            int seeded_frames, const float* z_dev, uint64_t seed, float sigma, float* audio_dev,
                                            void* ws_, size_t ws_bytes, void* const* flow_events, void* stream_) {
  FACPPG_REQUIRE(h && melp_dev && seeds_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0 && T_layout >= T, FACPPG_EINVAL, "need 0 < T <= T_layout (got %d, %d)", T, T_layout);
  FACPPG_REQUIRE(seeded_frames >= 0 && seeded_frames % 32 == 0 && seeded_frames <= round_up(T, 32), FACPPG_EINVAL,
                 "seeded_frames = %d: expected a multiple of 32 in [0, %d]", seeded_frames, round_up(T, 32));
  return wgs_infer(h, nullptr, nullptr, z_dev, seed, sigma, 1, T, audio_dev, ws_, ws_bytes, stream_, melp_dev, seeds_dev, seeded_frames,
                   T_layout, flow_events);
}
