// WaveGlow.infer in half precision for MI355X (gfx950): the reference's HalfTensor branch of WaveGlow.infer
// (glow.py:261-290, reached through inference.py --is_fp16: waveglow.half(), convinv kept in fp32, half mels)
// on v_mfma_f32_32x32x16_f16 with fp32 accumulation.
//
// Same inference algebra as facppg_wg.hip's phase-major path ("Folded conditioning" / "Folded flow edges"):
// the upsampler folded into per-phase conditioning weights, the `end` conv folded through the skip rows, the first
// layer's taps folded through `start`.  The images are made from an fp32 handle's (facppg_wg_create folds in fp32 /
// fp64 from the module's values) and rounded to fp16 once, here; the fp32 handle is destroyed afterwards.
//
// What is fp16: every weight image, the WN hidden state h, the conditioning audio channels xa of a first layer, the
// zero-margined mel, the gated activations fed to the res/skip GEMM, injected / drawn noise and the output audio.
// What stays fp32: every accumulator, biases, the gate, the running end-row (skip) sum, the 8-channel flow variable and
// all flow-edge arithmetic (affine inverse, W_inverse, early z).
//
// Layout (B utterances of T frames, P = hop/8 phases, Tr = round_up(T, 128), Tqp = HQ + Tr + HQ), CHANNEL-CONTIGUOUS
// so that the 8 consecutive K entries one MFMA lane feeds are one 16-byte access:
//   h0,h1 [B][P][Tqp][256] fp16   zero margins / frames past T_valid[b] = the dilated conv's zero padding
//   xa    [B][P][Tqp][8]   fp16   first layer's input: n_half audio channels, 1 inside the utterance, zeros
//   melp  [B][Tqp][80]     fp16
//   skip  [B][8][P][Tr]    fp32   end rows of the flow, running over its layers (folded end conv + bias)
//   aud   [B][8][L]        fp32   flow variable, natural position order (L = T*P)
//
// Kernels: k16_mel_pad, k16_mel_cvt, k16_noise, k16_begin (sigma*z, start conv of the last flow), k16_wn_layer<LAST, NCB, SEED>
// (one fused WN layer per launch), k16_cond_seed (the conditioning chunks of every layer ahead of time), k16_flow_end (affine inverse, W^-1, early z, next start conv or the final interleave).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "facppg_wg_internal.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

namespace facppg {

struct Wg16State {
  int P, kc, kcp;
  const u32x4* wconv[MAXF][8];   // gate GEMM, convolution part: [48 K steps][8 waves][2][64] (first layer: the folded taps, 4 K steps)
  const u32x4* wcond[MAXF][8];   // gate GEMM, folded conditioning: [P][kcp/16][8][2][64]
  const u32x4* wres[MAXF][8];    // res rows of a non-last res_skip conv: [16][8][64]; null for the last layer
  const u32x4* wend[MAXF][8];    // end rows (W_end . skip rows), padded to 32 rows: [16][64]
  const float *b1[MAXF][8], *b2[MAXF][8];
  const float *endb[MAXF], *start_w[MAXF], *start_b[MAXF], *winv[MAXF];
};

namespace {

constexpr int ZP = C + 8;     // gated-activation tile: halfs per column (16-byte pad)
constexpr int SP = 64 + 8;    // staged K chunk: halfs per column
constexpr int TWMAX = 128;    // widest tile; frame rows are padded to a multiple of it

__device__ __forceinline__ h16x8 as_h8(u32x4 v) { return __builtin_bit_cast(h16x8, v); }
__device__ __forceinline__ u32x4 as_u4(h16x8 v) { return __builtin_bit_cast(u32x4, v); }
__device__ __forceinline__ f32x16 mfma16(u32x4 a, h16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), b, c, 0, 0, 0);
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

// Gate image: u32x4 ((KS*8 + w)*2 + m)*64 + lane = 8 halfs of row m*256 + 32w + lane&31, K = 16 KS + 8(lane>>5) + e
// (the A operand of v_mfma_f32_32x32x16_f16 for wave w's tanh (m = 0) / sigmoid (m = 1) rows).
__global__ void k16_pack_gate(const float* __restrict__ src, u32x4* __restrict__ dst, int nks) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nks * 1024) return;
  const int lane = t & 63, m = (t >> 6) & 1, w = (t >> 7) & 7, KS = t >> 10;
  const int o = m * C + 32 * w + (lane & 31), K = 16 * KS + 8 * (lane >> 5);
  h16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (_Float16)pm_get(src, o, K + e);
  dst[t] = as_u4(v);
}
// res rows: u32x4 (ks*8 + w)*64 + lane = row 32w + lane&31, K = 16 ks + 8(lane>>5) + e
__global__ void k16_pack_res(const float* __restrict__ src, u32x4* __restrict__ dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 16 * 512) return;
  const int lane = t & 63, w = (t >> 6) & 7, ks = t >> 9;
  h16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (_Float16)w2_get(src, 32 * w + (lane & 31), 16 * ks + 8 * (lane >> 5) + e);
  dst[t] = as_u4(v);
}
// end rows: u32x4 ks*64 + lane = row lane&31 (rows >= 2*n_half are zero), K = 16 ks + 8(lane>>5) + e
__global__ void k16_pack_end(const float* __restrict__ src, u32x4* __restrict__ dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 16 * 64) return;
  const int lane = t & 63, ks = t >> 6;
  h16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (_Float16)we_get(src, lane & 31, 16 * ks + 8 * (lane >> 5) + e);
  dst[t] = as_u4(v);
}

// ------------------------------------------------------------------------------------------
// Inputs: mel, noise
// ------------------------------------------------------------------------------------------
// mel [B][80][T] fp16 -> melp [B][Tqp][80], zero outside each utterance's valid frames
__global__ void k16_mel_pad(const _Float16* __restrict__ mel, _Float16* __restrict__ melp, const int* __restrict__ t_valid, int T,
                            int Tqp) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (idx >= Tqp * NMEL) return;
  const int x = idx / NMEL, m = idx % NMEL, q = x - HQ, Tb = t_valid ? t_valid[b] : T;
  melp[(size_t)b * Tqp * NMEL + idx] = (q >= 0 && q < Tb) ? mel[((size_t)b * NMEL + m) * T + q] : (_Float16)0.0f;
}

// the draws of facppg_wg.hip's k_noise (Philox4x32-10 + Box-Muller, same counters and key), rounded to fp16
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__global__ void k16_noise(_Float16* __restrict__ z, size_t n, uint64_t seed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * i >= n) return;
  uint32_t r[4];
  philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  float o[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(r[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(r[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.28318530717958647692f * u2, &sn, &cs);
    o[2 * h] = rad * cs; o[2 * h + 1] = rad * sn;
  }
  for (int j = 0; j < 4; ++j)
    if (4 * i + j < n) z[4 * i + j] = (_Float16)o[j];
}

// ------------------------------------------------------------------------------------------
// k16_wn_layer<LAST, NCB>: one WN layer on a tile of TW = 32*NCB frames of one phase of one utterance, all 512 gate rows.
// 8 waves; wave w owns channels 32w..32w+31: their tanh and sigmoid rows of the gate GEMM (so the gate is formed in
// registers), then rows 32w..32w+31 of the res GEMM.
//   gate GEMM: [512 x K] x [K x TW], K = 3*256 taps (first layer: 64, the folded taps of xa) + kcp conditioning rows,
//              in chunks of 64 staged into LDS as [column][k] fp16 (double-buffered, one barrier per chunk); A fragments
//              straight from the packed image (1 KiB per wave and K step), one chunk ahead in registers
//   gate:      z = tanh(a) * sigmoid(b) in fp32, rounded to fp16 into an LDS tile [column][256]
//   res GEMM:  [256 x 256] x [256 x TW] from that tile; h_out = h_in + res + bias (fp32 sum, rounded once)
//   end rows:  wave w multiplies its own 32 channels by the folded end rows (32-row padded A), the eight partials are
//              summed in wave order and added to the running skip rows (first layer: + the folded end bias)
// Every output column is computed the same way in every tile width (same K order, same wave-order sum), so an utterance
// gets the same bits in any batch and any tile width.  The K order is a run-time argument (cond_first): taps then conditioning
// (the default), or conditioning first -- the order in which a tile may start from k16_cond_seed's accumulators instead of
// running the conditioning chunks itself (SEED launches, 32-frame tiles: seeded or not, a column gets the same bits).
// ------------------------------------------------------------------------------------------
struct Wn16Args {
  const _Float16* h_in;
  _Float16* h_out;
  const _Float16* xa;
  const _Float16* melp;
  float* skip;
  const u32x4 *wconv, *wcond, *wres, *wend;
  const float *b1, *b2, *endb;
  const int* t_valid;
  int T, P, Tr, Tqp, dil, first, nconv, ncond, kc;
  int cond_first;        // K order: 0 = taps, then conditioning (the default); 1 = conditioning first (what a seed can stand for)
  const float4* seeds;   // SEED launches: this (flow, layer)'s [P][seed_nt][8 waves][2][4][64 lanes] accumulators (k16_cond_seed)
  int seed_nt, seed_tiles;   // tiles per phase row of the seed buffer; tiles [0, seed_tiles) of the launch start from their seeds
};

template <int NCB>
constexpr int wn16_lds_bytes() { return 32 * NCB * (ZP + 2 * SP) * 2; }

template <bool LAST, int NCB, bool SEED = false>
__global__ __launch_bounds__(512, 1) void k16_wn_layer(Wn16Args p) {
  static_assert(!SEED || NCB == 1, "seeds are kept per 32-frame tile");
  constexpr int TW = 32 * NCB;
  constexpr int NV = (8 * TW + 511) / 512;   // staged 16-byte vectors per thread and chunk
  extern __shared__ __align__(16) char smem[];
  _Float16* zt = (_Float16*)smem;            // [TW][ZP]
  _Float16* stg = zt + TW * ZP;              // [2][TW][SP]
  float* ends = (float*)stg;                 // [8 waves][8 rows][TW], after the K loop
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
  // The K order is an index mapping of the chunk counter: step c of the loop runs chunk kmap(c).  Tap-first is the identity;
  // conditioning-first runs the ncond conditioning chunks (in their own order) from zero, then the taps.  A seeded tile of a
  // SEED launch starts at step ncond from k16_cond_seed's accumulators -- the registers those first steps would have left.
  const bool cfirst = SEED || p.cond_first != 0;
  const bool seeded = SEED && (int)blockIdx.x < p.seed_tiles;
  const int c_lo = seeded ? p.ncond : 0;
  auto kmap = [&](int c) __attribute__((always_inline)) { return cfirst ? (c < p.ncond ? c + p.nconv : c - p.ncond) : c; };
  const size_t hrow = (size_t)b * P;   // (b, phase) row base of h / xa, in units of Tqp frames
  auto load_stage = [&](int c, u32x4 (&sr)[NV]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + 512 * i, col = v >> 3, kv = v & 7;
      u32x4 val = {0u, 0u, 0u, 0u};
      if (v < 8 * TW) {
        const int q = q0 + col;
        if (c < p.nconv) {
          if (p.first) {
            if (kv < 3)
              val = *(const u32x4*)(p.xa + ((hrow + php[kv]) * p.Tqp + HQ + q + qs[kv]) * 8);
          } else {
            const int t = c >> 2, c0 = 64 * (c & 3) + 8 * kv;
            val = *(const u32x4*)(p.h_in + ((hrow + php[t]) * p.Tqp + HQ + q + qs[t]) * C + c0);
          }
        } else {
          const int kk = 64 * (c - p.nconv) + 8 * kv;
          if (kk < p.kc) {
            const int j = kk / NMEL, m = kk % NMEL;
            val = *(const u32x4*)(p.melp + ((size_t)b * p.Tqp + HQ + q - j) * NMEL + m);
          }
        }
      }
      sr[i] = val;
    }
  };
  auto store_stage = [&](int buf, const u32x4 (&sr)[NV]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + 512 * i, col = v >> 3, kv = v & 7;
      if (v < 8 * TW) *(u32x4*)(stg + (buf * TW + col) * SP + 8 * kv) = sr[i];
    }
  };
  const int ncks = 4 * p.ncond;
  auto load_a = [&](int c, u32x4 (&ar)[4][2]) __attribute__((always_inline)) {
    const u32x4* base = c < p.nconv ? p.wconv + (size_t)(4 * c) * 1024 : p.wcond + ((size_t)ph * ncks + 4 * (c - p.nconv)) * 1024;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int m = 0; m < 2; ++m) ar[kk][m] = base[((kk * 8 + w) * 2 + m) * 64 + lane];
  };

  f32x16 acc[2][NCB];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
  u32x4 sr[NV], ar[4][2], an[4][2];
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
    const _Float16* sb = stg + ((c - c_lo) & 1) * TW * SP;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int n = 0; n < NCB; ++n) {
        const h16x8 bf = *(const h16x8*)(sb + (32 * n + lr) * SP + 16 * kk + 8 * hf);
        acc[0][n] = mfma16(ar[kk][0], bf, acc[0][n]);
        acc[1][n] = mfma16(ar[kk][1], bf, acc[1][n]);
      }
    if (c + 1 < nch) store_stage((c + 1 - c_lo) & 1, sr);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int m = 0; m < 2; ++m) ar[kk][m] = an[kk][m];
  }

  // gate (fp32) -> fp16 tile.  Accumulator register r of lane (lr, hf) is row (r&3) + 8(r>>2) + 4hf, column lr.
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int ch = 32 * w + 8 * g + 4 * hf;
    const float4 bt = *(const float4*)(p.b1 + ch), bs = *(const float4*)(p.b1 + C + ch);
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
      h16x4 v;
      v[0] = (_Float16)gate_tanh_sigmoid(acc[0][n][4 * g + 0] + bt.x, acc[1][n][4 * g + 0] + bs.x);
      v[1] = (_Float16)gate_tanh_sigmoid(acc[0][n][4 * g + 1] + bt.y, acc[1][n][4 * g + 1] + bs.y);
      v[2] = (_Float16)gate_tanh_sigmoid(acc[0][n][4 * g + 2] + bt.z, acc[1][n][4 * g + 2] + bs.z);
      v[3] = (_Float16)gate_tanh_sigmoid(acc[0][n][4 * g + 3] + bt.w, acc[1][n][4 * g + 3] + bs.w);
      *(h16x4*)(zt + (32 * n + lr) * ZP + ch) = v;
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
      const u32x4 a = p.wend[ks * 64 + lane];
#pragma unroll
      for (int n = 0; n < NCB; ++n) e[n] = mfma16(a, *(const h16x8*)(zt + (32 * n + lr) * ZP + 16 * ks + 8 * hf), e[n]);
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
    u32x4 a = p.wres[w * 64 + lane];
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
      const u32x4 a_next = p.wres[(((ks + 1) & 15) * 8 + w) * 64 + lane];
#pragma unroll
      for (int n = 0; n < NCB; ++n) r2[n] = mfma16(a, *(const h16x8*)(zt + (32 * n + lr) * ZP + 16 * ks + 8 * hf), r2[n]);
      a = a_next;
    }
    // residual: h_out = h_in + res + bias, four consecutive channels per access
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
      const int q = q0 + 32 * n + lr;
      if (q >= Tb) continue;
      const size_t off = ((hrow + ph) * p.Tqp + HQ + q) * C;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = 32 * w + 8 * g + 4 * hf;
        const float4 bb = *(const float4*)(p.b2 + ch);
        const h16x4 hi = *(const h16x4*)(p.h_in + off + ch);
        h16x4 ho;
        ho[0] = (_Float16)((float)hi[0] + (r2[n][4 * g + 0] + bb.x));
        ho[1] = (_Float16)((float)hi[1] + (r2[n][4 * g + 1] + bb.y));
        ho[2] = (_Float16)((float)hi[2] + (r2[n][4 * g + 2] + bb.z));
        ho[3] = (_Float16)((float)hi[3] + (r2[n][4 * g + 3] + bb.w));
        *(h16x4*)(p.h_out + off + ch) = ho;
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
// k16_cond_seed: the conditioning chunks of every (flow, layer, phase) gate GEMM for a block of BT 32-frame tiles of ONE
// utterance, ahead of the layers (WN.forward's cond_layers, glow.py:154-175, on the upsampled mel, glow.py:253-259).
// The staged window is k16_wn_layer's load_stage for its conditioning chunks (zeros for kk >= kc), the A fragments are the same
// u32x4 of wcond, and every chunk issues the same mfma16 sequence from zero accumulators: the registers parked in the seed
// buffer are those a conditioning-first k16_wn_layer holds after its first ncond steps, bit for bit.  No bias (it stays at
// the gate).  The window depends on the frames alone: it is staged once per block ([ncond][32 BT][SP] halfs) and stays in
// LDS while the workgroup streams one 320 KiB (hop 256) weight image after the other past it -- 1.0 GB per pass.
// Work item = (group of lpw layers, phase, block), block-major so that a workgroup restages only when its block changes.
// ------------------------------------------------------------------------------------------
struct Seed16Args {
  const _Float16* melp;             // [Tqp][80] zero-margined mel frames
  float4* seeds;                    // [layers_total][P][seed_nt][8][2][4][64]
  const u32x4* wcond[MAXF * 8];     // per (flow, layer): [P][4 ncond][8][2][64]
  int lpw, P, Tr, seed_nt;
  int tile0, tile1, nblk;           // tiles [tile0, tile1) in nblk blocks of BT
  int ncond, kc;
  int layer0, layer1, items;
  const int* skip;                  // optional (device): *skip != 0 -> the launch does nothing
  int* counter;                     // bounded launch: hands out the items past the first gridDim (zero at launch), or null: strided
};

template <int BT>
__global__ __launch_bounds__(512) void k16_cond_seed(Seed16Args p) {
  constexpr int TW = 32 * BT;
  extern __shared__ __align__(16) char smem[];
  _Float16* win = (_Float16*)smem;   // [ncond][TW][SP]
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
        u32x4 val = {0u, 0u, 0u, 0u};
        if (kk < p.kc && q < p.Tr) {
          const int j = kk / NMEL, m = kk % NMEL;
          val = *(const u32x4*)(p.melp + ((size_t)HQ + q - j) * NMEL + m);
        }
        *(u32x4*)(win + (c * TW + col) * SP + 8 * kv) = val;
      }
      __syncthreads();
      cur_blk = blk;
    }
    const int l0 = p.layer0 + lg * p.lpw, l1 = min(l0 + p.lpw, p.layer1);
    for (int l = l0; l < l1; ++l) {
      const u32x4* img = p.wcond[l] + (size_t)ph * ncks * 1024 + w * 128 + lane;   // ((kk*8 + w)*2 + m)*64 + lane of K step kk
      f32x16 acc[2][BT];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < BT; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
      u32x4 ar[4][2], an[4][2];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int m = 0; m < 2; ++m) ar[kk][m] = __builtin_nontemporal_load(img + kk * 1024 + m * 64);
      for (int c = 0; c < p.ncond; ++c) {
        const int cn = c + 1 < p.ncond ? c + 1 : c;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int m = 0; m < 2; ++m) an[kk][m] = __builtin_nontemporal_load(img + (size_t)(4 * cn + kk) * 1024 + m * 64);
        const _Float16* sb = win + c * TW * SP;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int n = 0; n < BT; ++n) {
            const h16x8 bf = *(const h16x8*)(sb + (32 * n + lr) * SP + 16 * kk + 8 * hf);
            acc[0][n] = mfma16(ar[kk][0], bf, acc[0][n]);
            acc[1][n] = mfma16(ar[kk][1], bf, acc[1][n]);
          }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int m = 0; m < 2; ++m) ar[kk][m] = an[kk][m];
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

// frames [f0, f0 + n) of an fp32 mel [80][ld] (the streaming postnet's output) -> the zero-margined fp16 [Tqp][80] layout,
// rounded to nearest even as tensor.half() does
__global__ void k16_mel_cvt(const float* __restrict__ mel, int ld, _Float16* __restrict__ melp, int f0, int n, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * NMEL) return;
  const int m = idx / n, q = f0 + idx % n;
  melp[((size_t)HQ + q) * NMEL + m] = (_Float16)mel[(size_t)m * ld + q];
}

// ------------------------------------------------------------------------------------------
// Flow edges: 8 positions per 256-thread workgroup, 32 threads per position (8 start-conv channels each: one 16-byte
// store, a position's 512-byte h row written by 32 consecutive lanes).  grid = (ceil(T/8), B, P).
// ------------------------------------------------------------------------------------------
struct Edge16Args {
  const float* skip;
  const float* aud_in;
  float* aud_out;
  _Float16* h_out;
  _Float16* xa;
  _Float16* audio;          // [B][T*hop]
  const _Float16* z0;       // [B][2*HN][L]
  const _Float16* z_early;  // [B][2][L] or null
  const float *winv, *start_w, *start_b;
  const int* t_valid;
  float sigma;
  int T, P, Tr, Tqp, L, swap, swap_next, final_flow;
};

__device__ __forceinline__ bool edge16_pos(const Edge16Args& p, int& b, int& q, int& pos, int& cg) {
  b = blockIdx.y;
  q = blockIdx.x * 8 + (threadIdx.x >> 5);
  cg = threadIdx.x & 31;
  const int Tb = p.t_valid ? p.t_valid[b] : p.T;
  pos = q * p.P + blockIdx.z;
  return q < Tb;
}

// start conv (channels 8cg..8cg+7) of the flow whose conditioning channels are a0[0..HN), and (cg == 0) its xa row
template <int HN>
__device__ __forceinline__ void start16(const Edge16Args& p, int b, int q, int cg, const float* a0) {
  const size_t row = ((size_t)b * p.P + blockIdx.z) * p.Tqp + HQ + q;
  h16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ch = 8 * cg + e;
    float s = p.start_b[ch];
#pragma unroll
    for (int j = 0; j < HN; ++j) s = fmaf(p.start_w[ch * HN + j], a0[j], s);
    v[e] = (_Float16)s;
  }
  *(h16x8*)(p.h_out + row * C + 8 * cg) = v;
  if (cg == 0) {
    h16x8 x;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (_Float16)(j < HN ? a0[j] : j == HN ? 1.0f : 0.0f);
    *(h16x8*)(p.xa + row * 8) = x;
  }
}

template <int HN>
__global__ __launch_bounds__(256) void k16_begin(Edge16Args p) {
  int b, q, pos, cg;
  if (!edge16_pos(p, b, q, pos, cg)) return;
  float a[2 * HN];
#pragma unroll
  for (int j = 0; j < 2 * HN; ++j) {
    a[j] = p.sigma * (float)p.z0[((size_t)b * 2 * HN + j) * p.L + pos];
    if (cg == 0) p.aud_out[((size_t)b * 8 + j) * p.L + pos] = a[j];
  }
  start16<HN>(p, b, q, cg, a + (p.swap_next ? HN : 0));
}

template <int H, bool EARLY>
__global__ __launch_bounds__(256) void k16_flow_end(Edge16Args p) {
  constexpr int CC = 2 * H, CN = EARLY ? CC + 2 : CC;
  int b, q, pos, cg;
  if (!edge16_pos(p, b, q, pos, cg)) return;
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
    for (int j = 0; j < 2; ++j) y[j] = p.sigma * (float)p.z_early[((size_t)b * 2 + j) * p.L + pos];
  }
#pragma unroll
  for (int i = 0; i < CC; ++i) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < CC; ++j) v = fmaf(p.winv[i * CC + j], a[j], v);
    y[(EARLY ? 2 : 0) + i] = v;
  }
  if (p.final_flow) {
    if (cg < CN) p.audio[(size_t)b * p.T * p.P * 8 + (size_t)pos * CN + cg] = (_Float16)y[cg];   // glow.py:292 interleave
    return;
  }
  if (cg == 0) {
#pragma unroll
    for (int j = 0; j < CN; ++j) p.aud_out[((size_t)b * 8 + j) * p.L + pos] = y[j];
  }
  start16<CN / 2>(p, b, q, cg, y + (p.swap_next ? CN / 2 : 0));
}

struct Ws16 {
  int P, L, Tr, Tqp;
  size_t h0, h1, xa, melp, skip, aud0, aud1, z, total;
};
Ws16 ws16_layout(const facppg_wg_config& c, int B, int T) {
  Ws16 w;
  w.P = c.hop_length / 8;
  w.L = T * w.P;
  w.Tr = round_up(T, TWMAX);
  w.Tqp = HQ + w.Tr + HQ;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.h0 = take((size_t)B * w.P * w.Tqp * C * 2);
  w.h1 = take((size_t)B * w.P * w.Tqp * C * 2);
  w.xa = take((size_t)B * w.P * w.Tqp * 8 * 2);   // right behind h0 | h1: one memset zeroes all three
  w.melp = take((size_t)B * w.Tqp * NMEL * 2);
  w.skip = take((size_t)B * 8 * w.P * w.Tr * 4);
  w.aud0 = take((size_t)B * 8 * w.L * 4);
  w.aud1 = take((size_t)B * 8 * w.L * 4);
  w.z = take(((size_t)B * 8 * w.L + 4) * 2);
  w.total = off;
  return w;
}

template <int H>
void launch_flow_end16(bool early, dim3 grid, hipStream_t s, const Edge16Args& a) {
  if (early) k16_flow_end<H, true><<<grid, 256, 0, s>>>(a);
  else k16_flow_end<H, false><<<grid, 256, 0, s>>>(a);
}

}  // namespace

size_t wg16_workspace_bytes(const facppg_wg* h, int B, int T) { return ws16_layout(h->cfg, B, T).total; }

void wg16_destroy(facppg_wg* h) {
  delete h->w16;
  h->w16 = nullptr;
}

}  // namespace facppg

using namespace facppg;

extern "C" int facppg_wg_create_f16(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats, int device,
                                    void* stream_, facppg_wg** out) {
  FACPPG_REQUIRE(out, FACPPG_EINVAL, "out is NULL");
  // the fp32 handle folds the blob (upsampler into the conditioning, end conv through the skip rows, first taps through
  // start); its images are read back here and rounded to fp16 once
  facppg_wg* f = nullptr;
  if (int rc = facppg_wg_create(cfg, weights_dev, n_floats, device, stream_, &f)) return rc;
  hipStream_t s = (hipStream_t)stream_;
  const facppg_wg_config& c = f->cfg;
  const int P = f->P, kcp = f->kcp, nl = c.wn_layers, nf = c.n_flows;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  struct Off { size_t wconv[8], wcond[8], wres[8], wend[8], b1[8], b2[8], endb, start_w, start_b, winv; } fo[MAXF];
  for (int k = 0; k < nf; ++k) {
    const size_t hh = f->n_half[k], cc = 2 * hh;
    for (int i = 0; i < nl; ++i) {
      fo[k].wconv[i] = take((size_t)(i == 0 ? 4 : 48) * 1024 * 16);
      fo[k].wcond[i] = take((size_t)P * (kcp / 16) * 1024 * 16);
      fo[k].wres[i] = i == nl - 1 ? 0 : take((size_t)16 * 512 * 16);
      fo[k].wend[i] = take((size_t)16 * 64 * 16);
      fo[k].b1[i] = take(2 * C * 4);
      fo[k].b2[i] = take(C * 4);
    }
    fo[k].endb = take(8 * 4); fo[k].start_w = take(C * hh * 4); fo[k].start_b = take(C * 4); fo[k].winv = take(cc * cc * 4);
  }
  facppg_wg* h = new (std::nothrow) facppg_wg();
  Wg16State* st = new (std::nothrow) Wg16State();
  if (!h || !st || hipMalloc((void**)&h->arena, off) != hipSuccess) {
    delete h; delete st;
    facppg_wg_destroy(f);
    set_error("facppg_wg_create_f16: allocating %zu bytes of fp16 images failed", off);
    return FACPPG_EHIP;
  }
  h->cfg = c; h->device = f->device; h->arena_bytes = off; h->n_cu = f->n_cu; h->poll_limit = f->poll_limit; h->ev_layers = 1;
  memcpy(h->n_rem, f->n_rem, sizeof(h->n_rem)); memcpy(h->n_half, f->n_half, sizeof(h->n_half)); memcpy(h->early, f->early, sizeof(h->early));
  h->P = P; h->nj = f->nj; h->kc = f->kc; h->kcp = kcp;
  h->w16 = st;
  st->P = P; st->kc = f->kc; st->kcp = kcp;
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
      k16_pack_gate<<<nks * 4, 256, 0, s>>>(i == 0 ? (const float*)f->w1f[k] : (const float*)f->w1pm[k][i], U(fo[k].wconv[i]), nks);
      k16_pack_gate<<<ncks * 4, 256, 0, s>>>((const float*)f->wcpm[k][i], U(fo[k].wcond[i]), ncks);
      if (!last) k16_pack_res<<<32, 256, 0, s>>>((const float*)f->w2r[k][i], U(fo[k].wres[i]));
      k16_pack_end<<<4, 256, 0, s>>>(f->we[k][i], U(fo[k].wend[i]));
      cpy(fo[k].b1[i], f->b1pm[k][i], 2 * C);
      cpy(fo[k].b2[i], f->b2[k][i], C);
      st->wconv[k][i] = U(fo[k].wconv[i]); st->wcond[k][i] = U(fo[k].wcond[i]);
      st->wres[k][i] = last ? nullptr : U(fo[k].wres[i]); st->wend[k][i] = U(fo[k].wend[i]);
      st->b1[k][i] = F(fo[k].b1[i]); st->b2[k][i] = F(fo[k].b2[i]);
    }
    cpy(fo[k].endb, f->endb[k], 8);
    cpy(fo[k].start_w, f->start_w[k], C * hh);
    cpy(fo[k].start_b, f->start_b[k], C);
    cpy(fo[k].winv, f->winv[k], cc * cc);
    st->endb[k] = F(fo[k].endb); st->start_w[k] = F(fo[k].start_w); st->start_b[k] = F(fo[k].start_b); st->winv[k] = F(fo[k].winv);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // (the fp32 images are read by the packers above)
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k16_wn_layer<false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, wn16_lds_bytes<4>());
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k16_wn_layer<true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, wn16_lds_bytes<4>());
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k16_cond_seed<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k16_cond_seed<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k16_cond_seed<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k16_cond_seed<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  facppg_wg_destroy(f);
  if (e != hipSuccess) {
    set_error("facppg_wg_create_f16: %s", hipGetErrorString(e));
    facppg_wg_destroy(h);
    return FACPPG_EHIP;
  }
  *out = h;
  return FACPPG_OK;
}

// WaveGlow.infer on an fp16 handle.  cond_first: the K order of every layer launch.  melp_ext != null (B = 1): the caller's
// zero-margined fp16 mel buffer laid out, like `seeds`, for T_layout >= T frames; tiles wholly inside [0, seeded_frames) start
// from their seeds, the others run conditioning-first with full K in the same 32-frame-tile launches.
static int wg16_infer(facppg_wg* h, const uint16_t* mel_dev, const int32_t* T_valid_dev, const uint16_t* z_dev, uint64_t seed,
                      float sigma, int B, int T, uint16_t* audio_dev, void* ws_, size_t ws_bytes, void* stream_, int cond_first,
                      const uint16_t* melp_ext = nullptr, const float* seeds_dev = nullptr, int seeded_frames = 0, int T_layout = 0,
                      void* const* flow_events = nullptr) {
  if (!melp_ext) T_layout = T;
  const size_t need = wg16_workspace_bytes(h, B, T_layout);
  FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, need);
  const facppg_wg_config& c = h->cfg;
  const Wg16State& st = *h->w16;
  {
    int tot = h->n_rem[c.n_flows - 1];
    for (int k = 0; k < c.n_flows; ++k) tot += h->early[k] ? c.n_early_size : 0;
    FACPPG_REQUIRE(tot == 8, FACPPG_EUNSUPPORTED, "noise channel count %d != n_group", tot);
  }
  Ws16 w = ws16_layout(c, B, T_layout);   // rows (Tr, Tqp) of the layout; positions of the T frames that are there
  w.L = T * w.P;
  FACPPG_REQUIRE((1 << (c.wn_layers - 1)) / w.P + 1 <= HQ, FACPPG_EUNSUPPORTED, "hop %d: the dilated taps reach past the %d-frame margins",
                 c.hop_length, HQ);
  FACPPG_REQUIRE((double)B * w.P * w.Tqp * C < 2.0e9, FACPPG_EUNSUPPORTED, "B*T = %d*%d frames is too long", B, T);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  _Float16* hbuf[2] = {(_Float16*)(ws + w.h0), (_Float16*)(ws + w.h1)};
  _Float16* xa = (_Float16*)(ws + w.xa);
  const _Float16* melp = melp_ext ? (const _Float16*)melp_ext : (const _Float16*)(ws + w.melp);
  float* skip = (float*)(ws + w.skip);
  float* aud[2] = {(float*)(ws + w.aud0), (float*)(ws + w.aud1)};
  const int nf = c.n_flows;
  FACPPG_HIP_CHECK(hipMemsetAsync(ws + w.h0, 0, w.melp - w.h0, s));   // h0, h1, xa: margins and frames past each utterance
  if (!melp_ext)
    k16_mel_pad<<<dim3((w.Tqp * NMEL + 255) / 256, B), 256, 0, s>>>((const _Float16*)mel_dev, (_Float16*)(ws + w.melp), T_valid_dev, T, w.Tqp);
  const _Float16* z = (const _Float16*)z_dev;
  if (!z) {
    const size_t zn = (size_t)B * 8 * w.L;
    k16_noise<<<(unsigned)((zn / 4 + 255) / 256 + 1), 256, 0, s>>>((_Float16*)(ws + w.z), zn, seed);
    z = (const _Float16*)(ws + w.z);
  }
  // tile width: 128 frames when the launch still gives every CU a couple of workgroups, else narrower (the B = 1 latency
  // shape: 32-frame tiles spread one short utterance over the chip); FACPPG_WG16_TILE = 32 | 64 | 128 forces one
  const long tiles128 = (long)w.P * B * ((T + 127) / 128), tiles64 = (long)w.P * B * ((T + 63) / 64);
  const long ncu = h->n_cu > 0 ? h->n_cu : 256;
  int tw = tiles128 >= 2 * ncu ? 128 : tiles64 >= 2 * ncu ? 64 : 32;
  if (const char* env = getenv("FACPPG_WG16_TILE")) {
    const int v = atoi(env);
    FACPPG_REQUIRE(v == 32 || v == 64 || v == 128, FACPPG_EINVAL, "FACPPG_WG16_TILE=%s: expected 32, 64 or 128", env);
    tw = v;
  }
  if (melp_ext) tw = 32;   // seeds are kept per 32-frame tile
  const dim3 lgrid((T + tw - 1) / tw, B, w.P);
  h->last_tile = tw; h->last_waves = 8; h->last_tiles = (int)(lgrid.x * lgrid.y * lgrid.z);

  Edge16Args e;
  memset(&e, 0, sizeof(e));
  e.skip = skip; e.xa = xa; e.audio = (_Float16*)audio_dev; e.t_valid = T_valid_dev; e.sigma = sigma;
  e.T = T; e.P = w.P; e.Tr = w.Tr; e.Tqp = w.Tqp; e.L = w.L;
  const dim3 egrid((T + 7) / 8, B, w.P);
  int ai = 0, hi = 0;
  {
    const int k = nf - 1;
    e.z0 = z; e.aud_out = aud[ai]; e.h_out = hbuf[hi]; e.start_w = st.start_w[k]; e.start_b = st.start_b[k];
    e.swap_next = c.alternate_halves && (k & 1);
    switch (h->n_half[k]) {
      case 1: k16_begin<1><<<egrid, 256, 0, s>>>(e); break;
      case 2: k16_begin<2><<<egrid, 256, 0, s>>>(e); break;
      case 3: k16_begin<3><<<egrid, 256, 0, s>>>(e); break;
      case 4: k16_begin<4><<<egrid, 256, 0, s>>>(e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
  }
  size_t z_off = (size_t)B * h->n_rem[nf - 1] * w.L;
  Wn16Args a;
  memset(&a, 0, sizeof(a));
  a.xa = xa; a.melp = melp; a.skip = skip; a.t_valid = T_valid_dev;
  a.T = T; a.P = w.P; a.Tr = w.Tr; a.Tqp = w.Tqp; a.kc = st.kc; a.ncond = st.kcp / 64;
  a.cond_first = cond_first; a.seed_nt = w.Tr / 32; a.seed_tiles = melp_ext ? std::min(seeded_frames, round_up(T, 32)) / 32 : 0;
  for (int k = nf - 1; k >= 0; --k) {
    if (flow_events && flow_events[k]) FACPPG_HIP_CHECK(hipStreamWaitEvent(s, (hipEvent_t)flow_events[k], 0));
    a.endb = st.endb[k];
    for (int i = 0; i < c.wn_layers; ++i) {
      if (melp_ext) a.seeds = (const float4*)seeds_dev + (size_t)(k * c.wn_layers + i) * w.P * a.seed_nt * 4096;
      const bool last = i == c.wn_layers - 1;
      a.h_in = hbuf[hi]; a.h_out = hbuf[hi ^ 1];
      a.wconv = st.wconv[k][i]; a.wcond = st.wcond[k][i]; a.wres = st.wres[k][i]; a.wend = st.wend[k][i];
      a.b1 = st.b1[k][i]; a.b2 = st.b2[k][i];
      a.dil = 1 << i; a.first = i == 0; a.nconv = i == 0 ? 1 : 12;
#define WN16_LAUNCH(NCB)                                                                              \
  do {                                                                                                \
    if (last) k16_wn_layer<true, NCB><<<lgrid, 512, wn16_lds_bytes<NCB>(), s>>>(a);                   \
    else k16_wn_layer<false, NCB><<<lgrid, 512, wn16_lds_bytes<NCB>(), s>>>(a);                       \
  } while (0)
      if (melp_ext) {
        if (last) k16_wn_layer<true, 1, true><<<lgrid, 512, wn16_lds_bytes<1>(), s>>>(a);
        else k16_wn_layer<false, 1, true><<<lgrid, 512, wn16_lds_bytes<1>(), s>>>(a);
      } else if (tw == 128) WN16_LAUNCH(4);
      else if (tw == 64) WN16_LAUNCH(2);
      else WN16_LAUNCH(1);
#undef WN16_LAUNCH
      if (!last) hi ^= 1;
    }
    e.aud_in = aud[ai]; e.aud_out = aud[ai ^ 1]; e.h_out = hbuf[hi];
    e.winv = st.winv[k];
    e.final_flow = k == 0;
    e.swap = c.alternate_halves && (k & 1);
    e.swap_next = c.alternate_halves && k > 0 && ((k - 1) & 1);
    e.z_early = nullptr;
    if (h->early[k]) { e.z_early = z + z_off; z_off += (size_t)B * c.n_early_size * w.L; }
    if (k > 0) { e.start_w = st.start_w[k - 1]; e.start_b = st.start_b[k - 1]; }
    const int cn = 2 * h->n_half[k] + (h->early[k] ? 2 : 0);
    if (k > 0) FACPPG_REQUIRE(cn == 2 * h->n_half[k - 1], FACPPG_EUNSUPPORTED, "flow %d channel mismatch", k);
    else FACPPG_REQUIRE(cn == 8, FACPPG_EUNSUPPORTED, "final flow must yield n_group channels");
    switch (h->n_half[k]) {
      case 1: launch_flow_end16<1>(h->early[k], egrid, s, e); break;
      case 2: launch_flow_end16<2>(h->early[k], egrid, s, e); break;
      case 3: launch_flow_end16<3>(h->early[k], egrid, s, e); break;
      case 4: launch_flow_end16<4>(h->early[k], egrid, s, e); break;
      default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", h->n_half[k]);
    }
    ai ^= 1;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

static int wg16_infer_checks(const char* fn, facppg_wg* h, const void* mel, const void* audio, const void* ws, int B, int T) {
  FACPPG_REQUIRE(h && mel && audio && ws, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(h->w16, FACPPG_EINVAL, "%s: the handle holds fp32 images (facppg_wg_create); use the fp32 entry point, or make it with facppg_wg_create_f16", fn);
  FACPPG_REQUIRE(B > 0 && T > 0, FACPPG_EINVAL, "B and T must be positive (got %d, %d)", B, T);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EINVAL, "B too large");
  return FACPPG_OK;
}

extern "C" int facppg_wg_infer_f16(facppg_wg* h, const uint16_t* mel_dev, const int32_t* T_valid_dev, const uint16_t* z_dev,
                                   uint64_t seed, float sigma, int B, int T, uint16_t* audio_dev, void* ws_, size_t ws_bytes,
                                   void* stream_) {
  if (int rc = wg16_infer_checks("facppg_wg_infer_f16", h, mel_dev, audio_dev, ws_, B, T)) return rc;
  return wg16_infer(h, mel_dev, T_valid_dev, z_dev, seed, sigma, B, T, audio_dev, ws_, ws_bytes, stream_, 0);
}

extern "C" int facppg_wg_infer_f16_order(facppg_wg* h, const uint16_t* mel_dev, const int32_t* T_valid_dev, const uint16_t* z_dev,
                                         uint64_t seed, float sigma, int B, int T, int cond_first, uint16_t* audio_dev, void* ws_,
                                         size_t ws_bytes, void* stream_) {
  if (int rc = wg16_infer_checks("facppg_wg_infer_f16_order", h, mel_dev, audio_dev, ws_, B, T)) return rc;
  FACPPG_REQUIRE(cond_first == 0 || cond_first == 1, FACPPG_EINVAL, "cond_first must be 0 or 1 (got %d)", cond_first);
  return wg16_infer(h, mel_dev, T_valid_dev, z_dev, seed, sigma, B, T, audio_dev, ws_, ws_bytes, stream_, cond_first);
}

#define WG_REQUIRE_FP16(h, fn)                                   \
  FACPPG_REQUIRE(!(h) || (h)->w16, FACPPG_EINVAL,                \
                 fn ": the handle holds fp32 images (facppg_wg_create); use the fp32 entry point of the same name, or make it with facppg_wg_create_f16")

extern "C" int facppg_wg_seed_layout_f16(const facppg_wg* h, int T, int* Tqp, int* margin, size_t* seed_bytes) {
  WG_REQUIRE_FP16(h, "facppg_wg_seed_layout_f16");
  FACPPG_REQUIRE(h && T > 0 && Tqp && margin && seed_bytes, FACPPG_EINVAL, "NULL argument or T <= 0");
  const Ws16 w = ws16_layout(h->cfg, 1, T);
  *Tqp = w.Tqp; *margin = HQ;
  *seed_bytes = (size_t)h->cfg.n_flows * h->cfg.wn_layers * w.P * (w.Tr / 32) * 4096 * sizeof(float4);
  return FACPPG_OK;
}

extern "C" int facppg_wg_mel_pad_f16(const facppg_wg* h, const float* mel_dev, int T, int ld, int frame0, int nframes,
                                     uint16_t* melp_dev, const int32_t* skip_dev, void* stream_) {
  WG_REQUIRE_FP16(h, "facppg_wg_mel_pad_f16");
  FACPPG_REQUIRE(h && mel_dev && melp_dev && T > 0, FACPPG_EINVAL, "NULL argument or T <= 0");
  const Ws16 w = ws16_layout(h->cfg, 1, T);
  FACPPG_REQUIRE(frame0 >= 0 && nframes >= 0 && frame0 + nframes <= w.Tr && frame0 + nframes <= ld, FACPPG_EINVAL,
                 "frames [%d, %d) do not lie inside the %d padded frames and the row length %d", frame0, frame0 + nframes, w.Tr, ld);
  if (nframes == 0) return FACPPG_OK;
  k16_mel_cvt<<<(nframes * NMEL + 255) / 256, 256, 0, (hipStream_t)stream_>>>(mel_dev, ld, (_Float16*)melp_dev, frame0, nframes, skip_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_cond_seed_f16(facppg_wg* h, const uint16_t* melp_dev, int T, int frame0, int nframes, int block_tiles,
                                       int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                                       const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream_) {
  WG_REQUIRE_FP16(h, "facppg_wg_cond_seed_f16");
  FACPPG_REQUIRE(h && melp_dev && seeds_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0, FACPPG_EINVAL, "T must be positive (got %d)", T);
  const facppg_wg_config& c = h->cfg;
  const Wg16State& st = *h->w16;
  const Ws16 w = ws16_layout(c, 1, T);
  size_t need = 0; int tqp = 0, mg = 0;
  facppg_wg_seed_layout_f16(h, T, &tqp, &mg, &need);
  FACPPG_REQUIRE(seed_bytes >= need, FACPPG_EWORKSPACE, "seed buffer has %zu bytes, need %zu", seed_bytes, need);
  FACPPG_REQUIRE(frame0 >= 0 && frame0 % 32 == 0 && nframes > 0 && frame0 + nframes <= w.Tr, FACPPG_EINVAL,
                 "frames [%d, %d): the first must be a multiple of 32 and the range inside the %d padded frames", frame0, frame0 + nframes, w.Tr);
  FACPPG_REQUIRE(block_tiles >= 1 && block_tiles <= 4 && layers_per_workgroup >= 1, FACPPG_EINVAL, "block_tiles in 1..4, layers_per_workgroup >= 1");
  if (nflows <= 0) { flow0 = 0; nflows = c.n_flows; }
  FACPPG_REQUIRE(flow0 >= 0 && flow0 + nflows <= c.n_flows, FACPPG_EINVAL, "flows [%d, %d) of %d", flow0, flow0 + nflows, c.n_flows);
  FACPPG_REQUIRE(c.n_flows * c.wn_layers <= MAXF * 8, FACPPG_EUNSUPPORTED, "too many layers");
  Seed16Args a;
  memset(&a, 0, sizeof(a));
  a.melp = (const _Float16*)melp_dev; a.seeds = (float4*)seeds_dev; a.skip = skip_dev;
  for (int k = 0; k < c.n_flows; ++k)
    for (int i = 0; i < c.wn_layers; ++i) a.wcond[k * c.wn_layers + i] = st.wcond[k][i];
  a.lpw = layers_per_workgroup; a.P = w.P; a.Tr = w.Tr; a.seed_nt = w.Tr / 32;
  const int ntiles = (nframes + 31) / 32;
  a.tile0 = frame0 / 32; a.tile1 = a.tile0 + ntiles; a.nblk = (ntiles + block_tiles - 1) / block_tiles;
  a.ncond = st.kcp / 64; a.kc = st.kc;
  a.layer0 = flow0 * c.wn_layers; a.layer1 = (flow0 + nflows) * c.wn_layers;
  a.items = (a.layer1 - a.layer0 + a.lpw - 1) / a.lpw * w.P * a.nblk;
  size_t lds = (size_t)a.ncond * 32 * block_tiles * SP * 2;
  FACPPG_REQUIRE(lds <= 160 * 1024 - 64, FACPPG_EUNSUPPORTED, "block_tiles = %d needs %zu bytes of LDS", block_tiles, lds);
  // a BOUNDED launch (the caller shares the GPU with other streams) asks for a CU's whole LDS per workgroup, as
  // facppg_wg_cond_seed does: one workgroup per CU and no other stream's small workgroups next to it
  const int max_wgs = max_workgroups / 8 * 8;
  const bool bounded = max_wgs > 0 && max_wgs < a.items;
  if (max_workgroups > 0) lds = (size_t)160 * 1024 - 64;
  a.counter = bounded ? counter_dev : nullptr;
  const unsigned grid = (unsigned)(bounded ? max_wgs : a.items);
  hipStream_t s = (hipStream_t)stream_;
  switch (block_tiles) {
    case 1: k16_cond_seed<1><<<grid, 512, lds, s>>>(a); break;
    case 2: k16_cond_seed<2><<<grid, 512, lds, s>>>(a); break;
    case 3: k16_cond_seed<3><<<grid, 512, lds, s>>>(a); break;
    default: k16_cond_seed<4><<<grid, 512, lds, s>>>(a); break;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_wg_infer_seeded_f16(facppg_wg* h, const uint16_t* melp_dev, int T_layout, int T, const float* seeds_dev,
                                          int seeded_frames, const uint16_t* z_dev, uint64_t seed, float sigma, uint16_t* audio_dev,
                                          void* ws_, size_t ws_bytes, void* const* flow_events, void* stream_) {
  WG_REQUIRE_FP16(h, "facppg_wg_infer_seeded_f16");
  FACPPG_REQUIRE(h && melp_dev && seeds_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0 && T_layout >= T, FACPPG_EINVAL, "need 0 < T <= T_layout (got %d, %d)", T, T_layout);
  FACPPG_REQUIRE(seeded_frames >= 0 && seeded_frames % 32 == 0 && seeded_frames <= round_up(T, 32), FACPPG_EINVAL,
                 "seeded_frames = %d: expected a multiple of 32 in [0, %d]", seeded_frames, round_up(T, 32));
  return wg16_infer(h, nullptr, nullptr, z_dev, seed, sigma, 1, T, audio_dev, ws_, ws_bytes, stream_, 1, melp_dev, seeds_dev,
                    seeded_frames, T_layout, flow_events);
}
