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
// Kernels here: ks_pack_gate / ks_pack_res / ks_pack_end (create), ks_wn_layer<LAST, NCB, SEED> (one fused WN layer per launch),
// ks_cond_seed<BT> (the conditioning chunks of every layer ahead of time).  The mel and flow-edge kernels (in fp32 here), the
// workspace, image creation, the flow walk and the seeded path's host side are facppg_wg_cc.h's, shared with facppg_wg16.hip; Split
// below is what they need to know of this file.
#include "facppg_wg_cc.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

struct facppg_wg_split {
  facppg_wg_config cfg;
  int device, n_cu;
  int n_rem[facppg::MAXF], n_half[facppg::MAXF], early[facppg::MAXF];
  char* arena;   // one device allocation holding the images
  size_t arena_bytes;
  facppg::CcImages img;
  int last_tile, last_waves, last_tiles;   // shape of the WN layer launches of the most recent infer
};

namespace facppg {
namespace {

constexpr int ZP = C + 8;     // gated-activation tile: bf16 per column and plane (16-byte pad)
constexpr int SP = 64 + 8;    // staged K chunk: bf16 per column and plane

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
using SeedSplitArgs = SeedArgs<float>;

constexpr int SEED_BT_MAX = 3;

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

// what facppg_wg_cc.h needs to know of the split arithmetic
struct Split {
  using E = float;
  using Handle = facppg_wg_split;
  using LayerArgs = WnSplitSeedArgs;   // (an unseeded launch takes its WnSplitArgs part)
  using SeedKernelArgs = SeedSplitArgs;
  static constexpr int planes = 2, tw_max = 64;
  static constexpr const char *create_name = "facppg_wg_split_create", *image_name = "split bf16";
  static constexpr auto pack_gate = ks_pack_gate;
  static constexpr auto pack_res = ks_pack_res;
  static constexpr auto pack_end = ks_pack_end;
  static std::array<KernelLds, 5> lds_attrs() {
    return {{{(const void*)ks_wn_layer<false, 2>, wns_lds_bytes<2>()}, {(const void*)ks_wn_layer<true, 2>, wns_lds_bytes<2>()},
             {(const void*)ks_cond_seed<1>, SEED_LDS_MAX}, {(const void*)ks_cond_seed<2>, SEED_LDS_MAX},
             {(const void*)ks_cond_seed<3>, SEED_LDS_MAX}}};
  }
  static const CcImages& images(const facppg_wg_split* h) { return h->img; }

  // the fp32 path's Philox draw, unrounded
  static void noise(float* z, size_t n, uint64_t seed, hipStream_t s) { wg_launch_noise(z, n, seed, s); }
  // tile width: 64 frames when that still gives every CU a workgroup, else 32 (the B = 1 latency shape: narrow tiles spread one
  // short utterance over the chip); FACPPG_WG_SPLIT_TILE = 32 | 64 forces one
  static int tile(int P, int B, int T, long ncu, int* tw) {
    const long tiles64 = (long)P * B * ((T + 63) / 64);
    *tw = tiles64 >= ncu ? 64 : 32;
    if (const char* env = getenv("FACPPG_WG_SPLIT_TILE")) {
      const int v = atoi(env);
      FACPPG_REQUIRE(v == 32 || v == 64, FACPPG_EINVAL, "FACPPG_WG_SPLIT_TILE=%s: expected 32 or 64", env);
      *tw = v;
    }
    return FACPPG_OK;
  }
  void init_layer_args(WnSplitSeedArgs&) const {}   // the K order is the launch's SEED template argument
  template <int NCB, bool SEED = false>
  static void launch_ncb(const WnSplitSeedArgs& a, bool last, dim3 grid, hipStream_t s) {
    if (last) ks_wn_layer<true, NCB, SEED><<<grid, 512, wns_lds_bytes<NCB>(), s>>>(a);
    else ks_wn_layer<false, NCB, SEED><<<grid, 512, wns_lds_bytes<NCB>(), s>>>(a);
  }
  static void launch_layer(const WnSplitSeedArgs& a, int tw, bool seeded, bool last, dim3 grid, hipStream_t s) {
    if (seeded) launch_ncb<1, true>(a, last, grid, s);
    else if (tw == 64) launch_ncb<2>(a, last, grid, s);
    else launch_ncb<1>(a, last, grid, s);
  }

  static constexpr size_t seed_window_bytes(int ncond, int bt) { return (size_t)ncond * 2 * 32 * bt * SP * 2; }
  // the widest block whose window fits the LDS and whose accumulators fit the registers
  static int max_block_tiles(const CcImages& st) {
    int bt = 0;
    while (bt < SEED_BT_MAX && seed_window_bytes(st.kcp / 64, bt + 1) <= (size_t)SEED_LDS_MAX) ++bt;
    return bt;
  }
  static int check_seed_block(const facppg_wg_config& c, const CcImages& st, int block_tiles, int layers_per_workgroup) {
    const int bt_max = max_block_tiles(st);
    FACPPG_REQUIRE(layers_per_workgroup >= 1, FACPPG_EINVAL, "layers_per_workgroup >= 1");
    FACPPG_REQUIRE(bt_max >= 1, FACPPG_EUNSUPPORTED, "hop %d: the conditioning window of one 32-frame tile (%zu bytes) does not fit the LDS",
                   c.hop_length, seed_window_bytes(st.kcp / 64, 1));
    FACPPG_REQUIRE(block_tiles >= 1 && block_tiles <= bt_max, FACPPG_EINVAL,
                   "block_tiles = %d: the window of %zu bytes per tile must fit %d bytes of LDS and %d accumulator tiles the registers: "
                   "the maximum is %d", block_tiles, seed_window_bytes(st.kcp / 64, 1), SEED_LDS_MAX, SEED_BT_MAX, bt_max);
    return FACPPG_OK;
  }
  static int check_seed_lds(int, size_t) { return FACPPG_OK; }   // (check_seed_block has bounded block_tiles by it)
  static constexpr bool seed_needs_counter = true;              // a bounded launch without one is refused
  static void launch_seed(int block_tiles, unsigned grid, size_t lds, hipStream_t s, const SeedSplitArgs& a) {
    switch (block_tiles) {
      case 1: ks_cond_seed<1><<<grid, 512, lds, s>>>(a); break;
      case 2: ks_cond_seed<2><<<grid, 512, lds, s>>>(a); break;
      default: ks_cond_seed<3><<<grid, 512, lds, s>>>(a); break;
    }
  }
};

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
  // the fp32 handle's images are read back and split into bf16 planes once; it is destroyed afterwards
  facppg_wg* f = nullptr;
  if (int rc = facppg_wg_create(cfg, weights_dev, n_floats, device, stream_, &f)) return rc;
  facppg_wg_split* h = new (std::nothrow) facppg_wg_split();
  if (!h) {
    facppg_wg_destroy(f);
    set_error("facppg_wg_split_create: allocating the handle failed");
    return FACPPG_EHIP;
  }
  h->cfg = f->cfg; h->device = f->device; h->n_cu = f->n_cu;
  memcpy(h->n_rem, f->n_rem, sizeof(h->n_rem)); memcpy(h->n_half, f->n_half, sizeof(h->n_half)); memcpy(h->early, f->early, sizeof(h->early));
  const int rc = cc_create_images<Split>(f, (hipStream_t)stream_, &h->img, &h->arena, &h->arena_bytes);
  facppg_wg_destroy(f);
  if (rc) {
    facppg_wg_split_destroy(h);
    return rc;
  }
  *out = h;
  return FACPPG_OK;
}

extern "C" size_t facppg_wg_split_workspace_bytes(const facppg_wg_split* h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  return ws_layout<Split>(h->cfg, B, T).total;
}

extern "C" int facppg_wg_split_last_launch_shape(const facppg_wg_split* h, int* tile_frames, int* waves, int* n_tiles) {
  FACPPG_REQUIRE(h && tile_frames && waves && n_tiles, FACPPG_EINVAL, "NULL argument");
  *tile_frames = h->last_tile; *waves = h->last_waves; *n_tiles = h->last_tiles;
  return FACPPG_OK;
}

extern "C" int facppg_wg_split_infer(facppg_wg_split* h, const float* mel_dev, const int32_t* T_valid_dev, const float* z_dev,
                                     uint64_t seed, float sigma, int B, int T, float* audio_dev, void* ws_, size_t ws_bytes,
                                     void* stream_) {
  FACPPG_REQUIRE(h && mel_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && T > 0, FACPPG_EINVAL, "B and T must be positive (got %d, %d)", B, T);
  FACPPG_REQUIRE(B <= 65535, FACPPG_EINVAL, "B too large");
  return cc_infer(Split(), h, mel_dev, T_valid_dev, z_dev, seed, sigma, B, T, audio_dev, ws_, ws_bytes, (hipStream_t)stream_);
}

extern "C" int facppg_wg_split_seed_layout(const facppg_wg_split* h, int T, int* Tqp, int* margin, size_t* seed_bytes,
                                           int* max_block_tiles) {
  FACPPG_REQUIRE(h && T > 0 && Tqp && margin && seed_bytes && max_block_tiles, FACPPG_EINVAL, "NULL argument or T <= 0");
  cc_seed_layout<Split>(h->cfg, T, Tqp, margin, seed_bytes);
  *max_block_tiles = Split::max_block_tiles(h->img);
  return FACPPG_OK;
}

extern "C" int facppg_wg_split_mel_pad(const facppg_wg_split* h, const float* mel_dev, int T, int ld, int frame0, int nframes,
                                       float* melp_dev, const int32_t* skip_dev, void* stream_) {
  FACPPG_REQUIRE(h && mel_dev && melp_dev && T > 0, FACPPG_EINVAL, "NULL argument or T <= 0");
  return cc_mel_cvt<Split>(h->cfg, mel_dev, T, ld, frame0, nframes, melp_dev, skip_dev, (hipStream_t)stream_);
}

extern "C" int facppg_wg_split_cond_seed(facppg_wg_split* h, const float* melp_dev, int T, int frame0, int nframes, int block_tiles,
                                         int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                                         const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream_) {
  FACPPG_REQUIRE(h && melp_dev && seeds_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0, FACPPG_EINVAL, "T must be positive (got %d)", T);
  return cc_cond_seed<Split>(h->cfg, h->img, melp_dev, T, frame0, nframes, block_tiles, layers_per_workgroup, flow0, nflows, seeds_dev,
                             seed_bytes, skip_dev, max_workgroups, counter_dev, (hipStream_t)stream_);
}

// WaveGlow.infer on the caller's mel buffer (facppg_wg_split_mel_pad) and seeds (facppg_wg_split_cond_seed)
extern "C" int facppg_wg_split_infer_seeded(facppg_wg_split* h, const float* melp_dev, int T_layout, int T, const float* seeds_dev,
                                            int seeded_frames, const float* z_dev, uint64_t seed, float sigma, float* audio_dev,
                                            void* ws_, size_t ws_bytes, void* const* flow_events, void* stream_) {
  FACPPG_REQUIRE(h && melp_dev && seeds_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  if (int rc = cc_check_seeded(T, T_layout, seeded_frames)) return rc;
  return cc_infer(Split(), h, nullptr, nullptr, z_dev, seed, sigma, 1, T, audio_dev, ws_, ws_bytes, (hipStream_t)stream_, melp_dev,
                  seeds_dev, seeded_frames, T_layout, flow_events);
}
