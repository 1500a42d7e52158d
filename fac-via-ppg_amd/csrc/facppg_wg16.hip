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
// Kernels here: k16_pack_*, k16_noise, k16_wn_layer<LAST, NCB, SEED> (one fused WN layer per launch), k16_cond_seed (the conditioning
// chunks of every layer ahead of time).  The mel and flow-edge kernels, the workspace, image creation, the flow walk and the seeded
// path's host side are facppg_wg_cc.h's, shared with facppg_wg_split.hip; Fp16 below is what they need to know of this file.
#include "facppg_wg_cc.h"

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

namespace facppg {

struct Wg16State : CcImages {};

namespace {

constexpr int ZP = C + 8;     // gated-activation tile: halfs per column (16-byte pad)
constexpr int SP = 64 + 8;    // staged K chunk: halfs per column

__device__ __forceinline__ h16x8 as_h8(u32x4 v) { return __builtin_bit_cast(h16x8, v); }
__device__ __forceinline__ u32x4 as_u4(h16x8 v) { return __builtin_bit_cast(u32x4, v); }
__device__ __forceinline__ f32x16 mfma16(u32x4 a, h16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), b, c, 0, 0, 0);
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
using Seed16Args = SeedArgs<_Float16>;

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

// what facppg_wg_cc.h needs to know of the fp16 arithmetic; an object carries the K order of one infer call
struct Fp16 {
  using E = _Float16;
  using Handle = facppg_wg;
  using LayerArgs = Wn16Args;
  using SeedKernelArgs = Seed16Args;
  static constexpr int planes = 1, tw_max = 128;
  static constexpr const char *create_name = "facppg_wg_create_f16", *image_name = "fp16";
  static constexpr auto pack_gate = k16_pack_gate;
  static constexpr auto pack_res = k16_pack_res;
  static constexpr auto pack_end = k16_pack_end;
  static std::array<KernelLds, 6> lds_attrs() {
    return {{{(const void*)k16_wn_layer<false, 4>, wn16_lds_bytes<4>()}, {(const void*)k16_wn_layer<true, 4>, wn16_lds_bytes<4>()},
             {(const void*)k16_cond_seed<1>, SEED_LDS_MAX}, {(const void*)k16_cond_seed<2>, SEED_LDS_MAX},
             {(const void*)k16_cond_seed<3>, SEED_LDS_MAX}, {(const void*)k16_cond_seed<4>, SEED_LDS_MAX}}};
  }
  static const CcImages& images(const facppg_wg* h) { return *h->w16; }

  static void noise(_Float16* z, size_t n, uint64_t seed, hipStream_t s) {
    k16_noise<<<(unsigned)((n / 4 + 255) / 256 + 1), 256, 0, s>>>(z, n, seed);
  }
  // tile width: 128 frames when the launch still gives every CU a couple of workgroups, else narrower (the B = 1 latency
  // shape: 32-frame tiles spread one short utterance over the chip); FACPPG_WG16_TILE = 32 | 64 | 128 forces one
  static int tile(int P, int B, int T, long ncu, int* tw) {
    const long tiles128 = (long)P * B * ((T + 127) / 128), tiles64 = (long)P * B * ((T + 63) / 64);
    *tw = tiles128 >= 2 * ncu ? 128 : tiles64 >= 2 * ncu ? 64 : 32;
    if (const char* env = getenv("FACPPG_WG16_TILE")) {
      const int v = atoi(env);
      FACPPG_REQUIRE(v == 32 || v == 64 || v == 128, FACPPG_EINVAL, "FACPPG_WG16_TILE=%s: expected 32, 64 or 128", env);
      *tw = v;
    }
    return FACPPG_OK;
  }
  int cond_first;   // the K order of every layer launch (1 on the seeded path)
  void init_layer_args(Wn16Args& a) const { a.cond_first = cond_first; }
  template <int NCB, bool SEED = false>
  static void launch_ncb(const Wn16Args& a, bool last, dim3 grid, hipStream_t s) {
    if (last) k16_wn_layer<true, NCB, SEED><<<grid, 512, wn16_lds_bytes<NCB>(), s>>>(a);
    else k16_wn_layer<false, NCB, SEED><<<grid, 512, wn16_lds_bytes<NCB>(), s>>>(a);
  }
  static void launch_layer(const Wn16Args& a, int tw, bool seeded, bool last, dim3 grid, hipStream_t s) {
    if (seeded) launch_ncb<1, true>(a, last, grid, s);
    else if (tw == 128) launch_ncb<4>(a, last, grid, s);
    else if (tw == 64) launch_ncb<2>(a, last, grid, s);
    else launch_ncb<1>(a, last, grid, s);
  }

  static int check_seed_block(const facppg_wg_config&, const CcImages&, int block_tiles, int layers_per_workgroup) {
    FACPPG_REQUIRE(block_tiles >= 1 && block_tiles <= 4 && layers_per_workgroup >= 1, FACPPG_EINVAL, "block_tiles in 1..4, layers_per_workgroup >= 1");
    return FACPPG_OK;
  }
  static constexpr size_t seed_window_bytes(int ncond, int bt) { return (size_t)ncond * 32 * bt * SP * 2; }
  static int check_seed_lds(int block_tiles, size_t lds) {
    FACPPG_REQUIRE(lds <= (size_t)SEED_LDS_MAX, FACPPG_EUNSUPPORTED, "block_tiles = %d needs %zu bytes of LDS", block_tiles, lds);
    return FACPPG_OK;
  }
  static constexpr bool seed_needs_counter = false;   // a bounded launch without one runs strided
  static void launch_seed(int block_tiles, unsigned grid, size_t lds, hipStream_t s, const Seed16Args& a) {
    switch (block_tiles) {
      case 1: k16_cond_seed<1><<<grid, 512, lds, s>>>(a); break;
      case 2: k16_cond_seed<2><<<grid, 512, lds, s>>>(a); break;
      case 3: k16_cond_seed<3><<<grid, 512, lds, s>>>(a); break;
      default: k16_cond_seed<4><<<grid, 512, lds, s>>>(a); break;
    }
  }
};

}  // namespace

size_t wg16_workspace_bytes(const facppg_wg* h, int B, int T) { return ws_layout<Fp16>(h->cfg, B, T).total; }

void wg16_destroy(facppg_wg* h) {
  delete h->w16;
  h->w16 = nullptr;
}

}  // namespace facppg

using namespace facppg;

extern "C" int facppg_wg_create_f16(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats, int device,
                                    void* stream_, facppg_wg** out) {
  FACPPG_REQUIRE(out, FACPPG_EINVAL, "out is NULL");
  // the fp32 handle's images are read back and rounded to fp16 once; it is destroyed afterwards
  facppg_wg* f = nullptr;
  if (int rc = facppg_wg_create(cfg, weights_dev, n_floats, device, stream_, &f)) return rc;
  facppg_wg* h = new (std::nothrow) facppg_wg();
  Wg16State* st = new (std::nothrow) Wg16State();
  if (!h || !st) {
    delete h; delete st;
    facppg_wg_destroy(f);
    set_error("facppg_wg_create_f16: allocating the handle failed");
    return FACPPG_EHIP;
  }
  h->cfg = f->cfg; h->device = f->device; h->n_cu = f->n_cu; h->poll_limit = f->poll_limit; h->ev_layers = 1;
  memcpy(h->n_rem, f->n_rem, sizeof(h->n_rem)); memcpy(h->n_half, f->n_half, sizeof(h->n_half)); memcpy(h->early, f->early, sizeof(h->early));
  h->P = f->P; h->nj = f->nj; h->kc = f->kc; h->kcp = f->kcp;
  h->w16 = st;
  const int rc = cc_create_images<Fp16>(f, (hipStream_t)stream_, st, &h->arena, &h->arena_bytes);
  facppg_wg_destroy(f);
  if (rc) {
    facppg_wg_destroy(h);
    return rc;
  }
  *out = h;
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
  return cc_infer(Fp16{0}, h, (const _Float16*)mel_dev, T_valid_dev, (const _Float16*)z_dev, seed, sigma, B, T, (_Float16*)audio_dev, ws_,
                  ws_bytes, (hipStream_t)stream_);
}

extern "C" int facppg_wg_infer_f16_order(facppg_wg* h, const uint16_t* mel_dev, const int32_t* T_valid_dev, const uint16_t* z_dev,
                                         uint64_t seed, float sigma, int B, int T, int cond_first, uint16_t* audio_dev, void* ws_,
                                         size_t ws_bytes, void* stream_) {
  if (int rc = wg16_infer_checks("facppg_wg_infer_f16_order", h, mel_dev, audio_dev, ws_, B, T)) return rc;
  FACPPG_REQUIRE(cond_first == 0 || cond_first == 1, FACPPG_EINVAL, "cond_first must be 0 or 1 (got %d)", cond_first);
  return cc_infer(Fp16{cond_first}, h, (const _Float16*)mel_dev, T_valid_dev, (const _Float16*)z_dev, seed, sigma, B, T,
                  (_Float16*)audio_dev, ws_, ws_bytes, (hipStream_t)stream_);
}

#define WG_REQUIRE_FP16(h, fn)                                   \
  FACPPG_REQUIRE(!(h) || (h)->w16, FACPPG_EINVAL,                \
                 fn ": the handle holds fp32 images (facppg_wg_create); use the fp32 entry point of the same name, or make it with facppg_wg_create_f16")

extern "C" int facppg_wg_seed_layout_f16(const facppg_wg* h, int T, int* Tqp, int* margin, size_t* seed_bytes) {
  WG_REQUIRE_FP16(h, "facppg_wg_seed_layout_f16");
  FACPPG_REQUIRE(h && T > 0 && Tqp && margin && seed_bytes, FACPPG_EINVAL, "NULL argument or T <= 0");
  cc_seed_layout<Fp16>(h->cfg, T, Tqp, margin, seed_bytes);
  return FACPPG_OK;
}

extern "C" int facppg_wg_mel_pad_f16(const facppg_wg* h, const float* mel_dev, int T, int ld, int frame0, int nframes,
                                     uint16_t* melp_dev, const int32_t* skip_dev, void* stream_) {
  WG_REQUIRE_FP16(h, "facppg_wg_mel_pad_f16");
  FACPPG_REQUIRE(h && mel_dev && melp_dev && T > 0, FACPPG_EINVAL, "NULL argument or T <= 0");
  return cc_mel_cvt<Fp16>(h->cfg, mel_dev, T, ld, frame0, nframes, (_Float16*)melp_dev, skip_dev, (hipStream_t)stream_);
}

extern "C" int facppg_wg_cond_seed_f16(facppg_wg* h, const uint16_t* melp_dev, int T, int frame0, int nframes, int block_tiles,
                                       int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                                       const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream_) {
  WG_REQUIRE_FP16(h, "facppg_wg_cond_seed_f16");
  FACPPG_REQUIRE(h && melp_dev && seeds_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(T > 0, FACPPG_EINVAL, "T must be positive (got %d)", T);
  return cc_cond_seed<Fp16>(h->cfg, *h->w16, (const _Float16*)melp_dev, T, frame0, nframes, block_tiles, layers_per_workgroup, flow0,
                            nflows, seeds_dev, seed_bytes, skip_dev, max_workgroups, counter_dev, (hipStream_t)stream_);
}

// WaveGlow.infer on the caller's mel buffer (facppg_wg_mel_pad_f16) and seeds (facppg_wg_cond_seed_f16), conditioning-first
extern "C" int facppg_wg_infer_seeded_f16(facppg_wg* h, const uint16_t* melp_dev, int T_layout, int T, const float* seeds_dev,
                                          int seeded_frames, const uint16_t* z_dev, uint64_t seed, float sigma, uint16_t* audio_dev,
                                          void* ws_, size_t ws_bytes, void* const* flow_events, void* stream_) {
  WG_REQUIRE_FP16(h, "facppg_wg_infer_seeded_f16");
  FACPPG_REQUIRE(h && melp_dev && seeds_dev && audio_dev && ws_, FACPPG_EINVAL, "NULL argument");
  if (int rc = cc_check_seeded(T, T_layout, seeded_frames)) return rc;
  return cc_infer(Fp16{1}, h, nullptr, nullptr, (const _Float16*)z_dev, seed, sigma, 1, T, (_Float16*)audio_dev, ws_, ws_bytes,
                  (hipStream_t)stream_, (const _Float16*)melp_dev, seeds_dev, seeded_frames, T_layout, flow_events);
}
