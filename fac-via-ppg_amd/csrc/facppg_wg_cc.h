// Internal to facppg_wg16.hip (fp16) and facppg_wg_split.hip (bf16x3): the CHANNEL-CONTIGUOUS vocoder paths.
//
// The two files run one inference algebra on one layout -- h [B][P][Tqp][256], xa [B][P][Tqp][8], melp [B][Tqp][80], all of
// element type E (_Float16 / float), skip and the flow variable in fp32 -- and differ in E and in their MFMA kernels.  What does
// not depend on the MFMA kernels is here, once: the readers of the fp32 handle's images, the image table, the flow-edge kernels
// (templated on E), the workspace layout, the creation of the image arena, the flow walk and the host side of the seeded path.
// Each file keeps its WN layer, seed, pack (and noise) kernels and a traits struct that names them:
//
//   using E, Handle (facppg_wg / facppg_wg_split: cfg, n_rem, n_half, early, n_cu, last_tile, last_waves, last_tiles),
//   LayerArgs, SeedKernelArgs (= SeedArgs<E>)
//   planes, tw_max, create_name, image_name, pack_gate, pack_res, pack_end, lds_attrs()                  image creation
//   images(h), noise(), tile(), init_layer_args(), launch_layer()                                        the flow walk
//   check_seed_block(), seed_window_bytes(), check_seed_lds(), seed_needs_counter, launch_seed()         the seed pass
//
// Everything here is a template or lives in an anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "facppg_wg_internal.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace facppg {
namespace {

constexpr int SEED_LDS_MAX = 160 * 1024 - 64;   // a CU's LDS less the seed kernel's own word

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

// The images of a handle, in its arena.  Shapes are given per plane: an fp16 image is one plane, a split one a hi and a lo plane
// of 64 lanes each per A fragment.
struct CcImages {
  int P, kc, kcp;
  const u32x4* wconv[MAXF][8];   // gate GEMM, convolution part: [48 K steps][8 waves][2][planes][64] (first layer: the folded taps, 4 K steps)
  const u32x4* wcond[MAXF][8];   // gate GEMM, folded conditioning: [P][kcp/16][8][2][planes][64]
  const u32x4* wres[MAXF][8];    // res rows of a non-last res_skip conv: [16][8][planes][64]; null for the last layer
  const u32x4* wend[MAXF][8];    // end rows (W_end . skip rows), padded to 32 rows: [16][planes][64]
  const float *b1[MAXF][8], *b2[MAXF][8];
  const float *endb[MAXF], *start_w[MAXF], *start_b[MAXF], *winv[MAXF];
};

// ------------------------------------------------------------------------------------------
// Inputs: mel
// ------------------------------------------------------------------------------------------
// mel [B][80][T] -> melp [B][Tqp][80], zero outside each utterance's valid frames
template <class E>
__global__ void k_cc_mel_pad(const E* __restrict__ mel, E* __restrict__ melp, const int* __restrict__ t_valid, int T, int Tqp) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (idx >= Tqp * NMEL) return;
  const int x = idx / NMEL, m = idx % NMEL, q = x - HQ, Tb = t_valid ? t_valid[b] : T;
  melp[(size_t)b * Tqp * NMEL + idx] = (q >= 0 && q < Tb) ? mel[((size_t)b * NMEL + m) * T + q] : (E)0.0f;
}

// frames [f0, f0 + n) of an fp32 mel [80][ld] (the streaming postnet's output) -> the zero-margined [Tqp][80] layout (fp16: rounded
// to nearest even as tensor.half() does)
template <class E>
__global__ void k_cc_mel_cvt(const float* __restrict__ mel, int ld, E* __restrict__ melp, int f0, int n, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * NMEL) return;
  const int m = idx / n, q = f0 + idx % n;
  melp[((size_t)HQ + q) * NMEL + m] = (E)mel[(size_t)m * ld + q];
}

// ------------------------------------------------------------------------------------------
// Flow edges, in fp32: 8 positions per 256-thread workgroup, 32 threads per position (8 start-conv channels each, a position's h
// row written by 32 consecutive lanes).  grid = (ceil(T/8), B, P).
// ------------------------------------------------------------------------------------------
template <class E>
struct EdgeArgs {
  const float* skip;
  const float* aud_in;
  float* aud_out;
  E* h_out;
  E* xa;
  E* audio;          // [B][T*hop]
  const E* z0;       // [B][2*HN][L]
  const E* z_early;  // [B][2][L] or null
  const float *winv, *start_w, *start_b;
  const int* t_valid;
  float sigma;
  int T, P, Tr, Tqp, L, swap, swap_next, final_flow;
};

template <class E>
__device__ __forceinline__ bool edge_pos(const EdgeArgs<E>& p, int& b, int& q, int& pos, int& cg) {
  b = blockIdx.y;
  q = blockIdx.x * 8 + (threadIdx.x >> 5);
  cg = threadIdx.x & 31;
  const int Tb = p.t_valid ? p.t_valid[b] : p.T;
  pos = q * p.P + blockIdx.z;
  return q < Tb;
}

// 8 consecutive channels, already of the element type: one 16-byte store of fp16, two of fp32
__device__ __forceinline__ void store8(_Float16* dst, const _Float16 (&v)[8]) {
  h16x8 h;
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = v[e];
  *(h16x8*)dst = h;
}
__device__ __forceinline__ void store8(float* dst, const float (&v)[8]) {
  *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  *(float4*)(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// start conv (channels 8cg..8cg+7) of the flow whose conditioning channels are a0[0..HN), and (cg == 0) its xa row
template <class E, int HN>
__device__ __forceinline__ void start_conv(const EdgeArgs<E>& p, int b, int q, int cg, const float* a0) {
  const size_t row = ((size_t)b * p.P + blockIdx.z) * p.Tqp + HQ + q;
  E v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ch = 8 * cg + e;
    float s = p.start_b[ch];
#pragma unroll
    for (int j = 0; j < HN; ++j) s = fmaf(p.start_w[ch * HN + j], a0[j], s);
    v[e] = (E)s;
  }
  store8(p.h_out + row * C + 8 * cg, v);
  if (cg == 0) {
    E x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (E)(j < HN ? a0[j] : j == HN ? 1.0f : 0.0f);
    store8(p.xa + row * 8, x);
  }
}

// sigma * z and the start conv of the last flow
template <class E, int HN>
__global__ __launch_bounds__(256) void k_cc_begin(EdgeArgs<E> p) {
  int b, q, pos, cg;
  if (!edge_pos(p, b, q, pos, cg)) return;
  float a[2 * HN];
#pragma unroll
  for (int j = 0; j < 2 * HN; ++j) {
    a[j] = p.sigma * (float)p.z0[((size_t)b * 2 * HN + j) * p.L + pos];
    if (cg == 0) p.aud_out[((size_t)b * 8 + j) * p.L + pos] = a[j];
  }
  start_conv<E, HN>(p, b, q, cg, a + (p.swap_next ? HN : 0));
}

// affine inverse, W^-1, early z, then the next flow's start conv or the final interleave
template <class E, int H, bool EARLY>
__global__ __launch_bounds__(256) void k_cc_flow_end(EdgeArgs<E> p) {
  constexpr int CC = 2 * H, CN = EARLY ? CC + 2 : CC;
  int b, q, pos, cg;
  if (!edge_pos(p, b, q, pos, cg)) return;
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
    if (cg < CN) p.audio[(size_t)b * p.T * p.P * 8 + (size_t)pos * CN + cg] = (E)y[cg];   // glow.py:292 interleave
    return;
  }
  if (cg == 0) {
#pragma unroll
    for (int j = 0; j < CN; ++j) p.aud_out[((size_t)b * 8 + j) * p.L + pos] = y[j];
  }
  start_conv<E, CN / 2>(p, b, q, cg, y + (p.swap_next ? CN / 2 : 0));
}

// f(std::integral_constant<int, n_half>) for n_half in 1..4: the one place a flow's half width becomes a template argument
template <class F>
int with_n_half(int n_half, F&& f) {
  switch (n_half) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: FACPPG_REQUIRE(false, FACPPG_EUNSUPPORTED, "n_half %d", n_half);
  }
  return FACPPG_OK;
}

// ------------------------------------------------------------------------------------------
// Workspace
// ------------------------------------------------------------------------------------------
struct WsCc {
  int P, L, Tr, Tqp;
  size_t h0, h1, xa, melp, skip, aud0, aud1, z, total;
};
// tw_max: the widest tile of the arithmetic; frame rows are padded to a multiple of it
template <class E>
WsCc ws_layout(const facppg_wg_config& c, int B, int T, int tw_max) {
  WsCc w;
  w.P = c.hop_length / 8;
  w.L = T * w.P;
  w.Tr = round_up(T, tw_max);
  w.Tqp = HQ + w.Tr + HQ;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.h0 = take((size_t)B * w.P * w.Tqp * C * sizeof(E));
  w.h1 = take((size_t)B * w.P * w.Tqp * C * sizeof(E));
  w.xa = take((size_t)B * w.P * w.Tqp * 8 * sizeof(E));   // right behind h0 | h1: one memset zeroes all three
  w.melp = take((size_t)B * w.Tqp * NMEL * sizeof(E));
  w.skip = take((size_t)B * 8 * w.P * w.Tr * 4);
  w.aud0 = take((size_t)B * 8 * w.L * 4);
  w.aud1 = take((size_t)B * 8 * w.L * 4);
  w.z = take(((size_t)B * 8 * w.L + 4) * sizeof(E));
  w.total = off;
  return w;
}
template <class Tr>
WsCc ws_layout(const facppg_wg_config& c, int B, int T) { return ws_layout<typename Tr::E>(c, B, T, Tr::tw_max); }

// ------------------------------------------------------------------------------------------
// Image creation: the fp32 handle f folds the blob (upsampler into the conditioning, end conv through the skip rows, first taps
// through start); its images are read back by the arithmetic's pack kernels, once, into one arena
// ------------------------------------------------------------------------------------------
struct KernelLds {
  const void* kernel;
  int bytes;   // dynamic LDS the kernel may be launched with
};

// lays the images out from `base` on (256-byte aligned pieces), fills the table and returns the bytes taken; base == null: sizes only
template <class Tr>
size_t place_images(const facppg_wg* f, char* base, CcImages* img) {
  const int nl = f->cfg.wn_layers;
  const size_t frag = (size_t)Tr::planes * 64 * 16;   // one A fragment: 64 lanes of 16 bytes per plane
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
  img->P = f->P; img->kc = f->kc; img->kcp = f->kcp;
  for (int k = 0; k < f->cfg.n_flows; ++k) {
    const size_t hh = f->n_half[k], cc = 2 * hh;
    for (int i = 0; i < nl; ++i) {
      img->wconv[k][i] = (const u32x4*)take((size_t)(i == 0 ? 4 : 48) * 16 * frag);
      img->wcond[k][i] = (const u32x4*)take((size_t)f->P * (f->kcp / 16) * 16 * frag);
      img->wres[k][i] = i == nl - 1 ? nullptr : (const u32x4*)take((size_t)16 * 8 * frag);
      img->wend[k][i] = (const u32x4*)take((size_t)16 * frag);
      img->b1[k][i] = (const float*)take(2 * C * 4);
      img->b2[k][i] = (const float*)take(C * 4);
    }
    img->endb[k] = (const float*)take(8 * 4);
    img->start_w[k] = (const float*)take(C * hh * 4);
    img->start_b[k] = (const float*)take(C * 4);
    img->winv[k] = (const float*)take(cc * cc * 4);
  }
  return off;
}

// Allocates the arena and fills it and *img from f's images on stream s (synchronised before it returns), then raises the dynamic
// LDS limits of the arithmetic's kernels.  On failure *arena is null or the caller's to free.
template <class Tr>
int cc_create_images(const facppg_wg* f, hipStream_t s, CcImages* img, char** arena, size_t* arena_bytes) {
  const int nl = f->cfg.wn_layers, nf = f->cfg.n_flows;
  const size_t bytes = place_images<Tr>(f, nullptr, img);
  *arena = nullptr;
  if (hipMalloc((void**)arena, bytes) != hipSuccess) {
    *arena = nullptr;
    set_error("%s: allocating %zu bytes of %s images failed", Tr::create_name, bytes, Tr::image_name);
    return FACPPG_EHIP;
  }
  *arena_bytes = bytes;
  place_images<Tr>(f, *arena, img);
  hipError_t e = hipSuccess;
  auto cpy = [&](const float* dst, const float* src, size_t n) {
    if (e == hipSuccess) e = hipMemcpyAsync((float*)dst, src, n * 4, hipMemcpyDeviceToDevice, s);
  };
  auto U = [](const u32x4* p) { return (u32x4*)p; };
  for (int k = 0; k < nf && e == hipSuccess; ++k) {
    const size_t hh = f->n_half[k], cc = 2 * hh;
    for (int i = 0; i < nl; ++i) {
      const int nks = i == 0 ? 4 : 48, ncks = f->P * (f->kcp / 16);
      Tr::pack_gate<<<nks * 4, 256, 0, s>>>(i == 0 ? (const float*)f->w1f[k] : (const float*)f->w1pm[k][i], U(img->wconv[k][i]), nks);
      Tr::pack_gate<<<ncks * 4, 256, 0, s>>>((const float*)f->wcpm[k][i], U(img->wcond[k][i]), ncks);
      if (i != nl - 1) Tr::pack_res<<<32, 256, 0, s>>>((const float*)f->w2r[k][i], U(img->wres[k][i]));
      Tr::pack_end<<<4, 256, 0, s>>>(f->we[k][i], U(img->wend[k][i]));
      cpy(img->b1[k][i], f->b1pm[k][i], 2 * C);
      cpy(img->b2[k][i], f->b2[k][i], C);
    }
    cpy(img->endb[k], f->endb[k], 8);
    cpy(img->start_w[k], f->start_w[k], C * hh);
    cpy(img->start_b[k], f->start_b[k], C);
    cpy(img->winv[k], f->winv[k], cc * cc);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // (the fp32 images are read by the packers above)
  for (const KernelLds& a : Tr::lds_attrs())
    if (e == hipSuccess) e = hipFuncSetAttribute(a.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, a.bytes);
  if (e != hipSuccess) {
    set_error("%s: %s", Tr::create_name, hipGetErrorString(e));
    return FACPPG_EHIP;
  }
  return FACPPG_OK;
}

// ------------------------------------------------------------------------------------------
// WaveGlow.infer: the flow walk.  melp_ext != null (B = 1, the seeded path): the caller's zero-margined mel buffer laid out, like
// `seeds`, for T_layout >= T frames; the layer launches are then the arithmetic's seeded ones (32-frame tiles, conditioning-first):
// tiles wholly inside [0, seeded_frames) start from their seeds, the others run full K in the same launches.  flow_events[k] (may
// be null): the launches of flow k wait for it on the stream.
// ------------------------------------------------------------------------------------------
template <class Tr>
int cc_infer(const Tr& tr, typename Tr::Handle* h, const typename Tr::E* mel_dev, const int32_t* T_valid_dev, const typename Tr::E* z,
             uint64_t seed, float sigma, int B, int T, typename Tr::E* audio_dev, void* ws_, size_t ws_bytes, hipStream_t s,
             const typename Tr::E* melp_ext = nullptr, const float* seeds_dev = nullptr, int seeded_frames = 0, int T_layout = 0,
             void* const* flow_events = nullptr) {
  using E = typename Tr::E;
  if (!melp_ext) T_layout = T;
  const facppg_wg_config& c = h->cfg;
  const CcImages& st = Tr::images(h);
  WsCc w = ws_layout<Tr>(c, B, T_layout);   // rows (Tr, Tqp) of the layout; positions of the T frames that are there
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w.total);
  const int nf = c.n_flows;
  {
    int tot = h->n_rem[nf - 1];
    for (int k = 0; k < nf; ++k) tot += h->early[k] ? c.n_early_size : 0;
    FACPPG_REQUIRE(tot == 8, FACPPG_EUNSUPPORTED, "noise channel count %d != n_group", tot);
  }
  w.L = T * w.P;
  FACPPG_REQUIRE((1 << (c.wn_layers - 1)) / w.P + 1 <= HQ, FACPPG_EUNSUPPORTED, "hop %d: the dilated taps reach past the %d-frame margins",
                 c.hop_length, HQ);
  FACPPG_REQUIRE((double)B * w.P * w.Tqp * C < 2.0e9, FACPPG_EUNSUPPORTED, "B*T = %d*%d frames is too long", B, T);
  int tw = 0;
  if (int rc = Tr::tile(w.P, B, T, h->n_cu > 0 ? h->n_cu : 256, &tw)) return rc;
  if (melp_ext) tw = 32;   // seeds are kept per 32-frame tile
  char* ws = (char*)ws_;
  E* hbuf[2] = {(E*)(ws + w.h0), (E*)(ws + w.h1)};
  E* xa = (E*)(ws + w.xa);
  const E* melp = melp_ext ? melp_ext : (const E*)(ws + w.melp);
  float* skip = (float*)(ws + w.skip);
  float* aud[2] = {(float*)(ws + w.aud0), (float*)(ws + w.aud1)};
  FACPPG_HIP_CHECK(hipMemsetAsync(ws + w.h0, 0, w.melp - w.h0, s));   // h0, h1, xa: margins and frames past each utterance
  if (!melp_ext) k_cc_mel_pad<E><<<dim3((w.Tqp * NMEL + 255) / 256, B), 256, 0, s>>>(mel_dev, (E*)(ws + w.melp), T_valid_dev, T, w.Tqp);
  if (!z) {
    Tr::noise((E*)(ws + w.z), (size_t)B * 8 * w.L, seed, s);
    z = (const E*)(ws + w.z);
  }
  const dim3 lgrid((T + tw - 1) / tw, B, w.P);
  h->last_tile = tw; h->last_waves = 8; h->last_tiles = (int)(lgrid.x * lgrid.y * lgrid.z);

  EdgeArgs<E> e;
  memset(&e, 0, sizeof(e));
  e.skip = skip; e.xa = xa; e.audio = audio_dev; e.t_valid = T_valid_dev; e.sigma = sigma;
  e.T = T; e.P = w.P; e.Tr = w.Tr; e.Tqp = w.Tqp; e.L = w.L;
  const dim3 egrid((T + 7) / 8, B, w.P);
  int ai = 0, hi = 0;
  {
    const int k = nf - 1;
    e.z0 = z; e.aud_out = aud[ai]; e.h_out = hbuf[hi]; e.start_w = st.start_w[k]; e.start_b = st.start_b[k];
    e.swap_next = c.alternate_halves && (k & 1);
    if (int rc = with_n_half(h->n_half[k], [&](auto hn) { k_cc_begin<E, decltype(hn)::value><<<egrid, 256, 0, s>>>(e); })) return rc;
  }
  size_t z_off = (size_t)B * h->n_rem[nf - 1] * w.L;
  typename Tr::LayerArgs a;
  memset(&a, 0, sizeof(a));
  a.xa = xa; a.melp = melp; a.skip = skip; a.t_valid = T_valid_dev;
  a.T = T; a.P = w.P; a.Tr = w.Tr; a.Tqp = w.Tqp; a.kc = st.kc; a.ncond = st.kcp / 64;
  a.seed_nt = w.Tr / 32; a.seed_tiles = melp_ext ? std::min(seeded_frames, round_up(T, 32)) / 32 : 0;
  tr.init_layer_args(a);
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
      Tr::launch_layer(a, tw, melp_ext != nullptr, last, lgrid, s);
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
    const bool early = h->early[k];
    if (int rc = with_n_half(h->n_half[k], [&](auto hn) {
          if (early) k_cc_flow_end<E, decltype(hn)::value, true><<<egrid, 256, 0, s>>>(e);
          else k_cc_flow_end<E, decltype(hn)::value, false><<<egrid, 256, 0, s>>>(e);
        }))
      return rc;
    ai ^= 1;
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

// ------------------------------------------------------------------------------------------
// The seeded path's host side (B = 1): the layout of the caller's mel and seed buffers, the mel conversion, the seed pass
// ------------------------------------------------------------------------------------------
template <class E>
struct SeedArgs {
  const E* melp;                    // [Tqp][80] zero-margined mel frames
  float4* seeds;                    // [layers_total][P][seed_nt][8][2][4][64]
  const u32x4* wcond[MAXF * 8];     // per (flow, layer): [P][4 ncond][8][2][planes][64]
  int lpw, P, Tr, seed_nt;
  int tile0, tile1, nblk;           // tiles [tile0, tile1) in nblk blocks of BT
  int ncond, kc;
  int layer0, layer1, items;
  const int* skip;                  // optional (device): *skip != 0 -> the launch does nothing
  int* counter;                     // bounded launch: hands out the items past the first gridDim (zero at launch), or null: strided
};

template <class Tr>
void cc_seed_layout(const facppg_wg_config& c, int T, int* Tqp, int* margin, size_t* seed_bytes) {
  const WsCc w = ws_layout<Tr>(c, 1, T);
  *Tqp = w.Tqp; *margin = HQ;
  *seed_bytes = (size_t)c.n_flows * c.wn_layers * w.P * (w.Tr / 32) * 4096 * sizeof(float4);
}

template <class Tr>
int cc_mel_cvt(const facppg_wg_config& c, const float* mel_dev, int T, int ld, int frame0, int nframes, typename Tr::E* melp_dev,
               const int32_t* skip_dev, hipStream_t s) {
  const WsCc w = ws_layout<Tr>(c, 1, T);
  FACPPG_REQUIRE(frame0 >= 0 && nframes >= 0 && frame0 + nframes <= w.Tr && frame0 + nframes <= ld, FACPPG_EINVAL,
                 "frames [%d, %d) do not lie inside the %d padded frames and the row length %d", frame0, frame0 + nframes, w.Tr, ld);
  if (nframes == 0) return FACPPG_OK;
  k_cc_mel_cvt<typename Tr::E><<<(nframes * NMEL + 255) / 256, 256, 0, s>>>(mel_dev, ld, melp_dev, frame0, nframes, skip_dev);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

template <class Tr>
int cc_cond_seed(const facppg_wg_config& c, const CcImages& st, const typename Tr::E* melp_dev, int T, int frame0, int nframes,
                 int block_tiles, int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                 const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, hipStream_t s) {
  const WsCc w = ws_layout<Tr>(c, 1, T);
  size_t need = 0; int tqp = 0, mg = 0;
  cc_seed_layout<Tr>(c, T, &tqp, &mg, &need);
  FACPPG_REQUIRE(seed_bytes >= need, FACPPG_EWORKSPACE, "seed buffer has %zu bytes, need %zu", seed_bytes, need);
  FACPPG_REQUIRE(frame0 >= 0 && frame0 % 32 == 0 && nframes > 0 && frame0 + nframes <= w.Tr, FACPPG_EINVAL,
                 "frames [%d, %d): the first must be a multiple of 32 and the range inside the %d padded frames", frame0, frame0 + nframes, w.Tr);
  if (int rc = Tr::check_seed_block(c, st, block_tiles, layers_per_workgroup)) return rc;
  if (nflows <= 0) { flow0 = 0; nflows = c.n_flows; }
  FACPPG_REQUIRE(flow0 >= 0 && flow0 + nflows <= c.n_flows, FACPPG_EINVAL, "flows [%d, %d) of %d", flow0, flow0 + nflows, c.n_flows);
  FACPPG_REQUIRE(c.n_flows * c.wn_layers <= MAXF * 8, FACPPG_EUNSUPPORTED, "too many layers");
  typename Tr::SeedKernelArgs a;
  memset(&a, 0, sizeof(a));
  a.melp = melp_dev; a.seeds = (float4*)seeds_dev; a.skip = skip_dev;
  for (int k = 0; k < c.n_flows; ++k)
    for (int i = 0; i < c.wn_layers; ++i) a.wcond[k * c.wn_layers + i] = st.wcond[k][i];
  a.lpw = layers_per_workgroup; a.P = w.P; a.Tr = w.Tr; a.seed_nt = w.Tr / 32;
  const int ntiles = (nframes + 31) / 32;
  a.tile0 = frame0 / 32; a.tile1 = a.tile0 + ntiles; a.nblk = (ntiles + block_tiles - 1) / block_tiles;
  a.ncond = st.kcp / 64; a.kc = st.kc;
  a.layer0 = flow0 * c.wn_layers; a.layer1 = (flow0 + nflows) * c.wn_layers;
  a.items = (a.layer1 - a.layer0 + a.lpw - 1) / a.lpw * w.P * a.nblk;
  size_t lds = Tr::seed_window_bytes(a.ncond, block_tiles);
  if (int rc = Tr::check_seed_lds(block_tiles, lds)) return rc;
  // a BOUNDED launch (the caller shares the GPU with other streams) asks for a CU's whole LDS per workgroup, as
  // facppg_wg_cond_seed does: one workgroup per CU and no other stream's small workgroups next to it
  const int max_wgs = max_workgroups / 8 * 8;
  const bool bounded = max_wgs > 0 && max_wgs < a.items;
  if (max_workgroups > 0) lds = (size_t)SEED_LDS_MAX;
  a.counter = bounded ? counter_dev : nullptr;   // (bounded without a counter: the workgroups stride over the items)
  if (Tr::seed_needs_counter) FACPPG_REQUIRE(!bounded || counter_dev, FACPPG_EINVAL, "a bounded launch needs counter_dev");
  Tr::launch_seed(block_tiles, (unsigned)(bounded ? max_wgs : a.items), lds, s, a);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

// the argument checks of an infer_seeded entry point
inline int cc_check_seeded(int T, int T_layout, int seeded_frames) {
  FACPPG_REQUIRE(T > 0 && T_layout >= T, FACPPG_EINVAL, "need 0 < T <= T_layout (got %d, %d)", T, T_layout);
  FACPPG_REQUIRE(seeded_frames >= 0 && seeded_frames % 32 == 0 && seeded_frames <= round_up(T, 32), FACPPG_EINVAL,
                 "seeded_frames = %d: expected a multiple of 32 in [0, %d]", seeded_frames, round_up(T, 32));
  return FACPPG_OK;
}

}  // namespace
}  // namespace facppg
