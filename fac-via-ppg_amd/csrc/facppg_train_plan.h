// Which kernels the bf16 training entry points of facppg_train_bf16.hip launch, in what shape, and where their caller-owned
// buffers are carved: pure host arithmetic over the layer count, the batch, the segment length and the environment switches.
// No HIP header, no launch: the entry points parse the switches once per call, plan, and execute what these functions return;
// facppg_train_bf16_launch_plan and facppg_wn_bf16_launch_plan report the same plans to callers without a device
// (tests/test_train_plan_cpu.py pins the table).  The constants the conditions depend on live here too; the kernels use the
// same definitions (FACPPG_HD: callable from device code where a HIP compiler reads this header).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "facppg.h"

namespace facppg {

#ifndef FACPPG_HD
#ifdef __HIPCC__
#define FACPPG_HD __host__ __device__
#else
#define FACPPG_HD
#endif
#endif

constexpr int C = 256, NCOND = 640, HALO = 128;
constexpr int BM = 128, BN = 128, KC = 64;     // k_bgemm tile and K chunk
constexpr int K1 = 3 * C + NCOND;              // 1408: reduction length of the gate GEMM (tap 0 | tap 1 | tap 2 | cond)
// padded positions per batch item: a multiple of the 128-column GEMM tile, so a tile's staging loads never leave the
// batch item's rows (rows >= L are zero)
static FACPPG_HD inline int pad_len(int L) { return (L + BN - 1) / BN * BN; }

// the fused layer kernels k_wn_fwd / k_wn_bwd: K chunk and the LDS pitches of their tiles
constexpr int FKC = 128, FLDB = FKC + 8, FLDA = C + 8, FLDT = 2 * C + 8, FLDO = 2 * C + 4;
constexpr int DLDO = NCOND / 2 + 4;            // k_dspect: fp32 tile pitch
constexpr int LDP = 64 + 8;                    // k_wgrad / k_wgrad2: LDS pitch (positions) of the transposed images
constexpr int CS_SLICES = 256, MAXCS = 16;     // column sums: row slices per problem, problems per launch
#ifndef FACPPG_SMALL_PARTS
#define FACPPG_SMALL_PARTS 256
#endif
constexpr int SMALL_PARTS = FACPPG_SMALL_PARTS;   // partial sums of the <= 8-channel weight gradients (one block each)
constexpr int WG_MAXSPLIT = 8;                 // k_wgrad: position splits per output tile at most
constexpr int MAXRED = 48;                     // problems of one deferred weight-gradient reduce

// dynamic LDS per workgroup
// k_wn_fwd<TN>: staging (TN * 544) -> gated + tanh|sigmoid tiles (TN * 1568) -> fp32 res/skip tile (TN * 2064): 132 096 B (64) / 66 048 B (32)
inline size_t wn_fwd_lds(int TN) { return (size_t)TN * FLDO * 4; }
// k_wn_bwd<TN>: 135 168 B (64 positions) / 67 584 B (32)
inline size_t wn_bwd_lds(int TN) { return ((size_t)2 * TN * FLDB + (size_t)TN * FLDA + (size_t)TN * FLDT) * 2; }
constexpr size_t kDspectLds = (size_t)64 * DLDO * 4;          // 82 944 B (staging 34 816 B first)
constexpr size_t kWgradLds = (size_t)2 * 2 * 128 * LDP * 2;   // 73 728 B
constexpr size_t kWgrad2Lds = (size_t)2 * 2 * 256 * LDP * 2;  // 147 456 B

// ------------------------------------------------------------------------------------------
// The environment switches of the training entry points (INTEGRATION.md lists them), parsed once per entry call and never
// cached: tests flip them between calls of one process, and a step is captured into a HIP graph after eager warm-up calls.
// pack_per_step -- when the bf16 operand images of a flow's stack are formed.  Measured (round 6): all flows at the start of the
// step (one launch per flow, 12 instead of 24) leaves every layer launch fetching its 2 - 3 MB of weights from HBM milliseconds
// after they were written (k_wn_fwd 38.6 -> 42.7 us, k_wn_bwd 30.1 -> 32.4 at batch 12; 18.1 -> 22.6 at batch 3: +0.5 ms per
// step); packed right in front of the flow's stack, per direction, they are still in the L2s / the Infinity Cache when the layers
// read them.  FACPPG_TRAIN_PACK=step: the former.
struct TrainTuning {
  int tile;               // FACPPG_TRAIN_TILE: 0 = unset, else 32 ("32") or 64 (anything else)
  int fused_fwd;          // FACPPG_TRAIN_FUSED_FWD: -1 = unset, 0 ("0...") or 1 (anything else)
  int fused_bwd;          // FACPPG_TRAIN_FUSED_BWD: likewise
  bool dspect_bgemm;      // FACPPG_TRAIN_DSPECT_BGEMM=1: the k_bgemm<EP_ACC_F32> launch (bit-equality test, A/B timing)
  bool pack_per_step;     // FACPPG_TRAIN_PACK=step: every flow's operand images at the start of the step (see facppg_glow_bf16_begin)
  int wgrad_tile;         // FACPPG_WGRAD_TILE: 0 = unset, else 256 ("256") or 128 (anything else)
  bool wgrad_no_xcd_map;  // FACPPG_WGRAD_NO_XCD_MAP=1: k_wgrad's workgroups in plain grid order
  int edge_wgs;           // FACPPG_EDGE_WGS: workgroups a backward edge launch aims at (default, and for values <= 0: 512)
  bool upsample_gemm;     // FACPPG_UPSAMPLE_GEMM=0 turns the MFMA upsampler off (the scalar kernels run)
};

inline TrainTuning train_tuning_from_env() {
  auto forced = [](const char* name) {
    const char* e = getenv(name);
    return e ? (e[0] != '0' ? 1 : 0) : -1;
  };
  auto is_one = [](const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
  };
  TrainTuning t;
  const char* tile = getenv("FACPPG_TRAIN_TILE");
  t.tile = tile ? (atoi(tile) == 32 ? 32 : 64) : 0;
  t.fused_fwd = forced("FACPPG_TRAIN_FUSED_FWD");
  t.fused_bwd = forced("FACPPG_TRAIN_FUSED_BWD");
  t.dspect_bgemm = is_one("FACPPG_TRAIN_DSPECT_BGEMM");
  const char* pack = getenv("FACPPG_TRAIN_PACK");
  t.pack_per_step = pack && !strcmp(pack, "step");
  const char* wtile = getenv("FACPPG_WGRAD_TILE");
  t.wgrad_tile = wtile ? (atoi(wtile) == 256 ? 256 : 128) : 0;
  t.wgrad_no_xcd_map = is_one("FACPPG_WGRAD_NO_XCD_MAP");
  const char* wgs = getenv("FACPPG_EDGE_WGS");
  t.edge_wgs = wgs && atoi(wgs) > 0 ? atoi(wgs) : 512;
  const char* up = getenv("FACPPG_UPSAMPLE_GEMM");
  t.upsample_gemm = !(up && up[0] == '0');
  return t;
}

// ------------------------------------------------------------------------------------------
// Layouts of the caller-owned buffers.  One carve (256-byte aligned pieces in order) and one set of sizes; the stand-alone WN
// entry points' scratch is the group entry points' packed images and gradients in flight laid behind one another.
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
};

// saved activations of one flow's stack (forward -> backward)
struct StateLayout { size_t h, ts, acts, skip, total; size_t h_one, ts_one, acts_one; };
inline StateLayout state_layout(int nl, int B, int Lr) {
  StateLayout s;
  const int Lp = HALO + Lr + HALO;
  Carve c;
  s.h_one = (size_t)B * Lp * C * 2; s.ts_one = (size_t)B * Lr * 2 * C * 2; s.acts_one = (size_t)B * Lr * C * 2;
  s.h = c.take(s.h_one * (nl + 1)); s.ts = c.take(s.ts_one * nl); s.acts = c.take(s.acts_one * nl); s.skip = c.take((size_t)B * Lr * C * 4);
  s.total = c.off;
  return s;
}

// bf16 A-operand images of one flow's stack, both directions (*_one: per layer; condt: one image over all layers)
struct ImageLayout { size_t w1, w2, rst, int_, condt; size_t w1_one, w2_one, rst_one, int_one; };
inline void carve_images(Carve& c, int nl, ImageLayout& s) {
  s.w1_one = (size_t)16 * (K1 / 16) * 64 * 16; s.w2_one = (size_t)16 * (C / 16) * 64 * 16;
  s.rst_one = (size_t)8 * (2 * C / 16) * 64 * 16; s.int_one = (size_t)8 * (3 * 2 * C / 16) * 64 * 16;
  s.w1 = c.take(s.w1_one * nl); s.w2 = c.take(s.w2_one * nl); s.rst = c.take(s.rst_one * nl); s.int_ = c.take(s.int_one * nl);
  s.condt = c.take((size_t)(NCOND / 32) * (nl * 2 * C / 16) * 64 * 16);
}
// gradients in flight of one flow's backward (*_one: per layer)
struct GradLayout { size_t dpre, dh, dskip; size_t dpre_one, dh_one; };
inline void carve_grads(Carve& c, int nl, int B, int Lr, GradLayout& s) {
  const int Lp = HALO + Lr + HALO;
  s.dpre_one = (size_t)B * Lp * 2 * C * 2; s.dh_one = (size_t)B * Lr * C * 2;
  s.dpre = c.take(s.dpre_one * nl); s.dh = c.take(s.dh_one * (nl + 1)); s.dskip = c.take(s.dh_one);
}
inline size_t cspart_bytes() { return (size_t)MAXCS * CS_SLICES * 1024 * 4; }   // column-sum partials [problem][slice][1024]
// partial sums of ONE weight-gradient launch: 5 splits of the largest batch (3 taps x layers x [512 x 256]; k_wgrad2)
inline size_t wgpart_bytes(int nl) { return (size_t)3 * nl * 5 * (2 * C) * C * 4; }

// what one flow's stack keeps packed for a whole step: both directions' operand images and the summed gate biases
struct PackedLayout : ImageLayout { size_t b1, total; };
inline PackedLayout packed_layout(int nl) {
  PackedLayout s;
  Carve c;
  carve_images(c, nl, s);
  s.b1 = c.take((size_t)nl * 2 * C * 4);
  s.total = c.off;
  return s;
}
// gradients in flight of ONE flow's backward (the flows of a step take turns on it) + the reductions' partial buffers; a region
// of wgpart_bytes per weight-gradient launch of a flow (three regions: one ordered reduce)
struct WorkLayout : GradLayout { size_t cspart, wgpart, wgpart_bytes, total; };
inline WorkLayout work_layout(int nl, int B, int Lr) {
  WorkLayout s;
  Carve c;
  carve_grads(c, nl, B, Lr, s);
  s.cspart = c.take(cspart_bytes());
  s.wgpart_bytes = wgpart_bytes(nl);
  s.wgpart = c.take(s.wgpart_bytes * 3);
  s.total = c.off;
  return s;
}
// per-call scratch of the stand-alone WN entry points: images | gradients | <= 8-channel partials | the reductions' partials (one
// shared weight-gradient region).  facppg_wn_bf16_scratch_bytes adds the summed gate biases behind `total`.
struct ScratchLayout : ImageLayout, GradLayout { size_t part, cspart, wgpart, wgpart_bytes, total; };
inline ScratchLayout scratch_layout(int nl, int B, int Lr) {
  ScratchLayout s;
  Carve c;
  carve_images(c, nl, s);
  carve_grads(c, nl, B, Lr, s);
  s.part = c.take((size_t)SMALL_PARTS * 9 * C * 4);
  s.cspart = c.take(cspart_bytes());
  s.wgpart_bytes = wgpart_bytes(nl);
  s.wgpart = c.take(s.wgpart_bytes);
  s.total = c.off;
  return s;
}
inline size_t scratch_bias_bytes() { return (size_t)2 * C * 4 * 8; }   // [8 layers][512] summed gate biases behind the scratch

// ------------------------------------------------------------------------------------------
// k_bgemm: 128-column tiles once they give >= 1.5 workgroups per CU, else 64-column tiles (twice the workgroups).  A 256 x 128 /
// 8-wave tile with both operands through LDS was built and measured slower in every mode (profiles/r02_experiments.txt).
struct BgemmShape { int cols, grid; };   // columns per tile (128 or 64), workgroups
inline BgemmShape plan_bgemm(int M, int N, int B) {
  const int nm = (M + BM - 1) / BM;
  const long wide = (long)((N + 127) / 128) * nm * B;
  BgemmShape p;
  p.cols = wide >= 384 ? 128 : 64;
  const int ct = ((N + p.cols - 1) / p.cols) * B;
  p.grid = 8 * nm * ((ct + 7) / 8);
  return p;
}

// ---- the layer loop of one stack, forward and the backward's data-gradient chain ----
// Tiles: 64 positions once they give 160 workgroups, else 32 (FACPPG_TRAIN_TILE=64 / 32 forces one).
// Forward: one launch per layer once its tiles fill most of the chip (a tile streams ALL of the layer's weights into its CU: with
// few tiles the two-launch layer, which deals the weight rows over four times as many workgroups, is as fast or faster).  Measured,
// whole step, segment 10 000: batch 3 (120 tiles of 32 positions) 10.25 ms fused / 10.20 two launches; batch 6 (240 of 32) 12.7 /
// 13.6; batch 12 (240 of 64) 18.5 / 20.4.  FACPPG_TRAIN_FUSED_FWD=1 / 0 forces either path (the bit-equality test and A/B timing).
// Backward: FACPPG_TRAIN_FUSED_BWD=1 / 0 forces either path.  The backward pair is worth one launch much earlier than the forward
// pair (its tiles stream 1 MB of weights, not 1.7, and the two launches it replaces are the more latency-bound ones): batch 3,
// whole step, 10.8 ms two launches / 10.5 fused with 64-position tiles / 10.2 with 32.  A one-layer stack has no (conv_i,
// gate_{i-1}) pair to fuse.
struct WnStackPlan {
  int tile;                    // positions per tile of the fused launches: 64 or 32
  bool fused_fwd, fused_bwd;   // k_wn_fwd / k_wn_bwd instead of two k_bgemm launches per layer
  int ntiles, fused_grid;      // tiles of a fused launch and its workgroups (a multiple of 8: dealt round the XCDs)
  size_t fwd_lds, bwd_lds;     // dynamic LDS of k_wn_fwd<tile> / k_wn_bwd<tile>
  // the k_bgemm launches of the layer loop: gate [512 x 1408], res/skip [512 x 256] ([256 x 256] in the last layer), gate
  // backward [256 x 512], transposed conv [256 x 1536], and the conditioning gradient [640 x nl * 512] (EP_ACC_F32)
  BgemmShape gate, resskip, resskip_last, gate_bwd, conv_bwd, dspect_acc;
  bool dspect_bgemm;           // the conditioning gradient as k_bgemm<EP_ACC_F32> instead of k_dspect
  int dspect_ntiles, dspect_grid;   // k_dspect: tiles (64 positions x half of the 640 channels) and workgroups
  size_t dspect_lds;
};

inline WnStackPlan plan_wn_stack(const TrainTuning& t, int nl, int B, int L) {
  WnStackPlan p;
  p.tile = t.tile ? t.tile : (long)((L + 63) / 64) * B >= 160 ? 64 : 32;
  const long t32 = (long)((L + 31) / 32) * B;
  p.fused_fwd = t.fused_fwd >= 0 ? t.fused_fwd != 0 : t32 >= 160;
  p.fused_bwd = (t.fused_bwd >= 0 ? t.fused_bwd != 0 : t32 >= 40) && nl > 1;
  p.ntiles = ((L + p.tile - 1) / p.tile) * B;
  p.fused_grid = 8 * ((p.ntiles + 7) / 8);
  p.fwd_lds = wn_fwd_lds(p.tile); p.bwd_lds = wn_bwd_lds(p.tile);
  p.gate = plan_bgemm(2 * C, L, B); p.resskip = plan_bgemm(2 * C, L, B); p.resskip_last = plan_bgemm(C, L, B);
  p.gate_bwd = plan_bgemm(C, L, B); p.conv_bwd = plan_bgemm(C, L, B); p.dspect_acc = plan_bgemm(NCOND, L, B);
  p.dspect_bgemm = t.dspect_bgemm;
  p.dspect_ntiles = 2 * ((L + 63) / 64) * B;
  p.dspect_grid = 8 * ((p.dspect_ntiles + 7) / 8);
  p.dspect_lds = kDspectLds;
  return p;
}

// ---- one batch of weight-gradient products that share (M, K) tile counts ----
// 256 x 256 tiles (k_wgrad2) when they give >= 32 tiles and every workgroup then has >= 24 chunks of positions;
// FACPPG_WGRAD_TILE=128|256 forces the kernel.  k_wgrad2: one workgroup per CU (144 KB of LDS each), never more than 256, every
// split gets a chunk.  k_wgrad: about ONE workgroup per CU (two fit, 73 KB of LDS each): measured at batch 3 / 12, whole step,
// aiming at 64 / 128 / 256 / 384 / 512 / 768 / 1536 / 3072 workgroups: 11.48 / 11.23 / 11.09 / 11.18 / 11.31 / 11.53 / 11.99 /
// 12.93 ms and 24.42 / 23.43 / 22.46 / 22.55 / 22.66 / 23.06 / 23.12 / 24.26 ms -- every further split adds a 64 KB partial tile
// per workgroup and a longer reduction.  Either way the split count shrinks until the partials fit the caller's buffer.
struct WgradPlan {
  int rc = FACPPG_OK;        // != FACPPG_OK: the verdict wgrad_launch returns, with msg
  char msg[96] = "";
  int tile;                  // 256: k_wgrad2, 128: k_wgrad
  int ns;                    // position splits per output tile; > 1: partial sums + an ordered reduce
  int tiles_k, tiles_m, ngroups;
  int xcd_map;               // workgroups of one (problem, split) dealt to one XCD back to back
  unsigned grid[3];
  size_t lds;
  size_t pstride;            // floats per (problem, split) partial = max M * max K of the batch
  size_t part_floats;        // of the whole launch: nprob * ns * pstride
  long workgroups() const { return (long)grid[0] * grid[1] * grid[2]; }
};

inline WgradPlan plan_wgrad(const TrainTuning& t, int nprob, int maxM, int maxK, int B, int L, size_t part_bytes) {
  WgradPlan p;
  if (maxM % 128 != 0 || maxK % 128 != 0) {
    p.rc = FACPPG_EINVAL;
    snprintf(p.msg, sizeof(p.msg), "k_wgrad: M and K must be multiples of 128 (got %d, %d)", maxM, maxK);
    return p;
  }
  const int nall = B * ((L + 63) / 64);
  auto fit = [&](int ns) {
    ns = std::max(1, std::min(std::min(ns, WG_MAXSPLIT), nall));
    while (ns > 1 && (size_t)nprob * ns * maxM * maxK * 4 > part_bytes) --ns;
    return ns;
  };
  const int tiles256 = ((maxK + 255) / 256) * ((maxM + 255) / 256) * nprob;
  const int ns256 = fit(256 / std::max(tiles256, 1));
  const bool big = t.wgrad_tile ? t.wgrad_tile == 256 : (tiles256 >= 32 && nall / ns256 >= 24);
  p.tile = big ? 256 : 128;
  const int tiles128 = ((maxK + 127) / 128) * ((maxM + 127) / 128) * nprob;
  p.ns = big ? ns256 : fit((256 + tiles128 - 1) / std::max(tiles128, 1));
  p.tiles_k = (maxK + p.tile - 1) / p.tile; p.tiles_m = (maxM + p.tile - 1) / p.tile;
  p.ngroups = nprob * p.ns;
  p.xcd_map = big || !t.wgrad_no_xcd_map ? 1 : 0;
  if (p.xcd_map) { p.grid[0] = (unsigned)(8 * ((p.ngroups + 7) / 8) * p.tiles_k * p.tiles_m); p.grid[1] = p.grid[2] = 1; }
  else { p.grid[0] = (unsigned)p.tiles_k; p.grid[1] = (unsigned)p.tiles_m; p.grid[2] = (unsigned)p.ngroups; }
  p.lds = big ? kWgrad2Lds : kWgradLds;
  p.pstride = (size_t)maxM * maxK;
  p.part_floats = (size_t)p.ngroups * p.pstride;
  return p;
}

// the three launches of one stack: taps (3 nl problems [512 x 256]), conditioning (nl x [512 x 640]), res/skip (nl x [512 x 256])
struct WnWgradPlans { WgradPlan taps, cond, resskip; };
inline WnWgradPlans plan_wn_wgrads(const TrainTuning& t, int nl, int B, int L, size_t part_bytes) {
  return WnWgradPlans{plan_wgrad(t, nl * 3, 2 * C, C, B, L, part_bytes), plan_wgrad(t, nl, 2 * C, NCOND, B, L, part_bytes),
                      plan_wgrad(t, nl, 2 * C, C, B, L, part_bytes)};
}

// ---- the backward flow-edge launches of a group call ----
// nchunk: chunks of 32 positions a backward edge workgroup walks: at most ~512 workgroups (two per CU)
struct EdgePlan { int nchunk, gx, n_parts; };   // grid (gx, B); n_parts = B * gx partial sums per flow
inline EdgePlan plan_edges(const TrainTuning& t, int B, int L) {
  const int nblk = (L + 31) / 32;
  EdgePlan p;
  p.nchunk = std::max(1, (B * nblk + t.edge_wgs - 1) / t.edge_wgs);
  p.gx = (nblk + p.nchunk - 1) / p.nchunk;
  p.n_parts = B * p.gx;
  return p;
}

}  // namespace facppg
