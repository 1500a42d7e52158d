// Which kernels the Tacotron entry points of facppg_taco.hip launch, and in what shape: pure host arithmetic over the model's
// layer widths, the batch, the workgroup bound and the environment switches.  No HIP header, no launch: the entry points
// execute what these functions return, and facppg_taco_launch_plan reports the same plans to callers without a device
// (tests/test_taco_plan_cpu.py pins the table).  The constants the conditions depend on live here too; the kernels use the
// same definitions (FACPPG_HD: callable from device code where a HIP compiler reads this header).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "facppg.h"

namespace facppg {

constexpr int NTC = 512;  // threads of a cooperative decoder workgroup (8 waves, <= 256 VGPRs: no spills, deeper loads in flight)

// k_decoder_split's workers and k_decoder_forced<true>'s chain workgroups: register-resident weight slices
constexpr int SU = 4, SSC = 4 * SU, SKP = NTC / SSC;   // 16 rows x 32 K parts per workgroup
constexpr int SKR_LSTM = 40, SKR_PROJ = 32, SKR_P1 = 4, SKR_P2 = 12;   // columns per thread: K <= 1280 / 1024 / 128 / 384
constexpr int SKR_FA = 32;   // k_decoder_forced<true>, columns per thread: E + A <= 1024
constexpr int SNU = 4;   // max utterances sharing one set of workers
// A worker that has published its rows stays off the exchange words for SPLIT_PAUSE x 128 cycles (0.85 us at 2.4 GHz) before it
// starts to poll them -- ahead of the gate / X1, X2, AH and DH gathers.  The words of one exchange are a few KB in a few L2 channels,
// and 75 workgroups poll them with their eight waves: polls that start the moment the matvec ends (no barrier holds the waves back
// any more) queue ahead of the very stores they wait for and of the main workgroup's query-weight stream.  Without the pause the
// one-barrier stages make the FRAME slower than the legacy ones; with it they are faster, and faster than the legacy stages with
// the same pause, in every launch shape (Tacotron2.inference alone, 200 frames, ms, medians of 12, two alternating rounds each,
// round-to-round spread <= 0.03; `legacy` is the parent's code; profiles/r20_decoder_ab.txt section 7):
//   B, NU, workgroups      legacy   legacy + pause 16   one-barrier, no pause   one-barrier + pause 16   + pause 24
//   1, 1,  76               4.84         4.77                  4.93                    4.59                4.75
//   2, 1, 152               5.05         4.89                  5.21                    4.73                4.86
//   3, 1, 228               5.23         4.99                  5.40                    4.82                4.93
//   2, 2,  77               6.40         6.34                  6.46                    6.31                6.35
//   3, 3,  78               8.79         8.71                  8.42                    8.34                8.25
//   8, 3, 234 (3 groups)    9.34         9.23                  9.02                    8.94                8.78
// (legacy + pause 12 / 20 at B = 1: 4.76 / 4.88.)  The length was scanned at B = 1 only: no pause 4.85-4.93, 0.43 us 4.84, 0.53 us
// 4.76, 0.64 us 4.55-4.69, 0.75 us 4.50-4.61, 0.85 us 4.51-4.59, 0.96 us 4.53-4.60, 1.07 us 4.55-4.65, 1.28 us 4.63-4.75, 1.7 us 4.87,
// 2.6 us 5.37; each of the four pauses contributes (leaving one out: 4.54-4.77); a pause ahead of the context gather as well changes
// nothing.  With NU = 3 a longer pause would gain another 1 %; one constant serves all shapes.  The batch-1 bench runs the streamed
// path (the vocoder's seed passes under the decoder) and is the headline figure.  FACPPG_DECODER_PAUSE=n overrides (A/B runs; it
// also gives the legacy stages, which have none by default, the same pauses).
constexpr int SPLIT_PAUSE = 16;
constexpr int SPLIT_QR = 24;   // query-weight rows (float4) a thread of the main workgroup holds per frame

constexpr size_t LDS_CAP = 160 * 1024 - 1024;   // dynamic LDS a decoder workgroup may ask for
constexpr size_t Q_ROW_BYTES = (size_t)NTC * 16;   // one query-weight row of the main workgroup: a float4 per thread

#ifdef __HIPCC__
#define FACPPG_HD __host__ __device__
#else
#define FACPPG_HD
#endif

static FACPPG_HD inline int plan_round_up(int x, int m) { return (x + m - 1) / m * m; }

// floats of the decoder's LDS state (dec_carve)
static FACPPG_HD inline size_t dec_lds_floats(int P, int E, int A, int D, int NF, int AD, int NFIL, int KSZ, int Tin) {
  // feat [32][64], lconv^T [2*KSZ (even)][32], ldense [32][ADp32], v / processed query [ADp32]
  (void)NFIL;
  const size_t ADp32 = plan_round_up(AD, 32);
  return (size_t)(P + E + A) + (A + E + D) + (D + E) + A + D + plan_round_up(NF, 4) + plan_round_up(P, 4) + ADp32 + 4096 +
         64 * 32 + (size_t)plan_round_up(2 * KSZ, 2) * 32 + 32 * ADp32 + ADp32 + 3 * (size_t)Tin;
}

// In the wave layout the 32 K parts of an operand vector are distinct addresses of one LDS read, so the vector is kept with K part kp
// at kp * KRS floats: KRS = KR rounded up to a multiple of 4 whose quarter is odd.  A part is then read as float4 (a quarter of the
// reads of the legacy stage, which is bound by their latency), and the 16 lanes of a ds_read_b128 lane group -- 16 K parts that are
// distinct modulo 16 -- fall on 16 distinct 16-byte slots of the 256-byte bank row.  The padding stays zero.
static FACPPG_HD inline int stat_krs(int K) {
  const int k4 = plan_round_up((K + SKP - 1) / SKP, 4);
  return (k4 >> 2) & 1 ? k4 : k4 + 4;
}

// floats of a worker's operand vectors per utterance (legacy: plain, with the unused xin; else padded)
static FACPPG_HD inline int split_ustride(int P, int E, int A, int D, int NF, bool legacy) {
  return legacy ? (P + E + A) + (A + E + D) + (D + E) + plan_round_up(NF, 4) + plan_round_up(P, 4)
                : SKP * (stat_krs(P + E + A) + stat_krs(A + E + D) + stat_krs(D + E) + stat_krs(P));
}

// ------------------------------------------------------------------------------------------
// The environment switches of the Tacotron entry points (INTEGRATION.md lists them), parsed once per call.
struct TacoTuning {
  bool mode_split, mode_coop, mode_single;   // FACPPG_DECODER_MODE=split|coop|single forces a decoder shape
  const char* coop_u_env;                    // FACPPG_DECODER_COOP_U (tests / tuning): one slice width, as text (null = unset) ...
  int coop_u;                                // ... and as the integer it is compared by
  bool no_split;                             // FACPPG_DECODER_NO_SPLIT (any value): never the split shape
  int split_max_nu;                          // FACPPG_DECODER_SPLIT_MAX_NU: utterances per worker set at most (default 3:
                                             // 4 only ties with the cooperative kernel, 12.5 vs 12.4 ms at B = 12)
  bool decoder_legacy;                       // FACPPG_DECODER_STEP=legacy: the worker stages up to round 19
  bool has_qres; int qres;                   // FACPPG_DECODER_QRES (A/B runs): LDS-resident query-weight rows at most
  bool has_pause; int pause;                 // FACPPG_DECODER_PAUSE (A/B runs): units of 128 cycles, 0 = none
  bool no_rows;                              // FACPPG_DECODER_NO_ROWS (any value): DecArgs.dbg_flags bit 0
  bool prof;                                 // FACPPG_DECODER_PROF (any value): phase cycle counters, printed after the launch
  bool bilstm_single, bilstm_wide;           // FACPPG_BILSTM_MODE=single (one-workgroup kernel) | wide (64-unit slices)
  bool bilstm_legacy;                        // FACPPG_BILSTM_STEP=legacy: the three-barrier step
  bool forced_no_regw;                       // FACPPG_FORCED_NO_REGW (any value): streamed attention-LSTM slices at B <= 2 too
};

inline TacoTuning taco_tuning_from_env() {
  auto is = [](const char* v, const char* what) { return v && !strcmp(v, what); };
  auto num = [](const char* v) { return v ? atoi(v) : 0; };
  TacoTuning t;
  const char* mode = getenv("FACPPG_DECODER_MODE");
  t.mode_split = is(mode, "split"); t.mode_coop = is(mode, "coop"); t.mode_single = is(mode, "single");
  t.coop_u_env = getenv("FACPPG_DECODER_COOP_U"); t.coop_u = num(t.coop_u_env);
  t.no_split = getenv("FACPPG_DECODER_NO_SPLIT") != nullptr;
  const char* max_nu = getenv("FACPPG_DECODER_SPLIT_MAX_NU");
  t.split_max_nu = max_nu ? atoi(max_nu) : 3;
  t.decoder_legacy = is(getenv("FACPPG_DECODER_STEP"), "legacy");
  const char* qres = getenv("FACPPG_DECODER_QRES");
  t.has_qres = qres != nullptr; t.qres = num(qres);
  const char* pause = getenv("FACPPG_DECODER_PAUSE");
  t.has_pause = pause != nullptr; t.pause = num(pause);
  t.no_rows = getenv("FACPPG_DECODER_NO_ROWS") != nullptr;
  t.prof = getenv("FACPPG_DECODER_PROF") != nullptr;
  const char* bilstm = getenv("FACPPG_BILSTM_MODE");
  t.bilstm_single = is(bilstm, "single"); t.bilstm_wide = is(bilstm, "wide");
  t.bilstm_legacy = is(getenv("FACPPG_BILSTM_STEP"), "legacy");
  t.forced_no_regw = getenv("FACPPG_FORCED_NO_REGW") != nullptr;
  return t;
}

// ------------------------------------------------------------------------------------------
// What the plans need of a handle: the layer widths, the packed slice widths, and the co-residency bound of the device.
struct TacoGeometry {
  int P, E, A, D, AD, NF, NFIL, KSZ, H;
  // per-workgroup LSTM slices of k_decoder_coop / k_decoder_forced, packed for five slice widths: at the reference's 300 units
  // U = 8 (38 workgroups per utterance), 20 (15), 40 (8), 75 (4), 150 (2)
  int coop_U[5], coop_nwg[5];
  int split_nwk;    // k_decoder_split's workers (and k_decoder_forced<true>'s chain workgroups): 4 units each
  int coop_limit;   // workgroups the cooperative kernels may keep co-resident (facppg_taco_create); 0: none
};

inline TacoGeometry taco_geometry(const facppg_taco_config& c, int coop_limit) {
  TacoGeometry g;
  g.P = c.prenet_dim; g.E = c.encoder_embedding_dim; g.A = c.attention_rnn_dim; g.D = c.decoder_rnn_dim; g.AD = c.attention_dim;
  g.NF = c.n_acoustic_feat_dims; g.NFIL = c.attention_location_n_filters; g.KSZ = c.attention_location_kernel_size; g.H = g.E / 2;
  const int CUs[5] = {8, 20, 40, 75, 150};
  for (int v = 0; v < 5; ++v) { g.coop_U[v] = CUs[v]; g.coop_nwg[v] = (g.A + CUs[v] - 1) / CUs[v]; }
  g.split_nwk = (g.A + SU - 1) / SU;
  g.coop_limit = coop_limit;
  return g;
}

// the decoder holds a CU's whole LDS per workgroup: a caller that runs it UNDER another stream's kernels (the vocoder of
// the previous batch, facppg.pipeline.synthesize_stream) bounds the CUs it takes away from them
inline int taco_wg_limit(const TacoGeometry& g, int max_workgroups) {
  return max_workgroups > 0 && max_workgroups < g.coop_limit ? max_workgroups : g.coop_limit;
}

// A plan in place of which rc != FACPPG_OK holds a verdict: the code and the message the entry point returns.
struct PlanVerdict {
  int rc = FACPPG_OK;
  char msg[160] = "";
};
#define FACPPG_PLAN_REQUIRE(plan, cond, code, ...)           \
  do {                                                       \
    if (!(cond)) {                                           \
      (plan).rc = (code);                                    \
      snprintf((plan).msg, sizeof((plan).msg), __VA_ARGS__); \
      return (plan);                                         \
    }                                                        \
  } while (0)

// ---- the encoder's BiLSTM recurrence ----
// latency shapes: W_hh register-resident, sliced over co-resident workgroups per (utterance, direction):
// 32 units per workgroup (4 K parts of <= 96 columns) while they fit, else 64 units (2 K parts of <= 152); else k_bilstm
enum { BILSTM_SINGLE = 0, BILSTM_COOP32 = 1, BILSTM_COOP64 = 2 };
struct BilstmPlan {
  int kind;      // BILSTM_*
  bool legacy;   // cooperative kinds: the three-barrier step
  int grid[3];
};

inline BilstmPlan plan_bilstm(const TacoGeometry& g, int B, const TacoTuning& t) {
  const int H = g.H;
  const bool fit32 = (long)B * 2 * ((H + 31) / 32) <= g.coop_limit && (H + 3) / 4 <= 96 && !t.bilstm_wide;
  const bool fit64 = (long)B * 2 * ((H + 63) / 64) <= g.coop_limit && (H + 1) / 2 <= 152;
  BilstmPlan p;
  p.kind = t.bilstm_single || !(fit32 || fit64) ? BILSTM_SINGLE : fit32 ? BILSTM_COOP32 : BILSTM_COOP64;
  p.legacy = p.kind != BILSTM_SINGLE && t.bilstm_legacy;
  p.grid[0] = p.kind == BILSTM_SINGLE ? 2 : (H + (p.kind == BILSTM_COOP32 ? 31 : 63)) / (p.kind == BILSTM_COOP32 ? 32 : 64);
  p.grid[1] = p.kind == BILSTM_SINGLE ? B : 2;
  p.grid[2] = p.kind == BILSTM_SINGLE ? 1 : B;
  return p;
}

// ---- Decoder.inference ----
// mode 0, k_decoder: one workgroup per utterance, the throughput shape and the fallback.
// mode 1, k_decoder_coop: coop_nwg[v] cooperating workgroups per utterance, the narrowest slices (most workgroups) that keep the
//   batch co-resident; beyond that the widest slices run it in chunks of co-resident utterances, one cooperative launch after
//   the other (0.31 ms per utterance at 200 frames; the one-workgroup kernel needs 0.45).
// mode 2, k_decoder_split<NU>: split_nwk register-resident dense-layer workers serve NU utterances, each with its own main
//   (attention) workgroup.  NU = the fewest utterances per worker set that keeps every workgroup co-resident; a worker's
//   per-frame work grows with NU, so beyond split_max_nu the cooperative kernel wins.
struct DecodePlan : PlanVerdict {
  int mode;
  int variant;           // modes 1, 2: the slice widths DecArgs starts out with (index into coop_U); -1 in mode 0
  int NU;                // mode 2: utterances per worker set
  int step;              // mode 2: 1 = one-barrier worker stages, 2 = FACPPG_DECODER_STEP=legacy; else 0
  // launches: `launches - 1` of `chunk` utterances at slice widths v_full, then one of last_nb at v_last (modes 0, 2: one launch of B)
  int chunk, launches, last_nb, v_full, v_last;
  int q_res, pause, dbg_flags;   // mode 2: DecArgs fields of the same names
  size_t lds_state;      // modes 0, 1: dynamic LDS, the decoder's state
  size_t lds_split;      // mode 2: dynamic LDS, the larger of a worker's and the main workgroup's
  int grid[2];           // of the last launch
  bool publish;          // mode 2: the frames are published as tagged words
  bool prof;
  int workgroups() const { return grid[0] * grid[1]; }
};

inline DecodePlan plan_decode(const TacoGeometry& g, int B, int Tin, int max_steps, int max_workgroups, bool want_frame_words,
                              const TacoTuning& t) {
  (void)max_steps;
  DecodePlan p;
  p.mode = 0; p.variant = -1; p.NU = 0; p.step = 0; p.chunk = p.last_nb = B; p.launches = 1; p.v_full = p.v_last = -1;
  p.q_res = p.pause = p.dbg_flags = 0; p.lds_split = 0; p.grid[0] = B; p.grid[1] = 1; p.publish = false; p.prof = t.prof;
  p.lds_state = dec_lds_floats(g.P, g.E, g.A, g.D, g.NF, g.AD, g.NFIL, g.KSZ, Tin) * 4;
  FACPPG_PLAN_REQUIRE(p, p.lds_state <= LDS_CAP, FACPPG_EUNSUPPORTED, "decoder state (%zu bytes) exceeds LDS", p.lds_state);
  const int wg_limit = taco_wg_limit(g, max_workgroups);
  const bool force_u = t.coop_u_env != nullptr;
  for (int v = 0; v < 5 && p.variant < 0; ++v)
    if ((long)B * g.coop_nwg[v] <= wg_limit && (!force_u || t.coop_u == g.coop_U[v])) p.variant = v;
  if (p.variant < 0 && !force_u && wg_limit / g.coop_nwg[4] >= 1) { p.variant = 4; p.chunk = wg_limit / g.coop_nwg[4]; }
  const bool coop = p.variant >= 0 && !t.mode_single;
  if (t.mode_coop) FACPPG_PLAN_REQUIRE(p, coop, FACPPG_EUNSUPPORTED, "coop decoder needs B <= 120");
  // (the larger of the two worker layouts, so that NU does not depend on FACPPG_DECODER_STEP)
  const size_t ustride = std::max(split_ustride(g.P, g.E, g.A, g.D, g.NF, true), split_ustride(g.P, g.E, g.A, g.D, g.NF, false));
  int NU = 0;
  for (int nu = 1; nu <= SNU && nu <= t.split_max_nu && !NU; ++nu)
    if ((long)((B + nu - 1) / nu) * (g.split_nwk + nu) <= wg_limit && (nu * ustride + 1024) * 4 <= 150 * 1024) NU = nu;
  const bool split = coop && !t.no_split && NU > 0 && g.P + g.E + g.A <= SKP * SKR_LSTM && g.A + g.E + g.D <= SKP * SKR_LSTM &&
                     g.D + g.E <= SKP * SKR_PROJ && g.NF <= SKP * SKR_P1 && g.P <= SKP * SKR_P2 && g.NF + 1 <= g.split_nwk * SSC &&
                     g.P <= g.split_nwk * SSC && !t.mode_coop;
  if (t.mode_split)
    FACPPG_PLAN_REQUIRE(p, split, FACPPG_EUNSUPPORTED, "split decoder needs a small batch and the reference's layer widths");
  if (!coop) { p.variant = -1; p.chunk = B; return p; }
  if (split) {
    p.mode = 2; p.NU = NU; p.step = t.decoder_legacy ? 2 : 1; p.chunk = B;
    size_t main_lds = (plan_round_up((int)(p.lds_state / 4), 4) + (size_t)8 * NTC * 4) * 4;   // + attn_energy_pre's stash
    // ... + as many of the main workgroup's query-weight rows as the rest of the LDS holds
    p.q_res = t.decoder_legacy || main_lds > LDS_CAP ? 0 : (int)std::min<size_t>(SPLIT_QR, (LDS_CAP - main_lds) / Q_ROW_BYTES);
    if (t.has_qres) p.q_res = std::max(0, std::min(p.q_res, t.qres));
    main_lds += p.q_res * Q_ROW_BYTES;
    p.lds_split = std::max((NU * ustride + 1024) * 4, main_lds);
    p.dbg_flags = t.no_rows ? 1 : 0;
    p.pause = t.has_pause ? std::max(0, std::min(255, t.pause)) : t.decoder_legacy ? 0 : SPLIT_PAUSE;
    p.grid[0] = g.split_nwk + NU; p.grid[1] = (B + NU - 1) / NU;
    p.publish = B == 1 && want_frame_words;
    return p;
  }
  p.mode = 1;
  // a chunk may be small enough for narrower slices than the batch
  auto chunk_variant = [&](int nb) {
    if (!force_u)
      for (int v = 0; v < p.variant; ++v)
        if ((long)nb * g.coop_nwg[v] <= wg_limit) return v;
    return p.variant;
  };
  p.launches = (B + p.chunk - 1) / p.chunk;
  p.last_nb = B - (p.launches - 1) * p.chunk;
  p.v_full = chunk_variant(p.chunk < B ? p.chunk : B); p.v_last = chunk_variant(p.last_nb);
  p.grid[0] = g.coop_nwg[p.v_last]; p.grid[1] = p.last_nb;
  return p;
}

// ---- Decoder.forward, the teacher-forced recurrence ----
// One launch per chunk of co-resident utterances (one launch whenever B * workgroups-per-utterance fit).  Slice widths: the
// narrowest chain slices (the dependent chain) whose workgroups, with decoder-LSTM workgroups of the same or the next width
// (they have a frame's slack), stay co-resident for nb utterances; FACPPG_DECODER_COOP_U forces one width for both roles.
// Up to 2 utterances: register-resident attention-LSTM slices of 4 units (k_decoder_forced<true>, regw) next to the
// narrowest decoder slices.  Beyond what fits, the widest slices run the batch in chunks.
struct ForcedPlan : PlanVerdict {
  bool regw;
  int vc, vd;             // slice widths (indices into coop_U) of the chain and the decoder-LSTM workgroups, full chunks
  int vc_last, vd_last;   // ... of the last launch
  int chunk, launches, last_nb;
  size_t lds;             // a chain workgroup: the decoder's LDS state + attn_energy_pre's stash ([8][NTC] float4)
  int grid[2];            // of the last launch
  bool prof;
  int workgroups() const { return grid[0] * grid[1]; }
};

// workgroups per utterance of a launch with slice widths (vc, vd)
inline int forced_chain_wgs(const TacoGeometry& g, const ForcedPlan& p, int vc) { return p.regw ? g.split_nwk : g.coop_nwg[vc]; }

inline ForcedPlan plan_forced(const TacoGeometry& g, int B, int Tin, int max_workgroups, const TacoTuning& t) {
  ForcedPlan p;
  p.regw = false; p.vc = p.vd = p.vc_last = p.vd_last = 4; p.chunk = p.last_nb = B; p.launches = 1; p.grid[0] = p.grid[1] = 0;
  p.prof = t.prof;
  p.lds = (plan_round_up((int)dec_lds_floats(g.P, g.E, g.A, g.D, g.NF, g.AD, g.NFIL, g.KSZ, Tin), 4) + (size_t)8 * NTC * 4) * 4;
  FACPPG_PLAN_REQUIRE(p, p.lds <= LDS_CAP, FACPPG_EUNSUPPORTED, "decoder state (%zu bytes) exceeds LDS", p.lds);
  const int wg_limit = taco_wg_limit(g, max_workgroups);
  FACPPG_PLAN_REQUIRE(p, wg_limit >= 2 * g.coop_nwg[4], FACPPG_EUNSUPPORTED,
                      "the teacher-forced decoder needs %d co-resident workgroups, %d allowed", 2 * g.coop_nwg[4], wg_limit);
  const bool force_u = t.coop_u_env != nullptr;
  auto pick = [&](int nb, int* vc, int* vd) {
    for (int c2 = 0; c2 < 5; ++c2) {
      if (force_u && t.coop_u != g.coop_U[c2]) continue;
      for (int d2 = c2; d2 <= (force_u ? c2 : std::min(c2 + 1, 4)); ++d2)
        if ((long)nb * (g.coop_nwg[c2] + g.coop_nwg[d2]) <= wg_limit) { *vc = c2; *vd = d2; return true; }
    }
    return false;
  };
  p.regw = !force_u && !t.forced_no_regw && (long)B * (g.split_nwk + g.coop_nwg[0]) <= wg_limit && g.E + g.A <= SKP * SKR_FA &&
           g.A <= g.split_nwk * SU;
  if (p.regw) p.vc = p.vd = 0;
  else if (!pick(B, &p.vc, &p.vd)) {
    FACPPG_PLAN_REQUIRE(p, !force_u, FACPPG_EUNSUPPORTED, "FACPPG_DECODER_COOP_U=%s does not fit B = %d", t.coop_u_env, B);
    p.vc = p.vd = 4; p.chunk = wg_limit / (2 * g.coop_nwg[4]);
  }
  p.launches = (B + p.chunk - 1) / p.chunk;
  p.last_nb = B - (p.launches - 1) * p.chunk;
  p.vc_last = p.vc; p.vd_last = p.vd;   // the last chunk may be small enough for narrower slices
  if (p.last_nb < p.chunk && !force_u && !p.regw) pick(p.last_nb, &p.vc_last, &p.vd_last);
  p.grid[0] = forced_chain_wgs(g, p, p.vc_last) + g.coop_nwg[p.vd_last]; p.grid[1] = p.last_nb;
  return p;
}

}  // namespace facppg
