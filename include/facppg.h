/* facppg.h -- C ABI of libfacppg_hip.so: the MI355X (gfx950) implementation of the
 * PPG -> mel -> waveform synthesis hot path of guanlongzhao/fac-via-ppg.
 *
 * The reference has no FFI/plugin layer (it is 100 % Python on torch ops); its boundary is
 * the Python surface listed in SURVEY.md section 8b.  This header is the C ABI that sits
 * directly beneath that surface: every entry point names the reference function it
 * replaces (file:line under /root/reference).  The Python modules in fac-via-ppg_amd/
 * (common.*, waveglow.*, script.*) keep the reference's names and call these through ctypes.
 *
 * Conventions
 *   - return 0 on success, a negative FACPPG_E* code otherwise; nothing throws across the ABI;
 *     facppg_last_error() gives a thread-local message for the last failure.
 *   - every pointer named *_dev is DEVICE memory owned by the caller (e.g. a torch tensor);
 *     a handle owns only its packed weights.  All work is enqueued on the caller's
 *     hipStream_t (passed as void*); no entry point synchronises unless it says so.
 *   - a handle is bound to one device and is not thread-safe; handles on different devices
 *     are independent (one process per GPU).
 *   - all tensors are fp32, dense, row-major in the layouts given per function.
 */
#ifndef FACPPG_H
#define FACPPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FACPPG_VERSION 103 /* 0.1.2 */

#define FACPPG_OK 0
#define FACPPG_EINVAL (-1)       /* bad argument (NULL pointer, non-positive size, ...) */
#define FACPPG_EUNSUPPORTED (-2) /* configuration outside what the kernels are built for */
#define FACPPG_EHIP (-3)         /* a HIP runtime call failed */
#define FACPPG_EWORKSPACE (-4)   /* workspace smaller than facppg_*_workspace_bytes() */

int facppg_version(void);
/* Thread-local, valid until the next failing call on this thread. */
const char* facppg_last_error(void);

/* ------------------------------------------------------------------------------------
 * WaveGlow vocoder (src/waveglow/glow.py)
 * ---------------------------------------------------------------------------------- */

/* Constructor arguments of WaveGlow.__init__ (glow.py:179-206) / config.json:29-41. */
typedef struct facppg_wg_config {
  int32_t n_mel_channels; /* 80 */
  int32_t hop_length;     /* 160 (reference) or 256; must be a multiple of n_group */
  int32_t n_flows;        /* 12 */
  int32_t n_group;        /* 8 */
  int32_t n_early_every;  /* 4 */
  int32_t n_early_size;   /* 2 */
  int32_t wn_layers;      /* 8  (WN_config.n_layers)   */
  int32_t wn_channels;    /* 256 (WN_config.n_channels) */
  int32_t wn_kernel_size; /* 3  (WN_config.kernel_size) */
  int32_t upsample_kernel; /* 1024: ConvTranspose1d kernel size, glow.py:184-186 */
  int32_t alternate_halves; /* 0; 1 = legacy glow_old.py layout: odd flows condition on the second half */
} facppg_wg_config;

typedef struct facppg_wg facppg_wg;

/* Number of fp32 values in the plain weight blob facppg_wg_create() expects.  The blob is
 * the post-remove_weightnorm state dict (glow.py:295-311) flattened
 * in THIS order, each tensor dense row-major:
 *   upsample.weight [n_mel][n_mel][upsample_kernel], upsample.bias [n_mel]
 *   for k in 0..n_flows-1   (h_k = n_half of flow k, c_k = 2*h_k):
 *     WN.k.start.weight [C][h_k], WN.k.start.bias [C]
 *     for i in 0..wn_layers-1:
 *       WN.k.in_layers.i.weight [2C][C][ks], .bias [2C]
 *       WN.k.cond_layers.i.weight [2C][n_mel*n_group], .bias [2C]
 *       WN.k.res_skip_layers.i.weight [2C or C (last i)][C], .bias
 *     WN.k.end.weight [c_k][C], WN.k.end.bias [c_k]
 *     convinv.k  W_inverse [c_k][c_k]   (= conv.weight.squeeze().inverse(), glow.py:88-95)
 *     convinv.k  W [c_k][c_k]           (conv.weight.squeeze(), used by the training direction)
 */
size_t facppg_wg_weight_count(const facppg_wg_config* cfg);

/* Replaces: WaveGlow.__init__ + load_waveglow_model's weight preparation
 * (glow.py:179-206, common/utils.py:177-181).  Packs the plain blob into the MFMA operand
 * layouts on `device` using `stream`; synchronises that stream before returning, so the
 * caller may free `weights_dev` afterwards. */
int facppg_wg_create(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats,
                     int device, void* stream, facppg_wg** out);
void facppg_wg_destroy(facppg_wg* h);

/* Scratch bytes facppg_wg_infer needs for a batch of B mels of (max) T frames. */
size_t facppg_wg_workspace_bytes(const facppg_wg* h, int B, int T);

/* Replaces: WaveGlow.infer(spect, sigma) (glow.py:252-293), i.e. upsample + regroup, the
 * 12 x (WN, affine-coupling inverse, inverse 1x1 conv) flows, early-z concatenation and the
 * final group->time interleave.
 *   mel_dev   [B][n_mel][T]
 *   T_valid_dev  NULL, or [B] int32 frame counts <= T: utterance b is synthesised exactly as
 *             a batch-1 call on mel[b, :, :T_valid[b]] would be (frames beyond it are ignored,
 *             audio beyond T_valid[b]*hop is left untouched).
 *   z_dev     NULL -> noise is generated on the device from `seed` (Philox4x32-10 + Box-Muller);
 *             else the reference's three normal_() draws in call order, concatenated flat:
 *             [B][n_remaining][L] ++ [B][n_early_size][L] (flow 8) ++ [B][n_early_size][L] (flow 4),
 *             L = T*hop/n_group  (glow.py:261-270, 285-290).
 *   audio_dev [B][T*hop]
 */
int facppg_wg_infer(facppg_wg* h, const float* mel_dev, const int32_t* T_valid_dev,
                    const float* z_dev, uint64_t seed, float sigma, int B, int T,
                    float* audio_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The three normal_() draws of WaveGlow.infer (glow.py:261-270, 285-290) as PER-UTTERANCE streams:
 * writes z_dev in the flat injected-z layout of facppg_wg_infer for a batch of B mels of T frames, where
 * every value of utterance b is a function of seeds_dev[b] (uint64 [B]) and its own (draw, channel,
 * position) only.  A padded batch synthesised with this z therefore equals B independent batch-1 runs
 * with the same seeds, whatever the batch composition, padding or sharding over GPUs. */
int facppg_wg_draw_noise(const facppg_wg* h, const uint64_t* seeds_dev, int B, int T, float* z_dev,
                         void* stream);

/* Half-precision WaveGlow.infer: the reference's HalfTensor branch (glow.py:261-290), reached through
 * inference.py:38-48 --is_fp16 (waveglow.half(), convinv kept in fp32, mel.half()).
 * facppg_wg_create_f16 takes the SAME fp32 blob as facppg_wg_create (the half module's values widened), folds it
 * in fp32 and keeps only fp16 weight images (glow.py:179-206 / common/utils.py:177-181 as for facppg_wg_create).
 * facppg_wg_infer_f16 has the semantics of facppg_wg_infer (T_valid, flat injected-z layout, seed) with
 *   mel_dev [B][n_mel][T], z_dev (NULL or the flat layout) and audio_dev [B][T*hop] in IEEE fp16;
 * noise drawn from `seed` is facppg_wg_infer's Philox draw rounded to fp16.  Accumulation, the gate, the skip sum
 * and the flow-edge arithmetic (affine inverse, W_inverse, early z) run in fp32.
 * facppg_wg_workspace_bytes, facppg_wg_last_launch_shape, facppg_wg_draw_noise (fp32 values, any handle) and
 * facppg_wg_destroy accept either kind of handle; the other fp32 entry points return FACPPG_EINVAL for an fp16
 * handle and facppg_wg_infer_f16 does for an fp32 one (facppg_last_error names the mismatch). */
int facppg_wg_create_f16(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats,
                         int device, void* stream, facppg_wg** out);
int facppg_wg_infer_f16(facppg_wg* h, const uint16_t* mel_dev, const int32_t* T_valid_dev,
                        const uint16_t* z_dev, uint64_t seed, float sigma, int B, int T,
                        uint16_t* audio_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Replaces: WaveGlow.forward((spect, audio)) (glow.py:208-250), the training direction
 * audio -> z: upsample + crop to the audio length, 8-sample regroup, per flow the forward 1x1
 * mixing conv, WN, and a1 = exp(log_s)*a1 + b, with early outputs split off every n_early_every
 * flows.
 *   mel_dev [B][n_mel][F], audio_dev [B][N] (N a multiple of n_group; (F-1)*hop + kernel >= N)
 *   z_dev   [B][n_group][N/n_group]   = cat(early outputs..., final) along channels (glow.py:249)
 *   log_s_dev  the per-flow log_s tensors [B][h_k][N/n_group], flow 0 first, concatenated flat
 *              (facppg_wg_log_s_count values); log|det W_k| is a property of the weights alone and
 *              is left to the caller (glow.py:100).
 * Workspace: facppg_wg_workspace_bytes(h, B, ceil(N / hop)). */
size_t facppg_wg_log_s_count(const facppg_wg* h, int B, int N);
int facppg_wg_forward(facppg_wg* h, const float* mel_dev, const float* audio_dev, int B, int F,
                      int N, float* z_dev, float* log_s_dev, void* workspace_dev,
                      size_t workspace_bytes, void* stream);

/* Replaces Invertible1x1Conv.forward (glow.py:82-102) as a stand-alone op: out[b][i][l] = sum_j W[i][j] z[b][j][l]
 * for the c x c mixing matrix (c in {2,4,6,8}; z, out [B][c][L], not in place).  transpose_w != 0 applies W^T, which
 * is the op's data gradient; the reverse direction is the same call with W^-1.  log|det W| is a property of the
 * weights alone and is left to the caller (glow.py:100). */
int facppg_conv1x1(const float* w_dev, const float* z_dev, float* out_dev, int B, int c, int L,
                   int transpose_w, void* stream);
/* Its weight gradient dW[i][j] = sum_{b,l} dout[b][i][l] z[b][j][l], summed in a fixed order (bit-reproducible). */
size_t facppg_conv1x1_wgrad_workspace_bytes(int c);
int facppg_conv1x1_wgrad(const float* dout_dev, const float* z_dev, float* dw_dev, int B, int c, int L,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* Replaces torch.logdet(W) of Invertible1x1Conv.forward (glow.py:100) and, through winv_t = W^-T, its gradient
 * (d logdet / dW = W^-T): LU with partial pivoting of one c x c matrix (c <= 8) in one launch.  logdet_dev [1],
 * winv_t_dev [c][c].  NaN for a negative determinant, -inf for a singular matrix, as torch.logdet. */
int facppg_logdet(const float* w_dev, int c, float* logdet_dev, float* winv_t_dev, void* stream);

/* Replaces torch.nn.utils.weight_norm's per-conv recomputation (glow.py:118-146: w = g * v / ||v|| per output row) for
 * ALL weight-normed convs of the model in one launch, and its backward in one more.  table_dev: n_tensors entries of
 * 6 x 8 bytes {const float* v; const float* g; float* w; float* norm; int64 row0; int32 rows; int32 len} -- row0 = first
 * global row of the tensor (prefix sum of rows), len = elements per row; forward writes w and norm [rows].
 * Backward: same table with w := dw (read), norm (read); out_table_dev entries' v := dv, g := dg (written). */
int facppg_weight_norm_forward(const void* table_dev, int n_tensors, long total_rows, void* stream);
int facppg_weight_norm_backward(const void* table_dev, const void* out_table_dev, int n_tensors,
                                long total_rows, void* stream);

/* Replaces the reductions of WaveGlowLoss.forward (glow.py:43-59: torch.sum(z*z) and one torch.sum(log_s) per flow, 13 reduction
 * launches + 12 adds) by two launches: out[e] = sum over segment e, a segment being `outer` runs of `inner` contiguous floats
 * `outer_stride` elements apart (a flow's log_s is the upper half of every batch item of its WN output), squared first if
 * `square`.  Double accumulation, fixed summation order (bit-reproducible).  workspace: n * 64 doubles. */
#define FACPPG_MAX_SUM_SEGMENTS 16
typedef struct facppg_sum_segment {
  const float* data_dev;
  long outer_stride;
  int outer, inner;
  int square;
} facppg_sum_segment;
int facppg_segment_sums(const facppg_sum_segment* segs, int n, void* workspace_dev, size_t workspace_bytes, float* out_dev,
                        void* stream);

/* Replaces the affine coupling of WaveGlow.forward (glow.py:240-245): x = [x0 | x1] and wn_out = [b | log_s], all
 * [B][2h][L] fp32 -> y = cat(x0, exp(log_s) * x1 + b); and its backward: dx = [dy0 | dy1 exp(log_s)],
 * dwn_out = [dy1 | dy1 exp(log_s) x1] (the loss's own -sum(log_s) term reaches log_s through autograd separately). */
int facppg_affine_forward(const float* x_dev, const float* wn_out_dev, float* y_dev, int B, int h, int L, void* stream);
int facppg_affine_backward(const float* x_dev, const float* wn_out_dev, const float* dy_dev, float* dx_dev,
                           float* dwn_out_dev, int B, int h, int L, void* stream);

/* ---- WN training primitives (one flow's WN stack; WaveGlow training step, glow.py:154-175 +
 * its autograd backward).  Plain (un-packed, weight-norm already applied) device weights: */
typedef struct facppg_wn_weights {
  const float* start_w; /* [256][n_in] */
  const float* start_b; /* [256] */
  const float* in_w[8];   /* [512][256][3] */
  const float* in_b[8];   /* [512] */
  const float* cond_w[8]; /* [512][640] */
  const float* cond_b[8]; /* [512] */
  const float* rs_w[8];   /* [512][256], last layer [256][256] */
  const float* rs_b[8];
  const float* end_w; /* [2*n_in][256] */
  const float* end_b; /* [2*n_in] */
} facppg_wn_weights;
size_t facppg_wn_train_workspace_bytes(int n_layers, int B, int L);
/* Lr = round_up(L, 64), Lp = 128 + Lr + 128.  Forward of WN keeping what the backward needs:
 * h_all [n_layers+1][B][256][Lp], ts_all [n_layers][B][512][Lr], skip [B][256][Lr]. */
int facppg_wn_forward_save(const facppg_wn_weights* w, int n_in, int n_layers, const float* a0_dev,
                           const float* spect_pad_dev /*[B][640][Lr]*/, int B, int L, float* out_dev,
                           float* h_all_dev, float* ts_all_dev, float* skip_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);
/* Backward w.r.t. data; keeps dpre_all [n_layers][B][512][Lr], dh_all [n_layers+1][B][256][Lr] and
 * dskip [B][256][Lr] for the caller's weight-gradient matrix products; dspect [B][640][Lr], da0 [B][n_in][L]. */
int facppg_wn_backward_data(const facppg_wn_weights* w, int n_in, int n_layers, const float* dout_dev,
                            const float* ts_all_dev, int B, int L, float* dpre_all_dev,
                            float* dh_all_dev, float* dskip_dev, float* dspect_dev, float* da0_dev,
                            void* workspace_dev, size_t workspace_bytes, void* stream);

/* Weight and bias gradients of the stack from what facppg_wn_forward_save and facppg_wn_backward_data kept (the parameter half of
 * the autograd backward of src/waveglow/glow.py:154-175; reference: torch autograd over nn.Conv1d): every weight gradient
 * is an NT product over batch and positions on the exact-fp32 MFMA, every bias gradient a row sum, all in two launches,
 * deterministic.  g: fp32 outputs with the shapes of facppg_wn_weights. */
struct facppg_wn_grads;
size_t facppg_wn_weight_grads_workspace_bytes(int n_layers);
int facppg_wn_weight_grads(int n_in, int n_layers, const float* a0_dev, const float* spect_pad_dev, const float* h_all_dev,
                           const float* ts_all_dev, const float* skip_dev, const float* dout_dev, const float* dpre_all_dev,
                           const float* dh_all_dev, const float* dskip_dev, int B, int L, const struct facppg_wn_grads* g,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- the same stack with bf16 MFMA operands (BASELINE config 5: bf16 training, fp32 accumulation, fp32 master
 * weights and fp32 gradients).  Activations are kept POSITION-major ([B][Lr][channels] bf16, Lr =
 * facppg_wn_bf16_padded_len(L)) because the bf16 MFMA takes 8 consecutive reduction entries per lane; everything --
 * forward, data gradients AND the weight / bias gradients (NT products over the positions) -- runs in this library. */
typedef struct facppg_wn_grads {   /* fp32 outputs, same shapes as facppg_wn_weights */
  float* start_w; float* start_b;
  float* in_w[8]; float* in_b[8];
  float* cond_w[8]; float* cond_b[8];
  float* rs_w[8]; float* rs_b[8];
  float* end_w; float* end_b;
} facppg_wn_grads;
int facppg_wn_bf16_padded_len(int L);
/* ---- the whole model's training direction on the bf16 stack, GROUPS of consecutive flows per call (src/waveglow/glow.py:228-247 and
 * its autograd backward; src/script/train_waveglow.py:126-133).  Between two WN stacks everything is per-position arithmetic on <= 8
 * channels -- the end conv + affine coupling of the flow below (glow.py:175, 240-245), the early-output split (glow.py:231-233), the
 * 1x1 mixing conv (glow.py:98-102) and the start conv (glow.py:156) of the flow above: one launch per flow boundary and direction.
 * Per step: facppg_glow_bf16_begin once (packed bf16 weight images of every stack, zeroed margins of every flow's saved state), then
 * facppg_glow_bf16_group_forward per group in flow order, facppg_glow_bf16_group_backward per group in reverse order. */
#define FACPPG_GLOW_MAX_FLOWS 12
#define FACPPG_GLOW_PART_FLOATS 3400
typedef struct facppg_glow_bf16_sizes {
  size_t packed_bytes_per_flow;  /* bf16 operand images + summed gate biases of one flow's stack */
  size_t state_bytes_per_flow;   /* saved activations of one flow's stack (stride between flows in `states`) */
  size_t work_bytes;             /* gradients in flight of one flow's backward + reduction partials (shared by all flows) */
  int n_parts;                   /* workgroups of a backward edge launch: facppg_glow_flow.part is [n_parts][part_floats] */
  int part_floats;
} facppg_glow_bf16_sizes;
typedef struct facppg_glow_flow {
  const facppg_wn_weights* w;    /* effective (weight-normed) fp32 weights of the flow's WN, n_in = c / 2 */
  const facppg_wn_grads* g;      /* backward: where their gradients go */
  const float* conv_w;           /* [c][c] mixing matrix (Invertible1x1Conv, glow.py:62-102) */
  float* d_conv_w;               /* backward: its gradient, data term + g_logdet * ld_scale * W^-T */
  float* logdet;                 /* [1 + c*c]: ld_scale * log|det W| and W^-T, written by the forward, read by the backward */
  const float* g_logdet;         /* backward: upstream gradient of the flow's log_det_W output (one float), or NULL */
  float ld_scale;                /* B * L (glow.py:100) */
  int c;                         /* channels through the flow */
  int early;                     /* channels split off in front of it as an early output (glow.py:231-233), 0 if none */
  float* early_io; long early_bs; /* [B][early][L], batch stride early_bs floats: forward = the early output, backward = its gradient */
  float* u; float* z; float* wn_out; float* dzp;   /* [B][c][L] each: conv input, conv output, stack output (b | log_s), backward temp */
  const float* dlog_s; long dls_b, dls_j, dls_n;   /* backward: gradient of log_s = wn_out[:, c/2:] and its element strides (NULL: none) */
  float* part;                   /* backward: [n_parts][part_floats] partial sums */
  void* packed; void* state;                       /* this flow's slices of the step's `packed` and `states` buffers */
} facppg_glow_flow;
int facppg_glow_bf16_layout(int n_layers, int B, int L, facppg_glow_bf16_sizes* out);
int facppg_glow_bf16_begin(const facppg_wn_weights* wts /* [n_flows] */, int n_flows, int n_layers, int B, int L, void* packed_dev,
                           void* states_dev, void* work_dev, void* stream);
/* audio_in [B][flows[0].c + flows[0].early][L] -> audio_out [B][flows[n-1].c][L]; *_bs: batch strides in floats (rows are L apart) */
int facppg_glow_bf16_group_forward(const facppg_glow_flow* flows, int n, int n_layers, const float* audio_in_dev, long in_bs,
                                   float* audio_out_dev, long out_bs, const void* spect_pm_dev, int B, int L, void* stream);
int facppg_glow_bf16_group_backward(const facppg_glow_flow* flows, int n, int n_layers, const float* d_audio_out_dev, long d_out_bs,
                                    float* d_audio_in_dev, long d_in_bs, const void* spect_pm_dev, float* dspect_pm_dev, int accumulate_dspect,
                                    void* work_dev, int B, int L, void* stream);

size_t facppg_wn_bf16_state_bytes(int n_layers, int B, int L);    /* saved activations of one stack (forward -> backward) */
size_t facppg_wn_bf16_scratch_bytes(int n_layers, int B, int L);  /* per-call scratch (packed bf16 weight images, gradients in flight) */
/* Where the saved activations and the gradients in flight live inside `state` and `scratch` of the two calls below: byte offsets
 * of layer 0 and per-layer strides, from the carve the calls themselves use (csrc/facppg_train_plan.h) -- host-side only, for tests
 * and tools that read the buffers stage by stage.  State: h [n_layers + 1][B][Lp][256] bf16 (positions at rows [halo, halo + L)),
 * ts [n_layers][B][Lr][512] bf16, acts [n_layers][B][Lr][256] bf16, skip [B][Lr][256] fp32.  Scratch: dpre [n_layers][B][Lp][512]
 * bf16 (rows as h), dh [n_layers + 1][B][Lr][256] bf16, dskip [B][Lr][256] bf16.  *_end: one past the last byte of the last piece
 * (state_end = facppg_wn_bf16_state_bytes; the summed gate biases follow scratch_end).  FACPPG_EINVAL where the size queries return 0,
 * or out is NULL. */
typedef struct facppg_wn_bf16_offsets {
  int32_t Lr, Lp, halo;         /* padded positions per item, rows of an h / dpre image, margin rows on either side */
  int32_t reserved;
  size_t h, h_stride, ts, ts_stride, acts, acts_stride, skip, skip_bytes, state_end;
  size_t dpre, dpre_stride, dh, dh_stride, dskip, dskip_bytes, grads_end, scratch_end;
} facppg_wn_bf16_offsets;
int facppg_wn_bf16_layout(int n_layers, int B, int L, facppg_wn_bf16_offsets* out);
/* Which launches facppg_wn_forward_bf16 / facppg_wn_backward_bf16 use for B items of L positions (glow.py:154-175 and its autograd
 * backward), after the FACPPG_TRAIN_FUSED_FWD / _BWD, FACPPG_TRAIN_TILE and FACPPG_WGRAD_TILE overrides -- a diagnostic, host-side only:
 * bit 0: one launch per layer forward (k_wn_fwd) instead of two; bit 1: one launch per layer in the backward chain (k_wn_bwd);
 * bit 2: 256 x 256 weight-gradient tiles (k_wgrad2) for the tap and conditioning products; bits 8..15: positions per tile of the fused
 * launches (64 or 32).  Negative: bad argument. */
int facppg_wn_bf16_launch_plan(int n_layers, int B, int L);
/* The same decision in full, for the stand-alone calls above and the group calls (facppg_glow_bf16_*) alike: the host-side plan
 * alone, from the very functions the calls plan with (csrc/facppg_train_plan.h) -- no handle, no device.  The environment switches
 *  count as in the calls, which read them once per call.  FACPPG_EINVAL where facppg_wn_bf16_launch_plan is
 * negative, or out is NULL. */
typedef struct facppg_train_launch_report {
  int32_t tile_positions;       /* positions per tile of the fused layer launches: 64 or 32 */
  int32_t fused_fwd;            /* one launch per layer forward (k_wn_fwd) instead of two k_bgemm */
  int32_t fused_bwd;            /* one launch per layer in the backward chain (k_wn_bwd); never for a one-layer stack */
  int32_t fused_workgroups;     /* of a fused launch */
  /* the k_bgemm launches of the two-launch layers: gate, res/skip, res/skip of the last layer, gate backward, transposed conv */
  int32_t gemm_cols[5];         /* columns per tile: 128 or 64 */
  int32_t gemm_workgroups[5];
  int32_t dspect_bgemm;         /* conditioning gradient: 0 k_dspect, 1 k_bgemm (FACPPG_TRAIN_DSPECT_BGEMM=1) */
  int32_t dspect_cols;          /* k_bgemm: columns per tile; k_dspect: 0 */
  int32_t dspect_workgroups;
  int32_t dspect_lds_bytes;     /* dynamic LDS (k_bgemm: 0) */
  /* the weight-gradient products of one stack: taps (3 n_layers problems), conditioning, res/skip (n_layers each) */
  int32_t wgrad_tile[3];        /* 256 (k_wgrad2) or 128 (k_wgrad) */
  int32_t wgrad_splits[3];      /* position splits per output tile; > 1: partial sums and an ordered reduce */
  int32_t wgrad_workgroups[3];
  int32_t wgrad_xcd_map[3];     /* workgroups dealt to the XCDs by (problem, split); 0: FACPPG_WGRAD_NO_XCD_MAP=1 on 128-tiles */
  int32_t pack_per_step;        /* FACPPG_TRAIN_PACK=step */
  int32_t edge_nchunk;          /* 32-position chunks a backward edge workgroup walks */
  int32_t edge_n_parts;         /* facppg_glow_bf16_sizes.n_parts */
  int32_t upsample_gemm;        /* the upsampler as MFMA products where a workspace is passed (FACPPG_UPSAMPLE_GEMM=0: never) */
  int32_t fwd_lds_bytes;        /* dynamic LDS of k_wn_fwd / k_wn_bwd at tile_positions, of k_wgrad and of k_wgrad2 */
  int32_t bwd_lds_bytes;
  int32_t wgrad_lds_bytes;
  int32_t wgrad2_lds_bytes;
} facppg_train_launch_report;
int facppg_train_bf16_launch_plan(int n_layers, int B, int L, facppg_train_launch_report* out);
/* fp32 channel-major [B][channels][ld] (first L columns) -> bf16 position-major [B][Lr][channels], rows >= L zero */
int facppg_spect_to_bf16(const float* spect_dev, int B, int channels, int L, int ld, void* out_dev, void* stream);
/* fp32 position-major [B][Lr][channels] -> fp32 channel-major [B][channels][ld] (first L columns) */
int facppg_posmajor_to_f32(const float* src_dev, int B, int channels, int L, float* out_dev, int ld, void* stream);
/* Replaces WN.forward (glow.py:154-175): a0 [B][n_in][L] fp32, spect_pm bf16 [B][Lr][640] -> out [B][2*n_in][L] fp32. */
int facppg_wn_forward_bf16(const facppg_wn_weights* w, int n_in, int n_layers, const float* a0_dev,
                           const void* spect_pm_dev, int B, int L, float* out_dev, void* state_dev,
                           size_t state_bytes, void* scratch_dev, size_t scratch_bytes, void* stream);
/* Its autograd backward, complete: da0 [B][n_in][L], dspect_pm fp32 [B][Lr][640] (overwritten, or added to when
 * accumulate_dspect != 0: the flows of one step share the buffer) and all of `grads`. */
int facppg_wn_backward_bf16(const facppg_wn_weights* w, const facppg_wn_grads* grads, int n_in, int n_layers,
                            const float* a0_dev, const void* spect_pm_dev, const float* dout_dev, int B, int L,
                            const void* state_dev, size_t state_bytes, float* da0_dev, float* dspect_pm_dev,
                            int accumulate_dspect, void* scratch_dev, size_t scratch_bytes, void* stream);
/* Replaces WaveGlow.upsample + crop + regroup in the training direction (glow.py:184-186, 214-222), straight into
 * the bf16 position-major conditioning operand: mel [B][80][T] fp32, up_w [80][80][ksize], up_b [80] ->
 * spect_pm bf16 [B][Lr][640] for L = N/8 group positions (rows >= L zero). */
size_t facppg_upsample_forward_workspace_bytes(int B, int T, int n_mel, int hop, int ksize, int L);
/* workspace (may be NULL: the scalar kernels run): the transposed convolution as an exact-fp32 MFMA matrix product */
int facppg_upsample_regroup_bf16(const float* mel_dev, const float* up_w_dev, const float* up_b_dev, int B,
                                 int T, int n_mel, int hop, int ksize, int L, void* spect_pm_dev,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);
/* Its backward w.r.t. the parameters from the accumulated conditioning gradient dspect_pm fp32 [B][Lr][640]:
 * d_up_w [80][80][ksize], d_up_b [80]. */
size_t facppg_upsample_backward_workspace_bytes(int B, int T, int n_mel, int hop, int ksize, int L);
int facppg_upsample_regroup_backward(const float* mel_dev, const float* dspect_pm_dev, int B, int T, int n_mel,
                                     int hop, int ksize, int L, float* d_up_w_dev, float* d_up_b_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* Average device time (ms) of the dominant kernel (the fused WN layer) over the launches of
 * the most recent facppg_wg_infer on this handle, measured with hipEvents on the stream the
 * kernels ran on when profiling was enabled with facppg_wg_set_profiling(h, 1).  One event pair brackets the
 * back-to-back layer launches of a flow (nothing else runs between them) and the figure is that time / the layers:
 * a pair per launch costs a 78 us launch ~9 us of its own, and the summary of rocprofv3 --kernel-trace would not agree.  enable = n > 1 accumulates
 * over the next n facppg_wg_infer calls instead (their events are created by the set_profiling call itself, so
 * that a timed region creates none); any set_profiling call starts a new accumulation.  Synchronises
 * the recorded events.  *n_launches receives the number of launches averaged. */
int facppg_wg_set_profiling(facppg_wg* h, int enable);
int facppg_wg_last_layer_ms(facppg_wg* h, float* avg_ms, int* n_launches);

/* Shape of the fused-WN-layer launches of the most recent facppg_wg_infer on this handle: frames (phase-major
 * path) or group positions (FACPPG_WG_UNFOLDED=1) per tile, waves per workgroup, workgroups per launch.  The tile
 * width is picked per call from measured round costs; FACPPG_WN_TILE=16|32|64|128 in the environment forces one.
 * Lets the parity tests assert WHICH instantiation of k_wn_layer (glow.py:154-175) they compared with the oracle. */
int facppg_wg_last_launch_shape(const facppg_wg* h, int* tile_frames, int* waves, int* n_tiles);

/* Schedule of the 8-wave 32-frame layer tiles of the most recent facppg_wg_infer / facppg_wg_infer_seeded on this handle:
 * 2 = the small-launch schedule (second-GEMM operands requested ahead of the gate, write-through epilogue stores),
 * 1 = the schedule before it (FACPPG_WN_SMALL=legacy in the environment, read per call), 0 = the call ran no such tile.
 * Both schedules form the same sums in the same order: the outputs are equal bit for bit. */
int facppg_wg_last_layer_schedule(const facppg_wg* h, int* schedule);

/* ---- ONE utterance whose mel frames arrive over time (the metric's "batch = 1" case): the conditioning part of every WN
 * layer's gate GEMM ahead of the layers.  No reference counterpart as code -- the reference computes cond_layers[i](spect)
 * inside WN.forward (glow.py:154-175) on the upsampled mel (glow.py:253-259) -- but the same arithmetic: the fused layer
 * kernel accumulates bias + the folded conditioning chunks BEFORE any dilated tap, and that part depends on the mel frames
 * alone.  facppg_wg_cond_seed forms it for a block of frames and every (flow, layer, phase) with the layer kernel's own MFMA
 * sequence and parks the accumulators in `seeds`; facppg_wg_infer_seeded starts the layers from them (12 K chunks instead
 * of 17; first layers 1 instead of 6).  Same samples as facppg_wg_infer, bit for bit (tests/test_gpu_stream.py).
 *
 * facppg_wg_seed_layout: for an utterance of at most T frames, *Tqp = row length of the zero-margined mel buffer
 *   melp [n_mel][Tqp] (frame q at column *margin + q; the margins and every frame that is not (yet) there must be zero),
 *   *seed_bytes = size of the seed buffer.
 * facppg_wg_mel_pad: mel_dev [n_mel][ld] (T frames) -> melp_dev (zero margins written too).
 * facppg_wg_cond_seed: seeds of frames [frame0, frame0 + nframes) (frame0 a multiple of 32; the frames and the 3 before them
 *   must be final in melp), for flows [flow0, flow0 + nflows) (nflows <= 0: all).  block_tiles (1..4) 32-frame tiles share one
 *   pass over a weight image; layers_per_workgroup layers share one staging of the mel window.  *skip_dev != 0 (device, may be
 *   NULL): the launch does nothing.  max_workgroups > 0 bounds the launch to that many workgroups, which take the remaining
 *   work items from *counter_dev (a zeroed int32 on the device; NULL: strided) -- the CUs it leaves stay free for other streams.
 * facppg_wg_infer_seeded: WaveGlow.infer (glow.py:252-293) of the T frames in melp_dev, laid out (melp, seeds) for T_layout >= T
 *   frames.  Frames [0, seeded_frames) start from the seeds (seeded_frames a multiple of 32); the frames behind them run as
 *   unseeded 16-frame tiles of the same launches.  flow_events: NULL or n_flows hipEvent_t (NULL entries allowed): the launches
 *   of flow k first wait for flow_events[k] on `stream` (its seeds are still being formed on another stream).  z_dev / seed /
 *   sigma / audio_dev [T*hop] / workspace (facppg_wg_workspace_bytes(h, 1, T_layout)) as in facppg_wg_infer. */
int facppg_wg_seed_layout(const facppg_wg* h, int T, int* Tqp, int* margin, size_t* seed_bytes);
int facppg_wg_mel_pad(const facppg_wg* h, const float* mel_dev, int T, int ld, float* melp_dev, void* stream);
int facppg_wg_cond_seed(facppg_wg* h, const float* melp_dev, int T, int frame0, int nframes, int block_tiles,
                        int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                        const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream);
int facppg_wg_infer_seeded(facppg_wg* h, const float* melp_dev, int T_layout, int T, const float* seeds_dev,
                           int seeded_frames, const float* z_dev, uint64_t seed, float sigma, float* audio_dev,
                           void* workspace_dev, size_t workspace_bytes, void* const* flow_events, void* stream);

/* ---- The same for an fp16 handle (facppg_wg_create_f16): the reference's HalfTensor branch of WaveGlow.infer
 * (glow.py:252-293, 261-290) with WN.forward's cond_layers (glow.py:154-175) formed ahead of the layers.
 * The fp16 layer kernel's default K order is taps, then conditioning; a seed can only stand for the conditioning chunks if
 * they are summed first, and fp32 accumulation is not associative.  So the K order is an argument:
 * facppg_wg_infer_f16_order: facppg_wg_infer_f16 with cond_first = 0 (its bits) or 1 (the conditioning chunks from zero
 *   accumulators, then the taps; the bias is added at the gate either way).  The seeded path is conditioning-first throughout:
 *   facppg_wg_infer_seeded_f16 yields the bits of facppg_wg_infer_f16_order(cond_first = 1) on the same frames, whichever
 *   tiles were seeded.
 * facppg_wg_seed_layout_f16: as facppg_wg_seed_layout; the mel buffer is melp [Tqp][n_mel] in fp16 (frame q at row
 *   *margin + q, margins and missing frames zero), the seeds are raw fp32 gate accumulators (no bias) in the layer kernel's
 *   register order, 64 KiB per (flow, layer, phase, 32-frame tile).
 * facppg_wg_mel_pad_f16: frames [frame0, frame0 + nframes) of the fp32 mel_dev [n_mel][ld] -> melp_dev, rounded to nearest
 *   even; nothing else of melp_dev is written (the caller zeroes it once).  *skip_dev != 0 (may be NULL): does nothing.
 * facppg_wg_cond_seed_f16: the arguments of facppg_wg_cond_seed; layers_per_workgroup layers form one work item.
 * facppg_wg_infer_seeded_f16: the arguments of facppg_wg_infer_seeded with fp16 melp, injected z and audio.  The launches use
 *   32-frame tiles: tiles wholly inside [0, seeded_frames) (a multiple of 32, at most T rounded up to 32; 0 allowed) start from
 *   their seeds, the others run unseeded, conditioning-first, in the same launches.
 * An fp32 handle into any of these returns FACPPG_EINVAL (facppg_last_error names the mismatch), as an fp16 handle does into
 * the fp32 entry points above. */
int facppg_wg_infer_f16_order(facppg_wg* h, const uint16_t* mel_dev, const int32_t* T_valid_dev, const uint16_t* z_dev,
                              uint64_t seed, float sigma, int B, int T, int cond_first, uint16_t* audio_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);
int facppg_wg_seed_layout_f16(const facppg_wg* h, int T, int* Tqp, int* margin, size_t* seed_bytes);
int facppg_wg_mel_pad_f16(const facppg_wg* h, const float* mel_dev, int T, int ld, int frame0, int nframes,
                          uint16_t* melp_dev, const int32_t* skip_dev, void* stream);
int facppg_wg_cond_seed_f16(facppg_wg* h, const uint16_t* melp_dev, int T, int frame0, int nframes, int block_tiles,
                            int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                            const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream);
int facppg_wg_infer_seeded_f16(facppg_wg* h, const uint16_t* melp_dev, int T_layout, int T, const float* seeds_dev,
                               int seeded_frames, const uint16_t* z_dev, uint64_t seed, float sigma, uint16_t* audio_dev,
                               void* workspace_dev, size_t workspace_bytes, void* const* flow_events, void* stream);

/* ---- WaveGlow.infer (glow.py:252-293) on SPLIT bf16 operands: fp32 interface and fp32-class accuracy on the bf16 MFMA.
 * Every fp32 operand x of a WaveNet contraction (glow.py:154-175) is written as hi + lo, hi = RNE_bf16(x), lo = RNE_bf16(x - hi),
 * and a product A.B is A_hi.B_hi + A_hi.B_lo + A_lo.B_hi accumulated in fp32 (v_mfma_f32_32x32x16_bf16).  The hidden state, mel,
 * noise and audio stay fp32 in memory; accumulators, biases, the gate, the skip sum and all flow-edge arithmetic (affine inverse,
 * W_inverse, early z, start conv) are fp32.  The handle is a type of its own: it keeps only split weight images and is
 * accepted by these five entry points alone.
 * facppg_wg_split_create (glow.py:252-293; weights as glow.py:179-206 / common/utils.py:177-181): takes the SAME fp32 blob as
 *   facppg_wg_create, folds it in fp32 and keeps each image as two bf16 planes; accepts the configurations
 *   facppg_wg_create_f16 accepts and returns FACPPG_EUNSUPPORTED for the rest.
 * facppg_wg_split_destroy (glow.py:252-293): frees the handle (NULL allowed).
 * facppg_wg_split_workspace_bytes (glow.py:252-293): scratch bytes facppg_wg_split_infer needs for B mels of (max) T frames.
 * facppg_wg_split_infer (glow.py:252-293): the signature and semantics of facppg_wg_infer -- fp32 mel_dev [B][n_mel][T],
 *   T_valid_dev, flat injected z_dev or `seed` (facppg_wg_infer's Philox draw, unrounded), sigma, fp32 audio_dev [B][T*hop],
 *   caller-owned workspace, caller's stream.  An utterance gets the same bits in any batch and any tile width.
 * facppg_wg_split_last_launch_shape (glow.py:252-293, the layer launches of glow.py:154-175): frames per tile (32 or 64), waves
 *   per workgroup and workgroups per launch of the most recent facppg_wg_split_infer.  The width is picked per call
 *   from the launch shape; FACPPG_WG_SPLIT_TILE=32|64 in the environment forces one. */
typedef struct facppg_wg_split facppg_wg_split;
int facppg_wg_split_create(const facppg_wg_config* cfg, const float* weights_dev, size_t n_floats,
                           int device, void* stream, facppg_wg_split** out);
void facppg_wg_split_destroy(facppg_wg_split* h);
size_t facppg_wg_split_workspace_bytes(const facppg_wg_split* h, int B, int T);
int facppg_wg_split_infer(facppg_wg_split* h, const float* mel_dev, const int32_t* T_valid_dev,
                          const float* z_dev, uint64_t seed, float sigma, int B, int T,
                          float* audio_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int facppg_wg_split_last_launch_shape(const facppg_wg_split* h, int* tile_frames, int* waves, int* n_tiles);

/* ---- Seeded inference of ONE utterance on a split handle: WN.forward's cond_layers (glow.py:154-175) on the upsampled mel
 * (glow.py:253-259) formed ahead of the layers, as facppg_wg_*_f16 above do for an fp16 handle, with fp32 melp, fp32 injected z
 * and fp32 audio.  facppg_wg_split_infer sums the taps first and the conditioning chunks last; a seed can only stand for chunks
 * that are summed first from zero accumulators, and fp32 accumulation is not associative.  So the seeded path has a K order of
 * its own -- conditioning first --, and its samples differ from facppg_wg_split_infer's in the last bits (same accuracy: the
 * three terms per K step and accumulator keep their order).  facppg_wg_split_infer itself is unchanged.
 * facppg_wg_split_seed_layout (glow.py:253-259): as facppg_wg_seed_layout_f16 -- the mel buffer is melp [Tqp][n_mel] in fp32
 *   (frame q at row *margin + q, margins and missing frames zero), the seeds are raw fp32 gate accumulators (no bias) in the layer
 *   kernel's register order, 64 KiB per (flow, layer, phase, 32-frame tile) -- and *max_block_tiles, the largest block_tiles
 *   facppg_wg_split_cond_seed takes for this handle (the split window of a block must fit a CU's LDS: 3 at hop 256, 1 at hop 160).
 * facppg_wg_split_mel_pad (glow.py:253-259, the frames the upsampler reads): frames [frame0, frame0 + nframes) of the fp32
 *   mel_dev [n_mel][ld] -> melp_dev; nothing else of melp_dev is written (the caller zeroes it once).  *skip_dev != 0 (may be
 *   NULL): does nothing.
 * facppg_wg_split_cond_seed (glow.py:154-175, cond_layers): the arguments of facppg_wg_cond_seed_f16; a block_tiles above
 *   *max_block_tiles is refused, the message names the maximum.
 * facppg_wg_split_infer_seeded (glow.py:252-293): the arguments of facppg_wg_infer_seeded_f16; workspace
 *   facppg_wg_split_workspace_bytes(h, 1, T_layout).  The launches use 32-frame tiles: tiles wholly inside [0, seeded_frames) (a
 *   multiple of 32, at most T rounded up to 32) start from their seeds, the others run unseeded, conditioning-first, in the same
 *   launches -- a column gets the same bits either way.  seeded_frames = 0 is the unstreamed call with these bits.  Its launch
 *   shape is what facppg_wg_split_last_launch_shape then reports. */
int facppg_wg_split_seed_layout(const facppg_wg_split* h, int T, int* Tqp, int* margin, size_t* seed_bytes, int* max_block_tiles);
int facppg_wg_split_mel_pad(const facppg_wg_split* h, const float* mel_dev, int T, int ld, int frame0, int nframes,
                            float* melp_dev, const int32_t* skip_dev, void* stream);
int facppg_wg_split_cond_seed(facppg_wg_split* h, const float* melp_dev, int T, int frame0, int nframes, int block_tiles,
                              int layers_per_workgroup, int flow0, int nflows, float* seeds_dev, size_t seed_bytes,
                              const int32_t* skip_dev, int max_workgroups, int32_t* counter_dev, void* stream);
int facppg_wg_split_infer_seeded(facppg_wg_split* h, const float* melp_dev, int T_layout, int T, const float* seeds_dev,
                                 int seeded_frames, const float* z_dev, uint64_t seed, float sigma, float* audio_dev,
                                 void* workspace_dev, size_t workspace_bytes, void* const* flow_events, void* stream);

/* ------------------------------------------------------------------------------------
 * STFT / mel analysis / denoiser (src/common/stft.py, src/common/layers.py,
 * src/waveglow/denoiser.py)
 * ---------------------------------------------------------------------------------- */
typedef struct facppg_stft facppg_stft;

/* Replaces STFT.__init__ (stft.py:46-77) [+ TacotronSTFT.__init__ layers.py:75-87 when a mel
 * basis is given].  The caller supplies the constant tables (built on the host exactly as the
 * reference builds them) as device arrays:
 *   fwd_basis_dev   [filter_length+2][filter_length]  windowed DFT basis (real rows, then imag rows)
 *   inv_basis_t_dev [filter_length][filter_length+2]  TRANSPOSE of the windowed pinv basis
 *   win_sq_dev      [filter_length]  squared, centre-padded window (audio_processing.py:79-82)
 *   mel_basis_dev   [n_mel][filter_length/2+1] or NULL
 * Synchronises `stream` before returning. */
int facppg_stft_create(int filter_length, int hop_length, const float* fwd_basis_dev,
                       const float* inv_basis_t_dev, const float* win_sq_dev,
                       const float* mel_basis_dev, int n_mel, int device, void* stream,
                       facppg_stft** out);
void facppg_stft_destroy(facppg_stft* h);
size_t facppg_stft_workspace_bytes(const facppg_stft* h, int B, int N);

/* Replaces STFT.transform (stft.py:79-107): audio [B][N] -> magnitude, phase
 * [B][filter_length/2+1][N/hop+1] (phase_dev may be NULL).  n_valid_dev: NULL or [B] sample
 * counts <= N for padded batches (reflect padding is applied at each utterance's own end). */
int facppg_stft_transform(facppg_stft* h, const float* audio_dev, const int32_t* n_valid_dev,
                          int B, int N, float* mag_dev, float* phase_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
/* Replaces STFT.inverse (stft.py:109-138): magnitude, phase [B][cutoff][F] -> [B][hop*(F-1)]. */
int facppg_stft_inverse(facppg_stft* h, const float* mag_dev, const float* phase_dev, int B,
                        int F, float* out_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream);
/* Replaces TacotronSTFT.mel_spectrogram (layers.py:96-112) without its host-side range assert:
 * audio [B][N] in [-1,1] -> log(clamp(mel_basis . |STFT|, 1e-5)) [B][n_mel][N/hop+1]. */
int facppg_stft_mel(facppg_stft* h, const float* audio_dev, const int32_t* n_valid_dev, int B,
                    int N, float* mel_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Replaces Denoiser.forward (denoiser.py:63-68): STFT, magnitude - bias_spec*strength clamped
 * at 0, inverse STFT with the original phase.  bias_spec_dev [filter_length/2+1];
 * out [B][hop*(N/hop)]. */
int facppg_denoise(facppg_stft* h, const float* audio_dev, const int32_t* n_valid_dev,
                   const float* bias_spec_dev, float strength, int B, int N, float* out_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Vocoder-free preview: a mel back to a linear magnitude, and Griffin-Lim on the device.  BOTH
 * DEFINITIONS ARE THIS BUILD'S OWN: the reference has no mel inversion, and its griffin_lim
 * (audio_processing.py:91-107) draws NumPy phases on the host.
 *
 * Mel to magnitude.  P = pinv(mel_basis) [cutoff][n_mel] (cutoff = filter_length/2+1) is computed
 * by the caller on the host in float64, rounded to float32 and handed over once with
 * facppg_stft_set_mel_pinv (a handle created without a mel basis refuses it; the table must stay
 * alive until the stream has passed the call; nothing is synchronised).  Then
 *   mag = max(P . exp(mel), 0)   [B][cutoff][F]
 * for mel [B][n_mel][F] as facppg_stft_mel makes it (natural log of the clamped mel energies).
 * n_frames_dev: NULL or [B] frame counts <= F; frames at or beyond n_frames[b] are written as
 * zeros.  This is the pseudo-inverse seed of the usual NNLS inversion without the NNLS.
 * Workspace: B * n_mel * F floats (facppg_griffin_lim_workspace_bytes(h, B, F) covers it for F >= 2). */
int facppg_stft_set_mel_pinv(facppg_stft* h, const float* pinv_dev, void* stream);
int facppg_mel_to_magnitude(facppg_stft* h, const float* mel_dev, const int32_t* n_frames_dev, int B,
                            int F, float* mag_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream);

/* Griffin-Lim with optional momentum on magnitudes M = mag_dev [B][cutoff][F].  With
 *   Pc(X) = STFT(ISTFT(X))   this build's transform and inverse: reflect padding at each utterance's
 *                            own end, window sum-square normalisation, trim
 *   Pm(Y) = M . Y / |Y|      a bin with Y = 0 gives (M, 0), as atan2(0, 0) = 0 does
 * the call computes
 *   c_0 = M . exp(i phi0)
 *   for n = 1 .. n_iters:  t_n = Pc(c_{n-1});  y_n = t_n + alpha (t_n - t_{n-1})  (t_0 := t_1);  c_n = Pm(y_n)
 *   out = ISTFT(c_{n_iters})          [B][hop*(F-1)], zeros behind hop*(n_frames[b]-1)
 * 0 <= alpha < 1; alpha = 0 is the reference's loop up to the rounding of its atan2 / sincos
 * (n_iters + 1 inverses; n_iters = 0 is one inverse).  No phase is ever formed inside the loop.
 * n_frames_dev: NULL or [B] frame counts in [2, F] (values outside are clamped to [1, F]).  An
 * utterance with hop*(n_frames[b]-1) <= filter_length/2 samples, which reflect padding cannot
 * serve, takes the framing kernel's clamped reflection (as facppg_stft_transform documents for
 * ragged batches); callers that know the lengths on the host should refuse it.
 * phi0_dev [B][cutoff][F], or NULL: then the phases are drawn on the device, uniform in [-pi, pi)
 * on a 2^-24 grid, by Philox4x32-10 keyed by seeds_dev[b] with the counter (frame, bin) -- a
 * function of (seed, bin, frame) alone, so utterance b of a batch draws what its batch-1 call
 * draws.  THIS IS NOT NumPy's STREAM; facppg_griffin_lim_draw_phase returns the same phases
 * [B][cutoff][F] for inspection.
 * sc_dev: NULL or [B]: sc[b] = || |t_n| - M ||_2 / || M ||_2 at the last iteration over utterance
 * b's own frames, 0 where M = 0.  With n_iters = 0 there is no t_n and |t_0| := 0, so sc is 1
 * (0 where M = 0).  Summed in float64 in a fixed order without atomics: the same bits in any batch.
 * Nothing synchronises the stream. */
size_t facppg_griffin_lim_workspace_bytes(const facppg_stft* h, int B, int F);
int facppg_griffin_lim(facppg_stft* h, const float* mag_dev, const int32_t* n_frames_dev,
                       const float* phi0_dev, const uint64_t* seeds_dev, int n_iters, float alpha,
                       int B, int F, float* out_dev, float* sc_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);
int facppg_griffin_lim_draw_phase(const facppg_stft* h, const uint64_t* seeds_dev, int B, int F,
                                  float* phase_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Tacotron2-style PPG -> mel model (src/common/model.py)
 * ---------------------------------------------------------------------------------- */
/* The model hyper-parameters of create_hparams_stage() (hparams.py:161-241). */
typedef struct facppg_taco_config {
  int32_t n_symbols;                      /* 5816 (full PPG) or 40 (monophone) */
  int32_t symbols_embedding_dim;          /* 600 */
  int32_t encoder_kernel_size;            /* 5 */
  int32_t encoder_n_convolutions;         /* 3 */
  int32_t encoder_embedding_dim;          /* 600 */
  int32_t n_acoustic_feat_dims;           /* 80 */
  int32_t prenet_dim;                     /* 300 */
  int32_t attention_rnn_dim;              /* 300 */
  int32_t decoder_rnn_dim;                /* 300 */
  int32_t attention_dim;                  /* 150 */
  int32_t attention_location_n_filters;   /* 32 */
  int32_t attention_location_kernel_size; /* 31 */
  int32_t attention_window_size;          /* 20; -1 = None (no window) */
  int32_t postnet_embedding_dim;          /* 512 */
  int32_t postnet_kernel_size;            /* 5 */
  int32_t postnet_n_convolutions;         /* 5 */
  float gate_threshold;                   /* 0.5 */
  float bn_eps;                           /* 1e-5 (torch BatchNorm1d default) */
} facppg_taco_config;

typedef struct facppg_taco facppg_taco;

/* fp32 values in the plain weight blob, flattened in THIS order (names: SURVEY.md Appendix B):
 *   encoder.prenet.layers.{0,1}.linear_layer.weight
 *   encoder.convolutions.j: conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var
 *   encoder.lstm: weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, then the same four *_reverse
 *   decoder.prenet.layers.{0,1}.linear_layer.weight
 *   decoder.attention_rnn: weight_ih, weight_hh, bias_ih, bias_hh
 *   decoder.attention_layer: query_layer.W, memory_layer.W, v.W, location_conv.W, location_dense.W
 *   decoder.decoder_rnn: weight_ih, weight_hh, bias_ih, bias_hh
 *   decoder.linear_projection: W, b ; decoder.gate_layer: W, b
 *   postnet.convolutions.j: conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var */
size_t facppg_taco_weight_count(const facppg_taco_config* cfg);
/* Replaces Tacotron2.__init__ + load_state_dict's weight preparation (model.py:539-546). */
int facppg_taco_create(const facppg_taco_config* cfg, const float* weights_dev, size_t n_floats,
                       int device, void* stream, facppg_taco** out);
void facppg_taco_destroy(facppg_taco* h);
size_t facppg_taco_workspace_bytes(const facppg_taco* h, int B, int Tin);
size_t facppg_taco_decode_workspace_bytes(const facppg_taco* h, int B, int max_steps);
size_t facppg_taco_postnet_workspace_bytes(const facppg_taco* h, int B, int T);

/* ---- the decoder's frames while it is still producing them (B = 1, split decoder; facppg_taco_decode_opts.frame_words_dev).
 * The reference's decoder appends a frame per step to a Python list (model.py:516-531) and the postnet runs on the finished
 * spectrogram (model.py:604-605); here a consumer on another stream may start on the frames as they appear.
 * facppg_taco_collect_frames: waits (bounded in wall-clock time, FACPPG_POLL_LIMIT) for frames [frame_a, frame_b) and writes
 *   them channel-major into mel_dev [n_feat][ld].  If the decoder stops short of frame_b (out_length_dev, the decode call's
 *   output, becomes > 0 and <= a wanted frame) the block is VOID: *void_flag_dev = 1 and nothing more is waited for; a block
 *   whose predecessor is void (*prev_flag_dev != 0) is void at once.  Either flag may be NULL.
 * facppg_taco_postnet_range: Postnet.forward + residual (model.py:178-184, 604-605) as a streaming convolution stack.  With f
 *   frames of mel known, layer j (1-based) is final up to f - j*pad columns; the call extends every layer from the f_prev-frame
 *   frontier to the f_new-frame one (its inputs: mel_dev [n_feat][ld], the layers' own earlier columns in the workspace) and
 *   writes the new final columns of mel_post_dev [n_feat][ld_post].  final_T > 0 (= f_new): the utterance has ended there --
 *   every layer runs up to final_T with the convolutions' zero padding behind it.  Every output column is the sum, in the
 *   order, of facppg_taco_postnet's: same bits.  The workspace (facppg_taco_postnet_stream_workspace_bytes(h, max_frames))
 *   carries the layers' columns from call to call.  *skip_dev != 0 (device, may be NULL): the call's launches do nothing. */
int facppg_taco_collect_frames(const facppg_taco* h, const void* words_dev, const int32_t* out_length_dev, int frame_a,
                               int frame_b, float* mel_dev, int ld, int32_t* void_flag_dev, const int32_t* prev_flag_dev,
                               void* stream);
size_t facppg_taco_postnet_stream_workspace_bytes(const facppg_taco* h, int max_frames);
int facppg_taco_postnet_range(const facppg_taco* h, const float* mel_dev, int ld, int f_prev, int f_new, int final_T,
                              float* mel_post_dev, int ld_post, void* workspace_dev, size_t workspace_bytes,
                              int max_frames, const int32_t* skip_dev, void* stream);

/* Replaces Encoder.inference (model.py:237-249) and the memory_layer projection
 * (model.py:334).  ppg_dev [B][n_symbols][Tin]; lengths_dev NULL or [B] valid frame counts
 * (each utterance is encoded exactly as its own batch-1 run); masks_dev NULL (dropout keep-masks
 * are drawn on the device from `seed`) or uint8 {0,1} [2][B][symbols_embedding_dim][Tin]
 * (the prenet's two always-on p=0.5 dropouts, model.py:132-135).
 * Outputs: memory_dev [B][Tin][E] and processed-memory pm_dev [B][attention_dim][Tin] (an opaque
 * intermediate handed to facppg_taco_decode; positions contiguous). */
int facppg_taco_encode(const facppg_taco* h, const float* ppg_dev, const int32_t* lengths_dev,
                       const uint8_t* masks_dev, uint64_t seed, int B, int Tin, float* memory_dev,
                       float* pm_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Replaces Decoder.inference (model.py:489-535) including the attention window mask
 * (utils.py:46-78) and the stop rule (sigmoid(gate) > gate_threshold after appending the frame,
 * else stop at max_steps).  step_limits_dev NULL, or [B] int32: utterance b stops after
 * min(step_limits[b], max_steps) frames at the latest (a padded batch whose utterances each have their
 * own max_decoder_steps, e.g. = their PPG length).  masks_dev NULL or uint8 [max_steps][2][B][prenet_dim].
 * Outputs: mel_dev [B][n_feat][max_steps], gate_dev [B][max_steps], align_dev NULL or
 * [B][max_steps][Tin], out_lengths_dev [B] (= Tout per utterance; columns beyond it untouched).
 * One launch for the whole loop.  The launch shape follows B and the workgroups that may be co-resident (the device's, 240 on
 * an MI355X, or max_workgroups if that is less); facppg_taco_launch_plan answers for any batch.  At 240 and the reference's
 * layer widths: up to 9 utterances run as one attention workgroup each plus 75 register-resident dense-layer workers shared by
 * 1-3 of them (1 while B <= 3, 2 up to 6, 3 up to 9), up to 120 as 2-38 cooperating workgroups each (larger batches in chunks
 * of 120 and a rest), one workgroup per utterance as the fallback when nothing may be co-resident; the first two use
 * hipLaunchCooperativeKernel (the workgroups of an utterance must be co-resident) and every shape returns the same values to
 * fp32 round-off.  FACPPG_DECODER_MODE=split|coop|single forces one (FACPPG_EUNSUPPORTED if the batch does not allow it).
 * opts NULL, or the call's own options and launch report (the handle holds no per-call state):
 *   max_workgroups bounds the workgroups (= CUs: a decoder workgroup holds a CU's whole LDS) the launch may occupy; 0 = no bound
 *     beyond the device's.  No reference counterpart (the reference decodes one utterance at a time on the whole device): it
 *     exists for callers that run the latency-bound decoder of the NEXT batch on a second stream under the MFMA-bound vocoder
 *     of the current one (facppg.pipeline.synthesize_stream) and want it to take few CUs away from the vocoder.  A tighter
 *     bound selects wider weight slices per workgroup, which cuts the LSTM sums differently: results agree with the unbounded
 *     launch to rounding (1e-6 relative on the mel), not bit for bit.
 *   frame_words_dev NULL, or [frame_words_frames * n_feat] 8-byte words ZEROED by the caller: if B = 1, the launch is the split
 *     decoder and max_steps <= frame_words_frames, every mel value of frame t is ALSO stored as the word {value, t + 1} at
 *     words[t * n_feat + row] with an agent-scope store the moment it exists (the plain mel_dev stores are only guaranteed
 *     visible once the launch has ended); otherwise nothing is published.
 *   Filled in by the call: mode = 0 one workgroup per utterance (k_decoder), 1 cooperative slices (k_decoder_coop), 2 split
 *     (k_decoder_split); workgroups = workgroups of that launch (of the last one when a large batch runs in chunks);
 *     streamed = 1 if the frames were published; step = which worker stages a split launch ran: 1 the one-barrier stages,
 *     2 FACPPG_DECODER_STEP=legacy (0 for the other modes). */
typedef struct facppg_taco_decode_opts {
  int32_t max_workgroups;       /* in: 0 = no bound */
  void* frame_words_dev;        /* in: NULL = publish nothing */
  int32_t frame_words_frames;   /* in */
  int32_t mode;                 /* out */
  int32_t workgroups;           /* out */
  int32_t streamed;             /* out */
  int32_t step;                 /* out */
} facppg_taco_decode_opts;
int facppg_taco_decode(const facppg_taco* h, const float* memory_dev, const float* pm_dev,
                       const int32_t* lengths_dev, const int32_t* step_limits_dev,
                       const uint8_t* masks_dev, uint64_t seed, int B,
                       int Tin, int max_steps, float* mel_dev, float* gate_dev, float* align_dev,
                       int32_t* out_lengths_dev, void* workspace_dev, size_t workspace_bytes,
                       facppg_taco_decode_opts* opts, void* stream);
/* What facppg_taco_encode (its BiLSTM recurrence), facppg_taco_decode or facppg_taco_decode_forced would launch for a batch:
 * the host-side decision alone, from the very functions the calls plan with (csrc/facppg_taco_plan.h) -- no handle, no
 * device, no reference counterpart.  coop_limit: the co-resident workgroups of the device, facppg_taco_coop_limit(h) of a
 * handle (240 on an MI355X; 0: no cooperative launch).  steps: max_steps (decode) or T_out (forced).  The environment
 * switches count as in the calls.  Returns what the call would return for the plan: FACPPG_OK, or FACPPG_EUNSUPPORTED with the
 * call's message (facppg_last_error). */
#define FACPPG_TACO_PLAN_ENCODE 0
#define FACPPG_TACO_PLAN_DECODE 1
#define FACPPG_TACO_PLAN_FORCED 2
typedef struct facppg_taco_launch_report {
  int32_t mode;              /* decode, forced: as facppg_taco_decode_opts.mode; encode: 0 */
  int32_t workgroups;        /* of the last launch, as facppg_taco_decode_opts.workgroups */
  int32_t launches;          /* > 1: a batch that runs in chunks of co-resident utterances */
  int32_t step;              /* as facppg_taco_decode_opts.step */
  int32_t nu;                /* split decoder: utterances per worker set, else 0 */
  int32_t first_utts;        /* utterances of the first launch ... */
  int32_t last_utts;         /* ... and of the last */
  int32_t first_u[2];        /* LSTM units per workgroup in the first launch: {attention LSTM, decoder LSTM}; one-workgroup kernel: 0 */
  int32_t last_u[2];         /* ... in the last launch */
  int32_t regw;              /* forced: register-resident attention-LSTM slices */
  int32_t q_res;             /* split decoder: query-weight rows kept in LDS */
  int32_t pause;             /* split decoder: units of 128 cycles a worker pauses before polling */
  int32_t dbg_flags;         /* split decoder: bit 0 FACPPG_DECODER_NO_ROWS */
  int32_t prof;              /* FACPPG_DECODER_PROF is set */
  int32_t lds_bytes;         /* dynamic LDS per workgroup (decode, forced) */
  int32_t streamed_possible; /* decode: frame words would be published if the caller passed enough of them */
  int32_t bilstm_kind;       /* encode: 0 k_bilstm, 1 k_bilstm_coop on 32-unit slices, 2 on 64-unit slices */
  int32_t bilstm_legacy;     /* encode: FACPPG_BILSTM_STEP=legacy applies */
} facppg_taco_launch_report;
int facppg_taco_launch_plan(const facppg_taco_config* cfg, int coop_limit, int what, int B, int Tin, int steps,
                            int max_workgroups, facppg_taco_launch_report* out);
int facppg_taco_coop_limit(const facppg_taco* h);
/* ---- the teacher-forced pass (Tacotron2.forward, model.py:580-595, eval mode): encode_padded -> decode_forced ->
 * facppg_taco_postnet(out_lengths_dev = NULL); the parse_output masking (model.py:566-578) is the caller's.
 *
 * facppg_taco_encode_padded replaces Encoder.forward (model.py:215-235) + the memory_layer projection (model.py:334).  It is
 *   a PADDED-BATCH computation, not B independent runs: the prenet and the conv bank run over all Tin columns of every
 *   utterance (ppg_dev zero-padded by the caller), so the padded frames, non-zero behind the first bias / BatchNorm shift, reach
 *   the last valid frames of the shorter utterances through the convolutions; only the BiLSTM (pack_padded_sequence) and the
 *   memory layer follow the lengths.  memory_dev and pm_dev are zero beyond each length (written by the call).  lengths_dev /
 *   lengths_host: the same [B] values on the device and on the host (both NULL: every utterance has Tin frames); they must be
 *   in [1, Tin] and descending, as pack_padded_sequence demands -- anything else is FACPPG_EINVAL.  Masks, seed, workspace
 *   (facppg_taco_workspace_bytes) and output layouts as facppg_taco_encode.
 * facppg_taco_decode_forced replaces Decoder.forward (model.py:444-487): targets_dev [B][n_feat][T_out] (zero-padded), masks_dev
 *   NULL (drawn from `seed`) or uint8 [2][B][prenet_dim][T_out] -- layer, utterance, channel, INPUT frame (frame 0 is the go
 *   frame; the reference draws T_out + 1 frames and uses the first T_out).  The prenet of all frames, the attention LSTM's input
 *   product of its output, and the projection + gate of all frames are GEMMs around ONE cooperative launch for the recurrence
 *   (attention LSTMCell -> location-sensitive attention with the window mask of utils.py:46-78 -> decoder LSTMCell), exactly
 *   T_out steps for every utterance: no stop rule, shorter utterances go on decoding their zero targets.  Outputs, unmasked:
 *   mel_dev [B][n_feat][T_out], gate_dev [B][T_out], align_dev NULL or [B][T_out][Tin] (fully written).  opts NULL, or
 *   max_workgroups as in facppg_taco_decode; the call reports mode = 1 and the workgroups of its (last) launch.  Batches whose
 *   workgroups do not fit the device together run in chunks of co-resident utterances.  Unlike facppg_taco_decode there is no
 *   one-workgroup shape: the call needs a cooperative launch of at least 4 co-resident workgroups (2 chain + 2 decoder-LSTM;
 *   FACPPG_EUNSUPPORTED if the device or max_workgroups allows fewer).  A chain workgroup holds the decoder's LDS state plus a
 *   64 KiB stash of query-free energies, which bounds Tin lower than inference does: 2157 frames at the reference's
 *   layer widths (inference: 7618); beyond it FACPPG_EUNSUPPORTED.  Up to 2 utterances run with register-resident
 *   attention-LSTM slices (75 chain workgroups per utterance); FACPPG_FORCED_NO_REGW (environment, read per call, any value)
 *   keeps the streamed slices, and FACPPG_DECODER_COOP_U forces one slice width for both roles -- tests and A/B runs, the
 *   results agree to fp32 round-off.  Workspace: facppg_taco_decode_forced_workspace_bytes(h, B, T_out), about 27 KB per
 *   utterance and frame at the reference's widths (9.6 KB of it the frame-indexed exchange words, which the call zeroes):
 *   32 MB at B = 6, T_out = 200, 430 MB at B = 16, T_out = 1000.
 * facppg_taco_draw_dropout_forced: the decoder-prenet masks [2][B][prenet_dim][T_out] keyed by seeds_dev[b] -- for every
 *   (layer, channel, frame) the very bit facppg_taco_draw_dropout gives that utterance. */
int facppg_taco_encode_padded(const facppg_taco* h, const float* ppg_dev, const int32_t* lengths_dev,
                              const int32_t* lengths_host, const uint8_t* masks_dev, uint64_t seed, int B,
                              int Tin, float* memory_dev, float* pm_dev, void* workspace_dev,
                              size_t workspace_bytes, void* stream);
size_t facppg_taco_decode_forced_workspace_bytes(const facppg_taco* h, int B, int T_out);
int facppg_taco_decode_forced(const facppg_taco* h, const float* memory_dev, const float* pm_dev,
                              const int32_t* lengths_dev, const float* targets_dev,
                              const uint8_t* masks_dev, uint64_t seed, int B, int Tin, int T_out,
                              float* mel_dev, float* gate_dev, float* align_dev, void* workspace_dev,
                              size_t workspace_bytes, facppg_taco_decode_opts* opts, void* stream);
int facppg_taco_draw_dropout_forced(const facppg_taco* h, const uint64_t* seeds_dev, int B, int T_out,
                                    uint8_t* dec_masks_dev, void* stream);
/* ---- the backward pass of the teacher-forced pass, eval mode (csrc/facppg_taco_bwd.hip): the recurrences.  The dense
 * products around them (weight gradients, prenets, projection, postnet, encoder convolutions) are the caller's
 * (common/taco_grad.py).  All tensors fp32, contiguous; LSTM gate order i, f, g, o as torch stores it.
 *
 * facppg_taco_decode_forced_state / facppg_taco_encode_state read what the forward calls left in THEIR workspace (pass the
 *   very workspace, before anything else writes to it): ah_dev [B][T_out][attention_rnn_dim] and dh_dev
 *   [B][T_out][decoder_rnn_dim], the hidden states of the two LSTMCells of every frame (model.py:401, 427), and the prenet
 *   masks the call drew from its seed (masks_dev NULL: not wanted; only meaningful if the forward call got masks_dev = NULL).
 *   Saving them costs (attention_rnn_dim + decoder_rnn_dim) * 4 = 2.4 KB per utterance and frame at the reference's widths,
 *   next to the forward's 26.8 KB.
 * facppg_lstm_cell_scan: gates_dev [N][T][4H] holds the gate pre-activations of every frame (a GEMM on the saved hidden
 *   states) and receives the activations; c_dev [N][T][H] the cell states (zero initial state, nn.LSTMCell / nn.LSTM).
 *   lengths_dev NULL or [N]: frames at or beyond an utterance's length are zero (pack_padded_sequence, model.py:226).
 * facppg_lstm_backward: the backward chain of one LSTM, t = T-1 .. 0: dh(t) = dh_seed[n][t] + W_hh^T dgates(t+1), the
 *   cell's pointwise backward, dgates_dev [N][T][4H] (pre-activation gradients; zero beyond the length).  w_hh_dev [4H][H].
 *   Used for decoder_rnn (model.py:427-428; its chain needs nothing of the attention's) and for each direction of the
 *   encoder's BiLSTM (model.py:229-230; the reverse direction on time-reversed utterances).  4H <= 8192.
 *   Workspace: facppg_lstm_backward_workspace_bytes(N, H).
 * facppg_taco_attention_backward: the attention chain of Decoder.decode (model.py:400-424, Attention.forward 100-121,
 *   get_alignment_energies 78-98, LocationLayer 56-60), t = T_out-1 .. 0; see the argument struct.  Masked positions
 *   carry weight 0 and get gradient 0, whatever the window rule was.  Workspace:
 *   facppg_taco_attention_backward_workspace_bytes(config, B, Tin) (0 for a NULL config).
 * One launch per frame and kernel in stream order, no atomics: two runs give the same bits. */
typedef struct {
  const float* w_cat;       /* [4A][E + A]: attention_rnn.weight_ih[:, prenet_dim:] | attention_rnn.weight_hh */
  const float* w_query;     /* [AD][A] query_layer */
  const float* v;           /* [AD] */
  const float* w_loc_dense; /* [AD][NFIL] */
  const float* w_loc_conv;  /* [NFIL][2][KSZ] */
  const float* memory;      /* [B][Tin][E] */
  const float* align;       /* [B][T_out][Tin] attention weights of the forward pass */
  const float* tanh_s;      /* [B][T_out][Tin][AD] tanh(processed_query + processed_attention_weights + processed_memory) */
  const float* act_a;       /* [B][T_out][4A], c_a [B][T_out][A]: facppg_lstm_cell_scan of the attention LSTM */
  const float* c_a;
  const float* base_ctx;    /* [B][T_out][E]: d loss / d ctx(t) through the projection and the decoder LSTM's input */
  const float* base_ah;     /* [B][T_out][A]: d loss / d ah(t) through the decoder LSTM's input */
  float* dgates_a;          /* out [B][T_out][4A] */
  float* dctx;              /* out [B][T_out][E] total adjoint of the attention context */
  float* ds;                /* out [B][T_out][Tin][AD] adjoint of tanh's argument */
  float* de;                /* out [B][T_out][Tin] adjoint of the energies */
} facppg_taco_attention_backward_args;
int facppg_taco_decode_forced_state(const facppg_taco* h, const void* workspace_dev, size_t workspace_bytes, int B,
                                    int T_out, float* ah_dev, float* dh_dev, uint8_t* masks_dev, void* stream);
int facppg_taco_encode_state(const facppg_taco* h, const void* workspace_dev, size_t workspace_bytes, int B, int Tin,
                             uint8_t* masks_dev, void* stream);
int facppg_lstm_cell_scan(float* gates_dev, float* c_dev, const int32_t* lengths_dev, int N, int T, int H, void* stream);
size_t facppg_lstm_backward_workspace_bytes(int N, int H);
int facppg_lstm_backward(const float* w_hh_dev, const float* act_dev, const float* c_dev, const float* dh_seed_dev,
                         const int32_t* lengths_dev, int N, int T, int H, float* dgates_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream);
size_t facppg_taco_attention_backward_workspace_bytes(const facppg_taco_config* config, int B, int Tin);
int facppg_taco_attention_backward(const facppg_taco_config* config, const facppg_taco_attention_backward_args* args,
                                   int B, int Tin, int T_out, void* workspace_dev, size_t workspace_bytes, void* stream);
/* The always-on p=0.5 dropout draws of both prenets (Prenet.forward, model.py:132-135) as PER-UTTERANCE
 * streams keyed by seeds_dev[b] (uint64 [B]): enc_masks_dev uint8 [2][B][symbols_embedding_dim][Tin] and
 * dec_masks_dev uint8 [max_steps][2][B][prenet_dim] in the layouts facppg_taco_encode / _decode accept
 * (either may be NULL).  Bit (layer, channel, frame) of utterance b does not depend on B, Tin or max_steps. */
int facppg_taco_draw_dropout(const facppg_taco* h, const uint64_t* seeds_dev, int B, int Tin,
                             int max_steps, uint8_t* enc_masks_dev, uint8_t* dec_masks_dev,
                             void* stream);
/* Replaces get_mask_from_lengths_window_and_time_step(memory_lengths, attention_window_size,
 * time_step) (src/common/utils.py:46-78), the integer part of the attention: mask_dev [B][Tmax]
 * uint8, 0 = keep for index in [min(max(0, t-W), len-1), min(t+W, len-1)], 1 = masked (so the last
 * frame stays unmasked once t-W has passed it, utils.py:65-69); window < 0 = no window.  lengths_dev [B]
 * int32, each in [1, Tmax].  Uses the very range function the decoder kernels evaluate the attention on. */
int facppg_attention_window_mask(const int32_t* lengths_dev, int B, int Tmax, int window,
                                 int time_step, uint8_t* mask_dev, void* stream);
/* Replaces Postnet.forward + the residual add (model.py:178-184, 604-605):
 * mel_dev [B][n_feat][ld] (first T columns used) -> mel_post_dev, same layout.  out_lengths_dev [B]: utterance b is
 * convolved as its own out_lengths[b]-column run (columns beyond stay untouched); NULL: the padded-batch form of
 * Tacotron2.forward (model.py:591-592) -- all T columns of every utterance, whatever follows its last frame included. */
int facppg_taco_postnet(const facppg_taco* h, const float* mel_dev, const int32_t* out_lengths_dev,
                        int B, int T, int ld, float* mel_post_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * PPG front-end, the part that needs no acoustic-model blob (src/ppg/compute_ppg.py, src/common/feat.py; the Kaldi
 * feature code behind pykaldi): the nnet3 input features and the senone -> monophone reduction.
 * ---------------------------------------------------------------------------------- */
typedef struct facppg_mfcc facppg_mfcc;
/* Replaces kaldi.feat.mfcc.Mfcc(opts) (feat.py:74-100).  The caller folds Kaldi's per-frame linear steps (DC removal,
 * pre-emphasis, window, zero padding, DFT) into basis_dev [2*nbins][frame_length] (real rows, then imaginary rows) and
 * supplies the mel bank mel_dev [n_mel][nbins] and the liftered DCT dct_dev [n_ceps][n_mel].  Synchronises `stream`. */
int facppg_mfcc_create(int frame_length, int frame_shift, int nbins, const float* basis_dev,
                       const float* mel_dev, int n_mel, const float* dct_dev, int n_ceps, int device,
                       void* stream, facppg_mfcc** out);
void facppg_mfcc_destroy(facppg_mfcc* h);
int facppg_mfcc_num_frames(const facppg_mfcc* h, int n_samples);   /* (n + shift/2) / shift: snip_edges = false */
size_t facppg_mfcc_workspace_bytes(const facppg_mfcc* h, int n_samples);
/* Replaces Mfcc.compute_features (feat.py:98): wav_dev [n_samples] (int16-range floats) -> mfcc_dev [T][n_ceps];
 * frames are cut with Kaldi's snip_edges=false reflection; dither is not applied (deterministic); use_energy != 0
 * puts the log frame energy in coefficient 0. */
int facppg_mfcc_compute(facppg_mfcc* h, const float* wav_dev, int n_samples, int use_energy,
                        float* mfcc_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Replaces Kaldi's DownsampleWaveForm / LinearResample (what frame_opts.allow_downsample = True triggers for inputs above
 * 16 kHz, feat.py:85-87): windowed-sinc low-pass at 0.99 * min(fs) / 2, 6 zero crossings.  out_dev holds
 * facppg_resample_num_samples(n_in, fs_in, fs_out) samples. */
int facppg_resample_num_samples(int n_in, int fs_in, int fs_out);
int facppg_resample(const float* wav_dev, int n_in, int fs_in, int fs_out, float* out_dev, void* stream);
/* Replaces apply_cepstral_mean_norm (feat.py:103-118), kaldi.feat.functions.splice_frames(left, right) (edge frames
 * replicated) and apply_feat_transform (feat.py:121-156) in one pass: feats_dev [T][D] -> out_dev [T][M] with
 * transform_dev [M][cols], cols = (left+right+1)*D or one more (affine offset column); transform_dev NULL -> the spliced
 * (and, with do_cmn, mean-normalised) features [T][(left+right+1)*D].  mean_ws_dev: D floats of scratch. */
int facppg_cmn_splice_transform(const float* feats_dev, int T, int D, int do_cmn, int left, int right,
                                const float* transform_dev, int M, int cols, float* out_dev,
                                float* mean_ws_dev, void* stream);
/* The two front-end steps above for a BATCH of utterances laid end to end (the per-utterance loops of
 * PPGMelLoader.__init__ / get_ppg, data_utils.py:55-59, 204-209, over compute_feat_for_nnet_internal, compute_ppg.py:97-134):
 * wav_dev holds the B waveforms one after the other (all at the model's rate: facppg_resample stays per utterance),
 * sample_offsets[B + 1] and frame_offsets[B + 1] (off[0] = 0, increasing; T_b = facppg_mfcc_num_frames of utterance b's
 * sample count) both on the device and on the host.  Per frame the arithmetic is that of the single-utterance entry
 * points in the same order, so an utterance gets the same bits in any batch: frames reflect at the utterance's own ends
 * (Kaldi snip_edges = false), the cepstral mean is taken over its own frames, the splice clamps to its own first / last
 * frame.  facppg_mfcc_compute_batch (replaces Mfcc.compute_features, feat.py:98, per utterance): -> mfcc_dev
 * [sum T][n_ceps].  A sample count the single call refuses is refused with the same message. */
size_t facppg_mfcc_batch_workspace_bytes(const facppg_mfcc* h, int total_frames);
int facppg_mfcc_compute_batch(facppg_mfcc* h, const float* wav_dev, const int32_t* sample_offsets_dev,
                              const int32_t* sample_offsets_host, const int32_t* frame_offsets_dev,
                              const int32_t* frame_offsets_host, int B, int use_energy, float* mfcc_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);
/* facppg_cmn_splice_transform_batch (replaces apply_cepstral_mean_norm, splice_frames and apply_feat_transform,
 * feat.py:103-156, per utterance): feats_dev [sum T][D] -> out_dev [sum T][M]; mean_ws_dev: B * D floats of scratch. */
int facppg_cmn_splice_transform_batch(const float* feats_dev, const int32_t* frame_offsets_dev,
                                      const int32_t* frame_offsets_host, int B, int D, int do_cmn, int left,
                                      int right, const float* transform_dev, int M, int cols, float* out_dev,
                                      float* mean_ws_dev, void* stream);
/* Replaces reduce_ppg_dim (compute_ppg.py:73-94): out[t][m] = sum_k ppg[t][k] * transform_t[k][m]
 * (transform_t = the densified pdf -> monophone matrix, TRANSPOSED: [K][M], M <= 64). */
int facppg_reduce_ppg(const float* ppg_dev, const float* transform_t_dev, int T, int K, int M,
                      float* out_dev, void* stream);

/* Replaces torch.optim.Adam(model.parameters(), lr).step() of the training loop (src/script/train_waveglow.py:83,134) for
 * every parameter in ONE streaming launch.  table_dev: n_tensors entries {float* param, const float* grad, float* exp_avg,
 * float* exp_avg_sq, int64 numel} (40 bytes each); chunks_dev: n_chunks pairs {tensor index, chunk index} covering every
 * tensor in chunks of facppg_adam_chunk_elems() elements; step_dev: the step count (a float, as torch's fused Adam keeps
 * it), incremented on the device BEFORE the update so a captured launch advances it at every replay.  Arithmetic of
 * torch._fused_adam_ (amsgrad off, maximize off, L2-style weight_decay). */
int facppg_adam_chunk_elems(void);
int facppg_adam_step(const void* table_dev, int n_tensors, const int32_t* chunks_dev, int n_chunks, float* step_dev,
                     float lr, double beta1, double beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------
 * nnet3 TDNN acoustic model: feature frames -> senone posteriors (the "full PPG")
 * (src/ppg/compute_ppg.py:42-70 compute_full_ppg = Kaldi nnet3::DecodableNnetSimple through PyKaldi;
 *  src/common/decode.py:23-38 read_nnet3_model).  The model file (data/am/final.raw) is not shipped by the reference and
 * no Kaldi runtime exists in this image: PARITY UNPINNED at the Kaldi boundary (see common/nnet3.py, oracle/nnet3.py).
 * ---------------------------------------------------------------------------------- */
typedef struct facppg_tdnn facppg_tdnn;

/* One fused layer: y[:, t] = act(W . [x[:, t + first + j*dil], j = 0..taps-1] + b), optionally followed by Kaldi's
 * NormalizeComponent (renorm_target_rms > 0).  Test-mode BatchNorm / FixedAffine layers are folded into W, b by the
 * host (common.nnet3.plan_layers, as nnet3::CollapseModel does at compute_ppg.py:57).  first <= 0 <= first + (taps-1)*dil. */
typedef struct facppg_tdnn_layer {
  int32_t out_dim, in_dim, taps, dil, first, relu;
  float renorm_target_rms;
} facppg_tdnn_layer;

/* Values in the weight blob: per layer W [out_dim][taps*in_dim] (tap-major = Kaldi's Append order) then b [out_dim]. */
size_t facppg_tdnn_weight_count(const facppg_tdnn_layer* layers, int n_layers);
/* final_op: 0 = the last layer's output, 1 = softmax (posteriors), 2 = log-softmax.  weights_dev may be freed on return. */
int facppg_tdnn_create(const facppg_tdnn_layer* layers, int n_layers, int final_op, const float* weights_dev,
                       size_t n_weights, int device, void* stream, facppg_tdnn** out);
void facppg_tdnn_destroy(facppg_tdnn* h);
/* Frames of input context the network needs before / after a frame (nnet3::ComputeSimpleNnetContext). */
int facppg_tdnn_context(const facppg_tdnn* h, int* left, int* right);
size_t facppg_tdnn_workspace_bytes(const facppg_tdnn* h, int T);
/* feats_dev [T][in_dim] row-major (what compute_feat_for_nnet returns) -> out_dev [T][out_dim] row-major; frames beyond
 * the utterance's ends are the first / last frame repeated (DecodableNnetSimple's edge handling). */
int facppg_tdnn_forward(facppg_tdnn* h, const float* feats_dev, int T, float* out_dev, void* workspace_dev,
                        size_t ws_bytes, void* stream);

/* compute_full_ppg (compute_ppg.py:42-70) for a BATCH of utterances in one pass: feats_dev holds the utterances'
 * [T_b][in_dim] rows laid end to end, offsets[B + 1] their frame offsets (off[0] = 0, increasing), on the device and on
 * the host; out_dev [sum T][out_dim].  The utterances share one column space (each segment [left | T_b | right] with its
 * own edge frames repeated, starting on a 4-column boundary), every layer is ONE GEMM over all of it, and no valid frame
 * depends on a column of another utterance.  Softmax and renorm are the single call's arithmetic per frame; through the
 * GEMM layers the sums are k_gemm's, whose order does not depend on the column count. */
size_t facppg_tdnn_batch_workspace_bytes(const facppg_tdnn* h, const int32_t* offsets_host, int B);
int facppg_tdnn_forward_batch(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                              const int32_t* offsets_host, int B, float* out_dev, void* workspace_dev,
                              size_t ws_bytes, void* stream);
/* The same, followed by reduce_ppg_dim (compute_ppg.py:73-94) in the output kernel: out_dev [sum T][M] =
 * softmax(logits) . transform_t ([out_dim][M], M <= 64, as facppg_reduce_ppg takes it) -- the monophone PPGs of
 * compute_monophone_ppg (compute_ppg.py:161-181) without the [sum T][out_dim] posteriors in memory.  The model's
 * output must be a softmax (final_op 1), else FACPPG_EUNSUPPORTED.  Same workspace. */
int facppg_tdnn_forward_batch_reduced(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                                      const int32_t* offsets_host, int B, const float* transform_t_dev, int M,
                                      float* out_dev, void* workspace_dev, size_t ws_bytes, void* stream);
/* The posteriors in the layout the encoder reads (facppg_taco_encode's ppg_dev [B][n_symbols][Tin]): out_dev [B][K][Tmax],
 * out[b][k][t] = posterior k of frame t of utterance b, exactly 0.0f for T_b <= t < Tmax; the call writes every element.
 * transform_t_dev NULL: K = out_dim, the senone posteriors of compute_full_ppg (compute_ppg.py:42-70) -- the softmax runs
 * across the channel rows of the logits' own channel-major layout, in a fixed order, and a frame's values depend on its own
 * logit column alone (not on B, Tmax, or its neighbours).  transform_t_dev [out_dim][M], M <= 64: K = M, the monophone PPGs
 * of reduce_ppg_dim (compute_ppg.py:73-94), bit for bit facppg_tdnn_forward_batch_reduced's values.  The layers up to the
 * logits are facppg_tdnn_forward_batch's.  Workspace: facppg_tdnn_batch_workspace_bytes.  Refused before any launch:
 * B < 1, a NULL pointer, M out of range with a transform, Tmax < max T_b (FACPPG_EINVAL); a model whose output is not a
 * softmax (FACPPG_EUNSUPPORTED); a short workspace (FACPPG_EWORKSPACE). */
int facppg_tdnn_forward_batch_padded(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                                     const int32_t* offsets_host, int B, const float* transform_t_dev, int M, int Tmax,
                                     float* out_dev, void* workspace_dev, size_t ws_bytes, void* stream);
/* The same with batch_stride floats from one utterance's rows to the next (>= K * Tmax, else FACPPG_EINVAL):
 * out[b * batch_stride + k * Tmax + t].  The K rows of every utterance are written in full and nothing behind them is touched,
 * so the posteriors go straight into rows [:K] of a wider batch -- [B][K + 3][Tmax] with the log-F0 rows of
 * facppg_lf0_rows_padded behind them -- without a copy.  facppg_tdnn_forward_batch_padded is this call with K * Tmax. */
int facppg_tdnn_forward_batch_padded_strided(facppg_tdnn* h, const float* feats_dev, const int32_t* offsets_dev,
                                             const int32_t* offsets_host, int B, const float* transform_t_dev, int M,
                                             int Tmax, size_t batch_stride, float* out_dev, void* workspace_dev,
                                             size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Long recordings: cut at the pauses, convert the pieces as padded batches, join the audio
 * (facppg.pipeline.synthesize_long).  The reference has NO counterpart: Tacotron2.inference decodes at most
 * max_decoder_steps frames and a longer teacher recording is cut off with "Warning! Reached max decoder steps"
 * (src/common/model.py:527, src/script/generate_synthesis.py:90-93).  PPGs are fp32 in the layout
 * facppg_tdnn_forward_batch_padded writes and facppg_taco_encode reads: [B][K][Tmax], frames contiguous.  Tables come as a
 * device copy (read by the kernel) next to a host copy (validated before the launch); every refusal is FACPPG_EINVAL
 * (more than 65535 recordings / segments in one call: FACPPG_EUNSUPPORTED) and launches nothing.
 * ---------------------------------------------------------------------------------- */
/* flags_dev uint8 [B][Tmax]: flags[b][t] = t < lengths[b] && x[b][rows[0]][t] + x[b][rows[1]][t] + ... > threshold -- one fp32
 * accumulator, the rows in the order given, additions only (a NumPy float32 sum in that order has the same bits).  Every
 * element of flags is written.  Refused: n_rows < 1, a row outside [0, K), a threshold outside (0, n_rows). */
int facppg_ppg_pause_flags(const float* x_dev, const int32_t* lengths_dev, int B, int K, int Tmax, const int32_t* rows_dev,
                           const int32_t* rows_host, int n_rows, float threshold, uint8_t* flags_dev, void* stream);
/* table int32 [S][3] of (recording b, start, frames); y_dev [S][K][Lmax]: y[s][k][l] = l < frames_s ? x[b_s][k][start_s + l] : 0.
 * Every element of y is written (zeros behind each segment, as facppg_tdnn_forward_batch_padded pads).  Starts are arbitrary;
 * the rows of y are written 16 bytes at a time when Lmax % 4 == 0.  Refused: b outside [0, B), start < 0, frames outside
 * [1, Lmax], start + frames > Tmax. */
int facppg_ppg_gather_segments(const float* x_dev, int B, int K, int Tmax, const int32_t* table_dev, const int32_t* table_host,
                               int S, int Lmax, float* y_dev, void* stream);
/* audio_dev [S][Nmax], n[s] <= Nmax valid samples each -> out_dev [sum n]: the segments laid end to end with a linear fade on
 * both sides of every INTERIOR seam: gain (2 i + 1) / (2 f_s) over the first f_s samples of segments s > 0, mirrored over the
 * last f_s of segments s < S - 1, f_s = min(fade, n[s] / 2) rounded down to a power of two (or 0).  fade: 0 or a power of two
 * up to 4096 (anything else is refused) -- every gain is then exact in fp32.  S = 1 or fade = 0: a copy. */
int facppg_join_segments(const float* audio_dev, int Nmax, const int32_t* n_dev, const int32_t* n_host, int S, int fade,
                         float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Round-trip scoring: dynamic time warping of two padded PPG batches (facppg.score.ppg_dtw / roundtrip: the teacher's PPG
 * against the PPG of the converted audio).  The reference has NO counterpart: generate_synthesis.py:86-98 writes the wav and
 * never compares it with anything.  a_dev [B][D][Ta_max] and b_dev [B][D][Tb_max], fp32, frames contiguous -- the layout
 * facppg_tdnn_forward_batch_padded writes; pair p is a[p][:][0 .. la[p]) against b[p][:][0 .. lb[p]), and nothing behind a
 * length is read (it may hold NaN).  Per pair, with Ta = la[p], Tb = lb[p]:
 *   per frame      ra[k][i] = sqrt(max(a[k][i], 0)), ca[i] = arg max_k a[k][i] (the lowest k on a tie); rb, cb likewise
 *   local distance d(i,j) = max(0, 1 - sum_k ra[k][i] rb[k][j]): the squared Hellinger distance of two posteriors; the sum is
 *                  one fp32 fma chain from 0 with k increasing
 *   band           m = max(Ta - 1, Tb - 1, 1); (i,j) is admissible iff band == 0 or |i (Tb - 1) - j (Ta - 1)| <= band m, in
 *                  64-bit integers.  Both corners always are; from band 2 on an admissible path always exists
 *   recurrence     C(0,0) = d(0,0); else C(i,j) = d(i,j) + min over the admissible predecessors (i-1,j-1), (i-1,j), (i,j-1),
 *                  tried in that order with a strict <: a tie keeps the earlier one.  fp32 additions
 *   carried along the chosen predecessor: N(i,j) = N(pred) + 1, N(0,0) = 1; M(i,j) = M(pred) + [ca[i] == cb[j]]
 *   outputs        cost_dev[p] = C(Ta-1, Tb-1), steps_dev[p] = N(Ta-1, Tb-1), agree_dev[p] = M(Ta-1, Tb-1)   ([B] each)
 * so there is no back-pointer matrix and no backtrace.  Lengths come as a device copy (read by the kernels) next to a host
 * copy (validated before the first launch).  Refused, and nothing is launched: a NULL pointer, B, D, Ta_max or Tb_max < 1, a
 * length outside [1, T*_max], band 1 or band < 0 (FACPPG_EINVAL); D > 256 -- senone posteriors: reduce them to monophone
 * classes first --, B > 65535 (FACPPG_EUNSUPPORTED); a workspace smaller than facppg_ppg_dtw_workspace_bytes, which holds the
 * square roots and B (Ta_max + Tb_max - 1) Ta_max distances (FACPPG_EWORKSPACE).  Launches: two frame passes, one tiled
 * distance kernel over all pairs, and one sweep (one workgroup per pair) per 1024 rows of the longest a; all on ``stream``,
 * none cooperative, none waits on memory. */
size_t facppg_ppg_dtw_workspace_bytes(int B, int D, int Ta_max, int Tb_max, int band);
int facppg_ppg_dtw(const float* a_dev, const int32_t* la_dev, const int32_t* la_host, int Ta_max,
                   const float* b_dev, const int32_t* lb_dev, const int32_t* lb_host, int Tb_max,
                   int B, int D, int band,
                   float* cost_dev, int32_t* steps_dev, int32_t* agree_dev,
                   void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Free-running validation (facppg.score.mel_dtw / attention_path, script.train_ppg2mel.validate_free_running): the decoder's
 * free-running mels against the target mels by a mel-cepstral DTW, and a summary of what its attention did.  The reference has
 * NO counterpart: its validate() (train_ppg2mel.py:152-177) is teacher-forced only.  THE SCORE IS THIS BUILD'S OWN DEFINITION --
 * a DTW over an orthonormal DCT of natural-log mels, c0 left out -- as the F0 track below is; its values compare within this
 * build only, not with MCD figures computed from WORLD or SPTK cepstra.
 *
 * facppg_mel_dtw: a_dev [B][M][Ta_max] and b_dev [B][M][Tb_max], fp32 log-mels, frames contiguous (the layout of
 * Tacotron2.inference's mel_post and of the padded targets); pair p is a[p][:][0 .. la[p]) against b[p][:][0 .. lb[p]), and
 * nothing behind a length is read (it may hold NaN).  basis_dev [K][M] fp32, any matrix (facppg.score.cepstral_basis: rows 1 .. K
 * of the orthonormal DCT-II).  Per pair, with Ta = la[p], Tb = lb[p]:
 *   projection     ca[k][i] = sum_m basis[k][m] a[m][i]: one fp32 fma chain from 0 with m increasing,
 *                  acc = fma(basis[k][m], a[m][i], acc); cb likewise
 *   local distance d(i,j) = sqrtf(s), s one fp32 fma chain from 0 with k increasing: diff = ca[k][i] - cb[k][j] (an fp32
 *                  subtraction), s = fma(diff, diff, s).  DIRECT differences on purpose: |a|^2 + |b|^2 - 2 a.b loses about
 *                  eps |a|^2 in s when two frames are close, which is the case a validation score is about
 *   band, recurrence, tie order, N(i,j)   exactly facppg_ppg_dtw's above: m = max(Ta - 1, Tb - 1, 1), (i,j) admissible iff
 *                  band == 0 or |i (Tb - 1) - j (Ta - 1)| <= band m in 64-bit integers; C(0,0) = d(0,0), else C(i,j) = d(i,j) +
 *                  min over the admissible predecessors (i-1,j-1), (i-1,j), (i,j-1) tried in that order with a strict <; fp32
 *                  additions; N(i,j) = N(pred) + 1, N(0,0) = 1
 *   outputs        cost_dev[p] = C(Ta-1, Tb-1), steps_dev[p] = N(Ta-1, Tb-1)   ([B] each); no backtrace
 * facppg.score.mel_dtw reports mcd = (10 sqrt(2) / ln 10) cost / steps in dB (the mels are NATURAL-log mels, what
 * dynamic_range_compression produces).  Lengths come as a device copy (read by the kernels) next to a host copy (validated before
 * the first launch).  Refused, and nothing is launched: a NULL pointer, B, M, K, Ta_max or Tb_max < 1, a length outside
 * [1, T*_max], band 1 or band < 0 (FACPPG_EINVAL); M > 256, K > 64, B > 65535 (FACPPG_EUNSUPPORTED); a workspace smaller than
 * facppg_mel_dtw_workspace_bytes, which holds the cepstra and B (Ta_max + Tb_max - 1) Ta_max distances (FACPPG_EWORKSPACE).
 * Launches: two projections, one tiled distance kernel over all pairs, and facppg_ppg_dtw's own sweep (one workgroup per pair)
 * per 1024 rows of the longest a; all on ``stream``, none cooperative, none waits on memory, no atomics.
 *
 * facppg_attention_path: align_dev [B][Tout_max][Tin_max] fp32, finite -- Tacotron2.inference's alignments; utterance p has
 * T = tout[p] decoder steps over L = tin[p] input frames, and nothing behind T or L is read.  With pos[t] = arg max_{j < L}
 * A[p][t][j] (the lowest j on a tie) and w[t] that maximum, stats_dev[p] holds six integers:
 *   0 first          pos[0]
 *   1 last           pos[T-1]
 *   2 back           #{t >= 1 : pos[t] < pos[t-1]}
 *   3 max_jump       max(0, max_{t >= 1} pos[t] - pos[t-1])
 *   4 longest_stall  the longest run of consecutive equal pos (>= 1)
 *   5 visited        the number of distinct values among pos[0 .. T)
 * and focus_dev[p] = the mean of w[t], summed in float64 and rounded to fp32 once.  Refused, and nothing is launched: a NULL
 * pointer, B, Tout_max or Tin_max < 1, a length outside [1, T*_max] (FACPPG_EINVAL); B > 65535 (FACPPG_EUNSUPPORTED); a workspace
 * smaller than facppg_attention_path_workspace_bytes (FACPPG_EWORKSPACE).  Two launches on ``stream``, none cooperative, no
 * atomics. */
size_t facppg_mel_dtw_workspace_bytes(int B, int M, int K, int Ta_max, int Tb_max, int band);
int facppg_mel_dtw(const float* a_dev, const int32_t* la_dev, const int32_t* la_host, int Ta_max,
                   const float* b_dev, const int32_t* lb_dev, const int32_t* lb_host, int Tb_max,
                   int B, int M, const float* basis_dev, int K, int band,
                   float* cost_dev, int32_t* steps_dev, void* ws_dev, size_t ws_bytes, void* stream);
size_t facppg_attention_path_workspace_bytes(int B, int Tout_max, int Tin_max);
int facppg_attention_path(const float* align_dev, const int32_t* tout_dev, const int32_t* tout_host, int Tout_max,
                          const int32_t* tin_dev, const int32_t* tin_host, int Tin_max, int B,
                          int32_t* stats_dev /* [B][6] */, float* focus_dev /* [B] */,
                          void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * F0 track on the device, and the reference's log-F0 input columns (hparams.is_append_f0: append_ppg,
 * src/common/data_utils.py:142-160, makes n_symbols = K + 3).  The reference takes its F0 from WORLD through pyworld
 * (utterance.py:33-38: harvest, 48-400 Hz, 5 ms shift), which does not exist in this image and cannot be reproduced here:
 * PARITY UNPINNED at the WORLD boundary.  The tracker is therefore DEFINED here -- a normalised cross-correlation and one
 * Viterbi pass over its peaks -- and the kernels are held to a float64 / float32 restatement of this text
 * (tests/f0_helpers.py).  A user who has WORLD tracks brings them as files (common.data_utils.get_f0_batch).
 *
 * Input: the front end's own samples, int16-range floats at the model's rate (after common.feat's resampling), the B
 * utterances laid end to end with sample_offsets[B + 1], exactly as facppg_mfcc_compute_batch takes them.  Samples outside
 * an utterance's own [0, n) read as 0; an utterance never sees a neighbour's samples.
 * Frames are the PPG's frames: T_b = (n_b + S / 2) / S (facppg_mfcc_num_frames), frame t centred at t S + S / 2.  The
 * reference's WORLD shift is 5 ms and append_ppg just truncates to the shorter of the two tracks; here ONE F0 FRAME MEETS ONE
 * PPG FRAME.  With S = frame_shift, W = window, L = lag_max - lag_min + 1 candidate lags:
 *   tables_dev float [2][L], computed by the host: wl[l] = float32(1 - 0.3 l / lag_max), g[l] = float32(log2 l), l = lag_min ..
 *                  lag_max -- no transcendental function runs on the device inside the tracker
 *   NCCF           a = t S + S / 2 - (W + lag_max + 1) / 2 (integer division); for every lag l in lag_min - 1 .. lag_max + 1
 *                  (L + 2 columns): phi(t,l) = sum_{j<W} x[a+j] x[a+j+l] / sqrt(E(a) E(a+l) + (W ballast^2)^2),
 *                  E(p) = sum_{j<W} x[p+j]^2; fp32 sums in an order that depends on W alone (a frame has the same bits in any
 *                  batch).  nccf_dev [sum T][L + 2], row-major
 *   track          one Viterbi pass per utterance over its own rows.  State 0 is unvoiced, state s = 1 .. L is lag
 *                  lag_min + s - 1.  Lag l is a PEAK at t iff phi(t,l) >= phi(t,l-1) and phi(t,l) > phi(t,l+1).
 *                  voiced local cost   dv(t,l) = 1 - phi(t,l) wl[l] at a peak, +inf elsewhere
 *                  unvoiced local cost du(t) = max_l phi(t,l) over lag_min .. lag_max only
 *                  start               C(0,0) = du(0), C(0,l) = dv(0,l)
 *                  t >= 1              predecessors tried with s' increasing and a strict <:
 *                                      into unvoiced: C(t-1,0), then C(t-1,s') + voicing_cost
 *                                      into lag l:    C(t-1,0) + voicing_cost, then C(t-1,s') + freq_weight |g[l] - g[l']|
 *                                      and the local cost is added to the winner
 *                  all fp32, every multiply and add rounded on its own.  The end state is the first minimum of C(T-1, .);
 *                  back-pointers uint16 [T][L + 1] live in the workspace, then a backtrace
 *   outputs        per frame lag_dev int32 (0 = unvoiced) and f0_dev float: 0 when unvoiced; voiced, with p = phi(l-1), q = phi(l),
 *                  r = phi(l+1): den = (p - (q + q)) + r, delta = den < 0 ? 0.5 (p - r) / den : 0, f0 = sample_rate / (l + delta),
 *                  fp32 in that order (the two guard columns exist for this)
 * facppg_f0_nccf_batch writes the matrix, facppg_f0_track_batch reads one (the caller's own, if it likes), facppg_f0_batch
 * runs the two back to back with the matrix in the workspace.  Offsets come as a device copy (read by the kernels) next to a
 * host copy (validated before the first launch).  Refused, and nothing is launched: a NULL pointer, B < 1, offsets that do
 * not start at 0 or do not increase, a sample count with no frame, frame offsets that are not the sample counts' T_b,
 * lag_min < 2, lag_max >= 2048 or < lag_min, window < 1, a negative cost (FACPPG_EINVAL); more than 1023 candidate lags, a
 * frame span beyond what a workgroup stages, B > 65535 (FACPPG_EUNSUPPORTED); a workspace smaller than
 * facppg_f0_workspace_bytes(cfg, sum T) (FACPPG_EWORKSPACE; 0 with facppg_last_error set for a refused configuration).
 *
 * facppg_lf0_rows_padded: f0_dev [sum T] (Hz, 0 = unvoiced) -> the three rows append_ppg appends, in the padded batch:
 *   x0 = logf(f0 + 2.220446e-16f)  (the reference's np.finfo(float).eps: unvoiced frames come out near -36.04, as they do there)
 *   x1 = 0.5 (x0[t+1] - x0[t-1]),  x2 = 0.25 x0[t-2] - 0.5 x0[t] + 0.25 x0[t+2]      (DELTA_WIN, ACC_WIN)
 *   indices clamped to the utterance's own first and last frame (compute_dynamic_vector's edge replication)
 * out_dev[b * batch_stride + r * Tmax + t], r = 0 .. 2 -- with out_dev = x + K * Tmax and batch_stride = (K + 3) * Tmax these are
 * the rows [K:] of the [B][K + 3][Tmax] batch whose rows [:K] facppg_tdnn_forward_batch_padded_strided writes.  Exactly 0.0f
 * for T_b <= t < Tmax; every element of the three rows is written.  Refused: a NULL pointer, B < 1, bad offsets, Tmax below the
 * longest utterance, batch_stride < 3 Tmax. */
typedef struct facppg_f0_config {
  int32_t sample_rate;   /* 16000 */
  int32_t frame_shift;   /* 160 */
  int32_t window;        /* 320 */
  int32_t lag_min;       /* 40  = floor(16000 / 400) */
  int32_t lag_max;       /* 334 = ceil(16000 / 48): L = 295 */
  float ballast;         /* 50 */
  float voicing_cost;    /* 0.2 */
  float freq_weight;     /* 2.0 */
} facppg_f0_config;
size_t facppg_f0_workspace_bytes(const facppg_f0_config* cfg, int total_frames);
int facppg_f0_nccf_batch(const facppg_f0_config* cfg, const float* wav_dev, const int32_t* sample_offsets_dev,
                         const int32_t* sample_offsets_host, const int32_t* frame_offsets_dev,
                         const int32_t* frame_offsets_host, int B, float* nccf_dev, void* stream);
int facppg_f0_track_batch(const facppg_f0_config* cfg, const float* nccf_dev, const int32_t* frame_offsets_dev,
                          const int32_t* frame_offsets_host, int B, const float* tables_dev, int32_t* lag_dev,
                          float* f0_dev, void* ws_dev, size_t ws_bytes, void* stream);
int facppg_f0_batch(const facppg_f0_config* cfg, const float* wav_dev, const int32_t* sample_offsets_dev,
                    const int32_t* sample_offsets_host, const int32_t* frame_offsets_dev,
                    const int32_t* frame_offsets_host, int B, const float* tables_dev, int32_t* lag_dev, float* f0_dev,
                    void* ws_dev, size_t ws_bytes, void* stream);
int facppg_lf0_rows_padded(const float* f0_dev, const int32_t* frame_offsets_dev, const int32_t* frame_offsets_host,
                           int B, int Tmax, size_t batch_stride, float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Per-phone report of a conversion: phone-loop decode and forced alignment of monophone PPGs (facppg.align: decode_phones,
 * force_align, phone_report; score.roundtrip(phones=True)).  The reference has NO counterpart: its DataUtterance carries phone
 * tiers and its align.py reads and writes TextGrids that an EXTERNAL aligner produced from a transcript; the wav -> wav path
 * has neither.  Here the teacher's own phone sequence is decoded from its PPG and the conversion's PPG is aligned to it.  The
 * two dynamic programs are therefore DEFINED here and the kernels are held to a float64 / float32 restatement of this text
 * (tests/align_helpers.py).  All arithmetic is fp32 and every add is rounded on its own.
 *
 * Input: x_dev [B][D][Tmax], fp32, frames contiguous -- the layout facppg_tdnn_forward_batch_padded writes.  The lengths are
 * the differences T_b of frame_offsets[B + 1], which come as a device copy (read by the kernels) next to a host copy
 * (validated before the first launch); nothing behind a length is read (it may hold NaN).  Ragged per-frame arrays are laid
 * end to end by frame_offsets, as the F0 entry points lay theirs; ragged per-state arrays by seq_offsets[B + 1].
 *
 * facppg_ppg_emissions -- one kernel, frame-major outputs, so that both DPs read a frame's row:
 *   em_dev float [sum T][D]   em[t][k] = -logf(max(x[k][t], floor))      (finite by the floor, >= 0 for posteriors)
 *   eb_dev float [sum T]      eb[t] = min_k em[t][k]
 *   top_dev int32 [sum T]     top[t] = arg max_k x[k][t], the lowest k on a tie
 * The transpose from channel-major to frame-major goes through an LDS tile: the reads of x and the writes of em are both
 * coalesced.
 *
 * facppg_ppg_decode_phones -- the phone loop over the emissions, per utterance, T = T_b:
 *   start          C(0,k) = em[0][k]
 *   t >= 1         m = the first minimum of C(t-1,.), at class j;
 *                  C(t,k) = em[t][k] + (m + switch_cost < C(t-1,k) ? m + switch_cost : C(t-1,k))      (strict <: a tie stays)
 *                  back-pointer: k for a stay, j for a switch (one byte, in the workspace)
 *   end            the first minimum of C(T-1,.), then a backtrace
 *   outputs        labels_dev int32 [sum T], cost_dev float [B]
 * switch_cost is a parameter of the definition that the user tunes (the price of one more phone), not a measurement.  One
 * workgroup per utterance, one thread per class; D <= 64 (40 monophones: the real case) is a single wave whose frame loop has
 * no barrier.
 *
 * facppg_ppg_force_align -- utterance b has the states s = 0 .. S_b - 1 (seq_offsets), state s of class seq[s] in [0, D) and
 * with the flag optional[s] (one byte, 0 or not 0):
 *   start          C(0,0) = em[0][seq[0]]; if state 0 is optional also C(0,1) = em[0][seq[1]]; every other state +inf
 *   t >= 1         predecessors tried in the order stay (s), advance (s-1), skip (s-2, admissible only when state s-1 is
 *                  optional) with a strict <; the local cost em[t][seq[s]] is added to the winner
 *   end            state S-1; if S-1 is optional and C(T-1,S-2) < C(T-1,S-1): state S-2.  Then a backtrace over the
 *                  back-pointers, one byte per (frame, state), in the workspace
 *   +inf loses every strict comparison and +inf + em is +inf, so there is no second case, and no NaN can form
 *   per state [sum S]   start_dev int32 (first frame; -1 for a skipped optional state), frames_dev int32,
 *                  hits_dev int32 = the segment's frames with top[t] == seq[s],
 *                  gop_dev float = (sum over the segment's frames, in frame order, of (eb[t] - em[t][seq[s]])) / frames:
 *                  at most 0, 0 where the phone is the top class on every one of its frames, 0 for a skipped state
 *   per utterance [B]   cost_dev float, ok_dev int32.  An utterance with fewer frames than mandatory states has no path:
 *                  ok = 0, cost = +inf, start = -1 and frames = hits = gop = 0 throughout.  That is not an error of the call.
 * One workgroup per utterance, one thread per state; the neighbours' costs go through a two-slot LDS exchange (one write, two
 * reads, one barrier per frame), S <= 64 is a single wave without a barrier in the frame loop.
 *
 * Refused, and nothing is launched: a NULL pointer, B or D < 1, offsets that do not start at 0 or do not increase, a length
 * beyond Tmax, floor outside (0, 1], a negative switch_cost, a class outside [0, D), S_b < 1, two adjacent optional states --
 * the skip reaches over one state only -- (FACPPG_EINVAL); D > 256 -- senone posteriors: reduce them to monophone classes
 * first --, S_b > 1024, B > 65535 (FACPPG_EUNSUPPORTED); a workspace smaller than *_workspace_bytes: (sum T) D bytes for the
 * decode, (sum T) max_b S_b bytes for the alignment (FACPPG_EWORKSPACE; 0 with facppg_last_error set for refused sizes).
 * Plain grid launches on ``stream``: none cooperative, none waits on memory, no atomics; every loop is bounded by the lengths. */
typedef struct facppg_align_config {
  float floor;         /* 1e-10f */
  float switch_cost;   /* 2.0f */
} facppg_align_config;
int facppg_ppg_emissions(const facppg_align_config* cfg, const float* x_dev, int B, int D, int Tmax,
                         const int32_t* frame_offsets_dev, const int32_t* frame_offsets_host,
                         float* em_dev, float* eb_dev, int32_t* top_dev, void* stream);
size_t facppg_ppg_decode_phones_workspace_bytes(int total_frames, int D);
int facppg_ppg_decode_phones(const facppg_align_config* cfg, const float* em_dev, const int32_t* frame_offsets_dev,
                             const int32_t* frame_offsets_host, int B, int D, int32_t* labels_dev, float* cost_dev,
                             void* ws_dev, size_t ws_bytes, void* stream);
size_t facppg_ppg_force_align_workspace_bytes(int total_frames, int S_max);
int facppg_ppg_force_align(const float* em_dev, const float* eb_dev, const int32_t* top_dev,
                           const int32_t* frame_offsets_dev, const int32_t* frame_offsets_host, int B, int D,
                           const int32_t* seq_dev, const int32_t* seq_host,
                           const uint8_t* optional_dev, const uint8_t* optional_host,
                           const int32_t* seq_offsets_dev, const int32_t* seq_offsets_host,
                           int32_t* start_dev, int32_t* frames_dev, int32_t* hits_dev, float* gop_dev,
                           float* cost_dev, int32_t* ok_dev, void* ws_dev, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FACPPG_H */
