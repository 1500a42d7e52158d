// STFT / inverse STFT / mel analysis / WaveGlow denoiser on gfx950.
//
// Replaces src/common/stft.py:79-138 (STFT.transform / inverse as conv1d / conv_transpose1d
// with a windowed DFT basis), src/common/layers.py:96-112 (TacotronSTFT.mel_spectrogram),
// src/common/audio_processing.py:39-88,110-116 (window_sumsquare, log compression) and
// src/waveglow/denoiser.py:63-68 (Denoiser.forward).
//
// Structure: the strided framing conv is turned into a dense GEMM by first materialising the
// frame matrix X[1024][F] (reflect padding applied while gathering), so the DFT, the mel
// filterbank and the inverse DFT are all exact-fp32 MFMA GEMMs (facppg_gemm); the inverse
// transform's overlap-add, the window-sum-square normalisation (recomputed on the HOST with
// NumPy on every call in the reference, stft.py:119-130) and the trim are one gather kernel.
#include <cstring>
#include <new>

#include "facppg_gemm.h"

using namespace facppg;

struct facppg_stft {
  int fl, hop, cutoff, n_mel, device;
  char* arena;
  float4 *fwd, *inv_t, *melb;  // packed A operands
  float* win_sq;               // [fl]
  float4* pinv;                // packed pinv(mel_basis) [cutoff][n_mel], own allocation (facppg_stft_set_mel_pinv) or NULL
};

namespace {

// frames: X[b][k][f] = xpad[f*hop + k], xpad = reflect-pad(x, fl/2)   (stft.py:86-97)
__global__ void k_frames(const float* __restrict__ x, float* __restrict__ X, const int* __restrict__ n_valid, int N, int fl,
                         int hop, int F, int* __restrict__ f_valid) {
  const int b = blockIdx.z, k = blockIdx.y;
  const int Nb = n_valid ? n_valid[b] : N;
  const int Fb = Nb / hop + 1;
  if (f_valid && blockIdx.x == 0 && k == 0 && threadIdx.x == 0) f_valid[b] = Fb;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= Fb) return;
  int j = f * hop + k - fl / 2;
  if (j < 0) j = -j;
  if (j >= Nb) j = 2 * (Nb - 1) - j;
  // an utterance of a ragged batch with Nb <= fl/2 samples (one or two frames of audio; the reference's reflect padding refuses it)
  // reflects past its other end: the index stays inside the utterance instead of reading its neighbour, or in front of the buffer
  j = min(max(j, 0), Nb - 1);
  X[((size_t)b * fl + k) * F + f] = Nb > 0 ? x[(size_t)b * N + j] : 0.0f;      // (an empty utterance has one frame of silence)
}

// S[b][2*cutoff][F] (re rows then im rows) -> magnitude, phase   (stft.py:99-105)
__global__ void k_magphase(const float* __restrict__ S, float* __restrict__ mag, float* __restrict__ phase,
                           const int* __restrict__ f_valid, int cutoff, int F) {
  const int b = blockIdx.z, c = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= (f_valid ? f_valid[b] : F)) return;
  const float re = S[((size_t)b * 2 * cutoff + c) * F + f], im = S[((size_t)b * 2 * cutoff + cutoff + c) * F + f];
  const size_t o = ((size_t)b * cutoff + c) * F + f;
  mag[o] = sqrtf(re * re + im * im);
  if (phase) phase[o] = atan2f(im, re);
}

// R = [mag*cos(phase); mag*sin(phase)]   (stft.py:110-111)
__global__ void k_recombine(const float* __restrict__ mag, const float* __restrict__ phase, float* __restrict__ R,
                            const int* __restrict__ f_valid, int cutoff, int F) {
  const int b = blockIdx.z, c = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= (f_valid ? f_valid[b] : F)) return;
  const size_t o = ((size_t)b * cutoff + c) * F + f;
  float sn, cs;
  sincosf(phase[o], &sn, &cs);
  R[((size_t)b * 2 * cutoff + c) * F + f] = mag[o] * cs;
  R[((size_t)b * 2 * cutoff + cutoff + c) * F + f] = mag[o] * sn;
}

// Denoiser core (denoiser.py:64-67): mag' = max(mag - bias*strength, 0), same phase.  With
// phase = atan2(im, re): mag'*cos(phase) = mag' * re/mag; atan2(0,0) = 0 -> (mag', 0).
__global__ void k_spectral_subtract(float* __restrict__ S, const float* __restrict__ bias, float strength,
                                    const int* __restrict__ f_valid, int cutoff, int F) {
  const int b = blockIdx.z, c = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= (f_valid ? f_valid[b] : F)) return;
  const size_t ore = ((size_t)b * 2 * cutoff + c) * F + f, oim = ore + (size_t)cutoff * F;
  const float re = S[ore], im = S[oim];
  const float mag = sqrtf(re * re + im * im);
  const float m2 = fmaxf(mag - bias[c] * strength, 0.0f);
  if (mag > 0.0f) {
    const float sc = m2 / mag;
    S[ore] = re * sc; S[oim] = im * sc;
  } else {
    S[ore] = m2; S[oim] = 0.0f;
  }
}

// Overlap-add of Zt[b][f][k] (conv_transpose1d, stft.py:113-117), window-sum-square normalisation
// where > tiny, * fl/hop, trim fl/2 both sides (stft.py:119-136; audio_processing.py:76-88).
__global__ void k_overlap_add(const float* __restrict__ Zt, const float* __restrict__ win_sq, float* __restrict__ y,
                              const int* __restrict__ f_valid, int fl, int hop, int F, long y_bs) {
  const int b = blockIdx.y;
  const int Fb = f_valid ? f_valid[b] : F;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // output index, n = i + fl/2
  if (i >= hop * (Fb - 1)) return;
  const int n = i + fl / 2;
  int f_hi = n / hop;
  if (f_hi > Fb - 1) f_hi = Fb - 1;
  int f_lo = (n - fl + hop) / hop;  // ceil((n - fl + 1)/hop)
  if (f_lo < 0) f_lo = 0;
  float acc = 0.0f, ws = 0.0f;
  for (int f = f_lo; f <= f_hi; ++f) {
    const int k = n - f * hop;
    acc += Zt[((size_t)b * F + f) * fl + k];
    ws += win_sq[k];
  }
  if (ws > 1.17549435e-38f) acc /= ws;
  y[(size_t)b * y_bs + i] = acc * ((float)fl / (float)hop);
}

struct Ws {
  int F;
  size_t X, S, Z, fv, sk, sk_bytes, total;
};
Ws ws_layout(const facppg_stft* h, int B, int N) {
  Ws w;
  w.F = N / h->hop + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.X = take((size_t)B * (h->fl + 2) * w.F * 4);   // frames, reused as R
  w.S = take((size_t)B * (h->fl + 2) * w.F * 4);
  w.Z = take((size_t)B * w.F * h->fl * 4);
  w.fv = take((size_t)B * 4);
  // split-K partial sums of the two DFT products (K = filter_length resp. 2 * cutoff: gemm_launch splits by K alone, so an
  // utterance is summed in the same order in any batch): a short utterance's [1026 x 1024] x [1024 x 201] product is 36
  // workgroups with a 16-chunk serial K loop otherwise -- 70 us for 3 us of MFMA work
  w.sk_bytes = (size_t)4 * B * (h->fl + 2) * w.F * 4;
  w.sk = take(w.sk_bytes);
  w.total = off;
  return w;
}

int run_forward(facppg_stft* h, const float* audio, const int* n_valid, int B, int N, char* ws, const Ws& w, hipStream_t s) {
  float* X = (float*)(ws + w.X);
  float* S = (float*)(ws + w.S);
  int* fv = (int*)(ws + w.fv);
  dim3 g((w.F + 255) / 256, h->fl, B);
  k_frames<<<g, 256, 0, s>>>(audio, X, n_valid, N, h->fl, h->hop, w.F, fv);
  GemmArgs a;
  a.A = h->fwd; a.M = 2 * h->cutoff; a.Cin = h->fl; a.X = X; a.x_bs = (long)h->fl * w.F; a.ldx = w.F; a.N = w.F;
  a.n_valid = fv; a.C = S; a.c_bs = (long)2 * h->cutoff * w.F; a.ldc = w.F; a.B = B;
  a.splitk_ws = (float*)(ws + w.sk); a.splitk_ws_bytes = w.sk_bytes;
  return gemm_launch(a, s);
}

int run_inverse(facppg_stft* h, const float* R, int B, char* ws, const Ws& w, const int* fv, float* out, long out_bs, hipStream_t s) {
  float* Z = (float*)(ws + w.Z);
  GemmArgs a;
  a.A = h->inv_t; a.M = h->fl; a.Cin = 2 * h->cutoff; a.X = R; a.x_bs = (long)2 * h->cutoff * w.F; a.ldx = w.F; a.N = w.F;
  a.n_valid = fv; a.C = Z; a.c_bs = (long)w.F * h->fl; a.ldc = h->fl; a.c_transposed = 1; a.B = B;
  a.splitk_ws = (float*)(ws + w.sk); a.splitk_ws_bytes = w.sk_bytes;
  if (int rc = gemm_launch(a, s)) return rc;
  const int n_out = h->hop * (w.F - 1);
  if (n_out > 0) {
    dim3 g((n_out + 255) / 256, B);
    k_overlap_add<<<g, 256, 0, s>>>(Z, h->win_sq, out, fv, h->fl, h->hop, w.F, out_bs);
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

int check_common(const facppg_stft* h, const void* a, const void* b, const void* ws, int B, int N, size_t ws_bytes, Ws* w) {
  FACPPG_REQUIRE(h && a && b && ws, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && N > h->fl / 2, FACPPG_EINVAL, "need B > 0 and N > filter_length/2 (reflect padding), got B=%d N=%d", B, N);
  *w = ws_layout(h, B, N);
  FACPPG_REQUIRE(ws_bytes >= w->total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w->total);
  return FACPPG_OK;
}

}  // namespace

extern "C" int facppg_stft_create(int filter_length, int hop_length, const float* fwd_basis_dev, const float* inv_basis_t_dev,
                                  const float* win_sq_dev, const float* mel_basis_dev, int n_mel, int device, void* stream_,
                                  facppg_stft** out) {
  FACPPG_REQUIRE(fwd_basis_dev && inv_basis_t_dev && win_sq_dev && out, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(filter_length >= 16 && filter_length % 2 == 0 && hop_length > 0 && hop_length <= filter_length, FACPPG_EINVAL,
                 "bad filter_length/hop_length %d/%d", filter_length, hop_length);
  FACPPG_REQUIRE(!mel_basis_dev || n_mel > 0, FACPPG_EINVAL, "n_mel must be positive with a mel basis");
  hipStream_t s = (hipStream_t)stream_;
  FACPPG_HIP_CHECK(hipSetDevice(device));
  facppg_stft* h = new (std::nothrow) facppg_stft();
  FACPPG_REQUIRE(h, FACPPG_EINVAL, "out of host memory");
  h->fl = filter_length; h->hop = hop_length; h->cutoff = filter_length / 2 + 1; h->n_mel = mel_basis_dev ? n_mel : 0;
  h->device = device; h->pinv = nullptr;
  const int R = 2 * h->cutoff;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  const size_t o_fwd = take(packed_a_float4s(R, h->fl) * 16), o_inv = take(packed_a_float4s(h->fl, R) * 16);
  const size_t o_mel = take(h->n_mel ? packed_a_float4s(h->n_mel, h->cutoff) * 16 : 16), o_win = take((size_t)h->fl * 4);
  if (hipMalloc((void**)&h->arena, off) != hipSuccess) {
    set_error("hipMalloc(%zu) failed", off);
    delete h;
    return FACPPG_EHIP;
  }
  h->fwd = (float4*)(h->arena + o_fwd); h->inv_t = (float4*)(h->arena + o_inv); h->melb = (float4*)(h->arena + o_mel);
  h->win_sq = (float*)(h->arena + o_win);
  int rc = pack_a(fwd_basis_dev, R, h->fl, 1, h->fwd, s);
  if (!rc) rc = pack_a(inv_basis_t_dev, h->fl, R, 1, h->inv_t, s);
  if (!rc && h->n_mel) rc = pack_a(mel_basis_dev, h->n_mel, h->cutoff, 1, h->melb, s);
  if (!rc && hipMemcpyAsync(h->win_sq, win_sq_dev, (size_t)h->fl * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = FACPPG_EHIP;
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = FACPPG_EHIP;
  if (rc) {
    (void)hipFree(h->arena);
    delete h;
    return rc;
  }
  *out = h;
  return FACPPG_OK;
}

extern "C" void facppg_stft_destroy(facppg_stft* h) {
  if (!h) return;
  if (h->pinv) (void)hipFree(h->pinv);
  (void)hipFree(h->arena);
  delete h;
}

extern "C" size_t facppg_stft_workspace_bytes(const facppg_stft* h, int B, int N) {
  if (!h || B <= 0 || N <= 0) return 0;
  return ws_layout(h, B, N).total;
}

extern "C" int facppg_stft_transform(facppg_stft* h, const float* audio_dev, const int32_t* n_valid_dev, int B, int N,
                                     float* mag_dev, float* phase_dev, void* ws_, size_t ws_bytes, void* stream_) {
  Ws w;
  if (int rc = check_common(h, audio_dev, mag_dev, ws_, B, N, ws_bytes, &w)) return rc;
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  if (int rc = run_forward(h, audio_dev, n_valid_dev, B, N, ws, w, s)) return rc;
  dim3 g((w.F + 255) / 256, h->cutoff, B);
  k_magphase<<<g, 256, 0, s>>>((float*)(ws + w.S), mag_dev, phase_dev, (int*)(ws + w.fv), h->cutoff, w.F);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_stft_inverse(facppg_stft* h, const float* mag_dev, const float* phase_dev, int B, int F, float* out_dev,
                                   void* ws_, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(h && mag_dev && phase_dev && out_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && F > 1, FACPPG_EINVAL, "need B > 0 and at least 2 frames");
  const int N = (F - 1) * h->hop;
  const Ws w = ws_layout(h, B, N);
  FACPPG_REQUIRE(ws_bytes >= w.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  float* R = (float*)(ws + w.X);
  dim3 g((F + 255) / 256, h->cutoff, B);
  k_recombine<<<g, 256, 0, s>>>(mag_dev, phase_dev, R, nullptr, h->cutoff, F);
  return run_inverse(h, R, B, ws, w, nullptr, out_dev, (long)h->hop * (F - 1), s);
}

extern "C" int facppg_stft_mel(facppg_stft* h, const float* audio_dev, const int32_t* n_valid_dev, int B, int N, float* mel_dev,
                               void* ws_, size_t ws_bytes, void* stream_) {
  Ws w;
  if (int rc = check_common(h, audio_dev, mel_dev, ws_, B, N, ws_bytes, &w)) return rc;
  FACPPG_REQUIRE(h->n_mel > 0, FACPPG_EINVAL, "handle was created without a mel basis");
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  if (int rc = run_forward(h, audio_dev, n_valid_dev, B, N, ws, w, s)) return rc;
  float* mag = (float*)(ws + w.X);  // frames no longer needed
  int* fv = (int*)(ws + w.fv);
  dim3 g((w.F + 255) / 256, h->cutoff, B);
  k_magphase<<<g, 256, 0, s>>>((float*)(ws + w.S), mag, nullptr, fv, h->cutoff, w.F);
  GemmArgs a;
  a.A = h->melb; a.M = h->n_mel; a.Cin = h->cutoff; a.X = mag; a.x_bs = (long)h->cutoff * w.F; a.ldx = w.F; a.N = w.F;
  a.n_valid = fv; a.act = ACT_LOG_CLAMP; a.C = mel_dev; a.c_bs = (long)h->n_mel * w.F; a.ldc = w.F; a.B = B;
  return gemm_launch(a, s);
}

extern "C" int facppg_denoise(facppg_stft* h, const float* audio_dev, const int32_t* n_valid_dev, const float* bias_spec_dev,
                              float strength, int B, int N, float* out_dev, void* ws_, size_t ws_bytes, void* stream_) {
  Ws w;
  if (int rc = check_common(h, audio_dev, out_dev, ws_, B, N, ws_bytes, &w)) return rc;
  FACPPG_REQUIRE(bias_spec_dev, FACPPG_EINVAL, "bias_spec is NULL");
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  if (int rc = run_forward(h, audio_dev, n_valid_dev, B, N, ws, w, s)) return rc;
  float* S = (float*)(ws + w.S);
  int* fv = (int*)(ws + w.fv);
  dim3 g((w.F + 255) / 256, h->cutoff, B);
  k_spectral_subtract<<<g, 256, 0, s>>>(S, bias_spec_dev, strength, fv, h->cutoff, w.F);
  return run_inverse(h, S, B, ws, w, fv, out_dev, (long)h->hop * (w.F - 1), s);
}

// ------------------------------------------------------------------------------------------
// Vocoder-free preview: mel -> magnitude by the pseudo-inverse of the mel basis, and Griffin-Lim (with optional momentum)
// as a device loop over the transform and inverse above.  Both definitions are stated in include/facppg.h.
// One iteration is gemm(inverse basis), k_overlap_add, k_frames, gemm(forward basis), k_gl_project: the same kernels and GEMM
// plans as facppg_stft_transform / facppg_stft_inverse, so an utterance is computed alike in any batch.
// ------------------------------------------------------------------------------------------
namespace {

constexpr int GL_VEC = 4;                  // frames per thread of k_gl_project
constexpr int GL_COLS = 64 * GL_VEC;       // frames per workgroup: one wave along the frames ...
constexpr int GL_ROWS = 4;                 // ... and one wave per bin

// Philox4x32-10 (the generator of facppg_wg.hip's k_noise)
__device__ __forceinline__ void gl_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the starting phase of (bin c, frame f) of an utterance: uniform in [-pi, pi) on a 2^-24 grid, a function of (seed, c, f) alone
__device__ __forceinline__ float gl_phase(uint64_t seed, int c, int f) {
  uint32_t r[4];
  gl_philox((uint32_t)f, (uint32_t)c, 0u, 0x474Cu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  return fmaf((float)(r[0] >> 8) * (1.0f / 16777216.0f), 6.28318530717958647692f, -3.14159265358979323846f);
}

// per-utterance frame and sample counts of a call: fv[b] = clamp(n_frames[b], 1, F) (F without lengths), nv[b] = hop * (fv[b] - 1)
__global__ void k_gl_lengths(const int* __restrict__ n_frames, int B, int F, int hop, int* __restrict__ fv, int* __restrict__ nv) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int Fb = n_frames ? min(max(n_frames[b], 1), F) : F;
  fv[b] = Fb;
  nv[b] = hop * (Fb - 1);
}

// c_0 = M * exp(i * phi0) with the drawn phases, into the inverse GEMM's operand (what k_recombine writes for a given phi0);
// phase != NULL: the drawn phases alone (facppg_griffin_lim_draw_phase)
__global__ void k_gl_seed(const float* __restrict__ mag, const uint64_t* __restrict__ seeds, float* __restrict__ R, float* __restrict__ phase,
                          const int* __restrict__ f_valid, int cutoff, int F) {
  const int b = blockIdx.z, c = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= (f_valid ? f_valid[b] : F)) return;
  const size_t o = ((size_t)b * cutoff + c) * F + f;
  const float phi = gl_phase(seeds[b], c, f);
  if (phase) { phase[o] = phi; return; }
  float sn, cs;
  sincosf(phi, &sn, &cs);
  R[((size_t)b * 2 * cutoff + c) * F + f] = mag[o] * cs;
  R[((size_t)b * 2 * cutoff + cutoff + c) * F + f] = mag[o] * sn;
}

// The projection onto the given magnitudes, with momentum: y = t + alpha * (t - t_prev), c = M * y / |y| ((M, 0) where y = 0,
// as atan2(0, 0) = 0 gives and k_spectral_subtract does), written as the next inverse GEMM's operand R (re rows, then im rows).
// T, Tp, R: [B][2 * cutoff][F]; M: [B][cutoff][F].  A thread owns GL_VEC consecutive frames of one bin, re and im: with F a
// multiple of 4 (VEC) every row starts 16-byte aligned and a full group moves as one float4.
// A workgroup is GL_ROWS bins x GL_COLS frames, a wave per bin (utterances of a few hundred frames keep most lanes busy).
// part != NULL (last iteration): the workgroup's sums of (|t| - M)^2 and M^2 over its valid frames, in float64, at
// part[((b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2 + {0, 1}]; summed thread by thread, then by a fixed tree, so
// they depend on the utterance's own frames alone.  T == NULL: t = 0, sums only (the convergence figure of a call without iterations).
template <bool VEC>
__global__ __launch_bounds__(256) void k_gl_project(const float* __restrict__ T, const float* __restrict__ Tp, const float* __restrict__ M,
                                                    float* __restrict__ R, const int* __restrict__ f_valid, float alpha, int cutoff, int F,
                                                    double* __restrict__ part) {
  const int b = blockIdx.z, tid = threadIdx.x, c = blockIdx.y * GL_ROWS + (tid >> 6);
  const int f0 = (blockIdx.x * 64 + (tid & 63)) * GL_VEC;
  const int nvld = c < cutoff ? min(max(f_valid[b] - f0, 0), GL_VEC) : 0;
  const size_t ore = ((size_t)b * 2 * cutoff + c) * F + f0, oim = ore + (size_t)cutoff * F, om = ((size_t)b * cutoff + c) * F + f0;
  alignas(16) float re[GL_VEC], im[GL_VEC], pr[GL_VEC], pi[GL_VEC], m[GL_VEC];
#pragma unroll
  for (int j = 0; j < GL_VEC; ++j) re[j] = im[j] = pr[j] = pi[j] = m[j] = 0.0f;
  const bool full = VEC && nvld == GL_VEC;
  if (full) {
    *(float4*)m = *(const float4*)(M + om);
    if (T) {
      *(float4*)re = *(const float4*)(T + ore); *(float4*)im = *(const float4*)(T + oim);
      *(float4*)pr = *(const float4*)(Tp + ore); *(float4*)pi = *(const float4*)(Tp + oim);
    }
  } else {
    for (int j = 0; j < nvld; ++j) {
      m[j] = M[om + j];
      if (T) { re[j] = T[ore + j]; im[j] = T[oim + j]; pr[j] = Tp[ore + j]; pi[j] = Tp[oim + j]; }
    }
  }
  if (T) {
    alignas(16) float cr[GL_VEC], ci[GL_VEC];
#pragma unroll
    for (int j = 0; j < GL_VEC; ++j) {
      const float yr = re[j] + alpha * (re[j] - pr[j]), yi = im[j] + alpha * (im[j] - pi[j]);
      const float ym = sqrtf(yr * yr + yi * yi);
      if (ym > 0.0f) {
        const float sc = m[j] / ym;
        cr[j] = yr * sc; ci[j] = yi * sc;
      } else {
        cr[j] = m[j]; ci[j] = 0.0f;
      }
    }
    if (full) {
      *(float4*)(R + ore) = *(const float4*)cr; *(float4*)(R + oim) = *(const float4*)ci;
    } else {
      for (int j = 0; j < nvld; ++j) { R[ore + j] = cr[j]; R[oim + j] = ci[j]; }
    }
  }
  if (!part) return;
  __shared__ double red[2][256];
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int j = 0; j < GL_VEC; ++j) {
    if (j < nvld) {
      const double d = (double)sqrtf(re[j] * re[j] + im[j] * im[j]) - (double)m[j];
      num += d * d;
      den += (double)m[j] * (double)m[j];
    }
  }
  red[0][tid] = num; red[1][tid] = den;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    double* p = part + (((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    p[0] = red[0][0]; p[1] = red[1][0];
  }
}

// sc[b] = sqrt(sum (|t| - M)^2 / sum M^2) from k_gl_project's partial sums (0 where M = 0): thread t adds the bin groups t, t + 256,
// ... block by block, then a fixed tree.  Workgroups behind an utterance's last frame hold exact zeros, so the padded length of the
// batch does not enter the sum.
__global__ __launch_bounds__(256) void k_gl_sc_finish(const double* __restrict__ part, int nrow, int nblk, float* __restrict__ sc) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double red[2][256];
  double num = 0.0, den = 0.0;
  for (int c = tid; c < nrow; c += 256)
    for (int x = 0; x < nblk; ++x) {
      const double* p = part + (((size_t)b * nrow + c) * nblk + x) * 2;
      num += p[0]; den += p[1];
    }
  red[0][tid] = num; red[1][tid] = den;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) sc[b] = red[1][0] > 0.0 ? (float)sqrt(red[0][0] / red[1][0]) : 0.0f;
}

// E = exp(mel) over each utterance's own frames (the mel inversion's GEMM operand)
__global__ void k_exp(const float* __restrict__ mel, float* __restrict__ E, const int* __restrict__ f_valid, int n_mel, int F) {
  const int b = blockIdx.z, m = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= (f_valid ? min(f_valid[b], F) : F)) return;
  const size_t o = ((size_t)b * n_mel + m) * F + f;
  E[o] = expf(mel[o]);
}

// Griffin-Lim workspace: the transform's own layout for N = hop * (F - 1) samples, then the second spectrum (t_n and t_{n-1} swap
// places every iteration), the sample counts and the convergence partial sums
struct GlWs {
  Ws w;
  size_t S2, nv, part, total;
  int nblk, nrow;
};
GlWs gl_layout(const facppg_stft* h, int B, int F) {
  GlWs g;
  g.w = ws_layout(h, B, h->hop * (F - 1));
  size_t off = g.w.total;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  g.nblk = (F + GL_COLS - 1) / GL_COLS;
  g.nrow = (h->cutoff + GL_ROWS - 1) / GL_ROWS;
  g.S2 = take((size_t)B * (h->fl + 2) * F * 4);
  g.nv = take((size_t)B * 4);
  g.part = take((size_t)B * g.nrow * g.nblk * 2 * 8);
  g.total = off;
  const size_t mel = (size_t)B * (h->n_mel > 0 ? h->n_mel : 1) * F * 4;   // facppg_mel_to_magnitude's exp(mel)
  if (g.total < mel) g.total = mel;
  return g;
}

}  // namespace

extern "C" int facppg_stft_set_mel_pinv(facppg_stft* h, const float* pinv_dev, void* stream_) {
  FACPPG_REQUIRE(h && pinv_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(h->n_mel > 0, FACPPG_EINVAL, "handle was created without a mel basis");
  FACPPG_HIP_CHECK(hipSetDevice(h->device));
  if (!h->pinv) FACPPG_HIP_CHECK(hipMalloc((void**)&h->pinv, packed_a_float4s(h->cutoff, h->n_mel) * 16));
  return pack_a(pinv_dev, h->cutoff, h->n_mel, 1, h->pinv, (hipStream_t)stream_);
}

extern "C" size_t facppg_griffin_lim_workspace_bytes(const facppg_stft* h, int B, int F) {
  if (!h || B <= 0 || F < 2) return 0;
  return gl_layout(h, B, F).total;
}

extern "C" int facppg_mel_to_magnitude(facppg_stft* h, const float* mel_dev, const int32_t* n_frames_dev, int B, int F, float* mag_dev,
                                       void* ws_, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(h && mel_dev && mag_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && F > 0, FACPPG_EINVAL, "need B > 0 and F > 0, got B=%d F=%d", B, F);
  FACPPG_REQUIRE(h->n_mel > 0, FACPPG_EINVAL, "handle was created without a mel basis");
  FACPPG_REQUIRE(h->pinv, FACPPG_EINVAL, "handle has no mel pseudo-inverse (facppg_stft_set_mel_pinv)");
  const size_t need = (size_t)B * h->n_mel * F * 4;
  FACPPG_REQUIRE(ws_bytes >= need, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream_;
  float* E = (float*)ws_;
  if (n_frames_dev) FACPPG_HIP_CHECK(hipMemsetAsync(mag_dev, 0, (size_t)B * h->cutoff * F * 4, s));
  dim3 g((F + 255) / 256, h->n_mel, B);
  k_exp<<<g, 256, 0, s>>>(mel_dev, E, n_frames_dev, h->n_mel, F);
  GemmArgs a;
  a.A = h->pinv; a.M = h->cutoff; a.Cin = h->n_mel; a.X = E; a.x_bs = (long)h->n_mel * F; a.ldx = F; a.N = F;
  a.n_valid = n_frames_dev; a.act = ACT_RELU; a.C = mag_dev; a.c_bs = (long)h->cutoff * F; a.ldc = F; a.B = B;
  return gemm_launch(a, s);
}

extern "C" int facppg_griffin_lim_draw_phase(const facppg_stft* h, const uint64_t* seeds_dev, int B, int F, float* phase_dev, void* stream_) {
  FACPPG_REQUIRE(h && seeds_dev && phase_dev, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(B > 0 && F > 0, FACPPG_EINVAL, "need B > 0 and F > 0, got B=%d F=%d", B, F);
  dim3 g((F + 255) / 256, h->cutoff, B);
  k_gl_seed<<<g, 256, 0, (hipStream_t)stream_>>>(nullptr, seeds_dev, nullptr, phase_dev, nullptr, h->cutoff, F);
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}

extern "C" int facppg_griffin_lim(facppg_stft* h, const float* mag_dev, const int32_t* n_frames_dev, const float* phi0_dev,
                                  const uint64_t* seeds_dev, int n_iters, float alpha, int B, int F, float* out_dev, float* sc_dev,
                                  void* ws_, size_t ws_bytes, void* stream_) {
  FACPPG_REQUIRE(h && mag_dev && out_dev && ws_, FACPPG_EINVAL, "NULL argument");
  FACPPG_REQUIRE(phi0_dev || seeds_dev, FACPPG_EINVAL, "need the starting phases or the seeds to draw them from");
  FACPPG_REQUIRE(B > 0 && F >= 2, FACPPG_EINVAL, "need B > 0 and at least 2 frames, got B=%d F=%d", B, F);
  FACPPG_REQUIRE(n_iters >= 0, FACPPG_EINVAL, "n_iters must not be negative, got %d", n_iters);
  FACPPG_REQUIRE(alpha >= 0.0f && alpha < 1.0f, FACPPG_EINVAL, "need 0 <= alpha < 1, got %g", (double)alpha);
  const GlWs g = gl_layout(h, B, F);
  FACPPG_REQUIRE(ws_bytes >= g.total, FACPPG_EWORKSPACE, "workspace has %zu bytes, need %zu", ws_bytes, g.total);
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)ws_;
  const int N = h->hop * (F - 1), cutoff = h->cutoff;
  int *fv = (int*)(ws + g.w.fv), *nv = (int*)(ws + g.nv);
  float* R = (float*)(ws + g.w.X);
  double* part = (double*)(ws + g.part);
  k_gl_lengths<<<(B + 63) / 64, 64, 0, s>>>(n_frames_dev, B, F, h->hop, fv, nv);
  // the signal of every iteration lives in out_dev: k_overlap_add writes an utterance's own samples only, the rest stays zero
  if (n_frames_dev) FACPPG_HIP_CHECK(hipMemsetAsync(out_dev, 0, (size_t)B * N * 4, s));
  const dim3 gb((F + 255) / 256, cutoff, B), gp(g.nblk, g.nrow, B);
  if (phi0_dev) k_recombine<<<gb, 256, 0, s>>>(mag_dev, phi0_dev, R, fv, cutoff, F);
  else k_gl_seed<<<gb, 256, 0, s>>>(mag_dev, seeds_dev, R, nullptr, fv, cutoff, F);
  const bool vec = F % GL_VEC == 0 && (uintptr_t)mag_dev % 16 == 0;
  auto project = [&](const float* T, const float* Tp, float a, double* p) {
    if (vec) k_gl_project<true><<<gp, 256, 0, s>>>(T, Tp, mag_dev, R, fv, a, cutoff, F, p);
    else k_gl_project<false><<<gp, 256, 0, s>>>(T, Tp, mag_dev, R, fv, a, cutoff, F, p);
  };
  const float* Tprev = nullptr;
  for (int n = 1; n <= n_iters; ++n) {
    if (int rc = run_inverse(h, R, B, ws, g.w, fv, out_dev, N, s)) return rc;
    Ws w = g.w;
    if (!(n & 1)) w.S = g.S2;
    if (int rc = run_forward(h, out_dev, nv, B, N, ws, w, s)) return rc;   // frames overwrite R: its product is done
    const float* T = (const float*)(ws + w.S);
    project(T, Tprev ? Tprev : T, Tprev ? alpha : 0.0f, sc_dev && n == n_iters ? part : nullptr);
    Tprev = T;
  }
  if (int rc = run_inverse(h, R, B, ws, g.w, fv, out_dev, N, s)) return rc;
  if (sc_dev) {
    if (n_iters == 0) project(nullptr, nullptr, 0.0f, part);
    k_gl_sc_finish<<<B, 256, 0, s>>>(part, g.nrow, g.nblk, sc_dev);
  }
  FACPPG_HIP_CHECK(hipGetLastError());
  return FACPPG_OK;
}
