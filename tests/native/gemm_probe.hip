// Test-only probe over the internal tapped-GEMM entry points (facppg_gemm.h).  They are not part of the
// C ABI and stay out of it: this file is linked into tests/native/libfacppg_gemm_probe.so, never into
// the product library, and forwards plain-C calls to the facppg:: C++ symbols the product exports.
#include "facppg_gemm.h"

extern "C" {

// every field of facppg::GemmArgs, in its order, as plain C (tests/gemm_helpers.py binds this struct)
struct probe_gemm_args {
  const void* A;
  int M, Cin, taps, dil, pad;
  const float* X;
  long x_bs;
  int ldx, N, col0, src_hi;
  const int* skip;
  const int* n_valid;
  int n_valid_mul, n_valid_add;
  const float* bias;
  const float* scale;
  const float* shift;
  int act;
  const unsigned char* mask;
  long mask_bs;
  int ldmask;
  const float* res;
  long res_bs;
  int ldres;
  float* C;
  long c_bs;
  int ldc, c_transposed;
  const float* gate_ts;
  long gate_bs;
  int ldgate, B;
  float* splitk_ws;
  size_t splitk_ws_bytes;
};

// a field added to GemmArgs has to be added here (and to the binding) too
static_assert(sizeof(probe_gemm_args) == sizeof(facppg::GemmArgs), "probe_gemm_args does not mirror GemmArgs");

size_t probe_args_size(void) { return sizeof(probe_gemm_args); }

size_t probe_packed_a_bytes(int M, int K) { return facppg::packed_a_float4s(M, K) * sizeof(float4); }

int probe_pack_a(const float* src, int M, int Cin, int taps, void* dst, hipStream_t s) {
  return facppg::pack_a(src, M, Cin, taps, (float4*)dst, s);
}

int probe_pack_a_strided(const float* src, int M, int Cin, int taps, long sm, long sc, long st, long off, void* dst, hipStream_t s) {
  return facppg::pack_a_strided(src, M, Cin, taps, sm, sc, st, off, (float4*)dst, s);
}

int probe_gemm(const probe_gemm_args* p, hipStream_t s) {
  facppg::GemmArgs a;
  a.A = (const float4*)p->A;
  a.M = p->M; a.Cin = p->Cin; a.taps = p->taps; a.dil = p->dil; a.pad = p->pad;
  a.X = p->X; a.x_bs = p->x_bs; a.ldx = p->ldx; a.N = p->N; a.col0 = p->col0; a.src_hi = p->src_hi;
  a.skip = p->skip; a.n_valid = p->n_valid; a.n_valid_mul = p->n_valid_mul; a.n_valid_add = p->n_valid_add;
  a.bias = p->bias; a.scale = p->scale; a.shift = p->shift; a.act = p->act;
  a.mask = p->mask; a.mask_bs = p->mask_bs; a.ldmask = p->ldmask;
  a.res = p->res; a.res_bs = p->res_bs; a.ldres = p->ldres;
  a.C = p->C; a.c_bs = p->c_bs; a.ldc = p->ldc; a.c_transposed = p->c_transposed;
  a.gate_ts = p->gate_ts; a.gate_bs = p->gate_bs; a.ldgate = p->ldgate; a.B = p->B;
  a.splitk_ws = p->splitk_ws; a.splitk_ws_bytes = p->splitk_ws_bytes;
  return facppg::gemm_launch(a, s);
}

}  // extern "C"
