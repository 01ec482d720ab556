// The InstanceNorm-on-load operand transform, defined once.
//
// A producer writes its raw output plus fused statistics; every consumer turns the statistics into mean / rstd in its
// prologue and applies InstanceNorm, the activation and the squeeze-excite gate while it stages its operand.  This
// arithmetic is the numerical contract with the reference -- biased variance in fp64, clamped at 0, eps = 1e-5, rounded
// to fp32 -- and every kernel takes it from here.  Device functions only: no state, no kernel.
//
// Two scalings of the sums exist, and each consumer names the one it uses:
//   norm_coef_times_inv   sums * (double)inv, inv a FLOAT reciprocal of the pixel count: every on-load consumer (the
//                         MFMA, Winograd, split-bf16, direct pointwise and one-channel convolutions, the BiFPN nodes);
//   norm_coef_over_count  sums / (double)P: norm_apply_kernel, conv3d_out_fold_kernel (bit-equal to the former by
//                         contract) and the depthwise + pool kernel (which divides its LDS totals the same way).
// Where P is a power of two they are the same double.  Elsewhere they differ by the rounding of the float reciprocal
// (2^-24 relative), which is below the final fp32 rounding of mean / rstd in most cases but not in all.
//
// Two stored forms of the [C | C] coefficient table exist (NormTable), each with its apply: (mean, rstd) with norm_sub4,
// (-mean * rstd, rstd) with norm_fma4.  A consumer that splits a layer with another kernel form takes that form's table
// or derives the same products from it: conv3d_wino.hip stores FmaRstd, conv3d_wino_pw.hip stores MeanRstd and forms
// -mean * rstd at its commit -- the same product, so the two agree bit for bit.
#pragma once
#include <type_traits>
#include "jh_common.h"

namespace jh {

#if defined(__HIPCC__)
constexpr double kNormEps = 1e-5;

struct NormCoef { float mean, rstd; };

// THE formula.  m1 = E[x], m2 = E[x^2] in fp64.
__device__ __forceinline__ NormCoef norm_coef(double m1, double m2) {
  double var = m2 - m1 * m1;
  if (var < 0.0) var = 0.0;
  return NormCoef{(float)m1, (float)(1.0 / sqrt(var + kNormEps))};
}
// ... from one (n, c) statistics slot (kStatW doubles), in the two scalings (see above)
__device__ __forceinline__ NormCoef norm_coef_times_inv(const double* st, float inv) {
  return norm_coef(exact_read(st) * (double)inv, exact_read(st + kLimbs) * (double)inv);
}
__device__ __forceinline__ NormCoef norm_coef_over_count(const double* st, int P) {
  return norm_coef(exact_read(st) / (double)P, exact_read(st + kLimbs) / (double)P);
}

enum class NormTable {
  MeanRstd,   // (mean, rstd): applied as (v - mean) * rstd
  FmaRstd,    // (-mean * rstd, rstd): applied as one fma(v, rstd, -mean * rstd)
};
// Coefficients of image n's C channels from stats [N][C][kStatW] (times-inv scaling) into tbl[0 .. C) and
// tbl[rstd_at .. rstd_at + C): the [C | C] table of the workgroup kernels has rstd_at = C.
// Thread t of `stride`: 256-thread workgroups or a 64-lane loader wave.  (conv_pw_direct.hip, one lane per channel and
// no loop, calls the reader itself.)
__device__ __forceinline__ void norm_table_fill(NormTable form, float* tbl, int rstd_at, const double* stats, int n, int C,
                                                float inv, int t, int stride) {
  for (int c = t; c < C; c += stride) {
    const NormCoef k = norm_coef_times_inv(stats + ((size_t)n * C + c) * kStatW, inv);
    tbl[c] = form == NormTable::MeanRstd ? k.mean : -k.mean * k.rstd;
    tbl[rstd_at + c] = k.rstd;
  }
}

// ---- apply: four channels of one pixel
__device__ __forceinline__ float4 norm_sub4(float4 v, float4 mean, float4 rstd) {
  v.x = (v.x - mean.x) * rstd.x; v.y = (v.y - mean.y) * rstd.y;
  v.z = (v.z - mean.z) * rstd.z; v.w = (v.w - mean.w) * rstd.w;
  return v;
}
__device__ __forceinline__ float4 norm_fma4(float4 v, float4 nmr, float4 rstd) {
  v.x = __fmaf_rn(v.x, rstd.x, nmr.x); v.y = __fmaf_rn(v.y, rstd.y, nmr.y);
  v.z = __fmaf_rn(v.z, rstd.z, nmr.z); v.w = __fmaf_rn(v.w, rstd.w, nmr.w);
  return v;
}
// activation on load: SiLU through v_exp_f32 / v_rcp_f32 (silu_fast)
__device__ __forceinline__ float act(float v, int kind) {
  if (kind == ACT_RELU) return fmaxf(v, 0.f);
  if (kind == ACT_SILU) return silu_fast(v);
  return v;
}
__device__ __forceinline__ float4 act4(float4 v, int kind) {
  if (kind == ACT_RELU) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
  } else if (kind == ACT_SILU) {
    v.x = silu_fast(v.x); v.y = silu_fast(v.y);
    v.z = silu_fast(v.z); v.w = silu_fast(v.w);
  }
  return v;
}
// IEEE SiLU (expf + division): the stand-alone fusion pass and the squeeze-excite hidden unit
__device__ __forceinline__ float silu_exact(float v) { return v / (1.f + expf(-v)); }
__device__ __forceinline__ float act_exact(float v, int kind) {
  if (kind == ACT_RELU) return fmaxf(v, 0.f);
  if (kind == ACT_SILU) return silu_exact(v);
  return v;
}
// the operand split of the split-bf16 kernels: hi = bf16(v), lo = bf16(v - hi)
typedef __bf16 opbf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split_bf16x4(float4 v, opbf16x4& hi, opbf16x4& lo) {
  hi = opbf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
  lo = opbf16x4{(__bf16)(v.x - (float)hi[0]), (__bf16)(v.y - (float)hi[1]),
                (__bf16)(v.z - (float)hi[2]), (__bf16)(v.w - (float)hi[3])};
}

// ---- mode of a hand-scheduled commit: 0 copy, 1 norm, 2 norm + ReLU, 3 norm + SiLU; dispatched once per commit
__device__ __forceinline__ int operand_mode(const double* in_stats, int in_act) {
  return !in_stats ? 0 : (in_act == ACT_RELU ? 2 : (in_act == ACT_SILU ? 3 : 1));
}
__host__ __device__ constexpr int mode_act(int mode) { return mode == 2 ? ACT_RELU : (mode == 3 ? ACT_SILU : ACT_NONE); }
template <class F>
__device__ __forceinline__ void dispatch_mode(int mode, F&& f) {
  if (mode == 0) f(std::integral_constant<int, 0>{});
  else if (mode == 3) f(std::integral_constant<int, 3>{});
  else if (mode == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}

// ---- squeeze-excite gate: gate[c] = sigmoid(We silu(Wr mean + br) + be), one definition for se_gate_kernel and the
// consumers that compute the gate in their prologue (the loop structure is theirs)
__device__ __forceinline__ float se_mean(const double* pool_slot, float inv_hw) {
  return (float)(exact_read(pool_slot) * (double)inv_hw);
}
__device__ __forceinline__ float se_hidden(float br_j, const float* wr_row, const float* mean, int C) {
  float acc = br_j;
  for (int c = 0; c < C; ++c) acc = fmaf(wr_row[c], mean[c], acc);
  return silu_exact(acc);
}
__device__ __forceinline__ float se_gate_value(float be_c, const float* we_row, const float* hid, int S) {
  float acc = be_c;
  for (int j = 0; j < S; ++j) acc = fmaf(we_row[j], hid[j], acc);
  return 1.f / (1.f + expf(-acc));
}
#endif

}  // namespace jh
