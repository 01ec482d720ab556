// The soft-argmax tail of the V2V network (csrc/softargmax.h).
//
//  softargmax          softplus + spatial soft-argmax + confidences,
//                      jarvis/hybridnet/model.py:73-88
//  ... spread          the second moments and the arg-max of the same pass (jh_softargmax_spread)
//  heatmap_final       softplus(softplus(x)) in the reference's NCDHW layout
#include "jh_common.h"
#include "argmax.h"
#include "softargmax.h"

namespace jh {

// ------------------------------------------------------------------ soft-argmax
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// x: [T][Gh^3][Jp].  partial: [T][Jp][4][kLimbs] doubles (sum h, sum h*i, sum h*j, sum h*k; order-
// independent accumulation, jh_common.h),
// pmax: [T][Jp] floats as ordered ints (h > 0 so the int order equals the float order).
//
// SPREAD: the same pass also leaves the second moments and the arg-max of x (jh_softargmax_spread):
//   spart [T][Jp][kSpreadSums][kLimbs]: S_0, S_i, S_j, S_k, S_ii, S_ij, S_ik, S_jj, S_jk, S_kk of h, every one
//     accumulated in DOUBLE per lane (h * a * b of an fp32 h and two voxel indices is exact in fp64), summed over
//     the rows of the block in a fixed order and handed over through exact_add: one addend per block and sum, i.e.
//     ceil(Gh^3 / ppb) addends -- 98 per frame set at Gh = 32, Jp = 24; the launcher holds it to the 2^13 of the limb
//     scheme -- so the sums are bit-reproducible from run to run.  The float sums above are NOT reused for the
//     covariance: their relative error of ~1e-6 on a mean near 31 voxels is ~2e-3 voxel^2 after the subtraction,
//     more than the whole variance of a sharp joint.
//   skey [T][Jp]: max over the voxels of order_key(x, p) (argmax.h): the maximum of x, the LOWEST flat index among
//     equal maxima.  x may be negative, so the key is the order-preserving map of the float's bits, not the bits
//     themselves.
// The float sums and maxima are computed by the same statements in the same order with SPREAD on and off.
constexpr int kSpreadSums = 10, kSpreadRound = 5;          // (sums; sums per round of the block reduction)
// one voxel's contribution of one channel to the ten double sums
__device__ __forceinline__ void spread_acc(double* s, float h, double di, double dj, double dk) {
  const double d = (double)h, hi = d * di, hj = d * dj, hk = d * dk;
  s[0] += d; s[1] += hi; s[2] += hj; s[3] += hk;
  s[4] += hi * di; s[5] += hi * dj; s[6] += hi * dk;
  s[7] += hj * dj; s[8] += hj * dk; s[9] += hk * dk;
}

template <bool SPREAD>
__global__ __launch_bounds__(256) void softargmax_partial_kernel(
    const float* __restrict__ x, double* __restrict__ partial, int* __restrict__ pmax,
    double* __restrict__ spart, unsigned long long* __restrict__ skey, int Gh, int Jp, int ppb) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int q = Jp >> 2, rows = 256 / q, tid = threadIdx.x;
  const bool active = tid < rows * q;
  const int c4 = tid % q, row = tid / q;
  const int t = blockIdx.y;
  const int P = Gh * Gh * Gh;
  const int p0 = blockIdx.x * ppb, p1 = min(P, p0 + ppb);
  float4 s0 = make_float4(0, 0, 0, 0), si = s0, sj = s0, sk = s0, mx = s0;
  [[maybe_unused]] double ds[SPREAD ? 4 : 1][SPREAD ? kSpreadSums : 1] = {};
  [[maybe_unused]] unsigned long long key[SPREAD ? 4 : 1] = {};
  if (active) {
    for (int p = p0 + row; p < p1; p += rows) {
      const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)t * P + p) * Jp + c4 * 4);
      const float4 h = make_float4(softplus_f(v.x), softplus_f(v.y), softplus_f(v.z), softplus_f(v.w));
      const float fk = (float)(p % Gh), fj = (float)((p / Gh) % Gh), fi = (float)(p / (Gh * Gh));
      s0.x += h.x; s0.y += h.y; s0.z += h.z; s0.w += h.w;
      si.x += h.x * fi; si.y += h.y * fi; si.z += h.z * fi; si.w += h.w * fi;
      sj.x += h.x * fj; sj.y += h.y * fj; sj.z += h.z * fj; sj.w += h.w * fj;
      sk.x += h.x * fk; sk.y += h.y * fk; sk.z += h.z * fk; sk.w += h.w * fk;
      mx.x = fmaxf(mx.x, h.x); mx.y = fmaxf(mx.y, h.y); mx.z = fmaxf(mx.z, h.z); mx.w = fmaxf(mx.w, h.w);
      if constexpr (SPREAD) {
        const double di = (double)fi, dj = (double)fj, dk = (double)fk;
        spread_acc(ds[0], h.x, di, dj, dk);
        spread_acc(ds[1], h.y, di, dj, dk);
        spread_acc(ds[2], h.z, di, dj, dk);
        spread_acc(ds[3], h.w, di, dj, dk);
        key[0] = max_u64(key[0], order_key(v.x, (unsigned)p));
        key[1] = max_u64(key[1], order_key(v.y, (unsigned)p));
        key[2] = max_u64(key[2], order_key(v.z, (unsigned)p));
        key[3] = max_u64(key[3], order_key(v.w, (unsigned)p));
      }
    }
  }
  // block reduce: sm [rows][q][5][4]
  if (active) {
    float4* p = reinterpret_cast<float4*>(sm) + ((size_t)row * q + c4) * 5;
    p[0] = s0; p[1] = si; p[2] = sj; p[3] = sk; p[4] = mx;
  }
  __syncthreads();
  for (int i = tid; i < q * 4 * 5; i += 256) {
    const int comp = i & 3, v = (i >> 2) % 5, cq = (i >> 2) / 5;
    const int ch = cq * 4 + comp;
    if (v < 4) {
      float acc = 0.f;
      for (int r = 0; r < rows; ++r) acc += sm[(((size_t)r * q + cq) * 5 + v) * 4 + comp];
      exact_add(partial + (((size_t)t * Jp + ch) * 4 + v) * kLimbs, (double)acc);
    } else {
      float m = 0.f;
      for (int r = 0; r < rows; ++r) m = fmaxf(m, sm[(((size_t)r * q + cq) * 5 + v) * 4 + comp]);
      atomicMax(pmax + (size_t)t * Jp + ch, __float_as_int(m));
    }
  }
  if constexpr (SPREAD) {
    // the same LDS again, as doubles, in two rounds of five sums (all ten at once would be 88 B x 4 channels a lane:
    // 90 KB): dm [rows][Jp][kSpreadRound + 1], the last one the key's bits (first round only)
    constexpr int W = kSpreadRound + 1;
    double* dm = reinterpret_cast<double*>(sm);
#pragma unroll
    for (int round = 0; round < kSpreadSums / kSpreadRound; ++round) {
      __syncthreads();
      if (active) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double* d = dm + ((size_t)row * Jp + c4 * 4 + c) * W;
#pragma unroll
          for (int v = 0; v < kSpreadRound; ++v) d[v] = ds[c][round * kSpreadRound + v];
          if (round == 0) d[kSpreadRound] = __longlong_as_double((long long)key[c]);
        }
      }
      __syncthreads();
      for (int i = tid; i < Jp * W; i += 256) {
        const int v = i % W, ch = i / W;
        if (v < kSpreadRound) {
          double acc = 0.0;
          for (int r = 0; r < rows; ++r) acc += dm[((size_t)r * Jp + ch) * W + v];
          exact_add(spart + (((size_t)t * Jp + ch) * kSpreadSums + round * kSpreadRound + v) * kLimbs, acc);
        } else if (round == 0) {
          unsigned long long m = 0;
          for (int r = 0; r < rows; ++r)
            m = max_u64(m, (unsigned long long)__double_as_longlong(dm[((size_t)r * Jp + ch) * W + v]));
          atomicMax(skey + (size_t)t * Jp + ch, m);
        }
      }
    }
  }
}

__global__ void softargmax_final_kernel(const double* __restrict__ partial,
                                        const int* __restrict__ pmax,
                                        const int* __restrict__ center3d, float* __restrict__ points,
                                        float* __restrict__ conf, int J, int Jp, float spacing,
                                        float roi) {
  const int t = blockIdx.x, j = threadIdx.x;
  if (j >= J) return;
  const double* pl = partial + ((size_t)t * Jp + j) * 4 * kLimbs;
  const double p[4] = {exact_read(pl), exact_read(pl + kLimbs), exact_read(pl + 2 * kLimbs),
                       exact_read(pl + 3 * kLimbs)};
  const float norm = (float)p[0];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float idx = __fdiv_rn((float)p[1 + a], norm);
    // idx * GRID_SPACING * 2 - ROI_CUBE_SIZE / 2 + center3D   (model.py:86-87)
    const float mm = __fadd_rn(__fsub_rn(__fmul_rn(__fmul_rn(idx, spacing), 2.f), __fdiv_rn(roi, 2.f)),
                               (float)center3d[t * 3 + a]);
    points[((size_t)t * J + j) * 3 + a] = mm;
  }
  const float m = __int_as_float(pmax[(size_t)t * Jp + j]);
  conf[(size_t)t * J + j] = __fdiv_rn(fminf(m, 255.f), 255.f);
}

// The spread of the heat map of (t, j) from the sums above (include/jarvis_hip.h, jh_softargmax_spread):
//   mass = S_0 of the fp64 sums, rounded once (softargmax_final_kernel's `norm` is the same sum from the fp32 block
//          sums: the two agree to the fp32 summation error of a block, not to the bit);
//   cov  = (S_ab / S_0 - (S_a / S_0)(S_b / S_0)) * (2 * spacing)^2 in fp64, rounded once; xx, xy, xz, yy, yz, zz;
//   peak = the voxel of the key, mapped to millimetres by the points' own expression.
// valid != nullptr: the rows of a frame set that is not valid are NaN.
__global__ void softargmax_spread_final_kernel(const double* __restrict__ spart,
                                               const unsigned long long* __restrict__ skey,
                                               const int* __restrict__ center3d, const int* __restrict__ valid,
                                               float* __restrict__ cov, float* __restrict__ peak,
                                               float* __restrict__ mass, int J, int Jp, int Gh, float spacing,
                                               float roi) {
  const int t = blockIdx.x, j = threadIdx.x;
  if (j >= J) return;
  float* co = cov + ((size_t)t * J + j) * 6;
  float* pk = peak + ((size_t)t * J + j) * 3;
  if (valid && valid[t] == 0) {
    const float nan = __int_as_float(0x7fc00000);
    for (int a = 0; a < 6; ++a) co[a] = nan;
    for (int a = 0; a < 3; ++a) pk[a] = nan;
    mass[(size_t)t * J + j] = nan;
    return;
  }
  const double* sl = spart + ((size_t)t * Jp + j) * kSpreadSums * kLimbs;
  double S[kSpreadSums];
#pragma unroll
  for (int v = 0; v < kSpreadSums; ++v) S[v] = exact_read(sl + v * kLimbs);
  mass[(size_t)t * J + j] = (float)S[0];
  const double m[3] = {S[1] / S[0], S[2] / S[0], S[3] / S[0]};
  const double s2 = (2.0 * (double)spacing) * (2.0 * (double)spacing);
  int o = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b, ++o) co[o] = (float)((S[4 + o] / S[0] - m[a] * m[b]) * s2);
  const unsigned p = key_index(skey[(size_t)t * Jp + j]);
  const unsigned vox[3] = {p / (unsigned)(Gh * Gh), (p / (unsigned)Gh) % (unsigned)Gh, p % (unsigned)Gh};
#pragma unroll
  for (int a = 0; a < 3; ++a)
    pk[a] = __fadd_rn(__fsub_rn(__fmul_rn(__fmul_rn((float)vox[a], spacing), 2.f), __fdiv_rn(roi, 2.f)),
                      (float)center3d[t * 3 + a]);
}

// heatmap_final = softplus(softplus(x)) in the reference's NCDHW layout
__global__ __launch_bounds__(256) void heatmap_final_kernel(const float* __restrict__ x,
                                                            float* __restrict__ out, int J, int Jp,
                                                            size_t P, int T) {
  const size_t total = (size_t)T * J * P;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i % P;
    const int j = (int)((i / P) % J);
    const size_t t = i / (P * J);
    out[i] = softplus_f(softplus_f(x[(t * P + p) * Jp + j]));
  }
}

// sp == nullptr: the plain form.  Otherwise the spread form: sp->sums / sp->key are zeroed here (ONE allocation, key
// behind sums: softargmax_spread_sums() doubles, then T * Jp keys), the three outputs are rows of T frame sets.
int launch_softargmax(const float* x, const int* center3d, double* partial, int* pmax,
                      float* points, float* conf, float* heatmap_final, int T, int J, int Jp,
                      int Gh, float spacing, float roi, hipStream_t s, const SoftargmaxSpread* sp) {
  const int P = Gh * Gh * Gh;
  const int q = Jp / 4;
  JH_REQUIRE(q >= 1 && q <= 64 && J <= 256, "soft-argmax joint count");
  const int rows = 256 / q;
  const size_t pbytes = (size_t)T * Jp * 4 * kLimbs * sizeof(double), mbytes = (size_t)T * Jp * sizeof(int);
  if (reinterpret_cast<char*>(pmax) == reinterpret_cast<char*>(partial) + pbytes) {
    if (launch_zero(partial, pbytes + mbytes, s)) return 1;      // (one launch: the predictor allocates them as one)
  } else {
    if (launch_zero(partial, pbytes, s)) return 1;
    if (launch_zero(pmax, mbytes, s)) return 1;
  }
  const int ppb = rows * 8;
  dim3 grid((P + ppb - 1) / ppb, T);
  if (sp) {
    JH_REQUIRE(sp->sums && sp->key && sp->cov && sp->peak && sp->mass, "soft-argmax spread: null pointer");
    JH_REQUIRE(grid.x <= (1u << 13), "soft-argmax spread: more than 2^13 blocks per frame set");
    if (launch_zero(sp->sums, softargmax_spread_sums(T, Jp) * sizeof(double) +
                                  (size_t)T * Jp * sizeof(unsigned long long), s)) return 1;
    hipLaunchKernelGGL(softargmax_partial_kernel<true>, grid, dim3(256),
                       (size_t)rows * Jp * (kSpreadRound + 1) * sizeof(double), s, x, partial, pmax, sp->sums,
                       sp->key, Gh, Jp, ppb);
  } else {
    hipLaunchKernelGGL(softargmax_partial_kernel<false>, grid, dim3(256), (size_t)rows * q * 20 * sizeof(float),
                       s, x, partial, pmax, (double*)nullptr, (unsigned long long*)nullptr, Gh, Jp, ppb);
  }
  JH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(softargmax_final_kernel, dim3(T), dim3(256), 0, s, partial, pmax, center3d,
                     points, conf, J, Jp, spacing, roi);
  JH_CHECK_HIP(hipGetLastError());
  if (sp) {
    hipLaunchKernelGGL(softargmax_spread_final_kernel, dim3(T), dim3(256), 0, s, sp->sums, sp->key,
                       center3d, sp->valid, sp->cov, sp->peak, sp->mass, J, Jp, Gh, spacing, roi);
    JH_CHECK_HIP(hipGetLastError());
  }
  if (heatmap_final) {
    hipLaunchKernelGGL(heatmap_final_kernel, dim3(stride_blocks((size_t)T * J * P)), dim3(256), 0, s, x, heatmap_final, J, Jp,
                       (size_t)P, T);
    JH_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

size_t softargmax_spread_sums(int T, int Jp) { return (size_t)T * Jp * kSpreadSums * kLimbs; }

}  // namespace jh
