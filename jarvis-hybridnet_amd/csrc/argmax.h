// The selection orders of the small kernels, once (device code only): "largest value, lowest index
// among equals" as a compare, as an LDS tree and as a 64-bit key with its wave and block reductions; the key of the
// two-view consensus; and the reference's column / row of a flat heat-map index.  Users: centers.hip, views2d.hip,
// softargmax.hip, subjects.hip, joints3d.hip, tracks.hip.
#pragma once
#include "jh_common.h"

namespace jh {

// ------------------------------------------------------------------ the order as a compare
// (value descending, index ascending): total on non-NaN values; NaN never wins
__device__ __forceinline__ void argmax_take(float v, int i, float& best, int& bi) {
  if (v > best || (v == best && i < bi)) { best = v; bi = i; }
}

// The same order over the NT threads of a block through LDS (sv, si: NT slots each); the result is sv[0], si[0], after
// the last barrier.  (The partner's pair is loaded into locals and compared against the thread's own slot.)
template <int NT>
__device__ __forceinline__ void block_argmax(float* sv, int* si, float best, int bi) {
  sv[threadIdx.x] = best; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const float v = sv[threadIdx.x + s];
      const int ii = si[threadIdx.x + s];
      if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && ii < si[threadIdx.x])) {
        sv[threadIdx.x] = v; si[threadIdx.x] = ii;
      }
    }
    __syncthreads();
  }
}

// Column and row of the flat index m of an Hh x Wh map, the reference's expression:
//   preds = (m % shape[2], m // shape[3])   jarvis3D.py:151 (jarvis2D.py:139-149 alike)
// -- the modulus by the HEIGHT.  The maps of the networks are square, where it is the usual (m % Wh, m / Wh).
// (center_argmax_kernel spells the two expressions out between its stores.)
__device__ __forceinline__ void heat_xy(int m, int Hh, int Wh, int* x, int* y) {
  *x = m % Hh;
  *y = m / Wh;
}

// ------------------------------------------------------------------ the order as a 64-bit key
// (order-preserving map of the float's bits) << 32 | (0xFFFFFFFF - p): the maximum key is the largest value and, among
// equal values, the LOWEST index p.  Two keys, because their users define "equal" differently:
//   order_key  orders the bit patterns: -0 lies below +0, and a NaN is not treated specially (it sorts by its bits,
//              above +inf with a clear sign bit).  The soft-argmax spread relies on it: its peak is the arg-max of the
//              V2V network's raw output, which may be negative, and no real key is 0, the start value of its maximum.
//   peak_key   is the order of argmax_take: -0 folded onto +0 (the two compare equal, so the lower index wins) and 0
//              for NaN, below every real key -- NaN never wins.  The centre peaks rely on it: their maps come from a
//              caller, and slot 0 of the peaks must be the pixel center_argmax_kernel picks.
__device__ __forceinline__ unsigned long long order_key(float x, unsigned p) {
  const unsigned u = __float_as_uint(x);
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)k << 32) | (unsigned long long)(0xFFFFFFFFu - p);
}
__device__ __forceinline__ unsigned long long peak_key(float v, unsigned p) {
  return v != v ? 0ull : order_key(v == 0.f ? 0.f : v, p);
}
// the index p of either key
__device__ __forceinline__ unsigned key_index(unsigned long long k) {
  return 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
}

__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) {
  return a > b ? a : b;
}
// maximum / minimum of k over the 64 lanes of a wave (xor shuffles: every lane gets it)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = max_u64(k, (unsigned long long)__shfl_xor((long long)k, o));
  return k;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)k, o);
    k = k < other ? k : other;
  }
  return k;
}
// maximum of k over the block; every thread calls it and gets it.  red: one slot per wave.
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long k, unsigned long long* red) {
  k = wave_max_u64(k);
  const int nw = blockDim.x >> 6;
  __syncthreads();                              // (the slots of the previous call have been read)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
  __syncthreads();
  unsigned long long m = red[0];
  for (int i = 1; i < nw; ++i) m = max_u64(m, red[i]);
  return m;
}

// ------------------------------------------------------------------ the key of the two-view consensus
// views << 50 | ~bits(cost) << 18 | ~index  -- 14 / 32 / 18 bits -- whose maximum is the choice of the subject
// association (subjects.hip) and of the joint triangulation (joints3d.hip): most supporting views, then the smallest
// cost, then the lowest index of the hypothesis.  The cost is a sum of non-negative floats, never NaN: the bit pattern
// of a non-negative float (sign clear, exponent above mantissa) orders as the float does, so its complement orders the
// other way round.  Distinct hypotheses have distinct indices (below 2^18: at most 64 * 8 slots squared), so the order
// is total and a maximum over it does not depend on timing.  0 is below every real key: "no hypothesis".
__device__ __forceinline__ unsigned long long consensus_key(int views, float cost, int index) {
  return ((unsigned long long)views << 50) | ((unsigned long long)(~__float_as_uint(cost)) << 18) |
         (unsigned long long)(0x3FFFF - index);
}
__device__ __forceinline__ int consensus_views(unsigned long long k) { return (int)(k >> 50); }
__device__ __forceinline__ int consensus_index(unsigned long long k) { return 0x3FFFF - (int)(k & 0x3FFFF); }

}  // namespace jh
