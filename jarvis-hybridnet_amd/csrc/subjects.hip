// Several subjects in one frame set (csrc/subjects.h).
//
//  center_peaks        the top-P local maxima of a centre heat map, and
//  associate_subjects  their grouping across cameras into up to K triangulated subjects (new design: the reference
//                      keeps one maximum per camera, jarvis3D.py:147-160)
#include "jh_common.h"
#include "argmax.h"
#include "dlt.h"
#include "subjects.h"

namespace jh {

// ------------------------------------------------- several subjects: peaks of a map
// Top-P local maxima of channel 0 of heat [N][Hh][Wh][Cp] (include/jarvis_hip.h, jh_op_center_peaks).  Pixel p (flat
// index y * Wh + x) is a peak iff v(p) > min_peak and it is the maximum of the total order (value descending, index
// ascending) over its (2r+1)^2 window clipped at the map's edge; NaN takes no part.  The order is carried by ONE 64-bit
// key, peak_key (argmax.h): -0 folded onto +0 (the two compare equal, as in center_argmax_kernel) and 0 for NaN, below
// every real key.
// One 1024-thread workgroup per image.  LDS form: the channel is read from HBM once -- consecutive lanes take
// consecutive pixels, eight loads in flight per thread as in center_argmax_kernel; the Cp - 1 other channels share its
// cache lines, so the lines that arrive are the lines any load shape would fetch -- and kept as fp32 [P]; the window
// maximum is separable: bx [P] (16 bit) holds the column of the maximum of the row window [x-r, x+r], the column pass
// takes the maximum over the rows y-r .. y+r of those; 6 bytes per pixel plus the peak mask, so 160 x 160 fits the
// 160 KB.  A wave votes its 64 pixels into one mask word (__ballot).  The top P are P block maxima of the key over the
// set mask bits (wave shuffles, then one LDS slot per wave); the winner's bit is cleared.
// Global form (a map that does not fit): the same passes with the values read from `heat` and bx / mask in `ws`.
constexpr int kPeakThreads = 1024;
constexpr size_t kPeakLdsBytes = 160 * 1024 - 512;           // (the block maxima's slots are static LDS)

__host__ __device__ inline size_t peak_mask_words(int P) { return ((size_t)P + 63) >> 6; }
// bytes of one image's global-form scratch: mask words, then bx
__host__ __device__ inline size_t peak_ws_image(int P) {
  return (peak_mask_words(P) * 8 + (size_t)P * 2 + 255) / 256 * 256;
}

template <bool LDS>
__global__ __launch_bounds__(kPeakThreads) void center_peaks_kernel(
    const float* __restrict__ heat, float* __restrict__ peaks, int* __restrict__ count,
    unsigned char* __restrict__ ws, int Hh, int Wh, int Cp, int maxp, int r, float min_peak) {
  extern __shared__ __attribute__((aligned(16))) unsigned char peak_smem[];
  __shared__ unsigned long long red[kPeakThreads / 64];
  const int n = blockIdx.x, tid = threadIdx.x, P = Hh * Wh, words = (int)peak_mask_words(P);
  const float* h = heat + (size_t)n * P * Cp;
  unsigned long long* mask;
  unsigned short* bx;
  [[maybe_unused]] float* lv = nullptr;
  if constexpr (LDS) {
    mask = reinterpret_cast<unsigned long long*>(peak_smem);
    lv = reinterpret_cast<float*>(mask + words);
    bx = reinterpret_cast<unsigned short*>(lv + P);
    constexpr int U = 8;
    int p = tid;
    for (; p + (U - 1) * kPeakThreads < P; p += U * kPeakThreads) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = h[(size_t)(p + u * kPeakThreads) * Cp];
#pragma unroll
      for (int u = 0; u < U; ++u) lv[p + u * kPeakThreads] = v[u];
    }
    for (; p < P; p += kPeakThreads) lv[p] = h[(size_t)p * Cp];
    __syncthreads();
  } else {
    unsigned char* w = ws + (size_t)n * peak_ws_image(P);
    mask = reinterpret_cast<unsigned long long*>(w);
    bx = reinterpret_cast<unsigned short*>(mask + words);
  }
  auto val = [&](int p) -> float {
    if constexpr (LDS) return lv[p]; else return h[(size_t)p * Cp];
  };
  // rows: the column of the best pixel of [x-r, x+r]; 0xFFFF: the window holds NaN only
  for (int p = tid; p < P; p += kPeakThreads) {
    const int y = p / Wh, x = p - y * Wh;
    const int x0 = max(0, x - r), x1 = min(Wh - 1, x + r);
    unsigned long long best = 0;
    int bestx = 0xFFFF;
    for (int xx = x0; xx <= x1; ++xx) {
      const int q = y * Wh + xx;
      const unsigned long long k = peak_key(val(q), (unsigned)q);
      if (k > best) { best = k; bestx = xx; }
    }
    bx[p] = (unsigned short)bestx;
  }
  if constexpr (!LDS) __threadfence_block();
  __syncthreads();
  // columns: p is a peak iff it is the best of the row maxima of y-r .. y+r; one mask word per wave
  for (int base = 0; base < words * 64; base += kPeakThreads) {
    const int p = base + tid;
    bool pk = false;
    if (p < P) {
      const float v = val(p);
      if (v > min_peak) {                       // (NaN compares false)
        const int y = p / Wh, x = p - y * Wh;
        const int y0 = max(0, y - r), y1 = min(Hh - 1, y + r);
        unsigned long long best = 0;
        for (int yy = y0; yy <= y1; ++yy) {
          const int b = bx[yy * Wh + x];
          if (b == 0xFFFF) continue;
          const int q = yy * Wh + b;
          best = max_u64(best, peak_key(val(q), (unsigned)q));
        }
        pk = best == peak_key(v, (unsigned)p);
      }
    }
    const unsigned long long vote = __ballot(pk);
    if ((tid & 63) == 0 && (p >> 6) < words) mask[p >> 6] = vote;
  }
  if constexpr (!LDS) __threadfence_block();
  __syncthreads();
  float* out = peaks + (size_t)n * maxp * 3;
  int found = 0;
  for (; found < maxp; ++found) {
    unsigned long long best = 0;
    for (int w = tid; w < words; w += kPeakThreads) {
      unsigned long long m = mask[w];
      while (m) {
        const int p = w * 64 + __ffsll((long long)m) - 1;
        m &= m - 1;
        best = max_u64(best, peak_key(val(p), (unsigned)p));
      }
    }
    const unsigned long long win = block_max_u64(best, red);
    if (win == 0) break;                        // (uniform: every thread holds the same maximum)
    if (tid == 0) {
      const int m = (int)key_index(win);
      int x, y;
      heat_xy(m, Hh, Wh, &x, &y);               // (the expression of center_argmax_kernel)
      out[found * 3 + 0] = (float)x;
      out[found * 3 + 1] = (float)y;
      out[found * 3 + 2] = val(m);
      mask[m >> 6] &= ~(1ull << (m & 63));
    }
    if constexpr (!LDS) __threadfence_block();
    __syncthreads();
  }
  if (tid == 0) {
    for (int k = found; k < maxp; ++k) {
      out[k * 3 + 0] = -1.f; out[k * 3 + 1] = -1.f; out[k * 3 + 2] = -INFINITY;
    }
    count[n] = found;
  }
}

int subjects_check(const SubjectsParams& p) {
  JH_REQUIRE(p.max_subjects >= 1 && p.max_subjects <= kMaxSubjects, "jh_subjects_params: max_subjects must be 1 .. 8");
  JH_REQUIRE(p.max_peaks >= 1 && p.max_peaks <= kMaxPeaks, "jh_subjects_params: max_peaks must be 1 .. 8");
  JH_REQUIRE(p.nms_radius >= 1 && p.nms_radius <= kMaxNmsRadius, "jh_subjects_params: nms_radius must be 1 .. 16");
  JH_REQUIRE(p.min_views >= 2, "jh_subjects_params: min_views must be at least 2");
  JH_REQUIRE(p.min_peak == p.min_peak && p.min_peak < INFINITY, "jh_subjects_params: min_peak must be a number below "
             "+inf (-inf allowed)");
  JH_REQUIRE(p.max_error_px >= 0.f, "jh_subjects_params: max_error_px must be >= 0 (+inf allowed)");
  return 0;
}

static bool peaks_fit_lds(int P) { return peak_mask_words(P) * 8 + (size_t)P * 6 <= kPeakLdsBytes; }

size_t center_peaks_workspace(int N, int Hh, int Wh) {
  const int P = Hh * Wh;
  return peaks_fit_lds(P) ? 0 : (size_t)N * peak_ws_image(P);
}

int launch_center_peaks(const float* heat, float* peaks, int* count, int N, int Hh, int Wh, int Cp, int max_peaks,
                        int nms_radius, float min_peak, void* workspace, hipStream_t s) {
  JH_REQUIRE(N >= 1 && Hh >= 1 && Wh >= 1 && Cp >= 1, "centre peaks: heat map shape");
  JH_REQUIRE(Hh <= 32768 && Wh <= 32768 && (long long)Hh * Wh < (1ll << 30), "centre peaks: heat map too large");
  JH_REQUIRE(max_peaks >= 1 && max_peaks <= kMaxPeaks && nms_radius >= 1 && nms_radius <= kMaxNmsRadius,
             "centre peaks: max_peaks 1 .. 8, nms_radius 1 .. 16");
  JH_REQUIRE(min_peak == min_peak, "centre peaks: min_peak is NaN");
  const int P = Hh * Wh;
  if (peaks_fit_lds(P)) {
    const size_t lds = peak_mask_words(P) * 8 + (size_t)P * 6;
    static bool big = false;
    if (lds > 64 * 1024 && !big) {
      // (dynamic + static LDS together stay within the 160 KB: the static slots of block_max_u64 come off the top)
      JH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(center_peaks_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPeakLdsBytes));
      big = true;
    }
    hipLaunchKernelGGL(center_peaks_kernel<true>, dim3(N), dim3(kPeakThreads), lds, s, heat, peaks, count,
                       (unsigned char*)nullptr, Hh, Wh, Cp, max_peaks, nms_radius, min_peak);
  } else {
    JH_REQUIRE(workspace, "centre peaks: a map that does not fit the LDS needs its workspace");
    hipLaunchKernelGGL(center_peaks_kernel<false>, dim3(N), dim3(kPeakThreads), 0, s, heat, peaks, count,
                       static_cast<unsigned char*>(workspace), Hh, Wh, Cp, max_peaks, nms_radius, min_peak);
  }
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------- several subjects: association across cameras
// Peaks [T][C][P][3] of a frame set -> up to K subjects (include/jarvis_hip.h, jh_op_associate_subjects).  One
// 256-thread workgroup per frame set.  Staged once in LDS: the calibration rows of the frame set, and for every usable
// slot (camera unmasked, x >= 0 and y >= 0: an empty slot is (-1, -1, -inf), a masked camera's may be NaN and is not
// read) its two DLT rows (dlt_rows: the triangulation's) and its pixel (x * sx2, y * sy2).
// A round walks the pairs (ai, bj) of slots of two cameras a < b, a thread a pair at a time: the two-view DLT point, its
// support (per camera the nearest unused peak to project_one of the point, supporting iff the depth is positive and the
// distance is <= max_err), and consensus_key (argmax.h) of the views, the cost and the pair's index, whose maximum is
// the choice: most views, then the smallest cost, then the lowest (a, i, b, j).
// The block maximum is a total order on distinct indices, so the choice does not depend on timing.  Thread 0 then
// evaluates the winner again for its members, triangulates them -- A^T A summed in camera order, a non-member's term
// selected as an exact 0.0 like a masked camera's in triangulate_body: the bits of the triangulation of the members
// alone --, and marks their slots used.  The work of a round grows with (C * P)^2: meant for C * P up to a few hundred.
constexpr int kAssocThreads = 256, kAssocSlots = 64 * kMaxPeaks;

struct AssocShared {
  float rows[kAssocSlots][8];                   // r0[4], r1[4] of every slot
  float px[kAssocSlots], py[kAssocSlots];
  unsigned char state[kAssocSlots];             // 0 absent / masked, 1 unused, 2 used
  float M[64 * 12], K[64 * 9], D[64 * 5];
  int member[64];
  unsigned long long red[kAssocThreads / 64];
};

// support of the point X among the unused peaks: views and cost; member (nullable): the supporting slot per camera or -1
__device__ __forceinline__ void assoc_support(const AssocShared& sh, const float* X, int C, int P, float max_err,
                                              int* views, float* cost, int* member) {
  int n = 0;
  float sum = 0.f;
  for (int c = 0; c < C; ++c) {
    int bests = -1;
    float bestd = 0.f, u = 0.f, v = 0.f, depth = 0.f;
    bool projected = false;
    for (int sl = 0; sl < P; ++sl) {
      if (sh.state[c * P + sl] != 1) continue;
      if (!projected) {
        project_one(sh.M + c * 12, sh.K + c * 9, sh.D + c * 5, X[0], X[1], X[2], &u, &v, &depth);
        projected = true;
      }
      const float d = pixel_distance(u, v, sh.px[c * P + sl], sh.py[c * P + sl]);
      if (d == d && (bests < 0 || d < bestd)) { bests = sl; bestd = d; }   // (ties: the lowest slot; NaN: never)
    }
    const bool ok = bests >= 0 && depth > 0.f && bestd <= max_err;
    if (ok) { ++n; sum = __fadd_rn(sum, bestd); }
    if (member) member[c] = ok ? bests : -1;
  }
  *views = n;
  *cost = sum;
}

__global__ __launch_bounds__(kAssocThreads) void associate_subjects_kernel(
    const float* __restrict__ peaks, const float* __restrict__ cam, const float* __restrict__ intr,
    const float* __restrict__ dist, int fs, const unsigned char* __restrict__ mask, float* __restrict__ centers,
    int* __restrict__ views_out, int* __restrict__ members, float* __restrict__ error, int C, int P, int K,
    int min_views, float max_err, float sx2, float sy2, float wdiv) {
  __shared__ AssocShared sh;
  const int t = blockIdx.x, tid = threadIdx.x, CP = C * P;
  const size_t row0 = (size_t)t * fs;           // (fs: the calibration's frame stride, see triangulate_body)
  for (int i = tid; i < C * 12; i += kAssocThreads) sh.M[i] = cam[row0 * 12 + i];
  for (int i = tid; i < C * 9; i += kAssocThreads) sh.K[i] = intr[row0 * 9 + i];
  for (int i = tid; i < C * 5; i += kAssocThreads) sh.D[i] = dist[row0 * 5 + i];
  __syncthreads();
  for (int i = tid; i < CP; i += kAssocThreads) {
    const int c = i / P;
    unsigned char st = 0;
    if (!mask || mask[(size_t)t * C + c] != 0) {
      const float* d = peaks + ((size_t)t * CP + i) * 3;
      if (d[0] >= 0.f && d[1] >= 0.f) {         // (NaN compares false)
        dlt_rows(d, sh.M + c * 12, sh.K + c * 9, sh.D[c * 5 + 0], sh.D[c * 5 + 1], sx2, sy2, wdiv, sh.rows[i],
                 sh.rows[i] + 4);
        sh.px[i] = __fmul_rn(d[0], sx2);
        sh.py[i] = __fmul_rn(d[1], sy2);
        st = 1;
      }
    }
    sh.state[i] = st;
  }
  __syncthreads();
  const float nan = __int_as_float(0x7fc00000);
  int k = 0;
  for (; k < K; ++k) {
    unsigned long long best = 0;
    for (int idx = tid; idx < CP * CP; idx += kAssocThreads) {
      const int ai = idx / CP, bj = idx - ai * CP;
      if (ai / P >= bj / P || sh.state[ai] != 1 || sh.state[bj] != 1) continue;
      float X[3], cost;
      int nv;
      dlt_pair_point(sh.rows[ai], sh.rows[bj], X);  // (ai < bj: the cameras in order)
      assoc_support(sh, X, C, P, max_err, &nv, &cost, nullptr);
      best = max_u64(best, consensus_key(nv, cost, idx));
    }
    const unsigned long long win = block_max_u64(best, sh.red);
    if (consensus_views(win) < min_views) break;  // (uniform; also "no pair left": win == 0)
    if (tid == 0) {
      const int idx = consensus_index(win), ai = idx / CP, bj = idx - ai * CP;
      float X[3], cost, ctr[3];
      int nv;
      dlt_pair_point(sh.rows[ai], sh.rows[bj], X);
      assoc_support(sh, X, C, P, max_err, &nv, &cost, sh.member);
      // (the fallback row is slot 0: a non-member's term is evaluated, then selected away)
      dlt_members_point(sh.rows, C, 0, [&](int c) { return sh.member[c] >= 0 ? c * P + sh.member[c] : -1; }, ctr);
      float esum = 0.f;
      for (int c = 0; c < C; ++c) {
        members[((size_t)t * K + k) * C + c] = sh.member[c];
        if (sh.member[c] < 0) continue;
        const int sl = c * P + sh.member[c];
        float u, v;
        project_one(sh.M + c * 12, sh.K + c * 9, sh.D + c * 5, ctr[0], ctr[1], ctr[2], &u, &v);
        esum = __fadd_rn(esum, pixel_distance(u, v, sh.px[sl], sh.py[sl]));
        sh.state[sl] = 2;
      }
      for (int a = 0; a < 3; ++a) centers[((size_t)t * K + k) * 3 + a] = ctr[a];
      views_out[(size_t)t * K + k] = nv;
      error[(size_t)t * K + k] = __fdiv_rn(esum, (float)nv);
    }
    __syncthreads();
  }
  // the subjects that were not found
  for (int i = tid; i < (K - k) * C; i += kAssocThreads) members[((size_t)t * K + k) * C + i] = -1;
  for (int i = tid; i < (K - k) * 3; i += kAssocThreads) centers[((size_t)t * K + k) * 3 + i] = nan;
  for (int i = tid; i < K - k; i += kAssocThreads) {
    views_out[(size_t)t * K + k + i] = 0;
    error[(size_t)t * K + k + i] = nan;
  }
}

int launch_associate_subjects(const float* peaks, const Calib& cal, const unsigned char* mask, float* centers,
                              int* views, int* members, float* error, int T, int C, int P, int K, int min_views,
                              float max_error_px, float sx2, float sy2, float wdiv, hipStream_t s) {
  JH_REQUIRE(T >= 1 && C >= 1 && C <= 64, "subject association: at most 64 cameras");
  JH_REQUIRE(P >= 1 && P <= kMaxPeaks && K >= 1 && K <= kMaxSubjects && min_views >= 2 && max_error_px >= 0.f,
             "subject association: max_peaks 1 .. 8, max_subjects 1 .. 8, min_views >= 2, max_error_px >= 0");
  if (calib_check(cal, C)) return 1;
  hipLaunchKernelGGL(associate_subjects_kernel, dim3(T), dim3(kAssocThreads), 0, s, peaks, cal.cam, cal.intr, cal.dist,
                     cal.fs, mask, centers, views, members, error, C, P, K, min_views, max_error_px, sx2, sy2, wdiv);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
