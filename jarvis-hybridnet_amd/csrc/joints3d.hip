// Per-joint robust triangulation from the cameras' 2D keypoints (csrc/joints3d.h; the definition: include/jarvis_hip.h,
// jh_joints3d_params).  Two kernels behind the all-joint arg-max scan (views2d.hip, launch_joint_argmax_all):
//   joint_observations_kernel / joint_peaks_refine_kernel   the observation (u, v, w) of every (frame set, camera,
//       joint): views2d's pixel and confidence, the pixel moved by the centroid of the (2r+1)^2 window around the peak
//   joints3d_kernel   the consensus over two-view triangulations and the triangulation of its members
// The DLT and the projection are those of the triangulation (csrc/dlt.h), the merge of the scan's slices that of the 2D
// views (csrc/views2d.h): one definition each, the same bits.
#include "jh_common.h"
#include "argmax.h"
#include "dlt.h"
#include "views2d.h"
#include "joints3d.h"

namespace jh {

// ------------------------------------------------------------- sub-pixel offset
// Centroid of max(h, 0) over the window |x - mx| <= r, |y - my| <= r of channel j, clipped at the map's edge and walked
// y ascending, then x ascending; every product and sum rounded once in fp32, in walk order (a NaN pixel counts as 0:
// fmaxf returns the other operand).  img: pixel (0, 0) of the image, channel j; rows of Wh pixels, Hh of them, Jp floats
// per pixel.  At most (2r+1)^2 loads at stride Jp.  A non-positive window gives (0, 0).
__device__ __forceinline__ void refine_offset(const float* __restrict__ img, int Hh, int Wh, int Jp, int mx, int my,
                                              int r, float* ox, float* oy) {
  const int x0 = max(0, mx - r), x1 = min(Wh - 1, mx + r);
  const int y0 = max(0, my - r), y1 = min(Hh - 1, my + r);
  float s0 = 0.f, sx = 0.f, sy = 0.f;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      const float wgt = fmaxf(img[((size_t)y * Wh + x) * Jp], 0.f);
      s0 = __fadd_rn(s0, wgt);
      sx = __fadd_rn(sx, __fmul_rn(wgt, (float)(x - mx)));
      sy = __fadd_rn(sy, __fmul_rn(wgt, (float)(y - my)));
    }
  const bool pos = s0 > 0.f;
  *ox = pos ? __fdiv_rn(sx, s0) : 0.f;
  *oy = pos ? __fdiv_rn(sy, s0) : 0.f;
}

// The stand-alone operator (jh_op_joint_peaks_refine): block = image, thread = joint; x = m % Wh, y = m / Wh.  An index
// outside the map reads nothing and gives (0, 0).
__global__ void joint_peaks_refine_kernel(const float* __restrict__ heat, const int* __restrict__ idx,
                                          float* __restrict__ offsets, int Hh, int Wh, int J, int Jp, int r) {
  const int n = blockIdx.x, j = threadIdx.x;
  if (j >= J) return;
  const size_t o = (size_t)n * J + j;
  const int m = idx[o], P = Hh * Wh;
  float ox = 0.f, oy = 0.f;
  if (m >= 0 && m < P) refine_offset(heat + (size_t)n * P * Jp + j, Hh, Wh, Jp, m % Wh, m / Wh, r, &ox, &oy);
  offsets[o * 2 + 0] = ox;
  offsets[o * 2 + 1] = oy;
}

// The predictor's form: block = (frame set t, camera c), thread = joint, as views2d_final_kernel -- whose expressions
// for `used`, the peak's column and row, the full-frame pixel and the confidence these are.  Nothing of an unused
// camera's partials or heat map is read.  A map without any number (the scan's index stays at its start value) is not
// refined; its weight is not positive, so the observation is not usable whatever its pixel.
__global__ void joint_observations_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx,
                                          const float* __restrict__ heat, const int* __restrict__ center_hm,
                                          const int* __restrict__ valid, const unsigned char* __restrict__ mask,
                                          float* __restrict__ obs, int C, int J, int Jp, int slices, int Hh, int hw,
                                          int r) {
  const int n = blockIdx.x, t = n / C, c = n % C, j = threadIdx.x;
  if (j >= J) return;
  float* out = obs + ((size_t)n * J + j) * 3;
  const bool use = valid[t] != 0 && (mask == nullptr || mask[(size_t)t * C + c] != 0);
  if (!use) {
    const float nan = __int_as_float(0x7fc00000);
    out[0] = nan;
    out[1] = nan;
    out[2] = 0.f;
    return;
  }
  float b;
  int m;
  argmax_combine(pmax, pidx, n, slices, Jp, j, &b, &m);
  const int P = Hh * Hh;
  int mx, my;
  heat_xy(m, Hh, Hh, &mx, &my);
  const int x = mx * 2 + center_hm[(size_t)n * 2 + 0] - hw;
  const int y = my * 2 + center_hm[(size_t)n * 2 + 1] - hw;
  float ox = 0.f, oy = 0.f;
  if (r > 0 && m >= 0 && m < P) refine_offset(heat + (size_t)n * P * Jp + j, Hh, Hh, Jp, mx, my, r, &ox, &oy);
  out[0] = __fadd_rn((float)x, __fmul_rn(2.f, ox));
  out[1] = __fadd_rn((float)y, __fmul_rn(2.f, oy));
  out[2] = __fdiv_rn(fminf(b, 255.f), 255.f);
}

// ------------------------------------------------------------------- consensus
// One 64-lane wave per (frame set t, joint j), four waves per workgroup; a wave past the last (t, j) only keeps the
// barriers company.  Each wave stages, in its own part of the LDS, the calibration rows of its frame set and, lane =
// camera, the two DLT rows (dlt_rows: the triangulation's, the pixel as given, weight w) and the pixel of every usable
// observation (w > 0, w >= min_conf, finite pixel; an unused camera's row is (NaN, NaN, 0)).
// The C (C - 1) / 2 pairs a < b of cameras are strided over the lanes: the two-view DLT point, its support (a usable
// camera supports iff the point lies in front of it and projects within max_err of its pixel; NaN never does), and
// consensus_key (argmax.h) of the views, the cost and a * C + b, whose maximum is the choice: most views, then the
// smallest cost, then the lowest (a, b).  The key is a total order on distinct pairs and the wave maximum
// (wave_max_u64) is exact, so the choice does not depend on timing.  Lane 0 then
// evaluates the winner again for its members and triangulates them -- A^T A summed in camera order, a non-member's term
// selected as an exact 0.0 like a masked camera's in triangulate_body: the bits of the triangulation of the members
// alone.  The eigen-solves run in fp64, one per pair and lane: at C = 12 two per lane, then two on lane 0.
constexpr int kJ3Waves = 4;

struct J3Wave {
  float M[64 * 12], K[64 * 9], D[64 * 5];
  float rows[64][8];                            // r0[4], r1[4] of every camera
  float px[64], py[64];
  unsigned char usable[64];
  unsigned char member[64];
};

// support of the point X: views and cost; member (nullable): 1 per supporting camera
__device__ __forceinline__ void j3_support(const J3Wave& w, const float* X, int C, float max_err, int* views,
                                           float* cost, unsigned char* member) {
  int n = 0;
  float sum = 0.f;
  for (int c = 0; c < C; ++c) {
    bool ok = false;
    float d = 0.f;
    if (w.usable[c]) {
      float u, v, depth;
      project_one(w.M + c * 12, w.K + c * 9, w.D + c * 5, X[0], X[1], X[2], &u, &v, &depth);
      d = pixel_distance(u, v, w.px[c], w.py[c]);
      ok = depth > 0.f && d <= max_err;         // (NaN compares false)
    }
    if (ok) { ++n; sum = __fadd_rn(sum, d); }
    if (member) member[c] = ok ? 1 : 0;
  }
  *views = n;
  *cost = sum;
}

__global__ __launch_bounds__(kJ3Waves * 64) void joints3d_kernel(
    const float* __restrict__ obs, const float* __restrict__ cam, const float* __restrict__ intr,
    const float* __restrict__ dist, int fs, float* __restrict__ points, int* __restrict__ views_out,
    unsigned char* __restrict__ members, float* __restrict__ error, int TJ, int C, int J, int min_views,
    float min_conf, float max_err) {
  __shared__ J3Wave sh[kJ3Waves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tj = blockIdx.x * kJ3Waves + wave;
  const bool live = tj < TJ;                    // (wave-uniform)
  const int t = live ? tj / J : 0, j = live ? tj - t * J : 0;
  J3Wave& w = sh[wave];
  if (live) {
    const size_t row0 = (size_t)t * fs;         // (fs: the calibration's frame stride, see triangulate_body)
    for (int i = lane; i < C * 12; i += 64) w.M[i] = cam[row0 * 12 + i];
    for (int i = lane; i < C * 9; i += 64) w.K[i] = intr[row0 * 9 + i];
    for (int i = lane; i < C * 5; i += 64) w.D[i] = dist[row0 * 5 + i];
  }
  __syncthreads();
  if (live && lane < C) {
    const int c = lane;
    const float* o = obs + (((size_t)t * C + c) * J + j) * 3;
    const float d[3] = {o[0], o[1], o[2]};
    // (NaN compares false everywhere)
    const bool ok = d[2] > 0.f && d[2] >= min_conf && fabsf(d[0]) < INFINITY && fabsf(d[1]) < INFINITY;
    if (ok) {
      dlt_rows(d, w.M + c * 12, w.K + c * 9, w.D[c * 5 + 0], w.D[c * 5 + 1], 1.f, 1.f, 1.f, w.rows[c], w.rows[c] + 4);
      w.px[c] = d[0];
      w.py[c] = d[1];
    }
    w.usable[c] = ok ? 1 : 0;
  }
  __syncthreads();
  unsigned long long best = 0;
  if (live) {
    const int npairs = C * (C - 1) / 2;
    for (int p = lane; p < npairs; p += 64) {
      int a = 0, rest = p;                      // pair number -> (a, b): row a of the triangle holds C - 1 - a pairs
      while (rest >= C - 1 - a) { rest -= C - 1 - a; ++a; }
      const int b = a + 1 + rest;
      if (!w.usable[a] || !w.usable[b]) continue;
      float X[3], cost;
      int nv;
      dlt_pair_point(w.rows[a], w.rows[b], X);    // (a < b: the cameras in order)
      j3_support(w, X, C, max_err, &nv, &cost, nullptr);
      best = max_u64(best, consensus_key(nv, cost, a * C + b));
    }
  }
  best = wave_max_u64(best);
  if (!live || lane != 0) return;
  const size_t o = (size_t)t * J + j;
  if (consensus_views(best) < min_views) {      // (also "no pair": best == 0)
    const float nan = __int_as_float(0x7fc00000);
    for (int a = 0; a < 3; ++a) points[o * 3 + a] = nan;
    views_out[o] = 0;
    error[o] = nan;
    for (int c = 0; c < C; ++c) members[o * C + c] = 0;
    return;
  }
  const int idx = consensus_index(best), a = idx / C, b = idx - a * C;
  float X[3], cost, pt[3];
  int nv;
  dlt_pair_point(w.rows[a], w.rows[b], X);
  j3_support(w, X, C, max_err, &nv, &cost, w.member);
  // (the fallback row is camera a's: a non-member's rows may never have been written)
  dlt_members_point(w.rows, C, a, [&](int c) { return w.member[c] ? c : -1; }, pt);
  float esum = 0.f;
  for (int c = 0; c < C; ++c) {
    members[o * C + c] = w.member[c];
    if (!w.member[c]) continue;
    float u, v;
    project_one(w.M + c * 12, w.K + c * 9, w.D + c * 5, pt[0], pt[1], pt[2], &u, &v);
    esum = __fadd_rn(esum, pixel_distance(u, v, w.px[c], w.py[c]));
  }
  for (int k = 0; k < 3; ++k) points[o * 3 + k] = pt[k];
  views_out[o] = nv;
  error[o] = __fdiv_rn(esum, (float)nv);
}

// ------------------------------------------------------------------- host side
int joints3d_check(const Joints3dParams& p) {
  JH_REQUIRE(p.min_views >= 2, "jh_joints3d_params: min_views must be at least 2");
  JH_REQUIRE(p.refine_radius >= 0 && p.refine_radius <= kMaxRefineRadius,
             "jh_joints3d_params: refine_radius must be 0 .. 3");
  JH_REQUIRE(p.min_conf >= 0.f && p.min_conf <= 1.f, "jh_joints3d_params: min_conf must be 0 .. 1");
  JH_REQUIRE(p.max_error_px >= 0.f, "jh_joints3d_params: max_error_px must be >= 0 (+inf allowed)");
  return 0;
}

static int check_maps(int N, int Hh, int Wh, int J, int Jp, int radius) {
  JH_REQUIRE(N >= 1 && Hh >= 1 && Wh >= 1 && (long long)Hh * Wh < (1ll << 30), "joint peaks: heat map shape");
  JH_REQUIRE(J >= 1 && J <= Jp && Jp <= 1024, "joint peaks: channel count");
  JH_REQUIRE(radius >= 0 && radius <= kMaxRefineRadius, "joint peaks: refine radius 0 .. 3");
  return 0;
}

int launch_joint_peaks_refine(const float* heat, const int* idx, float* offsets, int N, int Hh, int Wh, int J, int Jp,
                              int radius, hipStream_t s) {
  if (check_maps(N, Hh, Wh, J, Jp, radius)) return 1;
  hipLaunchKernelGGL(joint_peaks_refine_kernel, dim3(N), dim3(round_up(J, kWave)), 0, s, heat, idx, offsets, Hh, Wh, J,
                     Jp, radius);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_joint_observations(const float* pmax, const int* pidx, const float* heat, const int* center_hm,
                              const int* valid, const unsigned char* mask, float* obs, int T, int C, int J, int Jp,
                              int Hh, int hw, int radius, hipStream_t s) {
  if (check_maps(T * C, Hh, Hh, J, Jp, radius)) return 1;
  const ScanShape sh = joint_argmax_all_shape(T * C, Hh, Hh, Jp);
  hipLaunchKernelGGL(joint_observations_kernel, dim3(T * C), dim3(round_up(J, kWave)), 0, s, pmax, pidx, heat,
                     center_hm, valid, mask, obs, C, J, Jp, sh.slices, Hh, hw, radius);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_joints3d(const float* obs, const Calib& cal, float* points, int* views, unsigned char* members,
                    float* error, int T, int C, int J, int min_views, float min_conf, float max_error_px,
                    hipStream_t s) {
  JH_REQUIRE(T >= 1 && J >= 1, "joint triangulation: at least one frame set and one joint");
  JH_REQUIRE(C >= 1 && C <= 64, "joint triangulation: 1 .. 64 cameras");
  JH_REQUIRE((long long)T * J < (1ll << 30), "joint triangulation: too many joints");
  JH_REQUIRE(min_views >= 2 && min_conf >= 0.f && max_error_px >= 0.f,
             "joint triangulation: min_views >= 2, min_conf >= 0, max_error_px >= 0");
  if (calib_check(cal, C)) return 1;
  const int TJ = T * J;
  hipLaunchKernelGGL(joints3d_kernel, dim3((TJ + kJ3Waves - 1) / kJ3Waves), dim3(kJ3Waves * 64), 0, s, obs, cal.cam,
                     cal.intr, cal.dist, cal.fs, points, views, members, error, TJ, C, J, min_views, min_conf,
                     max_error_px);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
