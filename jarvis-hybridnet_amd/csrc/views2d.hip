// Arg-max of the keypoint heat maps (csrc/views2d.h).
//
//  joint_argmax        one joint per block: the 2D predictor's keypoints, jarvis2D.py:139-149
//  joint_argmax_all    argmax of every joint's heat map in one pass + the per-camera 2D views of the 3D
//                      predictor (2D keypoints, reprojections, reprojection errors), jarvis2D.py:139-149
#include "jh_common.h"
#include "argmax.h"
#include "dlt.h"
#include "views2d.h"

namespace jh {

// Per-joint argmax of the keypoint heatmaps [T][Hh][Wh][Jp] (jarvis2D.py:139-149):
// points2D = (m % Hh, m // Wh) * 2 + centerHM - hw, confidence = min(max, 255) / 255.
// One block per (joint, image); the lowest index wins among equal maxima.
__global__ __launch_bounds__(256) void joint_argmax_kernel(
    const float* __restrict__ heat, const int* __restrict__ center_hm, int* __restrict__ points,
    float* __restrict__ conf, int J, int Jp, int Hh, int Wh, int hw) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int j = blockIdx.x, t = blockIdx.y;
  const int P = Hh * Wh;
  const float* h = heat + (size_t)t * P * Jp + j;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int p = threadIdx.x; p < P; p += blockDim.x) argmax_take(h[(size_t)p * Jp], p, best, bi);
  block_argmax<256>(sv, si, best, bi);
  if (threadIdx.x == 0) {
    int mx, my;
    heat_xy(si[0], Hh, Wh, &mx, &my);
    points[((size_t)t * J + j) * 2 + 0] = mx * 2 + center_hm[t * 2 + 0] - hw;
    points[((size_t)t * J + j) * 2 + 1] = my * 2 + center_hm[t * 2 + 1] - hw;
    conf[(size_t)t * J + j] = __fdiv_rn(fminf(sv[0], 255.f), 255.f);
  }
}

int launch_joint_argmax(const float* heat, const int* center_hm, int* points, float* conf, int T,
                        int J, int Jp, int Hh, int Wh, int hw, hipStream_t s) {
  hipLaunchKernelGGL(joint_argmax_kernel, dim3(J, T), dim3(256), 0, s, heat, center_hm, points, conf,
                     J, Jp, Hh, Wh, hw);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------- all-joint argmax in one pass
// heat: [N][P = Hh*Wh][Jp] channel-last.  joint_argmax_kernel above reads one float of every Jp-float pixel per
// block and so drags the whole image through the cache J times; this scan reads every byte once.  A thread keeps
// ONE channel quad (16-byte loads) and four running (max, flat index) pairs; the block has rows * q threads
// (q = Jp / 4 quads per pixel, rows = 256 / q pixels per step), so thread tid loads float4 number tid of the step:
// a wave's loads are contiguous, and the quad stays fixed for any q because the step is a multiple of q (252 threads
// for q = 6, 256 for q = 8).  U independent loads per thread are in flight (see center_argmax_kernel).
// An image is split into slices of `ppb` pixels (grid.x): at a time batch of 1 there are only C images.  A block
// writes the (max, index) of its slice per channel to pmax / pidx [N][slices][Jp]; argmax_combine() merges them.
// The order (value descending, index ascending) is total on non-NaN values, so the result does not depend on how
// the pixels are split over threads and slices: the lowest flat index among equal maxima wins, NaN never does.
constexpr int kScanThreads = 256, kScanUnroll = 8;

__global__ __launch_bounds__(kScanThreads) void joint_argmax_all_kernel(
    const float* __restrict__ heat, float* __restrict__ pmax, int* __restrict__ pidx, int P, int Jp, int ppb) {
  __shared__ float sv[kScanThreads * 4];
  __shared__ int si[kScanThreads * 4];
  const int q = Jp >> 2, rows = blockDim.x / q, tid = threadIdx.x;
  const int c4 = tid % q, row = tid / q;
  const int n = blockIdx.y, slice = blockIdx.x;
  const int p0 = slice * ppb, p1 = min(P, p0 + ppb);
  const float4* h = reinterpret_cast<const float4*>(heat + (size_t)n * P * Jp) + c4;
  float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bi[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
  constexpr int U = kScanUnroll;
  int p = p0 + row;
  for (; p + (U - 1) * rows < p1; p += U * rows) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = h[(size_t)(p + u * rows) * q];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int pp = p + u * rows;
      argmax_take(v[u].x, pp, best[0], bi[0]);
      argmax_take(v[u].y, pp, best[1], bi[1]);
      argmax_take(v[u].z, pp, best[2], bi[2]);
      argmax_take(v[u].w, pp, best[3], bi[3]);
    }
  }
  for (; p < p1; p += rows) {
    const float4 v = h[(size_t)p * q];
    argmax_take(v.x, p, best[0], bi[0]);
    argmax_take(v.y, p, best[1], bi[1]);
    argmax_take(v.z, p, best[2], bi[2]);
    argmax_take(v.w, p, best[3], bi[3]);
  }
  // block reduce over the rows: sv / si [row][Jp]; two steps, so that no thread walks all rows alone
  *reinterpret_cast<float4*>(sv + tid * 4) = make_float4(best[0], best[1], best[2], best[3]);
  *reinterpret_cast<int4*>(si + tid * 4) = make_int4(bi[0], bi[1], bi[2], bi[3]);
  __syncthreads();
  const int parts = blockDim.x / Jp, ch = tid % Jp, part = tid / Jp;
  float b = -INFINITY;
  int i = 0x7fffffff;
  if (part < parts)
    for (int r = part; r < rows; r += parts) argmax_take(sv[r * Jp + ch], si[r * Jp + ch], b, i);
  __syncthreads();
  if (part < parts) { sv[tid] = b; si[tid] = i; }
  __syncthreads();
  if (tid < Jp) {
    for (int k = 1; k < parts; ++k) argmax_take(sv[k * Jp + tid], si[k * Jp + tid], b, i);
    const size_t o = ((size_t)n * gridDim.x + slice) * Jp + tid;
    pmax[o] = b;
    pidx[o] = i;
  }
}

// the scan's own result, for the unit test: idx / maxv [N][J]
__global__ void joint_argmax_all_combine_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx,
                                                int* __restrict__ idx, float* __restrict__ maxv, int slices,
                                                int J, int Jp) {
  const int n = blockIdx.x, j = threadIdx.x;
  if (j >= J) return;
  float b;
  int i;
  argmax_combine(pmax, pidx, n, slices, Jp, j, &b, &i);
  idx[(size_t)n * J + j] = i;
  maxv[(size_t)n * J + j] = b;
}

// Per-camera 2D views of T3 frames (jh_predictor_views2d): block = (frame t, camera c), thread = joint.
//   used      = valid[t] && mask[t][c]
//   points2D  = (m % Hh, m / Wh) * 2 + centerHM - hw, conf2D = min(max, 255) / 255      (jarvis2D.py:139-149, as
//               joint_argmax_kernel) for a used camera; -1 / 0 otherwise
//   reproj    = reprojectPoint(points3D[t][j]) in camera c (project_one: the bits of jh_reproject_point) for EVERY
//               camera of a valid frame -- a masked camera's calibration is known --; NaN for an invalid frame
//   err       = |reproj - points2D|; NaN for a camera that is not used
// Nothing of an unused camera's partials is read: its heat map may hold anything.
__global__ void views2d_final_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx,
                                     const int* __restrict__ center_hm, const int* __restrict__ valid,
                                     const unsigned char* __restrict__ mask, const float* __restrict__ pts3d,
                                     const float* __restrict__ cam, const float* __restrict__ intr,
                                     const float* __restrict__ dist, int fs, int* __restrict__ points2d,
                                     float* __restrict__ conf2d, float* __restrict__ reproj, float* __restrict__ err,
                                     unsigned char* __restrict__ used, int C, int J, int Jp, int slices, int Hh,
                                     int Wh, int hw) {
  const int n = blockIdx.x, t = n / C, c = n % C, j = threadIdx.x;
  const bool ok = valid[t] != 0;
  const bool use = ok && (mask == nullptr || mask[(size_t)t * C + c] != 0);
  if (j == 0) used[n] = use ? 1 : 0;
  if (j >= J) return;
  const size_t o = (size_t)n * J + j;
  const float nan = __int_as_float(0x7fc00000);
  float u = nan, v = nan;
  if (ok) {
    const float* p = pts3d + ((size_t)t * J + j) * 3;
    const size_t row = (size_t)t * fs + c;      // (fs: the calibration's frame stride, see triangulate_body)
    project_one(cam + row * 12, intr + row * 9, dist + row * 5, p[0], p[1], p[2], &u, &v);
  }
  reproj[o * 2 + 0] = u;
  reproj[o * 2 + 1] = v;
  if (!use) {
    points2d[o * 2 + 0] = -1;
    points2d[o * 2 + 1] = -1;
    conf2d[o] = 0.f;
    err[o] = nan;
    return;
  }
  float b;
  int m;
  argmax_combine(pmax, pidx, n, slices, Jp, j, &b, &m);
  int mx, my;
  heat_xy(m, Hh, Wh, &mx, &my);
  const int x = mx * 2 + center_hm[(size_t)n * 2 + 0] - hw;
  const int y = my * 2 + center_hm[(size_t)n * 2 + 1] - hw;
  points2d[o * 2 + 0] = x;
  points2d[o * 2 + 1] = y;
  conf2d[o] = __fdiv_rn(fminf(b, 255.f), 255.f);
  err[o] = pixel_distance(u, v, (float)x, (float)y);
}

// Slicing of the scan: threads per block (a multiple of q), pixels per slice and slices per image -- a function of
// the shape alone, so that the workspace size and every launch agree.  Slices shrink until there are about four
// blocks per compute unit, or one unrolled step per thread is left.
ScanShape joint_argmax_all_shape(int N, int Hh, int Wh, int Jp) {
  ScanShape sh;
  const int q = Jp / 4, rows = kScanThreads / q, P = Hh * Wh;
  sh.threads = rows * q;
  int steps = 4;
  while (steps > 1 && (long long)N * ((P + rows * kScanUnroll * steps - 1) / (rows * kScanUnroll * steps)) < 1024)
    steps /= 2;
  sh.ppb = rows * kScanUnroll * steps;
  sh.slices = (P + sh.ppb - 1) / sh.ppb;
  return sh;
}

size_t joint_argmax_all_partials(int N, int Hh, int Wh, int Jp) {
  return (size_t)N * joint_argmax_all_shape(N, Hh, Wh, Jp).slices * Jp;
}

static int check_scan_shape(int N, int Hh, int Wh, int J, int Jp) {
  JH_REQUIRE(N >= 1 && Hh >= 1 && Wh >= 1, "heat map shape");
  JH_REQUIRE(Jp >= 8 && Jp % 8 == 0 && Jp <= kScanThreads && J >= 1 && J <= Jp, "channel count: J <= Jp, Jp a "
             "multiple of 8 up to 256");
  JH_REQUIRE((long long)Hh * Wh < (1ll << 30) && N <= 65535, "heat map too large for the all-joint argmax");
  return 0;
}

// the scan: heat -> pmax / pidx [N][slices][Jp] (joint_argmax_all_partials() elements each)
int launch_joint_argmax_all(const float* heat, float* pmax, int* pidx, int N, int Hh, int Wh, int J, int Jp,
                            hipStream_t s) {
  if (check_scan_shape(N, Hh, Wh, J, Jp)) return 1;
  const ScanShape sh = joint_argmax_all_shape(N, Hh, Wh, Jp);
  hipLaunchKernelGGL(joint_argmax_all_kernel, dim3(sh.slices, N), dim3(sh.threads), 0, s, heat, pmax, pidx,
                     Hh * Wh, Jp, sh.ppb);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_joint_argmax_all_combine(const float* pmax, const int* pidx, int* idx, float* maxv, int N, int Hh,
                                    int Wh, int J, int Jp, hipStream_t s) {
  if (check_scan_shape(N, Hh, Wh, J, Jp)) return 1;
  const ScanShape sh = joint_argmax_all_shape(N, Hh, Wh, Jp);
  hipLaunchKernelGGL(joint_argmax_all_combine_kernel, dim3(N), dim3(round_up(J, kWave)), 0, s, pmax, pidx, idx,
                     maxv, sh.slices, J, Jp);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_views2d_final(const float* pmax, const int* pidx, const int* center_hm, const int* valid,
                         const unsigned char* mask, const float* pts3d, const Calib& cal, int* points2d,
                         float* conf2d, float* reproj, float* err, unsigned char* used, int T, int C, int J, int Jp,
                         int Hh, int Wh, int hw, hipStream_t s) {
  if (check_scan_shape(T * C, Hh, Wh, J, Jp)) return 1;
  if (calib_check(cal, C)) return 1;
  const ScanShape sh = joint_argmax_all_shape(T * C, Hh, Wh, Jp);
  hipLaunchKernelGGL(views2d_final_kernel, dim3(T * C), dim3(round_up(J, kWave)), 0, s, pmax, pidx, center_hm,
                     valid, mask, pts3d, cal.cam, cal.intr, cal.dist, cal.fs, points2d, conf2d, reproj, err, used, C, J,
                     Jp, sh.slices, Hh, Wh, hw);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
