// From a centre heat map to the crop centres: centre argmax, confidence-weighted triangulation, projection.
//
//  center_argmax       per-camera argmax of the centre heatmap, jarvis3D.py:147-155
//  center2d            the 2D predictor's crop centre from its detection, jarvis2D.py:121-129
//  triangulate         ReprojectionTool.reconstructPoint + reprojectPoint +
//                      integer clamp, jarvis/utils/reprojection.py:49-90,
//                      jarvis3D.py:157-166
//  centers             the same integer path from a centre the caller supplies (no detection, no triangulation)
//  project_points      ReprojectionTool.reprojectPoint for tests and the API
#include "jh_common.h"
#include "argmax.h"
#include "dlt.h"
#include "centers.h"

namespace jh {

// --------------------------------------------------------------- centre argmax
// heat: [N][Hh][Wh][Cp], channel 0.  det[n] = (x, y, maxval); first maximum wins
// (torch.argmax on CPU returns the lowest index among equal maxima).
__global__ __launch_bounds__(1024) void center_argmax_kernel(const float* __restrict__ heat,
                                                            float* __restrict__ det, int Hh,
                                                            int Wh, int Cp) {
  __shared__ float sv[1024];
  __shared__ int si[1024];
  const int n = blockIdx.x;
  const int P = Hh * Wh;
  const float* h = heat + (size_t)n * P * Cp;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  // (eight independent loads in flight per thread: the scan is a chain of load latencies otherwise -- 26 us for
  //  a 256 x 256 map; the compares keep the ascending-index order, so the first maximum still wins)
  constexpr int U = 8;
  int p = threadIdx.x;
  for (; p + (U - 1) * (int)blockDim.x < P; p += U * blockDim.x) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = h[(size_t)(p + u * blockDim.x) * Cp];
#pragma unroll
    for (int u = 0; u < U; ++u) argmax_take(v[u], p + u * blockDim.x, best, bi);
  }
  for (; p < P; p += blockDim.x) argmax_take(h[(size_t)p * Cp], p, best, bi);
  block_argmax<1024>(sv, si, best, bi);
  if (threadIdx.x == 0) {
    const int m = si[0];
    // heat_xy (argmax.h), spelled out: each store right behind its division keeps this kernel's instruction stream
    det[n * 3 + 0] = (float)(m % Hh);
    det[n * 3 + 1] = (float)(m / Wh);
    det[n * 3 + 2] = sv[0];
  }
}

int launch_center_argmax(const float* heat, float* det, int N, int Hh, int Wh, int Cp,
                         hipStream_t s) {
  hipLaunchKernelGGL(center_argmax_kernel, dim3(N), dim3(1024), 0, s, heat, det, Hh, Wh, Cp);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------- 2D predictor glue kernels
// JarvisPredictor2D (jarvis/prediction/jarvis2D.py:121-129): crop centre of each image
// from its centre detection: trunc((x, y) * scale * 2), clamped to
// [hw, size - hw - 1]; valid = maxval > 40.
__global__ void center2d_kernel(const float* __restrict__ det, int* __restrict__ center_hm,
                                int* __restrict__ valid, int T, float sx, float sy, int hw, int W,
                                int H) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float* d = det + (size_t)t * 3;
  int cx = (int)__fmul_rn(__fmul_rn(d[0], sx), 2.f);
  int cy = (int)__fmul_rn(__fmul_rn(d[1], sy), 2.f);
  cx = min(max(cx, hw), W - hw - 1);
  cy = min(max(cy, hw), H - hw - 1);
  center_hm[t * 2 + 0] = cx;
  center_hm[t * 2 + 1] = cy;
  valid[t] = d[2] > 40.f ? 1 : 0;
}

int launch_center2d(const float* det, int* center_hm, int* valid, int T, float sx, float sy, int hw,
                    int W, int H, hipStream_t s) {
  hipLaunchKernelGGL(center2d_kernel, dim3((T + 63) / 64), dim3(64), 0, s, det, center_hm, valid, T,
                     sx, sy, hw, W, H);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// Crop centre of one camera from the 3D centre (x, y, z): reprojectPoint, .int() and the clamps of
// jarvis3D.py:161-166.  THE tail of the triangulation and of the caller-supplied centres (centers_kernel): one
// function, so that a centre handed back to the library gives the crop centres its detection gave.  row: the camera's
// calibration row (frame stride included); out: its two ints of center_hm.
// GUARD (centers_kernel: the centre is the caller's, the projection may be anything): a projection that is not finite or
// not below 2^31 in magnitude is not converted -- it takes the clamp's lower bound.  Without it the conversion is the
// one the triangulation always made.
template <bool GUARD>
__device__ __forceinline__ void crop_centre(const float* __restrict__ cam, const float* __restrict__ intr,
                                            const float* __restrict__ dist, size_t row, float x, float y, float z,
                                            int hw, int W, int H, int* __restrict__ out) {
  float u, v;
  project_one(cam + row * 12, intr + row * 9, dist + row * 5, x, y, z, &u, &v);
  int iu, iv;
  if constexpr (GUARD) {
    iu = fabsf(u) < 2147483648.f ? (int)u : hw;  // (NaN and inf compare false)
    iv = fabsf(v) < 2147483648.f ? (int)v : hw;
  } else {
    iu = (int)u;
    iv = (int)v;
  }
  iu = min(max(iu, hw), W - hw);               // jarvis3D.py:163-166
  iv = min(max(iv, hw), H - hw);
  out[0] = iu;
  out[1] = iv;
}

// One 64-thread block per frame t.  det: [T][C][3] (x, y, raw maxval).
// Outputs: center3d_f [T][3] float, center3d_i [T][3] int (truncated),
// center_hm [T][C][2] int (truncated + clamped crop centres), valid [T].
// MASK (nets.h): camera c of frame t takes part iff mask[t][c] != 0.  A masked camera's term of A^T A is an
// exact 0.0 -- SELECTED, not multiplied: its detection may be NaN -- and s + 0.0 == s, so the centre has the bits
// of a run over the unmasked cameras alone; it is not counted either.  Its crop centre is still written (the
// clamped projection of the centre: in range whatever its frame held).
// fs: the calibration's frame stride in cameras -- frame t reads row t * fs + c of cam / intr / dist; 0: one calibration
// shared by all frames, C: one per frame (jh_predictor_set_calibration_frames).  Only the address of the 26 floats
// moves: the operations on them are the same.
template <bool MASK>
__device__ __forceinline__ void triangulate_body(
    const float* __restrict__ det, const float* __restrict__ cam, const float* __restrict__ intr,
    const float* __restrict__ dist, int fs, float* __restrict__ center3d_f, int* __restrict__ center3d_i,
    int* __restrict__ center_hm, int* __restrict__ valid, int C, float sx2, float sy2, float wdiv,
    int hw, int W, int H, const unsigned char* __restrict__ mask, int* __restrict__ n_active,
    int* __restrict__ n_detect) {
  __shared__ double ata[16];
  __shared__ double contrib[64][17];            // per-camera terms of A^T A (summed in camera order)
  __shared__ float ctr[3];
  __shared__ int cnt;
  __shared__ int act;
  const int t = blockIdx.x, c = threadIdx.x;
  const size_t row = (size_t)t * fs + c;        // this camera's calibration
  if (c == 0) { cnt = 0; if constexpr (MASK) act = 0; }
  __syncthreads();
  if (c < C) {
    bool live = true;
    if constexpr (MASK) {
      live = mask[(size_t)t * C + c] != 0;
      if (live) atomicAdd(&act, 1);
    }
    const float* d = det + ((size_t)t * C + c) * 3;
    const float k1 = dist[row * 5 + 0], k2 = dist[row * 5 + 1];
    if (live && d[2] > 50.f) atomicAdd(&cnt, 1);
    float r0[4], r1[4];
    dlt_rows(d, cam + row * 12, intr + row * 9, k1, k2, sx2, sy2, wdiv, r0, r1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
      {
        const double term = dlt_term(r0, r1, i, j);
        contrib[c][i * 4 + j] = live ? term : 0.0;
      }
  }
  __syncthreads();
  if (c < 16) {                                 // fixed order: the result does not depend on timing
    double s = 0.0;
    for (int k = 0; k < C; ++k) s += contrib[k][c];
    ata[c] = s;
  }
  __syncthreads();
  if (c == 0) {
    float f[3];
    dlt_solve(ata, f);
    for (int k = 0; k < 3; ++k) {
      ctr[k] = f[k];
      center3d_f[t * 3 + k] = f[k];
      center3d_i[t * 3 + k] = (int)f[k];       // .int() truncates, jarvis3D.py:183
    }
    valid[t] = cnt >= 2 ? 1 : 0;
    if constexpr (MASK) { n_active[t] = act; n_detect[t] = cnt; }
  }
  __syncthreads();
  if (c < C) crop_centre<false>(cam, intr, dist, row, ctr[0], ctr[1], ctr[2], hw, W, H, center_hm + ((size_t)t * C + c) * 2);
}

__global__ __launch_bounds__(64) void triangulate_kernel(
    const float* __restrict__ det, const float* __restrict__ cam, const float* __restrict__ intr,
    const float* __restrict__ dist, int fs, float* __restrict__ center3d_f, int* __restrict__ center3d_i,
    int* __restrict__ center_hm, int* __restrict__ valid, int C, float sx2, float sy2, float wdiv,
    int hw, int W, int H) {
  triangulate_body<false>(det, cam, intr, dist, fs, center3d_f, center3d_i, center_hm, valid, C, sx2, sy2, wdiv, hw, W, H,
                          nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void triangulate_masked_kernel(
    const float* __restrict__ det, const float* __restrict__ cam, const float* __restrict__ intr,
    const float* __restrict__ dist, int fs, float* __restrict__ center3d_f, int* __restrict__ center3d_i,
    int* __restrict__ center_hm, int* __restrict__ valid, int C, float sx2, float sy2, float wdiv,
    int hw, int W, int H, const unsigned char* __restrict__ mask, int* __restrict__ n_active,
    int* __restrict__ n_detect) {
  triangulate_body<true>(det, cam, intr, dist, fs, center3d_f, center3d_i, center_hm, valid, C, sx2, sy2, wdiv, hw, W, H,
                         mask, n_active, n_detect);
}

int launch_triangulate(const float* det, const Calib& cal, float* center3d_f, int* center3d_i, int* center_hm,
                       int* valid, int T, int C, float sx2, float sy2, float wdiv, int hw, int W, int H,
                       const unsigned char* mask, int* n_active, int* n_detect, hipStream_t s) {
  JH_REQUIRE(C <= 64, "at most 64 cameras");
  if (calib_check(cal, C)) return 1;
  if (mask) {
    JH_REQUIRE(n_active && n_detect, "camera mask");
    hipLaunchKernelGGL(triangulate_masked_kernel, dim3(T), dim3(64), 0, s, det, cal.cam, cal.intr, cal.dist, cal.fs,
                       center3d_f, center3d_i, center_hm, valid, C, sx2, sy2, wdiv, hw, W, H, mask, n_active, n_detect);
  } else {
    hipLaunchKernelGGL(triangulate_kernel, dim3(T), dim3(64), 0, s, det, cal.cam, cal.intr, cal.dist, cal.fs,
                       center3d_f, center3d_i, center_hm, valid, C, sx2, sy2, wdiv, hw, W, H);
  }
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------- caller-supplied centres
// Stage 2 without stage 1 (jh_predictor_set_centers): the 3D centre of frame set t is centers[t] (world mm) instead of
// a triangulated detection.  One 64-thread block per frame set, one lane per camera; writes what triangulate_body
// writes, det excepted:
//   center3d_f = the centre as given; center3d_i = (int)centre, truncation toward zero (jarvis3D.py:183);
//   center_hm  = crop_centre() of it, the tail the triangulation runs;
//   valid      = the three coordinates are finite and |x| < 2^24 (no detection ran: there is no `> 50` gate), and
//                under a mask at least one camera of the row is unmasked; n_active as the masked triangulation counts
//                it, n_detect = 0.
// An invalid row is computed for the centre (0, 0, 0): nothing non-finite or out of range is ever converted to int,
// and its crop centres are in range.
template <bool MASK>
__global__ __launch_bounds__(64) void centers_kernel(
    const float* __restrict__ centers, const float* __restrict__ cam, const float* __restrict__ intr,
    const float* __restrict__ dist, int fs, float* __restrict__ center3d_f, int* __restrict__ center3d_i,
    int* __restrict__ center_hm, int* __restrict__ valid, int C, int hw, int W, int H,
    const unsigned char* __restrict__ mask, int* __restrict__ n_active, int* __restrict__ n_detect) {
  const int t = blockIdx.x, c = threadIdx.x;
  const float gx = centers[t * 3 + 0], gy = centers[t * 3 + 1], gz = centers[t * 3 + 2];
  // (NaN and inf compare false)
  const bool ok = fabsf(gx) < 16777216.f && fabsf(gy) < 16777216.f && fabsf(gz) < 16777216.f;
  const float x = ok ? gx : 0.f, y = ok ? gy : 0.f, z = ok ? gz : 0.f;
  int act = 0;
  if constexpr (MASK) act = __syncthreads_count(c < C && mask[(size_t)t * C + c] != 0);
  if (c == 0) {
    center3d_f[t * 3 + 0] = gx; center3d_f[t * 3 + 1] = gy; center3d_f[t * 3 + 2] = gz;
    center3d_i[t * 3 + 0] = (int)x; center3d_i[t * 3 + 1] = (int)y; center3d_i[t * 3 + 2] = (int)z;
    if constexpr (MASK) {
      valid[t] = ok && act >= 1 ? 1 : 0;
      n_active[t] = act;
      n_detect[t] = 0;
    } else {
      valid[t] = ok ? 1 : 0;
    }
  }
  if (c < C)
    crop_centre<true>(cam, intr, dist, (size_t)t * fs + c, x, y, z, hw, W, H, center_hm + ((size_t)t * C + c) * 2);
}

// mask == nullptr: all cameras (n_active / n_detect are not touched, as by launch_triangulate)
int launch_centers(const float* centers, const Calib& cal, float* center3d_f, int* center3d_i, int* center_hm,
                   int* valid, int T, int C, int hw, int W, int H, const unsigned char* mask, int* n_active,
                   int* n_detect, hipStream_t s) {
  JH_REQUIRE(C <= 64, "at most 64 cameras");
  JH_REQUIRE(centers, "caller-supplied centres");
  if (calib_check(cal, C)) return 1;
  if (mask) {
    JH_REQUIRE(n_active && n_detect, "camera mask");
    hipLaunchKernelGGL(centers_kernel<true>, dim3(T), dim3(64), 0, s, centers, cal.cam, cal.intr, cal.dist, cal.fs,
                       center3d_f, center3d_i, center_hm, valid, C, hw, W, H, mask, n_active, n_detect);
  } else {
    hipLaunchKernelGGL(centers_kernel<false>, dim3(T), dim3(64), 0, s, centers, cal.cam, cal.intr, cal.dist, cal.fs,
                       center3d_f, center3d_i, center_hm, valid, C, hw, W, H, nullptr, nullptr, nullptr);
  }
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// points [P][3] -> uv [C][P][2]  (ReprojectionTool.reprojectPoint for tests/API)
__global__ void project_points_kernel(const float* __restrict__ pts, const float* cam,
                                      const float* intr, const float* dist, float* uv, int P,
                                      int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * C) return;
  const int c = i / P, p = i % P;
  float u, v;
  project_one(cam + c * 12, intr + c * 9, dist + c * 5, pts[p * 3], pts[p * 3 + 1], pts[p * 3 + 2], &u, &v);
  uv[(size_t)i * 2] = u;
  uv[(size_t)i * 2 + 1] = v;
}

int launch_project_points(const float* pts, const float* cam, const float* intr, const float* dist,
                          float* uv, int P, int C, hipStream_t s) {
  hipLaunchKernelGGL(project_points_kernel, dim3((P * C + 63) / 64), dim3(64), 0, s, pts, cam, intr,
                     dist, uv, P, C);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
