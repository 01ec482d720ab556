// Small kernels around the networks: frame pre-processing, centre argmax,
// confidence-weighted triangulation, projection, and the soft-argmax tail.
//
//  preprocess_resize   torchvision tensor resize (bilinear, align_corners =
//                      False, no antialias) + (x-mean)/std
//                      jarvis/prediction/jarvis3D.py:143-145
//  preprocess_crop     bounding-box crop + normalisation   jarvis3D.py:168-178
//  center_argmax       per-camera argmax of the centre heatmap, jarvis3D.py:147-155
//  triangulate         ReprojectionTool.reconstructPoint + reprojectPoint +
//                      integer clamp, jarvis/utils/reprojection.py:49-90,
//                      jarvis3D.py:157-166
//  centers             the same integer path from a centre the caller supplies (no detection, no triangulation)
//  center_peaks        the top-P local maxima of a centre heat map, and
//  associate_subjects  their grouping across cameras into up to K triangulated subjects (new design: the reference
//                      keeps one maximum per camera, jarvis3D.py:147-160)
//  softargmax          softplus + spatial soft-argmax + confidences,
//                      jarvis/hybridnet/model.py:73-88
//  joint_argmax_all    argmax of every joint's heat map in one pass + the per-camera 2D views of the 3D
//                      predictor (2D keypoints, reprojections, reprojection errors), jarvis2D.py:139-149
#include "jh_common.h"
#include "dlt.h"
#include "preprocess.h"
#include "views2d.h"
#include "subjects.h"
#include "nets.h"

namespace jh {

// ------------------------------------------------------------------ preprocess
// out: [N][S][S][4] channel-last (one float4 per pixel: r, g, b, 0).
template <int SRC>
__global__ __launch_bounds__(256) void preprocess_resize_kernel(
    const void* __restrict__ frames, float* __restrict__ out, int N, int H, int W, int S,
    float sy, float sx, float3 mean, float3 stdv, const void* const* __restrict__ frames_cell, int per_image,
    SrcDesc<SRC> d) {
  // graph replays: the frame pointer of THIS call is read from a device cell (a captured launch
  // would otherwise keep the pointer of the call it was captured on); per_image: the cell is a table of N image
  // pointers and n varies inside the loop, so the entry is read per iteration (image_base)
  if (frames_cell && !per_image) frames = *frames_cell;
  const size_t total = (size_t)N * S * S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % S), oy = (int)((i / S) % S);
    int n = (int)(i / ((size_t)S * S));
    const void* base = image_base(frames, frames_cell, per_image, n);
    *reinterpret_cast<float4*>(out + i * 4) = resize_px<SRC>(base, n, oy, ox, H, W, sy, sx, mean, stdv, d);
  }
}

int launch_preprocess_resize(const void* frames, const FrameSource& src, float* out, int N, int H, int W, int S,
                             const float* mean, const float* stdv, hipStream_t s,
                             const void* const* frames_cell) {
  const size_t total = (size_t)N * S * S;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  const float3 m = make_float3(mean[0], mean[1], mean[2]), sd = make_float3(stdv[0], stdv[1], stdv[2]);
  JH_REQUIRE(!src.per_image || frames_cell, "per-image frames come with their pointer table");
  if (dispatch_src(src, [&](auto tag, const auto& d) {
        hipLaunchKernelGGL(preprocess_resize_kernel<decltype(tag)::value>, dim3(blocks), dim3(256), 0, s, frames, out,
                           N, H, W, S, (float)H / (float)S, (float)W / (float)S, m, sd, frames_cell,
                           (int)src.per_image, d);
        return 0;
      }))
    return 1;
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// frames: [T][Cloc] images; center_hm: [T][C][2] (all cameras); out [T*Cloc][B][B][4]
template <int SRC>
__global__ __launch_bounds__(256) void preprocess_crop_kernel(
    const void* __restrict__ frames, const int* __restrict__ center_hm, float* __restrict__ out,
    int T, int Cloc, int C, int cam0, int H, int W, int B, float3 mean, float3 stdv,
    const void* const* __restrict__ frames_cell, int per_image, SrcDesc<SRC> d) {
  if (frames_cell && !per_image) frames = *frames_cell;
  const size_t total = (size_t)T * Cloc * B * B;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % B), oy = (int)((i / B) % B);
    int n = (int)(i / ((size_t)B * B));
    const int t = n / Cloc, cl = n % Cloc;
    const int cx = center_hm[(t * C + cam0 + cl) * 2 + 0], cy = center_hm[(t * C + cam0 + cl) * 2 + 1];
    const void* base = image_base(frames, frames_cell, per_image, n);
    *reinterpret_cast<float4*>(out + i * 4) = crop_px<SRC>(base, n, cx, cy, oy, ox, H, W, B, mean, stdv, d);
  }
}

int launch_preprocess_crop(const void* frames, const FrameSource& src, const int* center_hm, float* out, int T,
                           int Cloc, int C, int cam0, int H, int W, int B, const float* mean,
                           const float* stdv, hipStream_t s, const void* const* frames_cell) {
  const size_t total = (size_t)T * Cloc * B * B;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  const float3 m = make_float3(mean[0], mean[1], mean[2]), sd = make_float3(stdv[0], stdv[1], stdv[2]);
  JH_REQUIRE(!src.per_image || frames_cell, "per-image frames come with their pointer table");
  if (dispatch_src(src, [&](auto tag, const auto& d) {
        hipLaunchKernelGGL(preprocess_crop_kernel<decltype(tag)::value>, dim3(blocks), dim3(256), 0, s, frames,
                           center_hm, out, T, Cloc, C, cam0, H, W, B, m, sd, frames_cell, (int)src.per_image, d);
        return 0;
      }))
    return 1;
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// A YUV 4:2:0 or raw sensor form (SRC 2 .. 7) -> [N][H][W][3] uint8 BGR through the pixel function the resize / crop
// use (rgb8_px): the unit-test form of yuv420_px, yuv_surface_px, yuv_wide_px and sensor_px.  One thread per output pixel; only
// plane bytes resp. the H x W samples are read.
template <int SRC>
__global__ __launch_bounds__(256) void frames_to_bgr_kernel(const void* __restrict__ frames,
                                                            unsigned char* __restrict__ out, int N, int H, int W,
                                                            SrcDesc<SRC> d) {
  const size_t total = (size_t)N * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const size_t n = i / ((size_t)H * W);
    const Rgb8 p = rgb8_px<SRC>(frames, n, y, x, H, W, d);
    out[i * 3 + 0] = (unsigned char)p.b;
    out[i * 3 + 1] = (unsigned char)p.g;
    out[i * 3 + 2] = (unsigned char)p.r;
  }
}

int launch_frames_to_bgr(const void* frames, const FrameSource& src, unsigned char* out, int N, int H, int W,
                         hipStream_t s) {
  const size_t total = (size_t)N * H * W;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  JH_REQUIRE(!src.per_image, "the to-BGR helper reads contiguous frames");
  if (dispatch_src(src, [&](auto tag, const auto& d) {
        constexpr int SRC = decltype(tag)::value;
        if constexpr (!kIsRgb8<SRC>) {
          JH_REQUIRE(kIsRgb8<SRC>, "YUV 4:2:0 format");
        } else {
          if constexpr (kIsSensor<SRC>)
            JH_REQUIRE(N >= 1 && H >= 1 && W >= 1 && d.h == H && d.w == W, "raw sensor frames: image size");
          else
            JH_REQUIRE(N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
                       "YUV 4:2:0 frames need an even height and width");
          hipLaunchKernelGGL(frames_to_bgr_kernel<SRC>, dim3(blocks), dim3(256), 0, s, frames, out, N, H, W, d);
        }
        return 0;
      }))
    return 1;
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

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
    for (int u = 0; u < U; ++u) {
      const int pp = p + u * blockDim.x;
      if (v[u] > best || (v[u] == best && pp < bi)) { best = v[u]; bi = pp; }
    }
  }
  for (; p < P; p += blockDim.x) {
    const float v = h[(size_t)p * Cp];
    if (v > best || (v == best && p < bi)) { best = v; bi = p; }
  }
  sv[threadIdx.x] = best; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const float v = sv[threadIdx.x + s];
      const int ii = si[threadIdx.x + s];
      if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && ii < si[threadIdx.x])) {
        sv[threadIdx.x] = v; si[threadIdx.x] = ii;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int m = si[0];
    // preds = (m % shape[2], m // shape[3])   jarvis3D.py:151
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
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    const float v = h[(size_t)p * Jp];
    if (v > best || (v == best && p < bi)) { best = v; bi = p; }
  }
  sv[threadIdx.x] = best; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const float v = sv[threadIdx.x + s];
      const int ii = si[threadIdx.x + s];
      if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && ii < si[threadIdx.x])) {
        sv[threadIdx.x] = v; si[threadIdx.x] = ii;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int m = si[0];
    points[((size_t)t * J + j) * 2 + 0] = (m % Hh) * 2 + center_hm[t * 2 + 0] - hw;
    points[((size_t)t * J + j) * 2 + 1] = (m / Wh) * 2 + center_hm[t * 2 + 1] - hw;
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
  const int x = (m % Hh) * 2 + center_hm[(size_t)n * 2 + 0] - hw;
  const int y = (m / Wh) * 2 + center_hm[(size_t)n * 2 + 1] - hw;
  points2d[o * 2 + 0] = x;
  points2d[o * 2 + 1] = y;
  conf2d[o] = __fdiv_rn(fminf(b, 255.f), 255.f);
  const float dx = __fsub_rn(u, (float)x), dy = __fsub_rn(v, (float)y);
  err[o] = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
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
//   skey [T][Jp]: max over the voxels of (ordered key of x) << 32 | (0xFFFFFFFF - p): the maximum of x, the LOWEST
//     flat index among equal maxima.  x may be negative, so the key is the order-preserving map of the float's
//     bits, not the bits themselves.
// The float sums and maxima are computed by the same statements in the same order with SPREAD on and off.
constexpr int kSpreadSums = 10, kSpreadRound = 5;          // (sums; sums per round of the block reduction)
__device__ __forceinline__ unsigned long long spread_key(float x, unsigned p) {
  const unsigned u = __float_as_uint(x);
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)k << 32) | (unsigned long long)(0xFFFFFFFFu - p);
}
__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) {
  return a > b ? a : b;
}
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
        key[0] = max_u64(key[0], spread_key(v.x, (unsigned)p));
        key[1] = max_u64(key[1], spread_key(v.y, (unsigned)p));
        key[2] = max_u64(key[2], spread_key(v.z, (unsigned)p));
        key[3] = max_u64(key[3], spread_key(v.w, (unsigned)p));
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
  const unsigned p = 0xFFFFFFFFu - (unsigned)(skey[(size_t)t * Jp + j] & 0xFFFFFFFFull);
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
    const size_t total = (size_t)T * J * P;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(heatmap_final_kernel, dim3(blocks), dim3(256), 0, s, x, heatmap_final, J, Jp,
                       (size_t)P, T);
    JH_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

size_t softargmax_spread_sums(int T, int Jp) { return (size_t)T * Jp * kSpreadSums * kLimbs; }

// ------------------------------------------------- several subjects: peaks of a map
// Top-P local maxima of channel 0 of heat [N][Hh][Wh][Cp] (include/jarvis_hip.h, jh_op_center_peaks).  Pixel p (flat
// index y * Wh + x) is a peak iff v(p) > min_peak and it is the maximum of the total order (value descending, index
// ascending) over its (2r+1)^2 window clipped at the map's edge; NaN takes no part.  The order is carried by ONE 64-bit
// key, peak_key: spread_key with -0 folded onto +0 (the two compare equal, as in center_argmax_kernel) and 0 for NaN,
// below every real key.
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

__device__ __forceinline__ unsigned long long peak_key(float v, unsigned p) {
  return v != v ? 0ull : spread_key(v == 0.f ? 0.f : v, p);
}

// maximum of k over the block; every thread calls it and gets it.  red: one slot per wave.
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long k, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = max_u64(k, (unsigned long long)__shfl_xor((long long)k, o));
  const int nw = blockDim.x >> 6;
  __syncthreads();                              // (the slots of the previous call have been read)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
  __syncthreads();
  unsigned long long m = red[0];
  for (int i = 1; i < nw; ++i) m = max_u64(m, red[i]);
  return m;
}

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
      const int m = (int)(0xFFFFFFFFu - (unsigned)(win & 0xFFFFFFFFull));
      out[found * 3 + 0] = (float)(m % Hh);     // (the expression of center_argmax_kernel)
      out[found * 3 + 1] = (float)(m / Wh);
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
// distance is <= max_err), and the key  views << 50 | ~bits(cost) << 18 | ~index  whose maximum is the choice: most
// views, then the smallest cost (a sum of non-negative floats: its bits order as it does), then the lowest (a, i, b, j).
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
      const float dx = __fsub_rn(u, sh.px[c * P + sl]), dy = __fsub_rn(v, sh.py[c * P + sl]);
      const float d = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
      if (d == d && (bests < 0 || d < bestd)) { bests = sl; bestd = d; }   // (ties: the lowest slot; NaN: never)
    }
    const bool ok = bests >= 0 && depth > 0.f && bestd <= max_err;
    if (ok) { ++n; sum = __fadd_rn(sum, bestd); }
    if (member) member[c] = ok ? bests : -1;
  }
  *views = n;
  *cost = sum;
}

// the two-view DLT point of the slots ai < bj (cameras in order)
__device__ __forceinline__ void assoc_pair_point(const AssocShared& sh, int ai, int bj, float* X) {
  double ata[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      s += dlt_term(sh.rows[ai], sh.rows[ai] + 4, i, j);
      s += dlt_term(sh.rows[bj], sh.rows[bj] + 4, i, j);
      ata[i * 4 + j] = s;
    }
  dlt_solve(ata, X);
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
      assoc_pair_point(sh, ai, bj, X);
      assoc_support(sh, X, C, P, max_err, &nv, &cost, nullptr);
      const unsigned long long key = ((unsigned long long)nv << 50) |
                                     ((unsigned long long)(~__float_as_uint(cost)) << 18) |
                                     (unsigned long long)(0x3FFFF - idx);
      best = max_u64(best, key);
    }
    const unsigned long long win = block_max_u64(best, sh.red);
    if ((int)(win >> 50) < min_views) break;    // (uniform; also "no pair left": win == 0)
    if (tid == 0) {
      const int idx = 0x3FFFF - (int)(win & 0x3FFFF), ai = idx / CP, bj = idx - ai * CP;
      float X[3], cost, ctr[3];
      int nv;
      assoc_pair_point(sh, ai, bj, X);
      assoc_support(sh, X, C, P, max_err, &nv, &cost, sh.member);
      double ata[16];
      for (int e = 0; e < 16; ++e) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) {
          const int sl = sh.member[c] >= 0 ? c * P + sh.member[c] : 0;
          const double term = dlt_term(sh.rows[sl], sh.rows[sl] + 4, e >> 2, e & 3);
          s += sh.member[c] >= 0 ? term : 0.0;
        }
        ata[e] = s;
      }
      dlt_solve(ata, ctr);
      float esum = 0.f;
      for (int c = 0; c < C; ++c) {
        members[((size_t)t * K + k) * C + c] = sh.member[c];
        if (sh.member[c] < 0) continue;
        const int sl = c * P + sh.member[c];
        float u, v;
        project_one(sh.M + c * 12, sh.K + c * 9, sh.D + c * 5, ctr[0], ctr[1], ctr[2], &u, &v);
        const float dx = __fsub_rn(u, sh.px[sl]), dy = __fsub_rn(v, sh.py[sl]);
        esum = __fadd_rn(esum, __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))));
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
