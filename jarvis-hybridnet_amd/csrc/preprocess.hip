// Frame pre-processing as kernels of its own (the fused form is the stem convolution's patch staging, stem.hip; the
// per-pixel arithmetic of both is preprocess.h):
//
//  preprocess_resize   torchvision tensor resize (bilinear, align_corners =
//                      False, no antialias) + (x-mean)/std
//                      jarvis/prediction/jarvis3D.py:143-145
//  preprocess_crop     bounding-box crop + normalisation   jarvis3D.py:168-178
//  frames_to_bgr       a YUV 4:2:0, raw sensor or pixel-surface form as uint8 BGR: the unit-test form of the pixel
//                      functions
#include "jh_common.h"
#include "preprocess.h"

namespace jh {

// ------------------------------------------------------------------ preprocess
// out: [N][S][S][4] channel-last (one float4 per pixel: r, g, b, 0).
template <int SRC, class Tone>
__global__ __launch_bounds__(256) void preprocess_resize_kernel(
    const void* __restrict__ frames, float* __restrict__ out, int N, int H, int W, int S,
    float sy, float sx, float3 mean, float3 stdv, const void* const* __restrict__ frames_cell, int per_image,
    SrcDesc<SRC> d, Tone tone) {
  // graph replays: the frame pointer of THIS call is read from a device cell (a captured launch
  // would otherwise keep the pointer of the call it was captured on); per_image: the cell is a table of N image
  // pointers and n varies inside the loop, so the entry is read per iteration (image_base)
  if (frames_cell && !per_image) frames = *frames_cell;
  const size_t total = (size_t)N * S * S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % S), oy = (int)((i / S) % S);
    int n = (int)(i / ((size_t)S * S));
    const auto lut = tone.of(n);
    const void* base = image_base(frames, frames_cell, per_image, n);
    *reinterpret_cast<float4*>(out + i * 4) = resize_px<SRC>(base, n, oy, ox, H, W, sy, sx, mean, stdv, d, lut);
  }
}

int launch_preprocess_resize(const void* frames, const FrameSource& src, float* out, int N, int H, int W, int S,
                             const float* mean, const float* stdv, hipStream_t s,
                             const void* const* frames_cell) {
  const int blocks = stride_blocks((size_t)N * S * S);
  const float3 m = make_float3(mean[0], mean[1], mean[2]), sd = make_float3(stdv[0], stdv[1], stdv[2]);
  JH_REQUIRE(!src.per_image || frames_cell, "per-image frames come with their pointer table");
  if (dispatch_src(src, [&](auto tag, const auto& d, auto tone) {
        hipLaunchKernelGGL((preprocess_resize_kernel<decltype(tag)::value, decltype(tone)>), dim3(blocks), dim3(256), 0,
                           s, frames, out, N, H, W, S, (float)H / (float)S, (float)W / (float)S, m, sd, frames_cell,
                           (int)src.per_image, d, tone);
        return 0;
      }))
    return 1;
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// frames: [T][Cloc] images; center_hm: [T][C][2] (all cameras); out [T*Cloc][B][B][4]
template <int SRC, class Tone>
__global__ __launch_bounds__(256) void preprocess_crop_kernel(
    const void* __restrict__ frames, const int* __restrict__ center_hm, float* __restrict__ out,
    int T, int Cloc, int C, int cam0, int H, int W, int B, float3 mean, float3 stdv,
    const void* const* __restrict__ frames_cell, int per_image, SrcDesc<SRC> d, Tone tone) {
  if (frames_cell && !per_image) frames = *frames_cell;
  const size_t total = (size_t)T * Cloc * B * B;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % B), oy = (int)((i / B) % B);
    int n = (int)(i / ((size_t)B * B));
    const int t = n / Cloc, cl = n % Cloc;
    const int cx = center_hm[(t * C + cam0 + cl) * 2 + 0], cy = center_hm[(t * C + cam0 + cl) * 2 + 1];
    const auto lut = tone.of(n);
    const void* base = image_base(frames, frames_cell, per_image, n);
    *reinterpret_cast<float4*>(out + i * 4) = crop_px<SRC>(base, n, cx, cy, oy, ox, H, W, B, mean, stdv, d, lut);
  }
}

int launch_preprocess_crop(const void* frames, const FrameSource& src, const int* center_hm, float* out, int T,
                           int Cloc, int C, int cam0, int H, int W, int B, const float* mean,
                           const float* stdv, hipStream_t s, const void* const* frames_cell) {
  const int blocks = stride_blocks((size_t)T * Cloc * B * B);
  const float3 m = make_float3(mean[0], mean[1], mean[2]), sd = make_float3(stdv[0], stdv[1], stdv[2]);
  JH_REQUIRE(!src.per_image || frames_cell, "per-image frames come with their pointer table");
  if (dispatch_src(src, [&](auto tag, const auto& d, auto tone) {
        hipLaunchKernelGGL((preprocess_crop_kernel<decltype(tag)::value, decltype(tone)>), dim3(blocks), dim3(256), 0,
                           s, frames, center_hm, out, T, Cloc, C, cam0, H, W, B, m, sd, frames_cell,
                           (int)src.per_image, d, tone);
        return 0;
      }))
    return 1;
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// A YUV 4:2:0, raw sensor or pixel-surface form (SRC 2 .. 8) -> [N][H][W][3] uint8 BGR through the pixel function the
// resize / crop use (rgb8_px): the unit-test form of yuv420_px, yuv_surface_px, yuv_wide_px, sensor_px and pixels_px.  One thread per output pixel; only
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
  const int blocks = stride_blocks((size_t)N * H * W);
  JH_REQUIRE(!src.per_image, "the to-BGR helper reads contiguous frames");
  JH_REQUIRE(!src.tone, "the to-BGR helper gives the bytes before any tone table");
  if (dispatch_src(src, [&](auto tag, const auto& d, auto) {
        constexpr int SRC = decltype(tag)::value;
        if constexpr (!kIsRgb8<SRC>) {
          JH_REQUIRE(kIsRgb8<SRC>, "YUV 4:2:0 format");
        } else {
          if constexpr (kIsSensor<SRC>)
            JH_REQUIRE(N >= 1 && H >= 1 && W >= 1 && d.h == H && d.w == W, "raw sensor frames: image size");
          else if constexpr (SRC == kSrcPixels)
            JH_REQUIRE(N >= 1 && H >= 1 && W >= 1, "pixel surfaces: image size");   // (checked for H x W by the caller)
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

// Any byte form -> [N][3][H][W] fp32, the three values the resize / crop fetch sees for every pixel (frame_px3 with the
// launch's tone form): the unit-test form of byte_value under each pixel function.  One thread per pixel; only plane
// bytes resp. the H x W samples are read, and a table is read at a byte's index only.
template <int SRC, class Tone>
__global__ __launch_bounds__(256) void frames_to_rgb_f32_kernel(const void* __restrict__ frames,
                                                                float* __restrict__ out, int N, int H, int W,
                                                                SrcDesc<SRC> d, Tone tone) {
  const size_t plane = (size_t)H * W, total = (size_t)N * plane;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const size_t n = i / plane;
    float v[3];
    frame_px3<SRC>(frames, n, y, x, H, W, d, v, tone.of((int)n));
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(n * 3 + c) * plane + (i - n * plane)] = v[c];
  }
}

int launch_frames_to_rgb_f32(const void* frames, const FrameSource& src, float* out, int N, int H, int W,
                             hipStream_t s) {
  const int blocks = stride_blocks((size_t)N * H * W);
  JH_REQUIRE(!src.per_image, "the to-fp32 helper reads contiguous frames");
  JH_REQUIRE(src.fmt != kSrcRgbF32, "the to-fp32 helper takes byte frames");
  JH_REQUIRE(N >= 1 && H >= 1 && W >= 1, "image size");
  if (dispatch_src(src, [&](auto tag, const auto& d, auto tone) {
        constexpr int SRC = decltype(tag)::value;
        if constexpr (SRC != kSrcRgbF32) {
          if constexpr (kIsSensor<SRC>) JH_REQUIRE(d.h == H && d.w == W, "raw sensor frames: image size");
          hipLaunchKernelGGL((frames_to_rgb_f32_kernel<SRC, decltype(tone)>), dim3(blocks), dim3(256), 0, s, frames,
                             out, N, H, W, d, tone);
        }
        return 0;
      }))
    return 1;
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
