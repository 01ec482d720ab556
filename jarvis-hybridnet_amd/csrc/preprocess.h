// Per-pixel arithmetic of the frame pre-processing (jarvis/prediction/jarvis3D.py:143-145 resize +
// normalise, :168-178 crop + normalise), shared by the stand-alone kernels (preprocess.hip) and the stem
// convolution that applies it while staging its input patch (stem.hip): ONE definition, so the fused
// and the unfused path produce the same bits.
//
// The frames come in one of nine SOURCE FORMS (SRC, the kSrc* codes; 0 .. 3 are JH_FRAME_* of include/jarvis_hip.h):
//   0 kSrcRgbF32      [N][3][H][W] fp32 RGB in [0,1] (the API input of JarvisPredictor3D.forward);
//   1 kSrcBgrU8       [N][H][W][3] uint8 BGR as the video decoder delivers it, converted like predict3D.py:79-80
//                     (`.float()...[:, [2,1,0]] / 255.`) on the fly, so the 4x larger fp32 frame never exists;
//   2 kSrcI420        YUV 4:2:0, one contiguous [3H/2][W] byte image per camera (H, W even): the Y plane [H][W],
//                     then U [H/2][W/2], then V [H/2][W/2];
//   3 kSrcNV12        the Y plane, then one interleaved [H/2][W/2][2] plane, U first.  A YUV pixel is converted to
//                     the BGR bytes cv2.cvtColor(COLOR_YUV2BGR_I420 / _NV12) gives (yuv420_px) and those bytes enter
//                     the uint8 arithmetic unchanged; layout and constants are compile-time immediates;
//   4 kSrcYuvSurface  a described YUV 4:2:0 surface (jh_yuv_surface): plane offsets, pitches, the chroma order and
//                     step, and the colour matrix / range come with the launch (YuvSurface), so pitched decoder
//                     surfaces, YV12 / NV21 and BT.709 / full-range streams are read in place (yuv_surface_px);
//   5 kSrcSensor      a raw sensor image (jh_sensor_surface): one byte per pixel, Mono8 or an 8-bit Bayer mosaic,
//                     demosaiced per fetched pixel (sensor_px); the (R, G, B) bytes enter the uint8 arithmetic
//                     unchanged, as the YUV forms' bytes do;
//   6 kSrcSensorWide  a raw sensor image whose samples are wider than a byte: 16-bit words or the GenICam 10p / 12p
//                     bit stream (jh_sensor_surface.sample).  A sample is reduced to its top byte where it is loaded
//                     (byte8) and the bytes go through the demosaic of form 5 (sensor_px);
//   7 kSrcYuvWide     a described YUV 4:2:0 surface of 16-bit samples (P010, yuv420p10le): reduced the same way, then
//                     converted with the constants of form 4 (yuv_wide_px);
//   8 kSrcPixels      a described pixel surface (jh_pixel_surface): three 8-bit components per pixel, R G B or Y U V,
//                     each found by its own address rule -- offset, pitch, step and the two subsampling shifts -- so
//                     RGB in any byte order, 4-byte and planar RGB, grey, packed YUYV / UYVY and planar or semi-planar
//                     4:2:2 / 4:4:4 / 4:4:0 / 4:1:1 are values of one description (pixels_px).  YUV components are
//                     converted with the constants of form 4.  No public JH_FRAME_* code: the form has entry points
//                     of its own (jh_predictor_forward_pixels and its like).
// Callers see 6 and 7 as JH_FRAME_SENSOR / JH_FRAME_SURFACE: the frame_source constructors choose them from the
// description's sample code, so the kernels of forms 4 and 5 carry nothing of the wide ones.
//
// A source form is four local things, and a new one adds exactly these:
//   1. its description: a specialisation of SrcDesc<SRC> (what a kernel of that form takes BY VALUE -- wave-uniform,
//      so it stays in scalar registers; a form that needs none keeps the empty primary template) with a field-wise
//      operator==, and its alternative in FrameSource::desc;
//   2. its pixel function, selected in rgb8_px<SRC> (a form delivering (R, G, B) bytes) or frame_px<SRC>;
//   3. its row in dispatch_src, the one place a run-time format code becomes a template argument: the resize, the
//      crop, the fused stem and the to-BGR launchers all instantiate through it;
//   4. its host constructor in api_frames.hip (frame_source), which validates what the caller gave and builds the FrameSource
//      every layer below takes.
// Nothing else names a form: the kernels, StemSource and the predictor's graph slots carry a SrcDesc<SRC> resp. a
// FrameSource whatever it holds.
//
// WHERE the images of a launch lie is independent of their form (image_base below): at `frames + n * stride` of one
// base pointer -- given with the launch, or read from a one-pointer device cell under graph replay --, or PER IMAGE,
// image n at table[n] of a device table of N pointers (jh_predictor_forward_images: every camera's buffer where its
// producer left it).  The per-image flag is wave-uniform launch data; with it set the pixel functions below get
// (table[n], image 0), otherwise (base, n): their arithmetic is the same either way.
// Alignment under a table: fp32 images are 4-byte aligned (checked on the host); the byte forms may start at ANY
// address -- the one wider load there is, the 2-byte chroma pair of NV12 and of semi-planar surfaces, is taken only
// from an even image base, and an image at an odd address reads the pair as two bytes (yuv420_px, yuv_surface_px).
// An image of 16-bit samples is 2-byte aligned (checked on the host, as fp32's rule is); its semi-planar chroma pair is
// one 4-byte load where the pair's address is a multiple of 4 and two 2-byte loads otherwise (yuv_wide_px).  Packed
// 10p / 12p images are read byte by byte and may start anywhere.
#pragma once
#include <type_traits>
#include <variant>
#include "jh_common.h"

namespace jh {

enum { kSrcRgbF32 = 0, kSrcBgrU8 = 1, kSrcI420 = 2, kSrcNV12 = 3, kSrcYuvSurface = 4, kSrcSensor = 5,
       kSrcSensorWide = 6, kSrcYuvWide = 7, kSrcPixels = 8, kSrcCount = 9 };
template <int SRC> constexpr bool kIsYuv = SRC == kSrcI420 || SRC == kSrcNV12 || SRC == kSrcYuvSurface ||
                                           SRC == kSrcYuvWide;
template <int SRC> constexpr bool kIsSensor = SRC == kSrcSensor || SRC == kSrcSensorWide;
// the forms whose pixel is converted once to (R, G, B) bytes for all three channels
template <int SRC> constexpr bool kIsRgb8 = kIsYuv<SRC> || kIsSensor<SRC> || SRC == kSrcPixels;

// The base pointer and the index under which the pixel functions find image n of a launch (see the head of this file).
// cell: the one-pointer cell of a graph replay (or nullptr: `frames` is the base), or with per_image the table.
__device__ __forceinline__ const void* image_base(const void* frames, const void* const* cell, int per_image, int& n) {
  if (per_image) {
    frames = cell[n];
    n = 0;
  }
  return frames;
}

// TONE TABLES (jh_predictor_set_tone): the one place a byte becomes a network input is byte_value below.  A byte form's
// kernels exist in two compile-time variants, chosen by the type of their last argument:
//   NoTone      the plain form, byte * (1/255): an empty class, so these kernels are what they were without tables;
//   ToneTables  the predictor's (cameras, 3, 256) fp32 tables, [camera][0 = R, 1 = G, 2 = B][byte]: image n of a launch
//               is camera cam0 + n % cams (the 3D predictor's images are (t, local camera); the 2D predictor has one
//               table) and byte k of channel ch becomes tables[camera][ch][k].
// of(n) is what the pixel functions take for image n: NoTone again, or the image's own 3 x 256 table (ToneLut).  The
// index is always a byte the conversion clamped to 0 .. 255, so no read leaves the 256 entries whatever the frames hold.
// The lookup goes through the vector cache, not through LDS: 3 KB per camera stay resident, and the stem keeps its LDS.
struct NoTone {
  __host__ __device__ NoTone of(int) const { return NoTone{}; }
};
struct ToneLut { const float* lut; };
struct ToneTables {
  const float* tables;
  int cam0, cams;
  __device__ __forceinline__ ToneLut of(int n) const { return ToneLut{tables + (size_t)(cam0 + n % cams) * 768}; }
};
template <class Tone> constexpr bool kIsTone = !std::is_same_v<Tone, NoTone>;

// the value the pre-processing sees for `byte` (0 .. 255) of channel ch (0 = R, 1 = G, 2 = B)
template <class Tone>
__device__ __forceinline__ float byte_value(int byte, int ch, const Tone& tone) {
  // the reference driver divides on the GPU, where torch evaluates `x / 255.` as
  // x * (1.f / 255.f) (division by a host scalar is a multiplication by its reciprocal)
  if constexpr (kIsTone<Tone>) return tone.lut[ch * 256 + byte];
  else return __fmul_rn((float)byte, __fdiv_rn(1.f, 255.f));
}

template <int SRC, class Tone = NoTone>
__device__ __forceinline__ float frame_px(const void* frames, size_t n, int c, int y, int x, int H,
                                          int W, const Tone& tone = Tone{}) {
  static_assert(SRC == kSrcRgbF32 || SRC == kSrcBgrU8, "frame_px: interleaved / planar RGB formats only");
  static_assert(SRC != kSrcRgbF32 || !kIsTone<Tone>, "tone tables apply to byte frames");
  if (SRC == 0)
    return static_cast<const float*>(frames)[((n * 3 + c) * H + y) * W + x];
  const unsigned char* p = static_cast<const unsigned char*>(frames) + ((n * H + y) * W + x) * 3;
  return byte_value(p[2 - c], c, tone);
}

// BT.601 limited range -> (R, G, B) bytes: the fixed-point arithmetic of OpenCV's
// cvtColor(COLOR_YUV2BGR_I420 / _NV12) (imgproc/src/color_yuv.simd.hpp).  Every partial sum
// stays below 2^30 in magnitude; >> on a negative int is an arithmetic shift.
struct Rgb8 { int r, g, b; };
__host__ __device__ __forceinline__ Rgb8 yuv_to_rgb8(int Y, int U, int V) {
  constexpr int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527;
  constexpr int SHIFT = 20, HALF = 1 << (SHIFT - 1);
  const int u = U - 128, v = V - 128;
  const int yy = (Y > 16 ? Y - 16 : 0) * CY + HALF;
  const auto clamp8 = [](int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); };
  return Rgb8{clamp8((yy + CVR * v) >> SHIFT), clamp8((yy + CVG * v + CUG * u) >> SHIFT),
              clamp8((yy + CUB * u) >> SHIFT)};
}

// pixel (y, x) of YUV 4:2:0 image n (SRC 2 / 3): one Y load and one chroma load (NV12: one
// 2-byte load, or the two bytes when the base is odd; I420: the U and V bytes of the same 2 x 2 block)
template <int SRC>
__device__ __forceinline__ Rgb8 yuv420_px(const void* frames, size_t n, int y, int x, int H, int W) {
  static_assert(SRC == kSrcI420 || SRC == kSrcNV12, "yuv420_px: YUV 4:2:0 formats only");
  const size_t plane = (size_t)H * W;
  const unsigned char* img = static_cast<const unsigned char*>(frames) + n * (plane + plane / 2);
  const int Y = img[(size_t)y * W + x];
  int U, V;
  if (SRC == kSrcNV12) {
    // (an image is H * W * 3 / 2 bytes, a multiple of 2, and the pair offset is even: with an even base the 16-bit
    //  load is aligned.  An odd base -- one image of a per-image table -- takes the two bytes.)
    const unsigned char* pair = img + plane + (size_t)(y >> 1) * W + (x & ~1);
    if (!(reinterpret_cast<uintptr_t>(frames) & 1)) {
      const unsigned short uv = *reinterpret_cast<const unsigned short*>(pair);
      U = uv & 0xff; V = uv >> 8;
    } else {
      U = pair[0]; V = pair[1];
    }
  } else {
    const size_t c = plane + (size_t)(y >> 1) * (W >> 1) + (x >> 1);
    U = img[c]; V = img[c + plane / 4];
  }
  return yuv_to_rgb8(Y, U, V);
}

// A described surface as the kernels take it: the layout of a jh_yuv_surface the host has checked
// (jh_yuv_surface_check) and the fixed-point constants of its (matrix, range).  Passed BY VALUE in the kernel
// arguments: every field is wave-uniform and stays in scalar registers.
struct YuvSurface {
  long long image_stride = 0, y_offset = 0, y_pitch = 0, u_offset = 0, v_offset = 0, c_pitch = 0;
  int c_step = 1;
  int pair = 0;                // c_step == 2 and image_stride even (per image: c_step == 2; every image is image 0 of
                               // its own base): U, V of a block in one 2-byte load, aligned when the base is even
  int y0 = 16, cy = 0, cvr = 0, cub = 0, cug = 0, cvg = 0;
  bool operator==(const YuvSurface& o) const {
    return image_stride == o.image_stride && y_offset == o.y_offset && y_pitch == o.y_pitch &&
           u_offset == o.u_offset && v_offset == o.v_offset && c_pitch == o.c_pitch && c_step == o.c_step &&
           pair == o.pair && y0 == o.y0 && cy == o.cy && cvr == o.cvr && cub == o.cub && cug == o.cug && cvg == o.cvg;
  }
};

// yuv_to_rgb8 with the constants of the surface's (matrix, range): the same scheme, int32 throughout (every
// partial sum of the four constant rows stays below 2^30, tests/test_yuv_surface_cpu.py).  S: a description that
// carries the six constants (YuvSurface and what derives from it, PixelSurface).
template <class S>
__host__ __device__ __forceinline__ Rgb8 yuv_to_rgb8(int Y, int U, int V, const S& s) {
  constexpr int SHIFT = 20, HALF = 1 << (SHIFT - 1);
  const int u = U - 128, v = V - 128;
  const int yy = (Y > s.y0 ? Y - s.y0 : 0) * s.cy + HALF;
  const auto clamp8 = [](int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); };
  return Rgb8{clamp8((yy + s.cvr * v) >> SHIFT), clamp8((yy + s.cvg * v + s.cug * u) >> SHIFT),
              clamp8((yy + s.cub * u) >> SHIFT)};
}

// pixel (y, x) of image n of a described surface (SRC 4): one Y load and, for the 2 x 2 block's chroma, one
// 2-byte load (semi-planar, when the pair is 2-byte aligned: with `pair` every image has the parity of `frames`, which
// per image is the image's own base) or the U and the V byte.
// 64-bit offsets: image_stride * n passes 2^31 at batch scale.  Only plane bytes are ever addressed.
__device__ __forceinline__ Rgb8 yuv_surface_px(const void* frames, size_t n, int y, int x, const YuvSurface& s) {
  const unsigned char* img = static_cast<const unsigned char*>(frames) + (long long)n * s.image_stride;
  const int Y = img[s.y_offset + (long long)y * s.y_pitch + x];
  const long long crow = (long long)(y >> 1) * s.c_pitch;
  int U, V;
  if (s.pair && !(reinterpret_cast<uintptr_t>(frames) & 1)) {
    const bool u_first = s.u_offset < s.v_offset;
    const unsigned short uv = *reinterpret_cast<const unsigned short*>(
        img + (u_first ? s.u_offset : s.v_offset) + crow + (x & ~1));
    U = u_first ? uv & 0xff : uv >> 8; V = u_first ? uv >> 8 : uv & 0xff;
  } else {
    const long long c = crow + (long long)(x >> 1) * s.c_step;
    U = img[s.u_offset + c]; V = img[s.v_offset + c];
  }
  return yuv_to_rgb8(Y, U, V, s);
}

// A raw sensor surface as the kernels take it: the layout of a jh_sensor_surface the host has checked
// (jh_sensor_surface_check) with the image size.  Passed BY VALUE in the kernel arguments, as YuvSurface is: every
// field is wave-uniform and stays in scalar registers.
struct SensorSurface {
  long long image_stride = 0, offset = 0, pitch = 0;
  int pattern = 0;             // JH_SENSOR_*: 0 mono, 1 rggb, 2 bggr, 3 grbg, 4 gbrg
  int h = 0, w = 0;            // Bayer: even and >= 4, so the clamp below has an interior to clamp to
  bool operator==(const SensorSurface& o) const {
    return image_stride == o.image_stride && offset == o.offset && pitch == o.pitch && pattern == o.pattern &&
           h == o.h && w == o.w;
  }
};

// How a sample wider than a byte is stored (the high byte of JH_SAMPLE_*, include/jarvis_hip.h).
enum { kSampleU16 = 1, kSampleP10 = 2, kSampleP12 = 3 };

// The byte of one 16-bit little-endian sample at p (2-byte aligned): min(sample >> shift, 255), shift 0 .. 8.  With
// shift 8 (MSB-aligned data: P010) the byte IS the sample's high byte, one byte load.  shift is wave-uniform.
__device__ __forceinline__ int u16_byte(const unsigned char* p, int shift) {
  if (shift == 8) return p[1];
  return min((int)*reinterpret_cast<const unsigned short*>(p) >> shift, 255);
}

// A raw sensor surface of wide samples (SRC 6): the layout of form 5 -- offset, pitch and image_stride in bytes --
// with how a sample is stored and how far it is shifted down.
struct SensorSurfaceWide : SensorSurface {
  int kind = kSampleU16;       // kSample*
  int shift = 0;               // kSampleU16: 0 .. 8; the packed kinds take the top 8 bits of the n they hold
  bool operator==(const SensorSurfaceWide& o) const {
    return SensorSurface::operator==(o) && kind == o.kind && shift == o.shift;
  }
};

// byte8: sample (y, x) of the wide image whose first sample lies at img, as the byte the demosaic works on.
// 16-bit words: u16_byte (offset, pitch, image_stride and the image base are even: the load is aligned).
// 10p / 12p: a row is a little-endian bit stream B[] starting at img + y * pitch; sample x holds bits
// [n x, n x + n) and its byte is bits [b, b + 8), b = n x + n - 8.  With k = b >> 3, r = b & 7 that is
// ((B[k] | B[k+1] << 8) >> r) & 0xff, and B[k+1] is loaded only when r != 0: then bit b + 7 = n x + n - 1, the
// sample's own top bit, lies in byte k + 1 = (n x + n - 1) >> 3 <= (n w - 1) >> 3 < ceil(n w / 8) = row_bytes(w), so
// no byte that holds no sample bit is addressed -- for the last sample of a row too, whatever w % 4 (10p: r = 2, 4,
// 6, 0 for x % 4 = 0 .. 3) or the parity of w (12p: r = 4 for even x, 0 for odd x).  When r == 0 byte k is the
// sample's last byte and B[k+1], which may be the next row's or nobody's, is left alone.  The & 0xff drops whatever
// lies above the sample in B[k+1]: the next sample, or the unused high bits of the row's last byte.
__device__ __forceinline__ int byte8(const unsigned char* img, int y, int x, const SensorSurfaceWide& s) {
  const unsigned char* row = img + (long long)y * s.pitch;
  if (s.kind == kSampleU16) return u16_byte(row + 2 * (long long)x, s.shift);
  const int n = s.kind == kSampleP10 ? 10 : 12;
  const int b = n * x + (n - 8), k = b >> 3, r = b & 7;
  int v = row[k];
  if (r) v |= row[k + 1] << 8;
  return (v >> r) & 0xff;
}

// pixel (y, x) of raw image n (SRC 5).  mono: the byte, three times.  Bayer: the bilinear demosaic defined in
// include/jarvis_hip.h -- a border pixel takes the RGB of the interior pixel it clamps to, so the 3 x 3 neighbourhood
// never leaves the h x w samples; then, by the parity of the site against the pattern, a green site reads 5 bytes
// (itself, W E, N S) and a red or blue site 9.  64-bit offsets, as yuv_surface_px.
__device__ __forceinline__ Rgb8 sensor_px(const void* frames, size_t n, int y, int x, const SensorSurface& s) {
  const unsigned char* img = static_cast<const unsigned char*>(frames) + (long long)n * s.image_stride + s.offset;
  if (s.pattern == 0) {
    const int v = img[(long long)y * s.pitch + x];
    return Rgb8{v, v, v};
  }
  y = min(max(y, 1), s.h - 2);
  x = min(max(x, 1), s.w - 2);
  const unsigned char* c = img + (long long)y * s.pitch + x;
  const long long p = s.pitch;
  // red sits at (ry, rx) of the top-left cell: rggb (0,0), bggr (1,1), grbg (0,1), gbrg (1,0)
  const int ry = s.pattern == 2 || s.pattern == 4, rx = s.pattern == 2 || s.pattern == 3;
  const int py = (y & 1) ^ ry, px = (x & 1) ^ rx;       // (0,0): red site, (1,1): blue site, else green
  const int own = c[0];
  if (py == px) {
    const int g = (c[-p] + c[p] + c[1] + c[-1] + 2) >> 2;
    const int opp = (c[-p - 1] + c[-p + 1] + c[p - 1] + c[p + 1] + 2) >> 2;
    return py == 0 ? Rgb8{own, g, opp} : Rgb8{opp, g, own};
  }
  const int lr = (c[-1] + c[1] + 1) >> 1, ab = (c[-p] + c[p] + 1) >> 1;
  // a green site of a red row (py == 0) has red left and right, blue above and below; of a blue row the reverse
  return py == 0 ? Rgb8{lr, own, ab} : Rgb8{ab, own, lr};
}

// The same pixel of a wide image (SRC 6): the clamp, the sites and the sums of the function above, every sample taken
// through byte8.  (Its own body, not a template over both: form 5 addresses its neighbours from the centre byte's
// pointer, and a shared body did not keep the instructions of its kernels.)
__device__ __forceinline__ Rgb8 sensor_px(const void* frames, size_t n, int y, int x, const SensorSurfaceWide& s) {
  const unsigned char* img = static_cast<const unsigned char*>(frames) + (long long)n * s.image_stride + s.offset;
  if (s.pattern == 0) {
    const int v = byte8(img, y, x, s);
    return Rgb8{v, v, v};
  }
  y = min(max(y, 1), s.h - 2);
  x = min(max(x, 1), s.w - 2);
  const auto at = [&](int dy, int dx) { return byte8(img, y + dy, x + dx, s); };
  const int ry = s.pattern == 2 || s.pattern == 4, rx = s.pattern == 2 || s.pattern == 3;
  const int py = (y & 1) ^ ry, px = (x & 1) ^ rx;
  const int own = at(0, 0);
  if (py == px) {
    const int g = (at(-1, 0) + at(1, 0) + at(0, 1) + at(0, -1) + 2) >> 2;
    const int opp = (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2;
    return py == 0 ? Rgb8{own, g, opp} : Rgb8{opp, g, own};
  }
  const int lr = (at(0, -1) + at(0, 1) + 1) >> 1, ab = (at(-1, 0) + at(1, 0) + 1) >> 1;
  return py == 0 ? Rgb8{lr, own, ab} : Rgb8{ab, own, lr};
}

// A described surface of 16-bit samples (SRC 7): the fields of form 4 -- offsets and pitches in bytes, c_step in
// samples, `pair` unused -- and the shift that reduces a sample.
struct YuvSurfaceWide : YuvSurface {
  int shift = 0;               // 0 .. 8
  bool operator==(const YuvSurfaceWide& o) const { return YuvSurface::operator==(o) && shift == o.shift; }
};

// pixel (y, x) of image n of a 16-bit surface: one Y load and, for the block's chroma, the two samples of a
// semi-planar pair in ONE 4-byte load where the pair's address is a multiple of 4 -- its offset in the image is one
// (jh_yuv_surface_check), so that is every image whose base is a multiple of 4 --, in two 2-byte loads otherwise;
// planar: the U and the V sample.  Every sample becomes a byte (u16_byte) before the conversion of form 4.
__device__ __forceinline__ Rgb8 yuv_wide_px(const void* frames, size_t n, int y, int x, const YuvSurfaceWide& s) {
  const unsigned char* img = static_cast<const unsigned char*>(frames) + (long long)n * s.image_stride;
  const int Y = u16_byte(img + s.y_offset + (long long)y * s.y_pitch + 2 * (long long)x, s.shift);
  const long long crow = (long long)(y >> 1) * s.c_pitch;
  int U, V;
  if (s.c_step == 2) {
    const bool u_first = s.u_offset < s.v_offset;
    const unsigned char* pair = img + (u_first ? s.u_offset : s.v_offset) + crow + 2 * (long long)(x & ~1);
    int a, b;                                           // the pair's first and second sample, reduced
    if (!(reinterpret_cast<uintptr_t>(pair) & 3)) {
      const unsigned int uv = *reinterpret_cast<const unsigned int*>(pair);
      a = min((int)(uv & 0xffffu) >> s.shift, 255); b = min((int)(uv >> 16) >> s.shift, 255);
    } else {
      a = u16_byte(pair, s.shift); b = u16_byte(pair + 2, s.shift);
    }
    U = u_first ? a : b; V = u_first ? b : a;
  } else {
    const long long c = crow + 2 * (long long)(x >> 1);
    U = u16_byte(img + s.u_offset + c, s.shift); V = u16_byte(img + s.v_offset + c, s.shift);
  }
  return yuv_to_rgb8(Y, U, V, s);
}

// A described pixel surface as the kernels take it (SRC 8): the address rules of a jh_pixel_surface the host has checked
// (jh_pixel_surface_check) and, for Y U V components, the fixed-point constants of its (matrix, range) -- the table of
// form 4.  Passed BY VALUE in the kernel arguments, as YuvSurface is: every field is wave-uniform and stays in scalar
// registers (the arrays are only ever indexed by constants).
struct PixelSurface {
  long long image_stride = 0;
  long long offset[3] = {0, 0, 0}, pitch[3] = {0, 0, 0};
  int step[3] = {1, 1, 1}, xs[3] = {0, 0, 0}, ys[3] = {0, 0, 0};
  int yuv = 0;                 // components are Y U V (JH_PIXEL_YUV): convert; else they are R G B
  int y0 = 16, cy = 0, cvr = 0, cub = 0, cug = 0, cvg = 0;
  float bytes = 3.f;           // distinct component bytes per pixel (FrameSource::px_bytes), computed once on the host
  bool operator==(const PixelSurface& o) const {
    for (int k = 0; k < 3; ++k)
      if (offset[k] != o.offset[k] || pitch[k] != o.pitch[k] || step[k] != o.step[k] || xs[k] != o.xs[k] ||
          ys[k] != o.ys[k]) return false;
    return image_stride == o.image_stride && yuv == o.yuv && y0 == o.y0 && cy == o.cy && cvr == o.cvr &&
           cub == o.cub && cug == o.cug && cvg == o.cvg && bytes == o.bytes;
  }
};

// pixel (y, x) of image n of a described pixel surface: three byte loads, component k at
// offset[k] + (y >> ys[k]) * pitch[k] + (x >> xs[k]) * step[k] -- inside [0, image_stride) for every (y, x) of the
// h x w image the description was checked for.  64-bit offsets, as yuv_surface_px.  The branch on `yuv` is wave-uniform.
// (One 4-byte load for the layouts whose three bytes share an aligned word -- BGRA, YUYV -- was measured and gained
//  nothing over the byte loads: DESIGN.md 3.15e.)
__device__ __forceinline__ Rgb8 pixels_px(const void* frames, size_t n, int y, int x, const PixelSurface& s) {
  const unsigned char* img = static_cast<const unsigned char*>(frames) + (long long)n * s.image_stride;
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = img[s.offset[k] + (long long)(y >> s.ys[k]) * s.pitch[k] + (long long)(x >> s.xs[k]) * s.step[k]];
  if (s.yuv) return yuv_to_rgb8(c[0], c[1], c[2], s);
  return Rgb8{c[0], c[1], c[2]};
}

// The description a kernel of source form SRC takes by value: the surface of the five described forms, nothing (an
// empty class) for the four whose layout follows from (H, W).
template <int SRC> struct SrcDesc {
  bool operator==(const SrcDesc&) const { return true; }
};
template <> struct SrcDesc<kSrcYuvSurface> : YuvSurface {};
template <> struct SrcDesc<kSrcSensor> : SensorSurface {};
template <> struct SrcDesc<kSrcSensorWide> : SensorSurfaceWide {};
template <> struct SrcDesc<kSrcYuvWide> : YuvSurfaceWide {};
template <> struct SrcDesc<kSrcPixels> : PixelSurface {};

// pixel (y, x) of image n as (R, G, B) bytes: the forms that convert once for all three channels
template <int SRC>
__device__ __forceinline__ Rgb8 rgb8_px(const void* frames, size_t n, int y, int x, int H, int W,
                                        const SrcDesc<SRC>& d) {
  static_assert(kIsRgb8<SRC>, "rgb8_px: YUV, raw sensor and pixel-surface formats only");
  if constexpr (kIsSensor<SRC>) return sensor_px(frames, n, y, x, d);
  else if constexpr (SRC == kSrcPixels) return pixels_px(frames, n, y, x, d);
  else if constexpr (SRC == kSrcYuvSurface) return yuv_surface_px(frames, n, y, x, d);
  else if constexpr (SRC == kSrcYuvWide) return yuv_wide_px(frames, n, y, x, d);
  else return yuv420_px<SRC>(frames, n, y, x, H, W);
}

// the three channels (r, g, b) of one pixel as the uint8 path scales them; YUV and raw sensor forms: one conversion
// for all three channels
template <int SRC, class Tone = NoTone>
__device__ __forceinline__ void frame_px3(const void* frames, size_t n, int y, int x, int H, int W,
                                          const SrcDesc<SRC>& d, float v[3], const Tone& tone = Tone{}) {
  if constexpr (kIsRgb8<SRC>) {
    const Rgb8 p = rgb8_px<SRC>(frames, n, y, x, H, W, d);
    v[0] = byte_value(p.r, 0, tone); v[1] = byte_value(p.g, 1, tone); v[2] = byte_value(p.b, 2, tone);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = frame_px<SRC>(frames, n, c, y, x, H, W, tone);
  }
}

// pixel (oy, ox) of the S x S resized + normalised image n: torchvision tensor resize (bilinear,
// align_corners = False, no antialias), then (x - mean) / std; (r, g, b, 0)
template <int SRC, class Tone = NoTone>
__device__ __forceinline__ float4 resize_px(const void* frames, int n, int oy, int ox, int H, int W, float sy,
                                            float sx, float3 mean, float3 stdv, const SrcDesc<SRC>& d,
                                            const Tone& tone = Tone{}) {
  float ry = fmaxf(__fsub_rn(__fmul_rn(sy, __fadd_rn((float)oy, 0.5f)), 0.5f), 0.f);
  float rx = fmaxf(__fsub_rn(__fmul_rn(sx, __fadd_rn((float)ox, 0.5f)), 0.5f), 0.f);
  int y0 = min((int)floorf(ry), H - 1), x0 = min((int)floorf(rx), W - 1);
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fminf(fmaxf(__fsub_rn(ry, (float)y0), 0.f), 1.f), ly0 = __fsub_rn(1.f, ly1);
  const float lx1 = fminf(fmaxf(__fsub_rn(rx, (float)x0), 0.f), 1.f), lx0 = __fsub_rn(1.f, lx1);
  const float mv[3] = {mean.x, mean.y, mean.z}, sv[3] = {stdv.x, stdv.y, stdv.z};
  float r[3];
  // YUV: each of the four taps is converted once for all three channels (the per-channel arithmetic
  // below is that of the uint8 path, so the result equals SRC 1 on the converted bytes bit for bit)
  float q00[3], q01[3], q10[3], q11[3];
  if constexpr (kIsRgb8<SRC>) {
    frame_px3<SRC>(frames, n, y0, x0, H, W, d, q00, tone); frame_px3<SRC>(frames, n, y0, x1, H, W, d, q01, tone);
    frame_px3<SRC>(frames, n, y1, x0, H, W, d, q10, tone); frame_px3<SRC>(frames, n, y1, x1, H, W, d, q11, tone);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float p00, p01, p10, p11;
    if constexpr (kIsRgb8<SRC>) {
      p00 = q00[c]; p01 = q01[c]; p10 = q10[c]; p11 = q11[c];
    } else {
      p00 = frame_px<SRC>(frames, n, c, y0, x0, H, W, tone); p01 = frame_px<SRC>(frames, n, c, y0, x1, H, W, tone);
      p10 = frame_px<SRC>(frames, n, c, y1, x0, H, W, tone); p11 = frame_px<SRC>(frames, n, c, y1, x1, H, W, tone);
    }
    const float a = __fmaf_rn(p00, lx0, __fmul_rn(p01, lx1));
    const float b = __fmaf_rn(p10, lx0, __fmul_rn(p11, lx1));
    const float v = __fmaf_rn(a, ly0, __fmul_rn(b, ly1));
    r[c] = __fdiv_rn(__fsub_rn(v, mv[c]), sv[c]);
  }
  return make_float4(r[0], r[1], r[2], 0.f);
}

// pixel (oy, ox) of the B x B crop of image n around (cx, cy), normalised; pixels of the window that
// lie outside the frame are 0 BEFORE the normalisation (jarvis3D.py:168-178 never leaves the frame: the
// crop centre is clamped; kept for safety as the stand-alone kernel has it)
template <int SRC, class Tone = NoTone>
__device__ __forceinline__ float4 crop_px(const void* frames, int n, int cx, int cy, int oy, int ox, int H,
                                          int W, int B, float3 mean, float3 stdv, const SrcDesc<SRC>& d,
                                          const Tone& tone = Tone{}) {
  const int hw = B / 2;
  const int ix = cx - hw + ox, iy = cy - hw + oy;
  const float mv[3] = {mean.x, mean.y, mean.z}, sv[3] = {stdv.x, stdv.y, stdv.z};
  float r[3];
  const bool ok = ix >= 0 && ix < W && iy >= 0 && iy < H;
  if constexpr (kIsRgb8<SRC>) {
    // (outside the frame: 0 before the normalisation, as for the other formats -- not the conversion of Y = U = V = 0)
    float q[3] = {0.f, 0.f, 0.f};
    if (ok) frame_px3<SRC>(frames, n, iy, ix, H, W, d, q, tone);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = __fdiv_rn(__fsub_rn(q[c], mv[c]), sv[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = ok ? frame_px<SRC>(frames, n, c, iy, ix, H, W, tone) : 0.f;
      r[c] = __fdiv_rn(__fsub_rn(v, mv[c]), sv[c]);
    }
  }
  return make_float4(r[0], r[1], r[2], 0.f);
}

// ---------------------------------------------------------------------------------------------------- host side
// Where a call's frames come from: the format code and the description that format has.  Built (and validated) by the
// frame_source constructors of api_frames.hip; everything between the C entry point and a kernel launch takes this.
struct FrameSource {
  int fmt = kSrcRgbF32;                                                                  // kSrc*
  std::variant<std::monostate, SrcDesc<kSrcYuvSurface>, SrcDesc<kSrcSensor>, SrcDesc<kSrcSensorWide>,
               SrcDesc<kSrcYuvWide>, SrcDesc<kSrcPixels>> desc;                          // monostate: fmt needs none
  bool per_image = false;      // the launches read a table of one device pointer per image instead of one base
  // Tone tables in force (nullptr: the plain form): the predictor's device buffer, and which of its cameras image n of
  // a launch is (ToneTables).  Part of the description, so a recorded graph is recorded again when tables are switched
  // on or off; their VALUES live in the buffer and may change under one recording.
  const float* tone = nullptr;
  int tone_cam0 = 0, tone_cams = 1;
  bool operator==(const FrameSource& o) const {
    return fmt == o.fmt && desc == o.desc && per_image == o.per_image && tone == o.tone && tone_cam0 == o.tone_cam0 &&
           tone_cams == o.tone_cams;
  }
  bool operator!=(const FrameSource& o) const { return !(*this == o); }
  // bytes of frame data per source pixel: fp32 RGB 12, uint8 BGR 3, YUV 4:2:0 1.5 (16-bit: 3), raw sensor 1 (16-bit
  // words 2, 10p 1.25, 12p 1.5), a pixel surface the distinct component bytes of its description
  double px_bytes() const {
    if (const auto* p = std::get_if<SrcDesc<kSrcPixels>>(&desc)) return p->bytes;
    if (const auto* w = std::get_if<SrcDesc<kSrcSensorWide>>(&desc))
      return w->kind == kSampleU16 ? 2.0 : w->kind == kSampleP10 ? 1.25 : 1.5;
    return fmt == kSrcRgbF32 ? 12.0 : fmt == kSrcBgrU8 ? 3.0 : fmt == kSrcSensor ? 1.0 : fmt == kSrcYuvWide ? 3.0 : 1.5;
  }
};

// The one place a run-time format code becomes a template argument: f(SrcTag<SRC>{}, const SrcDesc<SRC>&, tone) -> int
// for the form src holds, tone being NoTone{} or the ToneTables of src.tone; an unknown code, a described form without
// its description, or tables with fp32 frames (which have no byte) is an error.  A caller that has no tone form may
// pass f(tag, desc): it is then called for sources without tables only.
template <int SRC> using SrcTag = std::integral_constant<int, SRC>;
template <class F>
int dispatch_src(const FrameSource& src, F&& f) {
  const auto row = [&](auto tag) -> int {
    constexpr int SRC = decltype(tag)::value;
    const auto with_tone = [&](const SrcDesc<SRC>& d) -> int {
      if constexpr (!std::is_invocable_v<F&, decltype(tag), const SrcDesc<SRC>&, NoTone>) {
        JH_REQUIRE(!src.tone, "this launch has no tone form");
        return f(tag, d);
      } else if (!src.tone) {
        return f(tag, d, NoTone{});
      } else if constexpr (SRC == kSrcRgbF32) {
        set_error("tone tables apply to byte frames");
        return 1;
      } else {
        JH_REQUIRE(src.tone_cams >= 1 && src.tone_cam0 >= 0, "tone tables: camera range");
        return f(tag, d, ToneTables{src.tone, src.tone_cam0, src.tone_cams});
      }
    };
    if constexpr (std::is_empty_v<SrcDesc<SRC>>) {
      return with_tone(SrcDesc<SRC>{});
    } else {
      const SrcDesc<SRC>* d = std::get_if<SrcDesc<SRC>>(&src.desc);
      JH_REQUIRE(d, "a described surface comes with its own frame format");
      return with_tone(*d);
    }
  };
  switch (src.fmt) {
    case kSrcRgbF32: return row(SrcTag<kSrcRgbF32>{});
    case kSrcBgrU8: return row(SrcTag<kSrcBgrU8>{});
    case kSrcI420: return row(SrcTag<kSrcI420>{});
    case kSrcNV12: return row(SrcTag<kSrcNV12>{});
    case kSrcYuvSurface: return row(SrcTag<kSrcYuvSurface>{});
    case kSrcSensor: return row(SrcTag<kSrcSensor>{});
    case kSrcSensorWide: return row(SrcTag<kSrcSensorWide>{});
    case kSrcYuvWide: return row(SrcTag<kSrcYuvWide>{});
    case kSrcPixels: return row(SrcTag<kSrcPixels>{});
  }
  set_error("requirement failed: src.fmt is no kSrc* code (frame format)");
  return 1;
}

// What the stem convolution reads when the pre-processing is fused into its patch staging.
struct StemSource {
  int mode = 0;               // 0: the plan's own input tensor; 1: resize of the frames; 2: crop of the frames
  const void* frames = nullptr;
  const void* const* frames_cell = nullptr;    // graph replays: the frame pointer of the current call; with
                                               // source.per_image: the table of N image pointers (always set)
  FrameSource source;                          // the form of the frames and its description
  const int* center_hm = nullptr;              // crop: [T][C][2]
  int Cloc = 0, C = 0, cam0 = 0;               // crop: image n = (t, local camera)
  int H = 0, W = 0;                            // frame size
  float mean[3] = {0, 0, 0}, stdv[3] = {1, 1, 1};
};

// The stand-alone kernels (preprocess.hip).
// (frames_cell: the one-pointer cell of a graph replay, or nullptr; with src.per_image the table of N image pointers,
//  which must then be given -- image_base)
int launch_preprocess_resize(const void* frames, const FrameSource& src, float* out, int N, int H, int W, int S,
                             const float* mean, const float* stdv, hipStream_t s,
                             const void* const* frames_cell = nullptr);
int launch_preprocess_crop(const void* frames, const FrameSource& src, const int* center_hm, float* out, int T,
                           int Cloc, int C, int cam0, int H, int W, int B, const float* mean,
                           const float* stdv, hipStream_t s, const void* const* frames_cell = nullptr);
int launch_frames_to_bgr(const void* frames, const FrameSource& src, unsigned char* out, int N, int H, int W,
                         hipStream_t s);
// the values the fetch sees, [N][3][H][W] fp32, under src's tone tables (or none): the unit-test form of byte_value
int launch_frames_to_rgb_f32(const void* frames, const FrameSource& src, float* out, int N, int H, int W,
                             hipStream_t s);

}  // namespace jh
