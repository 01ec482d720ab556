// C ABI, the frame descriptions: the one validation of each described surface, the FrameSource every entry point hands
// to the kernels (preprocess.h), the pointer table of a per-image call, and the conversion operators.
#include "predictor.h"
#include "preprocess.h"

using namespace jh;

// A sample code (JH_SAMPLE_*) taken apart: kind 0 = one byte, else kSample* of preprocess.h; shift of the 16-bit words.
// Any value that is no code -- 1 in particular, or a shift above 8 -- gives kind -1.
struct SampleCode { int kind, shift; };
static SampleCode sample_code(int32_t code) {
  if (code == JH_SAMPLE_U8) return {0, 0};
  if (code >= JH_SAMPLE_U16(0) && code <= JH_SAMPLE_U16(8)) return {kSampleU16, code & 0xff};
  if (code == JH_SAMPLE_P10) return {kSampleP10, 2};
  if (code == JH_SAMPLE_P12) return {kSampleP12, 4};
  return {-1, 0};
}

// The one validation of a described YUV 4:2:0 surface of h x w images (include/jarvis_hip.h): every surface entry
// point and jh_yuv_surface_check.  Host arithmetic only.  (__int128: a plane's end may not wrap for any int64 field.)
// sb: bytes per sample; offsets and pitches are in bytes, c_step in samples.
static int yuv_surface_check(const jh_yuv_surface* sp, int h, int w) {
  JH_REQUIRE(sp, "null jh_yuv_surface");
  const jh_yuv_surface& q = *sp;
  JH_REQUIRE(h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "YUV 4:2:0 frames need an even, positive height and width");
  const SampleCode sc = sample_code(q.sample);
  JH_REQUIRE(sc.kind == 0 || sc.kind == kSampleU16, "jh_yuv_surface.sample (the reserved word of earlier headers) must "
             "be JH_SAMPLE_U8 or JH_SAMPLE_U16(shift) with shift 0 .. 8");
  const int sb = sc.kind == kSampleU16 ? 2 : 1;
  JH_REQUIRE(q.c_step == 1 || q.c_step == 2, "jh_yuv_surface.c_step must be 1 (planar) or 2 (semi-planar)");
  JH_REQUIRE(q.y_pitch >= (int64_t)w * sb, "jh_yuv_surface.y_pitch is smaller than the width");
  JH_REQUIRE(q.c_pitch >= (int64_t)(w / 2) * q.c_step * sb, "jh_yuv_surface.c_pitch is smaller than a chroma row");
  JH_REQUIRE(q.y_offset >= 0 && q.u_offset >= 0 && q.v_offset >= 0 && q.image_stride >= 0,
             "jh_yuv_surface offsets must not be negative");
  if (q.c_step == 2) {
    JH_REQUIRE(q.u_offset - q.v_offset == sb || q.v_offset - q.u_offset == sb,
               "jh_yuv_surface: semi-planar U and V are neighbouring samples");
    JH_REQUIRE((q.u_offset < q.v_offset ? q.u_offset : q.v_offset) % (2 * sb) == 0 && q.c_pitch % (2 * sb) == 0,
               "jh_yuv_surface: a semi-planar chroma pair starts at an even offset and c_pitch is even (16-bit "
               "samples: multiples of 4)");
  }
  if (sb == 2)
    JH_REQUIRE(q.image_stride % 2 == 0 && q.y_offset % 2 == 0 && q.y_pitch % 2 == 0 && q.u_offset % 2 == 0 &&
                   q.v_offset % 2 == 0 && q.c_pitch % 2 == 0,
               "jh_yuv_surface: 16-bit samples need even offsets, pitches and image_stride");
  const __int128 y_end = (__int128)q.y_offset + (__int128)(h - 1) * q.y_pitch + (__int128)w * sb;
  const __int128 c_span = (__int128)(h / 2 - 1) * q.c_pitch + ((__int128)(w / 2 - 1) * q.c_step + 1) * sb;
  JH_REQUIRE(y_end <= q.image_stride && q.u_offset + c_span <= q.image_stride && q.v_offset + c_span <= q.image_stride,
             "jh_yuv_surface: a plane ends beyond image_stride");
  JH_REQUIRE(q.matrix == JH_YUV_BT601 || q.matrix == JH_YUV_BT709, "jh_yuv_surface.matrix: unknown");
  JH_REQUIRE(q.range == JH_YUV_LIMITED || q.range == JH_YUV_FULL, "jh_yuv_surface.range: unknown");
  return 0;
}

// The fixed-point constants of a checked (matrix, range) into a description that carries them (YuvSurface,
// PixelSurface): {Y0, CY, CVR, CUB, CUG, CVG}.  BT.601 limited = OpenCV's literals (yuv_to_rgb8); the others
// round(x * 2^20) of the float64 matrix (include/jarvis_hip.h)
template <class S>
static void yuv_constants(int matrix, int range, S& a) {
  static const int k[2][2][6] = {{{16, 1220542, 1673527, 2116026, -409993, -852492},
                                  {0, 1048576, 1470104, 1858077, -360853, -748826}},
                                 {{16, 1220945, 1879825, 2215014, -223607, -558796},
                                  {0, 1048576, 1651297, 1945738, -196424, -490864}}};
  const int* c = k[matrix][range];
  a.y0 = c[0]; a.cy = c[1]; a.cvr = c[2]; a.cub = c[3]; a.cug = c[4]; a.cvg = c[5];
}

// FrameSource of a described YUV 4:2:0 surface of h x w images: the check above, then the description as the kernels
// take it (preprocess.h) -- the layout and the constants of its (matrix, range)
int jh::frame_source(const jh_yuv_surface* sp, int h, int w, FrameSource* out) {
  if (yuv_surface_check(sp, h, w)) return 1;
  const jh_yuv_surface& q = *sp;
  const auto fill = [&](YuvSurface& a) {
    a.image_stride = q.image_stride; a.y_offset = q.y_offset; a.y_pitch = q.y_pitch;
    a.u_offset = q.u_offset; a.v_offset = q.v_offset; a.c_pitch = q.c_pitch; a.c_step = q.c_step;
    yuv_constants(q.matrix, q.range, a);
  };
  // the sample code chooses the form: 16-bit samples are kSrcYuvWide, kernels of their own
  if (const SampleCode sc = sample_code(q.sample); sc.kind == kSampleU16) {
    SrcDesc<kSrcYuvWide> a;
    fill(a);
    a.shift = sc.shift;
    out->fmt = kSrcYuvWide; out->desc = a;
    return 0;
  }
  SrcDesc<kSrcYuvSurface> a;
  fill(a);
  a.pair = q.c_step == 2 && q.image_stride % 2 == 0;
  out->fmt = kSrcYuvSurface; out->desc = a;
  return 0;
}

// The one validation of a raw sensor surface of h x w images (include/jarvis_hip.h): every sensor entry point and
// jh_sensor_surface_check.  Host arithmetic only.
static int sensor_surface_check(const jh_sensor_surface* sp, int h, int w) {
  JH_REQUIRE(sp, "null jh_sensor_surface");
  const jh_sensor_surface& q = *sp;
  JH_REQUIRE(h > 0 && w > 0, "raw sensor frames need a positive height and width");
  JH_REQUIRE(q.pattern >= JH_SENSOR_MONO && q.pattern <= JH_SENSOR_GBRG, "jh_sensor_surface.pattern: unknown");
  if (q.pattern != JH_SENSOR_MONO)
    JH_REQUIRE(h % 2 == 0 && w % 2 == 0 && h >= 4 && w >= 4,
               "Bayer frames need an even height and width of at least 4");
  const SampleCode sc = sample_code(q.sample);
  JH_REQUIRE(sc.kind >= 0, "jh_sensor_surface.sample (the reserved word of earlier headers) must be JH_SAMPLE_U8, "
             "JH_SAMPLE_U16(shift) with shift 0 .. 8, JH_SAMPLE_P10 or JH_SAMPLE_P12");
  // bytes the w samples of a row occupy: w, 2 w, ceil(10 w / 8), ceil(12 w / 8)
  const int64_t row = sc.kind == 0 ? w : sc.kind == kSampleU16 ? 2 * (int64_t)w
                      : ((sc.kind == kSampleP10 ? 10 : 12) * (int64_t)w + 7) / 8;
  JH_REQUIRE(q.pitch >= row, "jh_sensor_surface.pitch is smaller than the width (the bytes of a row of samples)");
  JH_REQUIRE(q.offset >= 0, "jh_sensor_surface.offset must not be negative");
  JH_REQUIRE((__int128)q.offset + (__int128)(h - 1) * q.pitch + row <= q.image_stride,
             "jh_sensor_surface: the image ends beyond image_stride");
  if (sc.kind == kSampleU16)
    JH_REQUIRE(q.offset % 2 == 0 && q.pitch % 2 == 0 && q.image_stride % 2 == 0,
               "jh_sensor_surface: 16-bit samples need an even offset, pitch and image_stride");
  return 0;
}

// FrameSource of a raw sensor surface of h x w images: the check above, then the description as the kernels take it
int jh::frame_source(const jh_sensor_surface* sp, int h, int w, FrameSource* out) {
  if (sensor_surface_check(sp, h, w)) return 1;
  const jh_sensor_surface& q = *sp;
  const auto fill = [&](SensorSurface& a) {
    a.image_stride = q.image_stride; a.offset = q.offset; a.pitch = q.pitch; a.pattern = q.pattern; a.h = h; a.w = w;
  };
  // the sample code chooses the form: anything wider than a byte is kSrcSensorWide, kernels of their own
  if (const SampleCode sc = sample_code(q.sample); sc.kind != 0) {
    SrcDesc<kSrcSensorWide> a;
    fill(a);
    a.kind = sc.kind; a.shift = sc.shift;
    out->fmt = kSrcSensorWide; out->desc = a;
    return 0;
  }
  SrcDesc<kSrcSensor> a;
  fill(a);
  out->fmt = kSrcSensor; out->desc = a;
  return 0;
}

// The one validation of a described pixel surface of h x w images (include/jarvis_hip.h): every pixel entry point and
// jh_pixel_surface_check.  Host arithmetic only.  (__int128: a component's last byte may not wrap for any int64 field.)
static int pixel_surface_check(const jh_pixel_surface* sp, int h, int w) {
  JH_REQUIRE(sp, "null jh_pixel_surface");
  const jh_pixel_surface& q = *sp;
  JH_REQUIRE(h > 0 && w > 0, "pixel surfaces need a positive height and width");
  JH_REQUIRE(q.colour == JH_PIXEL_RGB || q.colour == JH_PIXEL_YUV, "jh_pixel_surface.colour: unknown");
  if (q.colour == JH_PIXEL_YUV) {
    JH_REQUIRE(q.matrix == JH_YUV_BT601 || q.matrix == JH_YUV_BT709, "jh_pixel_surface.matrix: unknown");
    JH_REQUIRE(q.range == JH_YUV_LIMITED || q.range == JH_YUV_FULL, "jh_pixel_surface.range: unknown");
  } else {
    JH_REQUIRE(q.matrix == 0 && q.range == 0, "jh_pixel_surface: matrix and range must be 0 for JH_PIXEL_RGB");
  }
  JH_REQUIRE(q.sample == JH_SAMPLE_U8, "jh_pixel_surface.sample must be JH_SAMPLE_U8");
  for (int k = 0; k < 3; ++k)
    JH_REQUIRE(q.step[k] >= 1 && q.step[k] <= 8, "jh_pixel_surface.step must be 1 .. 8");
  for (int k = 0; k < 3; ++k)
    JH_REQUIRE(q.xs[k] >= 0 && q.xs[k] <= 2 && q.ys[k] >= 0 && q.ys[k] <= 2, "jh_pixel_surface.xs and ys must be 0 .. 2");
  if (q.colour == JH_PIXEL_RGB) {
    for (int k = 0; k < 3; ++k)
      JH_REQUIRE(q.xs[k] == 0 && q.ys[k] == 0, "jh_pixel_surface: R, G and B are not subsampled (xs and ys must be 0)");
  } else {
    JH_REQUIRE(q.xs[0] == 0 && q.ys[0] == 0 && q.xs[1] == q.xs[2] && q.ys[1] == q.ys[2],
               "jh_pixel_surface: Y is not subsampled, and U and V are subsampled alike");
  }
  for (int k = 0; k < 3; ++k) JH_REQUIRE(q.offset[k] >= 0, "jh_pixel_surface.offset must not be negative");
  for (int k = 0; k < 3; ++k)
    JH_REQUIRE(q.pitch[k] >= (int64_t)((w - 1) >> q.xs[k]) * q.step[k] + 1,
               "jh_pixel_surface.pitch is smaller than a row of the component");
  for (int k = 0; k < 3; ++k)
    JH_REQUIRE((__int128)q.offset[k] + (__int128)((h - 1) >> q.ys[k]) * q.pitch[k] +
                       (__int128)((w - 1) >> q.xs[k]) * q.step[k] + 1 <= q.image_stride,
               "jh_pixel_surface: a component ends beyond image_stride");
  return 0;
}

// FrameSource of a described pixel surface of h x w images: the check above, then the description as the kernels take
// it -- the address rules, for Y U V the constants of its (matrix, range), and the distinct component bytes per pixel
// (components that share one address rule, as the three of a grey image do, count once)
int jh::frame_source(const jh_pixel_surface* sp, int h, int w, FrameSource* out) {
  if (pixel_surface_check(sp, h, w)) return 1;
  const jh_pixel_surface& q = *sp;
  SrcDesc<kSrcPixels> a;
  a.image_stride = q.image_stride;
  a.bytes = 0.f;
  for (int k = 0; k < 3; ++k) {
    a.offset[k] = q.offset[k]; a.pitch[k] = q.pitch[k]; a.step[k] = q.step[k]; a.xs[k] = q.xs[k]; a.ys[k] = q.ys[k];
    bool seen = false;
    for (int j = 0; j < k; ++j)
      seen = seen || (q.offset[j] == q.offset[k] && q.pitch[j] == q.pitch[k] && q.step[j] == q.step[k] &&
                      q.xs[j] == q.xs[k] && q.ys[j] == q.ys[k]);
    if (!seen) a.bytes += 1.f / (float)(1 << (q.xs[k] + q.ys[k]));
  }
  a.yuv = q.colour == JH_PIXEL_YUV;
  if (a.yuv) yuv_constants(q.matrix, q.range, a);
  out->fmt = kSrcPixels; out->desc = a;
  return 0;
}

static_assert(JH_FRAME_RGB_F32 == kSrcRgbF32 && JH_FRAME_BGR_U8 == kSrcBgrU8 && JH_FRAME_I420 == kSrcI420 &&
                  JH_FRAME_NV12 == kSrcNV12, "frame format codes of the C ABI are preprocess.h's SRC");

// FrameSource of h x w frames in one of the four fixed formats (JH_FRAME_*), whose layout follows from (h, w)
FrameSource jh::fixed_source(int format) {           // (fp32 RGB / uint8 BGR: any size, nothing to validate)
  FrameSource fs;
  fs.fmt = format;
  return fs;
}
int jh::frame_source(int format, int h, int w, FrameSource* out) {
  JH_REQUIRE(format >= JH_FRAME_RGB_F32 && format <= JH_FRAME_NV12, "frame format");
  if (format == JH_FRAME_I420 || format == JH_FRAME_NV12)
    JH_REQUIRE(h % 2 == 0 && w % 2 == 0, "YUV 4:2:0 frames need an even height and width");
  *out = fixed_source(format);
  return 0;
}

// Bytes from image n to image n + 1 of contiguous frames of h x w images: what the pixel functions of preprocess.h
// multiply n by -- the fixed formats' image size, a description's image_stride.
long long jh::image_bytes(const FrameSource& fs, int h, int w) {
  const long long px = (long long)h * w;
  return std::visit([&](const auto& d) -> long long {
    if constexpr (std::is_same_v<std::decay_t<decltype(d)>, std::monostate>)
      return fs.fmt == kSrcRgbF32 ? px * 12 : fs.fmt == kSrcBgrU8 ? px * 3 : px + px / 2;
    else
      return d.image_stride;
  }, fs.desc);
}

static_assert(JH_FRAME_SURFACE == kSrcYuvSurface && JH_FRAME_SENSOR == kSrcSensor,
              "frame format codes of the C ABI are preprocess.h's SRC");

// FrameSource of an entry point that takes any format (`who`: its name in the messages): `format` with exactly the
// description it needs, each checked by its one validation above.  per_image (jh_predictor_forward_images and its
// like): image_stride of a description is then only the extent every plane ends within; every image is image 0 of its
// own pointer, so a semi-planar surface takes the 2-byte chroma load whatever the parity of that extent (the kernel
// looks at the image's own base).
// pixels: the third description (the *_pixels entry points, whose frames have no JH_FRAME_* code): it comes alone.
int jh::call_source(const char* who, int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                    const jh_pixel_surface* pixels, int h, int w, bool per_image, FrameSource* out) {
  const std::string name(who);
  if (pixels) {
    JH_REQUIRE(!yuv && !sensor, name + ": a jh_pixel_surface comes with no other description");
    if (frame_source(pixels, h, w, out)) return 1;
    out->per_image = per_image;
    return 0;
  }
  JH_REQUIRE(format >= JH_FRAME_RGB_F32 && format <= JH_FRAME_SENSOR, name + ": unknown frame format");
  JH_REQUIRE((yuv != nullptr) == (format == JH_FRAME_SURFACE),
             name + ": JH_FRAME_SURFACE, and no other format, comes with a jh_yuv_surface");
  JH_REQUIRE((sensor != nullptr) == (format == JH_FRAME_SENSOR),
             name + ": JH_FRAME_SENSOR, and no other format, comes with a jh_sensor_surface");
  if (format == JH_FRAME_SURFACE ? frame_source(yuv, h, w, out)
      : format == JH_FRAME_SENSOR ? frame_source(sensor, h, w, out)
                                  : frame_source(format, h, w, out)) return 1;
  if (per_image)
    if (auto* d = std::get_if<SrcDesc<kSrcYuvSurface>>(&out->desc)) d->pair = d->c_step == 2;
  out->per_image = per_image;
  return 0;
}

namespace {
// per-image frames: up to kPtrChunk pointers of this call's table travel as kernel arguments into the predictor's
// device table -- no staging buffer, nothing the host has to keep alive or wait for
constexpr int kPtrChunk = 256;
struct PtrChunk { const void* p[kPtrChunk]; };
__global__ __launch_bounds__(kPtrChunk) void set_table_kernel(const void** table, int count, PtrChunk c) {
  const int i = threadIdx.x;
  if (i < count) table[i] = c.p[i];
}
}  // namespace

// The host table of a per-image call checked and sent into the predictor's device table (allocated by the first such
// call of a predictor) on the caller's stream.
int jh::upload_images(Scratch& mem, const void*** table, const void* const* images_host, int n_images, int want,
                      const FrameSource& fs, hipStream_t s) {
  JH_REQUIRE(images_host, "forward_images: null image table");
  JH_REQUIRE(n_images == want, "forward_images: n_images must be time_batch * num_cameras (2D predictor: time_batch)");
  // 16-bit samples (a wide sensor surface of 16-bit words, every wide YUV surface) are loaded as aligned 2-byte words
  const auto* sw = std::get_if<SrcDesc<kSrcSensorWide>>(&fs.desc);
  const bool words = fs.fmt == kSrcYuvWide || (sw && sw->kind == kSampleU16);
  for (int i = 0; i < n_images; ++i) {
    JH_REQUIRE(images_host[i], "forward_images: a null image pointer");
    JH_REQUIRE(fs.fmt != kSrcRgbF32 || reinterpret_cast<uintptr_t>(images_host[i]) % 4 == 0,
               "forward_images: an fp32 image that is not 4-byte aligned");
    JH_REQUIRE(!words || reinterpret_cast<uintptr_t>(images_host[i]) % 2 == 0,
               "forward_images: image " + std::to_string(i) + " of 16-bit samples is not 2-byte aligned");
  }
  if (!*table && first_call_alloc(mem, s, (size_t)want * sizeof(void*), "the first forward_images call of a predictor "
                                  "allocates its pointer table: make it outside a stream capture", table)) return 1;
  for (int off = 0; off < n_images; off += kPtrChunk) {
    PtrChunk c{};
    const int count = n_images - off < kPtrChunk ? n_images - off : kPtrChunk;
    for (int i = 0; i < count; ++i) c.p[i] = images_host[off + i];
    hipLaunchKernelGGL(set_table_kernel, dim3(1), dim3(kPtrChunk), 0, s, *table + off, count, c);
  }
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int jh_yuv_surface_check(const jh_yuv_surface* surface, int h, int w) { return yuv_surface_check(surface, h, w); }

int jh_sensor_surface_check(const jh_sensor_surface* surface, int h, int w) {
  return sensor_surface_check(surface, h, w);
}

int jh_pixel_surface_check(const jh_pixel_surface* surface, int h, int w) {
  return pixel_surface_check(surface, h, w);
}

int jh_op_pixels_to_bgr(const uint8_t* frames_dev, const jh_pixel_surface* surface, int n, int h, int w,
                        uint8_t* out_bgr_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(frames_dev && out_bgr_dev && n >= 1, "null frame / output pointer");
  FrameSource fs;
  if (frame_source(surface, h, w, &fs) || launch_frames_to_bgr(frames_dev, fs, out_bgr_dev, n, h, w, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_frames_to_rgb_f32(const void* frames_dev, int format, const jh_yuv_surface* yuv,
                            const jh_sensor_surface* sensor, const jh_pixel_surface* pixels, int n, int h, int w,
                            const float* tables_dev, int cams, float* out_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(frames_dev && out_dev && n >= 1 && h >= 1 && w >= 1, "jh_op_frames_to_rgb_f32: null frame / output "
             "pointer or empty size");
  JH_REQUIRE(!tables_dev || cams >= 1, "jh_op_frames_to_rgb_f32: tables come with their camera count");
  FrameSource fs;
  if (call_source("jh_op_frames_to_rgb_f32", format, yuv, sensor, pixels, h, w, false, &fs)) return 1;
  JH_REQUIRE(fs.fmt != kSrcRgbF32, "jh_op_frames_to_rgb_f32: tone tables apply to byte frames");
  if (tables_dev) { fs.tone = tables_dev; fs.tone_cam0 = 0; fs.tone_cams = cams; }
  if (launch_frames_to_rgb_f32(frames_dev, fs, out_dev, n, h, w, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_yuv420_to_bgr(const uint8_t* frames_dev, int format, int n, int h, int w, uint8_t* out_bgr_dev,
                        void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(frames_dev && out_bgr_dev, "null frame / output pointer");
  JH_REQUIRE(format == JH_FRAME_I420 || format == JH_FRAME_NV12, "jh_op_yuv420_to_bgr: format must be "
             "JH_FRAME_I420 or JH_FRAME_NV12");
  FrameSource fs;
  if (frame_source(format, h, w, &fs) || launch_frames_to_bgr(frames_dev, fs, out_bgr_dev, n, h, w, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_yuv_surface_to_bgr(const uint8_t* frames_dev, const jh_yuv_surface* surface, int n, int h, int w,
                             uint8_t* out_bgr_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(frames_dev && out_bgr_dev && n >= 1, "null frame / output pointer");
  FrameSource fs;
  if (frame_source(surface, h, w, &fs) || launch_frames_to_bgr(frames_dev, fs, out_bgr_dev, n, h, w, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_sensor_to_bgr(const uint8_t* frames_dev, const jh_sensor_surface* surface, int n, int h, int w,
                        uint8_t* out_bgr_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(frames_dev && out_bgr_dev && n >= 1, "null frame / output pointer");
  FrameSource fs;
  if (frame_source(surface, h, w, &fs) || launch_frames_to_bgr(frames_dev, fs, out_bgr_dev, n, h, w, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
