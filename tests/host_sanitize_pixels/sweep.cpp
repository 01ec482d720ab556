// Stand-alone sweep of the pixel-surface host code under ASan + UBSan (tests/host_sanitize_pixels/Makefile):
// jh_pixel_surface_check, the FrameSource construction (frame_source, call_source) and the host path of
// jh_op_pixels_to_bgr over random and extreme descriptions.  The sanitizers abort on a finding; the program itself
// checks what the validation promises -- an accepted description addresses no byte outside [0, image_stride) at the
// four corners of every component, computed here in 128 bits -- and that a refusal leaves a message.
// Prints "sweep OK: <accepted> accepted, <refused> refused" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "predictor.h"
#include "preprocess.h"

// the library's last-error sink lives in api.hip, which is not part of this build: the program's own
namespace { std::string g_err; }
namespace jh { void set_error(const std::string& msg) { g_err = msg; } }

using namespace jh;

static int fail(const char* what, const jh_pixel_surface& q, int h, int w) {
  std::fprintf(stderr, "sweep: %s (h %d, w %d, stride %lld, colour %d, last error '%s')\n", what, h, w,
               (long long)q.image_stride, q.colour, g_err.c_str());
  return 1;
}

// what an accepted description must satisfy, and what the FrameSource built from it must hold
static int accepted(const jh_pixel_surface& q, int h, int w) {
  for (int k = 0; k < 3; ++k)
    for (int cy = 0; cy < 2; ++cy)
      for (int cx = 0; cx < 2; ++cx) {
        const __int128 a = (__int128)q.offset[k] + (__int128)((cy ? h - 1 : 0) >> q.ys[k]) * q.pitch[k] +
                           (__int128)((cx ? w - 1 : 0) >> q.xs[k]) * q.step[k];
        if (a < 0 || a >= q.image_stride) return fail("an accepted description addresses a byte outside the image", q, h, w);
      }
  for (int per_image = 0; per_image < 2; ++per_image) {
    FrameSource fs, again;
    if (call_source("sweep", kSrcPixels, nullptr, nullptr, &q, h, w, per_image != 0, &fs) ||
        call_source("sweep", kSrcPixels, nullptr, nullptr, &q, h, w, per_image != 0, &again))
      return fail("call_source refuses what the check accepts", q, h, w);
    const auto* d = std::get_if<SrcDesc<kSrcPixels>>(&fs.desc);
    if (!d || fs.fmt != kSrcPixels || fs.per_image != (per_image != 0)) return fail("FrameSource of another form", q, h, w);
    if (!(fs == again) || fs != again) return fail("two sources of one description differ", q, h, w);
    if (!(fs.px_bytes() > 0.0 && fs.px_bytes() <= 3.0)) return fail("px_bytes outside (0, 3]", q, h, w);
    if (d->image_stride != q.image_stride || d->yuv != (q.colour == JH_PIXEL_YUV)) return fail("fields not carried", q, h, w);
    if (d->yuv && (d->cy <= 0 || d->cvr <= 0 || d->cub <= 0 || d->cug >= 0 || d->cvg >= 0))
      return fail("YUV constants not filled", q, h, w);
    int rows = 0;
    if (dispatch_src(fs, [&](auto tag, const auto&) { rows += decltype(tag)::value == kSrcPixels; return 0; }) || rows != 1)
      return fail("dispatch_src does not reach the form's row", q, h, w);
  }
  FrameSource other;
  jh_yuv_surface y{};
  if (!call_source("sweep", kSrcPixels, &y, nullptr, &q, h, w, false, &other))
    return fail("a pixel surface together with another description is accepted", q, h, w);
  return 0;
}

int main() {
  std::mt19937_64 g(13);
  const int64_t ext[] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, 2, 3, 4, 7, 8, 255, 256, 65535, (int64_t)1 << 31,
                         ((int64_t)1 << 31) - 1, ((int64_t)1 << 32) + 1, INT64_MAX / 3, INT64_MAX - 1, INT64_MAX};
  const int32_t ext32[] = {INT32_MIN, -1, 0, 1, 2, 3, 4, 8, 9, 255, 0x100, 0x102, 0x200, INT32_MAX};
  const int sizes[] = {INT32_MIN, -1, 0, 1, 2, 3, 5, 6, 10, 259, 1024, 65536, INT32_MAX};
  const int NE = sizeof(ext) / sizeof(ext[0]), NE32 = sizeof(ext32) / sizeof(ext32[0]), NS = sizeof(sizes) / sizeof(sizes[0]);
  long n_ok = 0, n_bad = 0;
  bool tame = false;              // every other description is drawn without the extremes, so that about a third passes
  const auto pick64 = [&](int small_bound) -> int64_t {
    const unsigned r = tame ? 2u : (unsigned)(g() % 8);
    return r == 0 ? ext[g() % NE] : r == 1 ? (int64_t)g() : (int64_t)(g() % (uint64_t)small_bound);
  };
  const auto pick32 = [&](int lo, int hi) -> int32_t {
    const unsigned r = tame ? 2u : (unsigned)(g() % 16);
    return r == 0 ? ext32[g() % NE32] : r == 1 ? (int32_t)g() : lo + (int32_t)(g() % (uint64_t)(hi - lo + 1));
  };
  for (long it = 0; it < 400000; ++it) {
    jh_pixel_surface q{};
    tame = it % 2 == 0;
    const int h = !tame && g() % 8 == 0 ? sizes[g() % NS] : 1 + (int)(g() % 40);
    const int w = !tame && g() % 8 == 0 ? sizes[g() % NS] : 1 + (int)(g() % 40);
    q.colour = pick32(0, 1);
    const int sub_x = (int)(g() % 3), sub_y = (int)(g() % 3);
    for (int k = 0; k < 3; ++k) {
      q.step[k] = pick32(1, 8);
      q.xs[k] = q.colour == JH_PIXEL_YUV && k > 0 && g() % 8 ? sub_x : pick32(0, g() % 4 ? 0 : 2);
      q.ys[k] = q.colour == JH_PIXEL_YUV && k > 0 && g() % 8 ? sub_y : pick32(0, g() % 4 ? 0 : 2);
      q.offset[k] = pick64(64);
      // mostly a pitch near the smallest one that fits, so that many descriptions pass
      const int64_t need = h > 0 && w > 0 && q.xs[k] >= 0 && q.xs[k] < 31 ? (int64_t)((w - 1) >> q.xs[k]) * q.step[k] + 1 : 1;
      q.pitch[k] = tame || g() % 4 ? need + (int64_t)(g() % 8) - (g() % 16 == 0) : pick64(4096);
    }
    q.matrix = q.colour == JH_PIXEL_YUV ? pick32(0, 1) : pick32(0, 0);
    q.range = q.colour == JH_PIXEL_YUV ? pick32(0, 1) : pick32(0, 0);
    q.sample = tame || g() % 16 ? 0 : ext32[g() % NE32];
    q.image_stride = g() % 4 ? (int64_t)(g() % 16384) : pick64(1 << 20);
    if ((tame ? g() % 3 != 0 : g() % 3 == 0) && h > 0 && w > 0 && h < 4096 && w < 4096) {      // ... or exactly the extent, or one byte less
      __int128 end = 0;
      for (int k = 0; k < 3; ++k) {
        if (q.xs[k] < 0 || q.xs[k] > 2 || q.ys[k] < 0 || q.ys[k] > 2) continue;
        const __int128 e = (__int128)q.offset[k] + (__int128)((h - 1) >> q.ys[k]) * q.pitch[k] +
                           (__int128)((w - 1) >> q.xs[k]) * q.step[k] + 1;
        if (e > end) end = e;
      }
      if (end > 0 && end < INT64_MAX) q.image_stride = (int64_t)end - (g() % 4 == 0);
    }
    g_err.clear();
    if (jh_pixel_surface_check(&q, h, w) == 0) {
      ++n_ok;
      if (accepted(q, h, w)) return 1;
      if (n_ok % 64 == 0 && q.image_stride <= (1 << 20)) {             // the operator's host path, on the stand-in
        void* in = std::malloc((size_t)q.image_stride * 2);
        void* out = std::malloc((size_t)2 * h * w * 3);
        const int rc = jh_op_pixels_to_bgr(static_cast<const uint8_t*>(in), &q, 2, h, w, static_cast<uint8_t*>(out), nullptr);
        std::free(in);
        std::free(out);
        if (rc) return fail("jh_op_pixels_to_bgr refuses what the check accepts", q, h, w);
      }
    } else {
      ++n_bad;
      if (g_err.empty()) return fail("a refusal without a message", q, h, w);
      FrameSource fs;
      if (!frame_source(&q, h, w, &fs)) return fail("frame_source accepts what the check refuses", q, h, w);
    }
  }
  jh_pixel_surface q{};
  if (jh_pixel_surface_check(nullptr, 4, 4) == 0 || jh_op_pixels_to_bgr(nullptr, &q, 1, 4, 4, nullptr, nullptr) == 0)
    return fail("null arguments accepted", q, 4, 4);
  if (n_ok < 20000 || n_bad < 20000) {
    std::fprintf(stderr, "sweep: the generator is lopsided: %ld accepted, %ld refused\n", n_ok, n_bad);
    return 1;
  }
  std::printf("sweep OK: %ld accepted, %ld refused\n", n_ok, n_bad);
  return 0;
}
