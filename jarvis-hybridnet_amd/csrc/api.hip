// C ABI of libjarvis_hip.so (declarations + reference citations: include/jarvis_hip.h)
#include <cstring>
#include <memory>
#include "../../include/jarvis_hip.h"
#include <cstdlib>
#include "nets.h"
#include "bifpn_node.h"
#include "views2d.h"
#include "subjects.h"
#include "joints3d.h"
#include "tracks.h"

namespace jh {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace jh

using namespace jh;

struct jh_params { ParamMap map; };
struct jh_efftrack { EffTrackPlan plan; };
struct jh_v2v { V2VPlan plan; };

namespace {

// RAII device scratch for the non-pipelined (test / API-parity) entry points.
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
  int get(void** p, size_t bytes) {
    JH_CHECK_HIP(hipMalloc(p, bytes));
    ptrs.push_back(*p);
    return 0;
  }
  int act(int N, int D, int H, int W, int C, Act* a) {
    a->N = N; a->D = D; a->H = H; a->W = W; a->C = C; a->Cp = cpad(C);
    return get(reinterpret_cast<void**>(&a->p), a->bytes());
  }
};

// Host values -> a device buffer of the scratch (synchronous: the host side may be a local).
template <typename T>
int op_upload(Scratch& sc, const T* host, size_t count, T** dev) {
  if (sc.get(reinterpret_cast<void**>(dev), count * sizeof(T))) return 1;
  JH_CHECK_HIP(hipMemcpy(*dev, host, count * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// Caller-provided workspace, carved into 256-byte aligned pieces.  With base == nullptr it
// only measures (jh_*_workspace_bytes).
struct Carver {
  char* base;
  size_t cap, off = 0;
  Carver(void* b, size_t c) : base(static_cast<char*>(b)), cap(c) {}
  template <typename T> T* take(size_t count) {
    const size_t at = off;
    off += (count * sizeof(T) + 255) / 256 * 256;
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
  void act(int N, int D, int H, int W, int C, Act* a) {
    a->N = N; a->D = D; a->H = H; a->W = W; a->C = C; a->Cp = cpad(C);
    a->p = take<float>(a->elems());
  }
  bool fits() const { return off <= cap; }
};

struct ReproWs { Act heat, vol; float2* coarse; };
static size_t carve_reproject(Carver& c, int cams, int joints, int hs, int g, ReproWs* w) {
  const int gh = g / 2;
  c.act(cams, 1, hs, hs, joints, &w->heat);
  c.act(1, g, g, g, joints, &w->vol);
  w->coarse = c.take<float2>((size_t)cams * gh * gh * gh);
  return c.off;
}
struct SoftWs { Act x; double* partial; int* pmax; };
static size_t carve_softargmax(Carver& c, int t, int joints, int gh, SoftWs* w) {
  c.act(t, gh, gh, gh, joints, &w->x);
  w->partial = c.take<double>((size_t)t * w->x.Cp * 4 * kLimbs);
  w->pmax = c.take<int>((size_t)t * w->x.Cp);
  return c.off;
}
// the spread form's sums and keys: one piece (launch_softargmax zeroes it with one launch)
static size_t carve_spread(Carver& c, int t, int Jp, SoftargmaxSpread* sp) {
  const size_t n = softargmax_spread_sums(t, Jp);
  sp->sums = c.take<double>(n + (size_t)t * Jp);
  sp->key = sp->sums ? reinterpret_cast<unsigned long long*>(sp->sums + n) : nullptr;
  return c.off;
}
struct ReconWs { float* det; int *c3i, *chm, *valid; };
static size_t carve_reconstruct(Carver& c, int cams, ReconWs* w) {
  w->det = c.take<float>((size_t)cams * 3);
  w->c3i = c.take<int>(3);
  w->chm = c.take<int>((size_t)cams * 2);
  w->valid = c.take<int>(1);
  return c.off;
}

// (T,C) channel-last heatmaps [N][Hh][Hh][Jp] -> padded NCHW (N,J,hs,hs)
__global__ void export_padded_kernel(const float* __restrict__ heat, float* __restrict__ out, int N,
                                     int J, int Jp, int Hh) {
  const int hs = Hh + 2;
  const size_t total = (size_t)N * J * hs * hs;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % hs), y = (int)((i / hs) % hs);
    const int j = (int)((i / ((size_t)hs * hs)) % J);
    const size_t n = i / ((size_t)hs * hs * J);
    float v = 0.f;
    if (x >= 1 && y >= 1 && x <= Hh && y <= Hh)
      v = heat[((n * Hh + (y - 1)) * Hh + (x - 1)) * Jp + j];
    out[i] = v;
  }
}

// all-gathered detections (blocks, T, C/blocks, 3) -> (T, C, 3), camera = block * C/blocks + local
__global__ void det_unblock_kernel(const float* __restrict__ src, float* __restrict__ dst, int T, int C,
                                   int cpb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * C * 3) return;
  const int k = i % 3, c = (i / 3) % C, t = i / (3 * C);
  dst[i] = src[(((size_t)(c / cpb) * T + t) * cpb + c % cpb) * 3 + k];
}

// graph replays: this call's frame pointer into the device cell the captured kernels read it from
__global__ void set_cell_kernel(const void** cell, const void* value) { *cell = value; }
// per-image frames: up to kPtrChunk pointers of this call's table travel as kernel arguments into the predictor's
// device table -- no staging buffer, nothing the host has to keep alive or wait for
constexpr int kPtrChunk = 256;
struct PtrChunk { const void* p[kPtrChunk]; };
__global__ __launch_bounds__(kPtrChunk) void set_table_kernel(const void** table, int count, PtrChunk c) {
  const int i = threadIdx.x;
  if (i < count) table[i] = c.p[i];
}
// ... and the results out of the predictor's own buffers into this call's output tensors
__global__ void copy_out_kernel(const float* __restrict__ gp, const float* __restrict__ gc,
                                const int* __restrict__ gv, float* __restrict__ points,
                                float* __restrict__ conf, int* __restrict__ valid, int n_pts, int n_conf,
                                int n_valid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pts) points[i] = gp[i];
  if (i < n_conf) conf[i] = gc[i];
  if (valid && i < n_valid) valid[i] = gv[i];
}

__global__ void pack_det_kernel(const float* __restrict__ pts2d, const float* __restrict__ maxvals,
                                float* __restrict__ det, int C) {
  const int c = threadIdx.x;
  if (c < C) {
    det[c * 3 + 0] = pts2d[c];
    det[c * 3 + 1] = pts2d[C + c];
    det[c * 3 + 2] = maxvals[c];
  }
}

}  // namespace

extern "C" {

const char* jh_last_error(void) { return g_err.c_str(); }
int jh_abi_version(void) { return JH_ABI_VERSION; }

int jh_set_precision(int mode) {
  JH_REQUIRE(mode == JH_PRECISION_F32 || mode == JH_PRECISION_BF16X3 || mode == JH_PRECISION_BF16X3_WIDE,
             "unknown precision mode");
  set_precision_mode(mode);
  return 0;
}
int jh_get_precision(void) { return precision_mode(); }

int jh_params_create(jh_params** out) {
  *out = new jh_params();
  return 0;
}
int jh_params_set(jh_params* p, const char* key, const float* host, int64_t numel) {
  JH_REQUIRE(p && key && host && numel >= 0, "bad argument");
  p->map[key] = std::vector<float>(host, host + numel);
  return 0;
}
void jh_params_destroy(jh_params* p) { delete p; }

// ---------------------------------------------------------------- EfficientTrack
int jh_efftrack_create(const jh_params* p, const char* prefix, int model_size, int joints, int n,
                       int h, int w, int want_res1, jh_efftrack** out) {
  JH_REQUIRE(p && out, "bad argument");
  std::unique_ptr<jh_efftrack> net(new jh_efftrack());
  if (net->plan.build(p->map, prefix ? prefix : "", model_size, joints, n, h, w, want_res1 != 0)) return 1;
  *out = net.release();
  return 0;
}
int jh_efftrack_forward(jh_efftrack* net, const float* x_dev, float* res1_dev, float* res2_dev,
                        void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(net && x_dev && res2_dev, "bad argument");
  JH_REQUIRE(!res1_dev || net->plan.res1.p, "res1 requested from a network created with want_res1 = 0");
  if (launch_to_channel_last(x_dev, net->plan.input, s)) return 1;
  if (net->plan.run(s)) return 1;
  if (res1_dev && launch_from_channel_last(net->plan.res1, res1_dev, s)) return 1;
  return launch_from_channel_last(net->plan.heat, res2_dev, s);
}
int64_t jh_efftrack_launches(const jh_efftrack* net) { return (int64_t)net->plan.launches(); }
void jh_efftrack_destroy(jh_efftrack* net) { delete net; }

// --------------------------------------------------------------------------- V2V
int jh_v2v_create(const jh_params* p, const char* prefix, int joints, int t, int g, jh_v2v** out) {
  JH_REQUIRE(p && out, "bad argument");
  std::unique_ptr<jh_v2v> net(new jh_v2v());
  if (net->plan.build(p->map, prefix ? prefix : "", joints, t, g)) return 1;
  *out = net.release();
  return 0;
}
int jh_v2v_forward(jh_v2v* net, const float* x_dev, float* y_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (launch_to_channel_last(x_dev, net->plan.input, s)) return 1;
  if (net->plan.run(s)) return 1;
  return launch_from_channel_last(net->plan.output, y_dev, s);
}
void jh_v2v_destroy(jh_v2v* net) { delete net; }
int jh_v2v_fold(int joints, int t, int g, int* folded) {
  JH_REQUIRE(joints >= 1 && t >= 1 && g >= 4 && g % 4 == 0 && folded, "jh_v2v_fold: bad argument");
  *folded = v2v_fold_applies(joints, g) ? 1 : 0;      // (never a function of t)
  return 0;
}

// ------------------------------------------------------------------ reprojection
int64_t jh_reproject_workspace_bytes(int cams, int joints, int hs, int grid_size) {
  Carver c(nullptr, 0);
  ReproWs w;
  return (int64_t)carve_reproject(c, cams, joints, hs, grid_size, &w);
}

int jh_reproject_forward(const float* heatmaps_padded_dev, int cams, int joints, int hs,
                         const int32_t* center3d_dev, const int32_t* center_hm_dev,
                         const float* cam_dev, const float* intr_dev, const float* dist_dev,
                         int grid_size, float grid_spacing, float* vol_dev, int32_t* idx_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_reproject_workspace_bytes)");
  JH_REQUIRE(grid_size > 0 && grid_size % 2 == 0, "grid size must be even");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  ReproWs w;
  carve_reproject(c, cams, joints, hs, grid_size, &w);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_reproject_workspace_bytes()");
  if (launch_to_channel_last(heatmaps_padded_dev, w.heat, s)) return 1;
  if (launch_reproject(Calib{cam_dev, intr_dev, dist_dev, /*fs=*/0}, center3d_dev, center_hm_dev, w.heat.p, w.coarse,
                       w.vol.p, idx_dev, 1, cams, grid_size, grid_spacing, hs, w.heat.Cp,
                       /*heat_pad=*/1, /*div255=*/0, /*mask=*/nullptr, s)) return 1;
  return launch_from_channel_last(w.vol, vol_dev, s);
}

// (the plain operator's pieces first, then the gather's channel sets and counts)
static size_t carve_reproject_joint(Carver& c, int cams, int joints, int hs, int g, ReproWs* w, JointSets* js) {
  carve_reproject(c, cams, joints, hs, g, w);
  js->sets = c.take<unsigned long long>((size_t)cams);
  js->ncam = c.take<int>((size_t)cpad(joints));
  return c.off;
}

int64_t jh_reproject_joint_masked_workspace_bytes(int cams, int joints, int hs, int grid_size) {
  Carver c(nullptr, 0);
  ReproWs w;
  JointSets js;
  return (int64_t)carve_reproject_joint(c, cams, joints, hs, grid_size, &w, &js);
}

int jh_reproject_forward_joint_masked(const float* heatmaps_padded_dev, int cams, int joints, int hs,
                                      const int32_t* center3d_dev, const int32_t* center_hm_dev,
                                      const float* cam_dev, const float* intr_dev, const float* dist_dev,
                                      int grid_size, float grid_spacing, const uint8_t* mask_dev,
                                      const uint8_t* joint_mask_dev, float* vol_dev, void* workspace_dev,
                                      int64_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_reproject_joint_masked_workspace_bytes)");
  JH_REQUIRE(grid_size > 0 && grid_size % 2 == 0, "grid size must be even");
  JH_REQUIRE(joint_mask_dev, "jh_reproject_forward_joint_masked: null joint mask");
  JH_REQUIRE(cams >= 1 && cams <= 64 && joints >= 1 && joints <= 64, "jh_reproject_forward_joint_masked: 1 .. 64 "
             "cameras and joints");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  ReproWs w;
  JointSets js;
  carve_reproject_joint(c, cams, joints, hs, grid_size, &w, &js);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_reproject_joint_masked_workspace_bytes()");
  if (launch_to_channel_last(heatmaps_padded_dev, w.heat, s)) return 1;
  if (launch_reproject_joint_masked(Calib{cam_dev, intr_dev, dist_dev, /*fs=*/0}, center3d_dev, center_hm_dev, w.heat.p,
                                    w.coarse, w.vol.p, nullptr, 1, cams, grid_size, grid_spacing, hs, joints, w.heat.Cp,
                                    /*heat_pad=*/1, /*div255=*/0, mask_dev, joint_mask_dev, js, s)) return 1;
  return launch_from_channel_last(w.vol, vol_dev, s);
}

int64_t jh_softargmax_workspace_bytes(int t, int joints, int gh) {
  Carver c(nullptr, 0);
  SoftWs w;
  return (int64_t)carve_softargmax(c, t, joints, gh, &w);
}

int jh_softargmax(const float* v2v_out_dev, int t, int joints, int gh, float grid_spacing,
                  float roi_cube_size, const int32_t* center3d_dev, float* heatmap_final_dev,
                  float* points_dev, float* conf_dev, void* workspace_dev, int64_t workspace_bytes,
                  void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_softargmax_workspace_bytes)");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  SoftWs w;
  carve_softargmax(c, t, joints, gh, &w);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_softargmax_workspace_bytes()");
  if (launch_to_channel_last(v2v_out_dev, w.x, s)) return 1;
  return launch_softargmax(w.x.p, center3d_dev, w.partial, w.pmax, points_dev, conf_dev,
                           heatmap_final_dev, t, joints, w.x.Cp, gh, grid_spacing, roi_cube_size, s);
}

int64_t jh_softargmax_spread_workspace_bytes(int t, int joints, int gh) {
  Carver c(nullptr, 0);
  SoftWs w;
  SoftargmaxSpread sp;
  carve_softargmax(c, t, joints, gh, &w);
  return (int64_t)carve_spread(c, t, w.x.Cp, &sp);
}

int jh_softargmax_spread(const float* v2v_out_dev, int t, int joints, int gh, float grid_spacing,
                         float roi_cube_size, const int32_t* center3d_dev, float* heatmap_final_dev,
                         float* points_dev, float* conf_dev, float* cov_dev, float* peak_dev, float* mass_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_softargmax_spread_workspace_bytes)");
  JH_REQUIRE(cov_dev && peak_dev && mass_dev, "jh_softargmax_spread: null output pointer");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  SoftWs w;
  SoftargmaxSpread sp;
  carve_softargmax(c, t, joints, gh, &w);
  carve_spread(c, t, w.x.Cp, &sp);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_softargmax_spread_workspace_bytes()");
  sp.cov = cov_dev; sp.peak = peak_dev; sp.mass = mass_dev;
  if (launch_to_channel_last(v2v_out_dev, w.x, s)) return 1;
  return launch_softargmax(w.x.p, center3d_dev, w.partial, w.pmax, points_dev, conf_dev,
                           heatmap_final_dev, t, joints, w.x.Cp, gh, grid_spacing, roi_cube_size, s, &sp);
}

int jh_reproject_point(const float* points_dev, int npoints, int cams, const float* cam_dev,
                       const float* intr_dev, const float* dist_dev, float* uv_dev, void* stream) {
  return launch_project_points(points_dev, cam_dev, intr_dev, dist_dev, uv_dev, npoints, cams,
                               static_cast<hipStream_t>(stream));
}

int64_t jh_reconstruct_workspace_bytes(int cams) {
  Carver c(nullptr, 0);
  ReconWs w;
  return (int64_t)carve_reconstruct(c, cams, &w);
}

int jh_reconstruct_point(const float* points2d_dev, const float* maxvals_dev, int cams,
                         const float* cam_dev, const float* intr_dev, const float* dist_dev,
                         float* point3d_dev, void* workspace_dev, int64_t workspace_bytes,
                         void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(cams >= 1 && cams <= 64, "at most 64 cameras");
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_reconstruct_workspace_bytes)");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  ReconWs w;
  carve_reconstruct(c, cams, &w);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_reconstruct_workspace_bytes()");
  hipLaunchKernelGGL(pack_det_kernel, dim3(1), dim3(64), 0, s, points2d_dev, maxvals_dev, w.det, cams);
  JH_CHECK_HIP(hipGetLastError());
  return launch_triangulate(w.det, Calib{cam_dev, intr_dev, dist_dev, /*fs=*/0}, point3d_dev, w.c3i, w.chm, w.valid, 1,
                            cams, 1.f, 1.f, 1.f, 0, 1 << 20, 1 << 20, /*mask=*/nullptr, nullptr, nullptr, s);
}

}  // extern "C"

// ------------------------------------------------------------------- predictor
// time one glue launch when the profiler is on
#define JH_PROF(name, flops, bytes, call)                      \
  do {                                                         \
    Profiler& _pf = profiler();                                \
    if (_pf.on) _pf.begin(name, flops, bytes, s);              \
    if (call) return 1;                                        \
    if (_pf.on) _pf.end(s);                                    \
  } while (0)

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

// FrameSource of a described YUV 4:2:0 surface of h x w images: the check above, then the description as the kernels
// take it (preprocess.h) -- the layout and the constants of its (matrix, range)
static int frame_source(const jh_yuv_surface* sp, int h, int w, FrameSource* out) {
  if (yuv_surface_check(sp, h, w)) return 1;
  const jh_yuv_surface& q = *sp;
  // {Y0, CY, CVR, CUB, CUG, CVG}: BT.601 limited = OpenCV's literals (yuv_to_rgb8); the others round(x * 2^20) of
  // the float64 matrix (include/jarvis_hip.h)
  static const int k[2][2][6] = {{{16, 1220542, 1673527, 2116026, -409993, -852492},
                                  {0, 1048576, 1470104, 1858077, -360853, -748826}},
                                 {{16, 1220945, 1879825, 2215014, -223607, -558796},
                                  {0, 1048576, 1651297, 1945738, -196424, -490864}}};
  const int* c = k[q.matrix][q.range];
  const auto fill = [&](YuvSurface& a) {
    a.image_stride = q.image_stride; a.y_offset = q.y_offset; a.y_pitch = q.y_pitch;
    a.u_offset = q.u_offset; a.v_offset = q.v_offset; a.c_pitch = q.c_pitch; a.c_step = q.c_step;
    a.y0 = c[0]; a.cy = c[1]; a.cvr = c[2]; a.cub = c[3]; a.cug = c[4]; a.cvg = c[5];
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
static int frame_source(const jh_sensor_surface* sp, int h, int w, FrameSource* out) {
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

static_assert(JH_FRAME_RGB_F32 == kSrcRgbF32 && JH_FRAME_BGR_U8 == kSrcBgrU8 && JH_FRAME_I420 == kSrcI420 &&
                  JH_FRAME_NV12 == kSrcNV12, "frame format codes of the C ABI are preprocess.h's SRC");

// FrameSource of h x w frames in one of the four fixed formats (JH_FRAME_*), whose layout follows from (h, w)
static FrameSource fixed_source(int format) {        // (fp32 RGB / uint8 BGR: any size, nothing to validate)
  FrameSource fs;
  fs.fmt = format;
  return fs;
}
static int frame_source(int format, int h, int w, FrameSource* out) {
  JH_REQUIRE(format >= JH_FRAME_RGB_F32 && format <= JH_FRAME_NV12, "frame format");
  if (format == JH_FRAME_I420 || format == JH_FRAME_NV12)
    JH_REQUIRE(h % 2 == 0 && w % 2 == 0, "YUV 4:2:0 frames need an even height and width");
  *out = fixed_source(format);
  return 0;
}

static_assert(JH_FRAME_SURFACE == kSrcYuvSurface && JH_FRAME_SENSOR == kSrcSensor,
              "frame format codes of the C ABI are preprocess.h's SRC");

// FrameSource of an entry point that takes any format (`who`: its name in the messages): `format` with exactly the
// description it needs, each checked by its one validation above.  per_image (jh_predictor_forward_images and its
// like): image_stride of a description is then only the extent every plane ends within; every image is image 0 of its
// own pointer, so a semi-planar surface takes the 2-byte chroma load whatever the parity of that extent (the kernel
// looks at the image's own base).
static int call_source(const char* who, int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor, int h,
                       int w, bool per_image, FrameSource* out) {
  const std::string name(who);
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

// A buffer that the first call of its kind allocates (never jh_predictor_create): `bytes` of the predictor's memory,
// not inside a stream capture -- `what` is the site's own message for that.
template <typename T>
static int first_call_alloc(Scratch& mem, hipStream_t s, size_t bytes, const char* what, T** out) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cs);
  JH_REQUIRE(cs == hipStreamCaptureStatusNone, what);
  return mem.get(reinterpret_cast<void**>(out), bytes);
}

// The host table of a per-image call checked and sent into the predictor's device table (allocated by the first such
// call of a predictor) on the caller's stream.
static int upload_images(Scratch& mem, const void*** table, const void* const* images_host, int n_images, int want,
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

// What the creation of both predictors shares: the precision resolved into cfg (the predictor's own setting;
// JH_PRECISION_DEFAULT follows the process-wide default), and EffTrackPlans set up, before build(), with it and with
// the forms of the predictor's time-batch class (EffTrackPlan::node_class, Plan::norm_block_kb).
struct PlanSetup {
  int precision = 0, norm_kb = 0;
  NodeBatchClass node_class = NodeBatchClass::ByLaunchSize;
  int init(jh_predictor_config* cfg, NodeBatchClass cls, int kb) {
    JH_REQUIRE(cfg->precision >= JH_PRECISION_DEFAULT && cfg->precision <= JH_PRECISION_BF16X3_WIDE,
               "jh_predictor_config.precision: unknown mode");
    if (cfg->precision == JH_PRECISION_DEFAULT) cfg->precision = precision_mode();
    precision = cfg->precision; node_class = cls; norm_kb = kb;
    return 0;
  }
  std::unique_ptr<EffTrackPlan> efftrack() const {
    std::unique_ptr<EffTrackPlan> p(new EffTrackPlan());
    p->precision = precision; p->node_class = node_class; p->norm_block_kb = norm_kb;
    return p;
  }
};

// preds * (downsampling_scale * 2), jarvis3D.py:138-141,158-160: CenterDetect's arg-max (or peaks) in full-frame pixels
struct Scale2 { float x, y; };
static Scale2 center_scale2(const jh_predictor_config& c) {
  return {(float)((double)c.img_w / (double)c.center_size) * 2.f,
          (float)((double)c.img_h / (double)c.center_size) * 2.f};
}

// What one call is, handed down to the stage functions: its frames and their source, the camera mask in force and the
// stream.  (A stage-3 call has no frames: it gives the mask and the stream.)
struct Call {
  const void* frames = nullptr;              // contiguous frames; per-image: the device table (never dereferenced here)
  FrameSource fs;
  const unsigned char* mask = nullptr;       // [T][C] device bytes, nullptr = no mask (the plain kernels)
  // [T][J][C] device bytes, nullptr = no joint mask: stage 3 runs the joint-masked gather (nets.h: JointSets)
  const unsigned char* joint_mask = nullptr;
  // what the launches read the frame pointer(s) through: the per-image table, the one-pointer cell of a forward that
  // is being captured, or nullptr = `frames` itself
  const void* const* cell = nullptr;
  hipStream_t s = nullptr;
};
static Call make_call(const void* frames, const FrameSource& fs, void* stream, const unsigned char* mask = nullptr) {
  Call c;
  c.frames = frames; c.fs = fs; c.mask = mask; c.s = static_cast<hipStream_t>(stream);
  if (fs.per_image) c.cell = static_cast<const void* const*>(frames);
  return c;
}
static Call stage3_call(void* stream, const unsigned char* mask = nullptr) {
  Call c;
  c.mask = mask; c.s = static_cast<hipStream_t>(stream);
  return c;
}

// The form of a whole-path forward, which names its graph slot: one slot per frame format (kSrc*, preprocess.h) and
// per combination of the four flags.  masked: the masked kernels.  per_image: slots of its OWN -- a stream of per-image
// calls and a stream of contiguous calls of one format never re-record each other.  centred: the forward from
// caller-supplied centres (centers_on), which records no stage 1 -- a tracking loop that falls back to one detected
// call between centred ones never re-records.  spread: the spread form of the tail (spread_on), which is another
// recording -- a loop that alternates spread-on and spread-off calls never re-records either.
constexpr int kGraphFmts = kSrcCount;
struct ForwardForm {
  int fmt = 0;
  bool masked = false, per_image = false, centred = false, spread = false;
  constexpr int index() const { return (((spread * 2 + centred) * 2 + per_image) * 2 + masked) * kGraphFmts + fmt; }
};
constexpr int kGraphSlots = kGraphFmts << 4;  // (four flags)
static_assert(ForwardForm{kGraphFmts - 1, true, true, true, true}.index() == kGraphSlots - 1,
              "the largest ForwardForm::index() is the last graph slot");

struct jh_predictor {
  jh_predictor_config cfg{};
  int T3 = 0;
  int T = 0, C = 0, Cloc = 0, J = 0, Jp = 0, B = 0, Hh = 0, G = 0, Gh = 0, hs = 0;
  std::unique_ptr<EffTrackPlan> center, kp;
  std::unique_ptr<V2VPlan> v2v;
  Scratch mem;
  float *cam = nullptr, *intr = nullptr, *dist = nullptr;
  // Per-frame calibration (jh_predictor_set_calibration_frames): T rows of the three arrays above, allocated by the
  // first such call.  calib_fs is the frame stride every launch that reads calibration is given: 0 -- all frames read
  // cam / intr / dist --, or C -- frame t reads row t of cam_f / intr_f / dist_f.  A call that starts at frame t0
  // (stage 3, views2d) passes the rows from t0 on, as it passes the centres' and the mask's.
  float *cam_f = nullptr, *intr_f = nullptr, *dist_f = nullptr;
  int calib_fs = 0;
  Calib calib_at(int t0) const {
    return calib_fs ? Calib{cam_f, intr_f, dist_f, calib_fs}.at(t0) : Calib{cam, intr, dist, 0};
  }
  float *det_all = nullptr, *c3f = nullptr;
  // Crop centres, truncated 3D centre and validity of a time batch: written by stage 2 (triangulation), read by
  // stage 3.  TWO sets: the staged entry points alternate between them, so that stage 3 of time batch i may run
  // on a second stream while stage 2 of batch i+1 (which writes the other set) is under way -- a stage-3 call
  // reads the set of the stage-2 call that preceded it in host call order (distributed.py).  The whole-path
  // forward always uses set 0 (its captured graph bakes the pointers).
  struct CentreSet { int *c3i = nullptr, *chm = nullptr, *valid = nullptr; };
  CentreSet cset[2];
  int slot = 0;
  const CentreSet& cur() const { return cset[slot]; }
  float2* coarse = nullptr;
  double* sa_partial = nullptr;
  int* sa_max = nullptr;
  // hipGraph replay of the whole forward (the reference driver's call pattern: one frame set per
  // call, predict3D.py:82-85 -- 150+ launches of small kernels, launch-bound when issued one by one)
  int use_graph = 0;
  const void** frames_cell = nullptr;        // device: the frame pointer of the current call
  // per-image frames (jh_predictor_forward_images): [T * C] device pointers, written on the caller's stream before
  // every such forward; the launches, captured or not, read this table.  Allocated by the first such call.
  const void** frames_table = nullptr;
  float *g_points = nullptr, *g_conf = nullptr;
  hipStream_t gstream = nullptr;             // capture stream (the caller's may be the null stream)
  // One slot per ForwardForm.  A launch carries its source's description by value, so a recording has ONE source: the
  // slot keeps the FrameSource its graph was captured with, and a call with another one records again (forward_graph).
  // The same holds for the calibration's form: a recording holds the pointers and the frame stride (calib_fs) it was
  // captured with.
  struct GraphSlot { hipGraphExec_t exec = nullptr; FrameSource src; int calib_fs = 0; };
  GraphSlot gslot[kGraphSlots];
  // Camera mask (nets.h).  mask_buf [T][C]: the predictor's copy of the mask of a whole-path forward -- the masked
  // kernels (and a captured graph of them) read this buffer, so the mask may change from call to call.
  // n_active / n_detect [T]: written by the masked triangulation.
  unsigned char* mask_buf = nullptr;
  int *n_active = nullptr, *n_detect = nullptr;
  // Caller-supplied centres (jh_predictor_set_centers).  centers_buf [T][3]: the predictor's copy of the centres in
  // force, allocated by the first such call -- the centred stage 2 (and a captured graph of it) reads this buffer, so
  // the centres may change from call to call.  centers_on: stage 1 is skipped and stage 2 takes its centres from the
  // buffer (launch_centers) instead of triangulating detections.
  float* centers_buf = nullptr;
  bool centers_on = false;
  // (max, index) partials of the all-joint argmax behind jh_predictor_views2d, [T3 * C][slices][Jp] each: allocated
  // by the first such call, so a predictor that never asks for 2D views owns what it always did
  float* v2d_max = nullptr;
  int* v2d_idx = nullptr;
  // Per-joint triangulation (jh_predictor_triangulate_joints): the observations [T3 * C][J][3] of a call that brings no
  // buffer for them, allocated by the first such call; the scan's partials above are shared with the 2D views
  float* j3_obs = nullptr;
  // Several subjects (jh_predictor_detect_subjects): peaks [T * C][kMaxPeaks][3], counts [T * C] and the global-form
  // scratch of the peak kernel (none where the heat map fits the LDS), ONE allocation made by the first such call
  float* subj_peaks = nullptr;
  int* subj_count = nullptr;
  void* subj_ws = nullptr;
  // Per-joint 3D spread (jh_predictor_set_spread).  spread_on: run_3d launches the spread form of the soft-argmax tail,
  // which writes rows t0 .. t0+T3-1 of sp_cov (T,J,6), sp_peak (T,J,3) and sp_mass (T,J); spread.sums / .key: its
  // accumulators for one 3D chunk.  All of it ONE allocation of spread_bytes, made by the first enabling call: a
  // predictor that never asks owns, and launches, what it always did.
  bool spread_on = false;
  SoftargmaxSpread spread;
  float *sp_cov = nullptr, *sp_peak = nullptr, *sp_mass = nullptr;
  size_t spread_bytes = 0;
  // Per-joint camera masks (jh_predictor_set_joint_mask).  jm_mode: JH_JOINT_MASK_*; while it is not off the whole-path
  // forward runs eagerly and gives stage 3 jm_buf [T][J][C] -- the caller's mask (GIVEN), or the members of the
  // consensus over its own heat maps, written between stage 2 and stage 3 with jm_params (CONSENSUS; jm_points /
  // jm_views / jm_error take the consensus' other outputs).  jm_sets: the workspace of the gather for one 3D chunk and,
  // in eff [T][J][C] / cnt [T][J], the effective sets of the last joint-masked stage 3, rows t0 .. t0+T3-1.
  // All of it allocated by the first call that asks (joint_mask_workspace), never by jh_predictor_create.
  int jm_mode = 0;
  unsigned char* jm_buf = nullptr;
  JointSets jm_sets;
  Joints3dParams jm_params{};
  float *jm_points = nullptr, *jm_error = nullptr;
  int* jm_views = nullptr;
  ~jh_predictor() {
    for (auto& g : gslot) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (gstream) (void)hipStreamDestroy(gstream);
  }

  // 3D stage for frames t0 .. t0+T3-1 of the batch (heat_all holds those frames)
  int run_3d(const Call& call, const float* heat_all, int t0, float* heatmap_final, float* points, float* conf,
             const HeatLayout* layout = nullptr) {
    hipStream_t s = call.s;
    const double g3 = (double)G * G * G;
    // algorithmic traffic of the gather: every heatmap byte once in, the volume once out
    // (under a mask as for all cameras: an upper bound, the unmasked cameras' heatmaps are what is read)
    if (call.joint_mask) {
      // (the sets of the chunk, then the gather; the effective sets land in rows t0 .. of eff / cnt)
      JointSets js = jm_sets;
      js.eff += (size_t)t0 * J * C; js.cnt += (size_t)t0 * J;
      JH_PROF("reproject_gather_joint_masked", 0.0, 4.0 * T3 * ((double)C * Hh * Hh * J + g3 * J),
              launch_reproject_joint_masked(calib_at(t0), cur().c3i + t0 * 3, cur().chm + t0 * C * 2, heat_all, coarse,
                                            v2v->input.p, nullptr, T3, C, G, cfg.grid_spacing, hs, J, Jp, /*heat_pad=*/0,
                                            /*div255=*/1, call.mask ? call.mask + (size_t)t0 * C : nullptr,
                                            call.joint_mask + (size_t)t0 * J * C, js, s, layout));
    } else {
      JH_PROF(call.mask ? "reproject_gather_masked" : "reproject_gather", 0.0,
              4.0 * T3 * ((double)C * Hh * Hh * J + g3 * J),
              launch_reproject(calib_at(t0), cur().c3i + t0 * 3, cur().chm + t0 * C * 2, heat_all, coarse, v2v->input.p,
                               nullptr, T3, C, G, cfg.grid_spacing, hs, Jp, /*heat_pad=*/0, /*div255=*/1,
                               call.mask ? call.mask + (size_t)t0 * C : nullptr, s, layout));
    }
    if (v2v->run(s)) return 1;
    SoftargmaxSpread sp = spread;
    if (spread_on) {
      sp.valid = cur().valid + t0;
      sp.cov = sp_cov + (size_t)t0 * J * 6; sp.peak = sp_peak + (size_t)t0 * J * 3; sp.mass = sp_mass + (size_t)t0 * J;
    }
    JH_PROF(spread_on ? "softargmax_spread" : "softargmax", 0.0, 4.0 * T3 * (g3 / 8) * J,
            launch_softargmax(v2v->output.p, cur().c3i + t0 * 3, sa_partial, sa_max, points, conf, heatmap_final, T3, J,
                              Jp, Gh, cfg.grid_spacing, cfg.roi_cube_size, s, spread_on ? &sp : nullptr));
    return 0;
  }
};

extern "C" {

int jh_predictor_create(const jh_params* center_params, const jh_params* hybrid_params,
                        const jh_predictor_config* cfg, jh_predictor** out) {
  JH_REQUIRE(hybrid_params && cfg && out, "bad argument");
  std::unique_ptr<jh_predictor> pr(new jh_predictor());
  pr->cfg = *cfg;
  pr->T = cfg->time_batch; pr->C = cfg->num_cameras; pr->Cloc = cfg->cam_n;
  pr->T3 = cfg->time_batch_3d > 0 ? cfg->time_batch_3d : cfg->time_batch;
  JH_REQUIRE(pr->T3 <= pr->T, "time_batch_3d must not exceed time_batch");
  pr->J = cfg->num_joints; pr->Jp = cpad(cfg->num_joints);
  pr->B = cfg->bbox; pr->Hh = cfg->bbox / 2; pr->hs = cfg->bbox / 2 + 2;
  pr->G = (int)(cfg->roi_cube_size / cfg->grid_spacing);
  pr->Gh = pr->G / 2;
  JH_REQUIRE(pr->T >= 1 && pr->C >= 1 && pr->C <= 64, "time batch / camera count");
  JH_REQUIRE(cfg->cam_lo >= 0 && cfg->cam_n >= 1 && cfg->cam_lo + cfg->cam_n <= pr->C, "camera range");
  JH_REQUIRE(pr->G % 4 == 0, "ROI_CUBE_SIZE / GRID_SPACING must be a multiple of 4");
  const int N = pr->T * pr->Cloc;
  // (form of the BiFPN nodes: by the time batch alone, see EffTrackPlan::node_class)
  const NodeBatchClass node_class = pr->T >= 8 ? NodeBatchClass::AtLeast8 : NodeBatchClass::Below8;
  // (... and with it the blocking of the InstanceNorm / pooled-sum passes, Plan::norm_block_kb; JH_NODE_ROWS=0 switches
  //  every class-dependent form off: one arithmetic for all time batches)
  const int norm_kb = node_class == NodeBatchClass::AtLeast8 && JH_ENV_KNOB("JH_NODE_ROWS") != 0 ? 64 : 0;
  PlanSetup setup;
  if (setup.init(&pr->cfg, node_class, norm_kb)) return 1;
  if (center_params) {
    pr->center = setup.efftrack();
    if (pr->center->build(center_params->map, "", cfg->center_model, 1, N, cfg->center_size,
                          cfg->center_size)) return 1;
  }
  pr->kp = setup.efftrack();
  if (pr->kp->build(hybrid_params->map, "effTrack.", cfg->kp_model, pr->J, N, pr->B, pr->B)) return 1;
  pr->v2v.reset(new V2VPlan());
  pr->v2v->precision = setup.precision;
  pr->v2v->norm_block_kb = norm_kb;
  if (pr->v2v->build(hybrid_params->map, "v2vNet.", pr->J, pr->T3, pr->G)) return 1;
  auto& m = pr->mem;
  const int T = pr->T, C = pr->C;
  if (m.get(reinterpret_cast<void**>(&pr->cam), (size_t)C * 12 * sizeof(float))) return 1;
  if (m.get(reinterpret_cast<void**>(&pr->intr), (size_t)C * 9 * sizeof(float))) return 1;
  if (m.get(reinterpret_cast<void**>(&pr->dist), (size_t)C * 5 * sizeof(float))) return 1;
  if (m.get(reinterpret_cast<void**>(&pr->det_all), (size_t)T * C * 3 * sizeof(float))) return 1;
  if (m.get(reinterpret_cast<void**>(&pr->c3f), (size_t)T * 3 * sizeof(float))) return 1;
  for (auto& cs : pr->cset) {
    if (m.get(reinterpret_cast<void**>(&cs.c3i), (size_t)T * 3 * sizeof(int))) return 1;
    if (m.get(reinterpret_cast<void**>(&cs.chm), (size_t)T * C * 2 * sizeof(int))) return 1;
    if (m.get(reinterpret_cast<void**>(&cs.valid), (size_t)T * sizeof(int))) return 1;
  }
  if (m.get(reinterpret_cast<void**>(&pr->coarse),
            (size_t)pr->T3 * C * pr->Gh * pr->Gh * pr->Gh * sizeof(float2))) return 1;
  {   // soft-argmax accumulators and maxima in ONE allocation (zeroed by one launch per forward)
    const size_t pb = (size_t)T * pr->Jp * 4 * kLimbs * sizeof(double), mb = (size_t)T * pr->Jp * sizeof(int);
    if (m.get(reinterpret_cast<void**>(&pr->sa_partial), pb + mb)) return 1;
    pr->sa_max = reinterpret_cast<int*>(reinterpret_cast<char*>(pr->sa_partial) + pb);
  }
  for (auto& cs : pr->cset) JH_CHECK_HIP(hipMemset(cs.valid, 0, (size_t)T * sizeof(int)));
  if (m.get(reinterpret_cast<void**>(&pr->mask_buf), (size_t)T * C)) return 1;
  if (m.get(reinterpret_cast<void**>(&pr->n_active), (size_t)T * sizeof(int))) return 1;
  if (m.get(reinterpret_cast<void**>(&pr->n_detect), (size_t)T * sizeof(int))) return 1;
  JH_CHECK_HIP(hipMemset(pr->mask_buf, 1, (size_t)T * C));
  JH_CHECK_HIP(hipMemset(pr->n_active, 0, (size_t)T * sizeof(int)));
  JH_CHECK_HIP(hipMemset(pr->n_detect, 0, (size_t)T * sizeof(int)));
  // graph replay: by default for the single-frame-set call (T = 1), where the forward is
  // launch-bound; JH_GRAPH=1 / 0 forces it on / off for every time batch
  const int knob = JH_ENV_KNOB("JH_GRAPH");
  pr->use_graph = knob >= 0 ? (knob != 0) : (pr->T == 1);
  if (pr->Cloc == pr->C && pr->T3 == pr->T && pr->center) {
    if (m.get(reinterpret_cast<void**>(&pr->frames_cell), 256)) return 1;
    if (m.get(reinterpret_cast<void**>(&pr->g_points), (size_t)T * pr->J * 3 * sizeof(float))) return 1;
    if (m.get(reinterpret_cast<void**>(&pr->g_conf), (size_t)T * pr->J * sizeof(float))) return 1;
    // (the capture stream itself is created on first use: HIP multiplexes streams onto a few hardware
    // queues, and an idle extra stream per predictor was seen to put the caller's copy stream on the
    // compute stream's queue -- the overlapped uint8 upload of bench.py fell from 1135 to 705 frames/s)
  } else {
    pr->use_graph = 0;
  }
  JH_CHECK_HIP(hipDeviceSynchronize());
  *out = pr.release();
  return 0;
}

void jh_predictor_destroy(jh_predictor* pr) { delete pr; }

int jh_predictor_set_graph_replay(jh_predictor* pr, int on) {
  JH_REQUIRE(pr, "bad argument");
  JH_REQUIRE(!on || pr->frames_cell, "graph replay needs a predictor that owns all cameras and CenterDetect");
  pr->use_graph = on != 0;
  return 0;
}
int jh_predictor_graph_replay(const jh_predictor* pr) { return pr ? pr->use_graph : 0; }

int64_t jh_predictor_launches(const jh_predictor* pr) {
  return (int64_t)((pr->center ? pr->center->launches() : 0) + pr->kp->launches() +
                   pr->v2v->launches());
}
int jh_predictor_precision(const jh_predictor* pr) { return pr ? pr->cfg.precision : -1; }

int64_t jh_predictor_device_bytes(const jh_predictor* pr) {
  return (int64_t)((pr->center ? pr->center->device_bytes() : 0) + pr->kp->device_bytes() +
                   pr->v2v->device_bytes() + pr->spread_bytes);
}

int jh_predictor_set_calibration(jh_predictor* pr, const float* cam_dev, const float* intr_dev,
                                 const float* dist_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_CHECK_HIP(hipMemcpyAsync(pr->cam, cam_dev, (size_t)pr->C * 12 * sizeof(float), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->intr, intr_dev, (size_t)pr->C * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->dist, dist_dev, (size_t)pr->C * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
  pr->calib_fs = 0;                           // (back to the shared form, if the per-frame one was in use)
  return 0;
}

int jh_predictor_set_calibration_frames(jh_predictor* pr, const float* cam_dev, const float* intr_dev,
                                        const float* dist_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_set_calibration_frames: null predictor");
  JH_REQUIRE(cam_dev && intr_dev && dist_dev, "jh_predictor_set_calibration_frames: null calibration pointer");
  const size_t rows = (size_t)pr->T * pr->C;
  if (!pr->cam_f) {
    // (one allocation: cam_f is set last, so a failure leaves the predictor as it was)
    float* base = nullptr;
    if (first_call_alloc(pr->mem, s, rows * 26 * sizeof(float), "the first jh_predictor_set_calibration_frames call of "
                         "a predictor allocates its per-frame calibration: make it outside a stream capture", &base))
      return 1;
    pr->intr_f = base + rows * 12;
    pr->dist_f = base + rows * 21;
    pr->cam_f = base;
  }
  JH_CHECK_HIP(hipMemcpyAsync(pr->cam_f, cam_dev, rows * 12 * sizeof(float), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->intr_f, intr_dev, rows * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->dist_f, dist_dev, rows * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
  pr->calib_fs = pr->C;
  return 0;
}

int jh_predictor_set_centers(jh_predictor* pr, const float* centers_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_set_centers: null predictor");
  if (!centers_dev) {                         // (back to detection; the buffer stays for the next centred call)
    pr->centers_on = false;
    return 0;
  }
  if (!pr->centers_buf &&
      first_call_alloc(pr->mem, s, (size_t)pr->T * 3 * sizeof(float), "the first jh_predictor_set_centers call of a "
                       "predictor allocates its centre buffer: make it outside a stream capture", &pr->centers_buf))
    return 1;
  JH_CHECK_HIP(hipMemcpyAsync(pr->centers_buf, centers_dev, (size_t)pr->T * 3 * sizeof(float), hipMemcpyDeviceToDevice,
                              s));
  pr->centers_on = true;
  return 0;
}

int jh_predictor_set_spread(jh_predictor* pr, int on) {
  JH_REQUIRE(pr, "jh_predictor_set_spread: null predictor");
  if (on && !pr->sp_cov) {
    // (allocates and clears: not inside a stream capture -- the call has no stream to ask, the allocation itself
    // fails there)
    const size_t T = pr->T, J = pr->J, Jp = pr->Jp;
    const size_t nsum = softargmax_spread_sums(pr->T3, pr->Jp), nkey = (size_t)pr->T3 * Jp;
    const size_t bytes = (nsum + nkey) * sizeof(double) + T * J * 10 * sizeof(float);
    char* base = nullptr;
    if (pr->mem.get(reinterpret_cast<void**>(&base), bytes)) return 1;
    JH_CHECK_HIP(hipMemset(base, 0, bytes));
    pr->spread.sums = reinterpret_cast<double*>(base);
    pr->spread.key = reinterpret_cast<unsigned long long*>(pr->spread.sums + nsum);
    float* f = reinterpret_cast<float*>(pr->spread.key + nkey);
    pr->sp_peak = f + T * J * 6;
    pr->sp_mass = f + T * J * 9;
    pr->sp_cov = f;
    pr->spread_bytes = bytes;
  }
  pr->spread_on = on != 0;
  return 0;
}

int jh_predictor_get_spread(jh_predictor* pr, float* cov_dev, float* peak_dev, float* mass_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_get_spread: null predictor");
  JH_REQUIRE(pr->sp_cov, "jh_predictor_get_spread: the spread was never enabled (jh_predictor_set_spread)");
  const size_t n = (size_t)pr->T * pr->J * sizeof(float);
  if (cov_dev) JH_CHECK_HIP(hipMemcpyAsync(cov_dev, pr->sp_cov, n * 6, hipMemcpyDeviceToDevice, s));
  if (peak_dev) JH_CHECK_HIP(hipMemcpyAsync(peak_dev, pr->sp_peak, n * 3, hipMemcpyDeviceToDevice, s));
  if (mass_dev) JH_CHECK_HIP(hipMemcpyAsync(mass_dev, pr->sp_mass, n, hipMemcpyDeviceToDevice, s));
  return 0;
}

int jh_predictor_debug_v2v(jh_predictor* pr, float* out_dev, void* stream) {
  JH_REQUIRE(pr && out_dev, "jh_predictor_debug_v2v: null pointer");
  return launch_from_channel_last(pr->v2v->output, out_dev, static_cast<hipStream_t>(stream));
}

// Stage 1 up to CenterDetect's heat map (pr->center->heat): resize or fused stem, then the plan
static int center_heat_impl(jh_predictor* pr, const Call& call) {
  hipStream_t s = call.s;
  const FrameSource& fs = call.fs;
  JH_REQUIRE(pr->center, "predictor was created without CenterDetect weights");
  const int N = pr->T * pr->Cloc, S = pr->cfg.center_size;
  if (pr->center->stem_fusable) {
    // resize + normalise happen inside the stem convolution's patch staging (csrc/stem.hip)
    StemSource& src = pr->center->stem_src;
    src.mode = 1; src.frames = call.frames; src.frames_cell = call.cell; src.source = fs;
    src.H = pr->cfg.img_h; src.W = pr->cfg.img_w;
    for (int i = 0; i < 3; ++i) { src.mean[i] = pr->cfg.mean[i]; src.stdv[i] = pr->cfg.std[i]; }
    // algorithmic bytes of the fused launch: the four bilinear taps of every network-input pixel (px_bytes
    // each) + the stem's output at half resolution (16 or 32 channels = 16 or 32 B per input pixel)
    pr->center->set_stem_traffic((double)N * S * S * (4.0 * fs.px_bytes() + pr->center->stem_channels()));
  } else {
    JH_PROF("preprocess_resize", 0.0, (double)N * S * S * (4.0 * fs.px_bytes() + 3 * 4),
            launch_preprocess_resize(call.frames, fs, pr->center->input.p, N, pr->cfg.img_h,
                                     pr->cfg.img_w, S, pr->cfg.mean, pr->cfg.std, s, call.cell));
  }
  return pr->center->run(s);
}

static int stage_center_impl(jh_predictor* pr, const Call& call, float* det_dev) {
  hipStream_t s = call.s;
  if (center_heat_impl(pr, call)) return 1;
  const int N = pr->T * pr->Cloc;
  const Act& h = pr->center->heat;
  JH_PROF("center_argmax", 0.0, 4.0 * N * h.H * h.W,
          launch_center_argmax(h.p, det_dev, N, h.H, h.W, h.Cp, s));
  return 0;
}

int jh_predictor_stage_center(jh_predictor* pr, const float* frames_dev, float* det_dev,
                              void* stream) {
  return stage_center_impl(pr, make_call(frames_dev, fixed_source(kSrcRgbF32), stream), det_dev);
}
int jh_predictor_stage_center_u8(jh_predictor* pr, const uint8_t* frames_dev, float* det_dev,
                                 void* stream) {
  return stage_center_impl(pr, make_call(frames_dev, fixed_source(kSrcBgrU8), stream), det_dev);
}

static int stage_keypoints_impl(jh_predictor* pr, const Call& call, const float* det_all_dev, float* heat_dev,
                                int det_blocks = 1, bool next_centre_set = false) {
  hipStream_t s = call.s;
  const FrameSource& fs = call.fs;
  const auto& c = pr->cfg;
  if (next_centre_set) pr->slot ^= 1;        // (the staged API: the previous batch's stage 3 may still read the other set)
  if (pr->centers_on) {                      // (no detections are read, none are kept: `det` may be NULL)
    det_blocks = 1;
    det_all_dev = pr->det_all;
  }
  if (det_blocks > 1) {
    JH_REQUIRE(pr->C % det_blocks == 0, "cameras must divide evenly over the detection blocks");
    const int n = pr->T * pr->C * 3;
    hipLaunchKernelGGL(det_unblock_kernel, dim3((n + 255) / 256), dim3(256), 0, s, det_all_dev, pr->det_all,
                       pr->T, pr->C, pr->C / det_blocks);
    JH_CHECK_HIP(hipGetLastError());
    det_all_dev = pr->det_all;
  }
  const jh_predictor::CentreSet& cs = pr->cur();
  if (pr->centers_on) {
    // the centres of jh_predictor_set_centers in place of a triangulation
    JH_PROF("centers", 0.0, 0.0,
            launch_centers(pr->centers_buf, pr->calib_at(0), pr->c3f, cs.c3i, cs.chm, cs.valid, pr->T, pr->C, pr->B / 2,
                           c.img_w, c.img_h, call.mask, pr->n_active, pr->n_detect, s));
  } else {
    const Scale2 k = center_scale2(c);
    JH_PROF(call.mask ? "triangulate_masked" : "triangulate", 0.0, 0.0,
            launch_triangulate(det_all_dev, pr->calib_at(0), pr->c3f, cs.c3i, cs.chm, cs.valid, pr->T, pr->C, k.x, k.y,
                               255.f, pr->B / 2, c.img_w, c.img_h, call.mask, pr->n_active, pr->n_detect, s));
  }
  if (det_all_dev != pr->det_all)
    JH_CHECK_HIP(hipMemcpyAsync(pr->det_all, det_all_dev, (size_t)pr->T * pr->C * 3 * sizeof(float),
                                hipMemcpyDeviceToDevice, s));
  if (pr->kp->stem_fusable) {
    // crop + normalise happen inside the stem convolution's patch staging (csrc/stem.hip)
    StemSource& src = pr->kp->stem_src;
    src.mode = 2; src.frames = call.frames; src.frames_cell = call.cell; src.source = fs;
    src.center_hm = cs.chm; src.Cloc = pr->Cloc; src.C = pr->C; src.cam0 = c.cam_lo;
    src.H = c.img_h; src.W = c.img_w;
    for (int i = 0; i < 3; ++i) { src.mean[i] = c.mean[i]; src.stdv[i] = c.std[i]; }
    pr->kp->set_stem_traffic((double)pr->T * pr->Cloc * pr->B * pr->B * (fs.px_bytes() + pr->kp->stem_channels()));
  } else {
    JH_PROF("preprocess_crop", 0.0, (double)pr->T * pr->Cloc * pr->B * pr->B * (fs.px_bytes() + 12.0),
            launch_preprocess_crop(call.frames, fs, cs.chm, pr->kp->input.p, pr->T, pr->Cloc, pr->C,
                                   c.cam_lo, c.img_h, c.img_w, pr->B, c.mean, c.std, s, call.cell));
  }
  if (pr->kp->run(s)) return 1;
  if (heat_dev && heat_dev != pr->kp->heat.p)
    JH_CHECK_HIP(hipMemcpyAsync(heat_dev, pr->kp->heat.p, pr->kp->heat.bytes(),
                                hipMemcpyDeviceToDevice, s));
  return 0;
}

int jh_predictor_stage_keypoints(jh_predictor* pr, const float* frames_dev,
                                 const float* det_all_dev, float* heat_dev, void* stream) {
  return stage_keypoints_impl(pr, make_call(frames_dev, fixed_source(kSrcRgbF32), stream), det_all_dev, heat_dev, 1,
                              true);
}
int jh_predictor_stage_keypoints_u8(jh_predictor* pr, const uint8_t* frames_dev,
                                    const float* det_all_dev, float* heat_dev, void* stream) {
  return stage_keypoints_impl(pr, make_call(frames_dev, fixed_source(kSrcBgrU8), stream), det_all_dev, heat_dev, 1,
                              true);
}

int jh_predictor_stage_keypoints_gathered(jh_predictor* pr, const void* frames_dev, int frames_u8,
                                          const float* det_gathered_dev, int n_blocks, float* heat_dev,
                                          void* stream) {
  JH_REQUIRE(n_blocks >= 1, "block count");
  return stage_keypoints_impl(pr, make_call(frames_dev, fixed_source(frames_u8 ? kSrcBgrU8 : kSrcRgbF32), stream),
                              det_gathered_dev, heat_dev, n_blocks, true);
}

static int stage_3d_impl(jh_predictor* pr, const Call& call, const float* heat_all_dev, int t0, float* points_dev,
                         float* conf_dev, int32_t* valid_dev, const HeatLayout* layout = nullptr) {
  JH_REQUIRE(t0 >= 0 && t0 + pr->T3 <= pr->T, "frame range of the 3D stage");
  if (pr->run_3d(call, heat_all_dev, t0, nullptr, points_dev, conf_dev, layout)) return 1;
  if (valid_dev)
    JH_CHECK_HIP(hipMemcpyAsync(valid_dev, pr->cur().valid + t0, (size_t)pr->T3 * sizeof(int),
                                hipMemcpyDeviceToDevice, call.s));
  return 0;
}

int jh_predictor_stage_3d(jh_predictor* pr, const float* heat_all_dev, int t0, float* points_dev,
                          float* conf_dev, int32_t* valid_dev, void* stream) {
  return stage_3d_impl(pr, stage3_call(stream), heat_all_dev, t0, points_dev, conf_dev, valid_dev);
}

int jh_predictor_stage_3d_blocks(jh_predictor* pr, const float* heat_blocks_dev, int n_blocks,
                                 int frames_per_block, int t_off, int t0, float* points_dev,
                                 float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(n_blocks >= 1 && pr->C % n_blocks == 0, "cameras must divide evenly over the blocks");
  JH_REQUIRE(t_off >= 0 && t_off + pr->T3 <= frames_per_block, "frame range inside a block");
  HeatLayout lay;
  const size_t plane = (size_t)pr->Hh * pr->Hh * pr->Jp;
  lay.cams_per_block = pr->C / n_blocks;
  lay.frame_stride = (size_t)lay.cams_per_block * plane;
  lay.block_stride = (size_t)frames_per_block * lay.frame_stride;
  return stage_3d_impl(pr, stage3_call(stream), heat_blocks_dev + (size_t)t_off * lay.frame_stride, t0, points_dev,
                       conf_dev, valid_dev, &lay);
}

// the three launches of jh_predictor_triangulate_joints (defined with it, below)
static int triangulate_joints_launches(jh_predictor* pr, const float* heat_all_dev, int t0, const unsigned char* mask_dev,
                                       const Joints3dParams& jp, float* points_dev, int* views_dev,
                                       unsigned char* members_dev, float* error_dev, float* obs_dev, hipStream_t s);

static int forward_eager(jh_predictor* pr, const Call& call, float* points_dev, float* conf_dev, int32_t* valid_dev) {
  // (centres supplied by the caller: stage 1 does not run at all)
  if (!pr->centers_on && stage_center_impl(pr, call, pr->det_all)) return 1;
  if (stage_keypoints_impl(pr, call, pr->det_all, nullptr)) return 1;
  // JH_JOINT_MASK_CONSENSUS: the members of the per-joint consensus over the heat maps stage 2 has just written -- the
  // call's camera mask, the centre set stage 2 wrote and the calibration in force -- become the joint mask of stage 3
  // (an invalid frame set has no members: its joints fall back)
  if (call.joint_mask && pr->jm_mode == JH_JOINT_MASK_CONSENSUS &&
      triangulate_joints_launches(pr, pr->kp->heat.p, 0, call.mask, pr->jm_params, pr->jm_points, pr->jm_views,
                                  pr->jm_buf, pr->jm_error, pr->j3_obs, call.s)) return 1;
  return stage_3d_impl(pr, call, pr->kp->heat.p, 0, points_dev, conf_dev, valid_dev);
}

// The forward as ONE graph launch.  Captured on first use (on the predictor's own stream: the
// caller's may be the null stream, which cannot capture) with the frame pointer read through
// `frames_cell` and the results written to the predictor's own buffers, so the same executable
// graph serves every later call: set the cell, launch the graph, copy the results out -- three
// submissions instead of ~150.  Calibration lives in the predictor's buffers (set_calibration
// copies into them), weights are immutable for the life of a predictor: nothing to invalidate.
static int forward_graph(jh_predictor* pr, const Call& call, float* points_dev, float* conf_dev, int32_t* valid_dev) {
  hipStream_t s = call.s;
  const FrameSource& fs = call.fs;
  const ForwardForm form{fs.fmt, call.mask != nullptr, fs.per_image, pr->centers_on, pr->spread_on};
  jh_predictor::GraphSlot& slot = pr->gslot[form.index()];
  // the recorded launches hold the description they were captured with: another one records again (rare: a stream
  // keeps its layout, and a fixed format has nothing to differ in; the replay in flight is waited for before its
  // executable graph goes).  Likewise the calibration's form, shared or per frame: its pointers and frame stride are
  // in the recording.  Its VALUES are not: they live in the predictor's buffers.
  if (slot.exec && (slot.src != fs || slot.calib_fs != pr->calib_fs)) {
    JH_CHECK_HIP(hipStreamSynchronize(s));
    (void)hipGraphExecDestroy(slot.exec);
    slot.exec = nullptr;
  }
  if (!slot.exec) {
    hipGraph_t g = nullptr;
    if (!pr->gstream) JH_CHECK_HIP(hipStreamCreateWithFlags(&pr->gstream, hipStreamNonBlocking));
    JH_CHECK_HIP(hipStreamBeginCapture(pr->gstream, hipStreamCaptureModeRelaxed));
    // the recording: this call on the capture stream, its frame pointer read through the cell (per-image: through the
    // table, as every such call)
    Call rec = call;
    rec.s = pr->gstream;
    rec.frames = nullptr;
    if (!fs.per_image) rec.cell = pr->frames_cell;
    const int rc = forward_eager(pr, rec, pr->g_points, pr->g_conf, nullptr);
    const hipError_t e = hipStreamEndCapture(pr->gstream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return 1; }
    JH_CHECK_HIP(e);
    const hipError_t ei = hipGraphInstantiate(&slot.exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) slot.exec = nullptr;
    JH_CHECK_HIP(ei);
    slot.src = fs;
    slot.calib_fs = pr->calib_fs;
  }
  // (per-image: the recording reads frames_table, which this call's pointers have already been sent into)
  if (!fs.per_image) hipLaunchKernelGGL(set_cell_kernel, dim3(1), dim3(1), 0, s, pr->frames_cell, call.frames);
  JH_CHECK_HIP(hipGetLastError());
  JH_CHECK_HIP(hipGraphLaunch(slot.exec, s));
  const int n_pts = pr->T * pr->J * 3;
  hipLaunchKernelGGL(copy_out_kernel, dim3((n_pts + 255) / 256), dim3(256), 0, s, pr->g_points, pr->g_conf,
                     pr->cset[0].valid, points_dev, conf_dev, valid_dev, n_pts, pr->T * pr->J, pr->T);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

// mask_dev != nullptr: the masked kernels, reading the predictor's copy of the mask (made here, on the caller's
// stream, outside any graph of the predictor's own: the captured launches keep pointing at mask_buf)
static int forward_impl(jh_predictor* pr, const void* frames_dev, const FrameSource& fs, float* points_dev,
                        float* conf_dev, int32_t* valid_dev, void* stream,
                        const unsigned char* mask_dev = nullptr) {
  if (mask_dev)
    JH_CHECK_HIP(hipMemcpyAsync(pr->mask_buf, mask_dev, (size_t)pr->T * pr->C, hipMemcpyDeviceToDevice,
                                static_cast<hipStream_t>(stream)));
  Call call = make_call(frames_dev, fs, stream, mask_dev ? pr->mask_buf : nullptr);
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "forward needs all cameras local");
  JH_REQUIRE(pr->T3 == pr->T, "forward needs time_batch_3d == time_batch");
  JH_REQUIRE(frames_dev && points_dev && conf_dev, "null frame / output pointer");
  pr->slot = 0;                               // (the whole-path forward and its captured graph: centre set 0)
  // a joint mask in force (jh_predictor_set_joint_mask): plain launches, no graph slot of its own -- the captured
  // graphs stay as they are and replay again once the mode is off
  if (pr->jm_mode != JH_JOINT_MASK_OFF) {
    call.joint_mask = pr->jm_buf;
    return forward_eager(pr, call, points_dev, conf_dev, valid_dev);
  }
  // per-launch profiling needs the launches one by one; a caller that is itself capturing this
  // stream gets the plain launches too (its graph then holds them)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (pr->use_graph && !profiler().on) (void)hipStreamIsCapturing(call.s, &cs);
  if (!pr->use_graph || profiler().on || cs != hipStreamCaptureStatusNone)
    return forward_eager(pr, call, points_dev, conf_dev, valid_dev);
  return forward_graph(pr, call, points_dev, conf_dev, valid_dev);
}
int jh_predictor_forward(jh_predictor* pr, const float* frames_dev, float* points_dev,
                         float* conf_dev, int32_t* valid_dev, void* stream) {
  return forward_impl(pr, frames_dev, fixed_source(kSrcRgbF32), points_dev, conf_dev, valid_dev, stream);
}
int jh_predictor_forward_u8(jh_predictor* pr, const uint8_t* frames_dev, float* points_dev,
                            float* conf_dev, int32_t* valid_dev, void* stream) {
  return forward_impl(pr, frames_dev, fixed_source(kSrcBgrU8), points_dev, conf_dev, valid_dev, stream);
}

int jh_predictor_forward_yuv(jh_predictor* pr, const uint8_t* frames_dev, int format, float* points_dev,
                             float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(format == JH_FRAME_I420 || format == JH_FRAME_NV12, "jh_predictor_forward_yuv: format must be "
             "JH_FRAME_I420 or JH_FRAME_NV12");
  JH_REQUIRE(pr, "bad argument");
  FrameSource fs;
  if (frame_source(format, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward_impl(pr, frames_dev, fs, points_dev, conf_dev, valid_dev, stream);
}

int jh_yuv_surface_check(const jh_yuv_surface* surface, int h, int w) { return yuv_surface_check(surface, h, w); }

int jh_predictor_forward_surface(jh_predictor* pr, const uint8_t* frames_dev, const jh_yuv_surface* surface,
                                 const uint8_t* mask_dev, float* points_dev, float* conf_dev, int32_t* valid_dev,
                                 void* stream) {
  JH_REQUIRE(pr, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward_impl(pr, frames_dev, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
}

int jh_sensor_surface_check(const jh_sensor_surface* surface, int h, int w) {
  return sensor_surface_check(surface, h, w);
}

int jh_predictor_forward_sensor(jh_predictor* pr, const uint8_t* frames_dev, const jh_sensor_surface* surface,
                                const uint8_t* mask_dev, float* points_dev, float* conf_dev, int32_t* valid_dev,
                                void* stream) {
  JH_REQUIRE(pr, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward_impl(pr, frames_dev, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
}

int jh_predictor_forward_masked(jh_predictor* pr, const void* frames_dev, int format, const uint8_t* mask_dev,
                                float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr, "bad argument");
  JH_REQUIRE(format >= JH_FRAME_RGB_F32 && format <= JH_FRAME_NV12, "jh_predictor_forward_masked: unknown frame format");
  FrameSource fs;
  if (frame_source(format, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward_impl(pr, frames_dev, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
}

int jh_predictor_forward_images(jh_predictor* pr, const void* const* images_host, int n_images, int format,
                                const jh_yuv_surface* yuv, const jh_sensor_surface* sensor, const uint8_t* mask_dev,
                                float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr, "bad argument");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "forward needs all cameras local");
  FrameSource fs;
  if (call_source("forward_images", format, yuv, sensor, pr->cfg.img_h, pr->cfg.img_w, true, &fs)) return 1;
  if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, pr->T * pr->C, fs,
                    static_cast<hipStream_t>(stream))) return 1;
  // (the launches read the table: `frames` itself is not dereferenced)
  return forward_impl(pr, pr->frames_table, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
}

int jh_predictor_stage_keypoints_masked(jh_predictor* pr, const void* frames_dev, int format,
                                        const float* det_all_dev, const uint8_t* mask_dev, float* heat_dev,
                                        void* stream) {
  JH_REQUIRE(pr && mask_dev, "bad argument");
  JH_REQUIRE(format == JH_FRAME_RGB_F32 || format == JH_FRAME_BGR_U8, "masked stage 2: fp32 RGB or uint8 BGR frames");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "masked stage 2 needs all cameras local");
  return stage_keypoints_impl(pr, make_call(frames_dev, fixed_source(format), stream, mask_dev), det_all_dev, heat_dev,
                              1, true);
}

int jh_predictor_stage_3d_masked(jh_predictor* pr, const float* heat_all_dev, int t0, const uint8_t* mask_dev,
                                 float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && mask_dev, "bad argument");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "masked stage 3 needs all cameras local");
  return stage_3d_impl(pr, stage3_call(stream, mask_dev), heat_all_dev, t0, points_dev, conf_dev, valid_dev);
}

int jh_predictor_debug_mask(jh_predictor* pr, int32_t* n_active_dev, int32_t* num_cams_detect_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "bad argument");
  const size_t T = pr->T;
  if (n_active_dev) JH_CHECK_HIP(hipMemcpyAsync(n_active_dev, pr->n_active, T * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (num_cams_detect_dev) JH_CHECK_HIP(hipMemcpyAsync(num_cams_detect_dev, pr->n_detect, T * sizeof(int), hipMemcpyDeviceToDevice, s));
  return 0;
}

}  // extern "C"

// The (max, index) partials of the all-joint argmax for the T3 * C heat maps of a 3D chunk, shared by
// jh_predictor_views2d and jh_predictor_triangulate_joints: allocated by whichever is called first (`what`: its message
// for a call inside a stream capture).
static int scan_workspace(jh_predictor* pr, hipStream_t s, const char* what) {
  if (pr->v2d_max) return 0;
  // (two allocations: v2d_max is set last, so a failure leaves the predictor without either)
  const size_t n = joint_argmax_all_partials(pr->T3 * pr->C, pr->Hh, pr->Hh, pr->Jp);
  float* pmax = nullptr;
  if (first_call_alloc(pr->mem, s, n * sizeof(float), what, &pmax)) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->v2d_idx), n * sizeof(int))) return 1;
  pr->v2d_max = pmax;
  return 0;
}

// The scan's partials and, with own_obs, the predictor's own observation buffer [T3 * C][J][3] of the per-joint
// triangulation: each allocated by the first call that needs it.
static int triangulate_joints_workspace(jh_predictor* pr, hipStream_t s, bool own_obs, const char* what) {
  if (scan_workspace(pr, s, what)) return 1;
  if (own_obs && !pr->j3_obs &&
      first_call_alloc(pr->mem, s, (size_t)pr->T3 * pr->C * pr->J * 3 * sizeof(float), what, &pr->j3_obs)) return 1;
  return 0;
}

extern "C" {

int jh_predictor_views2d(jh_predictor* pr, const float* heat_all_dev, int t0, const float* points_dev,
                         const uint8_t* mask_dev, int32_t* points2d_dev, float* conf2d_dev, float* reproj_dev,
                         float* err_dev, uint8_t* used_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr && points_dev && points2d_dev && conf2d_dev && reproj_dev && err_dev && used_dev,
             "null pointer");
  JH_REQUIRE(t0 >= 0 && t0 + pr->T3 <= pr->T, "frame range of the 2D views");
  const int N = pr->T3 * pr->C;
  if (!heat_all_dev) {
    JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "the predictor's own heat maps hold all cameras only when "
               "all cameras are local");
    heat_all_dev = pr->kp->heat.p + (size_t)t0 * pr->C * pr->Hh * pr->Hh * pr->Jp;
  }
  if (scan_workspace(pr, s, "the first jh_predictor_views2d call of a predictor allocates its workspace: make it "
                     "outside a stream capture")) return 1;
  const double bytes = 4.0 * N * pr->Hh * pr->Hh * pr->Jp;
  JH_PROF("joint_argmax_all", 0.0, bytes,
          launch_joint_argmax_all(heat_all_dev, pr->v2d_max, pr->v2d_idx, N, pr->Hh, pr->Hh, pr->J, pr->Jp, s));
  // (the merge reads the partials of every slice and writes 24 B per (frame, camera, joint))
  const int slices = joint_argmax_all_shape(N, pr->Hh, pr->Hh, pr->Jp).slices;
  JH_PROF("views2d_final", 0.0, 8.0 * N * slices * pr->Jp + 24.0 * N * pr->J,
          launch_views2d_final(pr->v2d_max, pr->v2d_idx, pr->cur().chm + (size_t)t0 * pr->C * 2, pr->cur().valid + t0,
                               mask_dev ? mask_dev + (size_t)t0 * pr->C : nullptr, points_dev, pr->calib_at(t0),
                               points2d_dev, conf2d_dev, reproj_dev, err_dev, used_dev, pr->T3, pr->C, pr->J, pr->Jp,
                               pr->Hh, pr->Hh, pr->B / 2, s));
  return 0;
}

// ---- per-joint robust triangulation (csrc/joints3d.h)
static int joints3d_params(const jh_joints3d_params* p, Joints3dParams* out) {
  JH_REQUIRE(p, "null jh_joints3d_params");
  *out = Joints3dParams{p->min_views, p->refine_radius, p->min_conf, p->max_error_px};
  return joints3d_check(*out);
}

int jh_joints3d_params_check(const jh_joints3d_params* params) {
  Joints3dParams jp;
  return joints3d_params(params, &jp);
}

int jh_op_joint_peaks_refine(const float* heat_dev, int n, int hh, int wh, int jp, const int32_t* idx_dev, int j,
                             int radius, float* offsets_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(heat_dev && idx_dev && offsets_dev, "jh_op_joint_peaks_refine: null pointer");
  JH_REQUIRE(n >= 1 && hh >= 1 && wh >= 1 && (long long)hh * wh < (1ll << 30), "jh_op_joint_peaks_refine: heat map shape");
  JH_REQUIRE(j >= 1 && j <= jp && jp <= 1024, "jh_op_joint_peaks_refine: 1 <= j <= jp <= 1024");
  JH_REQUIRE(radius >= 0 && radius <= kMaxRefineRadius, "jh_op_joint_peaks_refine: radius must be 0 .. 3");
  if (launch_joint_peaks_refine(heat_dev, idx_dev, offsets_dev, n, hh, wh, j, jp, radius, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_triangulate_joints(const float* obs_dev, int t, int cams, int j, const float* cam_dev, const float* intr_dev,
                             const float* dist_dev, int calib_per_frame, const jh_joints3d_params* params,
                             float* points_dev, int32_t* views_dev, uint8_t* members_dev, float* error_dev,
                             void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  Joints3dParams jp;
  if (joints3d_params(params, &jp)) return 1;
  JH_REQUIRE(obs_dev && cam_dev && intr_dev && dist_dev && points_dev && views_dev && members_dev && error_dev,
             "jh_op_triangulate_joints: null pointer");
  JH_REQUIRE(t >= 1 && j >= 1, "jh_op_triangulate_joints: at least one frame set and one joint");
  JH_REQUIRE(cams >= 1 && cams <= 64, "jh_op_triangulate_joints: 1 .. 64 cameras");
  if (launch_joints3d(obs_dev, Calib{cam_dev, intr_dev, dist_dev, calib_per_frame ? cams : 0}, points_dev, views_dev,
                      members_dev, error_dev, t, cams, j, jp.min_views, jp.min_conf, jp.max_error_px, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_predictor_triangulate_joints(jh_predictor* pr, const float* heat_all_dev, int t0, const uint8_t* mask_dev,
                                    const jh_joints3d_params* params, float* points_dev, int32_t* views_dev,
                                    uint8_t* members_dev, float* error_dev, float* obs_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_triangulate_joints: null predictor");
  Joints3dParams jp;
  if (joints3d_params(params, &jp)) return 1;
  JH_REQUIRE(points_dev && views_dev && members_dev && error_dev, "jh_predictor_triangulate_joints: null output pointer");
  JH_REQUIRE(t0 >= 0 && t0 + pr->T3 <= pr->T, "frame range of the joint triangulation");
  if (!heat_all_dev) {
    JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "the predictor's own heat maps hold all cameras only when "
               "all cameras are local");
    heat_all_dev = pr->kp->heat.p + (size_t)t0 * pr->C * pr->Hh * pr->Hh * pr->Jp;
  }
  // (the observations go straight into the caller's buffer when there is one; the predictor's own, allocated by the
  // first call that brings none, otherwise)
  if (triangulate_joints_workspace(pr, s, !obs_dev, "the first jh_predictor_triangulate_joints call of a predictor "
                                   "allocates its workspace: make it outside a stream capture")) return 1;
  return triangulate_joints_launches(pr, heat_all_dev, t0, mask_dev, jp, points_dev, views_dev, members_dev, error_dev,
                                     obs_dev ? obs_dev : pr->j3_obs, s);
}

}  // extern "C"

static int triangulate_joints_launches(jh_predictor* pr, const float* heat_all_dev, int t0, const unsigned char* mask_dev,
                                       const Joints3dParams& jp, float* points_dev, int* views_dev,
                                       unsigned char* members_dev, float* error_dev, float* obs_dev, hipStream_t s) {
  const int N = pr->T3 * pr->C;
  JH_PROF("joint_argmax_all", 0.0, 4.0 * N * pr->Hh * pr->Hh * pr->Jp,
          launch_joint_argmax_all(heat_all_dev, pr->v2d_max, pr->v2d_idx, N, pr->Hh, pr->Hh, pr->J, pr->Jp, s));
  const int slices = joint_argmax_all_shape(N, pr->Hh, pr->Hh, pr->Jp).slices;
  const int win = 2 * jp.refine_radius + 1;
  // (the partials of every slice; with a radius, win^2 sectors of the heat map per observation; 12 B written)
  JH_PROF("joint_observations", 0.0, 8.0 * N * slices * pr->Jp + (jp.refine_radius ? 32.0 * win * win : 0.0) * N * pr->J +
          12.0 * N * pr->J,
          launch_joint_observations(pr->v2d_max, pr->v2d_idx, heat_all_dev, pr->cur().chm + (size_t)t0 * pr->C * 2,
                                    pr->cur().valid + t0, mask_dev ? mask_dev + (size_t)t0 * pr->C : nullptr, obs_dev,
                                    pr->T3, pr->C, pr->J, pr->Jp, pr->Hh, pr->B / 2, jp.refine_radius, s));
  JH_PROF("joints3d", 0.0, 12.0 * N * pr->J + 24.0 * pr->T3 * pr->J,
          launch_joints3d(obs_dev, pr->calib_at(t0), points_dev, views_dev, members_dev, error_dev, pr->T3, pr->C,
                          pr->J, jp.min_views, jp.min_conf, jp.max_error_px, s));
  return 0;
}

// ---- per-joint camera masks (nets.h: JointSets)
// Everything a joint-masked stage 3 of this predictor needs beyond the caller's mask, ONE allocation made by the first
// call that asks: the gather's sets and counts for a 3D chunk, the effective sets and counts of a time batch, the
// predictor's own mask [T][J][C] and the consensus' other outputs.
static int joint_mask_workspace(jh_predictor* pr, hipStream_t s, const char* what) {
  if (pr->jm_buf) return 0;
  const size_t T = pr->T, T3 = pr->T3, J = pr->J, C = pr->C, Jp = pr->Jp;
  auto pad = [](size_t n) { return (n + 255) / 256 * 256; };
  const size_t b_sets = pad(T3 * C * 8), b_ncam = pad(T3 * Jp * 4), b_cnt = pad(T * J * 4), b_eff = pad(T * J * C);
  const size_t b_pts = pad(T * J * 12), b_tj = pad(T * J * 4);
  char* base = nullptr;
  if (first_call_alloc(pr->mem, s, b_sets + b_ncam + b_cnt + 2 * b_eff + b_pts + 2 * b_tj, what, &base)) return 1;
  pr->jm_sets.sets = reinterpret_cast<unsigned long long*>(base); base += b_sets;
  pr->jm_sets.ncam = reinterpret_cast<int*>(base); base += b_ncam;
  pr->jm_sets.cnt = reinterpret_cast<int*>(base); base += b_cnt;
  pr->jm_sets.eff = reinterpret_cast<unsigned char*>(base); base += b_eff;
  pr->jm_points = reinterpret_cast<float*>(base); base += b_pts;
  pr->jm_error = reinterpret_cast<float*>(base); base += b_tj;
  pr->jm_views = reinterpret_cast<int*>(base); base += b_tj;
  pr->jm_buf = reinterpret_cast<unsigned char*>(base);       // (set last: the workspace is there)
  return 0;
}

extern "C" {

int jh_predictor_set_joint_mask(jh_predictor* pr, int mode, const uint8_t* joint_mask_dev,
                                const jh_joints3d_params* params, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_set_joint_mask: null predictor");
  JH_REQUIRE(mode >= JH_JOINT_MASK_OFF && mode <= JH_JOINT_MASK_CONSENSUS, "jh_predictor_set_joint_mask: mode must be "
             "JH_JOINT_MASK_OFF, JH_JOINT_MASK_GIVEN or JH_JOINT_MASK_CONSENSUS");
  if (mode == JH_JOINT_MASK_OFF) {            // (the buffers stay for the next joint-masked call)
    pr->jm_mode = mode;
    return 0;
  }
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "jh_predictor_set_joint_mask needs all cameras local");
  JH_REQUIRE(pr->C <= 64, "jh_predictor_set_joint_mask: at most 64 cameras");
  JH_REQUIRE(mode != JH_JOINT_MASK_GIVEN || joint_mask_dev, "jh_predictor_set_joint_mask: JH_JOINT_MASK_GIVEN needs "
             "a mask");
  const jh_joints3d_params defaults{2, 1, 0.1f, 8.f};
  Joints3dParams jp;
  if (mode == JH_JOINT_MASK_CONSENSUS && joints3d_params(params ? params : &defaults, &jp)) return 1;
  const char* what = "the first jh_predictor_set_joint_mask call of a predictor allocates its buffers: make it outside "
                     "a stream capture";
  if (joint_mask_workspace(pr, s, what)) return 1;
  if (mode == JH_JOINT_MASK_CONSENSUS) {
    if (triangulate_joints_workspace(pr, s, true, what)) return 1;
    pr->jm_params = jp;
  } else {
    JH_CHECK_HIP(hipMemcpyAsync(pr->jm_buf, joint_mask_dev, (size_t)pr->T * pr->J * pr->C, hipMemcpyDeviceToDevice, s));
  }
  pr->jm_mode = mode;
  return 0;
}

int jh_predictor_get_joint_mask(jh_predictor* pr, uint8_t* cameras_out_dev, int32_t* count_out_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_get_joint_mask: null predictor");
  JH_REQUIRE(pr->jm_buf, "jh_predictor_get_joint_mask: no joint-masked call was made (jh_predictor_set_joint_mask, "
             "jh_predictor_stage_3d_joint_masked)");
  const size_t n = (size_t)pr->T * pr->J;
  if (cameras_out_dev)
    JH_CHECK_HIP(hipMemcpyAsync(cameras_out_dev, pr->jm_sets.eff, n * pr->C, hipMemcpyDeviceToDevice, s));
  if (count_out_dev)
    JH_CHECK_HIP(hipMemcpyAsync(count_out_dev, pr->jm_sets.cnt, n * sizeof(int), hipMemcpyDeviceToDevice, s));
  return 0;
}

int jh_predictor_stage_3d_joint_masked(jh_predictor* pr, const float* heat_all_dev, int t0, const uint8_t* mask_dev,
                                       const uint8_t* joint_mask_dev, float* points_dev, float* conf_dev,
                                       int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && joint_mask_dev, "jh_predictor_stage_3d_joint_masked: null predictor / joint mask");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "joint-masked stage 3 needs all cameras local");
  JH_REQUIRE(pr->C <= 64, "joint-masked stage 3: at most 64 cameras");
  if (joint_mask_workspace(pr, static_cast<hipStream_t>(stream), "the first joint-masked call of a predictor allocates "
                           "its buffers: make it outside a stream capture")) return 1;
  Call call = stage3_call(stream, mask_dev);
  call.joint_mask = joint_mask_dev;
  return stage_3d_impl(pr, call, heat_all_dev, t0, points_dev, conf_dev, valid_dev);
}

// ---- subject identity across frame sets (csrc/tracks.h)
static_assert(sizeof(jh_track_state) == sizeof(TrackState) && sizeof(jh_track_state) == 272, "jh_track_state layout");
static_assert(sizeof(jh_track_params) == 20, "jh_track_params layout");

static int track_params(const jh_track_params* p, TrackParams* out) {
  JH_REQUIRE(p, "null jh_track_params");
  *out = TrackParams{p->max_subjects, p->max_missed, p->predict, p->coast, p->max_jump_mm};
  return tracks_check(*out);
}

int jh_track_params_check(const jh_track_params* params) {
  TrackParams tp;
  return track_params(params, &tp);
}

int jh_op_track_reset(jh_track_state* state_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(state_dev, "jh_op_track_reset: null state");
  JH_PROF("track_reset", 0.0, (double)sizeof(jh_track_state),
          launch_track_reset(reinterpret_cast<TrackState*>(state_dev), s));
  return 0;
}

int jh_op_track_subjects(const float* centers_dev, const int32_t* views_dev, const int32_t* members_dev,
                         const float* error_dev, int t, int cams, const jh_track_params* params,
                         jh_track_state* state_dev, float* centers_out, int32_t* views_out, int32_t* members_out,
                         float* error_out, int32_t* ids_out, int32_t* slots_out, int32_t* missed_out,
                         int32_t* dropped_out, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  TrackParams tp;
  if (track_params(params, &tp)) return 1;
  JH_REQUIRE(centers_dev && state_dev && centers_out && ids_out && slots_out && missed_out && dropped_out,
             "jh_op_track_subjects: null pointer");
  JH_REQUIRE(t >= 1 && cams >= 1, "jh_op_track_subjects: at least one frame set and one camera");
  // (every row read and written once; members are the bulk)
  JH_PROF("track_subjects", 0.0, 8.0 * t * tp.max_subjects * (7.0 + (members_dev ? cams : 0)),
          launch_track_subjects(centers_dev, views_dev, members_dev, error_dev, t, cams, tp,
                                reinterpret_cast<TrackState*>(state_dev), centers_out, views_out, members_out,
                                error_out, ids_out, slots_out, missed_out, dropped_out, s));
  return 0;
}

// ---- several subjects (csrc/subjects.h)
static int subjects_params(const jh_subjects_params* p, SubjectsParams* out) {
  JH_REQUIRE(p, "null jh_subjects_params");
  *out = SubjectsParams{p->max_subjects, p->max_peaks, p->nms_radius, p->min_views, p->min_peak, p->max_error_px};
  return subjects_check(*out);
}

int jh_subjects_params_check(const jh_subjects_params* params) {
  SubjectsParams sp;
  return subjects_params(params, &sp);
}

int jh_op_center_peaks(const float* heat_dev, int n, int hh, int wh, int cp, const jh_subjects_params* params,
                       float* peaks_dev, int32_t* count_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SubjectsParams sp;
  if (subjects_params(params, &sp)) return 1;
  JH_REQUIRE(heat_dev && peaks_dev && count_dev, "jh_op_center_peaks: null pointer");
  JH_REQUIRE(n >= 1 && hh >= 1 && wh >= 1 && hh <= 32768 && wh <= 32768, "jh_op_center_peaks: heat map shape");
  Scratch sc;
  void* ws = nullptr;
  const size_t bytes = center_peaks_workspace(n, hh, wh);
  if (bytes && sc.get(&ws, bytes)) return 1;
  if (launch_center_peaks(heat_dev, peaks_dev, count_dev, n, hh, wh, cp, sp.max_peaks, sp.nms_radius, sp.min_peak, ws,
                          s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_associate_subjects(const float* peaks_dev, int t, int cams, const float* cam_dev, const float* intr_dev,
                             const float* dist_dev, int calib_per_frame, const uint8_t* mask_dev, float sx2, float sy2,
                             const jh_subjects_params* params, float* centers_dev, int32_t* views_dev,
                             int32_t* members_dev, float* error_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SubjectsParams sp;
  if (subjects_params(params, &sp)) return 1;
  JH_REQUIRE(peaks_dev && cam_dev && intr_dev && dist_dev && centers_dev && views_dev && members_dev && error_dev,
             "jh_op_associate_subjects: null pointer");
  JH_REQUIRE(t >= 1 && cams >= 1 && cams <= 64, "jh_op_associate_subjects: at most 64 cameras");
  if (launch_associate_subjects(peaks_dev, Calib{cam_dev, intr_dev, dist_dev, calib_per_frame ? cams : 0}, mask_dev,
                                centers_dev, views_dev, members_dev, error_dev, t, cams, sp.max_peaks, sp.max_subjects,
                                sp.min_views, sp.max_error_px, sx2, sy2, 255.f, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_predictor_detect_subjects(jh_predictor* pr, const void* frames_dev, const void* const* images_host, int n_images,
                                 int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                 const uint8_t* mask_dev, const jh_subjects_params* params, float* centers_dev,
                                 int32_t* views_dev, int32_t* members_dev, float* error_dev, float* peaks_dev,
                                 void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_detect_subjects: null predictor");
  SubjectsParams sp;
  if (subjects_params(params, &sp)) return 1;
  JH_REQUIRE(centers_dev && views_dev && members_dev && error_dev, "jh_predictor_detect_subjects: null output pointer");
  JH_REQUIRE(pr->center, "jh_predictor_detect_subjects: predictor was created without CenterDetect weights");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "jh_predictor_detect_subjects needs all cameras local");
  JH_REQUIRE((frames_dev != nullptr) != (images_host != nullptr),
             "jh_predictor_detect_subjects: give frames_dev or images_host, not both");
  const auto& c = pr->cfg;
  FrameSource fs;
  if (call_source("jh_predictor_detect_subjects", format, yuv, sensor, c.img_h, c.img_w, images_host != nullptr, &fs))
    return 1;
  const int N = pr->T * pr->C;
  const Act& h = pr->center->heat;
  if (!pr->subj_peaks) {
    // (one allocation: subj_peaks is set last, so a failure leaves the predictor as it was)
    const size_t pk = ((size_t)N * kMaxPeaks * 3 * sizeof(float) + 255) / 256 * 256;
    const size_t cn = ((size_t)N * sizeof(int) + 255) / 256 * 256;
    const size_t ws = center_peaks_workspace(N, h.H, h.W);
    char* base = nullptr;
    if (first_call_alloc(pr->mem, s, pk + cn + ws, "the first jh_predictor_detect_subjects call of a predictor "
                         "allocates its workspace: make it outside a stream capture", &base)) return 1;
    pr->subj_count = reinterpret_cast<int*>(base + pk);
    pr->subj_ws = ws ? base + pk + cn : nullptr;
    pr->subj_peaks = reinterpret_cast<float*>(base);
  }
  const void* frames = frames_dev;
  if (images_host) {
    if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, N, fs, s)) return 1;
    frames = pr->frames_table;                // (the launches read the table: `frames` itself is not dereferenced)
  }
  // (plain launches with this call's frame pointer)
  if (center_heat_impl(pr, make_call(frames, fs, stream))) return 1;
  JH_PROF("center_peaks", 0.0, 4.0 * N * h.H * h.W,
          launch_center_peaks(h.p, pr->subj_peaks, pr->subj_count, N, h.H, h.W, h.Cp, sp.max_peaks, sp.nms_radius,
                              sp.min_peak, pr->subj_ws, s));
  const Scale2 k = center_scale2(c);          // (as stage 2 scales the arg-max)
  JH_PROF("associate_subjects", 0.0, 0.0,
          launch_associate_subjects(pr->subj_peaks, pr->calib_at(0), mask_dev, centers_dev, views_dev, members_dev,
                                    error_dev, pr->T, pr->C, sp.max_peaks, sp.max_subjects, sp.min_views,
                                    sp.max_error_px, k.x, k.y, 255.f, s));
  if (peaks_dev)
    JH_CHECK_HIP(hipMemcpyAsync(peaks_dev, pr->subj_peaks, (size_t)N * sp.max_peaks * 3 * sizeof(float),
                                hipMemcpyDeviceToDevice, s));
  return 0;
}

int jh_predictor_debug(jh_predictor* pr, float* center3d_f_dev, int32_t* center3d_i_dev,
                       int32_t* center_hm_dev, float* det_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t T = pr->T, C = pr->C;
  if (center3d_f_dev) JH_CHECK_HIP(hipMemcpyAsync(center3d_f_dev, pr->c3f, T * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (center3d_i_dev) JH_CHECK_HIP(hipMemcpyAsync(center3d_i_dev, pr->cur().c3i, T * 3 * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (center_hm_dev) JH_CHECK_HIP(hipMemcpyAsync(center_hm_dev, pr->cur().chm, T * C * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (det_dev) JH_CHECK_HIP(hipMemcpyAsync(det_dev, pr->det_all, T * C * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}

int jh_predictor_hybridnet_forward(jh_predictor* pr, const float* crops_dev,
                                   const int32_t* center_hm_dev, const int32_t* center3d_dev,
                                   float* heatmap_final_dev, float* heatmaps_padded_dev,
                                   float* points_dev, float* conf_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr->Cloc == pr->C && pr->T3 == pr->T, "hybridnet_forward needs all cameras local");
  JH_CHECK_HIP(hipMemcpyAsync(pr->cur().chm, center_hm_dev, (size_t)pr->T * pr->C * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->cur().c3i, center3d_dev, (size_t)pr->T * 3 * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (launch_to_channel_last(crops_dev, pr->kp->input, s)) return 1;
  pr->kp->stem_src.mode = 0;                      // (the crops are given: the stem reads the plan's input)
  if (pr->kp->run(s)) return 1;
  if (heatmaps_padded_dev) {
    const Act& h = pr->kp->heat;
    const size_t total = (size_t)h.N * pr->J * pr->hs * pr->hs;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(export_padded_kernel, dim3(blocks), dim3(256), 0, s, h.p, heatmaps_padded_dev,
                       h.N, pr->J, h.Cp, pr->Hh);
    JH_CHECK_HIP(hipGetLastError());
  }
  return pr->run_3d(stage3_call(stream), pr->kp->heat.p, 0, heatmap_final_dev, points_dev, conf_dev);
}

// ----------------------------------------------------------------- 2D predictor
}  // extern "C"

struct jh_predictor2d {
  jh_predictor_config cfg{};
  int T = 0, J = 0, B = 0;
  std::unique_ptr<EffTrackPlan> center, kp;
  Scratch mem;
  float* det = nullptr;
  int *chm = nullptr, *valid = nullptr;
  const void** frames_table = nullptr;       // per-image frames: [T] device pointers (jh_predictor2d_forward_images)
};

extern "C" {

int jh_predictor2d_create(const jh_params* center_params, const jh_params* kp_params,
                          const jh_predictor_config* cfg, jh_predictor2d** out) {
  JH_REQUIRE(center_params && kp_params && cfg && out, "bad argument");
  std::unique_ptr<jh_predictor2d> pr(new jh_predictor2d());
  pr->cfg = *cfg;
  pr->T = cfg->time_batch; pr->J = cfg->num_joints; pr->B = cfg->bbox;
  JH_REQUIRE(pr->T >= 1, "batch");
  JH_REQUIRE(cfg->img_w >= pr->B + 1 && cfg->img_h >= pr->B + 1, "image smaller than the bounding box");
  PlanSetup setup;                            // (the plans' own node form and norm blocking: no time-batch class here)
  if (setup.init(&pr->cfg, NodeBatchClass::ByLaunchSize, 0)) return 1;
  pr->center = setup.efftrack();
  if (pr->center->build(center_params->map, "", cfg->center_model, 1, pr->T, cfg->center_size,
                        cfg->center_size)) return 1;
  pr->kp = setup.efftrack();
  if (pr->kp->build(kp_params->map, "", cfg->kp_model, pr->J, pr->T, pr->B, pr->B)) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->det), (size_t)pr->T * 3 * sizeof(float))) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->chm), (size_t)pr->T * 2 * sizeof(int))) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->valid), (size_t)pr->T * sizeof(int))) return 1;
  JH_CHECK_HIP(hipDeviceSynchronize());
  *out = pr.release();
  return 0;
}

void jh_predictor2d_destroy(jh_predictor2d* pr) { delete pr; }

static int forward2d_impl(jh_predictor2d* pr, const Call& call, int32_t* points_dev, float* conf_dev,
                          int32_t* valid_dev) {
  hipStream_t s = call.s;
  const FrameSource& fs = call.fs;
  const auto& c = pr->cfg;
  const int S = c.center_size;
  // algorithmic bytes as in the 3D stages: four taps (resize) or one pixel (crop) of frame data + the float4 written.
  // (These counts used to be a flat 24 B per pixel for every format: fp32 resize is 60, uint8 crop 15.)
  JH_PROF("preprocess_resize", 0.0, (double)pr->T * S * S * (4.0 * fs.px_bytes() + 12.0),
          launch_preprocess_resize(call.frames, fs, pr->center->input.p, pr->T, c.img_h, c.img_w, S,
                                   c.mean, c.std, s, call.cell));
  if (pr->center->run(s)) return 1;
  const Act& h = pr->center->heat;
  JH_PROF("center_argmax", 0.0, 4.0 * pr->T * h.H * h.W,
          launch_center_argmax(h.p, pr->det, pr->T, h.H, h.W, h.Cp, s));
  // img_size / float(IMAGE_SIZE) in fp32 (jarvis2D.py:106-109)
  const float sx = (float)c.img_w / (float)S, sy = (float)c.img_h / (float)S;
  if (launch_center2d(pr->det, pr->chm, pr->valid, pr->T, sx, sy, pr->B / 2, c.img_w, c.img_h, s))
    return 1;
  JH_PROF("preprocess_crop", 0.0, (double)pr->T * pr->B * pr->B * (fs.px_bytes() + 12.0),
          launch_preprocess_crop(call.frames, fs, pr->chm, pr->kp->input.p, pr->T, 1, 1, 0, c.img_h,
                                 c.img_w, pr->B, c.mean, c.std, s, call.cell));
  if (pr->kp->run(s)) return 1;
  const Act& k = pr->kp->heat;
  JH_PROF("joint_argmax", 0.0, 4.0 * pr->T * k.H * k.W * pr->J,
          launch_joint_argmax(k.p, pr->chm, points_dev, conf_dev, pr->T, pr->J, k.Cp, k.H, k.W,
                              pr->B / 2, s));
  if (valid_dev)
    JH_CHECK_HIP(hipMemcpyAsync(valid_dev, pr->valid, (size_t)pr->T * sizeof(int),
                                hipMemcpyDeviceToDevice, s));
  return 0;
}

int jh_predictor2d_forward(jh_predictor2d* pr, const float* frames_dev, int32_t* points_dev,
                           float* conf_dev, int32_t* valid_dev, void* stream) {
  return forward2d_impl(pr, make_call(frames_dev, fixed_source(kSrcRgbF32), stream), points_dev, conf_dev, valid_dev);
}
int jh_predictor2d_forward_u8(jh_predictor2d* pr, const uint8_t* frames_dev, int32_t* points_dev,
                              float* conf_dev, int32_t* valid_dev, void* stream) {
  return forward2d_impl(pr, make_call(frames_dev, fixed_source(kSrcBgrU8), stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_yuv(jh_predictor2d* pr, const uint8_t* frames_dev, int format, int32_t* points_dev,
                               float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(format == JH_FRAME_I420 || format == JH_FRAME_NV12, "jh_predictor2d_forward_yuv: format must be "
             "JH_FRAME_I420 or JH_FRAME_NV12");
  JH_REQUIRE(pr, "bad argument");
  FrameSource fs;
  if (frame_source(format, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward2d_impl(pr, make_call(frames_dev, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_surface(jh_predictor2d* pr, const uint8_t* frames_dev, const jh_yuv_surface* surface,
                                   int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && frames_dev, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward2d_impl(pr, make_call(frames_dev, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_sensor(jh_predictor2d* pr, const uint8_t* frames_dev, const jh_sensor_surface* surface,
                                  int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && frames_dev, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward2d_impl(pr, make_call(frames_dev, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_images(jh_predictor2d* pr, const void* const* images_host, int n_images, int format,
                                  const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                  int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && points_dev && conf_dev, "bad argument");
  FrameSource fs;
  if (call_source("forward_images", format, yuv, sensor, pr->cfg.img_h, pr->cfg.img_w, true, &fs)) return 1;
  if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, pr->T, fs,
                    static_cast<hipStream_t>(stream))) return 1;
  return forward2d_impl(pr, make_call(pr->frames_table, fs, stream), points_dev, conf_dev, valid_dev);
}

// ------------------------------------------------------------------- profiling
int jh_profile_begin(void) {
  Profiler& pf = profiler();
  pf.recs.clear();
  pf.on = true;
  return 0;
}
int jh_profile_end(int* n_records) {
  Profiler& pf = profiler();
  pf.on = false;
  if (pf.finish()) return 1;
  if (n_records) *n_records = (int)pf.recs.size();
  return 0;
}
int jh_profile_get(int i, char* name, int name_cap, double* ms, double* flops, double* bytes) {
  Profiler& pf = profiler();
  JH_REQUIRE(i >= 0 && i < (int)pf.recs.size(), "profile record index");
  const ProfRec& r = pf.recs[i];
  if (name && name_cap > 0) {
    strncpy(name, r.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ms) *ms = r.ms;
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  return 0;
}

// -------------------------------------------------------- single-operator tests
long jh_deconv4_window_launches(void) { return deconv4_window_launches(); }

int jh_conv_form(int nd, int kind, int k, int stride, int pad, int cin, int cout, int has_bias, int want_stats,
                 int gate, int precision, int in_px, char* name, int name_cap) {
  JH_REQUIRE((nd == 2 || nd == 3) && kind >= 0 && kind <= 2 && k >= 1 && stride >= 1 && pad >= 0 && cin >= 1 &&
             cout >= 1 && gate >= 0 && gate <= 2 && precision >= 0 && precision <= 2 && in_px >= 0 && name &&
             name_cap > 0, "jh_conv_form: bad argument");
  ConvUse use;
  use.desc = kind == 0 ? conv_desc(nd, k, stride, pad, cin, cout)
                       : (kind == 1 ? deconv2d_k4s2p1_desc(cin, cout) : deconv3d_k2s2_desc(cin, cout));
  use.transposed = kind != 0; use.has_bias = has_bias != 0; use.want_stats = want_stats != 0;
  use.gate = static_cast<ConvGate>(gate);
  use.precision = precision;
  use.in_px = in_px;
  snprintf(name, (size_t)name_cap, "%s", conv_choice_name(choose_conv(use)).c_str());
  return 0;
}

int jh_node_form(int c, int cout, int n, int h, int w, int n_in, const int* modes, int act, int batch_class,
                 int want_pool, char* name, int name_cap, int32_t* out) {
  JH_REQUIRE(c >= 1 && cout >= 1 && n >= 1 && h >= 1 && w >= 1 && n_in >= 2 && n_in <= 3 && modes && act >= 0 &&
             act <= 2 && batch_class >= 0 && batch_class <= 2 && name && name_cap > 0 && out,
             "jh_node_form: bad argument");
  NodeUse use;
  use.Cp = cpad(c); use.cout_p = cpad(cout); use.cout_p16 = round_up(cout, 16);
  use.N = n; use.H = h; use.W = w; use.n_in = n_in; use.act = act;
  for (int i = 0; i < n_in; ++i) use.mode[i] = modes[i];
  use.cls = static_cast<NodeBatchClass>(batch_class);
  use.want_pool = want_pool != 0;
  NodeChoice ch;
  if (choose_node(use, &ch)) return 1;
  snprintf(name, (size_t)name_cap, "%s", node_choice_name(ch).c_str());
  const int32_t v[8] = {ch.seg_rows, ch.strips, ch.segs, (int32_t)ch.grid.x, (int32_t)ch.grid.y, (int32_t)ch.block.x,
                        (int32_t)ch.lds, ch.pool ? 1 : 0};
  std::copy(v, v + 8, out);
  return 0;
}

// Host (n, c, 2) sums / sums of squares -> [N][Cp][kStatW]: the whole value in the first limb of each (exact_read then
// returns exactly the given double), pad channels zero.
static int op_upload_stats(Scratch& sc, const double* sums_host, int n, int c, int Cp, double** dev) {
  std::vector<double> st((size_t)n * Cp * kStatW, 0.0);
  for (int b = 0; b < n; ++b)
    for (int ch = 0; ch < c; ++ch) {
      st[((size_t)b * Cp + ch) * kStatW] = sums_host[((size_t)b * c + ch) * 2];
      st[((size_t)b * Cp + ch) * kStatW + kLimbs] = sums_host[((size_t)b * c + ch) * 2 + 1];
    }
  return op_upload(sc, st.data(), st.size(), dev);
}

// The squeeze-excite recipe from host values: pooled sums (n, C) -> [N][Cp][kLimbs] (first limb), weights as they are.
static int op_upload_se(Scratch& sc, const double* pool_host, int n, int C, int Cp, int S, float inv_hw,
                        const float* wr, const float* br, const float* we, const float* be, SeGate* out) {
  JH_REQUIRE(pool_host && wr && br && we && be && C >= 1 && C <= Cp && S >= 1, "squeeze-excite recipe");
  std::vector<double> pl((size_t)n * Cp * kLimbs, 0.0);
  for (int b = 0; b < n; ++b)
    for (int ch = 0; ch < C; ++ch) pl[((size_t)b * Cp + ch) * kLimbs] = pool_host[(size_t)b * C + ch];
  double* pool = nullptr;
  float *dwr = nullptr, *dbr = nullptr, *dwe = nullptr, *dbe = nullptr;
  if (op_upload(sc, pl.data(), pl.size(), &pool) || op_upload(sc, wr, (size_t)S * C, &dwr) ||
      op_upload(sc, br, (size_t)S, &dbr) || op_upload(sc, we, (size_t)C * S, &dwe) || op_upload(sc, be, (size_t)C, &dbe))
    return 1;
  out->pool = pool; out->wr = dwr; out->br = dbr; out->we = dwe; out->be = dbe;
  out->C = C; out->S = S; out->inv_hw = inv_hw;
  return 0;
}

// One convolution as a ConvLayer (csrc/conv_layer.h), the way Plan::add_conv runs it (kernel form by choose_conv, at the
// process-wide precision): the body of jh_op_conv (opd == nullptr: operand as it is, optional norm_apply behind the conv)
// and of jh_op_conv_operand (opd: the operand transform of the consumer -- InstanceNorm + activation from host
// statistics, gate tensor or recipe -- raw output).
static int op_conv_body(int nd, int kind, int k, int stride, int pad, int cin, int cout, const float* w_host,
                        const float* b_host, const float* x_dev, int n, int d, int h, int w, const float* gate_dev,
                        int norm_act, const jh_op_operand* opd, float* y_dev, hipStream_t s, const char* who) {
  const bool recipe = opd && opd->se_pool_host;
  const bool want_stats = opd ? opd->want_stats != 0 : norm_act >= 0;
  const bool plain_out = !want_stats && !gate_dev && !recipe;
  const ConvDesc desc = kind == 0 ? conv_desc(nd, k, stride, pad, cin, cout)
                                  : (kind == 1 ? deconv2d_k4s2p1_desc(cin, cout) : deconv3d_k2s2_desc(cin, cout));
  Scratch sc;
  Act x, y;
  if (nd == 2) d = 1;
  if (sc.act(n, d, h, w, cin, &x)) return 1;
  int Do, Ho, Wo;
  conv_out_shape(desc, d, h, w, &Do, &Ho, &Wo);
  if (sc.act(n, Do, Ho, Wo, cout, &y)) return 1;
  // (a plain ConvTranspose2d -- no statistics, no InstanceNorm behind it -- starts from NaN instead: an output element
  //  that no workgroup stores then reaches the caller as NaN; pad channels are not copied out.  The fill exists for the
  //  exactly-once-stores check of tests/test_hip_deconv4_window.py)
  JH_CHECK_HIP(hipMemsetAsync(y.p, kind == 1 && plain_out ? 0xFF : 0, y.bytes(), s));
  ConvUse use;
  use.desc = desc; use.desc.latency_class = opd ? opd->latency_class : 0;
  use.transposed = kind != 0; use.has_bias = b_host != nullptr; use.want_stats = want_stats;
  use.gate = recipe ? ConvGate::Recipe : (gate_dev ? ConvGate::Tensor : ConvGate::None);
  use.precision = precision_mode();
  use.in_px = x.Cp;
  ConvLayer layer;
  if (make_conv_layer(use, w_host, b_host, y.D, y.H, y.W, &layer)) return 1;
  double* stats = nullptr;
  float* gate_p = nullptr;
  if (want_stats) {
    if (sc.get(reinterpret_cast<void**>(&stats), (size_t)n * y.Cp * kStatW * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)n * y.Cp * kStatW * sizeof(double), s));
  }
  if (gate_dev) {   // (N,Cin) -> padded (N,Cin_p)
    if (sc.get(reinterpret_cast<void**>(&gate_p), (size_t)n * x.Cp * sizeof(float))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(gate_p, 0, (size_t)n * x.Cp * sizeof(float), s));
    JH_CHECK_HIP(hipMemcpy2DAsync(gate_p, x.Cp * sizeof(float), gate_dev, cin * sizeof(float), cin * sizeof(float), n,
                                  hipMemcpyDeviceToDevice, s));
  }
  InNorm in;
  SeGate se;
  if (opd && opd->in_sums_host) {
    double* st = nullptr;
    if (op_upload_stats(sc, opd->in_sums_host, n, cin, x.Cp, &st)) return 1;
    in.stats = st; in.inv = 1.f / (float)x.pixels(); in.act = opd->in_act;
  }
  if (recipe) {
    JH_REQUIRE(opd->se_c == cin, "the gate recipe has one gate per input channel");
    if (op_upload_se(sc, opd->se_pool_host, n, opd->se_c, x.Cp, opd->se_s, opd->se_inv_hw, opd->se_wr_host,
                     opd->se_br_host, opd->se_we_host, opd->se_be_host, &se)) return 1;
  }
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (layer.launch(x, y, gate_p, stats, in, recipe ? &se : nullptr, s)) return 1;
  if (!opd && norm_act >= 0 && launch_norm_apply(y, stats, norm_act, nullptr, nullptr, y.p, nullptr, s)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  if (hipStreamSynchronize(s) != hipSuccess) { set_error(std::string("stream sync failed in ") + who); return 1; }
  return 0;
}

int jh_op_conv(int nd, int kind, int k, int stride, int pad, int cin, int cout,
               const float* w_host, const float* b_host, const float* x_dev, int n, int d, int h,
               int w, const float* gate_dev, int norm_act, float* y_dev, void* stream) {
  return op_conv_body(nd, kind, k, stride, pad, cin, cout, w_host, b_host, x_dev, n, d, h, w, gate_dev, norm_act,
                      nullptr, y_dev, static_cast<hipStream_t>(stream), "jh_op_conv");
}

int jh_op_conv_operand(int nd, int kind, int k, int stride, int pad, int cin, int cout,
                       const float* w_host, const float* b_host, const float* x_dev, int n, int d, int h,
                       int w, const float* gate_dev, const jh_op_operand* operand, float* y_dev, void* stream) {
  JH_REQUIRE(operand && w_host && x_dev && y_dev && n >= 1, "bad argument");
  JH_REQUIRE(operand->in_act >= ACT_NONE && operand->in_act <= ACT_SILU, "jh_op_conv_operand: in_act");
  JH_REQUIRE(operand->latency_class == 0 || operand->latency_class == 1, "jh_op_conv_operand: latency_class");
  JH_REQUIRE(!(gate_dev && operand->se_pool_host), "either a gate tensor or a gate recipe");
  return op_conv_body(nd, kind, k, stride, pad, cin, cout, w_host, b_host, x_dev, n, d, h, w, gate_dev, -1, operand,
                      y_dev, static_cast<hipStream_t>(stream), "jh_op_conv_operand");
}

// The squeeze-excite gate kernel on its own: host pooled sums (n, c) and weights -> gate_dev (n, c).
int jh_op_se_gate(const double* pool_host, int n, int c, int squeeze, float inv_hw, const float* wr_host,
                  const float* br_host, const float* we_host, const float* be_host, float* gate_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(gate_dev && n >= 1, "bad argument");
  Scratch sc;
  SeGate se;
  const int Cp = cpad(c);
  if (op_upload_se(sc, pool_host, n, c, Cp, squeeze, inv_hw, wr_host, br_host, we_host, be_host, &se)) return 1;
  float* gate = nullptr;
  if (sc.get(reinterpret_cast<void**>(&gate), (size_t)n * Cp * sizeof(float))) return 1;
  if (launch_se_gate(se.pool, n, c, Cp, squeeze, inv_hw, se.wr, se.br, se.we, se.be, gate, s)) return 1;
  JH_CHECK_HIP(hipMemcpy2DAsync(gate_dev, c * sizeof(float), gate, Cp * sizeof(float), c * sizeof(float), n,
                                hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// norm_apply on its own, in place on x as the plans run it: statistics from the host, residual operands r1 (raw, with
// its own statistics, when r1_sums_host is given) and r2; y_dev (write_y) and / or the pooled sums pool_host (n, c).
int jh_op_norm_apply(const float* x_dev, int n, int c, int d, int h, int w, const double* sums_host, int act,
                     const float* r1_dev, const double* r1_sums_host, const float* r2_dev, int write_y, int want_pool,
                     int min_block_kb, float* y_dev, double* pool_host, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(x_dev && sums_host && n >= 1 && (!write_y || y_dev) && (!want_pool || pool_host), "bad argument");
  Scratch sc;
  Act x, r1, r2;
  if (sc.act(n, d, h, w, c, &x) || launch_to_channel_last(x_dev, x, s)) return 1;
  if (r1_dev && (sc.act(n, d, h, w, c, &r1) || launch_to_channel_last(r1_dev, r1, s))) return 1;
  if (r2_dev && (sc.act(n, d, h, w, c, &r2) || launch_to_channel_last(r2_dev, r2, s))) return 1;
  double *st = nullptr, *st1 = nullptr, *pool = nullptr;
  if (op_upload_stats(sc, sums_host, n, c, x.Cp, &st)) return 1;
  if (r1_sums_host && op_upload_stats(sc, r1_sums_host, n, c, x.Cp, &st1)) return 1;
  const size_t npl = (size_t)n * x.Cp * kLimbs;
  if (want_pool) {
    if (sc.get(reinterpret_cast<void**>(&pool), npl * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(pool, 0, npl * sizeof(double), s));
  }
  if (launch_norm_apply(x, st, act, r1.p, r2.p, write_y ? x.p : nullptr, pool, s, st1, min_block_kb)) return 1;
  if (write_y && launch_from_channel_last(x, y_dev, s)) return 1;
  std::vector<double> hp(want_pool ? npl : 0);
  if (want_pool) JH_CHECK_HIP(hipMemcpyAsync(hp.data(), pool, npl * sizeof(double), hipMemcpyDeviceToHost, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  if (want_pool)
    for (int i = 0; i < n; ++i)
      for (int ch = 0; ch < c; ++ch) {
        const double* q = hp.data() + ((size_t)i * x.Cp + ch) * kLimbs;
        pool_host[(size_t)i * c + ch] = (q[0] + q[1]) + q[2];
      }
  return 0;
}

int jh_op_depthwise(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w,
                    int norm_act, float* y_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  Scratch sc;
  Act x, y;
  if (sc.act(n, 1, h, w, c, &x)) return 1;
  if (sc.act(n, 1, h, w, c, &y)) return 1;
  const std::vector<float> wt = taps_major(w_host, c, k * k, x.Cp);
  float* wd; double* stats = nullptr;
  if (op_upload(sc, wt.data(), wt.size(), &wd)) return 1;
  if (norm_act >= 0) {
    if (sc.get(reinterpret_cast<void**>(&stats), (size_t)n * x.Cp * kStatW * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)n * x.Cp * kStatW * sizeof(double), s));
  }
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (launch_depthwise(x, wd, k, y.p, stats, s)) return 1;
  if (norm_act >= 0 && launch_norm_apply(y, stats, norm_act, nullptr, nullptr, y.p, nullptr, s)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
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

// Depthwise + the squeeze-excite pooled sums of SiLU(InstanceNorm(y)) in one launch (the form MBConv blocks with
// one-tile images use, efficientnet.py:100-107): y_dev (N,C,H,W) raw output, pool_dev (N,C) sums over the pixels.
int jh_op_depthwise_pool(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w,
                         float* y_dev, float* pool_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(depthwise_can_pool(h, w), "jh_op_depthwise_pool: the image must be one 16 x 16 tile");
  Scratch sc;
  Act x, y;
  if (sc.act(n, 1, h, w, c, &x)) return 1;
  if (sc.act(n, 1, h, w, c, &y)) return 1;
  const std::vector<float> wt = taps_major(w_host, c, k * k, x.Cp);
  float* wd; double *stats = nullptr, *pool = nullptr;
  if (op_upload(sc, wt.data(), wt.size(), &wd)) return 1;
  const size_t nst = (size_t)n * x.Cp * kStatW, npl = (size_t)n * x.Cp * kLimbs;
  if (sc.get(reinterpret_cast<void**>(&stats), nst * sizeof(double))) return 1;
  if (sc.get(reinterpret_cast<void**>(&pool), npl * sizeof(double))) return 1;
  JH_CHECK_HIP(hipMemsetAsync(stats, 0, nst * sizeof(double), s));
  JH_CHECK_HIP(hipMemsetAsync(pool, 0, npl * sizeof(double), s));
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (launch_depthwise(x, wd, k, y.p, stats, s, pool)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  std::vector<double> hp(npl);
  JH_CHECK_HIP(hipMemcpyAsync(hp.data(), pool, npl * sizeof(double), hipMemcpyDeviceToHost, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  std::vector<float> out((size_t)n * c);
  for (int i = 0; i < n; ++i)
    for (int ch = 0; ch < c; ++ch) {
      const double* q = hp.data() + ((size_t)i * x.Cp + ch) * kLimbs;
      out[(size_t)i * c + ch] = (float)((q[0] + q[1]) + q[2]);
    }
  JH_CHECK_HIP(hipMemcpy(pool_dev, out.data(), out.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

// The all-joint argmax on its own (csrc/geometry.hip): the (max, index) partials live in the caller's workspace.
static size_t carve_joint_argmax_all(Carver& c, int n, int hh, int wh, int jp, float** pmax, int** pidx) {
  const size_t k = joint_argmax_all_partials(n, hh, wh, jp);
  *pmax = c.take<float>(k);
  *pidx = c.take<int>(k);
  return c.off;
}

int64_t jh_joint_argmax_all_workspace_bytes(int n, int hh, int wh, int jp) {
  if (n < 1 || hh < 1 || wh < 1 || jp < 8 || jp % 8 || jp > 256) return 0;
  Carver c(nullptr, 0);
  float* pmax;
  int* pidx;
  return (int64_t)carve_joint_argmax_all(c, n, hh, wh, jp, &pmax, &pidx);
}

int jh_op_joint_argmax_all(const float* heat_dev, int n, int hh, int wh, int j, int jp, int32_t* idx_dev,
                           float* max_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(heat_dev && idx_dev && max_dev, "null pointer");
  JH_REQUIRE(n >= 1 && hh >= 1 && wh >= 1 && jp >= 8 && jp % 8 == 0 && jp <= 256 && j >= 1 && j <= jp,
             "jh_op_joint_argmax_all: shape");
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_joint_argmax_all_workspace_bytes)");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  float* pmax;
  int* pidx;
  carve_joint_argmax_all(c, n, hh, wh, jp, &pmax, &pidx);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_joint_argmax_all_workspace_bytes()");
  const double bytes = 4.0 * n * hh * wh * jp;
  JH_PROF("joint_argmax_all", 0.0, bytes, launch_joint_argmax_all(heat_dev, pmax, pidx, n, hh, wh, j, jp, s));
  if (launch_joint_argmax_all_combine(pmax, pidx, idx_dev, max_dev, n, hh, wh, j, jp, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}


// One fused BiFPN node (csrc/bifpn_node.hip) as a unit-test entry point: every input is a RAW
// tensor that the node normalises on load with its own InstanceNorm statistics (computed here
// on the host), exactly as inside the network plan.  The body of jh_op_bifpn_node (ex == nullptr: class ByLaunchSize,
// no pooled output, every input with the statistics of its own pixels) and of jh_op_bifpn_node_ex (the time-batch
// class, the pooled output, statistics a producer handed on, the node's emitted statistics).
static int op_node_body(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout, int h,
                        int w, const float* x0_dev, const float* x1_dev, const float* x2_dev, const float* dw_host,
                        const float* pw_host, const float* bias_host, float* y_dev, const jh_op_node_ex* ex,
                        hipStream_t s, const char* who) {
  JH_REQUIRE(n_in >= 2 && n_in <= 3 && modes && weights && y_dev, "bad argument");
  if (ex && ex->pool_written_host) *ex->pool_written_host = 0;
  JH_REQUIRE(n >= 1 && c >= 1 && cout >= 1 && h >= 1 && w >= 1 && x0_dev && x1_dev && (n_in < 3 || x2_dev) && dw_host &&
             pw_host, "bad argument");
  for (int i = 0; i < n_in; ++i) {   // (an up-sampled input of h / 2 rows has no source for output row h - 1 of an odd h)
    const int step = modes[i] == FUSE_UP2 ? 2 : (modes[i] == FUSE_UP4 ? 4 : 1);
    JH_REQUIRE(h % step == 0 && w % step == 0, "an up-sampled input needs a node of whole multiples of its step");
  }
  const float* xs[3] = {x0_dev, x1_dev, x2_dev};
  Scratch sc;
  Act in[3], y;
  NodeArgs a{};
  a.n_in = n_in; a.act = act;
  for (int i = 0; i < n_in; ++i) {
    int hi = h, wi = w;
    if (modes[i] == FUSE_UP2) { hi = h / 2; wi = w / 2; }
    else if (modes[i] == FUSE_UP4) { hi = h / 4; wi = w / 4; }
    else if (modes[i] == FUSE_POOL2) { hi = h * 2; wi = w * 2; }
    if (sc.act(n, 1, hi, wi, c, &in[i])) return 1;
    if (launch_to_channel_last(xs[i], in[i], s)) return 1;
    const size_t px = (size_t)hi * wi;
    if (ex && ex->in_sums_host[i]) {
      // statistics a producer handed on, over ITS pixel count (a pooled tensor carries its producer's: EffTrackPlan::node)
      JH_REQUIRE(ex->in_count[i] >= 1, "pixel count of the given statistics");
      double* st_dev = nullptr;
      if (op_upload_stats(sc, ex->in_sums_host[i], n, c, in[i].Cp, &st_dev)) return 1;
      a.in[i] = in[i].p; a.st[i] = st_dev; a.inv_cnt[i] = 1.f / (float)ex->in_count[i]; a.mode[i] = modes[i];
      a.w[i] = weights[i];
      continue;
    }
    // statistics of the raw input (sum, sum of squares per (n, channel)), whole value in limb 1
    std::vector<float> host((size_t)n * c * px);
    JH_CHECK_HIP(hipMemcpyAsync(host.data(), xs[i], host.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    JH_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<double> st((size_t)n * in[i].Cp * kStatW, 0.0);
    for (int b = 0; b < n; ++b)
      for (int ch = 0; ch < c; ++ch) {
        double s1 = 0.0, s2 = 0.0;
        const float* p = host.data() + ((size_t)b * c + ch) * px;
        for (size_t k = 0; k < px; ++k) { s1 += p[k]; s2 += (double)p[k] * p[k]; }
        st[((size_t)b * in[i].Cp + ch) * kStatW + 1] = s1;
        st[((size_t)b * in[i].Cp + ch) * kStatW + kLimbs + 1] = s2;
      }
    double* std_dev;
    if (sc.get(reinterpret_cast<void**>(&std_dev), st.size() * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemcpyAsync(std_dev, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, s));
    JH_CHECK_HIP(hipStreamSynchronize(s));                       // (st is a local)
    a.in[i] = in[i].p; a.st[i] = std_dev; a.inv_cnt[i] = 1.f / (float)px; a.mode[i] = modes[i];
    a.w[i] = weights[i];
  }
  if (sc.act(n, 1, h, w, cout, &y)) return 1;
  // (NaN: an output pixel that no workgroup stores reaches the caller as NaN, not as a zero that could pass)
  JH_CHECK_HIP(hipMemsetAsync(y.p, 0xFF, y.bytes(), s));
  const int Cp = in[0].Cp;
  const std::vector<float> dwt = taps_major(dw_host, c, 9, Cp);
  float* dwd;
  if (op_upload(sc, dwt.data(), dwt.size(), &dwd)) return 1;
  ConvWeights cw;
  if (pack_conv_weights(conv_desc(2, 1, 1, 0, c, cout), pw_host, bias_host, false, WeightLayout::Plain, &cw)) return 1;
  double* ost;
  const size_t nst = (size_t)n * y.Cp * kStatW;
  std::vector<double> hst(ex && ex->out_sums_host ? nst : 0);
  int rc = 0;
  do {
    if ((rc = sc.get(reinterpret_cast<void**>(&ost), nst * sizeof(double)))) break;
    if (hipMemsetAsync(ost, 0, nst * sizeof(double), s) != hipSuccess) { rc = 1; break; }
    a.dw = dwd; a.pw = cw.w; a.bias = cw.bias; a.y = y.p; a.stats = ost;
    a.N = n; a.H = h; a.W = w; a.Cp = Cp; a.cout_p = y.Cp; a.cout_p16 = cw.cout_p16;
    NodeChoice choice;
    const NodeBatchClass cls = ex ? static_cast<NodeBatchClass>(ex->batch_class) : NodeBatchClass::ByLaunchSize;
    if ((rc = choose_node(node_use(a, cls, ex && ex->want_pool), &choice))) break;
    Act yp;
    if (choice.pool) {   // the pooled output is written exactly when the choice says so, as in EffTrackPlan::node
      if (!ex->y_pool_dev) {
        set_error(std::string(who) + ": the node writes its pooled output, y_pool_dev is NULL");
        rc = 1;
        break;
      }
      if ((rc = sc.act(n, 1, h / 2, w / 2, cout, &yp))) break;
      if (hipMemsetAsync(yp.p, 0xFF, yp.bytes(), s) != hipSuccess) { rc = 1; break; }
      a.y_pool = yp.p;
    }
    if ((rc = launch_bifpn_node(a, choice, s))) break;
    if ((rc = launch_from_channel_last(y, y_dev, s))) break;
    if (choice.pool && (rc = launch_from_channel_last(yp, ex->y_pool_dev, s))) break;
    if (!hst.empty() &&
        hipMemcpyAsync(hst.data(), ost, nst * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) { rc = 1; break; }
    if (hipStreamSynchronize(s) != hipSuccess) { set_error(std::string("stream sync failed in ") + who); rc = 1; break; }
    if (ex && ex->pool_written_host) *ex->pool_written_host = choice.pool ? 1 : 0;
    // the emitted statistics as a consumer reads them: the limbs added in exact_read's order
    for (int b = 0; b < n && !hst.empty(); ++b)
      for (int ch = 0; ch < cout; ++ch) {
        const double* q = hst.data() + ((size_t)b * y.Cp + ch) * kStatW;
        ex->out_sums_host[((size_t)b * cout + ch) * 2] = (q[0] + q[1]) + q[2];
        ex->out_sums_host[((size_t)b * cout + ch) * 2 + 1] = (q[kLimbs] + q[kLimbs + 1]) + q[kLimbs + 2];
      }
  } while (0);
  free_conv_weights(&cw);
  return rc;
}

int jh_op_bifpn_node(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout,
                     int h, int w, const float* x0_dev, const float* x1_dev, const float* x2_dev,
                     const float* dw_host, const float* pw_host, const float* bias_host, float* y_dev,
                     void* stream) {
  return op_node_body(n_in, modes, weights, act, n, c, cout, h, w, x0_dev, x1_dev, x2_dev, dw_host, pw_host, bias_host,
                      y_dev, nullptr, static_cast<hipStream_t>(stream), "jh_op_bifpn_node");
}

int jh_op_bifpn_node_ex(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout,
                        int h, int w, const float* x0_dev, const float* x1_dev, const float* x2_dev,
                        const float* dw_host, const float* pw_host, const float* bias_host, float* y_dev,
                        const jh_op_node_ex* ex, void* stream) {
  JH_REQUIRE(ex && ex->batch_class >= 0 && ex->batch_class <= 2, "jh_op_bifpn_node_ex: batch_class");
  return op_node_body(n_in, modes, weights, act, n, c, cout, h, w, x0_dev, x1_dev, x2_dev, dw_host, pw_host, bias_host,
                      y_dev, ex, static_cast<hipStream_t>(stream), "jh_op_bifpn_node_ex");
}

}  // extern "C"
