// C ABI of libjarvis_hip.so (declarations + reference citations: include/jarvis_hip.h): the error text, ABI version,
// precision and parameters, the stand-alone networks, the geometry operators and the profiler.  The frame descriptions
// are api_frames.hip, the predictors api_predictor.hip / api_features.hip / api_predictor2d.hip, the test-only
// operators api_ops.hip; predictor.h is what they share.
#include <cstring>
#include "predictor.h"
#include "centers.h"
#include "reproject.h"
#include "softargmax.h"

namespace jh {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace jh

using namespace jh;

struct jh_efftrack { EffTrackPlan plan; };
struct jh_v2v { V2VPlan plan; };

namespace {

// Caller-provided workspace, carved into 256-byte aligned pieces (workspace.h): an activation as one piece
void carve_act(Carver& c, int N, int D, int H, int W, int C, Act* a) {
  a->N = N; a->D = D; a->H = H; a->W = W; a->C = C; a->Cp = cpad(C);
  a->p = c.take<float>(a->elems());
}

struct ReproWs { Act heat, vol; float2* coarse; };
static size_t carve_reproject(Carver& c, int cams, int joints, int hs, int g, ReproWs* w) {
  const int gh = g / 2;
  carve_act(c, cams, 1, hs, hs, joints, &w->heat);
  carve_act(c, 1, g, g, g, joints, &w->vol);
  w->coarse = c.take<float2>((size_t)cams * gh * gh * gh);
  return c.off;
}
// (the plain operator's pieces first, then the gather's channel sets and counts)
static size_t carve_reproject_joint(Carver& c, int cams, int joints, int hs, int g, ReproWs* w, JointSets* js) {
  carve_reproject(c, cams, joints, hs, g, w);
  js->sets = c.take<unsigned long long>((size_t)cams);
  js->ncam = c.take<int>((size_t)cpad(joints));
  return c.off;
}
struct SoftWs { Act x; double* partial; int* pmax; };
static size_t carve_softargmax(Carver& c, int t, int joints, int gh, SoftWs* w) {
  carve_act(c, t, gh, gh, gh, joints, &w->x);
  w->partial = c.take<double>((size_t)t * w->x.Cp * 4 * kLimbs);
  w->pmax = c.take<int>((size_t)t * w->x.Cp);
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

}  // extern "C"
