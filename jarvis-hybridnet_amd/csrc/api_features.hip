// C ABI, what a 3D predictor does only when asked: per-frame calibration, caller-supplied centres, the per-joint spread,
// the 2D views, per-joint triangulation, per-joint camera masks, the tracker operators and several subjects.  Each
// feature's memory is a workspace its first call carves (predictor.h: first_call_carve): a predictor that never asks
// owns what jh_predictor_create gave it.
#include "predictor.h"
#include "center_keys.h"
#include "views2d.h"
#include "subjects.h"
#include "tracks.h"

using namespace jh;

// The (max, index) partials of the all-joint argmax for the T3 * C heat maps of a 3D chunk, shared by
// jh_predictor_views2d and jh_predictor_triangulate_joints: allocated by whichever is called first (`what`: its message
// for a call inside a stream capture).
static int scan_workspace(jh_predictor* pr, hipStream_t s, const char* what) {
  if (pr->v2d_max) return 0;
  const size_t n = joint_argmax_all_partials(pr->T3 * pr->C, pr->Hh, pr->Hh, pr->Jp);
  struct Ws { float* max; int* idx; } w;
  if (first_call_carve(pr->mem, s, what, &w, [&](Carver& c, Ws& p) {
        p.max = c.take<float>(n);
        p.idx = c.take<int>(n);
      })) return 1;
  pr->v2d_max = w.max; pr->v2d_idx = w.idx;
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

// No heat maps given: the predictor's own from frame t0 on, which hold all cameras only when all cameras are local.
// (After a forward whose head ran with its box they are completed first -- jh_predictor::full_heat, on the reader's stream,
// which is the forward's by this entry's contract.)
static int own_heat_maps(jh_predictor* pr, int t0, const float** heat_all_dev, hipStream_t s) {
  if (*heat_all_dev) return 0;
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "the predictor's own heat maps hold all cameras only when "
             "all cameras are local");
  if (pr->full_heat(s)) return 1;
  *heat_all_dev = pr->kp->heat.p + (size_t)t0 * pr->C * pr->Hh * pr->Hh * pr->Jp;
  return 0;
}

// The scan of a 3D chunk's heat maps into the partials of scan_workspace.
static int launch_scan(jh_predictor* pr, const float* heat_all_dev, hipStream_t s) {
  const int N = pr->T3 * pr->C;
  JH_PROF("joint_argmax_all", 0.0, 4.0 * N * pr->Hh * pr->Hh * pr->Jp,
          launch_joint_argmax_all(heat_all_dev, pr->v2d_max, pr->v2d_idx, N, pr->Hh, pr->Hh, pr->J, pr->Jp, s));
  return 0;
}

int jh::triangulate_joints_launches(jh_predictor* pr, const float* heat_all_dev, int t0, const unsigned char* mask_dev,
                                    const Joints3dParams& jp, float* points_dev, int* views_dev,
                                    unsigned char* members_dev, float* error_dev, float* obs_dev, hipStream_t s) {
  const int N = pr->T3 * pr->C;
  if (launch_scan(pr, heat_all_dev, s)) return 1;
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
// consensus' other outputs and the predictor's own mask [T][J][C].
static int joint_mask_workspace(jh_predictor* pr, hipStream_t s, const char* what) {
  if (pr->jm_buf) return 0;
  const size_t T3 = pr->T3, C = pr->C, TJ = (size_t)pr->T * pr->J;
  struct Ws { JointSets sets; float *points, *error; int* views; unsigned char* buf; } w;
  if (first_call_carve(pr->mem, s, what, &w, [&](Carver& c, Ws& p) {
        p.sets.sets = c.take<unsigned long long>(T3 * C);
        p.sets.ncam = c.take<int>(T3 * pr->Jp);
        p.sets.cnt = c.take<int>(TJ);
        p.sets.eff = c.take<unsigned char>(TJ * C);
        p.points = c.take<float>(TJ * 3);
        p.error = c.take<float>(TJ);
        p.views = c.take<int>(TJ);
        p.buf = c.take<unsigned char>(TJ * C);
      })) return 1;
  pr->jm_sets = w.sets;
  pr->jm_points = w.points; pr->jm_error = w.error; pr->jm_views = w.views;
  pr->jm_buf = w.buf;
  return 0;
}

extern "C" {

// ---- per-frame calibration
int jh_predictor_set_calibration_frames(jh_predictor* pr, const float* cam_dev, const float* intr_dev,
                                        const float* dist_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_set_calibration_frames: null predictor");
  JH_REQUIRE(cam_dev && intr_dev && dist_dev, "jh_predictor_set_calibration_frames: null calibration pointer");
  const size_t rows = (size_t)pr->T * pr->C;
  if (!pr->cam_f) {
    struct Ws { float *cam, *intr, *dist; } w;
    if (first_call_carve(pr->mem, s, "the first jh_predictor_set_calibration_frames call of a predictor allocates its "
                         "per-frame calibration: make it outside a stream capture", &w, [&](Carver& c, Ws& p) {
          p.cam = c.take<float>(rows * 12);
          p.intr = c.take<float>(rows * 9);
          p.dist = c.take<float>(rows * 5);
        })) return 1;
    pr->cam_f = w.cam; pr->intr_f = w.intr; pr->dist_f = w.dist;
  }
  JH_CHECK_HIP(hipMemcpyAsync(pr->cam_f, cam_dev, rows * 12 * sizeof(float), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->intr_f, intr_dev, rows * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipMemcpyAsync(pr->dist_f, dist_dev, rows * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
  pr->calib_fs = pr->C;
  return 0;
}

// ---- caller-supplied centres
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

// ---- centre keyframes (csrc/center_keys.h)
int jh_center_keyframe_rows(int time_batch, int every, int n_rows, int32_t* rows, int cap) {
  int count = 0;
  return center_key_rows(time_batch, every, n_rows, rows, cap, &count) ? -1 : count;
}

int jh_predictor_set_center_keyframes(jh_predictor* pr, const jh_params* center_params, int every, int n_rows,
                                      void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_set_center_keyframes: null predictor");
  JH_REQUIRE(every >= 0, "jh_predictor_set_center_keyframes: every must be 0 (off) or at least 1");
  jh_predictor::CenterKeys& ck = pr->ck;
  if (every == 0) {                           // (back to detection on every row; the plan and the buffers stay)
    ck.every = 0;
    return 0;
  }
  JH_REQUIRE(pr->center, "jh_predictor_set_center_keyframes: predictor was created without CenterDetect weights");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "jh_predictor_set_center_keyframes needs all cameras local");
  JH_REQUIRE(n_rows >= 1 && n_rows <= pr->T, "jh_predictor_set_center_keyframes: n_rows must be 1 .. time_batch");
  const int K = center_key_slots(pr->T, every);
  const char* what = "a jh_predictor_set_center_keyframes call that builds the key plan allocates: make it outside a "
                     "stream capture";
  if (!ck.plan || ck.K != K) {
    JH_REQUIRE(center_params, "jh_predictor_set_center_keyframes: the key plan has to be built, which needs "
               "center_params");
    if (outside_capture(s, what)) return 1;
    // (in the PREDICTOR's time-batch class, as a predictor built for a camera subset is: node forms and the blocking of
    // the InstanceNorm passes follow T, not K)
    std::unique_ptr<EffTrackPlan> plan = pr->setup.efftrack();
    if (plan->build(center_params->map, "", pr->cfg.center_model, 1, K * pr->C, pr->cfg.center_size,
                    pr->cfg.center_size)) return 1;
    JH_CHECK_HIP(hipDeviceSynchronize());     // (the uploads are done; a plan this one replaces is no longer read)
    ck.plan = std::move(plan);
    ck.K = K;
  }
  if (!ck.table) {
    const size_t T = pr->T, C = pr->C;
    struct Ws { const void** table; float *det, *centers; int* source; } w;
    CarveSizes size;
    if (first_call_carve(pr->mem, s, what, &w, [&](Carver& c, Ws& p) {
          p.table = c.take<const void*>(T * C);
          p.det = c.take<float>(T * C * 3);
          p.centers = c.take<float>(T * 3);
          p.source = c.take<int>(T);
        }, &size)) return 1;
    ck.table = w.table; ck.det = w.det; ck.centers = w.centers; ck.source = w.source;
    ck.bytes = size.payload;
  }
  ck.every = every; ck.n_rows = n_rows;
  return 0;
}

int jh_predictor_get_center_keyframes(jh_predictor* pr, float* centers_dev, int32_t* source_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_get_center_keyframes: null predictor");
  JH_REQUIRE(pr->ck.centers, "jh_predictor_get_center_keyframes: centre keyframes were never enabled "
             "(jh_predictor_set_center_keyframes)");
  return copy_if(centers_dev, pr->ck.centers, (size_t)pr->T * 3 * sizeof(float), s) ||
         copy_if(source_dev, pr->ck.source, (size_t)pr->T * sizeof(int), s);
}

// ---- tone tables
int jh_predictor_set_tone(jh_predictor* pr, const float* tables_dev, void* stream) {
  JH_REQUIRE(pr, "jh_predictor_set_tone: null predictor");
  return pr->tone.set(pr->mem, tables_dev, pr->C, static_cast<hipStream_t>(stream));
}

// ---- per-joint 3D spread
int jh_predictor_set_spread(jh_predictor* pr, int on) {
  JH_REQUIRE(pr, "jh_predictor_set_spread: null predictor");
  if (on && !pr->sp_cov) {
    // (allocates and clears: not inside a stream capture -- the call has no stream to ask, the allocation itself
    // fails there)
    const size_t TJ = (size_t)pr->T * pr->J;
    struct Ws { SoftargmaxSpread acc; float *cov, *peak, *mass; } w;
    CarveSizes size;
    if (first_call_carve(pr->mem, nullptr, /*what=*/nullptr, &w, [&](Carver& c, Ws& p) {
          carve_spread(c, pr->T3, pr->Jp, &p.acc);
          p.cov = c.take<float>(TJ * 6);
          p.peak = c.take<float>(TJ * 3);
          p.mass = c.take<float>(TJ);
        }, &size)) return 1;
    JH_CHECK_HIP(hipMemset(w.acc.sums, 0, size.bytes));
    pr->spread.sums = w.acc.sums; pr->spread.key = w.acc.key;
    pr->sp_cov = w.cov; pr->sp_peak = w.peak; pr->sp_mass = w.mass;
    pr->spread_bytes = size.payload;          // (what jh_predictor_device_bytes reports: the pieces, not their padding)
  }
  pr->spread_on = on != 0;
  return 0;
}

int jh_predictor_get_spread(jh_predictor* pr, float* cov_dev, float* peak_dev, float* mass_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "jh_predictor_get_spread: null predictor");
  JH_REQUIRE(pr->sp_cov, "jh_predictor_get_spread: the spread was never enabled (jh_predictor_set_spread)");
  const size_t n = (size_t)pr->T * pr->J * sizeof(float);
  return copy_if(cov_dev, pr->sp_cov, n * 6, s) || copy_if(peak_dev, pr->sp_peak, n * 3, s) ||
         copy_if(mass_dev, pr->sp_mass, n, s);
}

// ---- per-camera 2D views (csrc/views2d.h)
int jh_predictor_views2d(jh_predictor* pr, const float* heat_all_dev, int t0, const float* points_dev,
                         const uint8_t* mask_dev, int32_t* points2d_dev, float* conf2d_dev, float* reproj_dev,
                         float* err_dev, uint8_t* used_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr && points_dev && points2d_dev && conf2d_dev && reproj_dev && err_dev && used_dev,
             "null pointer");
  JH_REQUIRE(t0 >= 0 && t0 + pr->T3 <= pr->T, "frame range of the 2D views");
  const int N = pr->T3 * pr->C;
  if (own_heat_maps(pr, t0, &heat_all_dev, s)) return 1;
  if (scan_workspace(pr, s, "the first jh_predictor_views2d call of a predictor allocates its workspace: make it "
                     "outside a stream capture")) return 1;
  if (launch_scan(pr, heat_all_dev, s)) return 1;
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
  if (own_heat_maps(pr, t0, &heat_all_dev, s)) return 1;
  // (the observations go straight into the caller's buffer when there is one; the predictor's own, allocated by the
  // first call that brings none, otherwise)
  if (triangulate_joints_workspace(pr, s, !obs_dev, "the first jh_predictor_triangulate_joints call of a predictor "
                                   "allocates its workspace: make it outside a stream capture")) return 1;
  return triangulate_joints_launches(pr, heat_all_dev, t0, mask_dev, jp, points_dev, views_dev, members_dev, error_dev,
                                     obs_dev ? obs_dev : pr->j3_obs, s);
}

// ---- per-joint camera masks
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
  return copy_if(cameras_out_dev, pr->jm_sets.eff, n * pr->C, s) ||
         copy_if(count_out_dev, pr->jm_sets.cnt, n * sizeof(int), s);
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

// jh_predictor_detect_subjects and jh_predictor_detect_subjects_pixels: the frames' description is (format, yuv,
// sensor) or `pixels` (call_source)
static int detect_subjects_impl(jh_predictor* pr, const void* frames_dev, const void* const* images_host, int n_images,
                                int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                const jh_pixel_surface* pixels, const uint8_t* mask_dev,
                                const jh_subjects_params* params, float* centers_dev, int32_t* views_dev,
                                int32_t* members_dev, float* error_dev, float* peaks_dev, void* stream) {
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
  if (call_source("jh_predictor_detect_subjects", format, yuv, sensor, pixels, c.img_h, c.img_w,
                  images_host != nullptr, &fs)) return 1;
  {   // (fp32 frames under tone tables are refused before anything is allocated or enqueued)
    Call probe = make_call(frames_dev, fs, stream);
    if (pr->tone_call(&probe)) return 1;
  }
  const int N = pr->T * pr->C;
  const Act& h = pr->center->heat;
  if (!pr->subj_peaks) {
    const size_t ws = center_peaks_workspace(N, h.H, h.W);
    struct Ws { float* peaks; int* count; char* ws; } w;
    if (first_call_carve(pr->mem, s, "the first jh_predictor_detect_subjects call of a predictor allocates its "
                         "workspace: make it outside a stream capture", &w, [&](Carver& k, Ws& p) {
          p.peaks = k.take<float>((size_t)N * kMaxPeaks * 3);
          p.count = k.take<int>((size_t)N);
          p.ws = k.take<char>(ws);
        })) return 1;
    pr->subj_peaks = w.peaks; pr->subj_count = w.count;
    pr->subj_ws = ws ? w.ws : nullptr;
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

int jh_predictor_detect_subjects(jh_predictor* pr, const void* frames_dev, const void* const* images_host, int n_images,
                                 int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                 const uint8_t* mask_dev, const jh_subjects_params* params, float* centers_dev,
                                 int32_t* views_dev, int32_t* members_dev, float* error_dev, float* peaks_dev,
                                 void* stream) {
  return detect_subjects_impl(pr, frames_dev, images_host, n_images, format, yuv, sensor, nullptr, mask_dev, params,
                              centers_dev, views_dev, members_dev, error_dev, peaks_dev, stream);
}

int jh_predictor_detect_subjects_pixels(jh_predictor* pr, const uint8_t* frames_dev, const void* const* images_host,
                                        int n_images, const jh_pixel_surface* surface, const uint8_t* mask_dev,
                                        const jh_subjects_params* params, float* centers_dev, int32_t* views_dev,
                                        int32_t* members_dev, float* error_dev, float* peaks_dev, void* stream) {
  JH_REQUIRE(surface, "jh_predictor_detect_subjects_pixels: null jh_pixel_surface");
  return detect_subjects_impl(pr, frames_dev, images_host, n_images, kSrcPixels, nullptr, nullptr, surface, mask_dev,
                              params, centers_dev, views_dev, members_dev, error_dev, peaks_dev, stream);
}

}  // extern "C"
