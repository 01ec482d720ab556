// C ABI, the 3D predictor: creation, the three stages, the whole-path forward (plain launches or one graph launch) and
// the debug entries.  What a predictor owns is predictor.h; the optional features are api_features.hip.
#include "predictor.h"
#include "center_keys.h"
#include "centers.h"
#include "preprocess.h"
#include "reproject.h"
#include "softargmax.h"

using namespace jh;

namespace {

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

}  // namespace

// 3D stage for frames t0 .. t0+T3-1 of the batch (heat_all holds those frames)
int jh_predictor::run_3d(const Call& call, const float* heat_all, int t0, float* heatmap_final, float* points,
                         float* conf, const HeatLayout* layout) {
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
                                          call.joint_mask + (size_t)t0 * J * C, js, s, layout, call.head_roi));
  } else {
    JH_PROF(call.mask ? "reproject_gather_masked" : "reproject_gather", 0.0,
            4.0 * T3 * ((double)C * Hh * Hh * J + g3 * J),
            launch_reproject(calib_at(t0), cur().c3i + t0 * 3, cur().chm + t0 * C * 2, heat_all, coarse, v2v->input.p,
                             nullptr, T3, C, G, cfg.grid_spacing, hs, Jp, /*heat_pad=*/0, /*div255=*/1,
                             call.mask ? call.mask + (size_t)t0 * C : nullptr, s, layout, call.head_roi));
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

// Stage 1 up to the heat map of a CenterDetect plan (plan->heat) for the N images of `call`: resize or fused stem, then
// the plan
static int center_heat_plan(jh_predictor* pr, EffTrackPlan* plan, int N, const Call& call) {
  hipStream_t s = call.s;
  const FrameSource& fs = call.fs;
  const int S = pr->cfg.center_size;
  if (plan->stem_fusable) {
    // resize + normalise happen inside the stem convolution's patch staging (csrc/stem.hip)
    StemSource& src = plan->stem_src;
    src.mode = 1; src.frames = call.frames; src.frames_cell = call.cell; src.source = fs;
    src.H = pr->cfg.img_h; src.W = pr->cfg.img_w;
    for (int i = 0; i < 3; ++i) { src.mean[i] = pr->cfg.mean[i]; src.stdv[i] = pr->cfg.std[i]; }
    // algorithmic bytes of the fused launch: the four bilinear taps of every network-input pixel (px_bytes
    // each) + the stem's output at half resolution (16 or 32 channels = 16 or 32 B per input pixel)
    plan->set_stem_traffic((double)N * S * S * (4.0 * fs.px_bytes() + plan->stem_channels()));
  } else {
    JH_PROF("preprocess_resize", 0.0, (double)N * S * S * (4.0 * fs.px_bytes() + 3 * 4),
            launch_preprocess_resize(call.frames, fs, plan->input.p, N, pr->cfg.img_h,
                                     pr->cfg.img_w, S, pr->cfg.mean, pr->cfg.std, s, call.cell));
  }
  return plan->run(s);
}

// ... of the predictor's own plan (pr->center->heat), all T * Cloc images
int jh::center_heat_impl(jh_predictor* pr, const Call& call_in) {
  Call call = call_in;
  if (pr->tone_call(&call)) return 1;
  JH_REQUIRE(pr->center, "predictor was created without CenterDetect weights");
  return center_heat_plan(pr, pr->center.get(), pr->T * pr->Cloc, call);
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

// Stage 1 on the key rows alone (jh_predictor_set_center_keyframes): the key rows' image pointers into the predictor's
// table, the key plan on them through the per-image fetch (image n = (key slot, camera): its tone camera is n % C), the
// arg-max, and the K * C detections into their rows of det_all, zeros elsewhere.
static int stage_center_keys_impl(jh_predictor* pr, const Call& call_in) {
  Call call = call_in;
  if (pr->tone_call(&call)) return 1;
  hipStream_t s = call.s;
  jh_predictor::CenterKeys& ck = pr->ck;
  const FrameSource& fs = call.fs;
  const void* const* src_table = fs.per_image ? call.cell : nullptr;
  JH_REQUIRE(fs.per_image || !call.cell, "a centre-keyframe call is not recorded into the predictor's graphs");
  JH_PROF("center_key_table", 0.0, 16.0 * ck.K * pr->C,
          launch_center_key_table(ck.table, ck.K, pr->C, ck.every, ck.n_rows, call.frames,
                                  fs.per_image ? 0 : image_bytes(fs, pr->cfg.img_h, pr->cfg.img_w), src_table, s));
  Call keys = call;
  keys.fs.per_image = true;
  keys.frames = ck.table;
  keys.cell = ck.table;
  const int N = ck.K * pr->C;
  if (center_heat_plan(pr, ck.plan.get(), N, keys)) return 1;
  const Act& h = ck.plan->heat;
  JH_PROF("center_argmax", 0.0, 4.0 * N * h.H * h.W, launch_center_argmax(h.p, ck.det, N, h.H, h.W, h.Cp, s));
  JH_PROF("center_key_scatter", 0.0, 4.0 * 3 * (N + pr->T * pr->C),
          launch_center_key_scatter(ck.det, pr->det_all, pr->T, pr->C, ck.every, ck.n_rows, s));
  return 0;
}

static int stage_keypoints_impl(jh_predictor* pr, const Call& call_in, const float* det_all_dev, float* heat_dev,
                                int det_blocks = 1, bool next_centre_set = false) {
  Call call = call_in;
  if (pr->tone_call(&call)) return 1;
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
    if (call.center_keys) {
      // the key rows have their float centre and validity with the arithmetic of a detected call; the fill gives every
      // row its centre, and from there on the batch is the centred one
      JH_PROF("center_key_fill", 0.0, 32.0 * pr->T,
              launch_center_key_fill(pr->c3f, cs.valid, pr->ck.centers, pr->ck.source, pr->T, pr->ck.every,
                                     pr->ck.n_rows, s));
      JH_PROF("centers", 0.0, 0.0,
              launch_centers(pr->ck.centers, pr->calib_at(0), pr->c3f, cs.c3i, cs.chm, cs.valid, pr->T, pr->C, pr->B / 2,
                             c.img_w, c.img_h, call.mask, pr->n_active, pr->n_detect, s));
    }
  }
  if (det_all_dev != pr->det_all)
    JH_CHECK_HIP(hipMemcpyAsync(pr->det_all, det_all_dev, (size_t)pr->T * pr->C * 3 * sizeof(float),
                                hipMemcpyDeviceToDevice, s));
  // The head's box.  The coarse (u, v) field of the voxel gather depends on the calibration and the
  // centres alone, both known here: it is projected now instead of in stage 3 (run_3d takes it as it is), and the box
  // of every image -- the heat-map pixels the gather can read -- is taken from it for the keypoint head.
  JH_REQUIRE(!call.head_roi || (pr->kp->head_takes_box && pr->T3 == pr->T && pr->Cloc == pr->C && c.cam_lo == 0),
             "a call whose head takes a box: all frames and cameras in one 3D chunk");
  if (call.head_roi) {
    JH_PROF("reproject_coarse", 0.0, 8.0 * pr->T * pr->C * pr->Gh * pr->Gh * pr->Gh,
            launch_repro_coarse(pr->calib_at(0), cs.c3i, cs.chm, pr->coarse, pr->T, pr->C, pr->G, c.grid_spacing,
                                pr->hs, s));
    JH_PROF("reproject_box", 0.0, 8.0 * pr->T * pr->C * pr->Gh * pr->Gh * pr->Gh,
            launch_repro_box(pr->coarse, cs.valid, call.mask, pr->head_box, pr->T, pr->C, c.cam_lo, pr->Cloc, pr->G,
                             pr->hs, /*heat_pad=*/0, s));
  }
  pr->kp->head_box = call.head_roi ? pr->head_box : nullptr;
  pr->heat_boxed = call.head_roi;
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

int jh::stage_3d_impl(jh_predictor* pr, const Call& call, const float* heat_all_dev, int t0, float* points_dev,
                      float* conf_dev, int32_t* valid_dev, const HeatLayout* layout) {
  JH_REQUIRE(t0 >= 0 && t0 + pr->T3 <= pr->T, "frame range of the 3D stage");
  if (pr->run_3d(call, heat_all_dev, t0, nullptr, points_dev, conf_dev, layout)) return 1;
  if (valid_dev)
    JH_CHECK_HIP(hipMemcpyAsync(valid_dev, pr->cur().valid + t0, (size_t)pr->T3 * sizeof(int),
                                hipMemcpyDeviceToDevice, call.s));
  return 0;
}

static int forward_eager(jh_predictor* pr, const Call& call, float* points_dev, float* conf_dev, int32_t* valid_dev) {
  // (centres supplied by the caller: stage 1 does not run at all; centre keyframes: on the key rows)
  if (call.center_keys) {
    if (stage_center_keys_impl(pr, call)) return 1;
  } else if (!pr->centers_on && stage_center_impl(pr, call, pr->det_all)) {
    return 1;
  }
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
    ++pr->graph_records;
  }
  // (per-image: the recording reads frames_table, which this call's pointers have already been sent into)
  if (!fs.per_image) hipLaunchKernelGGL(set_cell_kernel, dim3(1), dim3(1), 0, s, pr->frames_cell, call.frames);
  JH_CHECK_HIP(hipGetLastError());
  JH_CHECK_HIP(hipGraphLaunch(slot.exec, s));
  const int n_pts = pr->T * pr->J * 3;
  hipLaunchKernelGGL(copy_out_kernel, dim3((n_pts + 255) / 256), dim3(256), 0, s, pr->g_points, pr->g_conf,
                     pr->cset[0].valid, points_dev, conf_dev, valid_dev, n_pts, pr->T * pr->J, pr->T);
  JH_CHECK_HIP(hipGetLastError());
  // (what stage 2 notes when it is called; a replay calls nothing.  Every call of a slot has the same head_roi: it
  //  depends on the plan and on modes that never come here.)
  pr->kp->head_box = call.head_roi ? pr->head_box : nullptr;
  pr->heat_boxed = call.head_roi;
  return 0;
}

// mask_dev != nullptr: the masked kernels, reading the predictor's copy of the mask (made here, on the caller's
// stream, outside any graph of the predictor's own: the captured launches keep pointing at mask_buf)
static int forward_impl(jh_predictor* pr, const void* frames_dev, const FrameSource& fs, float* points_dev,
                        float* conf_dev, int32_t* valid_dev, void* stream,
                        const unsigned char* mask_dev = nullptr) {
  Call call = make_call(frames_dev, fs, stream, mask_dev ? pr->mask_buf : nullptr);
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "forward needs all cameras local");
  JH_REQUIRE(pr->T3 == pr->T, "forward needs time_batch_3d == time_batch");
  JH_REQUIRE(frames_dev && points_dev && conf_dev, "null frame / output pointer");
  JH_REQUIRE(!(pr->centers_on && pr->ck.every), "caller-supplied centres (jh_predictor_set_centers) and centre "
             "keyframes (jh_predictor_set_center_keyframes) are both in force: switch one of them off");
  // (tone tables in force become part of the call's source here, so that the graph slot below sees them)
  if (pr->tone_call(&call)) return 1;
  if (mask_dev)
    JH_CHECK_HIP(hipMemcpyAsync(pr->mask_buf, mask_dev, (size_t)pr->T * pr->C, hipMemcpyDeviceToDevice,
                                static_cast<hipStream_t>(stream)));
  pr->slot = 0;                               // (the whole-path forward and its captured graph: centre set 0)
  // a joint mask in force (jh_predictor_set_joint_mask): plain launches, no graph slot of its own -- the captured
  // graphs stay as they are and replay again once the mode is off
  // ... and so do centre keyframes (jh_predictor_set_center_keyframes)
  call.center_keys = pr->ck.every != 0;
  // is the CALLER capturing this stream?  Its graph then holds the plain launches, which every replay runs again
  // without this function: such a forward never boxes the head (HeatCall::Captured)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(call.s, &cs);
  // the head's box: only where stage 3 of this call is the one reader of the heat maps (conv_layer.h has the rule)
  call.head_roi = pr->kp->head_takes_box &&
                  head_box_allowed(cs != hipStreamCaptureStatusNone ? HeatCall::Captured : HeatCall::Forward,
                                   pr->jm_mode == JH_JOINT_MASK_CONSENSUS, pr->Cloc != pr->C, /*want_res1=*/false);
  if (pr->jm_mode != JH_JOINT_MASK_OFF) {
    call.joint_mask = pr->jm_buf;
    return forward_eager(pr, call, points_dev, conf_dev, valid_dev);
  }
  if (call.center_keys) return forward_eager(pr, call, points_dev, conf_dev, valid_dev);
  // per-launch profiling needs the launches one by one; a caller that is itself capturing this
  // stream gets the plain launches too
  if (!pr->use_graph || profiler().on || cs != hipStreamCaptureStatusNone)
    return forward_eager(pr, call, points_dev, conf_dev, valid_dev);
  return forward_graph(pr, call, points_dev, conf_dev, valid_dev);
}

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
  PlanSetup& setup = pr->setup;
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
  if (m.get(reinterpret_cast<void**>(&pr->head_box), (size_t)T * pr->Cloc * sizeof(int4))) return 1;
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
int64_t jh_predictor_graph_records(const jh_predictor* pr) { return pr ? pr->graph_records : 0; }

int64_t jh_predictor_launches(const jh_predictor* pr) {
  return (int64_t)((pr->center ? pr->center->launches() : 0) + pr->kp->launches() +
                   pr->v2v->launches());
}
int jh_predictor_precision(const jh_predictor* pr) { return pr ? pr->cfg.precision : -1; }

int64_t jh_predictor_device_bytes(const jh_predictor* pr) {
  return (int64_t)((pr->center ? pr->center->device_bytes() : 0) + pr->kp->device_bytes() +
                   pr->v2v->device_bytes() + pr->spread_bytes + pr->tone.bytes +
                   (pr->ck.plan ? pr->ck.plan->device_bytes() : 0) + pr->ck.bytes);
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

int jh_predictor_stage_center(jh_predictor* pr, const float* frames_dev, float* det_dev,
                              void* stream) {
  return stage_center_impl(pr, make_call(frames_dev, fixed_source(kSrcRgbF32), stream), det_dev);
}
int jh_predictor_stage_center_u8(jh_predictor* pr, const uint8_t* frames_dev, float* det_dev,
                                 void* stream) {
  return stage_center_impl(pr, make_call(frames_dev, fixed_source(kSrcBgrU8), stream), det_dev);
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

int jh_predictor_stage_keypoints_masked(jh_predictor* pr, const void* frames_dev, int format,
                                        const float* det_all_dev, const uint8_t* mask_dev, float* heat_dev,
                                        void* stream) {
  JH_REQUIRE(pr && mask_dev, "bad argument");
  JH_REQUIRE(format == JH_FRAME_RGB_F32 || format == JH_FRAME_BGR_U8, "masked stage 2: fp32 RGB or uint8 BGR frames");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "masked stage 2 needs all cameras local");
  return stage_keypoints_impl(pr, make_call(frames_dev, fixed_source(format), stream, mask_dev), det_all_dev, heat_dev,
                              1, true);
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

int jh_predictor_stage_3d_masked(jh_predictor* pr, const float* heat_all_dev, int t0, const uint8_t* mask_dev,
                                 float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && mask_dev, "bad argument");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "masked stage 3 needs all cameras local");
  return stage_3d_impl(pr, stage3_call(stream, mask_dev), heat_all_dev, t0, points_dev, conf_dev, valid_dev);
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

int jh_predictor_forward_surface(jh_predictor* pr, const uint8_t* frames_dev, const jh_yuv_surface* surface,
                                 const uint8_t* mask_dev, float* points_dev, float* conf_dev, int32_t* valid_dev,
                                 void* stream) {
  JH_REQUIRE(pr, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward_impl(pr, frames_dev, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
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
  if (call_source("forward_images", format, yuv, sensor, nullptr, pr->cfg.img_h, pr->cfg.img_w, true, &fs)) return 1;
  if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, pr->T * pr->C, fs,
                    static_cast<hipStream_t>(stream))) return 1;
  // (the launches read the table: `frames` itself is not dereferenced)
  return forward_impl(pr, pr->frames_table, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
}

int jh_predictor_forward_pixels(jh_predictor* pr, const uint8_t* frames_dev, const void* const* images_host,
                                int n_images, const jh_pixel_surface* surface, const uint8_t* mask_dev,
                                float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && surface, "jh_predictor_forward_pixels: null predictor / jh_pixel_surface");
  JH_REQUIRE(pr->Cloc == pr->C && pr->cfg.cam_lo == 0, "forward needs all cameras local");
  JH_REQUIRE((frames_dev != nullptr) != (images_host != nullptr),
             "jh_predictor_forward_pixels: give frames_dev or images_host, not both");
  FrameSource fs;
  if (call_source("jh_predictor_forward_pixels", kSrcPixels, nullptr, nullptr, surface, pr->cfg.img_h, pr->cfg.img_w,
                  images_host != nullptr, &fs)) return 1;
  const void* frames = frames_dev;
  if (images_host) {
    if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, pr->T * pr->C, fs,
                      static_cast<hipStream_t>(stream))) return 1;
    frames = pr->frames_table;                // (the launches read the table: `frames` itself is not dereferenced)
  }
  return forward_impl(pr, frames, fs, points_dev, conf_dev, valid_dev, stream, mask_dev);
}

int jh_predictor_debug_v2v(jh_predictor* pr, float* out_dev, void* stream) {
  JH_REQUIRE(pr && out_dev, "jh_predictor_debug_v2v: null pointer");
  return launch_from_channel_last(pr->v2v->output, out_dev, static_cast<hipStream_t>(stream));
}

int jh_predictor_debug_mask(jh_predictor* pr, int32_t* n_active_dev, int32_t* num_cams_detect_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(pr, "bad argument");
  const size_t n = (size_t)pr->T * sizeof(int);
  return copy_if(n_active_dev, pr->n_active, n, s) || copy_if(num_cams_detect_dev, pr->n_detect, n, s);
}

int jh_predictor_debug(jh_predictor* pr, float* center3d_f_dev, int32_t* center3d_i_dev,
                       int32_t* center_hm_dev, float* det_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t T = pr->T, C = pr->C;
  return copy_if(center3d_f_dev, pr->c3f, T * 3 * sizeof(float), s) ||
         copy_if(center3d_i_dev, pr->cur().c3i, T * 3 * sizeof(int), s) ||
         copy_if(center_hm_dev, pr->cur().chm, T * C * 2 * sizeof(int), s) ||
         copy_if(det_dev, pr->det_all, T * C * 3 * sizeof(float), s);
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
  pr->kp->head_box = nullptr;                     // (HeatCall::Hybridnet: the heat maps may go to the caller)
  pr->heat_boxed = false;
  if (pr->kp->run(s)) return 1;
  if (heatmaps_padded_dev) {
    const Act& h = pr->kp->heat;
    const size_t total = (size_t)h.N * pr->J * pr->hs * pr->hs;
    hipLaunchKernelGGL(export_padded_kernel, dim3(stride_blocks(total)), dim3(256), 0, s, h.p, heatmaps_padded_dev,
                       h.N, pr->J, h.Cp, pr->Hh);
    JH_CHECK_HIP(hipGetLastError());
  }
  return pr->run_3d(stage3_call(stream), pr->kp->heat.p, 0, heatmap_final_dev, points_dev, conf_dev);
}

}  // extern "C"
