// What the files of the C ABI (csrc/api*.hip) share: device scratch, the first-call workspaces, the value types a call
// is handed down as, the predictors themselves and the functions that cross files.  Internal: include/jarvis_hip.h is
// the interface.
#pragma once
#include <memory>
#include "../../include/jarvis_hip.h"
#include "nets.h"
#include "softargmax.h"
#include "joints3d.h"
#include "workspace.h"

// time one glue launch when the profiler is on (`s`: the stream of the function that uses it)
#define JH_PROF(name, flops, bytes, call)                      \
  do {                                                         \
    jh::Profiler& _pf = jh::profiler();                        \
    if (_pf.on) _pf.begin(name, flops, bytes, s);              \
    if (call) return 1;                                        \
    if (_pf.on) _pf.end(s);                                    \
  } while (0)

namespace jh {

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

// the spread form's sums and keys: one piece (launch_softargmax zeroes it with one launch)
inline size_t carve_spread(Carver& c, int t, int Jp, SoftargmaxSpread* sp) {
  const size_t n = softargmax_spread_sums(t, Jp);
  sp->sums = c.take<double>(n + (size_t)t * Jp);
  sp->key = sp->sums ? reinterpret_cast<unsigned long long*>(sp->sums + n) : nullptr;
  return c.off;
}

// Not inside a stream capture -- `what` is the site's own message for that.
inline int outside_capture(hipStream_t s, const char* what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cs);
  JH_REQUIRE(cs == hipStreamCaptureStatusNone, what);
  return 0;
}

// A buffer that the first call of its kind allocates (never jh_predictor_create): `bytes` of the predictor's memory,
// not inside a stream capture.
template <typename T>
int first_call_alloc(Scratch& mem, hipStream_t s, size_t bytes, const char* what, T** out) {
  if (outside_capture(s, what)) return 1;
  return mem.get(reinterpret_cast<void**>(out), bytes);
}

// ... and a workspace of several pieces (workspace.h: carve_first_call): ONE allocation of the predictor's memory, *out
// written only on success.  what == nullptr: a site without a stream, where the allocation itself fails inside a capture.
template <class Pieces, class Layout>
int first_call_carve(Scratch& mem, hipStream_t s, const char* what, Pieces* out, Layout&& lay,
                     CarveSizes* sizes = nullptr) {
  return carve_first_call([&](const char* w) { return outside_capture(s, w); },
                          [&](void** p, size_t bytes) { return mem.get(p, bytes); }, what, out, lay, sizes);
}

// An output a caller may leave out: copied on the stream, device to device, where a destination was given.
inline int copy_if(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (dst) JH_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
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
inline Scale2 center_scale2(const jh_predictor_config& c) {
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
  // centre keyframes in force (jh_predictor_set_center_keyframes): stage 1 ran on the key rows, and stage 2 fills the
  // rows in between behind its triangulation.  Set by the whole-path forward alone: the staged calls never have it.
  bool center_keys = false;
  // The voxel gather of this very call is the only reader of the heat maps stage 2 writes (conv_layer.h: head_box_allowed;
  // decided by the whole-path forward alone, the staged calls never have it): stage 2 projects the grid right behind
  // the centres, gives the keypoint head the box of every image and leaves stage 3 the coarse field.
  bool head_roi = false;
  hipStream_t s = nullptr;
};
inline Call make_call(const void* frames, const FrameSource& fs, void* stream, const unsigned char* mask = nullptr) {
  Call c;
  c.frames = frames; c.fs = fs; c.mask = mask; c.s = static_cast<hipStream_t>(stream);
  if (fs.per_image) c.cell = static_cast<const void* const*>(frames);
  return c;
}
inline Call stage3_call(void* stream, const unsigned char* mask = nullptr) {
  Call c;
  c.mask = mask; c.s = static_cast<hipStream_t>(stream);
  return c;
}

// Tone tables of a predictor (jh_predictor_set_tone / jh_predictor2d_set_tone): buf (cameras, 3, 256) is the predictor's
// copy, allocated by the first setting call; on: in force.  apply() puts them into a call's source -- image n of every
// launch is camera cam0 + n % cams -- and refuses fp32 frames, which have no byte; idempotent, so every function that
// fetches frames applies it to the call it was given.
struct ToneState {
  float* buf = nullptr;
  bool on = false;
  size_t bytes = 0;            // what jh_predictor_device_bytes reports for it
  int apply(Call* c, int cam0, int cams) const {
    if (!on) return 0;
    if (c->fs.fmt == kSrcRgbF32) {
      set_error("tone tables apply to byte frames");
      return 1;
    }
    c->fs.tone = buf; c->fs.tone_cam0 = cam0; c->fs.tone_cams = cams;
    return 0;
  }
  // the body of both setters: NULL switches the tables off (the buffer stays for the next setting call)
  int set(Scratch& mem, const float* tables_dev, int cams, hipStream_t s) {
    if (!tables_dev) {
      on = false;
      return 0;
    }
    const size_t n = (size_t)cams * 768 * sizeof(float);
    if (!buf) {
      if (first_call_alloc(mem, s, n, "the first set_tone call of a predictor allocates its table buffer: make it "
                           "outside a stream capture", &buf)) return 1;
      bytes = n;
    }
    JH_CHECK_HIP(hipMemcpyAsync(buf, tables_dev, n, hipMemcpyDeviceToDevice, s));
    on = true;
    return 0;
  }
};

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

}  // namespace jh

struct jh_params { jh::ParamMap map; };

struct jh_predictor {
  jh_predictor_config cfg{};
  int T3 = 0;
  int T = 0, C = 0, Cloc = 0, J = 0, Jp = 0, B = 0, Hh = 0, G = 0, Gh = 0, hs = 0;
  std::unique_ptr<jh::EffTrackPlan> center, kp;
  std::unique_ptr<jh::V2VPlan> v2v;
  jh::Scratch mem;
  float *cam = nullptr, *intr = nullptr, *dist = nullptr;
  // Per-frame calibration (jh_predictor_set_calibration_frames): T rows of the three arrays above, allocated by the
  // first such call.  calib_fs is the frame stride every launch that reads calibration is given: 0 -- all frames read
  // cam / intr / dist --, or C -- frame t reads row t of cam_f / intr_f / dist_f.  A call that starts at frame t0
  // (stage 3, views2d) passes the rows from t0 on, as it passes the centres' and the mask's.
  float *cam_f = nullptr, *intr_f = nullptr, *dist_f = nullptr;
  int calib_fs = 0;
  jh::Calib calib_at(int t0) const {
    return calib_fs ? jh::Calib{cam_f, intr_f, dist_f, calib_fs}.at(t0) : jh::Calib{cam, intr, dist, 0};
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
  // The keypoint head's boxes, [T * Cloc] (x0, y0, x1, y1): written by stage 2 of a call with
  // Call::head_roi, read by the head's launch of that call (device data: a captured graph bakes the pointer only).
  // heat_boxed: the predictor's own heat maps were last written by such a call -- outside the boxes they hold whatever
  // they held before -- and whoever reads them afterwards calls full_heat() first, which runs the head once more
  // without a box on the operand stage 2 left (the same bits a box-less call writes), every time it is needed.
  // heat_boxed is HOST knowledge about device data, so it is only ever changed by calls whose launches the host makes
  // itself: a forward on a stream the caller is capturing never boxes (HeatCall::Captured), and a reader that is being
  // captured -- its launches will run again behind forwards this flag knows nothing of -- records the head's launch
  // whatever the flag says.
  int4* head_box = nullptr;
  bool heat_boxed = false;
  int full_heat(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cs);
    if (cs != hipStreamCaptureStatusNone) return kp->head_takes_box ? kp->run_head(s) : 0;
    if (!heat_boxed) return 0;
    heat_boxed = false;
    return kp->run_head(s);
  }
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
  struct GraphSlot { hipGraphExec_t exec = nullptr; jh::FrameSource src; int calib_fs = 0; };
  GraphSlot gslot[jh::kGraphSlots];
  int64_t graph_records = 0;                 // recordings made so far (jh_predictor_graph_records): a replay adds none
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
  // (max, index) partials of the all-joint argmax behind jh_predictor_views2d, [T3 * C][slices][Jp] each: ONE
  // allocation made by the first such call, so a predictor that never asks for 2D views owns what it always did
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
  // accumulators for one 3D chunk.  All of it ONE allocation, made by the first enabling call (spread_bytes: the bytes
  // of its pieces): a predictor that never asks owns, and launches, what it always did.
  bool spread_on = false;
  jh::SoftargmaxSpread spread;
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
  jh::JointSets jm_sets;
  jh::Joints3dParams jm_params{};
  float *jm_points = nullptr, *jm_error = nullptr;
  int* jm_views = nullptr;
  // Centre keyframes (jh_predictor_set_center_keyframes; center_keys.h has the key rows).  every: 0 = off; n_rows: the
  // real rows of the batch.  plan: a second CenterDetect plan for K * C images -- K = center_key_slots(T, every) -- in
  // THIS predictor's time-batch class (setup), so that a key row gets the bits the full plan gives it.  table [T * C]:
  // the key rows' image pointers, which the plan's fetch reads per image; det [T][C][3]: the key slots' detections;
  // centers [T][3] / source [T]: what the fill wrote.  The buffers are ONE allocation (bytes: its pieces) and the plan
  // is built by the first enabling call, never by jh_predictor_create; another `every` builds another plan.
  struct CenterKeys {
    int every = 0, n_rows = 0, K = 0;
    std::unique_ptr<jh::EffTrackPlan> plan;
    const void** table = nullptr;
    float *det = nullptr, *centers = nullptr;
    int* source = nullptr;
    size_t bytes = 0;
  } ck;
  jh::PlanSetup setup;                       // what jh_predictor_create built its plans with
  // Tone tables (jh_predictor_set_tone), all num_cameras cameras': a launch's image n is camera cam_lo + n % Cloc
  jh::ToneState tone;
  int tone_call(jh::Call* c) const { return tone.apply(c, cfg.cam_lo, Cloc); }
  ~jh_predictor() {
    for (auto& g : gslot) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (gstream) (void)hipStreamDestroy(gstream);
  }

  // 3D stage for frames t0 .. t0+T3-1 of the batch (heat_all holds those frames): api_predictor.hip
  // (call.head_roi: stage 2 of this call has projected the grid already -- `coarse` is ready)
  int run_3d(const jh::Call& call, const float* heat_all, int t0, float* heatmap_final, float* points, float* conf,
             const jh::HeatLayout* layout = nullptr);
};

struct jh_predictor2d {
  jh_predictor_config cfg{};
  int T = 0, J = 0, B = 0;
  std::unique_ptr<jh::EffTrackPlan> center, kp;
  jh::Scratch mem;
  float* det = nullptr;
  int *chm = nullptr, *valid = nullptr;
  const void** frames_table = nullptr;       // per-image frames: [T] device pointers (jh_predictor2d_forward_images)
  jh::ToneState tone;                        // one camera's tables (jh_predictor2d_set_tone)
};

namespace jh {

// ---- what crosses files
// api_frames.hip: the frame descriptions
FrameSource fixed_source(int format);
int frame_source(const jh_yuv_surface* sp, int h, int w, FrameSource* out);
int frame_source(const jh_sensor_surface* sp, int h, int w, FrameSource* out);
int frame_source(const jh_pixel_surface* sp, int h, int w, FrameSource* out);
int frame_source(int format, int h, int w, FrameSource* out);
int call_source(const char* who, int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                const jh_pixel_surface* pixels, int h, int w, bool per_image, FrameSource* out);
int upload_images(Scratch& mem, const void*** table, const void* const* images_host, int n_images, int want,
                  const FrameSource& fs, hipStream_t s);
// api_frames.hip: bytes from one image of contiguous frames to the next
long long image_bytes(const FrameSource& fs, int h, int w);
// api_predictor.hip: the stages
int center_heat_impl(jh_predictor* pr, const Call& call);
int stage_3d_impl(jh_predictor* pr, const Call& call, const float* heat_all_dev, int t0, float* points_dev,
                  float* conf_dev, int32_t* valid_dev, const HeatLayout* layout = nullptr);
// api_features.hip: the three launches of jh_predictor_triangulate_joints (the consensus of the whole-path forward runs
// them between stage 2 and stage 3)
int triangulate_joints_launches(jh_predictor* pr, const float* heat_all_dev, int t0, const unsigned char* mask_dev,
                                const Joints3dParams& jp, float* points_dev, int* views_dev, unsigned char* members_dev,
                                float* error_dev, float* obs_dev, hipStream_t s);

}  // namespace jh
