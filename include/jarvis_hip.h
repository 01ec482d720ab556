/* libjarvis_hip.so -- C ABI of the MI355X (gfx950) implementation of the
 * JARVIS-HybridNet multi-view inference hot path.
 *
 * This is the drop-in boundary: plain C, raw device pointers, explicit shapes,
 * an explicit hipStream_t (passed as void*), int status (0 = OK; the message of
 * the last failure on the calling thread is returned by jh_last_error()).
 * No forward entry point synchronises the device or allocates memory: networks and
 * predictors own their intermediates (allocated by *_create), the stand-alone
 * operators (jh_reproject_forward, jh_softargmax, jh_reconstruct_point) take a
 * caller-provided device workspace sized by the matching jh_*_workspace_bytes().
 * A whole forward may therefore be captured into a hipGraph
 * (tests/test_hip_stages.py::test_submodule_path_graph_capture).  The only
 * exceptions are the jh_op_* unit-test helpers at the end of this file, which say so.
 *
 * The library occupies the seam the reference itself uses for acceleration:
 * JarvisPredictor3D replaces three sub-networks by compiled modules after
 * torch.ops.load_library(<native .so>)  (jarvis/prediction/jarvis3D.py:50-69,
 * 72-125, binary converters under libs/).  Each entry point below cites the
 * reference function it replaces.
 *
 * Conventions: all tensors fp32 unless noted; "dev" = device pointer, "host" =
 * host pointer; NCHW / NCDHW = the reference's layouts; calibration in the
 * reference's transposed storage (jarvis/utils/reprojection.py:33-39):
 * cameraMatrices (C,4,3), intrinsicMatrices (C,3,3) with the principal point in
 * row 2, distortionCoefficients (C,1,5) with k1,k2 first.
 */
#ifndef JARVIS_HIP_H
#define JARVIS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JH_ABI_VERSION 4

const char* jh_last_error(void);
int jh_abi_version(void);

/* ---- precision mode.  A predictor carries its own (jh_predictor_config.precision, ABI v4): two
 * predictors of different precision coexist in one process and do not depend on call order.
 * jh_set_precision() only sets the process-wide DEFAULT: what the stand-alone networks
 * (jh_efftrack_create, jh_v2v_create, jh_op_*) CREATED from now on use, and what a predictor
 * configured with JH_PRECISION_DEFAULT picks up when it is created.
 * JH_PRECISION_F32 (default): fp32 products and accumulation everywhere, the mode every parity
 * figure of this library is quoted in.  JH_PRECISION_BF16X3: the 3x3x3 stride-1 convolutions of
 * V2V, its stride-2 front convolution and the keypoint head's ConvTranspose2d run on the bf16 matrix
 * cores with each fp32 operand split into two bf16 terms (three MFMAs per product, fp32 accumulation;
 * about 2^-16 relative per product) -- the labelled
 * reduced-precision mode that stands where the reference has its half-precision TensorRT
 * engines (jarvis/prediction/jarvis3D.py:93,107,122: enabled_precisions={torch.half}).
 * JH_PRECISION_BF16X3_WIDE additionally splits the dense k x k convolutions of the EfficientNet trunk
 * (experimental: up to 7.6e-4 mm on the fixture cases, no margin under the 1e-3 mm bar).
 * Environment JH_PRECISION=bf16x3 / bf16x3_wide sets the initial mode. */
#define JH_PRECISION_DEFAULT (-1) /* jh_predictor_config.precision only: follow jh_set_precision / JH_PRECISION */
#define JH_PRECISION_F32 0
#define JH_PRECISION_BF16X3 1
#define JH_PRECISION_BF16X3_WIDE 2
int jh_set_precision(int mode);
int jh_get_precision(void);

/* ---- parameters: a state dict in the reference's .pth key layout ----------
 * Replaces torch.load + load_state_dict of jarvis/hybridnet/hybridnet.py:84-97
 * and jarvis/efficienttrack/efficienttrack.py:90-113 on the native side. */
typedef struct jh_params jh_params;
int jh_params_create(jh_params** out);
int jh_params_set(jh_params* p, const char* key, const float* host, int64_t numel);
void jh_params_destroy(jh_params* p);

/* ---- EfficientTrackBackbone.forward  (jarvis/efficienttrack/model.py:114-130)
 * model_size: 0 small, 1 medium, 2 large.  Built for a fixed (N,3,H,W) input.
 * forward: x (N,3,H,W) NCHW dev -> res1 (N,J,H/4,W/4), res2 (N,J,H/2,W/2) NCHW dev:
 * the (res1, res2) tuple of model.py:126-130, i.e. the tensor contract of the
 * reference's trt_mode seam (jarvis3D.py:64-69).  res1 (final_conv1, model.py:128) is
 * never read on the inference path (hybridnet/model.py:57-58, jarvis3D.py:147): it is
 * computed only by networks created with want_res1 != 0, and res1_dev may be NULL. */
typedef struct jh_efftrack jh_efftrack;
int jh_efftrack_create(const jh_params* p, const char* prefix, int model_size, int joints, int n,
                       int h, int w, int want_res1, jh_efftrack** out);
int jh_efftrack_forward(jh_efftrack* net, const float* x_dev, float* res1_dev, float* res2_dev,
                        void* stream);
int64_t jh_efftrack_launches(const jh_efftrack* net);
void jh_efftrack_destroy(jh_efftrack* net);

/* ---- V2VNet.forward  (jarvis/hybridnet/v2vnet.py:98-102)
 * x (T,J,G,G,G) NCDHW dev -> y (T,J,G/2,G/2,G/2) NCDHW dev. */
typedef struct jh_v2v jh_v2v;
int jh_v2v_create(const jh_params* p, const char* prefix, int joints, int t, int g, jh_v2v** out);
int jh_v2v_forward(jh_v2v* net, const float* x_dev, float* y_dev, void* stream);
void jh_v2v_destroy(jh_v2v* net);
/* Whether a V2V plan created NOW for (joints, t, g) ends in the output fold (no GPU needed): *folded = 1 -- the closing
 * passes of skip_res1 and decoder_res1 are applied by the output layer's launch on load, two launches fewer, same bits
 * -- or 0: the three launches.  A function of (joints, g) -- at most 32 joints, g a multiple of 8 -- and of JH_V2V_FOLD
 * (default on; 0: never) as it stands at the call, never of t.  Predictors build their V2V plan by the same rule. */
int jh_v2v_fold(int joints, int t, int g, int* folded);

/* ---- ReprojectionLayer.forward  (jarvis/hybridnet/repro_layer.py:110-119)
 * heatmaps_padded (1,C,J,hs,hs) NCHW dev, center3d (3) int32 dev, center_hm
 * (C,2) int32 dev, calibration dev -> vol (1,J,G,G,G) NCDHW dev (NOT divided by
 * 255, like the reference layer).  idx_dev (C,G,G,G) int32 optional (may be
 * NULL): the reference's integer gather index (reprojectPoints, :40-85).
 * workspace_dev: >= jh_reproject_workspace_bytes(cams, joints, hs, grid_size) bytes of
 * device memory (256-byte aligned), owned by the caller, contents irrelevant. */
int64_t jh_reproject_workspace_bytes(int cams, int joints, int hs, int grid_size);
int jh_reproject_forward(const float* heatmaps_padded_dev, int cams, int joints, int hs,
                         const int32_t* center3d_dev, const int32_t* center_hm_dev,
                         const float* cam_dev, const float* intr_dev, const float* dist_dev,
                         int grid_size, float grid_spacing, float* vol_dev, int32_t* idx_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ---- soft-argmax tail of HybridNetBackbone.forward (hybridnet/model.py:73-88)
 * v2v_out (T,J,Gh,Gh,Gh) NCDHW dev, center3d (T,3) int32 dev -> points (T,J,3),
 * conf (T,J), heatmap_final (T,J,Gh,Gh,Gh) optional (NULL to skip).
 * workspace_dev: >= jh_softargmax_workspace_bytes(t, joints, gh) bytes, as above. */
int64_t jh_softargmax_workspace_bytes(int t, int joints, int gh);
int jh_softargmax(const float* v2v_out_dev, int t, int joints, int gh, float grid_spacing,
                  float roi_cube_size, const int32_t* center3d_dev, float* heatmap_final_dev,
                  float* points_dev, float* conf_dev, void* workspace_dev, int64_t workspace_bytes,
                  void* stream);

/* ---- ReprojectionTool  (jarvis/utils/reprojection.py:49-90)
 * reproject: points (P,3) dev -> uv (C,P,2) dev.
 * reconstruct: points2d (2,C) dev (pixels), maxvals (C) dev -> point3d (3) dev;
 * workspace_dev: >= jh_reconstruct_workspace_bytes(cams) bytes, as above. */
int jh_reproject_point(const float* points_dev, int npoints, int cams, const float* cam_dev,
                       const float* intr_dev, const float* dist_dev, float* uv_dev, void* stream);
int64_t jh_reconstruct_workspace_bytes(int cams);
int jh_reconstruct_point(const float* points2d_dev, const float* maxvals_dev, int cams,
                         const float* cam_dev, const float* intr_dev, const float* dist_dev,
                         float* point3d_dev, void* workspace_dev, int64_t workspace_bytes,
                         void* stream);

/* ---- JarvisPredictor3D  (jarvis/prediction/jarvis3D.py:20-46,129-190) and
 * HybridNetBackbone.forward (jarvis/hybridnet/model.py:53-90).
 * One object owns both 2D networks, the V2V network and every intermediate.
 * time_batch T independent multi-view frames are processed per call (the
 * reference's batch-1 call is T = 1).  cam_lo/cam_n select the cameras whose 2D
 * work this process owns (camera sharding across GPUs); the 3D stage always
 * sees all cameras. */
typedef struct jh_predictor jh_predictor;
typedef struct {
  int32_t num_cameras, num_joints;
  int32_t center_size;        /* CENTERDETECT.IMAGE_SIZE */
  int32_t bbox;               /* KEYPOINTDETECT.BOUNDING_BOX_SIZE */
  float roi_cube_size;        /* HYBRIDNET.ROI_CUBE_SIZE (mm) */
  float grid_spacing;         /* HYBRIDNET.GRID_SPACING (mm) */
  int32_t center_model, kp_model;   /* 0 small, 1 medium, 2 large */
  int32_t img_h, img_w;
  int32_t time_batch;         /* T: frames per call through the 2D stages */
  int32_t time_batch_3d;      /* frames per stage_3d call (<= T; 0 means T) */
  int32_t cam_lo, cam_n;
  float mean[3], std[3];      /* DATASET.MEAN / DATASET.STD */
  int32_t precision;          /* JH_PRECISION_F32 (0: what a zero-initialised struct gets), _BF16X3, _BF16X3_WIDE,
                               * or JH_PRECISION_DEFAULT = the process default at creation time.  The mode that
                               * stands where the reference has trt_mode != 'off' (jarvis3D.py:42-46,93,107,122) */
} jh_predictor_config;

/* center_params may be NULL (HybridNetBackbone-only use). */
int jh_predictor_create(const jh_params* center_params, const jh_params* hybrid_params,
                        const jh_predictor_config* cfg, jh_predictor** out);
void jh_predictor_destroy(jh_predictor* pr);
int64_t jh_predictor_launches(const jh_predictor* pr);
int64_t jh_predictor_device_bytes(const jh_predictor* pr);
int jh_predictor_precision(const jh_predictor* pr);    /* the resolved mode (never JH_PRECISION_DEFAULT) */

/* calibration of all cameras (device pointers, copied). */
int jh_predictor_set_calibration(jh_predictor* pr, const float* cam_dev, const float* intr_dev,
                                 const float* dist_dev, void* stream);
/* Per-frame-set calibration (ABI v4, additive): one calibration PER FRAME SET of the time batch, as the reference
 * passes one with every call (jarvis3D.py:127-133) and its validation analysis takes each sample's own
 * (jarvis/analysis/analyze.py:54-96).
 *   cam (T,C,4,3), intr (T,C,3,3), dist (T,C,1,5) dev, T = time_batch: row t is the calibration of frame set t, in the
 *   layout of jh_predictor_set_calibration.  Rows of ALL T frame sets are given, also with time_batch_3d < T and
 *   on a camera-sharded predictor (every rank triangulates all T frames; stage 3 and the 2D views of the frames
 *   t0 .. read rows t0 ..).
 * Lifetime: the rows are COPIED, on `stream`, into buffers the predictor owns (T times the shared ones).  The first such
 * call of a predictor allocates them -- never jh_predictor_create, so jh_predictor_device_bytes and the memory of a
 * predictor that never uses it are unchanged -- and that first call must not be made inside a stream capture.
 * After it every entry point of this predictor reads row t for frame set t -- all forwards,
 * jh_predictor_stage_keypoints*, jh_predictor_stage_3d* (_blocks, _masked), jh_predictor_views2d,
 * jh_predictor_hybridnet_forward -- until
 * jh_predictor_set_calibration returns it to the shared form; the two calls may alternate freely.  The stand-alone
 * operators (jh_reproject_forward, jh_reconstruct_point, jh_reproject_point) take one calibration, as before.
 * Graph replay: a recorded graph holds the buffers' addresses and the form.  A change of FORM (shared <-> per frame)
 * between two forwards records again (the replay in flight is waited for before its executable graph goes), as a
 * described surface whose description changes does; a change of VALUES within one form keeps replaying the one
 * recording, because the values live in the predictor's buffers.
 * Results: only the address of a frame set's 12 + 9 + 5 floats per camera differs between the forms -- the arithmetic
 * is the same, operation for operation.  Row t of a batch under per-frame calibration therefore equals, BIT FOR BIT,
 * row t of the same batch (same predictor, frames and mask row) run with calibration k(t) as the shared calibration:
 * points, confidences, valid, the float and integer 3D centre, the crop centres, num_cams_detect and the five outputs
 * of jh_predictor_views2d.  jh_predictor_set_calibration and everything that follows it keep the bits they had.
 * Validation: pr and the three pointers non-NULL; otherwise non-zero with jh_last_error() set, nothing enqueued. */
int jh_predictor_set_calibration_frames(jh_predictor* pr, const float* cam_dev /* (T,C,4,3) */,
                                        const float* intr_dev /* (T,C,3,3) */, const float* dist_dev /* (T,C,1,5) */,
                                        void* stream);

/* Caller-supplied 3D centres (ABI v4, additive; new design: the reference always detects, jarvis3D.py:135-166).  Stage 1
 * only decides where the crops and the voxel cube go; a caller that knows where the subject is -- the centroid of the
 * previous result when tracking, a fixed volume, an external detector, several subjects seen in the same frames (one
 * centre per row of a jh_predictor_forward_images batch whose rows share their image pointers) -- gives the centres
 * and stage 1 does not run: no resize, no CenterDetect, no centre arg-max, no triangulation.
 *   centers (T,3) fp32 dev, T = time_batch: row t is the centre of frame set t in world millimetres; NULL returns the
 *   predictor to detection.  The two may alternate freely, call by call.
 * Lifetime: the rows are COPIED, on `stream`, into a buffer the predictor owns (T * 12 bytes).  The first such call of
 * a predictor allocates it -- never jh_predictor_create, so jh_predictor_device_bytes and the memory of a predictor that
 * never uses it are unchanged -- and that first call must not be made inside a stream capture.
 * After it every whole-path forward of this predictor (jh_predictor_forward, _u8, _yuv, _surface, _sensor, _masked,
 * _images) skips stage 1 and runs stage 2 from the centres, and every jh_predictor_stage_keypoints* call (_u8, _masked,
 * _gathered) ignores its det argument, which may then be NULL; jh_predictor_stage_center* is not affected.  A
 * predictor created with center_params == NULL runs centred whole-path forwards (without graph replay, which such a
 * predictor does not have); its detected ones keep failing with "created without CenterDetect weights".
 * For every frame set t:
 *   center3d float = centers[t];  center3d int = (int)centers[t], truncation toward zero (center3D.int(),
 *   jarvis3D.py:183);  center_hm[t][c] = clamp((int)reprojectPoint(centers[t])[c]) under the calibration in force
 *   (shared or per frame set) -- the very operations that follow the triangulation of a detected call;
 *   valid[t] = 1 iff the three coordinates are finite and |x| < 2^24 (no detection ran: there is no `> 50` gate) and,
 *   under a camera mask, at least one camera of row t is unmasked.  jh_predictor_debug_mask then reports n_active as for
 *   a detected masked call and num_cams_detect = 0.
 *   An invalid row is computed as if its centre were (0,0,0): nothing that is not finite or not in range is converted
 *   to an integer, a projection that is not finite or not representable takes the clamp's lower bound, and the row's
 *   crops are in range.  Its points / confidences are unspecified, as for the invalid rows of a detected call.
 * Everything downstream is the code of a detected call on those buffers: crop stem or crop kernel, KeypointDetect,
 * reprojection gather (plain or masked), V2V, soft-argmax, jh_predictor_views2d.
 * Graph replay: the centred forward has graph slots of its own, as the masked and the per-image forms have, so
 * alternating centred and detected calls records each once; the centres' VALUES live in the predictor's buffer and may
 * change from call to call under one recording.
 * Results: a centred call whose centres are the float centres of a detected call (jh_predictor_debug's center3d of the
 * same frames, calibration and mask) equals that call BIT FOR BIT in points, confidences, valid, the integer centre,
 * the crop centres and the five outputs of jh_predictor_views2d, wherever the detected call is valid.  A predictor that
 * is never given centres makes the launches it always made.
 * jh_predictor_debug after a centred call reports the supplied center3d and the integers and crop centres derived
 * from it; det is left as the last detected call wrote it.
 * Validation: pr non-NULL; otherwise non-zero with jh_last_error() set, nothing enqueued. */
int jh_predictor_set_centers(jh_predictor* pr, const float* centers_dev /* (T,3) or NULL */, void* stream);

/* Centre keyframes (ABI v4, additive; new design: the reference detects on every frame set).  The rows of a time batch
 * are consecutive frame sets, and stage 1 only decides where the crops and the voxel cube go: CenterDetect runs on the
 * KEY rows of the batch -- every k-th row and the last one --, the rows in between take a centre interpolated on the
 * device between their two key rows, and every row then runs the centred stage 2 and stage 3 of
 * jh_predictor_set_centers.  Opt-in: a predictor that never asks owns, launches and computes what it always did.
 *
 * Definition, for T = time_batch rows of which the first n_rows are real (1 <= n_rows <= T; a short last group of a
 * recording is padded behind them) and every = k >= 1:
 *  1. Key rows.  Key slot i holds row min(i * k, n_rows - 1).  The distinct ones are keys = {0, k, 2k, ... < n_rows}
 *     and n_rows - 1, ascending: ceil((n_rows - 1) / k) + 1 of them.  A predictor has K(T, k) = ceil((T - 1) / k) + 1
 *     key slots (1 for T = 1), the count at n_rows = T; with n_rows < T the slots behind the last key repeat it, so no
 *     launch size depends on n_rows and nothing is read out of range.  jh_center_keyframe_rows is this rule on the host.
 *  2. Stage 1 on the key slots.  The resize (or fused stem fetch), CenterDetect and the centre arg-max run on K * C
 *     images, image (i, c) being camera c of key slot i's row, read where it lies through the per-image fetch (any frame
 *     format, tone tables included).  CenterDetect is a second launch plan of the predictor, for K * C images in the
 *     PREDICTOR's time-batch class, so a key row's detection has the bits the full plan gives that row.  The detections
 *     of slot i go to row keys[i] of the (T,C,3) detection buffer; every other row of it is zero.
 *  3. The triangulation of a detected call (plain, or masked under a camera mask) runs over all T rows: a key row gets
 *     its float centre and valid = (cameras with maxval > 50) >= 2 with the arithmetic of a detected call.
 *  4. Fill, row t -> centre[t] (fp32) and source[t] (int32):
 *       t a key row:   valid -> its float centre unchanged, source 0 (detected); not valid -> NaN, source -1.  An invalid
 *                      key row is never given a neighbour's centre.
 *       t between the key rows ta < t < tb, a and b their float centres:
 *         both valid   w = (float)(t - ta) / (float)(tb - ta);  centre = a + (b - a) * w, per coordinate, every operation
 *                      rounded once to fp32 and none contracted (fdiv, fsub, fmul, fadd in that order); source 1.
 *         one valid    that key's centre unchanged, source 2 (held).
 *         none valid   NaN, source -1.
 *       t >= n_rows:   the centre of row n_rows - 1, source 2, or NaN and -1 where that row is not valid.
 *  5. The filled (T,3) centres go through the code of jh_predictor_set_centers: integer centre, crop centres and valid
 *     as defined there (a NaN centre is its invalid row), then the crop stem, KeypointDetect, the gather, V2V and the
 *     tail, and behind them jh_predictor_views2d, the spread, jh_predictor_triangulate_joints and the joint-mask
 *     consensus, exactly as after jh_predictor_set_centers.
 * Results: with every = 1 every row is a key row and the call equals the detected call bit for bit wherever that is
 * valid (an invalid row is the invalid row of a centred call: computed as if its centre were (0,0,0)).  For any k the
 * call equals, bit for bit, the centred call on the filled centres, whose key rows are the detected call's.  A valid
 * key row whose triangulated centre is not finite or not below 2^24 is an invalid row here (jh_predictor_set_centers).
 * The result depends on which rows share a batch: the key rows are rows of the batch.
 *
 * jh_center_keyframe_rows: host only, no device is touched.  The distinct key rows of (time_batch, every, n_rows),
 * ascending, into rows[0 .. cap); rows may be NULL (cap is then ignored).  Returns their number, or -1 with
 * jh_last_error() set: time_batch < 1, every < 1, n_rows outside 1 .. time_batch, cap below the number.
 *
 * jh_predictor_set_center_keyframes: every = 0 switches the feature off (center_params may be NULL; the plan and the
 * buffers stay for the next enabling call).  every >= 1: from now on every whole-path forward of this predictor
 * (jh_predictor_forward, _u8, _yuv, _surface, _sensor, _pixels, _masked, _images) is a keyframe call with that every
 * and n_rows.  It runs plain launches and touches no graph slot, like a joint-masked call; the captured graphs replay
 * with their bits once it is off.  The staged entry points, jh_predictor_detect_subjects and the 2D predictor are not
 * affected.  The first enabling call builds the key plan and allocates the buffers (T * C pointers and detections, the
 * (T,3) centres and (T) sources) -- never jh_predictor_create, so jh_predictor_device_bytes grows only then --, and a
 * call whose every gives another K builds another plan in place of it.  Such a call needs center_params (CenterDetect's
 * parameters again: those of jh_predictor_create may be gone), must be made outside a stream capture and synchronises
 * the device; a call that changes n_rows alone, or every within one K, builds nothing, and center_params may be NULL.
 * Validation, non-zero with jh_last_error() set and nothing enqueued: pr NULL; every < 0; a predictor created without
 * CenterDetect weights; cam_n < num_cameras; n_rows outside 1 .. time_batch; center_params NULL where the plan has to be
 * built.  Caller-supplied centres and keyframes both in force: the FORWARD fails, with a message that names both.
 *
 * jh_predictor_get_center_keyframes: the filled centres (T,3) fp32 and sources (T) int32 of the last keyframe call,
 * copied on `stream`; either may be NULL.
 * jh_predictor_debug after a keyframe call: center3d is the filled centre, the integers and crop centres are derived
 * from it, det holds the key rows' detections and zeros elsewhere.  jh_predictor_debug_mask after a masked one: n_active
 * as for a detected masked call, num_cams_detect = 0 as after a centred call (the key rows' counts are not kept). */
int jh_center_keyframe_rows(int time_batch, int every, int n_rows, int32_t* rows, int cap);   /* no GPU needed */
int jh_predictor_set_center_keyframes(jh_predictor* pr, const jh_params* center_params, int every, int n_rows,
                                      void* stream);
int jh_predictor_get_center_keyframes(jh_predictor* pr, float* centers_dev /* (T,3) */, int32_t* source_dev /* (T) */,
                                      void* stream);

/* Per-camera tone tables: black level, gain, white balance and gamma as ONE byte-to-value lookup inside the resize /
 * crop fetch, so that raw-sensor, decoder-surface and plain BGR frames reach the networks in the distribution the
 * networks were trained on without a host pass.
 * tables (num_cameras,3,256) fp32 (the 2D predictor: (3,256)): tables[c][ch][k] is the value the pre-processing sees
 * for byte k of channel ch (0 = R, 1 = G, 2 = B) of camera c, in place of k * (1/255).  All num_cameras cameras' tables
 * are given, also to a camera-sharded predictor (cam_lo, cam_n), which reads rows cam_lo .. cam_lo + cam_n - 1.
 * Every byte source form is covered: uint8 BGR, I420 / NV12, jh_yuv_surface, jh_sensor_surface, their wide forms and
 * jh_pixel_surface.  A pixel is first converted to its (R, G, B) bytes exactly as without tables (colour conversion,
 * demosaic, sample reduction); each byte is then replaced by tables[c][ch][byte]; everything after that is untouched:
 * the four-tap bilinear resize, the crop's zero outside the frame, (v - mean) / std.
 * Results: a forward under tables equals, BIT FOR BIT, jh_predictor_forward on the fp32 RGB frames
 * F[t][c][ch][y][x] = tables[c][ch][B[t][c][y][x][ch]], B being the bytes the form's jh_op_*_to_bgr helper gives --
 * in points, confidences, valid, jh_predictor_debug, jh_predictor_views2d and everything else that follows a forward.
 * tables[..][k] = fl(fl(k) * fl(1/255)) gives the bits of the call without tables;
 * tables[c][ch][k] = fl(fl(L[c][ch][k]) * fl(1/255)) for a uint8 LUT L gives the bits of jh_predictor_forward_u8 on the
 * L-mapped bytes.
 * The index is always the clamped byte the conversion produced, 0 .. 255: whatever the frames hold (a masked camera's
 * garbage, padding), no table read leaves its 256 entries, and nothing outside the planes is read, as without tables.
 * Table values are taken as given and should be finite.
 * fp32 RGB frames have no byte: a call with fp32 frames while tables are set fails with jh_last_error()
 * "tone tables apply to byte frames" and enqueues nothing.
 * Read by every entry point that fetches frames: the whole-path forwards (_u8, _yuv, _surface, _sensor, _pixels,
 * _masked, _images), jh_predictor_stage_center_u8, jh_predictor_stage_keypoints_u8 / _masked / _gathered,
 * jh_predictor_detect_subjects*, and the 2D forwards.
 * Lifetime, as jh_predictor_set_centers: the tables are copied on `stream` into a buffer the predictor owns, allocated
 * by the first such call (never by *_create, not inside a stream capture; jh_predictor_device_bytes grows by it only
 * then).  NULL returns to the plain form.  A predictor that never asks makes the launches it always made.
 * Graph replay: a recording is made with or without tables, so switching them on or off records again; the VALUES live
 * in the predictor's buffer and may change from call to call under one recording.
 * Out of scope: tables indexed by more than 8 bits (with JH_SAMPLE_U16(shift) a caller chooses WHICH 8 bits of a wide
 * sample index the table); a 3x3 colour-correction matrix; gains applied before the demosaic (with linear gains the
 * per-channel table commutes with the bilinear demosaic up to rounding); rounding instead of truncation of wide samples.
 * Validation: pr non-NULL; otherwise non-zero with jh_last_error() set, nothing enqueued. */
int jh_predictor_set_tone(jh_predictor* pr, const float* tables_dev /* (num_cameras,3,256) or NULL */, void* stream);
/* (jh_predictor2d_set_tone and the unit-test helper jh_op_frames_to_rgb_f32 are declared with the 2D predictor and
 *  the frame descriptions, below) */

/* Stage 1 (jarvis3D.py:135-155): resize + normalise + CenterDetect + argmax for
 * the owned cameras.  frames (T,cam_n,3,H,W) dev -> det (T,cam_n,3) = (x, y,
 * raw maxval) dev. */
int jh_predictor_stage_center(jh_predictor* pr, const float* frames_dev, float* det_dev,
                              void* stream);
/* Stage 2 (jarvis3D.py:157-178 + model.py:55-63): det_all (T,C,3) of ALL cameras
 * -> triangulate, project, crop + normalise + KeypointDetect for the owned
 * cameras -> heat (T,cam_n,B/2,B/2,Jp) channel-last dev, Jp = joints rounded up
 * to 8. */
int jh_predictor_stage_keypoints(jh_predictor* pr, const float* frames_dev,
                                 const float* det_all_dev, float* heat_dev, void* stream);
/* Stage 3 (model.py:65-88) for the time_batch_3d frames t0 .. t0+T3-1 of the
 * batch: heat_all (T3,C,B/2,B/2,Jp) of ALL cameras for those frames -> points
 * (T3,J,3), conf (T3,J), valid (T3) int32 (0 = fewer than two cameras saw the
 * subject: the reference returns (None, None), jarvis3D.py:187-190).
 * Pipelining: a predictor keeps TWO sets of (crop centres, truncated 3D centre, validity).  Every
 * stage-2 call (jh_predictor_stage_keypoints*) writes the set the previous stage-2 call did not; a
 * stage-3 call reads the set of the stage-2 call that preceded it in HOST CALL ORDER.  Stage 3 of
 * time batch i may therefore run on a second stream concurrently with stage 2 of batch i+1 -- they
 * share no buffer -- provided the caller orders (events) stage 3 of batch i before stage 2 of batch
 * i+2 and keeps heat_all alive until stage 3 has read it (jarvis_hybridnet_amd/distributed.py). */
int jh_predictor_stage_3d(jh_predictor* pr, const float* heat_all_dev, int t0, float* points_dev,
                          float* conf_dev, int32_t* valid_dev, void* stream);
/* Stage 2 fed directly from the all-gather of the per-rank detections (new design, no
 * reference line): det_gathered is (n_blocks, T, C / n_blocks, 3), block b = the det output of
 * the rank that owns cameras [b*C/n_blocks, (b+1)*C/n_blocks).  frames_u8 != 0: uint8 BGR
 * frames as for the *_u8 entry points.  n_blocks = 1 is jh_predictor_stage_keypoints[_u8]. */
int jh_predictor_stage_keypoints_gathered(jh_predictor* pr, const void* frames_dev, int frames_u8,
                                          const float* det_gathered_dev, int n_blocks,
                                          float* heat_dev, void* stream);
/* Stage 3 reading the heatmaps IN PLACE from the receive buffer of the camera-sharded
 * exchange (jarvis_hybridnet_amd/distributed.py; new design, no reference line): heat_blocks
 * is (n_blocks, frames_per_block, C / n_blocks, B/2, B/2, Jp) -- block b holds cameras
 * [b*C/n_blocks, (b+1)*C/n_blocks) as source rank b produced them -- and the T3 frames
 * t_off .. t_off+T3-1 of every block are the frames t0 .. t0+T3-1 of the batch.
 * n_blocks = 1, frames_per_block = T3, t_off = 0 is jh_predictor_stage_3d. */
int jh_predictor_stage_3d_blocks(jh_predictor* pr, const float* heat_blocks_dev, int n_blocks,
                                 int frames_per_block, int t_off, int t0, float* points_dev,
                                 float* conf_dev, int32_t* valid_dev, void* stream);
/* All three stages for cam_lo = 0, cam_n = num_cameras. */
int jh_predictor_forward(jh_predictor* pr, const float* frames_dev, float* points_dev,
                         float* conf_dev, int32_t* valid_dev, void* stream);
/* jh_predictor_forward[_u8] as ONE hipGraph launch.  The reference driver calls the predictor
 * with one frame set at a time (jarvis/prediction/predict3D.py:82-85); at that size the ~150
 * launches of a forward are launch-bound, so a predictor with time_batch == 1 captures its
 * forward on first use and replays the graph afterwards (the call's frame pointer goes through a
 * device cell, results are copied out of the predictor's buffers: any pointers may be passed on
 * every call, results are bit-identical to the plain launches).  Default: on for time_batch
 * == 1, off otherwise (environment JH_GRAPH=0 / 1 overrides for the process); this switches it
 * per predictor.  Not used while jh_profile_begin() is active or while the caller's stream is
 * itself being captured. */
int jh_predictor_set_graph_replay(jh_predictor* pr, int on);
int jh_predictor_graph_replay(const jh_predictor* pr);
/* how many times a whole-path forward of this predictor has been recorded so far (a first call of a form, a changed
 * description or calibration form, tone tables switched on or off): a call that replays adds none */
int64_t jh_predictor_graph_records(const jh_predictor* pr);
/* uint8 ingest (jarvis/prediction/predict3D.py:72-80): the
 * same three entry points for frames (T,cam_n,H,W,3) uint8 BGR exactly as the video
 * decoder delivers them.  The `.float().permute(0,3,1,2)[:, [2,1,0]] / 255.` of the
 * reference driver happens inside the resize / crop kernels, so the fp32 frame (4x the
 * bytes) is never materialised and only 1 byte per sample crosses PCIe. */
int jh_predictor_stage_center_u8(jh_predictor* pr, const uint8_t* frames_dev, float* det_dev,
                                 void* stream);
int jh_predictor_stage_keypoints_u8(jh_predictor* pr, const uint8_t* frames_dev,
                                    const float* det_all_dev, float* heat_dev, void* stream);
int jh_predictor_forward_u8(jh_predictor* pr, const uint8_t* frames_dev, float* points_dev,
                            float* conf_dev, int32_t* valid_dev, void* stream);

/* YUV 4:2:0 ingest (ABI v4, additive): frames as video decoders produce them natively, half the bytes of
 * uint8 BGR.  Each camera image is one contiguous (3H/2, W) uint8 buffer, H and W even:
 *   JH_FRAME_I420 (FFmpeg yuv420p): the Y plane (H, W), then U (H/2, W/2), then V (H/2, W/2);
 *   JH_FRAME_NV12 (hardware decoders): the Y plane, then one interleaved plane (H/2, W), U first.
 * frames (T,cam_n,3H/2,W).  Every pixel is converted to BGR bytes with the fixed-point BT.601 limited-range
 * arithmetic of OpenCV's cvtColor(COLOR_YUV2BGR_I420 / _NV12), chroma shared by each 2 x 2 block; those bytes
 * then take the uint8 path unchanged, so the result equals, bit for bit, jh_predictor_forward_u8 on the converted
 * frames.  The conversion runs inside the resize / crop kernels.  A graph-replaying predictor keeps one captured
 * graph per frame format.  JH_FRAME_RGB_F32 / JH_FRAME_BGR_U8 name the formats of the plain / _u8 entry points. */
#define JH_FRAME_RGB_F32 0
#define JH_FRAME_BGR_U8 1
#define JH_FRAME_I420 2
#define JH_FRAME_NV12 3
int jh_predictor_forward_yuv(jh_predictor* pr, const uint8_t* frames_dev, int format, float* points_dev,
                             float* conf_dev, int32_t* valid_dev, void* stream);

/* Described YUV 4:2:0 surfaces (ABI v4, additive): what decoders really hand out, read in place.  A jh_yuv_surface
 * says where the three planes of ONE image lie inside a buffer of `image_stride` bytes and how its colour is coded;
 * frames are (T,cam_n) such images back to back (the 2D predictor: (T)), image n = t * cam_n + c at byte
 * n * image_stride.  Pitched decoder surfaces (row pitch above the width, chroma after pitch * aligned height),
 * FFmpeg AVFrames copied plane by plane with their linesize, and the four plane orders are values of the fields:
 *   I420: u_offset < v_offset, c_step 1;   YV12: v_offset < u_offset, c_step 1;
 *   NV12: v_offset == u_offset + 1, c_step 2;   NV21: u_offset == v_offset + 1, c_step 2.
 * Bytes of an image that belong to no plane (pitch padding, rows between the planes, the gap up to image_stride) may
 * hold anything: they are never read.
 * Conversion: u = U - 128, v = V - 128, yy = max(0, Y - Y0) * CY + 2^19, then
 *   R = clamp8((yy + CVR v) >> 20), G = clamp8((yy + CVG v + CUG u) >> 20), B = clamp8((yy + CUB u) >> 20)
 * in int32, the chroma of pixel (y, x) that of block (y/2, x/2), with (Y0, CY, CVR, CUB, CUG, CVG) =
 *   BT.601 limited  (16, 1220542, 1673527, 2116026, -409993, -852492)   -- OpenCV's literals: the bits of _forward_yuv
 *   BT.601 full     ( 0, 1048576, 1470104, 1858077, -360853, -748826)
 *   BT.709 limited  (16, 1220945, 1879825, 2215014, -223607, -558796)
 *   BT.709 full     ( 0, 1048576, 1651297, 1945738, -196424, -490864)
 * (the last three: round(x * 2^20) of the real matrix, within 0.51 of it everywhere).  The bytes then take the
 * uint8 path unchanged: the result equals, bit for bit, jh_predictor_forward_u8 on the converted frames.
 * jh_yuv_surface_check (no GPU needed) is the validation every entry point applies: h, w even and positive;
 * c_step 1 or 2; y_pitch >= w, c_pitch >= (w/2) * c_step; offsets >= 0; for c_step 2, |u_offset - v_offset| == 1
 * with min(u_offset, v_offset) and c_pitch even; every plane ends at or before image_stride; matrix and range
 * known; sample a known code (below).  Returns 0, or nonzero with jh_last_error() set.
 * Samples wider than a byte (additive: the last word, `reserved` in earlier headers, is the sample code).
 * JH_SAMPLE_U8 = 0 is every description above.  JH_SAMPLE_U16(shift), shift 0 .. 8: every Y, U and V sample is a
 * little-endian 16-bit word and is reduced to a byte inside the fetch, byte = min(sample >> shift, 255); the
 * conversion above then runs on the bytes, so the result equals, bit for bit, that of the 8-bit description of the
 * reduced planes.  shift = bits - 8 is LSB-aligned data (yuv420p10le: 2, yuv420p12le: 4), shift = 8 MSB-aligned data
 * (P010 / P012 / P016).  Truncation, not rounding: what a decoder's own 8-bit output of the same stream is not
 * guaranteed to be, but what a shift on the host gives; gain and gamma are tables over that byte (jh_predictor_set_tone), and the network
 * never sees more than 8 bits.
 * Offsets and pitches stay in BYTES, c_step counts SAMPLES.  The rules for JH_SAMPLE_U16: every offset, pitch and
 * image_stride even (every 16-bit load is aligned); y_pitch >= 2 w; c_pitch >= (w/2) * c_step * 2; for c_step 2,
 * |u_offset - v_offset| == 2 with min(u_offset, v_offset) and c_pitch multiples of 4 (the pair is one 4-byte load
 * where the image base is a multiple of 4, two 2-byte loads otherwise); every plane's last BYTE lies before
 * image_stride.  The packed codes of jh_sensor_surface, and every other value, are refused.
 * jh_predictor_forward_surface: jh_predictor_forward_yuv through a description; mask_dev as in
 * jh_predictor_forward_masked, or NULL.  A graph-replaying predictor keeps one captured graph for this form (and
 * one for its masked form); a recording has one layout, so a call whose description differs from the recorded one
 * records again. */
#define JH_SAMPLE_U8 0
#define JH_SAMPLE_U16(shift) (0x100 | (shift))
#define JH_SAMPLE_P10 0x200
#define JH_SAMPLE_P12 0x300
#define JH_YUV_BT601 0
#define JH_YUV_BT709 1
#define JH_YUV_LIMITED 0
#define JH_YUV_FULL 1
typedef struct jh_yuv_surface {
  int64_t image_stride;        /* bytes from image n to image n+1 (n = t * cameras + c) */
  int64_t y_offset, y_pitch;   /* Y(y, x)  at y_offset + y * y_pitch + x */
  int64_t u_offset, v_offset;  /* U / V of block (y/2, x/2) at *_offset + (y/2) * c_pitch + (x/2) * c_step */
  int64_t c_pitch;
  int32_t c_step;              /* 1: planar (I420, YV12); 2: semi-planar (NV12, NV21) */
  int32_t matrix;              /* JH_YUV_BT601 = 0, JH_YUV_BT709 = 1 */
  int32_t range;               /* JH_YUV_LIMITED = 0, JH_YUV_FULL = 1 */
  int32_t sample;              /* JH_SAMPLE_U8 = 0 (the `reserved` word of earlier headers) or JH_SAMPLE_U16(shift) */
} jh_yuv_surface;
int jh_yuv_surface_check(const jh_yuv_surface* surface, int h, int w);
int jh_predictor_forward_surface(jh_predictor* pr, const uint8_t* frames_dev, const jh_yuv_surface* surface,
                                 const uint8_t* mask_dev, float* points_dev, float* conf_dev, int32_t* valid_dev,
                                 void* stream);

/* Raw sensor frames (ABI v4, additive): one byte per pixel as a machine-vision camera (GenICam Mono8, BayerRG8 and
 * its siblings) delivers it, a third of the bytes of uint8 BGR, demosaiced inside the resize / crop kernels.  A
 * jh_sensor_surface says where ONE h x w image lies inside `image_stride` bytes: raw(y, x) at
 * offset + y * pitch + x; frames are (T,cam_n) such images back to back (the 2D predictor: (T)).  Bytes that are no
 * sample (pitch padding, the bytes before `offset`, the gap up to image_stride) may hold anything: never read.
 * `pattern` names the top-left 2 x 2 cell:
 *   JH_SENSOR_MONO: one grey byte per pixel, R = G = B = the byte;
 *   JH_SENSOR_RGGB (R G / G B): red at (even y, even x);   JH_SENSOR_BGGR (B G / G R): blue at (even y, even x);
 *   JH_SENSOR_GRBG (G R / B G): red at (even y, odd x);    JH_SENSOR_GBRG (G B / R G): blue at (even y, odd x).
 * Bilinear demosaic, integer arithmetic.  Interior pixel (1 <= y <= h-2, 1 <= x <= w-2), N S E W and NW NE SW SE its
 * neighbouring bytes:
 *   at a red or blue site: its own colour is the byte, green = (N + S + E + W + 2) >> 2, the opposite colour
 *     = (NW + NE + SW + SE + 2) >> 2;
 *   at a green site: green is the byte, the colour whose samples lie left and right = (W + E + 1) >> 1, the colour
 *     whose samples lie above and below = (N + S + 1) >> 1.
 * A border pixel (y in {0, h-1} or x in {0, w-1}) takes the RGB of the interior pixel (clamp(y, 1, h-2),
 * clamp(x, 1, w-2)): clamp first, then demosaic, so no byte outside the h x w samples is addressed.  The
 * bytes are taken as the camera delivers them; black level, white balance and gamma are per-channel tables applied to
 * the demosaiced bytes (jh_predictor_set_tone), a colour-correction matrix is not offered.  The (R, G, B) bytes then
 * take the uint8 path unchanged: the result equals, bit for bit, jh_predictor_forward_u8 on the converted frames.
 * jh_sensor_surface_check (no GPU needed) is the validation every entry point applies: h, w positive; pattern
 * known; for a Bayer pattern h, w even and >= 4; pitch >= w; offset >= 0; offset + (h-1) * pitch + w <=
 * image_stride; sample a known code (below).  Returns 0, or nonzero with jh_last_error() set.
 * Samples wider than a byte (additive: the fifth word, `reserved` in earlier headers, is the sample code; pitch,
 * offset and image_stride stay in bytes).  A sample is reduced to a byte inside the fetch, byte = min(sample >> shift,
 * 255) -- the truncation a camera applies when its PixelFormat is switched from Mono12 to Mono8 --, and the bytes go
 * the way described above: the result equals, bit for bit, that of the 8-bit description of the reduced bytes.
 * Rounding instead of truncation and more than 8 bits for the network are not offered; gain, black level, gamma and
 * white balance are tables over the reduced byte (jh_predictor_set_tone).
 *   JH_SAMPLE_U8 = 0: one byte per sample, every description above.
 *   JH_SAMPLE_U16(shift), shift 0 .. 8: raw(y, x) is the little-endian 16-bit word at offset + y * pitch + 2 x.
 *     shift = bits - 8 is LSB-aligned data (Mono10 / 12 / 14 / 16, BayerXX10 / 12 / 16), shift = 8 MSB-aligned data;
 *     a sample with bits above the declared depth saturates to 255.  offset, pitch and image_stride are even.
 *   JH_SAMPLE_P10 / JH_SAMPLE_P12: GenICam PFNC 10p / 12p (Mono10p, Mono12p, BayerRG12p ...).  Every row is a
 *     little-endian bit stream that starts at offset + y * pitch, at any byte; sample x occupies bits
 *     [n x, n x + n) of it and the byte is its top 8 bits, bits [n x + n - 8, n x + n).  The unused high bits of a
 *     row's last byte may hold anything.  The legacy GigE Vision Mono12Packed / Mono10Packed nibble order is ANOTHER
 *     layout and has no code: unpack it first.
 * With row_bytes(w) = w, 2 w, ceil(10 w / 8), ceil(12 w / 8): pitch >= row_bytes(w) and offset + (h-1) * pitch +
 * row_bytes(w) <= image_stride.  Every other value of `sample` is refused.
 * Per-image pointers (jh_predictor_forward_images and its like): an image of a JH_SAMPLE_U16 description, sensor or
 * YUV, must be 2-byte aligned -- checked on the host as the 4-byte rule of fp32 images is: nothing is enqueued and
 * jh_last_error() names the image; packed and 8-bit images may start anywhere.
 * jh_predictor_forward_sensor: mask_dev as in jh_predictor_forward_masked, or NULL; jh_predictor_views2d follows it
 * as it follows any forward.  A graph-replaying predictor keeps one captured graph for this form (and one for its
 * masked form); a call whose description differs from the recorded one records again. */
#define JH_SENSOR_MONO 0
#define JH_SENSOR_RGGB 1
#define JH_SENSOR_BGGR 2
#define JH_SENSOR_GRBG 3
#define JH_SENSOR_GBRG 4
typedef struct jh_sensor_surface {
  int64_t image_stride;        /* bytes from image n to image n+1 (n = t * cameras + c) */
  int64_t offset, pitch;       /* raw(y, x) at offset + y * pitch + x */
  int32_t pattern;             /* JH_SENSOR_* */
  int32_t sample;              /* JH_SAMPLE_* (the `reserved` word of earlier headers): 0 = one byte per sample */
} jh_sensor_surface;
int jh_sensor_surface_check(const jh_sensor_surface* surface, int h, int w);
int jh_predictor_forward_sensor(jh_predictor* pr, const uint8_t* frames_dev, const jh_sensor_surface* surface,
                                const uint8_t* mask_dev, float* points_dev, float* conf_dev, int32_t* valid_dev,
                                void* stream);

/* Integer path of the last call, for parity tests: center3d float (T,3),
 * center3d int (T,3), center_hm (T,C,2), det (T,C,3).  Any pointer may be NULL.
 * After a call from caller-supplied centres (jh_predictor_set_centers): center3d is the supplied centre, the integers
 * and crop centres are derived from it, and det is what the last DETECTED call wrote. */
int jh_predictor_debug(jh_predictor* pr, float* center3d_f_dev, int32_t* center3d_i_dev,
                       int32_t* center_hm_dev, float* det_dev, void* stream);

/* Per-frame camera masks (ABI v4, additive).  mask_dev: (T, num_cameras) bytes on the device, nonzero = the
 * camera takes part in frame t; NULL = all cameras, i.e. exactly the unmasked entry point.  Frame t is computed
 * as the reference computes it for the cameras with mask[t][c] != 0 alone, in their original order (its
 * `cameras_to_use` subset, utils/reprojection.py): a masked camera adds nothing to the triangulation, is not
 * counted among the detecting cameras, and is left out of the mean over cameras of the voxel grid, which divides
 * by the number of unmasked cameras.  valid[t] = 0 when fewer than two unmasked cameras detect (maxval > 50).
 * The frame slot of a masked camera may hold anything (stale bytes, NaN): its 2D networks still run, per image,
 * and nothing of them reaches a result.
 * jh_predictor_forward_masked: jh_predictor_forward / _u8 / _yuv by format code (JH_FRAME_*).  The mask is copied
 * into a buffer the predictor owns (T * num_cameras bytes, beside two T-int32 count buffers), so the caller's buffer
 * is free once the stream has passed the call, and a graph-replaying predictor keeps replaying: it captures one
 * further graph per frame format for the masked form.
 * The staged pair, for cam_lo = 0, cam_n = num_cameras (what the masked forward runs between stage 1, which has no
 * camera sum, and the results): jh_predictor_stage_keypoints_masked is jh_predictor_stage_keypoints / _u8 by format
 * code (JH_FRAME_RGB_F32 / JH_FRAME_BGR_U8) with the masked triangulation -- it decides valid[] and the centres --
 * and jh_predictor_stage_3d_masked is jh_predictor_stage_3d with the masked gather (rows t0 .. t0+T3-1 of the
 * mask).  Give both the SAME mask: stage 3 after an unmasked stage 2 would average other cameras than the centre
 * was triangulated from.  These two read mask_dev in place: keep it alive and unchanged until the stream has
 * passed the call. */
int jh_predictor_forward_masked(jh_predictor* pr, const void* frames_dev, int format, const uint8_t* mask_dev,
                                float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);
int jh_predictor_stage_keypoints_masked(jh_predictor* pr, const void* frames_dev, int format,
                                        const float* det_all_dev, const uint8_t* mask_dev, float* heat_dev,
                                        void* stream);
int jh_predictor_stage_3d_masked(jh_predictor* pr, const float* heat_all_dev, int t0, const uint8_t* mask_dev,
                                 float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);
/* Counts of the last MASKED forward / masked stage 2, for parity tests: n_active (T) int32 = unmasked cameras per frame (the
 * divisor of the mean over cameras), num_cams_detect (T) int32 = those of them with maxval > 50.  Any pointer may
 * be NULL.  Unmasked calls do not update them. */
int jh_predictor_debug_mask(jh_predictor* pr, int32_t* n_active_dev, int32_t* num_cams_detect_dev, void* stream);

/* Per-camera 2D views of a 3D result (ABI v4, additive; new design: the reference gets 2D keypoints only from a
 * second pass over every video, JarvisPredictor2D, jarvis/prediction/jarvis2D.py).  For the frames t0 .. t0+T3-1
 * whose 3D result is points_dev (T3,J,3): call after the forward / stage-3 call that produced it, on the same stream.
 * heat_all_dev NULL = the heat maps of the last whole-path forward (the predictor's own buffer; all cameras local);
 * otherwise (T3,C,B/2,B/2,Jp) as for jh_predictor_stage_3d.  mask_dev: the (T,C) mask that forward was given (rows
 * t0 .. t0+T3-1 are read, in place: keep it alive until the stream has passed the call), or NULL.  Reads the crop
 * centres / validity set that stage 3 read.  Outputs, with m the flat index y*(B/2) + x of the maximum of joint j's
 * heat map (the lowest index among equal maxima, as torch.argmax on the CPU):
 *   used (T3,C) uint8        valid[t] && (mask == NULL || mask[t][c] != 0)
 *   points2d (T3,C,J,2) int32  (m % (B/2), m / (B/2)) * 2 + centerHM[t][c] - B/2: full-frame pixels (jarvis2D.py:143-149,
 *                            the expression of jh_predictor2d_forward); -1 for a camera that is not used
 *   conf2d (T3,C,J)          min(max, 255) / 255 (jarvis2D.py:147-148); 0 for a camera that is not used
 *   reproj (T3,C,J,2)        ReprojectionTool.reprojectPoint of points[t][j] in camera c (utils/reprojection.py:49-61),
 *                            the bits of jh_reproject_point, for EVERY camera of a valid frame -- a masked camera's
 *                            calibration is known: where the joint should be in the camera that dropped the frame --;
 *                            NaN for a frame that is not valid
 *   err (T3,C,J)             sqrt(dx*dx + dy*dy), dx = u - (float)x2d, dy = v - (float)y2d, each operation rounded
 *                            once in fp32; NaN for a camera that is not used
 * Nothing of the heat map of a camera that is not used reaches an output (it may hold anything).
 * These are HybridNet's own 2D detections, on the crop around the projection of the TRIANGULATED centre;
 * JarvisPredictor2D crops around each camera's own centre detection.  The two agree wherever the crops cover the
 * subject; they are not bit-equal.
 * The (max, index) workspace of the scan is allocated by the first call of a predictor -- never by
 * jh_predictor_create, so jh_predictor_device_bytes and the memory of a predictor that never asks for 2D views are
 * unchanged -- and that first call must not be made inside a stream capture.  Plain launches, also on a
 * graph-replaying predictor: the call runs behind the replay and the captured graphs are untouched. */
int jh_predictor_views2d(jh_predictor* pr, const float* heat_all_dev, int t0, const float* points_dev,
                         const uint8_t* mask_dev, int32_t* points2d_dev, float* conf2d_dev, float* reproj_dev,
                         float* err_dev, uint8_t* used_dev, void* stream);

/* Per-joint 3D spread (ABI v4, additive; new design: the reference computes the mean of the normalised heat map and
 * throws the rest away, hybridnet/model.py:73-88).  For frame set t and joint j, with x the V2V output on the Gh^3
 * half grid, voxel (i, j, k) at flat index p = (i * Gh + j) * Gh + k, h = softplus(x) the weight the soft-argmax uses,
 * S_0 = sum h, S_a = sum h * a, S_ab = sum h * a * b over a, b in (i, j, k), and s = 2 * grid_spacing:
 *   mass (T,J)     S_0, the normaliser, from the fp64 sum rounded once (the float the points are divided by is the
 *                  same sum from fp32 block sums: it agrees with mass to that summation's error, not to the bit)
 *   cov (T,J,6)    cov_ab = (S_ab / S_0 - (S_a / S_0)(S_b / S_0)) * s^2 in mm^2, order xx, xy, xz, yy, yz, zz, the
 *                  axes those of points[..., 0..2]; the ten sums are accumulated in fp64 (every product h * a * b is
 *                  exact there) and added across workgroups order-independently, the expression is evaluated in fp64
 *                  and rounded once: bit-reproducible from run to run
 *   peak (T,J,3)   the voxel of the maximum of x -- of x, not of h: softplus is monotone and float ties of h would
 *                  hide the index --, the lowest flat index among equal maxima, in millimetres by the points' own
 *                  expression idx * grid_spacing * 2 - roi_cube_size / 2 + center3d with the integer voxel index as
 *                  idx.  A joint whose peak and point disagree by more than the spread has a multi-modal map.
 * jh_softargmax_spread: jh_softargmax with these three outputs; points and conf have the bits of jh_softargmax on
 * the same input.  workspace_dev: >= jh_softargmax_spread_workspace_bytes(t, joints, gh) bytes.
 * jh_predictor_set_spread(pr, on): from the next call on, the 3D stage of every entry point (the whole-path forwards,
 * jh_predictor_stage_3d / _blocks / _masked, jh_predictor_hybridnet_forward) runs the spread form of the tail and
 * writes rows t0 .. t0+T3-1 of the predictor's own (T,J,6), (T,J,3) and (T,J) buffers; points, conf and valid keep
 * the bits they have with it off.  The buffers are allocated by the first enabling call -- never by
 * jh_predictor_create, so jh_predictor_device_bytes, the memory and the launches of a predictor that never asks are
 * unchanged; jh_predictor_device_bytes grows by them -- and that first call must not be made inside a stream capture.
 * A graph-replaying predictor records the spread form in graph slots of its own: alternating calls with the spread on
 * and off never re-record.
 * jh_predictor_get_spread: the three buffers copied out (any pointer may be NULL), after a forward / stage-3 call, on
 * the same stream.  Rows of a frame set that is not valid are NaN in all three. */
int64_t jh_softargmax_spread_workspace_bytes(int t, int joints, int gh);
int jh_softargmax_spread(const float* v2v_out_dev, int t, int joints, int gh, float grid_spacing,
                         float roi_cube_size, const int32_t* center3d_dev, float* heatmap_final_dev,
                         float* points_dev, float* conf_dev, float* cov_dev, float* peak_dev, float* mass_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream);
int jh_predictor_set_spread(jh_predictor* pr, int on);
int jh_predictor_get_spread(jh_predictor* pr, float* cov_dev, float* peak_dev, float* mass_dev, void* stream);
/* The V2V output of the last 3D chunk, for parity tests: out (T3,J,Gh,Gh,Gh) NCDHW -- what jh_softargmax_spread
 * takes. */
int jh_predictor_debug_v2v(jh_predictor* pr, float* out_dev, void* stream);

/* Per-image frame pointers (ABI v4, additive): every camera's buffer read where its producer left it.  The entry
 * points above take ONE base pointer with all T * num_cameras images at one constant distance; twelve decoder sessions
 * or frame-grabber rings deliver twelve unrelated device pointers.  Here a call says where EACH image is.
 * images_host: a HOST array of n_images = T * num_cameras device pointers (the 2D predictor: T), index t * C + c, each
 * pointing at ONE image in the layout `format` gives a single image:
 *   JH_FRAME_RGB_F32 (3,H,W) fp32, 4-byte aligned;   JH_FRAME_BGR_U8 (H,W,3) uint8;
 *   JH_FRAME_I420 / JH_FRAME_NV12 (3H/2,W) uint8;
 *   JH_FRAME_SURFACE: one image of the jh_yuv_surface `yuv`;   JH_FRAME_SENSOR: one image of the jh_sensor_surface
 *   `sensor`.  Give exactly the description the format needs and NULL for the other (both NULL for the first four).
 *   Of a description, image_stride keeps only its role as the extent every plane must end within.
 * The byte forms may start at ANY address.  The one wider load of the fetch, the 2-byte chroma pair of NV12 and of
 * semi-planar surfaces, is taken from an image at an even address; an image at an odd address reads the pair as two
 * bytes (the kernels test the image's own pointer; nothing is demanded of the caller).
 * Duplicate pointers are allowed.  Every entry, a masked camera's too, points at readable memory of one image: its 2D
 * networks run, per image, and nothing of them reaches a result.
 * The array is free again when the call returns: the pointers travel as kernel arguments (chunks of up to 256) into a
 * table the predictor owns, on `stream` -- no staging buffer, no host synchronisation.  The launches read that table,
 * so a graph-replaying predictor keeps replaying ONE recording per format while the pointers change from call to
 * call.  The per-image form has graph slots of its OWN (per format, unmasked and masked): per-image and contiguous
 * calls of one format may alternate freely and never re-record each other; as everywhere, a described call whose
 * description differs from the recorded one records again.  Like the mask buffer the table belongs to the predictor:
 * calls of one predictor go to one stream, or are ordered by the caller.
 * The table (n_images pointers) is allocated by the first such call of a predictor -- never by *_create, so
 * jh_predictor_device_bytes and the memory of a predictor that never uses it are unchanged -- and that first call
 * must not be made inside a stream capture.
 * Validation (non-zero with jh_last_error() set, nothing enqueued): n_images == T * num_cameras (2D: T); no NULL
 * entry; fp32 images 4-byte aligned; exactly the description the format needs; the description passes
 * jh_yuv_surface_check / jh_sensor_surface_check.
 * Results: bit for bit those of the contiguous entry point of the format on the same images.  mask_dev as in
 * jh_predictor_forward_masked, or NULL; jh_predictor_views2d follows the call as it follows any forward.
 * Whole-path forwards only: the staged entry points (jh_predictor_stage_*) take one base pointer. */
#define JH_FRAME_SURFACE  4   /* needs yuv    */
#define JH_FRAME_SENSOR   5   /* needs sensor */
int jh_predictor_forward_images(jh_predictor* pr, const void* const* images_host, int n_images, int format,
                                const jh_yuv_surface* yuv, const jh_sensor_surface* sensor, const uint8_t* mask_dev,
                                float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);

/* Several subjects in one frame set (ABI v4, additive; new design: the reference keeps ONE maximum per camera and puts
 * every camera's maximum into one triangulation, jarvis3D.py:147-160).  Stage 1 as it stands finds the strongest subject;
 * if the cameras disagree about which one that is, or one camera's maximum sits on a reflection, the one weighted DLT
 * averages rays to different things.  Here the top few local maxima of every camera's centre heat map are kept, grouped
 * across cameras by reprojection consistency, and each group is triangulated with the arithmetic of the existing
 * triangulation.  A centre goes back in through jh_predictor_set_centers; robust single-subject detection is
 * max_subjects = 1.
 *
 * jh_subjects_params.  Library defaults -- documented values, not recommendations: what suits a rig depends on its
 * pixel scale and on what its CenterDetect emits -- are min_peak = 50 (the reference's `> 50` gate), nms_radius = 4,
 * min_views = 2, max_error_px = 24.  Ranges, checked by every entry point below (non-zero with jh_last_error() set,
 * nothing enqueued): max_subjects 1 .. 8, max_peaks 1 .. 8, nms_radius 1 .. 16, min_views >= 2, min_peak a number below
 * +inf (-inf allowed), max_error_px >= 0 (+inf allowed).
 *
 * jh_op_center_peaks: heat (n,hh,wh,cp) channel-last dev, channel 0 -- what the centre arg-max reads -- -> peaks
 * (n,max_peaks,3) = (x, y, value), count (n) int32.  With v(p) the value at flat index p = y*wh + x: p is a PEAK iff
 * v(p) > min_peak and no q != p of the window |dx| <= nms_radius, |dy| <= nms_radius, clipped at the map's edge, has
 * v(q) > v(p) or (v(q) == v(p) and q < p): of a plateau only the lowest index survives; NaN is never a peak and never
 * suppresses one.  The peaks of an image are ordered by (value descending, index ascending) and the first max_peaks
 * kept, as x = p % hh, y = p / wh (the arg-max's expression); empty slots are (-1, -1, -inf).  Slot 0 with min_peak =
 * -inf is therefore the centre arg-max (jh_predictor_debug's det) bit for bit for any map that holds a value above -inf.
 * One workgroup per image; a map up to 160 x 160 is read from memory once and held in LDS, a larger one takes a
 * global-memory form of the same passes (scratch from hipMalloc: unit-test helper, synchronises).
 *
 * jh_op_associate_subjects: peaks (t,cams,max_peaks,3) dev as above, one calibration (calib_per_frame == 0: (cams,..))
 * or one per frame set (!= 0: (t,cams,..)), mask (t,cams) bytes or NULL; sx2, sy2: full-frame pixels per heat-map pixel
 * (a peak lies at (x*sx2, y*sy2)).  A slot takes part iff its camera is unmasked and x >= 0 and y >= 0; a masked
 * camera's slots are never read and may be NaN.  For round k = 0 .. max_subjects-1:
 *   candidates  every (a, i, b, j), cameras a < b, unused slots i of a and j of b: X = the weighted DLT of the existing
 *               triangulation (weights value / 255) over exactly those two observations;
 *   support     per camera with an unused slot, the unused peak nearest to reprojectPoint(X), d = sqrt(dx*dx + dy*dy),
 *               one fp32 rounding per operation, ties to the lowest slot; the camera supports iff the homogeneous depth
 *               of the projection is > 0 and d <= max_error_px (a NaN d never supports); views = supporting cameras,
 *               cost = the fp32 sum of their d in camera order;
 *   choice      largest views, then smallest cost, then lowest (a, i, b, j); views < min_views: this and all later
 *               subjects are empty;
 *   subject k   members[k][c] = the supporting slot of camera c or -1; centers[k] = the triangulation over the member
 *               observations, BIT FOR BIT jh_reconstruct_point on the members' pixels and value / 255; error[k] = the
 *               mean over the members of d against the projection of centers[k]; the members' slots become used.
 * -> centers (t,max_subjects,3) world mm, NaN for an empty subject (an invalid row for jh_predictor_set_centers), views
 * (t,max_subjects) int32 (0), members (t,max_subjects,cams) int32 (-1), error (t,max_subjects) px (NaN).  The result
 * does not depend on timing.  cams <= 64.  The work of a frame set grows with cams^2 * max_peaks^2 per round: it is
 * meant for cams * max_peaks up to a few hundred.  Synchronises (unit-test helper).
 *
 * jh_predictor_detect_subjects: stage 1 of the call's frames up to CenterDetect's heat map (resize or fused stem, the
 * CenterDetect plan), then the two kernels in place of the arg-max and the triangulation, under the calibration in
 * force (shared or per frame set).  Frames: exactly one of frames_dev (contiguous, as the forward of `format` takes
 * them) and images_host + n_images (per-image pointers, as jh_predictor_forward_images); format any JH_FRAME_*, with yuv
 * / sensor exactly where the format needs one.  mask_dev (T,C) or NULL: read in place, keep it alive until the stream
 * has passed the call.  peaks_dev (T,C,max_peaks,3) optional (NULL to skip).  sx2, sy2 are the predictor's
 * 2 * img_w / center_size and 2 * img_h / center_size.
 * Plain launches, asynchronous, also on a graph-replaying predictor: the captured graphs, det, the centres set by
 * jh_predictor_set_centers and whether they are in force, the mask buffer and the spread state are not touched, so the
 * forwards before and after keep their bits.  The workspace (peaks and counts, and the global-form scratch of a map
 * that does not fit the LDS) is allocated by the first such call of a predictor -- never by jh_predictor_create, so
 * jh_predictor_device_bytes, the memory and the launches of a predictor that never asks are unchanged -- and that first
 * call must not be made inside a stream capture.  Needs CenterDetect weights and all cameras local; otherwise, and for
 * parameters out of range, non-zero with jh_last_error() set and nothing enqueued.
 * Subject k of one call and subject k of the next are unrelated; jh_op_track_subjects below gives them an identity. */
typedef struct jh_subjects_params {
  int32_t max_subjects, max_peaks, nms_radius, min_views;
  float min_peak, max_error_px;
} jh_subjects_params;
int jh_subjects_params_check(const jh_subjects_params* params);    /* no GPU needed */
int jh_op_center_peaks(const float* heat_dev, int n, int hh, int wh, int cp, const jh_subjects_params* params,
                       float* peaks_dev, int32_t* count_dev, void* stream);
int jh_op_associate_subjects(const float* peaks_dev, int t, int cams, const float* cam_dev, const float* intr_dev,
                             const float* dist_dev, int calib_per_frame, const uint8_t* mask_dev, float sx2, float sy2,
                             const jh_subjects_params* params, float* centers_dev, int32_t* views_dev,
                             int32_t* members_dev, float* error_dev, void* stream);
int jh_predictor_detect_subjects(jh_predictor* pr, const void* frames_dev, const void* const* images_host, int n_images,
                                 int format, const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                 const uint8_t* mask_dev, const jh_subjects_params* params, float* centers_dev,
                                 int32_t* views_dev, int32_t* members_dev, float* error_dev,
                                 float* peaks_dev /* optional */, void* stream);

/* Subject identity across frame sets (ABI v4, additive; new design: the reference follows one animal).  The rows of
 * jh_predictor_detect_subjects are ordered inside one frame set, so two animals swap rows whenever their view counts or
 * costs swap.  Here up to eight TRACKS live in caller-owned device memory (jh_track_state); the detections of every
 * frame set are matched to them greedily, nearest first, and come out again in SLOT order: slot k of frame set t and of
 * t+1 is the same track, and ids[t][k] names it for the whole run.  Everything happens on the device: no host
 * synchronisation per frame set.
 *
 * jh_track_params.  max_subjects = K, 1 .. 8: the slots in use, and the detections per frame set.  max_missed >= 0: the
 * frame sets a track may go unmatched and still keep its identity.  predict 0: a track is matched against its last
 * position; 1: against last position + velocity * frame sets elapsed.  coast 1: the output centre of an unmatched live
 * track is its predicted position; 0: NaN.  max_jump_mm > 0 (+inf allowed, NaN refused): the gate per elapsed frame set.
 * predict and coast are 0 or 1.  There are no defaults on this side; max_jump_mm is the rig's.  Checked by
 * jh_track_params_check (no GPU needed) and by jh_op_track_subjects: non-zero with jh_last_error() set, nothing enqueued.
 *
 * jh_track_state: device memory owned by the caller, 272 bytes; jh_op_track_subjects touches no slot >= K.
 * missed[k] = -1: slot k is free (id -1, pos = vel = 0); >= 0: the frame sets since the track's last match.
 * jh_op_track_reset makes all eight slots free, next_id 0, every float and reserved word 0.
 *
 * jh_op_track_subjects: centers (t,K,3), views (t,K) int32, members (t,K,cams) int32, error (t,K) dev: the four tensors
 * jh_predictor_detect_subjects writes.  views / members / error may be NULL together; views_out / members_out /
 * error_out are then NULL too.  Outputs must not alias inputs.  The frame sets of a call are consecutive in time and
 * processed in ascending t; the state carries over from call to call, so one call of t frame sets and t calls of one give
 * the same bits.  For each frame set:
 *   1 live, prediction   slot k is live iff missed[k] >= 0.  With predict, p_k = pos_k + vel_k * (float)(missed_k + 1),
 *                        one fp32 multiply and one add per component; without, p_k = pos_k.
 *   2 present            detection i is present iff its three centre components are finite.
 *   3 distance, gate     d(k,i) = sqrt(dx*dx + dy*dy + dz*dz), dx = p_k.x - c_i.x and so on, one fp32 rounding per
 *                        operation, the sum left to right.  The pair of a live slot and a present detection is eligible
 *                        iff d <= max_jump_mm * (float)(missed_k + 1) (one fp32 multiply); a NaN d is never eligible.
 *   4 greedy match       among the eligible pairs whose slot and detection are both unassigned, the smallest d, ties to
 *                        the lowest k, then the lowest i; assign it; repeat until none is left.
 *   5 matched slot       vel = predict ? (c_i - pos) / (float)(missed + 1) : 0 (one fp32 subtract and one divide per
 *                        component), then pos = c_i, missed = 0.
 *   6 unmatched live     missed += 1; if missed > max_missed the slot becomes free: missed = -1, id = -1, pos = vel = 0.
 *   7 births             the unmatched present detections in ascending i each take the lowest free slot (one freed in
 *                        step 6 of this frame set counts): id = next_id++, pos = c_i, vel = 0, missed = 0.  With no free
 *                        slot the detection is dropped and dropped[t] counts it.
 *   8 row (t,k)          slots: the detection the slot holds in this frame set, or -1.  ids, missed: the slot's values
 *                        after the frame set (-1 when free).  centers_out: c_i bit for bit; for a live unmatched slot
 *                        with coast, pos + vel * (float)missed (pos when predict == 0); otherwise NaN.  views_out: the
 *                        detection's views, or 0.  members_out: its members row, or all -1.  error_out: its error, or
 *                        NaN.
 * -> centers_out (t,K,3), views_out (t,K), members_out (t,K,cams), error_out (t,K), ids / slots / missed (t,K) int32,
 * dropped (t) int32.  A row of centers_out goes into jh_predictor_set_centers as a row of centers does.
 * Asynchronous: one launch of one 64-lane wave on `stream`, no synchronisation, nothing allocated, legal inside a stream
 * capture; calls on one state must be ordered by the caller (one stream, or events).  The result does not depend on
 * timing.  The time of a call is the latency of t * K dependent wave steps.
 * Out of scope: the optimal (min-sum) assignment -- the match is greedy --, eviction of a coasting track in favour of
 * a new detection, more than eight slots, and several trackers per launch. */
typedef struct jh_track_params {
  int32_t max_subjects;   /* K, 1 .. 8 */
  int32_t max_missed;     /* >= 0: frame sets a track may go unmatched and still keep its identity */
  int32_t predict;        /* 0: match against the last position; 1: against last position + velocity * frames elapsed */
  int32_t coast;          /* 1: an unmatched live track's output centre is its predicted position, 0: NaN */
  float   max_jump_mm;    /* > 0, +inf allowed, NaN refused: the gate per elapsed frame set */
} jh_track_params;

typedef struct jh_track_state {      /* device memory owned by the caller; slots >= K are never touched */
  float pos[8][3], vel[8][3];
  int32_t missed[8];                 /* -1: free slot; >= 0: frame sets since the last match */
  int32_t id[8];                     /* identity of the slot's track, -1 when free */
  int32_t next_id, reserved[3];
} jh_track_state;

int jh_track_params_check(const jh_track_params* params);          /* no GPU needed */
int jh_op_track_reset(jh_track_state* state_dev, void* stream);    /* all slots free, next_id 0, floats 0 */
int jh_op_track_subjects(const float* centers_dev, const int32_t* views_dev, const int32_t* members_dev,
                         const float* error_dev, int t, int cams, const jh_track_params* params,
                         jh_track_state* state_dev,
                         float* centers_out, int32_t* views_out, int32_t* members_out, float* error_out,
                         int32_t* ids_out, int32_t* slots_out, int32_t* missed_out, int32_t* dropped_out,
                         void* stream);

/* Per-joint robust triangulation (ABI v4, additive; new design: the reference's only 3D keypoints are V2V's).  A
 * classical 3D point per joint, triangulated from the cameras' own 2D keypoints with the cameras that disagree left out:
 * the one 3D estimate that does not pass through the voxel cube.  It still meets the rays of a limb that has left
 * roi_cube_size (V2V's soft-argmax saturates at the cube face), it names the camera whose keypoint sits on a reflection
 * or an occluder (the reprojection layer's camera mean is dragged by it), and it is a check on V2V that is independent
 * of V2V (err of jh_predictor_views2d is measured against V2V's own point).
 *
 * jh_joints3d_params.  Library defaults -- documented values, not recommendations -- are min_views = 2, refine_radius =
 * 1, min_conf = 0.1, max_error_px = 8.  Ranges, checked by every entry point below (non-zero with jh_last_error() set,
 * nothing enqueued; jh_joints3d_params_check needs no GPU): min_views >= 2, refine_radius 0 .. 3, min_conf 0 .. 1,
 * max_error_px >= 0 (+inf allowed); a NaN is out of range.
 *
 * Observation of joint j in camera c of frame set t: used[t][c], points2d = (x2d, y2d) and conf2d exactly as
 * jh_predictor_views2d defines them, the sub-pixel offset (ox, oy) of the peak, and the weight w = conf2d.  Its pixel is
 *   u = (float)x2d + 2 * ox,  v = (float)y2d + 2 * oy      (the product is exact, the sum rounded once in fp32).
 * It is USABLE iff used[t][c] is set, w > 0 and w >= min_conf, and u and v are finite.
 * Sub-pixel offset, refine_radius = r > 0: m the arg-max index of joint j's map, (mx, my) its column and row by the
 * expression of jh_predictor_views2d for the predictor's square maps, (m % (B/2), m / (B/2)) (jh_op_joint_peaks_refine
 * on an hh x wh map: mx = m % wh, my = m / wh).  Over the window |x - mx| <= r, |y - my| <= r clipped at the map's edge,
 * walked y ascending, then x ascending, with h the heat value at (x, y) and wgt = fmaxf(h, 0) (a NaN pixel counts as 0):
 *   S0 = sum wgt,  Sx = sum wgt * (x - mx),  Sy = sum wgt * (y - my),
 * every product and every sum rounded once in fp32, in walk order, starting from 0;  ox = S0 > 0 ? Sx / S0 : 0,  oy = S0 >
 * 0 ? Sy / S0 : 0  (one fp32 division each): the centroid of the window, in heat-map pixels, |ox|, |oy| <= r.  An index m
 * outside the map (a map without any number has no arg-max) reads nothing and has offset 0.  r = 0: the heat map is not
 * read again, ox = oy = 0, and (u, v) are the integers converted.
 *
 * Consensus per (t, j): the association of jh_op_associate_subjects with one slot per camera and one round.
 *   candidates  every pair of usable cameras a < b: X = the weighted DLT of the existing triangulation over exactly those
 *               two observations -- pixel (u, v) as given (no scaling), weight w (no division);
 *   support     a usable camera c supports X iff the homogeneous depth of the projection of X in c is > 0 and d =
 *               sqrt(dx*dx + dy*dy) <= max_error_px, dx and dy the differences between reprojectPoint(X) and (u, v), one
 *               fp32 rounding per operation (a NaN d never supports); views = the number of supporting cameras, cost =
 *               the fp32 sum of their d in camera order;
 *   choice      most views, then smallest cost, then lowest (a, b);
 *   empty       no pair, or views < min_views: the joint is empty;
 *   result      members[t][j][c] uint8 = 1 for a supporting camera, else 0; views[t][j] int32; points[t][j] = the
 *               triangulation over the members' observations, A^T A summed in camera order, BIT FOR BIT
 *               jh_reconstruct_point on the members' pixels (u, v) and weights w; error[t][j] = the fp32 mean (sum in
 *               camera order, one division by views) over the members of d against the projection of points[t][j].
 * An empty joint, and every joint of a frame set that is not valid: points and error NaN, views 0, members 0.
 * The result does not depend on timing.  Two consequences:
 *   - with max_error_px = +inf, min_conf = 0 and min_views = 2 the members of a joint with a pair are all usable cameras
 *     in front of which the chosen pair's point lies; the point is then jh_reconstruct_point over them;
 *   - nothing of the heat map of a camera that is not used reaches an output (it may hold anything).
 *
 * jh_op_joint_peaks_refine: heat (n,hh,wh,jp) channel-last dev, idx (n,j) int32 flat indices y*wh + x (what
 * jh_op_joint_argmax_all writes) -> offsets (n,j,2) = (ox, oy) as above for radius 0 .. 3 (0: all zero).  At most
 * (2 radius + 1)^2 values are read per (n, j).  Synchronises (unit-test helper).
 * jh_op_triangulate_joints: obs (t,cams,j,3) = (u, v, w) dev, a camera that is not used as (NaN, NaN, 0); one
 * calibration (calib_per_frame == 0: (cams,..)) or one per frame set (!= 0: (t,cams,..)); params->refine_radius is
 * checked and not used -> points (t,j,3), views (t,j) int32, members (t,j,cams) uint8, error (t,j).  cams <= 64; the
 * work of a joint grows with cams^3.  Synchronises (unit-test helper).
 * jh_predictor_triangulate_joints: for the frames t0 .. t0+T3-1, after the forward / stage-3 call, on the same stream,
 * with the conventions of jh_predictor_views2d: heat_all_dev NULL = the heat maps of the last whole-path forward (all
 * cameras local), otherwise (T3,C,B/2,B/2,Jp); mask_dev the (T,C) mask that forward was given, read in place, or NULL;
 * the crop centres / validity set that stage 3 read; the calibration in force, shared or per frame set.  Outputs points
 * (T3,J,3) world mm, views (T3,J), members (T3,J,C), error (T3,J) px, and obs_dev (T3,C,J,3) optional (NULL to skip): the
 * observations (u, v, w), (NaN, NaN, 0) for a camera that is not used.  With refine_radius = 0 the observations are
 * points2d converted and conf2d of jh_predictor_views2d, bit for bit.
 * Plain launches, asynchronous, also on a graph-replaying predictor: the call runs behind the replay and the captured
 * graphs are untouched: the scan, the observations -- written straight into obs_dev when it is given, into a buffer of
 * the predictor's own otherwise -- and the consensus, three launches and no copy.  The scan's (max, index) workspace is
 * shared with jh_predictor_views2d: a later views2d call runs its own scan again.  Workspace and buffer
 * are allocated by the first call that needs them -- never by jh_predictor_create, so jh_predictor_device_bytes,
 * the memory, the launches and the bits of a predictor that never asks are unchanged -- and that first call must not be
 * made inside a stream capture. */
typedef struct jh_joints3d_params {
  int32_t min_views, refine_radius;
  float min_conf, max_error_px;
} jh_joints3d_params;
int jh_joints3d_params_check(const jh_joints3d_params* params);    /* no GPU needed */
int jh_op_joint_peaks_refine(const float* heat_dev, int n, int hh, int wh, int jp, const int32_t* idx_dev, int j,
                             int radius, float* offsets_dev, void* stream);
int jh_op_triangulate_joints(const float* obs_dev, int t, int cams, int j, const float* cam_dev, const float* intr_dev,
                             const float* dist_dev, int calib_per_frame, const jh_joints3d_params* params,
                             float* points_dev, int32_t* views_dev, uint8_t* members_dev, float* error_dev,
                             void* stream);
int jh_predictor_triangulate_joints(jh_predictor* pr, const float* heat_all_dev, int t0, const uint8_t* mask_dev,
                                    const jh_joints3d_params* params, float* points_dev, int32_t* views_dev,
                                    uint8_t* members_dev, float* error_dev, float* obs_dev /* optional */,
                                    void* stream);

/* ---- per-joint camera masks: leave a camera out of the voxel gather for the joints it gets wrong (additive, ABI 4)
 * The reprojection layer averages every joint's heat map over the cameras; a camera mask leaves a camera out for a
 * whole frame set.  A joint mask jm (T,J,C) uint8 gives every joint a camera set of its own -- members (T,J,C) of
 * jh_predictor_triangulate_joints is one.  With a(t,c) the camera mask of the call (1 when there is none):
 *   e(t,j,c) = a(t,c) && jm[t][j][c] != 0,  n(t,j) = sum_c e(t,j,c);
 *   fallback: n(t,j) == 0 -> e(t,j,.) = a(t,.), n(t,j) = sum_c a(t,c) -- an empty joint behaves as in the plain or
 *   camera-masked forward; the padding channels J <= j < Jp have e = a;
 *   vol[t][vox][j] = (sum over c ascending with e(t,j,c) of heat[t][c][tap(t,c,vox)][j]) / n(t,j): an fp32 sum from +0
 *   in camera order, an IEEE division by (float)n as the camera-masked kernels divide (no camera at all: divisor 1, sums
 *   0), then the /255 of the forward in its existing form; tap is the gather index of the existing kernels, virtual zero
 *   border included.
 * A heat value with e = 0 is selected out, not multiplied -- it may be NaN --, and a camera with e(t,.,c) = 0 for every
 * channel is not loaded at all.  So: all ones is bit-equal to no joint mask; jm[t][j][c] = m[t][c] for all j is bit-equal
 * to the camera-masked gather with m; a camera mask composes as jm & m; an all-zero jm is the plain result; rows of a
 * batch are independent.  The joint-masked gather has the voxel-row form only (any even grid, up to 64 channels, up to 64
 * cameras): where the plain gather runs its cube form the two are different kernels with the same indices and sum order.
 * jh_predictor_set_joint_mask: the mode of every later whole-path forward of this predictor.  JH_JOINT_MASK_GIVEN copies
 * joint_mask_dev (T,J,C) into a buffer of the predictor's own, on `stream`; JH_JOINT_MASK_CONSENSUS makes the forward run
 * the three launches of jh_predictor_triangulate_joints between stage 2 and stage 3 -- on its own heat maps, with the
 * call's camera mask, the centres stage 2 wrote and the calibration in force; params NULL = min_views 2, refine_radius 1,
 * min_conf 0.1, max_error_px 8 -- and takes the members as the joint mask (an invalid frame set has no members and falls
 * back), so V2V runs once, on the cleaned volume; JH_JOINT_MASK_OFF (mask and params ignored) returns to the plain
 * forward.  While the mode is not off every whole-path forward entry runs plain launches: there is no graph slot for the
 * form, the captured graphs stay untouched and replay again once the mode is off.  Spread, centres, camera masks and
 * per-frame-set calibration compose unchanged.  The buffers are allocated by the first call with a mode that is not off
 * -- never by jh_predictor_create, and jh_predictor_device_bytes does not count them --, which must not be made inside a
 * stream capture.  A bad mode, a NULL mask with GIVEN, out-of-range params, more than 64 cameras or cameras that are not
 * all local: non-zero, jh_last_error() set, nothing enqueued, the mode unchanged.
 * jh_predictor_get_joint_mask: the effective sets e as cameras_out (T,J,C) uint8 and n as count_out (T,J) int32 (either
 * may be NULL) of the last joint-masked forward / stage 3 (rows t0 .. t0+T3-1 each), copied on `stream`.
 * jh_predictor_stage_3d_joint_masked: jh_predictor_stage_3d_masked (mask_dev (T,C) or NULL) with joint_mask_dev (T,J,C),
 * rows t0 .. t0+T3-1 read in place.  A caller gets the consensus in the staged path by calling
 * jh_predictor_triangulate_joints between its stages.  The gather's workspace is the predictor's: joint-masked stage-3
 * calls of one predictor are ordered on one stream.
 * jh_reproject_forward_joint_masked: the operator alone, with jh_reproject_forward's conventions (T = 1, padded NCHW
 * in, NCDHW out, not divided by 255): mask_dev (cams) uint8 or NULL, joint_mask_dev (joints,cams) uint8; workspace of
 * jh_reproject_joint_masked_workspace_bytes. */
#define JH_JOINT_MASK_OFF 0
#define JH_JOINT_MASK_GIVEN 1
#define JH_JOINT_MASK_CONSENSUS 2
int jh_predictor_set_joint_mask(jh_predictor* pr, int mode, const uint8_t* joint_mask_dev /* (T,J,C) or NULL */,
                                const jh_joints3d_params* params /* NULL = defaults */, void* stream);
int jh_predictor_get_joint_mask(jh_predictor* pr, uint8_t* cameras_out_dev, int32_t* count_out_dev, void* stream);
int jh_predictor_stage_3d_joint_masked(jh_predictor* pr, const float* heat_all_dev, int t0,
                                       const uint8_t* mask_dev /* or NULL */, const uint8_t* joint_mask_dev,
                                       float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);
int64_t jh_reproject_joint_masked_workspace_bytes(int cams, int joints, int hs, int grid_size);
int jh_reproject_forward_joint_masked(const float* heatmaps_padded_dev, int cams, int joints, int hs,
                                      const int32_t* center3d_dev, const int32_t* center_hm_dev,
                                      const float* cam_dev, const float* intr_dev, const float* dist_dev,
                                      int grid_size, float grid_spacing, const uint8_t* mask_dev /* or NULL */,
                                      const uint8_t* joint_mask_dev, float* vol_dev, void* workspace_dev,
                                      int64_t workspace_bytes, void* stream);

/* HybridNetBackbone.forward: crops (T,C,3,B,B) normalised NCHW dev, center_hm
 * (T,C,2) int32, center3d (T,3) int32 -> heatmap_final (T,J,Gh,Gh,Gh) optional,
 * heatmaps_padded (T,C,J,hs,hs) optional, points (T,J,3), conf (T,J). */
int jh_predictor_hybridnet_forward(jh_predictor* pr, const float* crops_dev,
                                   const int32_t* center_hm_dev, const int32_t* center3d_dev,
                                   float* heatmap_final_dev, float* heatmaps_padded_dev,
                                   float* points_dev, float* conf_dev, void* stream);

/* ---- JarvisPredictor2D  (jarvis/prediction/jarvis2D.py:20-44,102-155)
 * Single-camera 2D pose: resize -> CenterDetect -> argmax -> crop -> KeypointDetect ->
 * per-joint argmax.  `time_batch` independent images per call (the reference's call is
 * 1); num_cameras / roi / spacing / cam_* of the config are ignored.
 * frames (T,3,H,W) fp32 RGB [or (T,H,W,3) uint8 BGR] -> points2D (T,J,2) int32 full-frame
 * pixels, conf (T,J), valid (T) int32 (0 = centre maxval <= 40: the reference returns
 * (None, None), jarvis2D.py:121,150-153). */
typedef struct jh_predictor2d jh_predictor2d;
int jh_predictor2d_create(const jh_params* center_params, const jh_params* kp_params,
                          const jh_predictor_config* cfg, jh_predictor2d** out);
void jh_predictor2d_destroy(jh_predictor2d* pr);
int jh_predictor2d_forward(jh_predictor2d* pr, const float* frames_dev, int32_t* points_dev,
                           float* conf_dev, int32_t* valid_dev, void* stream);
int jh_predictor2d_forward_u8(jh_predictor2d* pr, const uint8_t* frames_dev, int32_t* points_dev,
                              float* conf_dev, int32_t* valid_dev, void* stream);

/* frames (T,3H/2,W) YUV 4:2:0, format JH_FRAME_I420 or JH_FRAME_NV12 (as jh_predictor_forward_yuv). */
int jh_predictor2d_forward_yuv(jh_predictor2d* pr, const uint8_t* frames_dev, int format, int32_t* points_dev,
                               float* conf_dev, int32_t* valid_dev, void* stream);
/* frames (T) images of a described surface (as jh_predictor_forward_surface). */
int jh_predictor2d_forward_surface(jh_predictor2d* pr, const uint8_t* frames_dev, const jh_yuv_surface* surface,
                                   int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);
/* frames (T) raw sensor images (as jh_predictor_forward_sensor). */
int jh_predictor2d_forward_sensor(jh_predictor2d* pr, const uint8_t* frames_dev, const jh_sensor_surface* surface,
                                  int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);

/* images_host: T device pointers, one image each (as jh_predictor_forward_images, which see). */
int jh_predictor2d_forward_images(jh_predictor2d* pr, const void* const* images_host, int n_images, int format,
                                  const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                  int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);

/* ---- pixel surfaces: RGB in any byte order, 4-byte and planar RGB, grey, and YUV that is not 4:2:0 (additive, ABI 4)
 * ONE description for what Python imaging libraries, cameras and capture cards hand out besides BGR and YUV 4:2:0,
 * read in place.  An image is three 8-bit components per pixel -- R, G, B (JH_PIXEL_RGB) or Y, U, V (JH_PIXEL_YUV) --
 * and every component has its own address rule inside the `image_stride` bytes of ONE h x w image:
 *   component k of pixel (y, x) is the byte at offset[k] + (y >> ys[k]) * pitch[k] + (x >> xs[k]) * step[k].
 * Frames are (T,cam_n) such images back to back (the 2D predictor: (T)), image n at byte n * image_stride.
 * Chroma is replicated: pixel (y, x) takes sample (y >> ys, x >> xs), as the 4:2:0 forms do and as OpenCV's
 * COLOR_YUV2BGR_YUY2 does.  JH_PIXEL_YUV converts with the formula and the four constant rows printed for
 * jh_yuv_surface above (same table, same int32 arithmetic), selected by (matrix, range).  The (R, G, B) bytes then take
 * the uint8 path unchanged: the result equals, bit for bit, jh_predictor_forward_u8 on the converted frames.
 * Components may interleave and may coincide (grey), so there is no overlap rule.  No byte before an image's base and
 * none at or beyond image_stride is ever addressed; bytes inside the image that are no component (an alpha byte, pitch
 * padding, gaps) may hold anything and never reach a result.
 * The common layouts as values of the fields, for h x w tight (cw = ceil(w/2), ch = ceil(h/2)):
 *   layout      offset (R,G,B resp. Y,U,V)            step     pitch                 xs      ys
 *   rgb24       0, 1, 2                               3        3w                    0       0
 *   bgr24       2, 1, 0                               3        3w                    0       0
 *   bgra/bgr0   2, 1, 0   (rgba 0,1,2; argb 1,2,3; abgr 3,2,1)  4   4w               0       0
 *   planar RGB  0, hw, 2hw                            1        w                     0       0
 *   gbrp        R 2hw, G 0, B hw                      1        w                     0       0
 *   grey        0, 0, 0                               1        w                     0       0
 *   yuyv422     Y 0, U 1, V 3  (yvyu: U 3, V 1)       2, 4, 4  4cw                   0,1,1   0
 *   uyvy422     Y 1, U 0, V 2                         2, 4, 4  4cw                   0,1,1   0
 *   nv16        Y 0, U hw, V hw+1                     1, 2, 2  w, 2cw, 2cw           0,1,1   0
 *   yuv422p     Y 0, U hw, V hw + h cw                1        w, cw, cw             0,1,1   0
 *   yuv444p     0, hw, 2hw                            1        w                     0       0
 *   nv24        Y 0, U hw, V hw+1                     1, 2, 2  w, 2w, 2w             0       0
 *   yuv440p     Y 0, U hw, V hw + ch w                1        w                     0       0,1,1
 *   yuv411p     Y 0, U hw, V hw + h ceil(w/4)         1        w, ceil(w/4) twice    0,2,2   0
 *   4:2:0       as jh_yuv_surface places them         1 or 2   as there              0,1,1   0,1,1
 * jh_pixel_surface_check (no GPU needed) is the validation every entry point applies: h, w > 0 of ANY parity (a
 * subsampled plane is ceil wide / high); colour known; JH_PIXEL_YUV: matrix and range known, JH_PIXEL_RGB: both 0;
 * sample == JH_SAMPLE_U8 (every other value refused: room for later); step[k] 1 .. 8; xs[k], ys[k] 0 .. 2;
 * JH_PIXEL_RGB: every shift 0; JH_PIXEL_YUV: xs[0] == ys[0] == 0, xs[1] == xs[2], ys[1] == ys[2]; offset[k] >= 0;
 * pitch[k] >= ((w-1) >> xs[k]) * step[k] + 1;
 * offset[k] + ((h-1) >> ys[k]) * pitch[k] + ((w-1) >> xs[k]) * step[k] + 1 <= image_stride.
 * Returns 0, or nonzero with jh_last_error() set.
 * The entry points take EXACTLY ONE OF frames_dev (contiguous, image n at n * image_stride) and images_host + n_images
 * (one device pointer per image, as jh_predictor_forward_images; an image may start at any address and image_stride is
 * then only the extent every component ends within).  mask_dev as in jh_predictor_forward_masked, or NULL.  Everything
 * that follows a forward (jh_predictor_views2d, set_centers, set_spread, set_joint_mask, triangulate_joints, per-frame
 * calibration) follows these as it follows any forward.  A graph-replaying predictor keeps captured graphs of its own
 * for this form -- contiguous and per image, each unmasked and masked --; a call whose description differs from the
 * recorded one records again, and alternating with any other format re-records neither.
 * Out of scope: the staged jh_predictor_stage_* entries, the camera-sharded path, and samples wider than a byte. */
#define JH_PIXEL_RGB 0   /* components 0,1,2 are R,G,B bytes */
#define JH_PIXEL_YUV 1   /* components 0,1,2 are Y,U,V; converted as jh_yuv_surface converts */
typedef struct jh_pixel_surface {
  int64_t image_stride;          /* bytes from image n to image n+1 */
  int64_t offset[3], pitch[3];   /* component k of pixel (y,x): the byte at                        */
  int32_t step[3];               /*   offset[k] + (y >> ys[k]) * pitch[k] + (x >> xs[k]) * step[k] */
  int32_t xs[3], ys[3];
  int32_t colour;                /* JH_PIXEL_RGB / JH_PIXEL_YUV */
  int32_t matrix, range;         /* JH_YUV_*; must be 0 for JH_PIXEL_RGB */
  int32_t sample;                /* JH_SAMPLE_U8 only; every other value refused (room for later) */
} jh_pixel_surface;
int jh_pixel_surface_check(const jh_pixel_surface* surface, int h, int w);
/* unit-test helper, as jh_op_yuv_surface_to_bgr: n images -> (n,h,w,3) uint8 BGR; synchronises */
int jh_op_pixels_to_bgr(const uint8_t* frames_dev, const jh_pixel_surface* surface, int n, int h, int w,
                        uint8_t* out_bgr_dev, void* stream);
int jh_predictor_forward_pixels(jh_predictor* pr, const uint8_t* frames_dev, const void* const* images_host,
                                int n_images, const jh_pixel_surface* surface, const uint8_t* mask_dev /* or NULL */,
                                float* points_dev, float* conf_dev, int32_t* valid_dev, void* stream);
/* the outputs of jh_predictor2d_forward_surface */
int jh_predictor2d_forward_pixels(jh_predictor2d* pr, const uint8_t* frames_dev, const void* const* images_host,
                                  int n_images, const jh_pixel_surface* surface, int32_t* points_dev, float* conf_dev,
                                  int32_t* valid_dev, void* stream);
/* Tone tables of the 2D predictor: one camera's (3,256); see jh_predictor_set_tone */
int jh_predictor2d_set_tone(jh_predictor2d* pr, const float* tables_dev /* (3,256) or NULL */, void* stream);
/* unit-test helper of the tone tables: n images of any byte form -> (n,3,h,w) fp32 RGB, the values the resize / crop
 * fetch sees for every pixel; synchronises.  The form is `format` (JH_FRAME_BGR_U8 .. JH_FRAME_SENSOR, with the
 * jh_yuv_surface resp. jh_sensor_surface that JH_FRAME_SURFACE / JH_FRAME_SENSOR come with) or a jh_pixel_surface
 * alone (format ignored), validated as the entry points validate.  tables_dev (cams,3,256) or NULL: image i reads
 * camera i % cams; NULL gives byte * (1/255). */
int jh_op_frames_to_rgb_f32(const void* frames_dev, int format, const jh_yuv_surface* yuv,
                            const jh_sensor_surface* sensor, const jh_pixel_surface* pixels, int n, int h, int w,
                            const float* tables_dev, int cams, float* out_dev, void* stream);
/* jh_predictor_detect_subjects with the description in place of (format, yuv, sensor) */
int jh_predictor_detect_subjects_pixels(jh_predictor* pr, const uint8_t* frames_dev, const void* const* images_host,
                                        int n_images, const jh_pixel_surface* surface, const uint8_t* mask_dev,
                                        const jh_subjects_params* params, float* centers_dev, int32_t* views_dev,
                                        int32_t* members_dev, float* error_dev, float* peaks_dev, void* stream);

/* ---- per-launch timing (HIP events on the launch stream; used by bench.py for
 * the roofline figures).  begin() switches recording on for every kernel the
 * library launches from this process; end() synchronises and returns the number
 * of records; get() returns name, milliseconds, algorithmic FLOPs and bytes. */
int jh_profile_begin(void);
int jh_profile_end(int* n_records);
int jh_profile_get(int i, char* name, int name_cap, double* ms, double* flops, double* bytes);

/* ---- single-operator entry points (unit-test helpers, NOT part of the forward path:
 * they repack host weights, allocate scratch with hipMalloc and end in a stream
 * synchronisation, so they are neither asynchronous nor graph-capturable)
 * conv: x (N,Cin,[D,]H,W) -> y; weights/bias are HOST pointers in torch layout
 * ((Cout,Cin,k..) or, transposed, (Cin,Cout,k..)); kind 0 = conv (k, stride,
 * pad), 1 = ConvTranspose2d k4 s2 p1, 2 = ConvTranspose3d k2 s2.  When
 * norm_act >= 0 the InstanceNorm (+ activation 0 none / 1 relu / 2 silu) that
 * follows the conv in the networks is applied from the fused statistics.  The layer takes the kernel form the network
 * plans give it (jh_conv_form below, at the process-wide precision). */
int jh_op_conv(int nd, int kind, int k, int stride, int pad, int cin, int cout,
               const float* w_host, const float* b_host, const float* x_dev, int n, int d, int h,
               int w, const float* gate_dev, int norm_act, float* y_dev, void* stream);
/* TEST-ONLY: launches of the window form of ConvTranspose2d k4 s2 p1 (layers without statistics and gate;
 * JH_DECONV4_WINDOW=0 at weight-packing time selects the four-parity forms) by this process so far -- how a test tells
 * which form ran.  Under hipGraph capture it counts captures, not replays. */
long jh_deconv4_window_launches(void);
/* Which kernel form a convolution layer takes (no GPU needed; csrc/conv_layer.h): the layer as jh_op_conv describes it,
 * used with / without bias, fused statistics and a gate (0 none, 1 tensor, 2 recipe) at precision 0 / 1 / 2
 * (jh_predictor_config::precision); in_px: floats per input pixel in memory, 0 = cin rounded up to 8.  Reads JH_WINO,
 * JH_WINO_PW and JH_DECONV4_WINDOW as they stand at the call, as making a layer does.  name receives "mfma" (+ "_paired"
 * / "_tappair" / "_window": the weight layout), "wino", "wino_bf16x3", "conv_bf16x3", "deconv4_bf16x3" or "deconv_c1". */
int jh_conv_form(int nd, int kind, int k, int stride, int pad, int cin, int cout, int has_bias,
                 int want_stats, int gate /*0 none, 1 tensor, 2 recipe*/, int precision,
                 int in_px /*0: cpad(cin)*/, char* name, int name_cap);
/* Which kernel form a fused BiFPN node takes, with its row segmentation and launch shape (no GPU needed;
 * csrc/node_layer.h): c -> cout channels (unpadded) on n images of h x w, n_in inputs in modes[] (0 same level, 1 x2
 * up-sampled, 2 x4 up-sampled, 3 2x2-max-pooled), activation 0 none / 1 relu / 2 silu, batch_class 0 by launch size
 * (jh_op_bifpn_node) / 1 time batch below 8 / 2 time batch of 8 and more, want_pool: the caller could use the
 * 2x2-max-pooled output.  Reads JH_NODE_ROWS once per process.  name receives "tile", "rows_wave", "rows_pairs" or
 * "rows_wg"; out receives seg_rows, strips, segs, grid.x, grid.y, block.x, dynamic LDS bytes, pool (the node writes the
 * pooled output).  Fails for a node no form takes. */
int jh_node_form(int c, int cout, int n, int h, int w, int n_in, const int* modes, int act, int batch_class,
                 int want_pool, char* name, int name_cap, int32_t out[8]);
/* ---- the keypoint head's box.  A whole-path forward whose voxel gather is the only reader of the heat
 * maps computes, per image, only the tiles of the head that cover the box of pixels the gather can read; JH_HEAD_ROI=0,
 * read when a predictor is created, switches that off.
 * jh_head_roi_form (no GPU needed; csrc/conv_layer.h): does the head of a 3D predictor -- ConvTranspose2d k4 s2 p1,
 * cin -> cout, at precision 0 / 1 / 2 -- take a box in a call of kind 0 whole-path forward / 1 staged stage 2 /
 * 2 jh_predictor_hybridnet_forward / 3 whole-path forward on a stream the caller is capturing, with the joint-mask
 * consensus in force, on a camera-sharded predictor, in a plan built with want_res1?  Reads JH_HEAD_ROI and
 * JH_DECONV4_WINDOW as they stand at the call.
 * jh_predictor_views2d / jh_predictor_triangulate_joints on the predictor's own heat maps behind a boxed forward run the
 * head once more without a box first (the full maps, the same bits); a caller that wants both on every call and
 * nothing extra sets JH_HEAD_ROI=0. */
int jh_head_roi_form(int call_kind, int consensus, int sharded, int want_res1, int cin, int cout, int precision,
                     int32_t* takes_box);
/* TEST-ONLY: jh_op_conv's ConvTranspose2d k4 s2 p1 (no bias) with one box per image, box_host (n, 4) = (x0, y0, x1, y1)
 * inclusive in output pixels, or NULL = no box.  The output starts as NaN: what no workgroup stores stays NaN.  Fails
 * for a layer that is not of the window form. */
int jh_op_deconv4_box(int cin, int cout, const float* w_host, const float* x_dev, int n, int h, int w,
                      const int32_t* box_host, float* y_dev, void* stream);
/* TEST-ONLY: the boxes of t x cams images as stage 2 takes them -- coarse projection of the grid_size^3 grid, then
 * min / max per camera -> box_dev (t, cams, 4) stored-pixel boxes (x0, y0, x1, y1) of heat maps of side
 * hs - 2 + 2 heat_pad -- and, with idx_dev (t, cams, grid_size^3), the voxel gather's own indices iv * hs + iu from
 * that same field.  center3d_dev (t, 3), center_hm_dev (t, cams, 2); valid_dev (t) / mask_dev (t, cams) may be NULL;
 * calib_per_frame: the calibration arrays hold t * cams rows. */
int jh_op_repro_box(const float* cam_dev, const float* intr_dev, const float* dist_dev, int calib_per_frame,
                    const int32_t* center3d_dev, const int32_t* center_hm_dev, const int32_t* valid_dev,
                    const uint8_t* mask_dev, int t, int cams, int joints, int hs, int heat_pad, int grid_size,
                    float grid_spacing, int32_t* box_dev, int32_t* idx_dev, void* stream);
/* TEST-ONLY: the boxes (time_batch, cam_n, 4) the last boxed stage 2 of the predictor wrote (box_dev may be NULL) and
 * whether the predictor's own heat maps are, right now, complete only inside them. */
int jh_predictor_debug_head_boxes(jh_predictor* pr, int32_t* box_dev, int32_t* boxed, void* stream);
/* TEST-ONLY: the operand transform a consumer applies while it stages its input (csrc/jh_common.h: InNorm, SeGate),
 * described from the host so that only the consumer is under test. */
typedef struct jh_op_operand {
  const double* in_sums_host; /* (n, cin, 2) sum and sum of squares per image and channel of x, or NULL: x is read as it
                               * is.  InstanceNorm (eps 1e-5) + in_act are applied on load, 1 / pixels as a float */
  int32_t in_act;             /* 0 none / 1 relu / 2 silu, behind that InstanceNorm */
  int32_t latency_class;      /* ConvDesc::latency_class: 1 = the tile forms of the single-frame-set plans */
  int32_t want_stats;         /* 1: the launch also accumulates the fused statistics of y (out_sums_host); 0 and no gate:
                               * a ConvTranspose2d k4 s2 p1 may take the window form */
  int32_t se_c, se_s;         /* the squeeze-excite gate as the recipe (se_pool_host != NULL): channels (= cin), squeeze */
  float se_inv_hw;            /* 1 / pixels the pooled sums were taken over */
  const float *se_wr_host, *se_br_host, *se_we_host, *se_be_host; /* (se_s, se_c), (se_s), (se_c, se_s), (se_c) */
  const double* se_pool_host; /* (n, se_c) pooled sums of the activated tensor */
  double* out_sums_host;      /* (n, cout, 2), with want_stats: the statistics the launch emitted for its consumers, the
                               * limbs of each value added in the reader's fixed order; the buffer behind y then starts
                               * as NaN.  NULL: not returned */
} jh_op_operand;
/* jh_op_conv with the operand transform: y is always the RAW convolution output (no InstanceNorm behind it).  The gate
 * is either gate_dev (n, cin) or the recipe in `operand`.  kind 1 with cout == 1, no bias, no statistics: the
 * one-channel ConvTranspose2d kernel of the CenterDetect head. */
int jh_op_conv_operand(int nd, int kind, int k, int stride, int pad, int cin, int cout,
                       const float* w_host, const float* b_host, const float* x_dev, int n, int d, int h,
                       int w, const float* gate_dev, const jh_op_operand* operand, float* y_dev, void* stream);
/* The squeeze-excite gate kernel on its own: pooled sums (n, c) and the two layers' weights from the host ->
 * gate_dev (n, c) = sigmoid(We silu(Wr (pool * inv_hw) + br) + be). */
int jh_op_se_gate(const double* pool_host, int n, int c, int squeeze, float inv_hw, const float* wr_host,
                  const float* br_host, const float* we_host, const float* be_host, float* gate_dev, void* stream);
/* The InstanceNorm pass on its own, in place on a copy of x (n, c, [d,] h, w) as the plans run it:
 * act((x - mean) * rstd + r1) + r2 with statistics sums_host (n, c, 2); r1_sums_host: r1 is raw, its
 * InstanceNorm + ReLU is applied on load (act must be 1).  write_y: y_dev receives the result; want_pool: pool_host
 * (n, c) doubles receive the sums of the result over the pixels.  min_block_kb: Plan::norm_block_kb (0 or 64). */
int jh_op_norm_apply(const float* x_dev, int n, int c, int d, int h, int w, const double* sums_host, int act,
                     const float* r1_dev, const double* r1_sums_host, const float* r2_dev, int write_y, int want_pool,
                     int min_block_kb, float* y_dev, double* pool_host, void* stream);
/* depthwise k x k stride 1: x (N,C,H,W), w_host (C,1,k,k) -> y. */
int jh_op_depthwise(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w,
                    int norm_act, float* y_dev, void* stream);
/* ... with the squeeze-excite pooled sums of the same launch (MBConvBlock.forward,
 * jarvis/efficienttrack/efficientnet.py:100-107: _depthwise_conv -> _gn1 -> swish -> adaptive_avg_pool2d): h, w <= 16;
 * y_dev (N,C,h,w) RAW depthwise output, pool_dev (N,C) = sum over pixels of SiLU(InstanceNorm(y)). */
int jh_op_depthwise_pool(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w,
                         float* y_dev, float* pool_dev, void* stream);
/* TEST-ONLY: the depthwise launch with everything it hands to its consumers: y_dev (n,c,h,w) RAW, out_sums_host
 * (n, c, 2) the emitted sum and sum of squares (limbs added in the reader's order) and, want_pool (refused unless the
 * image is one tile: h, w <= 20), pool_host (n, c) doubles = the pooled sums of SiLU(InstanceNorm(y)) of the same
 * launch, read from their limbs as jh_op_norm_apply reads them.  The buffer behind y starts as NaN. */
int jh_op_depthwise_ex(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w, int want_pool,
                       float* y_dev, double* out_sums_host, double* pool_host, void* stream);
/* TEST-ONLY: the stem convolution Conv2d(3 -> cout, k3, s2, p1, no bias) of the EfficientNet trunk on its own
 * (csrc/stem.hip, the form fed by a pre-processed tensor): w_host (cout,3,3,3), x_dev (n,3,h,w) -> y_dev
 * (n,cout,h/2,w/2) RAW and out_sums_host (n, cout, 2) as above.  cout 16 or 32; h, w even.  The input is laid out as
 * jh_efftrack_forward lays it out (one float4 per pixel); the buffer behind y starts as NaN. */
int jh_op_stem(int cout, const float* w_host, const float* x_dev, int n, int h, int w, float* y_dev,
               double* out_sums_host, void* stream);

/* The YUV 4:2:0 -> BGR conversion of jh_predictor_forward_yuv on its own: frames (n,3h/2,w) in format
 * JH_FRAME_I420 / JH_FRAME_NV12 -> out_bgr (n,h,w,3) uint8 BGR (device pointers; h, w even). */
int jh_op_yuv420_to_bgr(const uint8_t* frames_dev, int format, int n, int h, int w, uint8_t* out_bgr_dev,
                        void* stream);
/* The same for images of a described surface (jh_yuv_surface above): frames n * image_stride bytes -> out_bgr
 * (n,h,w,3) uint8 BGR. */
int jh_op_yuv_surface_to_bgr(const uint8_t* frames_dev, const jh_yuv_surface* surface, int n, int h, int w,
                             uint8_t* out_bgr_dev, void* stream);
/* The demosaic on its own (jh_sensor_surface above): frames n * image_stride bytes -> out_bgr (n,h,w,3) uint8 BGR. */
int jh_op_sensor_to_bgr(const uint8_t* frames_dev, const jh_sensor_surface* surface, int n, int h, int w,
                        uint8_t* out_bgr_dev, void* stream);

/* The scan of jh_predictor_views2d on its own: the argmax of every joint's heat map in ONE pass over the buffer (each
 * byte read once; jh_predictor2d_forward's per-joint kernel reads the image once per joint).  heat (n,hh,wh,jp)
 * channel-last dev, jp a multiple of 8 up to 256, channels j..jp-1 ignored -> idx (n,j) int32 flat index
 * y*wh + x of the maximum (the lowest among equal maxima; NaN never wins), max (n,j).  workspace_dev: >=
 * jh_joint_argmax_all_workspace_bytes(n, hh, wh, jp) bytes, 256-byte aligned (0 for a shape the scan does not take). */
int64_t jh_joint_argmax_all_workspace_bytes(int n, int hh, int wh, int jp);
int jh_op_joint_argmax_all(const float* heat_dev, int n, int hh, int wh, int j, int jp, int32_t* idx_dev,
                           float* max_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* One fused BiFPN node (jarvis/efficienttrack/model.py:301-353 fusion expressions + :223-232
 * SeparableConvBlock.forward, without its trailing InstanceNorm):
 *   y = pointwise(depthwise3x3(act(sum_i weights[i] * resample_i(InstanceNorm(x_i))))) + bias
 * x_i (N,C,h_i,w_i) NCHW dev at the resolution its mode implies (0 same, 1 nearest x2 up from
 * (h/2,w/2), 2 nearest x4 up from (h/4,w/4), 3 2x2 max-pool from (2h,2w)); modes / weights host
 * arrays of 3; act 0 none / 2 SiLU; dw_host (C,1,3,3), pw_host (Cout,C), bias_host (Cout). */
int jh_op_bifpn_node(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout,
                     int h, int w, const float* x0_dev, const float* x1_dev, const float* x2_dev,
                     const float* dw_host, const float* pw_host, const float* bias_host, float* y_dev,
                     void* stream);
/* TEST-ONLY: what jh_op_bifpn_node leaves out of a node as the network plans run it (csrc/node_layer.h). */
typedef struct jh_op_node_ex {
  int32_t batch_class;             /* as in jh_node_form: 0 by launch size / 1 time batch below 8 / 2 of 8 and more */
  int32_t want_pool;               /* the caller could use the 2x2-max-pooled raw output, if the form can write it */
  const double* in_sums_host[3];   /* per input (n, c, 2) sum and sum of squares that REPLACE the statistics the entry
                                    * computes from the tensor's own pixels, or NULL */
  int64_t in_count[3];             /* ... and the pixels they were taken over: inv_cnt = 1 / count as a float (a pooled
                                    * tensor carries its producer's statistics and pixel count) */
  float* y_pool_dev;               /* (n, cout, h/2, w/2) NCHW dev: written exactly when the choice says `pool` */
  int32_t* pool_written_host;      /* receives 1 when y_pool_dev was written, else 0; or NULL */
  double* out_sums_host;           /* (n, cout, 2): the statistics the node emitted for its consumers, the limbs of each
                                    * value added in the reader's fixed order; or NULL */
} jh_op_node_ex;
/* jh_op_bifpn_node in the time-batch class `ex` names, with the pooled output, handed-on input statistics and the
 * emitted statistics.  jh_op_bifpn_node is this call with class 0, no pooled output, no overrides and no extra outputs.
 * Both fill the buffers behind y and y_pool with NaN before the launch: a pixel nobody wrote arrives as NaN. */
int jh_op_bifpn_node_ex(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout,
                        int h, int w, const float* x0_dev, const float* x1_dev, const float* x2_dev,
                        const float* dw_host, const float* pw_host, const float* bias_host, float* y_dev,
                        const jh_op_node_ex* ex, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JARVIS_HIP_H */
