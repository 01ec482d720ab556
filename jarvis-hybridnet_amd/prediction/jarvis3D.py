"""JarvisPredictor3D on MI355X (mirrors jarvis/prediction/jarvis3D.py:19-190).

Same constructor and forward signature, same attributes (`centerDetect`,
`hybridNet` with `.effTrack/.reproLayer/.v2vNet`, `reproTool`), same
`(None, None)` convention when fewer than two cameras see the subject.  The
reference's acceleration slot (`trt_mode`, jarvis3D.py:42-46) is where this
implementation lives permanently: `forward` is a single native call that runs
resize -> CenterDetect -> argmax -> triangulation -> crops -> KeypointDetect ->
reprojection -> V2V -> soft-argmax without any host synchronisation; the one
sync happens when the validity flag is read at the API edge.
"""
import torch
import torch.nn as nn

from .. import _native as N
from .._params import flat_state, weights_fingerprint
from .._predictor import NativePredictor
from ..efficienttrack.efficienttrack import EfficientTrack
from ..hybridnet.hybridnet import HybridNet
from ..tracks import check_tracker
from ..utils.reprojection import ReprojectionTool


def precision_for_trt_mode(trt_mode, precision=None):
    """The reference's `trt_mode` ('off' | 'new' | 'previous', utils/paramClasses.py:21,34; forwarded by the
    drivers, prediction/predict3D.py:36-37) selects its half-precision TensorRT engines (jarvis3D.py:42-46,
    93,107,122: enabled_precisions={torch.half}).  There are no engines to compile or load here -- the native
    HIP path is always on -- so 'new' and 'previous' both select what stands in that seat: the labelled
    reduced-precision mode bf16x3 (3D keypoints within 3e-4 mm of the fp32 reference on every fixture).
    'off' = fp32, the parity mode.  An explicit `precision` wins over trt_mode; returns None for
    "follow the process default" (`_native.set_precision`)."""
    if trt_mode not in ("off", "new", "previous"):
        raise ValueError("trt_mode must be 'off', 'new' or 'previous' (utils/paramClasses.py:21), got %r"
                         % (trt_mode,))
    if precision is not None:
        return precision
    if trt_mode != "off":
        print("[Info] trt_mode='%s': no TensorRT on MI355X -- using the native reduced-precision mode "
              "bf16x3 (split-bf16 MFMA, fp32 accumulate) in its place" % trt_mode)
        return "bf16x3"
    return None


def check_native_seam(predictor):
    """The reference accelerates by ASSIGNING compiled callables to three attributes after construction
    (jarvis3D.py:64-69,89,103,119: `self.centerDetect`, `self.hybridNet.effTrack`, `self.hybridNet.v2vNet`).  Here
    the whole forward is one native launch plan built from the WEIGHTS of those attributes, so a foreign callable
    put in their place would be silently ignored -- refuse it instead.  (Another native module of the same class --
    e.g. one carrying other weights -- is fine: plans are rebuilt when the weights' fingerprint changes.)"""
    from ..efficienttrack.model import EfficientTrackBackbone
    from ..hybridnet.model import HybridNetBackbone
    from ..hybridnet.v2vnet import V2VNet
    slots = [("centerDetect", getattr(predictor, "centerDetect", None), EfficientTrackBackbone)]
    hyb = getattr(predictor, "hybridNet", None)
    slots.append(("hybridNet", hyb, HybridNetBackbone))
    if isinstance(hyb, HybridNetBackbone):
        slots += [("hybridNet.effTrack", getattr(hyb, "effTrack", None), EfficientTrackBackbone),
                  ("hybridNet.v2vNet", getattr(hyb, "v2vNet", None), V2VNet)]
    for name, obj, cls in slots:
        if not isinstance(obj, cls):
            raise RuntimeError(
                "JarvisPredictor3D.%s has been replaced by a %s: this implementation runs the whole forward as one "
                "native HIP launch plan built from the weights of its own %s modules, so an assigned callable cannot "
                "take effect (the reference's trt_mode seam, jarvis3D.py:64-69).  Load weights with load_state_dict() "
                "/ the weights_* constructor arguments, select the reduced-precision mode with trt_mode='new', or "
                "call the replacement yourself." % (name, type(obj).__name__, cls.__name__))


def image_frames(num_cameras, images, frame_format, frame_layout):
    """The `images` argument of the per-image forms (C tensors, or T sequences of C tensors) checked -> Frames."""
    if isinstance(images, (list, tuple)) and len(images) > 0 and torch.is_tensor(images[0]):
        images = [images]
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError("images must be a sequence of %d tensors or a sequence of such sequences"
                         % num_cameras)
    for t, frame_set in enumerate(images):
        if not isinstance(frame_set, (list, tuple)) or len(frame_set) != num_cameras:
            raise ValueError("frame set %d: expected a sequence of %d images (one per camera), got %s" % (
                t, num_cameras,
                len(frame_set) if isinstance(frame_set, (list, tuple)) else type(frame_set).__name__))
    flat = [img for frame_set in images for img in frame_set]
    return N.frame_images(flat, (len(images), num_cameras), frame_format, frame_layout)


class JarvisPredictor3D(nn.Module):
    def __init__(self, cfg, weights_center_detect="latest", weights_hybridnet="latest",
                 trt_mode="off", precision=None):
        super().__init__()
        # None: the process default (fp32 unless JH_PRECISION / set_precision says otherwise)
        self.precision = precision_for_trt_mode(trt_mode, precision)
        self.trt_mode = trt_mode
        self.cfg = cfg
        self.centerDetect = EfficientTrack("CenterDetectInference", cfg, weights_center_detect).model
        self.hybridNet = HybridNet("inference", cfg, weights_hybridnet).model
        self.bbox_hw = int(cfg.KEYPOINTDETECT.BOUNDING_BOX_SIZE / 2)
        self.num_cameras = cfg.HYBRIDNET.NUM_CAMERAS
        self.bounding_box_size = cfg.KEYPOINTDETECT.BOUNDING_BOX_SIZE
        self.reproTool = ReprojectionTool()
        self.center_detect_img_size = int(cfg.CENTERDETECT.IMAGE_SIZE)
        self._native = {}
        self._tone = None                                    # the ToneTables in force (set_tone)

    def set_tone(self, tone):
        """tone: a ToneTables of NUM_CAMERAS cameras (tone.ToneTables: identity, from_bytes, from_curve), or None.  From
        now on every forward of byte frames -- uint8 BGR, YUV, surfaces, raw sensor and pixel surfaces -- replaces byte
        k of channel ch of camera c by tone.tables[c][ch][k] in place of k / 255 inside the resize / crop fetch: black
        level, gain, white balance and gamma without a host pass.  The result equals, bit for bit, forward() on the
        fp32 frames tables[c][ch][bytes].  It holds for every native predictor this object has or later makes
        (native(), native_streams()).  fp32 frames have no byte: forward() then raises RuntimeError ("tone tables apply
        to byte frames").  None: back to the plain form."""
        from ..tone import check_tone
        self._tone = check_tone(tone, self.num_cameras)
        for pr in self._native.values():
            pr.set_tone(self._tone)

    def _make_native(self, img_h, img_w, time_batch, cam_lo, cam_n):
        pr = self._make_native_plain(img_h, img_w, time_batch, cam_lo, cam_n)
        if self._tone is not None:
            pr.set_tone(self._tone)
        return pr

    def _make_native_plain(self, img_h, img_w, time_batch, cam_lo, cam_n):
        c = self.cfg
        return NativePredictor(
            flat_state(self.centerDetect), flat_state(self.hybridNet),
            num_cameras=self.num_cameras, num_joints=c.KEYPOINTDETECT.NUM_JOINTS,
            center_size=self.center_detect_img_size, bbox=self.bounding_box_size,
            roi_cube_size=c.HYBRIDNET.ROI_CUBE_SIZE, grid_spacing=c.HYBRIDNET.GRID_SPACING,
            img_h=img_h, img_w=img_w, mean=list(c.DATASET.MEAN), std=list(c.DATASET.STD),
            center_model=c.CENTERDETECT.MODEL_SIZE, kp_model=c.KEYPOINTDETECT.MODEL_SIZE,
            time_batch=time_batch, cam_lo=cam_lo, cam_n=cam_n, precision=self.precision)

    def _fresh_cache(self):
        """Native predictors hold packed copies of the weights: drop them when any of the
        sub-modules has been (re)loaded since they were built (load_state_dict into
        centerDetect / hybridNet / hybridNet.effTrack / hybridNet.v2vNet)."""
        fp = weights_fingerprint(self.centerDetect, self.hybridNet)
        if fp != getattr(self, "_native_fp", None):
            for pr in self._native.values():
                for q in getattr(pr, "preds", [pr]):
                    q.close()
            self._native = {}
            self._native_fp = fp
        return self._native

    def native(self, img_h, img_w, time_batch=1, cam_lo=0, cam_n=None):
        """The native predictor for a frame size (built on first use)."""
        self._fresh_cache()
        key = (img_h, img_w, time_batch, cam_lo, cam_n)
        pr = self._native.get(key)
        if pr is None:
            pr = self._native[key] = self._make_native(img_h, img_w, time_batch, cam_lo, cam_n)
        return pr

    def native_streams(self, img_h, img_w, time_batch, streams):
        """`streams` native predictors of that shape (own launch plans and buffers each) behind a
        MultiStreamPredictor: independent time batches in flight on `streams` HIP streams (the
        throughput form, see _predictor.MultiStreamPredictor)."""
        from .._predictor import MultiStreamPredictor
        self._fresh_cache()
        key = ("streams", img_h, img_w, time_batch, streams)
        msp = self._native.get(key)
        if msp is None:
            msp = self._native[key] = MultiStreamPredictor(
                lambda: self._make_native(img_h, img_w, time_batch, 0, None), streams=streams)
        return msp

    def _frame_mask(self, camera_mask):
        """camera_mask of the single-frame forms: (C,) -> (1,C) checked, or None."""
        m = N.camera_mask(camera_mask, (self.num_cameras,))
        return None if m is None else m.unsqueeze(0)

    def forward(self, imgs, cameraMatrices, intrinsicMatrices, distortionCoefficients, camera_mask=None,
                return_2d=False, centers=None, return_spread=False, return_triangulated=False, joint_mask=None):
        """imgs (C,3,H,W) RGB in [0,1] -> (points3D (1,J,3), confidences (1,J)) or (None, None).
        return_2d: a third element, the per-camera `Views2D` of this frame set (leading dimension 1: 2D keypoints of
        every camera from the heat maps this forward computed anyway, the reprojections of the 3D keypoints and
        their distance in pixels; see _single), or (None, None, None).
        camera_mask (C,) bool / integer tensor or sequence, host or device: the frame is computed as the reference
        computes it for the cameras with a nonzero entry alone, in their order (its `cameras_to_use` subset); what
        the other cameras' slots of `imgs` hold does not matter.  Fewer than two cameras left, or fewer than two of
        them detecting: (None, None).  None: all cameras.
        centers (3,) world millimetres, host or device: where the subject is -- the centroid of the previous result
        when tracking, a fixed volume, another detector's answer.  Stage 1 (resize, CenterDetect, arg-max,
        triangulation) then does not run: the crops and the voxel cube are placed around this centre, truncated and
        projected as the reference truncates and projects its triangulated one (jarvis3D.py:161-166,183).  The frame is
        valid iff the centre is finite and below 2^24 in magnitude (and, under camera_mask, a camera is left): there is
        no detection gate, so (None, None) means an unusable centre.  A centre taken from a detected call of the same
        frames, calibration and mask (native(...).debug("cuda")["center3d"]) gives that call's result bit for bit.
        A device tensor computed from the previous result costs no host synchronisation.  None: detect, as always.
        (weights_center_detect=None builds CenterDetect with its initial weights, as it always did; a predictor whose
        every call brings centres never runs it.)
        return_spread: a further element behind Views2D, (points3D, confidences[, views][, spread]): the `Spread3D` of
        the frame set (leading dimension 1), or None with the others.  Per joint, of the normalised heat map
        softplus(V2V output) whose mean is the keypoint: cov (1,J,3,3) its covariance in mm^2 from fp64 sums, peak
        (1,J,3) the voxel of its maximum in mm (the mode: |peak - point| beyond the spread means a multi-modal map),
        mass (1,J) its sum.  points3D and confidences keep their bits.
        return_triangulated (True = the library's defaults, or what _native.joints3d_params made, or a dict of its
        keywords): the last element, the `Triangulated3D` of the frame set (leading dimension 1), or None with the
        others: per joint a second 3D point triangulated from the cameras' own 2D keypoints (the arg-max of the heat
        maps this forward computed anyway, refined to sub-pixel position by the centroid of a (2 refine_radius + 1)^2
        window), with the cameras that disagree left out by a consensus over two-view triangulations -- the one 3D
        estimate that does not pass through the voxel cube: it still meets the rays of a limb outside ROI_CUBE_SIZE, it
        names the camera whose keypoint sits on a reflection (members), and it checks V2V independently of V2V.
        points3D and confidences keep their bits; it composes with everything above.
        joint_mask: every joint's voxel volume is averaged over that joint's own cameras, so a camera whose keypoint
        sits on a reflection or an occluder no longer drags that joint (it keeps counting for its good joints).  A
        (J,C) bool / integer tensor, host or device (nonzero = camera c counts for joint j; the `members` of a
        previous call's Triangulated3D is one); or 'consensus' / True: the members of this call's own per-joint
        consensus, computed between KeypointDetect and the voxel gather with the library's default parameters, so V2V
        runs once, on the cleaned volume; or a dict of _native.joints3d_params keywords, or what it made: the
        consensus with those.  camera_mask composes as joint_mask & camera_mask; a joint left without a camera falls
        back to the cameras of the call.  All ones gives the bits of the call without it.  The call runs plain
        launches (no graph replay).  The last element, behind the Triangulated3D, is the `JointMask` of the frame set
        (cameras (1,J,C), count (1,J): the sets that were used), or None with the others.  This says nothing about
        trained networks: whether the cleaned volume gives better keypoints is the user's to measure."""
        mask = self._frame_mask(camera_mask)
        centers = N.centers(centers, 1)                      # (3,) -> (1,3) checked, or None
        frames = N.describe_frames(imgs, (self.num_cameras,))
        self.reproTool.cameraMatrices = cameraMatrices
        self.reproTool.intrinsicMatrices = intrinsicMatrices
        self.reproTool.distortionCoefficients = distortionCoefficients
        return self._run(frames, (cameraMatrices, intrinsicMatrices, distortionCoefficients), mask, return_2d, True,
                         centers, return_spread, return_triangulated, joint_mask)

    def _run(self, frames, calib, mask, return_2d, single=False, centers=None, return_spread=False,
             return_triangulated=False, joint_mask=None, center_every=None):
        """The forward of checked frames (a _native.Frames; single: one frame set, lead (C,)) with a checked mask and
        checked centres (_native.centers for the frames' time batch, or None), on the native predictor of their size:
        nothing of the predictor is touched before this.  joint_mask: the argument as given (_native.joint_mask checks
        it here, for the frames' time batch); center_every likewise (_native.center_every; the batched forms only)."""
        check_native_seam(self)
        keys = N.center_every(center_every, frames.lead[0])
        if keys is not None and centers is not None:
            raise ValueError("centers= and center_every= do not combine: a call either brings its centres or detects "
                             "them on its key rows")
        tri = N.triangulation_params(return_triangulated)   # (True: the defaults; None: not asked for)
        per_frame = False
        if single:
            frames = frames._replace(lead=(1,) + frames.lead, data=frames.data.unsqueeze(0))
        else:
            # the batched forms take one calibration for the batch, (C,...), or one per frame set, (T,C,...)
            per_frame = N.calibration(tuple(calib), frames.lead[0], self.num_cameras)[0] == "frames"
        jm = None
        if joint_mask is not None:
            jm = N.joint_mask(joint_mask, frames.lead[0], self.cfg.KEYPOINTDETECT.NUM_JOINTS, self.num_cameras)
        pr = self.native(frames.height, frames.width, time_batch=frames.lead[0])
        (pr.set_calibration_frames if per_frame else pr.set_calibration)(*calib)
        # (return_spread and joint_mask decide for this call alone: the native predictor sets its flags, on or off,
        # before it runs)
        res = pr._forward(frames, None, mask, centers, *((True,) if return_spread else ()),
                          **({} if jm is None else {"joint_mask": jm}),
                          **({} if keys is None else {"center_keys": keys}))
        used = ()
        if keys is not None:                                 # (the CenterKeyframes comes last of all)
            res, used = tuple(res[:-1]), (res[-1],)
        if jm is not None:                                   # (the JointMask comes behind the Triangulated3D)
            res, used = tuple(res[:-1]), (res[-1],) + used
        return self._single(pr, res, mask, return_2d, tri, used) if single else \
            self._batch(pr, res, mask, return_2d, tri, used)

    @staticmethod
    def _single(pr, res, mask, return_2d, tri=None, used=()):
        """The single-frame forms' return value: (points3D, confidences[, Views2D][, Spread3D][, Triangulated3D]), every
        element None when fewer than two cameras saw the subject (jarvis3D.py:157,187-190).  The 2D views and the
        triangulation (tri: its checked parameters) are enqueued behind the forward, before the one host
        synchronisation (reading the validity flag).  used: the call's JointMask, which comes last.
        Views2D are HybridNet's own 2D detections, on the crop around the projection of the TRIANGULATED centre;
        JarvisPredictor2D crops around each camera's own centre detection.  The two agree wherever the crops cover
        the subject; they are not bit-equal."""
        points, conf, valid = res[:3]
        extra = ((pr.views2d(points, camera_mask=mask),) if return_2d else ()) + tuple(res[3:])
        if tri is not None:
            extra += (pr.triangulate_joints(camera_mask=mask, params=tri),)
        extra += tuple(used)
        if int(valid[0].item()) == 0:
            return (None, None) + (None,) * len(extra)
        return (points, conf) + extra

    def forward_uint8(self, imgs_bgr, cameraMatrices, intrinsicMatrices, distortionCoefficients, camera_mask=None,
                      return_2d=False, centers=None, return_spread=False, return_triangulated=False,
                      joint_mask=None):
        """imgs_bgr (C,H,W,3) uint8 BGR exactly as the video decoder delivers them
        (predict3D.py:72-78).  Same result as forward() on
        `imgs_bgr.float().permute(0,3,1,2)[:, [2,1,0]] / 255.` (predict3D.py:79-80); the
        conversion runs inside the resize / crop kernels.  camera_mask, return_2d, centers, return_spread,
        return_triangulated: as forward() -- the Spread3D (covariance in mm^2, peak voxel in mm and mass of every joint's
        heat map), then the Triangulated3D come last."""
        mask = self._frame_mask(camera_mask)
        centers = N.centers(centers, 1)                      # (3,) -> (1,3) checked, or None
        frames = N.describe_frames(imgs_bgr, (self.num_cameras,), "bgr")
        return self._run(frames, (cameraMatrices, intrinsicMatrices, distortionCoefficients), mask, return_2d, True,
                         centers, return_spread, return_triangulated, joint_mask)

    def forward_yuv(self, frames, frame_format, cameraMatrices, intrinsicMatrices, distortionCoefficients,
                    camera_mask=None, return_2d=False, centers=None, return_spread=False,
                    return_triangulated=False, joint_mask=None):
        """frames (C,3H/2,W) uint8 YUV 4:2:0 as video decoders produce them natively, frame_format 'i420'
        (FFmpeg yuv420p: Y, U, V planes) or 'nv12' (Y plane, interleaved UV plane); H and W even.  Same result,
        bit for bit, as forward_uint8 on the BGR bytes of cv2.cvtColor(COLOR_YUV2BGR_I420 / _NV12) of each
        image (BT.601 limited range); the conversion runs inside the resize / crop kernels.
        -> (points3D (1,J,3), confidences (1,J)) or (None, None).  camera_mask, return_2d, centers, return_spread,
        return_triangulated: as forward() -- the Spread3D (covariance in mm^2, peak voxel in mm and mass of every joint's
        heat map), then the Triangulated3D come last."""
        mask = self._frame_mask(camera_mask)
        centers = N.centers(centers, 1)                      # (3,) -> (1,3) checked, or None
        frames = N.describe_frames(frames, (self.num_cameras,), N.yuv_format(frame_format))
        return self._run(frames, (cameraMatrices, intrinsicMatrices, distortionCoefficients), mask, return_2d, True,
                         centers, return_spread, return_triangulated, joint_mask)

    def forward_surface(self, frames, surface, cameraMatrices, intrinsicMatrices, distortionCoefficients,
                        camera_mask=None, return_2d=False, centers=None, return_spread=False,
                        return_triangulated=False, joint_mask=None):
        """frames (C,image_stride) uint8: one YUV 4:2:0 image per camera, read in place through the YuvSurface
        `surface` (pitched decoder surfaces, I420 / YV12 / NV12 / NV21, BT.601 / BT.709, limited / full range), or one
        raw sensor image per camera through the SensorSurface `surface` (Mono8, or an 8-bit Bayer mosaic demosaiced
        bilinearly on the GPU; pitched buffers with a header in front likewise), or one image per camera through the
        PixelSurface `surface` (RGB in any byte order, 4-byte and planar RGB, grey, YUYV / UYVY, planar and semi-planar
        YUV 4:2:2 / 4:4:4 / 4:4:0 / 4:1:1): frames (C,image_stride), or any (C,...) with exactly image_stride bytes per
        camera -- (C,H,W,3), (C,H,W,4) and (C,3,H,W) tensors go in as they are.
        Same result, bit for bit, as forward_uint8 on the BGR bytes the surface's conversion gives
        (include/jarvis_hip.h); bytes outside the planes are never read.
        -> (points3D (1,J,3), confidences (1,J)) or (None, None).  camera_mask, return_2d, centers, return_spread,
        return_triangulated: as forward() -- the Spread3D (covariance in mm^2, peak voxel in mm and mass of every joint's
        heat map), then the Triangulated3D come last."""
        mask = self._frame_mask(camera_mask)
        centers = N.centers(centers, 1)                      # (3,) -> (1,3) checked, or None
        frames = N.describe_frames(frames, (self.num_cameras,), None, N.surface(surface))
        return self._run(frames, (cameraMatrices, intrinsicMatrices, distortionCoefficients), mask, return_2d, True,
                         centers, return_spread, return_triangulated, joint_mask)

    def forward_batch(self, imgs, cameraMatrices, intrinsicMatrices, distortionCoefficients, frame_format=None,
                      camera_mask=None, return_2d=False, frame_layout=None, centers=None, return_spread=False,
                      return_triangulated=False, joint_mask=None, center_every=None):
        """Throughput form: imgs (T,C,3,H,W) fp32 RGB or (T,C,H,W,3) uint8 BGR,
        independent time steps -> points (T,J,3), confidences (T,J), valid (T) int32;
        no host synchronisation.  frame_format 'i420' / 'nv12': imgs (T,C,3H/2,W) uint8 YUV 4:2:0 (see
        forward_yuv); 'bgr': uint8 BGR required; None: the dtype decides.
        camera_mask (T,C) bool / integer, host or device: row t names the cameras frame set t uses (see forward());
        a row with fewer than two cameras gives valid[t] = 0.  Rows are independent: a frame set's result depends on
        its own mask row only.  None: all cameras.
        return_2d: the per-camera `Views2D` of the batch (leading dimension T; see forward()) follows `valid`:
        (points, confidences, valid, views).  Rows of invalid frames: used 0, points2D -1, NaN reprojections.
        frame_layout: a YuvSurface, a SensorSurface or a PixelSurface -- imgs (T,C,image_stride) uint8 (a PixelSurface:
        any (T,C,...) with exactly image_stride bytes per image), see forward_surface; not together with frame_format
        'i420' / 'nv12'.
        Calibration: cameraMatrices (C,4,3), intrinsicMatrices (C,3,3), distortionCoefficients (C,1,5) -- one
        calibration shared by the T frame sets --, or the same three with a leading T -- (T,C,4,3) / (T,C,3,3) /
        (T,C,1,5), row t the calibration of frame set t, as the reference's validation analysis gives every sample the
        calibration of its own dataset (analysis/analyze.py).  All three in one form (ValueError otherwise).  Row t of
        the result under per-frame calibration equals, bit for bit, row t of the same batch run with row t's
        calibration shared; camera_mask and return_2d compose with either form (the reprojections of row t use row
        t's calibration).  The single-frame forms (forward, forward_uint8, forward_yuv, forward_surface) take (C,...).
        centers (T,3) world millimetres, host or device: row t is the centre of frame set t and stage 1 does not run
        (see forward()).  valid[t] = 1 iff row t is finite and below 2^24 in magnitude (and, under camera_mask, a
        camera of row t is left); rows are independent.  Centres taken from a detected run of the same batch
        (native(...).debug("cuda")["center3d"]) give that run bit for bit -- points, confidences, valid and the 2D
        views -- wherever it is valid.  It composes with camera_mask, return_2d, every frame format and per-frame-set
        calibration (row t's centre is projected with row t's calibration).  None: detect.
        return_spread: the `Spread3D` of the batch comes last, (points, confidences, valid[, views], spread): per joint
        the covariance cov (T,J,3,3) in mm^2 of the normalised heat map softplus(V2V output) (fp64 sums, rounded once),
        the voxel of its maximum peak (T,J,3) in mm and its sum mass (T,J); NaN rows where valid[t] = 0.  The other
        outputs keep their bits; it composes with everything above.
        return_triangulated: the `Triangulated3D` of the batch comes last (see forward()): points (T,J,3), views (T,J),
        members (T,J,C), error (T,J), observations (T,C,J,3); NaN / 0 rows where valid[t] = 0 and for a joint on which
        fewer than min_views cameras agree.  Under per-frame-set calibration row t uses row t's calibration.
        joint_mask: as forward(), (T,J,C) for a tensor; row t of the batch depends on row t of the mask alone, and an
        invalid frame set is as in the plain call.  The `JointMask` of the batch (cameras (T,J,C), count (T,J)) comes
        last.  `Triangulated3D.members` of one call is a valid joint_mask of the next.
        center_every = k (an int >= 1), or (k, n_rows): the rows of the batch are CONSECUTIVE frame sets, and CenterDetect
        runs on the key rows alone -- rows 0, k, 2k, ... and the last one (_native.center_keyframe_rows) --; a row in
        between takes the centre interpolated linearly, on the device, between its two key rows (one of them invalid:
        the other one's; both: the row is invalid), and every row then runs as under centers= (include/jarvis_hip.h has
        the definition).  (k, n_rows): only the first n_rows rows are real (a padded last group); the rows behind them
        hold the last real row's centre and never serve as keys.  The `CenterKeyframes` of the call (centers (T,3),
        source (T): 0 detected, 1 interpolated, 2 held, -1 none) comes last of all.  k = 1 gives the detected call bit
        for bit; any k gives, bit for bit, forward_batch(centers=CenterKeyframes.centers).  The flag decides for this
        call alone; it composes with everything above except centers= (ValueError).  None: every row detects.  Whether
        a trained network keeps its accuracy under a given k is the user's to measure."""
        if centers is not None and center_every is not None:
            raise ValueError("centers= and center_every= do not combine: a call either brings its centres or detects "
                             "them on its key rows")
        if centers is not None:
            if not torch.is_tensor(imgs) or imgs.dim() < 1:
                raise ValueError("imgs must be a tensor of time steps")
            centers = N.centers(centers, imgs.shape[0])
        if camera_mask is not None:
            if not torch.is_tensor(imgs) or imgs.dim() < 1:
                raise ValueError("imgs must be a tensor of time steps")
            camera_mask = N.camera_mask(camera_mask, (imgs.shape[0], self.num_cameras))
        frames = N.describe_frames(imgs, (None, self.num_cameras), frame_format, frame_layout)
        return self._run(frames, (cameraMatrices, intrinsicMatrices, distortionCoefficients), camera_mask, return_2d,
                         centers=centers, return_spread=return_spread, return_triangulated=return_triangulated,
                         joint_mask=joint_mask, center_every=center_every)

    def forward_images(self, images, cameraMatrices, intrinsicMatrices, distortionCoefficients, frame_format=None,
                       frame_layout=None, camera_mask=None, return_2d=False, centers=None,
                       return_spread=False, return_triangulated=False, joint_mask=None, center_every=None):
        """forward_batch on images that lie where their producers left them: `images` a sequence of C tensors (one
        frame set) or a sequence of T such sequences, each tensor ONE image -- fp32 (3,H,W); uint8 (H,W,3);
        frame_format 'i420' / 'nv12': uint8 (3H/2,W); frame_layout (a YuvSurface or a SensorSurface): 1-D uint8 of at
        least image_stride bytes.  All of one shape, dtype and device, contiguous, on the GPU; any address (views
        into a decoder's surface pool included), the same tensor may appear more than once, and a masked camera's
        entry is still an image.  Nothing is gathered: the kernels read every image through its own pointer
        (jh_predictor_forward_images).
        -> what forward_batch returns for the (T,C,...) stack of the same images, bit for bit; no host
        synchronisation.  camera_mask (T,C), return_2d: as forward_batch.  Calibration: shared (C,...) or one per frame
        set (T,C,...), as forward_batch.
        centers (T,3): as forward_batch.  With the same images in several rows and one centre per row, the rows of a
        batch are different subjects seen in the same frames (a detected batch finds the strongest one in every row).
        return_spread, return_triangulated: as forward_batch -- the Spread3D of the batch (covariance in mm^2, peak voxel
        in mm and mass of every joint's heat map), then its Triangulated3D come last.  joint_mask: as forward_batch;
        its JointMask comes last.  center_every: as forward_batch; its CenterKeyframes comes last of all."""
        if centers is not None and center_every is not None:
            raise ValueError("centers= and center_every= do not combine: a call either brings its centres or detects "
                             "them on its key rows")
        frames = image_frames(self.num_cameras, images, frame_format, frame_layout)
        T = frames.lead[0]
        camera_mask = N.camera_mask(camera_mask, (T, self.num_cameras))
        return self._run(frames, (cameraMatrices, intrinsicMatrices, distortionCoefficients), camera_mask, return_2d,
                         centers=N.centers(centers, T), return_spread=return_spread,
                         return_triangulated=return_triangulated, joint_mask=joint_mask, center_every=center_every)

    def detect_subjects(self, imgs, cameraMatrices, intrinsicMatrices, distortionCoefficients, max_subjects,
                        frame_format=None, frame_layout=None, camera_mask=None, images=False, return_peaks=False,
                        tracker=None, **params):
        """Where the subjects are, for a time batch: imgs as forward_batch takes them -- or, with images=True, as
        forward_images takes them -- -> `Subjects` (centers (T,K,3) world mm, views (T,K), members (T,K,C), error
        (T,K); K = max_subjects), device tensors, no host synchronisation.
        CenterDetect runs once on the frames; instead of ONE maximum per camera the top `max_peaks` local maxima of
        every camera's heat map are kept (maxima of their (2 nms_radius + 1)^2 window above `min_peak`), grouped
        across cameras by reprojection consistency (a group's peaks lie within `max_error_px` full-frame pixels of the
        projection of the point two of them triangulate; at least `min_views` cameras), most views first, and every
        group is triangulated with the arithmetic of the detected forward.  **params: max_peaks, nms_radius, min_views,
        min_peak, max_error_px (_native.subjects_params: the library's defaults 50 / 4 / 2 / 24 are defaults, not
        recommendations).  An empty subject has NaN centres, views 0, members -1.
        camera_mask (T,C), frame_format, frame_layout, per-frame-set calibration (T,C,...): as forward_batch.
        return_peaks: (subjects, peaks (T,C,max_peaks,3) = (x, y, value) in heat-map pixels).
        A centre goes back in as `centers=` of forward_batch / forward_images (forward_subjects does that).  Robust
        single-subject detection is max_subjects=1: the cameras whose maximum lies on something else are left out of
        the triangulation instead of dragging it.
        tracker: a tracks.SubjectTracker of max_subjects slots.  Without one, subject k of frame set t and of t+1 are
        unrelated.  With one, the Subjects come back in SLOT order -- slot k is the same animal from frame set to frame
        set and from call to call, as far as nearest-first matching under the tracker's gate can tell -- and a `Tracks`
        (ids, slots, missed, dropped) follows, behind `peaks` when those are asked for: (subjects[, peaks], tracks).
        The tracker's kernel runs behind the detection on the same stream: still no host synchronisation.
        Not covered: JarvisPredictor2D, analyze_frames and the camera-sharded path (the driver: predict3D_frames(...,
        max_subjects=))."""
        check_native_seam(self)
        p = N.subjects_params(max_subjects, **params)
        check_tracker(tracker, max_subjects)
        if images:
            frames = image_frames(self.num_cameras, imgs, frame_format, frame_layout)
        else:
            frames = N.describe_frames(imgs, (None, self.num_cameras), frame_format, frame_layout)
        T = frames.lead[0]
        mask = N.camera_mask(camera_mask, (T, self.num_cameras))
        calib = (cameraMatrices, intrinsicMatrices, distortionCoefficients)
        per_frame = N.calibration(calib, T, self.num_cameras)[0] == "frames"
        pr = self.native(frames.height, frames.width, time_batch=T)
        (pr.set_calibration_frames if per_frame else pr.set_calibration)(*calib)
        res = pr.detect_subjects(frames, p, mask, return_peaks)
        if tracker is None:
            return res
        subjects, tracks = tracker.update(res[0] if return_peaks else res)
        return (subjects, res[1], tracks) if return_peaks else (subjects, tracks)

    def forward_subjects(self, imgs, cameraMatrices, intrinsicMatrices, distortionCoefficients, max_subjects,
                         frame_format=None, frame_layout=None, camera_mask=None, images=False, return_2d=False,
                         return_spread=False, return_triangulated=False, tracker=None, joint_mask=None, **params):
        """Several subjects in one time batch: detect_subjects, then one centred forward_batch (images=True:
        forward_images) per subject k on the same frames with centers=subjects.centers[:, k].
        -> points (T,K,J,3), confidences (T,K,J), valid (T,K) int32, subjects[, views][, spreads]: row (t, k) is row t
        of that centred call, bit for bit; an empty subject (NaN centre) is an invalid row, valid 0.  return_2d /
        return_spread / return_triangulated: a tuple of K Views2D / Spread3D / Triangulated3D, one per subject, follows,
        in that order.  camera_mask and the other arguments: as detect_subjects.  No host synchronisation.
        tracker (a tracks.SubjectTracker, see detect_subjects): the subjects are put into slot order first and the
        centred forwards run on the tracked centres, so k is a slot -- one animal -- in every output; the `Tracks` comes
        last.  Row (t, k) is then row (t, tracks.slots[t, k]) of the call without a tracker, bit for bit, and an invalid
        row where the slot holds no detection (with coast=True: the forward at the track's predicted centre).
        joint_mask: passed to each centred forward (as forward_batch); a tuple of K JointMasks follows the other
        per-subject tuples."""
        calib = (cameraMatrices, intrinsicMatrices, distortionCoefficients)
        subjects = self.detect_subjects(imgs, *calib, max_subjects, frame_format=frame_format, tracker=tracker,
                                        frame_layout=frame_layout, camera_mask=camera_mask, images=images, **params)
        tracks = ()
        if tracker is not None:
            subjects, tracks = subjects[0], subjects[1:]
        rows = []
        for k in range(max_subjects):
            kw = dict(frame_format=frame_format, frame_layout=frame_layout, camera_mask=camera_mask,
                      return_2d=return_2d, centers=subjects.centers[:, k], return_spread=return_spread,
                      return_triangulated=return_triangulated, joint_mask=joint_mask)
            rows.append((self.forward_images if images else self.forward_batch)(imgs, *calib, **kw))
        out = tuple(torch.stack([r[i] for r in rows], 1) for i in range(3)) + (subjects,)
        for i in range(3, len(rows[0])):             # (views, spreads, triangulations, joint masks: one per subject)
            out += (tuple(r[i] for r in rows),)
        return out + tracks

    @staticmethod
    def _batch(pr, res, mask, return_2d, tri=None, used=()):
        # (points, conf, valid[, views][, spread][, triangulated][, joint mask]): the Spread3D, when asked for, is res[3]
        if return_2d:
            res = tuple(res[:3]) + (pr.views2d(res[0], camera_mask=mask),) + tuple(res[3:])
        if tri is not None:
            res = tuple(res) + (pr.triangulate_joints(camera_mask=mask, params=tri),)
        return tuple(res) + tuple(used) if used else res
