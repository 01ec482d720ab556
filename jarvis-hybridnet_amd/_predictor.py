"""Python handle of the native predictor (jh_predictor_* in include/jarvis_hip.h)."""
import collections
import ctypes

import torch

from . import _native as N
from . import arch
from .joint_mask import JointMask
from .spread import Spread3D  # noqa: F401 -- the name the forwards return
from .subjects import Subjects
from .tone import check_tone
from .tracks import check_tracker
from .triangulated import Triangulated3D


# Per-camera 2D views of a 3D result (jh_predictor_views2d, include/jarvis_hip.h): points2D (T,C,J,2) int32 full-frame
# pixels, confidences2D (T,C,J), reprojections (T,C,J,2) of the 3D keypoints, errors (T,C,J) = their distance to
# points2D in pixels, used (T,C) uint8.  A camera that is not used (masked, or an invalid frame) has points2D -1,
# confidences2D 0, errors NaN; an invalid frame has NaN reprojections too.
Views2D = collections.namedtuple("Views2D", "points2D confidences2D reprojections errors used")

# What a centre-keyframe call placed its rows by (jh_predictor_get_center_keyframes, include/jarvis_hip.h): centers (T,3)
# fp32 world millimetres, NaN where the row has none; source (T) int32: 0 detected (a valid key row), 1 interpolated
# between its two key rows, 2 held (one neighbouring key row's centre; a padding row), -1 none.
CenterKeyframes = collections.namedtuple("CenterKeyframes", "centers source")


class NativePredictor:
    """Owns the launch plans of CenterDetect, KeypointDetect and V2V plus all
    intermediates for `time_batch` multi-view frames of a fixed size."""

    def __init__(self, center_state, hybrid_state, *, num_cameras, num_joints, center_size, bbox,
                 roi_cube_size, grid_spacing, img_h, img_w, mean, std, center_model="small",
                 kp_model="small", time_batch=1, time_batch_3d=0, cam_lo=0, cam_n=None, precision=None):
        """precision: "f32" | "bf16x3" | "bf16x3_wide" for THIS predictor, or None = the process default
        (`_native.set_precision`, environment JH_PRECISION) at creation time."""
        cam_n = num_cameras if cam_n is None else cam_n
        cfg = N.PredictorConfig(
            num_cameras, num_joints, center_size, bbox, float(roi_cube_size), float(grid_spacing),
            arch.SIZE_IDS[center_model], arch.SIZE_IDS[kp_model], img_h, img_w, time_batch,
            time_batch_3d, cam_lo, cam_n, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std),
            N.precision_id(precision))
        self.cfg = cfg
        self.T, self.C, self.Cloc, self.J = time_batch, num_cameras, cam_n, num_joints
        self.T3 = time_batch_3d if time_batch_3d > 0 else time_batch
        self.Jp = (num_joints + 7) // 8 * 8
        self.Hh = bbox // 2
        self.handle = ctypes.c_void_p()
        pc = N.Params(center_state) if center_state is not None else None
        # (kept: the first set_center_keyframes call of an `every` hands CenterDetect's parameters over again)
        self._center_state = center_state
        ph = N.Params(hybrid_state)
        N.check(N.lib().jh_predictor_create(pc.handle if pc else None, ph.handle,
                                            ctypes.byref(cfg), ctypes.byref(self.handle)))
        self.precision = {v: k for k, v in N.PRECISIONS.items()}[N.lib().jh_predictor_precision(self.handle)]
        self.launches = N.lib().jh_predictor_launches(self.handle)
        self.device_bytes = N.lib().jh_predictor_device_bytes(self.handle)
        self._centred = False                        # centres are in force (set_centers)
        self._spread = False                         # the 3D stage runs the spread form of its tail (set_spread)
        self._joint_masked = False                   # a joint mask is in force (set_joint_mask)
        self._toned = False                          # tone tables are in force (set_tone)
        self._keyframed = False                      # centre keyframes are in force (set_center_keyframes)
        self._key_slots = 0                          # the key slots the predictor's key plan was built for (0: none)

    def close(self):
        if getattr(self, "handle", None) and N is not None and N._lib is not None:
            N.lib().jh_predictor_destroy(self.handle)
            self.handle = None

    __del__ = close

    # ---- graph replay of the whole forward (default: on for time_batch == 1) ---
    @property
    def graph_replay(self):
        return bool(N.lib().jh_predictor_graph_replay(self.handle))

    @graph_replay.setter
    def graph_replay(self, on):
        N.check(N.lib().jh_predictor_set_graph_replay(self.handle, int(bool(on))))

    @property
    def graph_records(self):
        """How many times a whole-path forward has been recorded so far: a call that replays adds none."""
        return int(N.lib().jh_predictor_graph_records(self.handle))

    # ---- calibration -----------------------------------------------------
    def set_calibration(self, cam, intr, dist):
        N.check(N.lib().jh_predictor_set_calibration(
            self.handle, N.ptr(N.dev(cam)), N.ptr(N.dev(intr)), N.ptr(N.dev(dist)), N.stream()))

    def set_calibration_frames(self, cam, intr, dist):
        """One calibration per frame set of the time batch: cam (T,C,4,3), intr (T,C,3,3), dist (T,C,1,5) device
        tensors, row t for frame set t (jh_predictor_set_calibration_frames; copied on the current stream).  Every
        later call of this predictor reads row t for frame set t until set_calibration() returns it to the shared
        form.  Row t of a result equals, bit for bit, row t of the same batch under set_calibration(row t)."""
        form, cam, intr, dist = N.calibration((cam, intr, dist), self.T, self.C)
        if form != "frames":
            raise ValueError("set_calibration_frames takes (%d, %d, 4, 3) / (%d, %d, 3, 3) / (%d, %d, 1, 5) tensors; "
                             "got %s" % (self.T, self.C, self.T, self.C, self.T, self.C, tuple(cam.shape)))
        N.check(N.lib().jh_predictor_set_calibration_frames(
            self.handle, N.ptr(N.dev(cam)), N.ptr(N.dev(intr)), N.ptr(N.dev(dist)), N.stream()))

    # ---- caller-supplied centres ------------------------------------------
    def set_centers(self, centers):
        """centers (T,3), world millimetres, host or device (_native.centers; (3,) too at time_batch 1): from now on
        every forward of this predictor skips stage 1 -- resize, CenterDetect, arg-max, triangulation -- and puts the
        crops and the voxel cube of frame set t where row t says (jh_predictor_set_centers; copied on the current
        stream).  None: back to detection; a predictor that holds no centres is not called at all.
        valid[t] = 1 iff row t is finite and below 2^24 in magnitude (and, under a camera mask, a camera of the row is
        unmasked); there is no detection gate.  Centres taken from debug()["center3d"] of a detected call reproduce
        that call bit for bit."""
        centers = N.centers(centers, self.T)
        if centers is None:
            if self._centred:
                N.check(N.lib().jh_predictor_set_centers(self.handle, None, N.stream()))
                self._centred = False
            return
        dev = centers.to("cuda", non_blocking=True)
        N.check(N.lib().jh_predictor_set_centers(self.handle, N.ptr(dev), N.stream()))
        dev.record_stream(torch.cuda.current_stream())          # (copied by the call: free once it is enqueued)
        self._centred = True

    # ---- centre keyframes ---------------------------------------------------
    def set_center_keyframes(self, every, n_rows=None):
        """every = k >= 1: from now on every forward of this predictor runs CenterDetect on the key rows of its time
        batch alone -- rows 0, k, 2k, ... and the last real one (_native.center_keyframe_rows) -- and gives the rows in
        between a centre interpolated on the device between their two key rows; every row then runs the centred stage 2
        and 3 (jh_predictor_set_center_keyframes has the definition).  n_rows: how many leading rows of the batch are
        real (default: all); the padding rows behind them hold the last real row's centre and never serve as keys.
        None / 0: off; a predictor that holds none is not called at all.  The first call of an `every` builds a second
        CenterDetect plan for the key rows (not inside a stream capture; device_bytes grows); with every = 1 the result
        equals the detected one bit for bit.  The library refuses (RuntimeError) every < 0, n_rows outside 1 .. T, a
        predictor without CenterDetect weights and one that does not own all cameras."""
        if not every:
            if self._keyframed:
                N.check(N.lib().jh_predictor_set_center_keyframes(self.handle, None, 0, 0, N.stream()))
                self._keyframed = False
            return
        every, n_rows = int(every), self.T if n_rows is None else int(n_rows)
        slots = N.lib().jh_center_keyframe_rows(self.T, every, self.T, None, 0)      # (-1: the library refuses below)
        params = None
        if slots != self._key_slots and self._center_state is not None:
            params = N.Params(self._center_state)
        N.check(N.lib().jh_predictor_set_center_keyframes(self.handle, params.handle if params else None, every,
                                                          n_rows, N.stream()))
        self._keyframed, self._key_slots = True, slots
        self.device_bytes = N.lib().jh_predictor_device_bytes(self.handle)

    def center_keyframes(self):
        """The centres the last keyframe call placed its rows by and where each came from -> CenterKeyframes of device
        tensors, copied on the current stream (jh_predictor_get_center_keyframes)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        out = CenterKeyframes(torch.empty((self.T, 3), device=dev),
                              torch.empty((self.T,), device=dev, dtype=torch.int32))
        N.check(N.lib().jh_predictor_get_center_keyframes(self.handle, N.ptr(out.centers), N.ptr(out.source),
                                                          N.stream()))
        return out

    # ---- per-camera tone tables --------------------------------------------
    def set_tone(self, tone):
        """tone: a ToneTables of num_cameras cameras (all of them, also on a camera-sharded predictor), or an array it
        accepts: from now on every call of this predictor that fetches byte frames replaces byte k of channel ch of
        camera c by tone.tables[c][ch][k] in place of k / 255 (jh_predictor_set_tone; copied on the current stream; the
        first such call allocates the buffer: not inside a stream capture).  fp32 frames are then refused
        (RuntimeError "tone tables apply to byte frames").  None: back to the plain form."""
        tone = check_tone(tone, self.C)
        if tone is None:
            if self._toned:
                N.check(N.lib().jh_predictor_set_tone(self.handle, None, N.stream()))
                self._toned = False
            return
        dev = torch.tensor(tone.tables).to("cuda")
        N.check(N.lib().jh_predictor_set_tone(self.handle, N.ptr(dev), N.stream()))
        dev.record_stream(torch.cuda.current_stream())          # (copied by the call: free once it is enqueued)
        self._toned = True
        self.device_bytes = N.lib().jh_predictor_device_bytes(self.handle)

    # ---- per-joint 3D spread ----------------------------------------------
    def set_spread(self, on):
        """From the next call on the 3D stage (forward and the staged calls alike) also leaves the per-joint spread
        in the predictor's own buffers (jh_predictor_set_spread; the first enabling call allocates them: not inside a
        stream capture); points, conf and valid keep their bits.  Read it with spread()."""
        if bool(on) != self._spread:
            N.check(N.lib().jh_predictor_set_spread(self.handle, int(bool(on))))
            self._spread = bool(on)
            self.device_bytes = N.lib().jh_predictor_device_bytes(self.handle)

    def spread(self, out=None):
        """The spread of the last forward / stage_3d made with the spread enabled -> Spread3D of device tensors, copied
        on the current stream (jh_predictor_get_spread).  Enables the spread on first use, so before the staged calls
        (stage_3d ...) whose spread is wanted call it, or set_spread(True), once; forward() and forward_images() set
        the flag themselves, from their return_spread, on every call.  out: a Spread3D to write into."""
        self.set_spread(True)
        dev = torch.device("cuda", torch.cuda.current_device())
        cov6 = torch.empty((self.T, self.J, 6), device=dev)
        peak = torch.empty((self.T, self.J, 3), device=dev) if out is None else out.peak
        mass = torch.empty((self.T, self.J), device=dev) if out is None else out.mass
        N.check(N.lib().jh_predictor_get_spread(self.handle, N.ptr(cov6), N.ptr(peak), N.ptr(mass), N.stream()))
        # xx xy xz yy yz zz mirrored into the symmetric 3 x 3: slices, no index tensor (an index made from a list is a
        # synchronous upload, which would stall every stream of a MultiStreamPredictor)
        xx, xy, xz, yy, yz, zz = cov6.unbind(-1)
        cov = torch.stack((xx, xy, xz, xy, yy, yz, xz, yz, zz), -1).reshape(self.T, self.J, 3, 3)
        if out is not None:
            out.cov.copy_(cov)
            cov = out.cov
        return Spread3D(cov, peak, mass)

    # ---- per-joint camera masks --------------------------------------------
    def set_joint_mask(self, joint_mask):
        """joint_mask: what _native.joint_mask made, or None.  From now on every forward of this predictor gathers every
        joint's voxel volume from that joint's own cameras (jh_predictor_set_joint_mask; a given mask is copied on the
        current stream; the first such call allocates the buffers: not inside a stream capture) and runs plain
        launches; None: back to the plain forward and its graph replay."""
        if joint_mask is None:
            if self._joint_masked:
                N.check(N.lib().jh_predictor_set_joint_mask(self.handle, N.JOINT_MASK_OFF, None, None, N.stream()))
                self._joint_masked = False
            return
        mode, what = joint_mask
        if mode == N.JOINT_MASK_GIVEN:
            dev = what.to("cuda", non_blocking=True)
            N.check(N.lib().jh_predictor_set_joint_mask(self.handle, mode, N.ptr(dev), None, N.stream()))
            dev.record_stream(torch.cuda.current_stream())      # (copied by the call: free once it is enqueued)
        else:
            N.check(N.lib().jh_predictor_set_joint_mask(self.handle, mode, None, ctypes.byref(what), N.stream()))
        self._joint_masked = True

    def joint_mask(self):
        """The effective camera sets of the last joint-masked forward / stage_3d -> JointMask of device tensors, copied
        on the current stream (jh_predictor_get_joint_mask)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        out = JointMask(torch.empty((self.T, self.J, self.C), device=dev, dtype=torch.uint8),
                        torch.empty((self.T, self.J), device=dev, dtype=torch.int32))
        N.check(N.lib().jh_predictor_get_joint_mask(self.handle, N.ptr(out.cameras), N.ptr(out.count), N.stream()))
        return out

    def debug_v2v(self, device):
        """The V2V output of the last 3D chunk, (T3,J,Gh,Gh,Gh): what the soft-argmax tail read (jh_predictor_debug_v2v)."""
        Gh = int(self.cfg.roi_cube_size / self.cfg.grid_spacing) // 2
        out = torch.empty((self.T3, self.J, Gh, Gh, Gh), device=device)
        N.check(N.lib().jh_predictor_debug_v2v(self.handle, N.ptr(out), N.stream()))
        return out

    # ---- single-GPU forward ----------------------------------------------
    def forward(self, frames, out=None, frame_format=None, camera_mask=None, frame_layout=None, centers=None,
                return_spread=False, joint_mask=None, center_every=None):
        """frames (T,C,3,H,W) fp32 RGB, or (T,C,H,W,3) uint8 BGR as decoded, or with frame_format 'i420' / 'nv12'
        (T,C,3H/2,W) uint8 YUV 4:2:0 -> points (T,J,3), conf (T,J), valid (T) int32.  frame_format None: the
        dtype decides between fp32 RGB and uint8 BGR; 'bgr' requires uint8 BGR.
        camera_mask (T,C) bool / integer, host or device: frame t uses the cameras with a nonzero entry only
        (jh_predictor_forward_masked); None: all cameras, the unmasked entry points.
        frame_layout: a YuvSurface -- frames (T,C,image_stride) uint8, each image a YUV 4:2:0 surface read through
        that description (jh_predictor_forward_surface) --, or a SensorSurface -- each image a raw Mono8 / Bayer
        sensor image (jh_predictor_forward_sensor); not together with frame_format 'i420' / 'nv12'.
        centers (T,3): this call runs from these centres (set_centers); None: it detects -- centres set earlier are
        cleared first.
        return_spread: the Spread3D of this call follows valid: (points, conf, valid, spread).  The flag is set before
        the call (set_spread) and decides for this call alone; points, conf and valid keep their bits.
        joint_mask (_native.joint_mask: a (T,J,C) mask, 'consensus', or joints3d_params keywords): every joint's
        voxel volume is averaged over that joint's own cameras and the call's JointMask comes last; None: the plain
        forward -- a joint mask set earlier is cleared first.
        center_every (k, or (k, n_rows); _native.center_every): this call detects on its key rows only
        (set_center_keyframes) and its CenterKeyframes comes last of all; None: every row detects -- keyframes set
        earlier are cleared first.  Not together with centers (ValueError)."""
        return self._forward(self._describe(frames, frame_format, frame_layout), out,
                             N.camera_mask(camera_mask, (self.T, self.C)), N.centers(centers, self.T), return_spread,
                             N.joint_mask(joint_mask, self.T, self.J, self.C), N.center_every(center_every, self.T))

    def forward_images(self, frames, out=None, camera_mask=None, centers=None, return_spread=False, joint_mask=None,
                       center_every=None):
        """forward() on T * C separately placed images: `frames` what _native.frame_images made of the flat list
        (index t * C + c) (jh_predictor_forward_images).  The images are read where they lie; nothing is gathered."""
        if len(frames.images) != self.T * self.C:
            raise ValueError("expected %d images (time_batch * num_cameras), got %d" % (self.T * self.C,
                                                                                         len(frames.images)))
        return self._forward(frames, out, N.camera_mask(camera_mask, (self.T, self.C)), N.centers(centers, self.T),
                             return_spread, N.joint_mask(joint_mask, self.T, self.J, self.C),
                             N.center_every(center_every, self.T))

    def _describe(self, frames, frame_format=None, frame_layout=None):
        """Raw pointers cross the C ABI: refuse anything whose bytes would be misread (_native.describe_frames for
        this predictor's time batch, local cameras and frame size; the frames are read in place)."""
        return N.describe_frames(frames, (self.T, self.Cloc), frame_format, frame_layout,
                                 (self.cfg.img_h, self.cfg.img_w), error=RuntimeError, in_place=True)

    def _forward(self, frames, out, mask, centers=None, spread=False, joint_mask=None, center_keys=None):
        """The forward of checked frames (a _native.Frames) with a checked mask (_native.camera_mask) or None, and
        checked centres (_native.centers) or None = detect.  spread: the call runs the spread form and its Spread3D
        follows the three outputs.  joint_mask: what _native.joint_mask made, or None = the plain forward; the call's
        JointMask comes last.  center_keys: what _native.center_every made, or None = every row detects; the call's
        CenterKeyframes comes last of all."""
        if centers is not None and center_keys is not None:
            raise ValueError("centers= and center_every= do not combine: a call either brings its centres or detects "
                             "them on its key rows")
        dev = frames.device
        self.set_spread(spread)
        if joint_mask is not None or self._joint_masked:
            self.set_joint_mask(joint_mask)
        if centers is not None or self._centred:
            self.set_centers(centers)
        if center_keys is not None or self._keyframed:
            self.set_center_keyframes(*(center_keys or (0,)))
        if out is None:
            out = (torch.empty((self.T, self.J, 3), device=dev),
                   torch.empty((self.T, self.J), device=dev),
                   torch.empty((self.T,), device=dev, dtype=torch.int32))
        if mask is not None:
            mask = mask.to(dev, non_blocking=True)                # (copied by the call)
        N.call_forward("jh_predictor", self.handle, frames, mask, out)
        if mask is not None and mask.is_cuda:
            mask.record_stream(torch.cuda.current_stream())     # (free once the call is enqueued)
        res = tuple(out) + (self.spread(),) if spread else out
        res = tuple(res) + (self.joint_mask(),) if joint_mask is not None else res
        return tuple(res) + (self.center_keyframes(),) if center_keys is not None else res

    # ---- camera-sharded stages -------------------------------------------
    def stage_center(self, frames, det):
        frames = self._describe(frames).data
        fn = N.lib().jh_predictor_stage_center_u8 if frames.dtype == torch.uint8 else \
            N.lib().jh_predictor_stage_center
        N.check(fn(self.handle, N.ptr(frames), N.ptr(det), N.stream()))

    def stage_keypoints(self, frames, det_all, heat, camera_mask=None):
        """camera_mask: a (T,C) uint8 DEVICE tensor (kept alive by the caller until the stream has passed the call;
        all cameras local) for the masked triangulation; give stage_3d the same one.
        det_all may be None while centres are set (set_centers): stage 2 then takes them and reads no detection."""
        self._need_det(det_all)
        frames = self._describe(frames).data
        if camera_mask is not None:
            mask = self._device_mask(camera_mask)
            N.check(N.lib().jh_predictor_stage_keypoints_masked(
                self.handle, N.ptr(frames), int(frames.dtype == torch.uint8), N.ptr(det_all), N.ptr(mask), N.ptr(heat),
                N.stream()))
            return
        fn = N.lib().jh_predictor_stage_keypoints_u8 if frames.dtype == torch.uint8 else \
            N.lib().jh_predictor_stage_keypoints
        N.check(fn(self.handle, N.ptr(frames), N.ptr(det_all), N.ptr(heat), N.stream()))

    def _need_det(self, det):
        if det is None and not self._centred:
            raise ValueError("stage 2 needs the detections of stage 1 (det_all) unless centres are set (set_centers)")

    def _device_mask(self, camera_mask):
        if not (torch.is_tensor(camera_mask) and camera_mask.is_cuda and camera_mask.dtype == torch.uint8
                and camera_mask.is_contiguous() and tuple(camera_mask.shape) == (self.T, self.C)):
            raise ValueError("the staged calls take camera_mask as a contiguous (%d, %d) uint8 device tensor"
                             % (self.T, self.C))
        return camera_mask

    def stage_3d(self, heat_all, t0, points, conf, valid, camera_mask=None, joint_mask=None):
        """joint_mask: a contiguous (T,J,C) uint8 DEVICE tensor, rows t0 .. t0+T3-1 read in place (kept alive by the
        caller until the stream has passed the call; all cameras local): the joint-masked gather
        (jh_predictor_stage_3d_joint_masked); read the effective sets with joint_mask()."""
        if joint_mask is not None:
            if not (torch.is_tensor(joint_mask) and joint_mask.is_cuda and joint_mask.dtype == torch.uint8
                    and joint_mask.is_contiguous() and tuple(joint_mask.shape) == (self.T, self.J, self.C)):
                raise ValueError("the staged calls take joint_mask as a contiguous (%d, %d, %d) uint8 device tensor"
                                 % (self.T, self.J, self.C))
            mask = self._device_mask(camera_mask) if camera_mask is not None else None
            N.check(N.lib().jh_predictor_stage_3d_joint_masked(
                self.handle, N.ptr(heat_all), t0, N.ptr(mask), N.ptr(joint_mask), N.ptr(points), N.ptr(conf),
                N.ptr(valid), N.stream()))
            return
        if camera_mask is not None:
            mask = self._device_mask(camera_mask)
            N.check(N.lib().jh_predictor_stage_3d_masked(self.handle, N.ptr(heat_all), t0, N.ptr(mask), N.ptr(points),
                                                         N.ptr(conf), N.ptr(valid), N.stream()))
            return
        N.check(N.lib().jh_predictor_stage_3d(self.handle, N.ptr(heat_all), t0, N.ptr(points),
                                              N.ptr(conf), N.ptr(valid), N.stream()))

    def stage_keypoints_gathered(self, frames, det_gathered, n_blocks, heat):
        """Stage 2 reading the all-gathered detections (n_blocks, T, C/n_blocks, 3) in place (None while centres are
        set, as stage_keypoints)."""
        self._need_det(det_gathered)
        frames = self._describe(frames).data
        N.check(N.lib().jh_predictor_stage_keypoints_gathered(
            self.handle, N.ptr(frames), int(frames.dtype == torch.uint8), N.ptr(det_gathered), n_blocks,
            N.ptr(heat), N.stream()))

    def stage_3d_blocks(self, heat_blocks, n_blocks, frames_per_block, t_off, t0, points, conf, valid):
        """3D stage reading the exchange's receive buffer (n_blocks, frames_per_block, C/n_blocks,
        h, w, Jp) in place: frames t_off .. t_off+T3-1 of every block."""
        N.check(N.lib().jh_predictor_stage_3d_blocks(
            self.handle, N.ptr(heat_blocks), n_blocks, frames_per_block, t_off, t0, N.ptr(points),
            N.ptr(conf), N.ptr(valid), N.stream()))

    def views2d(self, points, heat=None, t0=0, camera_mask=None, out=None):
        """Per-camera 2D views of the frames t0 .. t0+T3-1 whose 3D keypoints are `points` (T3,J,3): call right
        after the forward / stage_3d that produced them, on the same stream -> Views2D of device tensors.
        heat None: the heat maps of the last forward(); otherwise the (T3,C,B/2,B/2,Jp) tensor stage_3d was given.
        camera_mask: the (T,C) mask that forward / those stages were given (host or device), or None.
        These are HybridNet's own 2D detections, on the crop around the projection of the triangulated centre;
        JarvisPredictor2D crops around each camera's own centre detection, so the two are not bit-equal."""
        dev, T3 = points.device, self.T3
        if not (points.is_cuda and points.is_contiguous() and points.dtype == torch.float32
                and tuple(points.shape) == (T3, self.J, 3)):
            raise ValueError("points must be the contiguous (%d, %d, 3) float32 device tensor of the 3D stage" % (T3, self.J))
        if heat is not None and not (heat.is_cuda and heat.is_contiguous() and heat.dtype == torch.float32 and
                                     tuple(heat.shape) == (T3, self.C, self.Hh, self.Hh, self.Jp)):
            raise ValueError("heat must be a contiguous (%d, %d, %d, %d, %d) float32 device tensor"
                             % (T3, self.C, self.Hh, self.Hh, self.Jp))
        mask = N.camera_mask(camera_mask, (self.T, self.C))
        if mask is not None:
            mask = mask.to(dev, non_blocking=True)
        if out is None:
            out = Views2D(torch.empty((T3, self.C, self.J, 2), device=dev, dtype=torch.int32),
                          torch.empty((T3, self.C, self.J), device=dev),
                          torch.empty((T3, self.C, self.J, 2), device=dev),
                          torch.empty((T3, self.C, self.J), device=dev),
                          torch.empty((T3, self.C), device=dev, dtype=torch.uint8))
        N.check(N.lib().jh_predictor_views2d(self.handle, N.ptr(heat), int(t0), N.ptr(points), N.ptr(mask),
                                             *(N.ptr(t) for t in out), N.stream()))
        if mask is not None:
            mask.record_stream(torch.cuda.current_stream())     # (read in place by the enqueued kernel)
        return Views2D(*out)

    def triangulate_joints(self, heat=None, t0=0, camera_mask=None, params=None):
        """A second 3D estimate of every joint of the frames t0 .. t0+T3-1, triangulated from the cameras' own 2D
        keypoints with the cameras that disagree left out (jh_predictor_triangulate_joints): call right after the
        forward / stage_3d, on the same stream -> Triangulated3D of device tensors.  heat, camera_mask: as views2d().
        params: what _native.joints3d_params made, a dict of its keywords, or None / True = the library's defaults
        (min_views 2, refine_radius 1, min_conf 0.1, max_error_px 8).  Plain launches behind a graph replay; the first
        call allocates its workspace (not inside a stream capture).  Nothing of the forwards' state is touched."""
        p = N.triangulation_params(True if params is None else params)
        if p is None:
            raise ValueError("params must be True, a dict or come from _native.joints3d_params")
        T3 = self.T3
        if heat is not None and not (heat.is_cuda and heat.is_contiguous() and heat.dtype == torch.float32 and
                                     tuple(heat.shape) == (T3, self.C, self.Hh, self.Hh, self.Jp)):
            raise ValueError("heat must be a contiguous (%d, %d, %d, %d, %d) float32 device tensor"
                             % (T3, self.C, self.Hh, self.Hh, self.Jp))
        dev = heat.device if heat is not None else torch.device("cuda", torch.cuda.current_device())
        mask = N.camera_mask(camera_mask, (self.T, self.C))
        if mask is not None:
            mask = mask.to(dev, non_blocking=True)
        out = Triangulated3D(torch.empty((T3, self.J, 3), device=dev),
                             torch.empty((T3, self.J), device=dev, dtype=torch.int32),
                             torch.empty((T3, self.J, self.C), device=dev, dtype=torch.uint8),
                             torch.empty((T3, self.J), device=dev),
                             torch.empty((T3, self.C, self.J, 3), device=dev))
        N.check(N.lib().jh_predictor_triangulate_joints(self.handle, N.ptr(heat), int(t0), N.ptr(mask), ctypes.byref(p),
                                                        *(N.ptr(t) for t in out), N.stream()))
        if mask is not None:
            mask.record_stream(torch.cuda.current_stream())     # (read in place by the enqueued kernel)
        return out

    def detect_subjects(self, frames, params, camera_mask=None, return_peaks=False):
        """Up to params.max_subjects subjects per frame set of checked frames (a _native.Frames with `data`, from
        _describe, or with `images`, from _native.frame_images) -> Subjects of device tensors, on the current stream
        (jh_predictor_detect_subjects): stage 1 up to CenterDetect's heat map, the top local maxima of every camera,
        their grouping across cameras, one triangulation per group -- under the calibration in force.  params: what
        _native.subjects_params made.  camera_mask (T,C) as forward().  return_peaks: the (T,C,max_peaks,3) peaks
        (x, y, value; empty slots (-1, -1, -inf)) follow.  Plain launches: nothing of the forwards' state -- graphs,
        centres, mask, spread -- is touched.  Needs CenterDetect weights and all cameras local (RuntimeError)."""
        if not isinstance(params, N.SubjectsParamsStruct):
            raise ValueError("params must come from _native.subjects_params, got %s" % type(params).__name__)
        if frames.images is not None and len(frames.images) != self.T * self.C:
            raise ValueError("expected %d images (time_batch * num_cameras), got %d" % (self.T * self.C,
                                                                                         len(frames.images)))
        mask = N.camera_mask(camera_mask, (self.T, self.C))
        dev, K = frames.device, params.max_subjects
        if mask is not None:
            mask = mask.to(dev, non_blocking=True)
        out = Subjects(torch.empty((self.T, K, 3), device=dev), torch.empty((self.T, K), device=dev, dtype=torch.int32),
                       torch.empty((self.T, K, self.C), device=dev, dtype=torch.int32),
                       torch.empty((self.T, K), device=dev))
        peaks = torch.empty((self.T, self.C, params.max_peaks, 3), device=dev) if return_peaks else None
        struct = frames.layout.struct() if frames.layout is not None else None
        table = None
        if frames.images is not None:
            table = (N.c_void_p * len(frames.images))(*(t.data_ptr() for t in frames.images))
        where = (self.handle, N.ptr(frames.data), table, 0 if table is None else len(frames.images))
        rest = (N.ptr(mask), ctypes.byref(params), *(N.ptr(t) for t in out), N.ptr(peaks), N.stream())
        if frames.fmt == N.FRAME_PIXELS:                     # (a PixelSurface: the entry point of its own)
            N.check(N.lib().jh_predictor_detect_subjects_pixels(*where, struct, *rest))
        else:
            N.check(N.lib().jh_predictor_detect_subjects(
                *where, frames.fmt, struct if frames.fmt == N.FRAME_SURFACE else None,
                struct if frames.fmt == N.FRAME_SENSOR else None, *rest))
        if mask is not None:
            mask.record_stream(torch.cuda.current_stream())     # (read in place by the enqueued kernel)
        return (out, peaks) if return_peaks else out

    def debug(self, device):
        c3f = torch.empty((self.T, 3), device=device)
        c3i = torch.empty((self.T, 3), device=device, dtype=torch.int32)
        chm = torch.empty((self.T, self.C, 2), device=device, dtype=torch.int32)
        det = torch.empty((self.T, self.C, 3), device=device)
        N.check(N.lib().jh_predictor_debug(self.handle, N.ptr(c3f), N.ptr(c3i), N.ptr(chm),
                                           N.ptr(det), N.stream()))
        return dict(center3d=c3f, center3d_int=c3i, center_hm=chm, det=det)

    def debug_mask(self, device):
        """Counts of the last MASKED forward: n_active (T) unmasked cameras, num_cams_detect (T) those of them with
        maxval > 50."""
        n_act = torch.empty((self.T,), device=device, dtype=torch.int32)
        n_det = torch.empty((self.T,), device=device, dtype=torch.int32)
        N.check(N.lib().jh_predictor_debug_mask(self.handle, N.ptr(n_act), N.ptr(n_det), N.stream()))
        return dict(n_active=n_act, num_cams_detect=n_det)

    def hybridnet_forward(self, crops, center_hm, center3d, want_final=True, want_padded=True):
        dev = crops.device
        Gh = int(self.cfg.roi_cube_size / self.cfg.grid_spacing) // 2
        hs = self.Hh + 2
        final = torch.empty((self.T, self.J, Gh, Gh, Gh), device=dev) if want_final else None
        padded = torch.empty((self.T, self.C, self.J, hs, hs), device=dev) if want_padded else None
        pts = torch.empty((self.T, self.J, 3), device=dev)
        conf = torch.empty((self.T, self.J), device=dev)
        N.check(N.lib().jh_predictor_hybridnet_forward(
            self.handle, N.ptr(crops), N.ptr(center_hm), N.ptr(center3d), N.ptr(final),
            N.ptr(padded), N.ptr(pts), N.ptr(conf), N.stream()))
        return final, padded, pts, conf


class MultiStreamPredictor:
    """K independent time batches in flight on K HIP streams.

    Every stream has its own NativePredictor (own launch plans, activations and scratch), so
    consecutive `forward` calls have no hazards between them and the GPU interleaves their
    kernels: the phases in which one batch leaves resources idle (the Winograd V2V kernel runs
    one workgroup per CU and keeps the matrix cores busy about half the time; the 2D layers
    are mostly latency / bandwidth bound) are filled by another batch.  Measured on one
    MI355X at BASELINE configs[2]: 1602 frames/s with 3 streams x 32 frames against 1528 for
    one stream x 64 frames.

    forward() returns the output tensors of the batch it has just ENQUEUED on its stream; call
    synchronize() (or wait on `last_event`) before reading them.
    """

    def __init__(self, make_predictor, streams=3, timing=False):
        self.timing = timing                         # events usable with elapsed_time (bench.py)
        self.preds = [make_predictor() for _ in range(streams)]
        self.streams = [torch.cuda.Stream() for _ in range(streams)]
        self.events = [None] * streams
        self._next = 0
        self._calib = None
        self._calib_of = [None] * streams            # per predictor: (key, tensors) of the per-frame calibration it holds

    def set_calibration(self, *calib):
        """Calibration of every predictor, written on that predictor's OWN stream (so the copy
        is ordered against the forwards in flight there).  Setting the same tensors again is a
        no-op: drivers may call this once per group of frames.
        Per-frame form -- (T,C,4,3) / (T,C,3,3) / (T,C,1,5), row t for frame set t (_native.calibration) --: the
        calibration of ONE batch, the one the next forward() enqueues.  It goes to the predictor that batch runs on
        alone, on that predictor's stream, inside forward(); the batches in flight on the other streams keep theirs.
        It stays in force for later forwards until another calibration is set (each predictor is given it when its
        turn comes; one that holds these very tensors already is left alone)."""
        p0 = self.preds[0]
        # (the shared form is taken as it always was; what has a leading T is checked as the per-frame form)
        form = N.calibration(calib, p0.T, p0.C)[0] if len(calib) == 3 and calib[0].dim() == 4 else "shared"
        key = (form,) + tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in calib)
        if key == self._calib:
            return
        if form == "frames":
            self._calib_refs = tuple(calib)          # (alive while keyed, as below)
            self._calib = key
            return
        # the key is only meaningful while the keyed tensors are alive: a freed calibration's
        # address is handed out again by the caching allocator (same size, _version 0), and the
        # next recording's tensors would then look like "the same tensors again".  Holding them
        # makes address + version identify the contents.
        self._calib_refs = tuple(calib)
        cur = torch.cuda.current_stream()
        for p, s in zip(self.preds, self.streams):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                p.set_calibration(*calib)
            for t in calib:
                if t.is_cuda:
                    t.record_stream(s)
        self._calib = key
        self._calib_of = [None] * len(self.preds)

    def set_tone(self, tone):
        """Tone tables of every predictor (NativePredictor.set_tone), written on that predictor's OWN stream, so the
        copy is ordered against the forwards in flight there.  None: back to the plain form."""
        tone = check_tone(tone, self.preds[0].C)
        cur = torch.cuda.current_stream()
        for p, s in zip(self.preds, self.streams):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                p.set_tone(tone)

    def _frames_calibration(self, i):
        """Inside predictor i's stream context: its copy of the per-frame calibration in force, if it has not got it."""
        if self._calib is None or self._calib[0] != "frames":
            return
        held = self._calib_of[i]
        if held is not None and held[0] == self._calib:
            return
        self.preds[i].set_calibration_frames(*self._calib_refs)
        for t in self._calib_refs:
            if t.is_cuda:
                t.record_stream(self.streams[i])
        self._calib_of[i] = (self._calib, self._calib_refs)       # the tensors live as long as their key is compared

    def forward(self, frames, out=None, then=None, frame_format=None, camera_mask=None, return_2d=False,
                frame_layout=None, centers=None, return_spread=False, return_triangulated=False, joint_mask=None,
                center_every=None):
        """return_2d: the five tensors of NativePredictor.views2d for this batch are appended to the outputs
        (points, conf, valid, points2D, confidences2D, reprojections, errors, used).
        return_spread: the three tensors of the batch's Spread3D (cov (T,J,3,3), peak, mass) are appended behind them.
        return_triangulated (True or what _native.joints3d_params made): the five tensors of the batch's Triangulated3D
        (NativePredictor.triangulate_joints) are appended behind them.
        joint_mask (as NativePredictor.forward): the two tensors of the batch's JointMask (cameras, count) are appended
        last.
        `then(outputs)`, when given, runs inside the batch's stream context right behind the forward and
        before its event is recorded (the drivers enqueue the device->host copy of the results there); its
        return value replaces the outputs.  frame_format, camera_mask, frame_layout: as NativePredictor.forward.
        centers (T,3): the centres of THIS batch (NativePredictor.set_centers), written on the stream of the predictor
        the batch runs on; None: the batch detects.
        center_every (k, or (k, n_rows) for a batch whose first n_rows rows are real; _native.center_every): THIS batch
        detects on its key rows only (NativePredictor.set_center_keyframes) and the two tensors of its CenterKeyframes
        (centers, source) are appended last of all.  The key rows are rows of the batch, so with k > 1 the result
        depends on how a recording is cut into batches (time_batch), not on the number of streams."""
        p0 = self.preds[0]
        described = p0._describe(frames, frame_format, frame_layout)               # before any stream work
        camera_mask = N.camera_mask(camera_mask, (p0.T, p0.C))
        centers = N.centers(centers, p0.T)
        center_keys = N.center_every(center_every, p0.T)
        if centers is not None and center_keys is not None:
            raise ValueError("centers= and center_every= do not combine")
        tri_params = N.triangulation_params(return_triangulated)
        if joint_mask is not None:
            joint_mask = N.joint_mask(joint_mask, p0.T, p0.J, p0.C)
        i = self._next
        self._next = (i + 1) % len(self.preds)
        s = self.streams[i]
        s.wait_stream(torch.cuda.current_stream())       # `frames` may still be in the making
        # The kernels see raw pointers only, so the caching allocator must be told that the
        # side stream uses these blocks: without record_stream a caller that drops `frames`
        # right after this call could get the same memory back for its next batch while the
        # forward in flight here still reads it (it reads the frames twice: resize, then crops).
        frames.record_stream(s)
        for t in (out or ()):
            t.record_stream(s)
        with torch.cuda.stream(s):
            self._frames_calibration(i)
            res = self.preds[i]._forward(described, out, camera_mask, centers, return_spread,
                                         **({} if joint_mask is None else {"joint_mask": joint_mask}),
                                         **({} if center_keys is None else {"center_keys": center_keys}))
            if center_keys is not None:
                res, keyframes = res[:-1], tuple(res[-1])
            if joint_mask is not None:
                res, jm = res[:-1], tuple(res[-1])
            if return_spread:
                res, spread = res[:3], tuple(res[3])
            if return_2d:
                res = tuple(res) + tuple(self.preds[i].views2d(res[0], camera_mask=camera_mask))
            if return_spread:
                res = tuple(res) + spread
            if tri_params is not None:
                res = tuple(res) + tuple(self.preds[i].triangulate_joints(camera_mask=camera_mask, params=tri_params))
            if joint_mask is not None:
                res = tuple(res) + jm
            if center_keys is not None:
                res = tuple(res) + keyframes
            if then is not None:
                res = then(res)
            ev = torch.cuda.Event(enable_timing=self.timing)
            ev.record(s)
        self.events[i] = ev
        self.last_event = ev
        return res

    def forward_subjects(self, frames, params, tracker=None, then=None, frame_format=None, camera_mask=None,
                         frame_layout=None):
        """Several subjects of one batch, on the batch's stream: detect_subjects (params: what _native.subjects_params
        made, K = params.max_subjects), the update of `tracker` (a tracks.SubjectTracker of K slots, or None) and K
        centred forwards, one per subject (or slot) -> points (T,K,J,3), conf (T,K,J), valid (T,K), then the four
        tensors of the Subjects (centers, views, members, error; in slot order under a tracker), then the four of the
        Tracks (ids, slots, missed, dropped) when there is a tracker.  The tracker orders its updates itself (an event
        from batch to batch), so the batches of a recording update it in call order although they run on different
        streams.  then, frame_format, camera_mask, frame_layout: as forward()."""
        p0 = self.preds[0]
        described = p0._describe(frames, frame_format, frame_layout)               # before any stream work
        camera_mask = N.camera_mask(camera_mask, (p0.T, p0.C))
        K = params.max_subjects
        check_tracker(tracker, K)
        i = self._next
        self._next = (i + 1) % len(self.preds)
        s = self.streams[i]
        s.wait_stream(torch.cuda.current_stream())       # `frames` may still be in the making
        frames.record_stream(s)                          # (see forward)
        with torch.cuda.stream(s):
            self._frames_calibration(i)
            pr = self.preds[i]
            subjects = pr.detect_subjects(described, params, camera_mask)
            tracks = ()
            if tracker is not None:
                subjects, tracks = tracker.update(subjects)
            rows = [pr._forward(described, None, camera_mask, N.centers(subjects.centers[:, k], p0.T))
                    for k in range(K)]
            res = tuple(torch.stack([r[j] for r in rows], 1) for j in range(3)) + tuple(subjects) + tuple(tracks)
            if then is not None:
                res = then(res)
            ev = torch.cuda.Event(enable_timing=self.timing)
            ev.record(s)
        self.events[i] = ev
        self.last_event = ev
        return res

    def synchronize(self):
        for s in self.streams:
            s.synchronize()
