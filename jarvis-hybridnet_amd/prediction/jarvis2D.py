"""JarvisPredictor2D on MI355X (mirrors jarvis/prediction/jarvis2D.py:19-155).

Same constructor / forward signature and attributes (`centerDetect`,
`keypointDetect`), same `(None, None)` convention (centre heatmap maximum
<= 40).  `forward` is one native call (jh_predictor2d_* in include/jarvis_hip.h).
"""
import ctypes
import math

import torch
import torch.nn as nn

from .. import _native as N
from .. import arch
from .._params import flat_state
from ..efficienttrack.efficienttrack import EfficientTrack
from .jarvis3D import precision_for_trt_mode


class _Native2D:
    def __init__(self, center_state, kp_state, cfg, img_h, img_w, batch, precision=None):
        c = N.PredictorConfig(
            1, cfg.KEYPOINTDETECT.NUM_JOINTS, int(cfg.CENTERDETECT.IMAGE_SIZE),
            cfg.KEYPOINTDETECT.BOUNDING_BOX_SIZE, 0.0, 0.0,
            arch.SIZE_IDS[cfg.CENTERDETECT.MODEL_SIZE], arch.SIZE_IDS[cfg.KEYPOINTDETECT.MODEL_SIZE],
            img_h, img_w, batch, 0, 0, 1, (ctypes.c_float * 3)(*cfg.DATASET.MEAN),
            (ctypes.c_float * 3)(*cfg.DATASET.STD), N.precision_id(precision))
        self.T, self.J = batch, cfg.KEYPOINTDETECT.NUM_JOINTS
        self.H, self.W = img_h, img_w
        self.handle = ctypes.c_void_p()
        pc, pk = N.Params(center_state), N.Params(kp_state)
        N.check(N.lib().jh_predictor2d_create(pc.handle, pk.handle, ctypes.byref(c),
                                              ctypes.byref(self.handle)))
        self._toned = False

    def set_tone(self, tone):
        """tone: a ToneTables of one camera, or None = the plain form (jh_predictor2d_set_tone; copied on the current
        stream, the first such call allocates the buffer)."""
        from ..tone import check_tone
        tone = check_tone(tone, 1)
        if tone is None:
            if self._toned:
                N.check(N.lib().jh_predictor2d_set_tone(self.handle, None, N.stream()))
                self._toned = False
            return
        dev = torch.tensor(tone.tables).to("cuda")
        N.check(N.lib().jh_predictor2d_set_tone(self.handle, N.ptr(dev), N.stream()))
        dev.record_stream(torch.cuda.current_stream())          # (copied by the call: free once it is enqueued)
        self._toned = True

    def _forward(self, frames):
        """The forward of checked frames (a _native.Frames of T images of this predictor's size)."""
        if (frames.height, frames.width, math.prod(frames.lead)) != (self.H, self.W, self.T):
            raise RuntimeError("%d frames of %d x %d given to a predictor of %d frames of %d x %d" % (
                math.prod(frames.lead), frames.height, frames.width, self.T, self.H, self.W))
        dev = frames.device
        pts = torch.empty((self.T, self.J, 2), device=dev, dtype=torch.int32)
        conf = torch.empty((self.T, self.J), device=dev)
        valid = torch.empty((self.T,), device=dev, dtype=torch.int32)
        N.call_forward("jh_predictor2d", self.handle, frames, None, (pts, conf, valid))
        return pts, conf, valid

    def close(self):
        if getattr(self, "handle", None) and N is not None and N._lib is not None:
            N.lib().jh_predictor2d_destroy(self.handle)
            self.handle = None

    __del__ = close


class JarvisPredictor2D(nn.Module):
    def __init__(self, cfg, weights_center_detect="latest", weights_keypoint_detect="latest",
                 trt_mode="off", precision=None):
        super().__init__()
        # trt_mode 'new' / 'previous' (jarvis2D.py:39-43) select the reduced-precision mode bf16x3, see
        # jarvis3D.precision_for_trt_mode
        self.precision = precision_for_trt_mode(trt_mode, precision)
        self.trt_mode = trt_mode
        self.cfg = cfg
        self.centerDetect = EfficientTrack("CenterDetectInference", cfg, weights_center_detect).model
        self.keypointDetect = EfficientTrack("KeypointDetectInference", cfg,
                                             weights_keypoint_detect).model
        self.bbox_hw = int(cfg.KEYPOINTDETECT.BOUNDING_BOX_SIZE / 2)
        self.bounding_box_size = cfg.KEYPOINTDETECT.BOUNDING_BOX_SIZE
        self.center_detect_img_size = int(cfg.CENTERDETECT.IMAGE_SIZE)
        self._native = {}
        self._tone = None                                    # the ToneTables in force (set_tone)

    def set_tone(self, tone):
        """tone: a ToneTables of ONE camera ((1,3,256); a (3,256) array too), or None: every forward of byte frames then
        replaces byte k of channel ch by tone.tables[0][ch][k] in place of k / 255 (JarvisPredictor3D.set_tone).  It
        holds for every native predictor this object has or later makes."""
        from ..tone import check_tone
        self._tone = check_tone(tone, 1)
        for pr in self._native.values():
            pr.set_tone(self._tone)

    def native(self, img_h, img_w, batch=1):
        key = (img_h, img_w, batch)
        if key not in self._native:
            self._native[key] = _Native2D(flat_state(self.centerDetect),
                                          flat_state(self.keypointDetect), self.cfg, img_h, img_w,
                                          batch, self.precision)
            if self._tone is not None:
                self._native[key].set_tone(self._tone)
        return self._native[key]

    def forward(self, img, frame_layout=None):
        """img (1,3,H,W) RGB in [0,1] -> (points2D (J,2) int64 pixels, confidences (J,))
        or (None, None).  frame_layout: a YuvSurface or a SensorSurface -- img is forward_surface's."""
        if frame_layout is not None:
            return self.forward_surface(img, frame_layout)
        frames = N.describe_frames(img, (None,))
        return self._run(frames, True)

    def _run(self, frames, single=False):
        """The forward of checked frames (a _native.Frames) on the native predictor of their size and count; single:
        the first image's (points2D int64, confidences), or (None, None) where nothing is detected
        (jarvis2D.py:121,150-153)."""
        pts, conf, valid = self.native(frames.height, frames.width, frames.lead[0])._forward(frames)
        if not single:
            return pts, conf, valid
        if int(valid[0].item()) == 0:
            return None, None
        return pts[0].long(), conf[0]

    def forward_yuv(self, img, frame_format):
        """img (3H/2,W) or (1,3H/2,W) uint8 YUV 4:2:0, frame_format 'i420' / 'nv12' (H, W even; see
        JarvisPredictor3D.forward_yuv) -> (points2D (J,2) int64 pixels, confidences (J,)) or (None, None)."""
        if torch.is_tensor(img) and img.dim() == 2:
            img = img.unsqueeze(0)
        frames = N.describe_frames(img, (None,), N.yuv_format(frame_format))
        return self._run(frames, True)

    def forward_surface(self, img, surface):
        """img (image_stride,) or (1,image_stride) uint8: one YUV 4:2:0 image read through the YuvSurface `surface`,
        or one raw Mono8 / Bayer image read through the SensorSurface `surface`, or one image of a PixelSurface (any
        shape of exactly image_stride bytes, e.g. (H,W,3) RGB; see JarvisPredictor3D.forward_surface) -> (points2D (J,2) int64 pixels, confidences (J,)) or (None, None)."""
        from ..pixel_surface import PixelSurface
        if torch.is_tensor(img) and (img.dim() == 1 or (isinstance(surface, PixelSurface) and
                                                        img.numel() == surface.image_stride)):
            img = img.unsqueeze(0)                           # (a PixelSurface: ONE image of any shape, e.g. (H,W,3))
        frames = N.describe_frames(img, (1,), None, N.surface(surface))
        return self._run(frames, True)

    def forward_batch(self, imgs, frame_format=None, frame_layout=None):
        """imgs (T,3,H,W) fp32 RGB or (T,H,W,3) uint8 BGR, independent images ->
        points2D (T,J,2) int32, confidences (T,J), valid (T) int32; no host sync.  frame_format 'i420' / 'nv12':
        imgs (T,3H/2,W) uint8 YUV 4:2:0; 'bgr': uint8 BGR required; None: the dtype decides.  frame_layout: a
        YuvSurface or a SensorSurface -- imgs (T,image_stride) uint8 (forward_surface); not together with 'i420' / 'nv12'."""
        frames = N.describe_frames(imgs, (None,), frame_format, frame_layout)
        return self._run(frames)

    def forward_images(self, images, frame_format=None, frame_layout=None):
        """forward_batch on T images that lie where their producers left them: `images` a sequence of T tensors, each
        ONE image -- fp32 (3,H,W); uint8 (H,W,3); 'i420' / 'nv12': uint8 (3H/2,W); frame_layout: 1-D uint8 of at least
        image_stride bytes (see JarvisPredictor3D.forward_images) -> what forward_batch returns for their stack, bit
        for bit; no host sync."""
        if not isinstance(images, (list, tuple)) or len(images) == 0:
            raise ValueError("images must be a non-empty sequence of tensors, one per image")
        frames = N.frame_images(list(images), len(images), frame_format, frame_layout)
        return self._run(frames)
