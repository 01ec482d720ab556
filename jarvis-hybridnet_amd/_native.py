"""ctypes binding of libjarvis_hip.so (the C ABI in include/jarvis_hip.h).

There is deliberately no fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  PyTorch is used only as the owner of device
memory and streams -- every pointer crossing this boundary is a raw address.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# JH_LIBRARY_PATH: another build of the SAME library (tests/host_sanitize: the host halves under ASan / UBSan against a
# malloc-backed HIP stand-in).  Not a fallback: whatever is named must exist and export every symbol.
LIB_PATH = os.environ.get("JH_LIBRARY_PATH") or os.path.join(_HERE, "libjarvis_hip.so")
_lib = None

c_void_p, c_int, c_float, c_int64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
c_char_p = ctypes.c_char_p


class PredictorConfig(ctypes.Structure):
    _fields_ = [("num_cameras", ctypes.c_int32), ("num_joints", ctypes.c_int32),
                ("center_size", ctypes.c_int32), ("bbox", ctypes.c_int32),
                ("roi_cube_size", c_float), ("grid_spacing", c_float),
                ("center_model", ctypes.c_int32), ("kp_model", ctypes.c_int32),
                ("img_h", ctypes.c_int32), ("img_w", ctypes.c_int32),
                ("time_batch", ctypes.c_int32), ("time_batch_3d", ctypes.c_int32),
                ("cam_lo", ctypes.c_int32),
                ("cam_n", ctypes.c_int32), ("mean", c_float * 3), ("std", c_float * 3),
                ("precision", ctypes.c_int32)]


class YuvSurfaceStruct(ctypes.Structure):
    """jh_yuv_surface of include/jarvis_hip.h (built by yuv_surface.YuvSurface.struct())."""
    _fields_ = [("image_stride", ctypes.c_int64), ("y_offset", ctypes.c_int64), ("y_pitch", ctypes.c_int64),
                ("u_offset", ctypes.c_int64), ("v_offset", ctypes.c_int64), ("c_pitch", ctypes.c_int64),
                ("c_step", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(YuvSurfaceStruct) == 64


class SensorSurfaceStruct(ctypes.Structure):
    """jh_sensor_surface of include/jarvis_hip.h (built by sensor_surface.SensorSurface.struct())."""
    _fields_ = [("image_stride", ctypes.c_int64), ("offset", ctypes.c_int64), ("pitch", ctypes.c_int64),
                ("pattern", ctypes.c_int32), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(SensorSurfaceStruct) == 32

ABI_VERSION = 4                      # JH_ABI_VERSION of include/jarvis_hip.h
# sizeof(jh_predictor_config): statically asserted on the C side (tests/abi_smoke.c) and here
assert ctypes.sizeof(PredictorConfig) == 84

_WORKSPACES = {}


def workspace(nbytes, device):
    """A cached device byte buffer of at least `nbytes` (the caller-provided workspace of the
    stand-alone operators), one per (device, current stream): operators on different streams
    never share scratch space.  A buffer that is outgrown is kept alive (not freed) because its
    address may be baked into a captured hipGraph; graph-capturing callers that want to bound
    that should own their workspace and call the C entry points directly."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    bufs = _WORKSPACES.setdefault(key, [])
    if not bufs or bufs[-1].numel() < nbytes:
        bufs.append(torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=device))
    return bufs[-1]


_SIGS = {
    "jh_last_error": (c_char_p, []),
    "jh_abi_version": (c_int, []),
    "jh_set_precision": (c_int, [c_int]),
    "jh_get_precision": (c_int, []),
    "jh_params_create": (c_int, [ctypes.POINTER(c_void_p)]),
    "jh_params_set": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "jh_params_destroy": (None, [c_void_p]),
    "jh_efftrack_create": (c_int, [c_void_p, c_char_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                   ctypes.POINTER(c_void_p)]),
    "jh_efftrack_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_efftrack_launches": (c_int64, [c_void_p]),
    "jh_efftrack_destroy": (None, [c_void_p]),
    "jh_v2v_create": (c_int, [c_void_p, c_char_p, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "jh_v2v_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_v2v_destroy": (None, [c_void_p]),
    "jh_reproject_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "jh_reproject_forward": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
    "jh_softargmax_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "jh_softargmax": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "jh_reproject_point": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "jh_reconstruct_workspace_bytes": (c_int64, [c_int]),
    "jh_reconstruct_point": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_void_p]),
    "jh_predictor_create": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PredictorConfig),
                                    ctypes.POINTER(c_void_p)]),
    "jh_predictor_destroy": (None, [c_void_p]),
    "jh_predictor_set_graph_replay": (c_int, [c_void_p, c_int]),
    "jh_predictor_graph_replay": (c_int, [c_void_p]),
    "jh_predictor_launches": (c_int64, [c_void_p]),
    "jh_predictor_device_bytes": (c_int64, [c_void_p]),
    "jh_predictor_precision": (c_int, [c_void_p]),
    "jh_predictor_set_calibration": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_center": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_keypoints": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_3d": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "jh_predictor_stage_keypoints_gathered": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                      c_void_p]),
    "jh_predictor_stage_3d_blocks": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                             c_void_p, c_void_p, c_void_p]),
    "jh_profile_begin": (c_int, []),
    "jh_profile_end": (c_int, [ctypes.POINTER(c_int)]),
    "jh_profile_get": (c_int, [c_int, c_char_p, c_int, ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "jh_predictor_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_center_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_keypoints_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_forward_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_forward_yuv": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_yuv_surface_check": (c_int, [ctypes.POINTER(YuvSurfaceStruct), c_int, c_int]),
    "jh_predictor_forward_surface": (c_int, [c_void_p, c_void_p, ctypes.POINTER(YuvSurfaceStruct), c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p]),
    "jh_predictor2d_forward_surface": (c_int, [c_void_p, c_void_p, ctypes.POINTER(YuvSurfaceStruct), c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "jh_op_yuv_surface_to_bgr": (c_int, [c_void_p, ctypes.POINTER(YuvSurfaceStruct), c_int, c_int, c_int, c_void_p,
                                         c_void_p]),
    "jh_sensor_surface_check": (c_int, [ctypes.POINTER(SensorSurfaceStruct), c_int, c_int]),
    "jh_predictor_forward_sensor": (c_int, [c_void_p, c_void_p, ctypes.POINTER(SensorSurfaceStruct), c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    "jh_predictor2d_forward_sensor": (c_int, [c_void_p, c_void_p, ctypes.POINTER(SensorSurfaceStruct), c_void_p,
                                              c_void_p, c_void_p, c_void_p]),
    "jh_op_sensor_to_bgr": (c_int, [c_void_p, ctypes.POINTER(SensorSurfaceStruct), c_int, c_int, c_int, c_void_p,
                                    c_void_p]),
    "jh_predictor_forward_masked": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "jh_predictor_forward_images": (c_int, [c_void_p, ctypes.POINTER(c_void_p), c_int, c_int,
                                            ctypes.POINTER(YuvSurfaceStruct), ctypes.POINTER(SensorSurfaceStruct),
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor2d_forward_images": (c_int, [c_void_p, ctypes.POINTER(c_void_p), c_int, c_int,
                                              ctypes.POINTER(YuvSurfaceStruct), ctypes.POINTER(SensorSurfaceStruct),
                                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_keypoints_masked": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                                    c_void_p]),
    "jh_predictor_stage_3d_masked": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p]),
    "jh_predictor_debug_mask": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_views2d": (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 8),
    "jh_joint_argmax_all_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "jh_op_joint_argmax_all": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_void_p]),
    "jh_predictor2d_create": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PredictorConfig),
                                      ctypes.POINTER(c_void_p)]),
    "jh_predictor2d_destroy": (None, [c_void_p]),
    "jh_predictor2d_forward": (c_int, [c_void_p] * 6),
    "jh_predictor2d_forward_u8": (c_int, [c_void_p] * 6),
    "jh_predictor2d_forward_yuv": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_debug": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_hybridnet_forward": (c_int, [c_void_p] * 9),
    "jh_op_conv": (c_int, [c_int] * 7 + [c_void_p, c_void_p, c_void_p] + [c_int] * 4 +
                   [c_void_p, c_int, c_void_p, c_void_p]),
    "jh_op_depthwise": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                c_void_p, c_void_p]),
    "jh_op_depthwise_pool": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p]),
    "jh_op_yuv420_to_bgr": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "jh_op_bifpn_node": (c_int, [c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_float), c_int, c_int, c_int,
                                 c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
}


def symbols():
    """Names of every entry point include/jarvis_hip.h declares."""
    return sorted(_SIGS)


def lib():
    """Load the shared library once; raise if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                "jarvis_hybridnet_amd: %s is missing -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                "There is no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)          # AttributeError if the .so lacks a symbol
            fn.restype, fn.argtypes = res, args
        if handle.jh_abi_version() != ABI_VERSION:
            raise RuntimeError("libjarvis_hip.so ABI version mismatch")
        _lib = handle
    return _lib


# frame_format names of the Python API -> JH_FRAME_* of include/jarvis_hip.h.  'bgr': uint8 BGR (H,W,3) images as
# cv2 delivers them; 'i420' / 'nv12': YUV 4:2:0, one contiguous (3H/2, W) uint8 image per camera, H and W even.
FRAME_FORMATS = {"bgr": 1, "i420": 2, "nv12": 3}
YUV_FORMATS = ("i420", "nv12")


def frame_format(name):
    """A frame_format argument checked: None (the frame tensor's dtype decides, the behaviour without the argument)
    or one of FRAME_FORMATS; anything else raises ValueError."""
    if name is not None and name not in FRAME_FORMATS:
        raise ValueError("frame_format must be one of %s or None, got %r" % (sorted(FRAME_FORMATS), name))
    return name


def yuv_frame_hw(shape):
    """(rows, W) of a YUV 4:2:0 image -> (H, W).  rows = 3H/2 with H and W even: ValueError otherwise (an odd
    frame height leaves rows that are no multiple of 3)."""
    rows, w = int(shape[-2]), int(shape[-1])
    if rows <= 0 or rows % 3 or w <= 0 or w % 2:
        raise ValueError("a YUV 4:2:0 image is (3H/2, W) bytes with H and W even; got (%d, %d)" % (rows, w))
    return rows // 3 * 2, w


def frame_layout(layout, frame_format, lead, hw=None, frames=None):
    """A frame_layout argument checked, before anything reaches the GPU: None stays None; otherwise a
    yuv_surface.YuvSurface or a sensor_surface.SensorSurface, not combined with frame_format 'i420' / 'nv12' (the
    layout says what the bytes are), of the frame size `hw` when that is given, and `frames` (when given) a uint8
    tensor of shape lead + (image_stride,) -- `lead` a tuple whose None entries match any size.  ValueError
    otherwise."""
    if layout is None:
        return None
    if not is_frame_layout(layout):
        raise ValueError("frame_layout must be a YuvSurface or a SensorSurface or None, got %r"
                         % (type(layout).__name__,))
    if frame_format in YUV_FORMATS:
        raise ValueError("frame_layout describes the bytes itself: do not combine it with frame_format=%r"
                         % (frame_format,))
    if hw is not None and (layout.height, layout.width) != tuple(hw):
        raise ValueError("frame_layout is %d x %d; this predictor is %d x %d" % (layout.height, layout.width, *hw))
    if frames is not None:
        want = tuple(lead) + (layout.image_stride,)
        ok = torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == len(want) and all(
            w is None or int(g) == w for g, w in zip(frames.shape, want))
        if not ok:
            raise ValueError("frames of a %s must be uint8 %s (image_stride bytes per image); got %s" % (
                type(layout).__name__, tuple("*" if w is None else w for w in want),
                (frames.dtype, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__))
    return layout


def is_frame_layout(layout):
    """True for the two descriptions frame_layout= takes: a YuvSurface or a SensorSurface."""
    from .sensor_surface import SensorSurface
    from .yuv_surface import YuvSurface
    return isinstance(layout, (YuvSurface, SensorSurface))


def forward_entry(which, frames, frame_format=None, layout=None, mask=None):
    """The whole-path entry point of the library for a call's frames, and the arguments that say what they are:
    (fn, fmt_args), called as fn(handle, ptr(frames), *fmt_args, <outputs>, stream).  which = 'jh_predictor' (3D,
    whose masked and described entry points take the device mask pointer, NULL for none) or 'jh_predictor2d' (no
    masks).  layout: a checked frame_layout (its struct is kept alive by fmt_args); otherwise frame_format 'i420' /
    'nv12', or the dtype decides between uint8 BGR and fp32 RGB."""
    if layout is not None:
        from .sensor_surface import SensorSurface
        kind = "sensor" if isinstance(layout, SensorSurface) else "surface"
        return (getattr(lib(), "%s_forward_%s" % (which, kind)),
                (layout.struct(),) + ((ptr(mask),) if which == "jh_predictor" else ()))
    fmt = FRAME_FORMATS[frame_format] if frame_format in YUV_FORMATS else int(frames.dtype == torch.uint8)
    if mask is not None:
        return lib().jh_predictor_forward_masked, (fmt, ptr(mask))
    if frame_format in YUV_FORMATS:
        return getattr(lib(), which + "_forward_yuv"), (fmt,)
    return getattr(lib(), which + ("_forward_u8" if fmt else "_forward")), ()


FRAME_RGB_F32, FRAME_SURFACE, FRAME_SENSOR = 0, 4, 5      # JH_FRAME_* beside FRAME_FORMATS
_checked_format, _checked_layout = frame_format, frame_layout   # (frame_images' arguments carry the public names)


def frame_images(images, count, frame_format=None, frame_layout=None):
    """The images of a per-image call (forward_images) checked, before anything reaches the GPU: `images` a sequence
    of `count` tensors, each ONE image -- fp32 (3,H,W); uint8 (H,W,3); with frame_format 'i420' / 'nv12' uint8
    (3H/2,W); with frame_layout a 1-D uint8 tensor of at least image_stride bytes -- all of one shape, dtype and
    device, contiguous and on the GPU.  Nothing is copied: the tensors are read where they lie.
    -> (format code JH_FRAME_*, (H, W), the checked layout or None).  ValueError for what does not fit the call
    (count, mixed images, shapes, frame_layout with 'i420' / 'nv12'), RuntimeError for a CPU or a non-contiguous
    tensor, as the contiguous forms raise them."""
    frame_format = _checked_format(frame_format)
    frame_layout = _checked_layout(frame_layout, frame_format, ())
    if not isinstance(images, (list, tuple)) or len(images) != count:
        raise ValueError("expected a sequence of %d images (one tensor per image); got %s" % (
            count, len(images) if isinstance(images, (list, tuple)) else type(images).__name__))
    for i, t in enumerate(images):
        if not torch.is_tensor(t):
            raise ValueError("image %d is a %s, not a tensor" % (i, type(t).__name__))
        if (t.shape, t.dtype, t.device) != (images[0].shape, images[0].dtype, images[0].device):
            raise ValueError("the images of a call have one shape, dtype and device: image %d is %s, image 0 is %s" % (
                i, (t.dtype, tuple(t.shape), str(t.device)),
                (images[0].dtype, tuple(images[0].shape), str(images[0].device))))
    t = images[0]
    if frame_layout is not None:
        if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < frame_layout.image_stride:
            raise ValueError("an image of a %s must be 1-D uint8 of at least image_stride = %d bytes; got %s" % (
                type(frame_layout).__name__, frame_layout.image_stride, (t.dtype, tuple(t.shape))))
        from .sensor_surface import SensorSurface
        fmt = FRAME_SENSOR if isinstance(frame_layout, SensorSurface) else FRAME_SURFACE
        hw = (frame_layout.height, frame_layout.width)
    elif frame_format in YUV_FORMATS:
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise ValueError("a %s image must be uint8 (3H/2, W); got %s" % (frame_format, (t.dtype, tuple(t.shape))))
        fmt, hw = FRAME_FORMATS[frame_format], yuv_frame_hw(t.shape)
    elif t.dtype == torch.uint8:
        if t.dim() != 3 or t.shape[2] != 3:
            hint = " (YUV 4:2:0 images: pass frame_format='i420' or 'nv12')" if t.dim() == 2 else ""
            raise ValueError("a uint8 BGR image must be (H, W, 3); got %s%s" % (tuple(t.shape), hint))
        fmt, hw = FRAME_FORMATS["bgr"], (int(t.shape[0]), int(t.shape[1]))
    elif t.dtype == torch.float32 and frame_format is None:
        if t.dim() != 3 or t.shape[0] != 3:
            raise ValueError("an fp32 RGB image must be (3, H, W); got %s" % (tuple(t.shape),))
        fmt, hw = FRAME_RGB_F32, (int(t.shape[1]), int(t.shape[2]))
    else:
        raise ValueError("an image must be float32 RGB (3,H,W) or uint8; frame_format 'bgr' needs uint8; got dtype %s"
                         % (t.dtype,))
    for i, t in enumerate(images):
        if not t.is_contiguous():
            raise RuntimeError("image %d is not contiguous: the kernels read it in place" % i)
        if not t.is_cuda:
            raise RuntimeError("jarvis_hybridnet_amd needs CUDA (HIP) tensors; image %d is a CPU tensor" % i)
    return fmt, hw, frame_layout


def image_table(images):
    """The host array of device pointers jh_predictor*_forward_images takes (free again when the call returns)."""
    return (c_void_p * len(images))(*(t.data_ptr() for t in images))


def layout_args(fmt, layout):
    """(yuv, sensor) of jh_predictor*_forward_images: the struct the format needs, NULL for the other."""
    s = layout.struct() if layout is not None else None
    return (s if fmt == FRAME_SURFACE else None, s if fmt == FRAME_SENSOR else None)


def camera_mask(mask, shape, what="camera_mask"):
    """A camera_mask argument checked and made a contiguous uint8 CPU or device tensor of `shape` with values
    0 / 1: None stays None; a bool or integer tensor, or a sequence of bools / integers, nonzero = use the camera.
    A floating dtype or another shape raises ValueError."""
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        try:
            mask = torch.as_tensor(mask)
        except Exception as e:                              # noqa: BLE001 -- ragged / non-numeric sequences
            raise ValueError("%s must be a bool or integer tensor or sequence of shape %s: %s" % (what, tuple(shape), e))
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise ValueError("%s must be bool or integer (nonzero = use the camera); got dtype %s" % (what, mask.dtype))
    if tuple(mask.shape) != tuple(shape):
        raise ValueError("%s must have shape %s; got %s" % (what, tuple(shape), tuple(mask.shape)))
    return (mask != 0).to(torch.uint8).contiguous()


PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16x3_wide": 2}
PRECISION_DEFAULT = -1               # jh_predictor_config.precision: follow set_precision() / JH_PRECISION


def precision_id(mode):
    """jh_predictor_config.precision for a mode name; None = the process default (set_precision)."""
    if mode is None:
        return PRECISION_DEFAULT
    if mode not in PRECISIONS:
        raise ValueError("precision must be one of %s or None, got %r" % (sorted(PRECISIONS), mode))
    return PRECISIONS[mode]


def set_precision(mode):
    """Process-wide DEFAULT precision: the mode of the stand-alone networks created from now on and of
    predictors built with precision=None; a predictor built with an explicit `precision=` ignores it.
    "f32" (default, the
    parity mode), "bf16x3" (V2V's 3x3x3 convolutions and the keypoint head's ConvTranspose2d on the bf16
    matrix cores with split operands; a separately labelled reduced-precision mode) or "bf16x3_wide"
    (experimental: the trunk's dense 2D convolutions too).  Returns the previous mode."""
    prev = get_precision()
    check(lib().jh_set_precision(PRECISIONS[mode]))
    return prev


def get_precision():
    return {v: k for k, v in PRECISIONS.items()}[lib().jh_get_precision()]


def check(rc):
    if rc != 0:
        raise RuntimeError("libjarvis_hip: " + lib().jh_last_error().decode())


def ptr(t):
    """Raw address of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous"
    return t.data_ptr()


def dev(t, dtype=torch.float32):
    """Contiguous CUDA tensor of the given dtype (the API's input convention)."""
    if not t.is_cuda:
        raise RuntimeError("jarvis_hybridnet_amd needs CUDA (HIP) tensors; got a CPU tensor")
    return t.to(dtype).contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Params:
    """A state dict handed to the native side (host copies, reference key layout)."""

    def __init__(self, state_dict):
        self.handle = c_void_p()
        check(lib().jh_params_create(ctypes.byref(self.handle)))
        self._keep = []
        for key, t in state_dict.items():
            h = t.detach().to("cpu", torch.float32).contiguous()
            self._keep.append(h)
            check(lib().jh_params_set(self.handle, key.encode(), h.data_ptr(), h.numel()))

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.jh_params_destroy(self.handle)
            self.handle = None


def profile(fn):
    """Run fn() with per-launch HIP-event timing; returns a list of
    (kernel name, milliseconds, algorithmic flops, algorithmic bytes)."""
    check(lib().jh_profile_begin())
    try:
        fn()
    finally:
        n = c_int(0)
        check(lib().jh_profile_end(ctypes.byref(n)))
    out = []
    buf = ctypes.create_string_buffer(128)
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for i in range(n.value):
        check(lib().jh_profile_get(i, buf, 128, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)))
        out.append((buf.value.decode(), ms.value, fl.value, by.value))
    return out
