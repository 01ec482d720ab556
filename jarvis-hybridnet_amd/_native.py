"""ctypes binding of libjarvis_hip.so (the C ABI in include/jarvis_hip.h).

There is deliberately no fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  PyTorch is used only as the owner of device
memory and streams -- every pointer crossing this boundary is a raw address.
"""
import ctypes
import math
import os
from typing import NamedTuple

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
    """jh_yuv_surface of include/jarvis_hip.h (built by yuv_surface.YuvSurface.struct()).  The last field keeps the
    name it had when it was spare: it is the header's `sample`, the JH_SAMPLE_* code (0 = one byte per sample)."""
    _fields_ = [("image_stride", ctypes.c_int64), ("y_offset", ctypes.c_int64), ("y_pitch", ctypes.c_int64),
                ("u_offset", ctypes.c_int64), ("v_offset", ctypes.c_int64), ("c_pitch", ctypes.c_int64),
                ("c_step", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(YuvSurfaceStruct) == 64


class SensorSurfaceStruct(ctypes.Structure):
    """jh_sensor_surface of include/jarvis_hip.h (built by sensor_surface.SensorSurface.struct()).  `reserved` is the
    header's `sample`, as in YuvSurfaceStruct."""
    _fields_ = [("image_stride", ctypes.c_int64), ("offset", ctypes.c_int64), ("pitch", ctypes.c_int64),
                ("pattern", ctypes.c_int32), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(SensorSurfaceStruct) == 32


class PixelSurfaceStruct(ctypes.Structure):
    """jh_pixel_surface of include/jarvis_hip.h (built by pixel_surface.PixelSurface.struct())."""
    _fields_ = [("image_stride", ctypes.c_int64), ("offset", ctypes.c_int64 * 3), ("pitch", ctypes.c_int64 * 3),
                ("step", ctypes.c_int32 * 3), ("xs", ctypes.c_int32 * 3), ("ys", ctypes.c_int32 * 3),
                ("colour", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32),
                ("sample", ctypes.c_int32)]


assert ctypes.sizeof(PixelSurfaceStruct) == 112

class OpOperand(ctypes.Structure):
    """jh_op_operand of include/jarvis_hip.h (test entry jh_op_conv_operand): host pointers as raw addresses."""
    _fields_ = [("in_sums_host", c_void_p), ("in_act", ctypes.c_int32), ("latency_class", ctypes.c_int32),
                ("want_stats", ctypes.c_int32), ("se_c", ctypes.c_int32), ("se_s", ctypes.c_int32),
                ("se_inv_hw", c_float), ("se_wr_host", c_void_p), ("se_br_host", c_void_p),
                ("se_we_host", c_void_p), ("se_be_host", c_void_p), ("se_pool_host", c_void_p),
                ("out_sums_host", c_void_p)]


assert ctypes.sizeof(OpOperand) == 80


class OpNodeEx(ctypes.Structure):
    """jh_op_node_ex of include/jarvis_hip.h (test entry jh_op_bifpn_node_ex): host and device pointers as raw
    addresses."""
    _fields_ = [("batch_class", ctypes.c_int32), ("want_pool", ctypes.c_int32), ("in_sums_host", c_void_p * 3),
                ("in_count", ctypes.c_int64 * 3), ("y_pool_dev", c_void_p),
                ("pool_written_host", ctypes.POINTER(ctypes.c_int32)), ("out_sums_host", c_void_p)]


assert ctypes.sizeof(OpNodeEx) == 80

class SubjectsParamsStruct(ctypes.Structure):
    """jh_subjects_params of include/jarvis_hip.h (built by subjects_params())."""
    _fields_ = [("max_subjects", ctypes.c_int32), ("max_peaks", ctypes.c_int32), ("nms_radius", ctypes.c_int32),
                ("min_views", ctypes.c_int32), ("min_peak", c_float), ("max_error_px", c_float)]


assert ctypes.sizeof(SubjectsParamsStruct) == 24


class Joints3dParamsStruct(ctypes.Structure):
    """jh_joints3d_params of include/jarvis_hip.h (built by joints3d_params())."""
    _fields_ = [("min_views", ctypes.c_int32), ("refine_radius", ctypes.c_int32), ("min_conf", c_float),
                ("max_error_px", c_float)]


assert ctypes.sizeof(Joints3dParamsStruct) == 16


class TrackParamsStruct(ctypes.Structure):
    """jh_track_params of include/jarvis_hip.h (built by track_params())."""
    _fields_ = [("max_subjects", ctypes.c_int32), ("max_missed", ctypes.c_int32), ("predict", ctypes.c_int32),
                ("coast", ctypes.c_int32), ("max_jump_mm", c_float)]


class TrackStateStruct(ctypes.Structure):
    """jh_track_state of include/jarvis_hip.h: the layout of the tracker's device memory (tracks.SubjectTracker)."""
    _fields_ = [("pos", c_float * 3 * 8), ("vel", c_float * 3 * 8), ("missed", ctypes.c_int32 * 8),
                ("id", ctypes.c_int32 * 8), ("next_id", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


assert ctypes.sizeof(TrackParamsStruct) == 20 and ctypes.sizeof(TrackStateStruct) == 272

ABI_VERSION = 4                    # JH_ABI_VERSION of include/jarvis_hip.h
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
    "jh_v2v_fold": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "jh_reproject_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "jh_reproject_forward": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
    "jh_softargmax_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "jh_softargmax": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "jh_softargmax_spread_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "jh_softargmax_spread": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "jh_predictor_set_spread": (c_int, [c_void_p, c_int]),
    "jh_predictor_get_spread": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_debug_v2v": (c_int, [c_void_p, c_void_p, c_void_p]),
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
    "jh_predictor_graph_records": (c_int64, [c_void_p]),
    "jh_predictor_launches": (c_int64, [c_void_p]),
    "jh_predictor_device_bytes": (c_int64, [c_void_p]),
    "jh_predictor_precision": (c_int, [c_void_p]),
    "jh_predictor_set_calibration": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_set_calibration_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_set_centers": (c_int, [c_void_p, c_void_p, c_void_p]),
    "jh_predictor_set_tone": (c_int, [c_void_p, c_void_p, c_void_p]),
    "jh_center_keyframe_rows": (c_int, [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int]),
    "jh_predictor_set_center_keyframes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "jh_predictor_get_center_keyframes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor2d_set_tone": (c_int, [c_void_p, c_void_p, c_void_p]),
    "jh_op_frames_to_rgb_f32": (c_int, [c_void_p, c_int, ctypes.POINTER(YuvSurfaceStruct),
                                        ctypes.POINTER(SensorSurfaceStruct), ctypes.POINTER(PixelSurfaceStruct), c_int,
                                        c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "jh_predictor_stage_center":(c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
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
    "jh_pixel_surface_check": (c_int, [ctypes.POINTER(PixelSurfaceStruct), c_int, c_int]),
    "jh_op_pixels_to_bgr": (c_int, [c_void_p, ctypes.POINTER(PixelSurfaceStruct), c_int, c_int, c_int, c_void_p,
                                    c_void_p]),
    "jh_predictor_forward_pixels": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_void_p), c_int,
                                            ctypes.POINTER(PixelSurfaceStruct), c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "jh_predictor2d_forward_pixels": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_void_p), c_int,
                                              ctypes.POINTER(PixelSurfaceStruct), c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "jh_predictor_detect_subjects_pixels": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_void_p), c_int,
                                                    ctypes.POINTER(PixelSurfaceStruct), c_void_p,
                                                    ctypes.POINTER(SubjectsParamsStruct), c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_void_p]),
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
    "jh_subjects_params_check": (c_int, [ctypes.POINTER(SubjectsParamsStruct)]),
    "jh_op_center_peaks": (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(SubjectsParamsStruct), c_void_p,
                                   c_void_p, c_void_p]),
    "jh_op_associate_subjects": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         c_float, c_float, ctypes.POINTER(SubjectsParamsStruct), c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "jh_predictor_detect_subjects": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_void_p), c_int, c_int,
                                             ctypes.POINTER(YuvSurfaceStruct), ctypes.POINTER(SensorSurfaceStruct),
                                             c_void_p, ctypes.POINTER(SubjectsParamsStruct), c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_track_params_check": (c_int, [ctypes.POINTER(TrackParamsStruct)]),
    "jh_op_track_reset": (c_int, [c_void_p, c_void_p]),
    "jh_op_track_subjects": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     ctypes.POINTER(TrackParamsStruct)] + [c_void_p] * 10),
    "jh_joints3d_params_check": (c_int, [ctypes.POINTER(Joints3dParamsStruct)]),
    "jh_op_joint_peaks_refine": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                         c_void_p]),
    "jh_op_triangulate_joints": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                         ctypes.POINTER(Joints3dParamsStruct), c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "jh_predictor_triangulate_joints": (c_int, [c_void_p, c_void_p, c_int, c_void_p,
                                                ctypes.POINTER(Joints3dParamsStruct)] + [c_void_p] * 6),
    "jh_predictor_set_joint_mask": (c_int, [c_void_p, c_int, c_void_p, ctypes.POINTER(Joints3dParamsStruct), c_void_p]),
    "jh_predictor_get_joint_mask": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_stage_3d_joint_masked": (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 6),
    "jh_reproject_joint_masked_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "jh_reproject_forward_joint_masked": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_int64, c_void_p]),
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
    "jh_deconv4_window_launches": (ctypes.c_long, []),
    "jh_conv_form": (c_int, [c_int] * 12 + [c_char_p, c_int]),
    "jh_node_form": (c_int, [c_int] * 6 + [ctypes.POINTER(c_int)] + [c_int] * 3 +
                     [c_char_p, c_int, ctypes.POINTER(ctypes.c_int32)]),
    "jh_head_roi_form": (c_int, [c_int] * 7 + [ctypes.POINTER(ctypes.c_int32)]),
    "jh_op_deconv4_box": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "jh_op_repro_box": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p] +
                        [c_int] * 6 + [c_float, c_void_p, c_void_p, c_void_p]),
    "jh_predictor_debug_head_boxes": (c_int, [c_void_p, c_void_p, ctypes.POINTER(ctypes.c_int32), c_void_p]),
    "jh_op_conv_operand": (c_int, [c_int] * 7 + [c_void_p, c_void_p, c_void_p] + [c_int] * 4 +
                           [c_void_p, ctypes.POINTER(OpOperand), c_void_p, c_void_p]),
    "jh_op_se_gate": (c_int, [c_void_p, c_int, c_int, c_int, c_float] + [c_void_p] * 6),
    "jh_op_norm_apply": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                                           c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "jh_op_depthwise": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                c_void_p, c_void_p]),
    "jh_op_depthwise_pool": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p]),
    "jh_op_depthwise_ex": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "jh_op_stem": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "jh_op_yuv420_to_bgr": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "jh_op_bifpn_node": (c_int, [c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_float), c_int, c_int, c_int,
                                 c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "jh_op_bifpn_node_ex": (c_int, [c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_float), c_int, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, ctypes.POINTER(OpNodeEx), c_void_p]),
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


# JH_FRAME_* of include/jarvis_hip.h.  'rgb': fp32 RGB (3,H,W) images; 'bgr': uint8 BGR (H,W,3) images as cv2 delivers
# them; 'i420' / 'nv12': YUV 4:2:0, one contiguous (3H/2, W) uint8 image per camera, H and W even; 'surface' / 'sensor':
# image_stride bytes per image, read through a YuvSurface / a SensorSurface.
FRAME_CODES = {"rgb": 0, "bgr": 1, "i420": 2, "nv12": 3, "surface": 4, "sensor": 5}
FRAME_FORMATS = {k: FRAME_CODES[k] for k in ("bgr", "i420", "nv12")}       # the names a frame_format argument takes
YUV_FORMATS = ("i420", "nv12")
FRAME_SURFACE, FRAME_SENSOR = FRAME_CODES["surface"], FRAME_CODES["sensor"]
# What Frames.fmt carries for image_stride bytes per image read through a PixelSurface.  No JH_FRAME_* code of the header:
# the form has entry points of its own (jh_predictor_forward_pixels and its like), and this value never reaches a C
# `format` argument.
FRAME_PIXELS = 8


class Frames(NamedTuple):
    """What the frames of one call are, checked once and carried to the ctypes call: fmt the JH_FRAME_* code, height
    and width of a frame, layout the checked YuvSurface / SensorSurface or None, lead the leading shape ((T, C) of a
    3D call, (T,) of a 2D one), and the bytes: `data`, one contiguous device tensor of shape lead + (one image), or
    `images`, the flat list of prod(lead) separately placed device tensors.  Built by describe_frames and
    frame_images alone (describe_shape gives one without bytes)."""
    fmt: int
    height: int
    width: int
    layout: object
    lead: tuple
    data: object = None
    images: object = None

    @property
    def device(self):
        return self.data.device if self.images is None else self.images[0].device


def yuv_format(name):
    """The frame_format of the forms that take YUV 4:2:0 frames only (forward_yuv): 'i420' or 'nv12'."""
    if name not in YUV_FORMATS:
        raise ValueError("frame_format must be one of %s, got %r" % (list(YUV_FORMATS), name))
    return name


def surface(layout):
    """The `surface` argument of the forms that take described frames only (forward_surface): not None."""
    if layout is None:
        raise ValueError("surface must be a YuvSurface or a SensorSurface (or a PixelSurface), got None")
    return layout


def check_layout(layout, frame_format=None, hw=None):
    """A frame_layout argument checked: None stays None; otherwise a yuv_surface.YuvSurface, a
    sensor_surface.SensorSurface or a pixel_surface.PixelSurface, not combined with frame_format 'i420' / 'nv12' (the layout says what the bytes
    are) and of the frame size `hw` when that is given.  ValueError otherwise."""
    if layout is None:
        return None
    from .pixel_surface import PixelSurface
    from .sensor_surface import SensorSurface
    from .yuv_surface import YuvSurface
    if not isinstance(layout, (YuvSurface, SensorSurface, PixelSurface)):
        raise ValueError("frame_layout must be a YuvSurface or a SensorSurface (or a PixelSurface) or None, got %r"
                         % (type(layout).__name__,))
    if frame_format in YUV_FORMATS:
        raise ValueError("frame_layout describes the bytes itself: do not combine it with frame_format=%r"
                         % (frame_format,))
    if hw is not None and (layout.height, layout.width) != tuple(hw):
        raise ValueError("frame_layout is %d x %d; this predictor is %d x %d" % (layout.height, layout.width, *hw))
    return layout


def describe_shape(shape, dtype, lead, frame_format=None, frame_layout=None, hw=None, error=ValueError,
                   in_place=False, at_least=False):
    """THE rules of what frames are, on a shape and a dtype alone (no tensor, no device) -> Frames without bytes.
    lead: the leading dimensions, None entries match any size.  After them one image is
      frame_layout (a YuvSurface / SensorSurface)  uint8 (image_stride,); with at_least, image_stride bytes or more
      frame_layout (a PixelSurface)                 likewise, or uint8 of ANY shape with exactly image_stride bytes
                                                    ((H,W,3), (H,W,4), (3,H,W) tensors go in as they are)
      frame_format 'i420' / 'nv12'                  uint8 (3H/2, W), H and W even
      dtype uint8                                   BGR (H, W, 3)
      otherwise                                     fp32 RGB (3, H, W); frame_format 'bgr' refuses it
    hw: the fixed (H, W) of a predictor the frames are for; None: the shape says it.
    in_place: the bytes are read as they are, so fp32 means float32; otherwise any other dtype is taken for frames
    that the caller converts to float32.
    An unknown frame_format, a bad frame_layout and a YUV size that cannot be are ValueErrors; a dtype or shape that
    does not fit raises `error` for the fixed formats (the public predictors, the drivers and frame_images say
    ValueError, NativePredictor always said RuntimeError) and ValueError for a frame_layout.
    shape None: what was given is no tensor (dtype: its type's name)."""
    if frame_format is not None and frame_format not in FRAME_FORMATS:
        raise ValueError("frame_format must be one of %s or None, got %r" % (sorted(FRAME_FORMATS), frame_format))
    layout = check_layout(frame_layout, frame_format, hw)
    H, W = hw if hw is not None else ("H", "W")
    hint = ""
    if layout is not None:
        from .pixel_surface import PixelSurface
        from .sensor_surface import SensorSurface
        kind, error = "sensor" if isinstance(layout, SensorSurface) else "surface", ValueError
        if isinstance(layout, PixelSurface):
            kind = "pixels"
        what = "frames of a %s (%simage_stride = %d bytes per image)" % (
            type(layout).__name__, "at least " if at_least else "", layout.image_stride)
        want, tail = torch.uint8, ("image_stride" if at_least else layout.image_stride,)
        H, W = layout.height, layout.width
    elif frame_format in YUV_FORMATS:
        if hw is not None and (H % 2 or W % 2):
            raise ValueError("YUV 4:2:0 frames need an even height and width; this predictor is %d x %d" % (H, W))
        kind, what, want = frame_format, "%s frames" % frame_format, torch.uint8
        tail = (H * 3 // 2, W) if hw is not None else ("3H/2", "W")
    elif dtype == torch.uint8:
        kind, what, want, tail = "bgr", "uint8 BGR frames", torch.uint8, (H, W, 3)
        if shape is not None and len(shape) == len(lead) + 2:
            hint = " (YUV 4:2:0 frames: pass frame_format='i420' or 'nv12')"
    elif frame_format == "bgr":
        raise error("frame_format 'bgr' needs uint8 %s frames; got dtype %s" % (_shape_text(lead, (H, W, 3)), dtype))
    elif dtype == torch.float32 or (not in_place and isinstance(dtype, torch.dtype)):
        kind, what, want, tail = "rgb", "fp32 RGB frames", dtype, (3, H, W)
    else:
        raise error("frames must be float32 RGB %s or uint8 BGR %s; got dtype %s"
                    % (_shape_text(lead, (3, H, W)), _shape_text(lead, (H, W, 3)), dtype))
    full = tuple(lead) + tail
    fits = shape is not None and dtype == want and len(shape) == len(full) and all(
        not isinstance(w, int) or int(g) == w for g, w in zip(shape, full))
    if fits and at_least and layout is not None:
        fits = int(shape[-1]) >= layout.image_stride
    if not fits and kind == "pixels" and shape is not None and dtype == want and len(shape) > len(lead):
        # any trailing shape of exactly image_stride bytes
        fits = math.prod(int(n) for n in shape[len(lead):]) == layout.image_stride and all(
            w is None or int(g) == w for g, w in zip(shape, lead))
        hint = " (or any trailing shape of exactly image_stride bytes)"
    if not fits:
        raise error("%s must be %s of shape %s; got %s%s" % (
            what, "uint8" if want == torch.uint8 else "float32", _shape_text(lead, tail),
            dtype if shape is None else "dtype %s, shape %s" % (dtype, tuple(shape)), hint))
    if kind in YUV_FORMATS and hw is None:
        rows, W = int(shape[-2]), int(shape[-1])
        if rows <= 0 or rows % 3 or W <= 0 or W % 2:
            raise ValueError("a YUV 4:2:0 image is (3H/2, W) bytes with H and W even; got (%d, %d)" % (rows, W))
        H = rows // 3 * 2
    elif hw is None and layout is None:
        H, W = (int(shape[-3]), int(shape[-2])) if kind == "bgr" else (int(shape[-2]), int(shape[-1]))
    return Frames(FRAME_PIXELS if kind == "pixels" else FRAME_CODES[kind], H, W, layout, tuple(int(n) for n in shape[:len(lead)]))


def _shape_text(lead, tail):
    """(2, *, H, W, 3): a wanted shape for an error message, * for a leading dimension of any size."""
    return "(%s)" % ", ".join("*" if n is None else str(n) for n in tuple(lead) + tuple(tail))


def describe_frames(frames, lead, frame_format=None, frame_layout=None, hw=None, error=ValueError, in_place=False):
    """The frames of a call in one tensor, checked -> Frames with `data`.  The rules are describe_shape's (lead,
    frame_format, frame_layout, hw, error and in_place as there) and need no device; the device comes last:
    in_place: `frames` itself must be a contiguous device tensor (RuntimeError otherwise); else it is made one
    (_native.dev: uint8 stays uint8, the fp32 form is converted to float32; RuntimeError for a CPU tensor)."""
    shape, dtype = (frames.shape, frames.dtype) if torch.is_tensor(frames) else (None, type(frames).__name__)
    d = describe_shape(shape, dtype, lead, frame_format, frame_layout, hw, error, in_place)
    if not in_place:
        return d._replace(data=dev(frames, torch.uint8 if d.fmt else torch.float32))
    if not (frames.is_cuda and frames.is_contiguous()):
        raise RuntimeError("frames must be a contiguous CUDA (HIP) tensor")
    return d._replace(data=frames)


def frame_images(images, count, frame_format=None, frame_layout=None):
    """The images of a per-image call (forward_images) checked -> Frames with `images`.  `images`: a sequence of
    `count` tensors (count an int, or the leading shape (T, C) whose product it is), each ONE image as describe_shape
    has it with no leading dimension -- fp32 (3,H,W); uint8 (H,W,3); with frame_format 'i420' / 'nv12' uint8
    (3H/2,W); with frame_layout a 1-D uint8 tensor of at least image_stride bytes -- all of one shape, dtype and
    device, contiguous and on the GPU.  Nothing is copied: the tensors are read where they lie.
    ValueError for what does not fit the call (count, mixed images, shapes, frame_layout with 'i420' / 'nv12'),
    RuntimeError for a CPU or a non-contiguous tensor, as the contiguous forms raise them."""
    lead = (count,) if isinstance(count, int) else tuple(count)
    count = math.prod(lead)
    if not isinstance(images, (list, tuple)) or len(images) != count or not images:
        raise ValueError("expected a sequence of %d images (one tensor per image); got %s" % (
            count, len(images) if isinstance(images, (list, tuple)) else type(images).__name__))
    for i, t in enumerate(images):
        if not torch.is_tensor(t):
            raise ValueError("image %d is a %s, not a tensor" % (i, type(t).__name__))
        if (t.shape, t.dtype, t.device) != (images[0].shape, images[0].dtype, images[0].device):
            raise ValueError("the images of a call have one shape, dtype and device: image %d is %s, image 0 is %s" % (
                i, (t.dtype, tuple(t.shape), str(t.device)),
                (images[0].dtype, tuple(images[0].shape), str(images[0].device))))
    d = describe_shape(images[0].shape, images[0].dtype, (), frame_format, frame_layout, in_place=True, at_least=True)
    for i, t in enumerate(images):
        if not t.is_contiguous():
            raise RuntimeError("image %d is not contiguous: the kernels read it in place" % i)
        if not t.is_cuda:
            raise RuntimeError("jarvis_hybridnet_amd needs CUDA (HIP) tensors; image %d is a CPU tensor" % i)
    return d._replace(lead=lead, images=list(images))


def forward_symbol(which, fmt, masked=False, per_image=False):
    """The whole-path entry point of the library for a call's frames, by name.  which: 'jh_predictor' (3D) or
    'jh_predictor2d' (which takes no masks); fmt: the JH_FRAME_* code; masked: a camera mask is given; per_image: the
    frames are separately placed images.  Per-image frames of any format have one entry point, so have described
    surfaces and sensor images (their 3D forms take the mask, NULL for none); a mask on the fixed formats goes
    through the 3D predictor's masked entry point; otherwise every fixed format has its own.  Pixel surfaces have one
    entry point for contiguous and per-image frames."""
    if fmt == FRAME_PIXELS:
        return which + "_forward_pixels"
    if per_image:
        return which + "_forward_images"
    if fmt in (FRAME_SURFACE, FRAME_SENSOR):
        return which + ("_forward_surface" if fmt == FRAME_SURFACE else "_forward_sensor")
    if masked:
        return which + "_forward_masked"
    return which + ("_forward", "_forward_u8", "_forward_yuv", "_forward_yuv")[fmt]


def call_forward(which, handle, frames, mask, outs):
    """THE call into the library for the whole forward: `frames` a Frames with its bytes, mask the (T,C) uint8
    device mask or None, outs the output tensors; on the current stream.  The arguments that say what the frames
    are follow the entry point (include/jarvis_hip.h); a layout's struct lives until the call returns."""
    masks = which == "jh_predictor"
    if mask is not None and not masks:
        raise ValueError("%s takes no camera mask" % which)
    name = forward_symbol(which, frames.fmt, mask is not None, frames.images is not None)
    struct = frames.layout.struct() if frames.layout is not None else None
    if frames.fmt == FRAME_PIXELS:
        # (exactly one of the contiguous frames and the table of per-image pointers)
        n = 0 if frames.images is None else len(frames.images)
        table = (c_void_p * n)(*(t.data_ptr() for t in frames.images)) if n else None
        args = (ptr(frames.data) if not n else None, table, n, struct) + ((ptr(mask),) if masks else ())
    elif frames.images is not None:
        table = (c_void_p * len(frames.images))(*(t.data_ptr() for t in frames.images))
        args = (table, len(frames.images), frames.fmt, struct if frames.fmt == FRAME_SURFACE else None,
                struct if frames.fmt == FRAME_SENSOR else None) + ((ptr(mask),) if masks else ())
    elif struct is not None:
        args = (ptr(frames.data), struct) + ((ptr(mask),) if masks else ())
    elif mask is not None:
        args = (ptr(frames.data), frames.fmt, ptr(mask))
    else:
        args = (ptr(frames.data),) + ((frames.fmt,) if frames.fmt >= FRAME_CODES["i420"] else ())
    check(getattr(lib(), name)(handle, *args, *(ptr(t) for t in outs), stream()))


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


_CALIB_TAILS = ((4, 3), (3, 3), (1, 5))       # cameraMatrices, intrinsicMatrices, distortionCoefficients per camera


def calibration(calib, T, C):
    """The calibration arguments of a batched call checked -> (form, cam, intr, dist), form "shared" or "frames".
    calib: the three tensors (cameraMatrices, intrinsicMatrices, distortionCoefficients) in the reference's transposed
    storage, either (C,4,3) / (C,3,3) / (C,1,5) -- one calibration shared by the T frame sets
    (jh_predictor_set_calibration) -- or the same three with a leading T -- row t is the calibration of frame set t
    (jh_predictor_set_calibration_frames).  The tensors are returned as given: no copy, no device, no dtype change.
    ValueError for fewer or more than three tensors, a non-floating dtype, a wrong T or C, any other shape, and for
    a mix of the two forms."""
    if not isinstance(calib, (list, tuple)) or len(calib) != 3 or not all(torch.is_tensor(t) for t in calib):
        raise ValueError("calibration is three tensors (cameraMatrices, intrinsicMatrices, distortionCoefficients); "
                         "got %s" % ([type(t).__name__ for t in calib] if isinstance(calib, (list, tuple))
                                     else type(calib).__name__))
    names = ("cameraMatrices", "intrinsicMatrices", "distortionCoefficients")
    forms = []
    for name, t, tail in zip(names, calib, _CALIB_TAILS):
        if not t.dtype.is_floating_point:
            raise ValueError("%s must be a floating-point tensor; got dtype %s" % (name, t.dtype))
        shape = tuple(int(n) for n in t.shape)
        if shape == (C,) + tail:
            forms.append("shared")
        elif shape == (T, C) + tail:
            forms.append("frames")
        else:
            raise ValueError("%s must have shape %s (shared by the frame sets) or %s (one per frame set); got %s"
                             % (name, (C,) + tail, (T, C) + tail, shape))
    if len(set(forms)) != 1:
        raise ValueError("the three calibration tensors are either all per camera (C, ...) or all per frame set "
                         "(T, C, ...); got %s" % ", ".join("%s: %s" % nf for nf in zip(names, forms)))
    return (forms[0],) + tuple(calib)


def centers(value, T):
    """A centers argument checked and made a contiguous fp32 tensor of shape (T,3), world millimetres, one row per
    frame set (jh_predictor_set_centers): None stays None; a tensor, numpy array or sequence of shape (T,3) -- (3,) too
    when T == 1 -- of any real numeric dtype.  The device is left alone (a device tensor computed from the previous
    result costs no host synchronisation); values are not looked at -- a row that is not finite is an invalid row of
    the result, not an error.  Anything else raises ValueError."""
    if value is None:
        return None
    want = "(%d, 3)" % T + (" or (3,)" if T == 1 else "")
    if not torch.is_tensor(value):
        try:
            value = torch.as_tensor(value)
        except Exception as e:                              # noqa: BLE001 -- ragged / non-numeric sequences
            raise ValueError("centers must be a real numeric tensor, array or sequence of shape %s: %s" % (want, e))
    if value.dtype == torch.bool or value.dtype.is_complex:
        raise ValueError("centers must have a real numeric dtype; got %s" % value.dtype)
    shape = tuple(int(n) for n in value.shape)
    if shape == (3,) and T == 1:
        value = value.unsqueeze(0)
    elif shape != (T, 3):
        raise ValueError("centers must have shape %s (world millimetres, one row per frame set); got %s" % (want, shape))
    return value.to(torch.float32).contiguous()


def center_keyframe_rows(time_batch, every, n_rows=None):
    """The key rows of a time batch under centre keyframes, ascending (jh_center_keyframe_rows: the library's own rule,
    host arithmetic, no device): {0, every, 2 every, ... < n_rows} and n_rows - 1, of the first n_rows (default: all)
    rows of the batch.  ValueError for what the library refuses: time_batch < 1, every < 1, n_rows outside
    1 .. time_batch, or an argument that is no int."""
    n_rows = time_batch if n_rows is None else n_rows
    for name, v in dict(time_batch=time_batch, every=every, n_rows=n_rows).items():
        if isinstance(v, bool) or not isinstance(v, int) or abs(v) >= 2 ** 31:
            raise ValueError("%s must be an int, got %r" % (name, v))
    rows = (ctypes.c_int32 * max(1, min(time_batch, 1 << 20)))()
    n = lib().jh_center_keyframe_rows(time_batch, every, n_rows, rows, len(rows))
    if n < 0:
        raise ValueError(lib().jh_last_error().decode())
    return list(rows[:n])


def center_every(value, T):
    """A center_every argument checked -> None or (every, n_rows).  None stays None; an int k >= 1: CenterDetect on
    every k-th row of the T-row batch and on the last one; (k, n_rows): likewise for a batch whose first n_rows rows
    are real (the padded last group of a recording), 1 <= n_rows <= T.  Anything else raises ValueError."""
    if value is None:
        return None
    every, n_rows = value if isinstance(value, (tuple, list)) and len(value) == 2 else (value, T)
    if n_rows is None:
        raise ValueError("center_every=(every, n_rows): n_rows must be an int, got None")
    center_keyframe_rows(T, every, n_rows)
    return every, n_rows


def subjects_params(max_subjects, max_peaks=None, nms_radius=4, min_views=2, min_peak=50.0, max_error_px=24.0):
    """The parameters of a detect_subjects call checked -> SubjectsParamsStruct (jh_subjects_params).  The defaults are
    the library's documented defaults, not recommendations: min_peak 50 (the reference's `> 50` gate), nms_radius 4
    heat-map pixels, min_views 2, max_error_px 24 full-frame pixels; max_peaks None = min(8, 2 * max_subjects).
    Ranges (the library's own check, jh_subjects_params_check: host arithmetic, no device): max_subjects 1 .. 8,
    max_peaks 1 .. 8, nms_radius 1 .. 16, min_views >= 2, min_peak a number below +inf (-inf allowed), max_error_px
    >= 0 (+inf allowed).  ValueError for anything else, a non-integer count included."""
    ints = dict(max_subjects=max_subjects, max_peaks=max_peaks, nms_radius=nms_radius, min_views=min_views)
    if max_peaks is None and isinstance(max_subjects, int):
        ints["max_peaks"] = max(1, min(8, 2 * max_subjects))
    for name, v in ints.items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an int, got %r" % (name, v))
        if abs(v) >= 2 ** 31:
            raise ValueError("%s is out of range: %r" % (name, v))
    try:
        floats = (float(min_peak), float(max_error_px))
    except (TypeError, ValueError):
        raise ValueError("min_peak and max_error_px must be numbers, got %r and %r" % (min_peak, max_error_px))
    p = SubjectsParamsStruct(ints["max_subjects"], ints["max_peaks"], ints["nms_radius"], ints["min_views"], *floats)
    if lib().jh_subjects_params_check(ctypes.byref(p)) != 0:
        raise ValueError(lib().jh_last_error().decode())
    return p


def track_params(max_subjects, max_jump_mm, max_missed=0, predict=True, coast=False):
    """The parameters of a subject tracker checked -> TrackParamsStruct (jh_track_params).  max_jump_mm has no default:
    it is the rig's (how far an animal moves between two frame sets).  The others are documented values, not
    recommendations: max_missed 0 (a track that goes unmatched once ends), predict True (match against last position +
    velocity * frame sets elapsed), coast False (an unmatched live track's centre is NaN).  Ranges (the library's own
    check, jh_track_params_check: host arithmetic, no device): max_subjects 1 .. 8, max_missed >= 0, max_jump_mm > 0
    (+inf allowed).  ValueError for anything else, a non-integer count and a predict / coast that is no bool included."""
    for name, v in dict(max_subjects=max_subjects, max_missed=max_missed).items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an int, got %r" % (name, v))
        if abs(v) >= 2 ** 31:
            raise ValueError("%s is out of range: %r" % (name, v))
    for name, v in dict(predict=predict, coast=coast).items():
        if not (isinstance(v, int) and v in (0, 1)):            # (a bool is an int)
            raise ValueError("%s must be a bool, got %r" % (name, v))
    try:
        jump = float(max_jump_mm)
    except (TypeError, ValueError):
        raise ValueError("max_jump_mm must be a number, got %r" % (max_jump_mm,))
    p = TrackParamsStruct(max_subjects, max_missed, int(predict), int(coast), jump)
    if lib().jh_track_params_check(ctypes.byref(p)) != 0:
        raise ValueError(lib().jh_last_error().decode())
    return p


def joints3d_params(min_views=2, refine_radius=1, min_conf=0.1, max_error_px=8.0):
    """The parameters of a triangulate_joints call checked -> Joints3dParamsStruct (jh_joints3d_params).  The defaults
    are the library's documented defaults, not recommendations: min_views 2, refine_radius 1 heat-map pixel (0: the
    integer peak), min_conf 0.1, max_error_px 8 full-frame pixels.  Ranges (the library's own check,
    jh_joints3d_params_check: host arithmetic, no device): min_views >= 2, refine_radius 0 .. 3, min_conf 0 .. 1,
    max_error_px >= 0 (+inf allowed).  ValueError for anything else, a non-integer count included."""
    ints = dict(min_views=min_views, refine_radius=refine_radius)
    for name, v in ints.items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an int, got %r" % (name, v))
        if abs(v) >= 2 ** 31:
            raise ValueError("%s is out of range: %r" % (name, v))
    try:
        floats = (float(min_conf), float(max_error_px))
    except (TypeError, ValueError):
        raise ValueError("min_conf and max_error_px must be numbers, got %r and %r" % (min_conf, max_error_px))
    p = Joints3dParamsStruct(min_views, refine_radius, *floats)
    if lib().jh_joints3d_params_check(ctypes.byref(p)) != 0:
        raise ValueError(lib().jh_last_error().decode())
    return p


def triangulation_params(value):
    """What return_triangulated= / params= of the forwards accept -> Joints3dParamsStruct, or None for a false value:
    True = the defaults, a Joints3dParamsStruct (joints3d_params()) as it is, a dict = the keywords of
    joints3d_params()."""
    if value is None or value is False:
        return None
    if value is True:
        return joints3d_params()
    if isinstance(value, dict):
        return joints3d_params(**value)
    if isinstance(value, Joints3dParamsStruct):
        if lib().jh_joints3d_params_check(ctypes.byref(value)) != 0:
            raise ValueError(lib().jh_last_error().decode())
        return value
    raise ValueError("return_triangulated must be True or come from _native.joints3d_params, got %r" % (value,))


JOINT_MASK_OFF, JOINT_MASK_GIVEN, JOINT_MASK_CONSENSUS = 0, 1, 2       # JH_JOINT_MASK_* of include/jarvis_hip.h


def joint_mask(value, T, J, C):
    """A joint_mask argument checked (jh_predictor_set_joint_mask) -> None, (JOINT_MASK_GIVEN, mask) or
    (JOINT_MASK_CONSENSUS, params).  None stays None.  A bool or integer tensor (or array / sequence) of shape (T,J,C)
    -- (J,C) too when T == 1 --, host or device, nonzero = camera c counts for joint j of frame set t: made a contiguous
    uint8 tensor of (T,J,C) with values 0 / 1 on the device it is on (Triangulated3D.members of one call is a joint_mask
    of the next).  'consensus' or True: the members of the forward's own per-joint consensus, with the library's
    default parameters; a dict of joints3d_params() keywords, or what joints3d_params() made: with those.  Anything
    else -- False, another string, a floating dtype, another shape -- raises ValueError."""
    if value is None:
        return None
    if value is True or (isinstance(value, str) and value == "consensus"):
        return JOINT_MASK_CONSENSUS, joints3d_params()
    if isinstance(value, (dict, Joints3dParamsStruct)):
        return JOINT_MASK_CONSENSUS, triangulation_params(value)
    if value is False or isinstance(value, str):
        raise ValueError("joint_mask must be None, a (%d, %d, %d) bool / integer tensor, 'consensus' / True, or the "
                         "parameters of joints3d_params; got %r" % (T, J, C, value))
    if not torch.is_tensor(value):
        try:
            value = torch.as_tensor(value)
        except Exception as e:                              # noqa: BLE001 -- ragged / non-numeric sequences
            raise ValueError("joint_mask must be a bool or integer tensor or sequence of shape (%d, %d, %d): %s"
                             % (T, J, C, e))
    if T == 1 and tuple(value.shape) == (J, C):
        value = value.unsqueeze(0)
    return JOINT_MASK_GIVEN, camera_mask(value, (T, J, C), "joint_mask")


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
