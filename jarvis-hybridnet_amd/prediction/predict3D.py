"""Output side of the predict3D driver (mirrors jarvis/prediction/predict3D.py:64-70,
87-97,141-155): `data3D.csv` rows and `info.yaml`, so that the
reference's visualisation / analysis tools consume the results unchanged.

Video decoding (cv2.VideoCapture) and project management are outside the hot path:
`predict3D_frames` takes any iterable of decoded multi-view frame sets instead.
"""
import csv
import itertools
import json
import os
import re

import torch

from .. import _native as N

_PLAIN = re.compile(r"^[A-Za-z0-9_./\\][A-Za-z0-9_./\\ +=,@%-]*$")
_RESERVED = {"", "~", "null", "true", "false", "yes", "no", "on", "off", "y", "n"}


def yaml_scalar(val):
    """One YAML scalar.  Numbers and None as such; strings plain when that is unambiguous,
    double-quoted (JSON escapes are valid YAML) otherwise -- a `recording_path` containing
    ': ', '#', quotes or a leading '-' / '*' must still load as the same string."""
    if val is None:
        return "null"
    if isinstance(val, bool):
        return "true" if val else "false"
    if isinstance(val, (int, float)):
        return repr(val)
    s = str(val)
    numberlike = re.match(r"^[-+.]?[0-9]", s) is not None or s.lower() in (".inf", ".nan")
    if (_PLAIN.match(s) and s.lower() not in _RESERVED and not numberlike and s == s.strip()
            and ": " not in s and " #" not in s and not s.endswith(":")):
        return s
    return json.dumps(s)


def create_header(writer, cfg):
    """Two header rows: every joint name four times, then x,y,z,confidence per joint."""
    joints = list(itertools.chain.from_iterable(itertools.repeat(x, 4) for x in cfg.KEYPOINT_NAMES))
    coords = ["x", "y", "z", "confidence"] * len(cfg.KEYPOINT_NAMES)
    writer.writerow(joints)
    writer.writerow(coords)


def create_info_file(params, keys=("recording_path", "dataset_name", "frame_start", "number_frames")):
    """info.yaml with the four keys the reference writes (predict3D.py:149-155; a block
    mapping in the reference's key order; strings quoted where YAML needs it)."""
    with open(os.path.join(params.output_dir, "info.yaml"), "w") as f:
        for key in keys:
            f.write("%s: %s\n" % (key, yaml_scalar(getattr(params, key))))


def frame_row(points3D, confidences, num_joints):
    """One CSV row: [x, y, z, confidence] per joint, or 'NaN' x 4J when the predictor
    returned (None, None).  Same element types as the reference (Python floats from
    `.tolist()`, numpy float32 confidences), hence the same text."""
    if points3D is None:
        return ["NaN"] * (num_joints * 4)
    row = []
    for point, conf in zip(points3D.squeeze(), confidences.squeeze().cpu().numpy()):
        row = row + point.tolist() + [conf]
    return row


SPREAD_COLUMNS = ("cxx", "cxy", "cxz", "cyy", "cyz", "czz", "px", "py", "pz")


def spread_row(cov, peak, num_joints):
    """One row of spread3D.csv from a frame set's slice of a `Spread3D`: cov (J,3,3) mm^2, peak (J,3) mm ->
    [cxx, cxy, cxz, cyy, cyz, czz, px, py, pz] per joint as numpy float32 elements (the element type of the
    confidences in data3D.csv), or 'NaN' x 9J when the frame set is invalid (cov None)."""
    if cov is None:
        return ["NaN"] * (num_joints * len(SPREAD_COLUMNS))
    cov = cov.detach().cpu().float().reshape(num_joints, 9).numpy()
    peak = peak.detach().cpu().float().reshape(num_joints, 3).numpy()
    row = []
    for c, p in zip(cov, peak):
        row = row + [c[0], c[1], c[2], c[4], c[5], c[8]] + list(p)
    return row


def create_header_spread(writer, cfg):
    """Two header rows: every joint name nine times, then SPREAD_COLUMNS per joint."""
    names = list(cfg.KEYPOINT_NAMES)
    writer.writerow(list(itertools.chain.from_iterable(itertools.repeat(x, len(SPREAD_COLUMNS)) for x in names)))
    writer.writerow(list(SPREAD_COLUMNS) * len(names))


TRIANGULATED_COLUMNS = ("x", "y", "z", "views", "error")


def triangulated_row(points, views, error, num_joints):
    """One row of triangulated3D.csv from a frame set's slice of a `Triangulated3D`: points (J,3) mm, views (J), error
    (J) px -> [x, y, z, views, error] per joint, the floats as numpy float32 elements (the element type of the
    confidences in data3D.csv), views as an int; an empty joint (views 0) is ['NaN', 'NaN', 'NaN', 0, 'NaN'], an
    invalid frame set (points None) 'NaN' x 5J."""
    if points is None:
        return ["NaN"] * (num_joints * len(TRIANGULATED_COLUMNS))
    points = points.detach().cpu().float().reshape(num_joints, 3).numpy()
    views = views.detach().cpu().reshape(num_joints).numpy()
    error = error.detach().cpu().float().reshape(num_joints).numpy()
    row = []
    for p, v, e in zip(points, views, error):
        row = row + (list(p) + [int(v), e] if int(v) > 0 else ["NaN"] * 3 + [0, "NaN"])
    return row


def create_header_triangulated(writer, cfg):
    """Two header rows: every joint name five times, then TRIANGULATED_COLUMNS per joint."""
    names = list(cfg.KEYPOINT_NAMES)
    writer.writerow(list(itertools.chain.from_iterable(itertools.repeat(x, len(TRIANGULATED_COLUMNS)) for x in names)))
    writer.writerow(list(TRIANGULATED_COLUMNS) * len(names))


SUBJECT_COLUMNS = ("id", "cx", "cy", "cz", "views", "error", "missed")


def subjects_row(centers, views, error, ids=None, missed=None, dropped=0):
    """One row of subjects3D.csv from a frame set's slice of a `Subjects` -- centers (K,3) mm, views (K), error (K) px
    -- and of a `Tracks` -- ids (K), missed (K), dropped -- or None for both (no tracker: id -1, missed -1) ->
    [id, cx, cy, cz, views, error, missed] per slot, then dropped: ints as ints, the floats as numpy float32 elements
    (the element type of the confidences in data3D.csv), 'NaN' for a NaN."""
    import math
    centers = centers.detach().cpu().float().reshape(-1, 3).numpy()
    error = error.detach().cpu().float().reshape(-1).numpy()
    row = []
    for k in range(centers.shape[0]):
        row.append(-1 if ids is None else int(ids[k]))
        row += ["NaN" if math.isnan(v) else v for v in centers[k]]
        row += [int(views[k]), "NaN" if math.isnan(error[k]) else error[k], -1 if missed is None else int(missed[k])]
    return row + [int(dropped)]


def create_header_subjects(writer, max_subjects):
    """Two header rows: subject<k> once per column of the slot, then SUBJECT_COLUMNS per slot; `dropped` closes both."""
    n = len(SUBJECT_COLUMNS)
    writer.writerow(list(itertools.chain.from_iterable(itertools.repeat("subject%d" % k, n)
                                                       for k in range(max_subjects))) + ["dropped"])
    writer.writerow(list(SUBJECT_COLUMNS) * max_subjects + ["dropped"])


def _tracker(track, max_subjects):
    """The driver's `track` argument -> a tracks.SubjectTracker of max_subjects slots, or None: None stays None, a
    SubjectTracker is taken as it is (its slots must be max_subjects), a dict is its keywords.  ValueError otherwise."""
    from ..tracks import SubjectTracker, check_tracker
    if track is None or isinstance(track, SubjectTracker):
        return check_tracker(track, max_subjects)
    if not isinstance(track, dict):
        raise ValueError("track must be a dict of SubjectTracker's keywords, a SubjectTracker or None, got %r" % (track,))
    if "max_subjects" in track or "max_jump_mm" not in track:
        raise ValueError("track takes max_jump_mm (required), max_missed, predict, coast and device; the slots are "
                         "max_subjects")
    return SubjectTracker(max_subjects, **track)


def views2d_row(points2D, confidences2D, used, num_joints):
    """One row of a camera's data2D_<name>.csv from its slice of a frame set's `Views2D`: points2D (J,2),
    confidences2D (J): predict2D.frame_row of the same numbers ([x, y, confidence] per joint), or 'NaN' x 3J when
    the camera is not used in that frame set (masked, or the frame set is invalid)."""
    from .predict2D import frame_row as frame_row_2d
    if not int(used):
        return frame_row_2d(None, None, num_joints)
    return frame_row_2d(points2D.long(), confidences2D, num_joints)


def reprojection_error_row(errors):
    """One row of reprojection_error.csv: the (C,J) reprojection errors of a frame set in pixels, camera-major,
    as numpy float32 elements (the element type of the confidences in the other files); 'NaN' where the error is
    undefined (a camera that is not used in the frame set)."""
    import math
    return ["NaN" if math.isnan(v) else v for v in errors.detach().cpu().float().reshape(-1).numpy()]


def create_header_reprojection_error(writer, cfg, camera_names):
    """Two header rows: every camera name once per joint, then the joint names once per camera."""
    names = list(cfg.KEYPOINT_NAMES)
    writer.writerow(list(itertools.chain.from_iterable(itertools.repeat(c, len(names)) for c in camera_names)))
    writer.writerow(names * len(camera_names))


def predict3D_frames(predictor, frame_sets, cameraMatrices, intrinsicMatrices,
                     distortionCoefficients, cfg, output_dir, params=None, time_batch=1, streams=1,
                     frame_spec=None, frame_format="bgr", camera_mask=None, output_2d=False, camera_names=None,
                     frame_layout=None, centers=None, output_spread=False, output_triangulated=False,
                     max_subjects=None, subject_params=None, track=None, joint_mask=None, tone=None,
                     center_every=None):
    """Run `predictor` over an iterable of multi-view frame sets -- (C,H,W,3) uint8 BGR
    arrays / tensors exactly as cv2 delivers them, or (C,3,H,W) fp32 RGB -- and write
    data3D.csv (+ info.yaml when `params` is given).  Returns the number of frames.

    Ingest is overlapped as in the reference driver, which reads the next frame set with 12 threads
    and uploads it while nothing else waits (predict3D.py:72-85): frame sets are copied into pinned
    staging buffers by a thread pool as the iterator yields them, uploaded per time batch on a copy
    stream and consumed by `streams` predictors on their own HIP streams (`_ingest.FramePipeline`;
    no `torch.stack`, no pageable host->device copy).  An item of `frame_sets` may also be a callable
    `fill(dst)` that decodes one frame set straight into the pinned numpy view `dst` (the reference's
    `read_images(cap, slice, imgs_orig)` pattern; pass `frame_spec=((C,H,W,3), torch.uint8)` then).

    time_batch > 1 groups that many consecutive frame sets into one launch sequence
    (the throughput form the bench measures); rows are written in frame
    order and are the same as with time_batch = 1 -- bit for bit up to time_batch 7; from 8 on (the class in which
    the high-resolution BiFPN nodes run in their row-streaming form and the InstanceNorm / pooled-sum passes take
    >= 64 KB blocks) to 2-6e-5 mm for the small and medium models and 1.8e-4 mm for the large
    one (measured; tests/test_hip_predictor.py::test_predictor3d_time_batch_8_vs_fixture holds 3e-4).  A row does
    not depend on its position in the group, on the group size inside a class, or on `streams`.
    A short last group is padded with its last frame set and the padding rows are dropped.
    streams > 1 keeps that many groups in flight on as many HIP streams (host frame sets and frame sets already
    resident in HBM alike); rows still come out in frame order and are identical to the streams = 1 run.

    Retained memory: the predictor keeps ONE ingest pipeline (streams + 2 pinned host buffers and as many HBM
    buffers of a whole time batch, e.g. 7.5 GB + 7.5 GB at 12 x 1280 x 1024 uint8, T = 32, 3 streams) for the next
    call with the same frame format; a call with another format / time batch / stream count replaces it, an
    aborted call drops it, `_ingest.release_ingest_buffers(predictor)` frees it.

    frame_format 'i420' / 'nv12': the frame sets are (C,3H/2,W) uint8 YUV 4:2:0 as video decoders produce them
    (FFmpeg yuv420p / hardware NV12; H and W even; fill callables with `frame_spec=((C,3H/2,W), torch.uint8)`): half
    the bytes of BGR to stage and upload, converted inside the resize / crop kernels (JarvisPredictor3D.forward_yuv).
    The default 'bgr' is the behaviour described above.  Anything else raises ValueError.

    frame_layout: a YuvSurface -- the frame sets are (C, image_stride) uint8, one described YUV 4:2:0 surface per
    camera (pitched decoder output, I420 / YV12 / NV12 / NV21, BT.601 / BT.709, limited / full range; fill callables
    with `frame_spec=((C, image_stride), torch.uint8)`; device-resident frame sets likewise), read in place
    (JarvisPredictor3D.forward_surface).  Or a PixelSurface -- (C, image_stride) uint8, or any (C, ...) uint8 with exactly
    image_stride bytes per camera, such as (C,H,W,3) RGB or (C,H,W,4) BGRA arrays as they are.
    Or a SensorSurface -- the frame sets are (C, image_stride) uint8 raw
    sensor images, Mono8 or an 8-bit Bayer mosaic as a machine-vision camera delivers them: a third of the bytes of
    BGR to stage and upload, demosaiced inside the resize / crop kernels.  Not together with frame_format
    'i420' / 'nv12': ValueError.  The predictor is given `frame_layout=` only when it is set here.

    camera_mask: a (C,) bool / integer mask for the whole run (the reference's `cameras_to_use` subset: the rows
    are those of a predictor built for the unmasked cameras alone, fed their frames and calibration), or an iterable
    that yields one (C,) mask -- or None for all cameras -- per frame set, consumed in step with `frame_sets` (a
    camera that dropped a frame: mask it for that frame set; whatever its slot holds is ignored).  A frame set with
    fewer than two cameras left gives a 'NaN' row, like one in which fewer than two cameras detect.  A mask of the
    wrong shape or of a floating dtype, and a mask iterable that ends before the frame sets do, or after, raise
    ValueError.  The CSV and info.yaml formats do not change.

    output_2d: also write, beside data3D.csv (which, like info.yaml, is byte-identical with and without the option),
    the per-camera 2D views of every frame set (JarvisPredictor3D.forward(..., return_2d=True): no second pass over
    the videos): `data2D_<name>.csv` per camera in the format of the predict2D driver (rows of predict2D.frame_row,
    the header of predict2D.create_header when data3D.csv gets its header; 'NaN' x 3J where the camera is not used:
    masked in that frame set, or the frame set is invalid) and `reprojection_error.csv`, one row per frame set of
    C * J distances in pixels between a camera's 2D keypoint and the projection of the 3D keypoint, camera-major,
    'NaN' where undefined, under a camera-name row and a joint-name row.  camera_names: C names, default
    Camera_0 ...  These 2D keypoints are HybridNet's own detections, on the crop around the projection of the
    TRIANGULATED centre; the predict2D driver (JarvisPredictor2D) crops around each camera's own centre detection.
    The two agree wherever the crops cover the subject; they are not bit-equal.

    centers: where the subject is, in world millimetres -- stage 1 (resize, CenterDetect, arg-max, triangulation) then
    does not run (JarvisPredictor3D.forward_batch(..., centers=)).  One (3,) centre for the whole run (a fixed volume),
    or an iterable that yields one (3,) centre -- or None -- per frame set, consumed in step with `frame_sets` exactly
    as camera_mask is (a tracker's or another detector's answer per frame).  None, or a centre that is not finite,
    gives that frame set a 'NaN' row; the rows of the others are those of a detected run that found these centres,
    byte for byte.  A wrong shape, and an iterable that ends before the frame sets do, or after, raise ValueError.  The
    padding rows of a short last group repeat the last centre.  It composes with camera_mask, output_2d, frame_format,
    frame_layout, time_batch and streams; the CSV and info.yaml formats do not change.

    output_spread: also write `spread3D.csv` beside data3D.csv (which, like info.yaml, is byte-identical with and
    without the option): one row per frame set, per joint the six covariance entries of its 3D heat map in mm^2 and the
    voxel of its maximum in mm -- cxx,cxy,cxz,cyy,cyz,czz,px,py,pz (JarvisPredictor3D.forward_batch(...,
    return_spread=True); rows of spread_row, the header of create_header_spread when data3D.csv gets its header) --,
    'NaN' x 9J for an invalid frame set.  It composes with time_batch, streams, camera_mask, centers and output_2d.

    output_triangulated (True = the library's defaults, or what _native.joints3d_params made, or a dict of its
    keywords): also write `triangulated3D.csv` beside data3D.csv (which, like info.yaml, is byte-identical with and
    without the option): one row per frame set, per joint the 3D point triangulated from the cameras' own 2D keypoints
    with the cameras that disagree left out, the number of cameras that agree and their mean reprojection error in
    pixels -- x,y,z,views,error (JarvisPredictor3D.forward_batch(..., return_triangulated=); rows of triangulated_row,
    the header of create_header_triangulated when data3D.csv gets its header) --, 'NaN' for an empty joint's numbers
    and for an invalid frame set.  It composes with time_batch, streams, camera_mask, centers, output_2d and
    output_spread.

    max_subjects = K (1 .. 8): a recording with several animals.  Every batch goes through forward_subjects
    (JarvisPredictor3D.forward_subjects / MultiStreamPredictor.forward_subjects): up to K subjects are detected per frame
    set and each gets its own centred forward.  subject_params: a dict of detect_subjects' keywords (max_peaks,
    nms_radius, min_views, min_peak, max_error_px).  track: a dict of tracks.SubjectTracker's keywords -- max_jump_mm,
    the rig's, is required; max_missed, predict, coast -- or a SubjectTracker of K slots; ONE tracker lives for the run
    and is updated batch after batch in frame order, on the device, whatever `streams` is.  track=None: the rows are in
    detection order -- most views first within each frame set -- and have NO identity: file k is then not one animal.
    Files, in place of data3D.csv (which is not written in this mode; info.yaml is):
      data3D_subject{k}.csv  k = 0 .. K-1, the slot (the row, without a tracker): exactly the format and header of
                             data3D.csv; the 'NaN' row where the slot holds no detection in that frame set -- with
                             coast=True it holds the forward at the track's predicted centre -- or the row is invalid.
      subjects3D.csv         one row per frame set: per slot id,cx,cy,cz,views,error,missed -- the track's identity (-1:
                             the slot is free, or there is no tracker), the centre in world mm ('NaN' when empty), the
                             cameras that support it (0 when empty), their mean reprojection error in pixels ('NaN'),
                             the frame sets since the track's last match (-1: free, or no tracker) -- and last
                             `dropped`, the detections of the frame set that found no slot; under a row of slot names
                             and a row of column names when data3D_subject{k}.csv get their header.
    It works with time_batch, streams, camera_mask, frame_format and frame_layout, and the files do not depend on
    time_batch (below 8, as above) or streams.  The padding rows of a short last group pass through the tracker behind
    the real ones: a SubjectTracker handed in is not where the recording ended once the call returns (reset() it before
    it is used again).  Together with centers, output_2d, output_spread or output_triangulated: ValueError; so are
    subject_params or track without max_subjects.  Calls without max_subjects are untouched.

    joint_mask ('consensus' or True = the library's defaults, or what _native.joints3d_params made, or a dict of its
    keywords): every forward is the joint-masked one (JarvisPredictor3D.forward_batch(..., joint_mask=)) -- per joint,
    the cameras whose own 2D keypoint disagrees with the consensus of the others are left out of that joint's voxel
    volume --, so data3D.csv holds the joint-masked keypoints, and `joint_cameras.csv` is written beside it: one row per
    frame set, per joint count,cameras -- the number of cameras the joint was averaged over and their set as the decimal
    sum of 2^c (rows of joint_mask.joint_cameras_row, the header of joint_mask.create_header_joint_cameras when
    data3D.csv gets its header) --, 'NaN' x 2J for an invalid frame set.  It composes with time_batch, streams,
    camera_mask, centers and the other outputs; a tensor-valued mask is not taken here, and together with max_subjects
    it is a ValueError.

    tone: a ToneTables of NUM_CAMERAS cameras (black level, gain, white balance and gamma per camera and channel as one
    byte-to-value table, applied inside the resize / crop fetch): the run is made under predictor.set_tone(tone), and
    its files are byte-identical to those of a run on the fp32 frames tables[c][ch][bytes].  Byte frames only (fp32
    frame sets raise RuntimeError).  The predictor keeps the setting afterwards; None leaves it as it is.

    center_every = k (an int >= 1): CenterDetect runs on every k-th frame set of a group of time_batch consecutive frame
    sets and on its last one; the frame sets in between take a centre interpolated linearly between their two key frame
    sets, and every frame set then runs as under centers= (JarvisPredictor3D.forward_batch(..., center_every=)).  A
    short last group passes its real row count, so its padding rows never serve as keys for real rows.  With k > 1 THE
    RESULT DEPENDS ON time_batch: the key rows are rows of the group, so another time_batch detects on other frame sets
    and interpolates over other spans (and time_batch = 1 makes every frame set a key).  It does not depend on
    `streams`.  k = 1 gives the rows of the run without the option, byte for byte.  The files and their formats do not
    change.  Together with centers or max_subjects: ValueError.  Whether a trained network keeps its accuracy under a
    given k at a rig's frame rate is the user's to measure."""
    import contextlib
    from ..joint_mask import create_header_joint_cameras, joint_cameras_row
    from ._ingest import check_driver_frames, driver_format, host_outputs, pipeline_for
    yuv = driver_format(frame_format, frame_spec, 3, frame_layout)
    if tone is not None:
        predictor.set_tone(tone)
    tri_params = N.triangulation_params(output_triangulated)
    tail = 3 if tri_params is not None else 0                   # (points, views and error of the Triangulated3D ...)
    jm_params = None
    if joint_mask is not None:
        if torch.is_tensor(joint_mask) or isinstance(joint_mask, (list, tuple)) or hasattr(joint_mask, "__array__"):
            raise ValueError("predict3D_frames takes joint_mask='consensus' or the consensus' parameters, not a mask")
        jm_params = N.joint_mask(joint_mask, 1, 1, 1)[1]
    jm_tail = 2 if jm_params is not None else 0                 # (... then cameras and count of the JointMask, last)
    time_batch, streams = max(1, int(time_batch)), max(1, int(streams))
    if center_every is not None:
        if isinstance(center_every, (tuple, list)):
            raise ValueError("predict3D_frames takes center_every as one int: the driver knows the rows of its groups")
        center_every = N.center_every(center_every, time_batch)[0]
        if centers is not None:
            raise ValueError("center_every does not combine with centers")
    subj_params, tracker = None, None
    if max_subjects is not None:
        clash = [name for name, on in (("centers", centers is not None), ("output_2d", output_2d),
                                       ("center_every", center_every is not None),
                                       ("output_spread", output_spread), ("output_triangulated", tri_params is not None),
                                       ("joint_mask", jm_params is not None))
                 if on]
        if clash:
            raise ValueError("max_subjects does not combine with %s" % ", ".join(clash))
        if subject_params is not None and not isinstance(subject_params, dict):
            raise ValueError("subject_params must be a dict of detect_subjects' keywords, got %r" % (subject_params,))
        subj_params = N.subjects_params(max_subjects, **(subject_params or {}))
        tracker = _tracker(track, max_subjects)
    elif subject_params is not None or track is not None:
        raise ValueError("subject_params and track need max_subjects")
    run_mask, mask_iter = None, None
    if camera_mask is not None:
        C = cfg.HYBRIDNET.NUM_CAMERAS
        if _is_single_mask(camera_mask):
            run_mask = N.camera_mask(camera_mask, (C,)).cpu()
        else:
            mask_iter = iter(camera_mask)
    run_center, center_iter = None, None
    if centers is not None:
        if _is_single_mask(centers):
            run_center = _center(centers)
        else:
            center_iter = iter(centers)
    os.makedirs(output_dir, exist_ok=True)
    if params is not None:
        params.output_dir = output_dir
        create_info_file(params)
    J = cfg.KEYPOINTDETECT.NUM_JOINTS
    calib = (cameraMatrices, intrinsicMatrices, distortionCoefficients)
    n = 0
    if output_2d:
        num_cams = cfg.HYBRIDNET.NUM_CAMERAS
        camera_names = ["Camera_%d" % i for i in range(num_cams)] if camera_names is None else list(camera_names)
        if len(camera_names) != num_cams or len(set(camera_names)) != num_cams:
            raise ValueError("camera_names must be %d distinct names, got %r" % (num_cams, camera_names))
    with contextlib.ExitStack() as files:
        def open_csv(name):
            f = files.enter_context(open(os.path.join(output_dir, name), "w", newline=""))
            return csv.writer(f, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)

        names = getattr(cfg, "KEYPOINT_NAMES", [])
        writer, writers_subj, writer_tracks = None, [], None
        if max_subjects is None:
            writer = open_csv("data3D.csv")
            if len(names) == J:
                create_header(writer, cfg)
        else:
            writers_subj = [open_csv("data3D_subject%d.csv" % k) for k in range(max_subjects)]
            writer_tracks = open_csv("subjects3D.csv")
            if len(names) == J:
                for w in writers_subj:
                    create_header(w, cfg)
                create_header_subjects(writer_tracks, max_subjects)
        writers_2d, writer_err = [], None
        if output_2d:
            from .predict2D import create_header as create_header_2d
            writers_2d = [open_csv("data2D_%s.csv" % name) for name in camera_names]
            writer_err = open_csv("reprojection_error.csv")
            if len(names) == J:
                for w in writers_2d:
                    create_header_2d(w, cfg)
                create_header_reprojection_error(writer_err, cfg, camera_names)
        writer_spread = None
        if output_spread:
            writer_spread = open_csv("spread3D.csv")
            if len(names) == J:
                create_header_spread(writer_spread, cfg)

        writer_tri = None
        if tri_params is not None:
            writer_tri = open_csv("triangulated3D.csv")
            if len(names) == J:
                create_header_triangulated(writer_tri, cfg)

        writer_jm = None
        if jm_params is not None:
            writer_jm = open_csv("joint_cameras.csv")
            if len(names) == J:
                for row in create_header_joint_cameras(names):
                    writer_jm.writerow(row)

        def emit(outs, real):
            pts, conf, valid = outs[:3]
            if jm_params is not None:
                outs, (jm_cams, jm_count) = outs[:-2], outs[-2:]
            for t in range(real):
                ok = int(valid[t]) != 0
                writer.writerow(frame_row(pts[t] if ok else None, conf[t] if ok else None, J))
                if output_spread:
                    cov, peak = outs[-3 - tail], outs[-2 - tail]
                    writer_spread.writerow(spread_row(cov[t] if ok else None, peak[t] if ok else None, J))
                if tri_params is not None:
                    tp, tv, te = outs[-3:]
                    writer_tri.writerow(triangulated_row(tp[t] if ok else None, tv[t], te[t], J))
                if jm_params is not None:
                    writer_jm.writerow(joint_cameras_row(jm_cams[t].tolist(), jm_count[t].tolist(), ok))
                if output_2d:
                    p2d, c2d, _, err, used = outs[3:8]
                    for c, w in enumerate(writers_2d):
                        w.writerow(views2d_row(p2d[t, c], c2d[t, c], used[t, c], J))
                    writer_err.writerow(reprojection_error_row(err[t]))

        ring = {}                                               # pinned host copies of the outputs, per slot

        def written(outs):
            """The tensors of a batch that a file gets: the five of a Triangulated3D cut to points, views, error."""
            if center_every is not None:                         # (the CenterKeyframes' two tensors: no file holds them)
                outs = outs[:-2]
            if tri_params is None:
                return outs
            end = len(outs) - jm_tail
            return tuple(outs[:end - 5]) + (outs[end - 5], outs[end - 4], outs[end - 2]) + tuple(outs[end:])

        def submit(x, slot, mask=None, centers=None, rows=None):
            kw = {} if mask is None else {"camera_mask": mask}
            if center_every is not None:
                kw["center_every"] = (center_every, time_batch if rows is None else rows)
            if centers is not None:
                kw["centers"] = centers
            if output_2d:
                kw["return_2d"] = True
            if output_spread:
                kw["return_spread"] = True
            if tri_params is not None:
                kw["return_triangulated"] = tri_params
            if jm_params is not None:
                kw["joint_mask"] = jm_params
            if frame_layout is not None:
                kw["frame_layout"] = frame_layout
            if hasattr(predictor, "native_streams"):
                d = N.describe_shape(x.shape, x.dtype, (time_batch, None), frame_format if yuv else None, frame_layout)
                msp = predictor.native_streams(d.height, d.width, time_batch, streams)
                msp.set_calibration(*calib)
                # results leave for pinned host memory on the forward's own stream (behind it, before its event)
                # (of a Triangulated3D only what the CSV holds: members and observations stay on the device)
                res = msp.forward(x, then=lambda outs: host_outputs(ring, slot, written(outs)),
                                  frame_format=frame_format if yuv else None, **kw)
                return res, msp.last_event
            # any object with the batch interface
            res = predictor.forward_batch(x, *calib, frame_format=frame_format, **kw) if yuv else \
                predictor.forward_batch(x, *calib, **kw)
            tri = ()
            if center_every is not None:
                res = tuple(res[:-1])                          # (the CenterKeyframes: no file holds it)
            if jm_params is not None:
                res, tri = tuple(res[:-1]), tuple(res[-1])     # (the JointMask's two tensors go last)
            if tri_params is not None:
                res, tri = tuple(res[:-1]), (res[-1].points, res[-1].views, res[-1].error) + tri
            if output_spread:
                res = tuple(res[:-1]) + tuple(res[-1])         # (..., Spread3D) -> its three tensors
            if output_2d:
                res = tuple(res[:3]) + tuple(res[3]) + tuple(res[4:])     # (points, conf, valid, Views2D, ...) -> tensors
            res = tuple(res) + tri
            ev = None
            if x.is_cuda:
                res = host_outputs(ring, slot, res)
                ev = torch.cuda.Event()
                ev.record()
            return res, ev

        def emit_subjects(outs, real):
            """outs: points (T,K,J,3), conf (T,K,J), valid (T,K), centers, views, error[, ids, missed, dropped]."""
            pts, conf, valid, ctr, views, err = outs[:6]
            ids, missed, dropped = outs[6:9] if tracker is not None else (None, None, None)
            for t in range(real):
                for k, w in enumerate(writers_subj):
                    ok = int(valid[t, k]) != 0
                    w.writerow(frame_row(pts[t, k] if ok else None, conf[t, k] if ok else None, J))
                writer_tracks.writerow(subjects_row(ctr[t], views[t], err[t], None if ids is None else ids[t],
                                                    None if ids is None else missed[t],
                                                    0 if ids is None else dropped[t]))

        def submit_subjects(x, slot, mask=None):
            kw = {} if mask is None else {"camera_mask": mask}
            if frame_layout is not None:
                kw["frame_layout"] = frame_layout
            if yuv:
                kw["frame_format"] = frame_format

            def written(outs):
                # (members and slots stay on the device: no file holds them)
                return tuple(outs[:5]) + (outs[6],) + ((outs[7], outs[9], outs[10]) if tracker is not None else ())

            if hasattr(predictor, "native_streams"):
                d = N.describe_shape(x.shape, x.dtype, (time_batch, None), frame_format if yuv else None, frame_layout)
                msp = predictor.native_streams(d.height, d.width, time_batch, streams)
                msp.set_calibration(*calib)
                res = msp.forward_subjects(x, subj_params, tracker,
                                           then=lambda outs: host_outputs(ring, slot, written(outs)), **kw)
                return res, msp.last_event
            # any object with forward_subjects
            res = predictor.forward_subjects(x, *calib, max_subjects, tracker=tracker, **kw, **(subject_params or {}))
            res = written(tuple(res[:3]) + tuple(res[3]) + (tuple(res[4]) if tracker is not None else ()))
            ev = None
            if x.is_cuda:
                res = host_outputs(ring, slot, res)
                ev = torch.cuda.Event()
                ev.record()
            return res, ev

        submit.takes_rows = True                               # (the pipelines say how many rows of a batch are real)
        if max_subjects is not None:
            submit, emit = submit_subjects, emit_subjects

        pipe, key = None, None
        _end = object()
        try:
            for frames in frame_sets:
                mask = run_mask
                if mask_iter is not None:
                    mask = next(mask_iter, _end)
                    if mask is _end:
                        raise ValueError("camera_mask yielded fewer masks than there are frame sets")
                    mask = None if mask is None else N.camera_mask(mask, (C,)).cpu()
                center = run_center
                if center_iter is not None:
                    center = next(center_iter, _end)
                    if center is _end:
                        raise ValueError("centers yielded fewer centres than there are frame sets")
                    # (None inside a centred run: a NaN centre, i.e. an invalid frame set -- rows do not mix forms)
                    center = torch.full((3,), float("nan")) if center is None else _center(center)
                if not callable(frames):
                    frames = frames if torch.is_tensor(frames) and frames.is_cuda else _as_host(frames)
                    if yuv or frame_layout is not None:
                        check_driver_frames(frames, frame_format, 3, frame_layout)
                    k = (frames.dtype, tuple(frames.shape), torch.is_tensor(frames))
                else:
                    k = key if key is not None else ("fill",)
                if pipe is None or k != key:                        # first frame set, or a new frame format
                    if pipe is not None:
                        n += pipe.finish()
                    pipe, key = pipeline_for(predictor, frames, time_batch, streams, submit, emit, frame_spec,
                                             frame_layout), k
                if center is not None:
                    pipe.push(frames, mask, center)
                else:
                    pipe.push(frames) if mask is None else pipe.push(frames, mask)
            if mask_iter is not None and next(mask_iter, _end) is not _end:
                raise ValueError("camera_mask yielded more masks than there are frame sets")
            if center_iter is not None and next(center_iter, _end) is not _end:
                raise ValueError("centers yielded more centres than there are frame sets")
            if pipe is not None:
                n += pipe.finish()
        except BaseException:
            # an aborted run leaves copies / uploads / forwards in flight on the cached staging buffers: wait for
            # them and drop the cache, so that a retry starts from fresh buffers
            from ._ingest import release_ingest_buffers
            release_ingest_buffers(predictor)
            raise
    return n


def _is_single_mask(camera_mask):
    """The drivers' camera_mask argument: ONE mask for the whole run when it is a 1-d tensor, a 1-d numpy array, or a
    list / tuple whose elements are all plain scalars (bool, int, float, numpy scalars; an empty one too: it then
    fails the shape check); anything else -- a list of masks / Nones, a 2-d tensor, a generator -- is an iterable of
    one mask per frame set."""
    import numpy as np
    if torch.is_tensor(camera_mask) or isinstance(camera_mask, np.ndarray):
        return camera_mask.ndim == 1
    if isinstance(camera_mask, (list, tuple)):
        return all(isinstance(v, (bool, int, float, np.generic)) for v in camera_mask)
    return False


def _center(value):
    """One frame set's centre checked: a (3,) host fp32 tensor (_native.centers; ValueError for another shape)."""
    return N.centers(value, 1)[0].cpu()


def _as_host(frames):
    """numpy view of a decoded frame set (numpy array or CPU tensor), C-contiguous."""
    import numpy as np
    a = frames.detach().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    return a if a.flags.c_contiguous else np.ascontiguousarray(a)
