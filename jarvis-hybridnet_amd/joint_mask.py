"""The per-joint camera sets a forward returns with joint_mask= (pure Python: no library, no torch)."""
from typing import NamedTuple


class JointMask(NamedTuple):
    """The cameras every joint's voxel volume was averaged over (jh_predictor_get_joint_mask, include/jarvis_hip.h):
    cameras (T,J,C) uint8, 1 where camera c counted for joint j of frame set t -- the joint mask of the call and its
    camera mask combined, with the fallback applied: a joint whose set would be empty has the cameras of the plain
    (or camera-masked) forward --; count (T,J) int32 their number, the divisor of the joint's mean (0: no camera at
    all).  An invalid frame set has no consensus members, so under joint_mask='consensus' its rows are the fallback."""
    cameras: object
    count: object


def create_header_joint_cameras(keypoint_names):
    """The two header rows of joint_cameras.csv, in the style of the reference's data3D.csv header: the joint's name
    over each of its columns, then the columns' names."""
    names = [name for name in keypoint_names for _ in range(2)]
    return [names, ["count", "cameras"] * len(keypoint_names)]


def joint_cameras_row(cameras, count, valid=True):
    """One frame set's row of joint_cameras.csv from cameras (J,C) and count (J) (host sequences): per joint its count
    and the decimal sum of 2^c over its cameras; 'NaN' x 2J for a frame set that is not valid."""
    if not valid:
        return ["NaN"] * (2 * len(count))
    row = []
    for cams, n in zip(cameras, count):
        row += [int(n), sum(1 << c for c, on in enumerate(cams) if int(on))]
    return row
