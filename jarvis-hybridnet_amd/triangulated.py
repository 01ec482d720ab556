"""The per-joint triangulation a forward returns with return_triangulated=True (pure Python: no library, no torch)."""
from typing import NamedTuple


class Triangulated3D(NamedTuple):
    """A second 3D estimate per joint, triangulated from the cameras' own 2D keypoints with the cameras that disagree
    left out (jh_predictor_triangulate_joints, include/jarvis_hip.h) -- the one that does not pass through the voxel
    cube: points (T,J,3) world millimetres, the weighted DLT over the members' observations; views (T,J) int32 the
    number of members (0 for an empty joint); members (T,J,C) uint8, 1 for a camera whose keypoint lies within
    max_error_px of the projection of the consensus point; error (T,J) the mean distance in full-frame pixels between
    the members' observations and the projection of the point; observations (T,C,J,3) = (u, v, w) the full-frame pixel
    -- the arg-max of the heat map moved by the centroid of its (2 refine_radius + 1)^2 window -- and the weight
    (the 2D confidence) of every camera, (NaN, NaN, 0) for a camera that is not used.  An empty joint (fewer than
    min_views cameras agree) and every joint of a frame set that is not valid: NaN points and error, views 0."""
    points: object
    views: object
    members: object
    error: object
    observations: object
