"""The per-joint 3D spread a forward returns with return_spread=True (pure Python: no library, no torch)."""
from typing import NamedTuple


class Spread3D(NamedTuple):
    """Per-joint 3D spread of the normalised heat map softplus(V2V output) whose mean is the keypoint
    (jh_predictor_set_spread, include/jarvis_hip.h): cov (T,J,3,3) its covariance in mm^2 (axes as points3D[..., 0..2];
    fp64 sums, rounded once), peak (T,J,3) the voxel of the maximum in mm (the mode; the lowest index among equal
    maxima), mass (T,J) the sum of the weights (the normaliser).  NaN rows where a frame set is not
    valid."""
    cov: object
    peak: object
    mass: object
