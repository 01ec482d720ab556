"""numpy float32 reference of centre keyframes, written from the definition in include/jarvis_hip.h
(jh_predictor_set_center_keyframes): the key rows of a time batch and the fill of the rows in between.  No GPU, no
library: the tests compare the library with this."""
import numpy as np

DETECTED, INTERPOLATED, HELD, NONE = 0, 1, 2, -1


def key_slots(T, every):
    """K(T, every) = ceil((T - 1) / every) + 1, taken as 1 for T = 1: the key slots of a predictor."""
    return 1 if T == 1 else -(-(T - 1) // every) + 1


def key_rows(T, every, n_rows=None):
    """{0, every, 2 every, ... < n_rows} and n_rows - 1, ascending."""
    n_rows = T if n_rows is None else n_rows
    assert T >= 1 and every >= 1 and 1 <= n_rows <= T
    return sorted(set(range(0, n_rows, every)) | {n_rows - 1})


def fill(T, every, n_rows, key_centers, key_valid):
    """key_centers: {key row: (3,) float32 centre}, key_valid: {key row: bool} -> centers (T,3) float32, source (T)
    int32.  Every operation of the interpolation is one float32 operation, in the header's order."""
    keys = key_rows(T, every, n_rows)
    assert sorted(key_centers) == keys and sorted(key_valid) == keys
    nan = np.float32("nan")
    centers = np.full((T, 3), nan, np.float32)
    source = np.full((T,), NONE, np.int32)
    for t in range(n_rows):
        if t in keys:
            if key_valid[t]:
                centers[t], source[t] = np.asarray(key_centers[t], np.float32), DETECTED
            continue
        ta = max(k for k in keys if k < t)
        tb = min(k for k in keys if k > t)
        a, b = np.asarray(key_centers[ta], np.float32), np.asarray(key_centers[tb], np.float32)
        if key_valid[ta] and key_valid[tb]:
            w = np.float32(t - ta) / np.float32(tb - ta)
            d = (b - a).astype(np.float32)
            centers[t], source[t] = (a + (d * w).astype(np.float32)).astype(np.float32), INTERPOLATED
        elif key_valid[ta] or key_valid[tb]:
            centers[t], source[t] = (a if key_valid[ta] else b), HELD
    last = n_rows - 1
    for t in range(n_rows, T):                                  # padding rows hold the last real row
        if key_valid[last]:
            centers[t], source[t] = centers[last], HELD
    return centers, source
