"""CPU: several subjects per frame set (jh_op_center_peaks, jh_op_associate_subjects, jh_predictor_detect_subjects) --
the numpy reference of the two definitions (tests/subjects_ref.py) against hand-made cases, the parameter check, the
exported `Subjects`, and the new symbols in the header, the ctypes table and the built library.  Every test uses a name
this feature adds."""
import os
import re

import numpy as np
import pytest
import torch

from tests import subjects_ref as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("jh_op_center_peaks", "jh_op_associate_subjects", "jh_predictor_detect_subjects", "jh_subjects_params_check")
INF = float("inf")


def rows(peaks, n=0):
    return [tuple(float(v) for v in p) for p in peaks[n]]


# ---- the reference of the peak definition, on maps small enough to check by eye
def test_ref_plateau_keeps_lowest_index():
    h = np.zeros((1, 5, 5), np.float32)
    h[0, 1:3, 1:4] = 7.0                       # a 2 x 3 plateau: flat indices 6 7 8 11 12 13
    p, n = R.peaks_ref(h, 4, 1, 0.0)
    assert n.tolist() == [1] and rows(p)[0] == (1.0, 1.0, 7.0) and rows(p)[1] == R.EMPTY
    # a constant map above the threshold: index 0 suppresses its window, the others chain-suppress each other, so the
    # peaks are the pixels with no equal neighbour of a lower index -- only (0, 0)
    p, n = R.peaks_ref(np.full((1, 4, 6), 3.0, np.float32), 4, 1, 0.0)
    assert n.tolist() == [1] and rows(p)[0] == (0.0, 0.0, 3.0)
    # ... and at or below the threshold: none (the comparison is strict)
    assert R.peaks_ref(np.full((1, 4, 6), 3.0, np.float32), 2, 1, 3.0)[1].tolist() == [0]


def test_ref_edges_corners_and_order():
    h = np.zeros((1, 6, 6), np.float32)
    h[0, 0, 0], h[0, 0, 5], h[0, 5, 0], h[0, 5, 5] = 9, 8, 7, 6        # the four corners
    h[0, 0, 3], h[0, 3, 0] = 5, 5                                     # top and left edge, equal values
    p, n = R.peaks_ref(h, 8, 1, 1.0)
    # value descending, then index ascending: (x=3, y=0) is index 3, (x=0, y=3) is index 18
    assert n.tolist() == [6]
    assert rows(p)[:6] == [(0, 0, 9), (5, 0, 8), (0, 5, 7), (5, 5, 6), (3, 0, 5), (0, 3, 5)]
    assert rows(p)[6:] == [R.EMPTY] * 2
    # only the first max_peaks are kept; a wider window lets the corner 9 suppress the edge peaks within 3 pixels
    assert rows(R.peaks_ref(h, 2, 1, 1.0)[0]) == [(0, 0, 9), (5, 0, 8)]
    assert rows(R.peaks_ref(h, 8, 3, 1.0)[0])[:4] == [(0, 0, 9), (5, 0, 8), (0, 5, 7), (5, 5, 6)]
    assert R.peaks_ref(h, 8, 3, 1.0)[1].tolist() == [4]


def test_ref_nan_and_inf_pixels():
    h = np.zeros((1, 4, 4), np.float32)
    h[0, 1, 1], h[0, 1, 2] = np.nan, 4.0       # NaN beside a maximum: neither a peak nor a suppressor
    h[0, 3, 3] = -np.inf
    p, n = R.peaks_ref(h, 4, 1, -INF)
    # besides (2, 1): the zeros that have no greater and no earlier-equal neighbour -- only index 0
    assert n.tolist() == [2] and rows(p)[:2] == [(2, 1, 4), (0, 0, 0)]
    # -inf is never above min_peak = -inf, NaN never above anything
    h2 = np.full((1, 3, 3), -np.inf, np.float32)
    h2[0, 1, 1] = np.nan
    assert R.peaks_ref(h2, 2, 1, -INF)[1].tolist() == [0]
    # x = p % Hh and y = p // Wh, the arg-max kernel's expression, on a non-square map: p = 7 of a 2 x 5 map
    h3 = np.zeros((1, 2, 5), np.float32)
    h3[0, 1, 2] = 1.0
    assert rows(R.peaks_ref(h3, 1, 1, 0.5)[0]) == [(7 % 2, 7 // 5, 1.0)]


def test_ref_fewer_than_p_peaks_and_batch():
    h = np.zeros((2, 8, 8), np.float32)
    h[0, 2, 2], h[0, 6, 5] = 3.0, 2.0
    p, n = R.peaks_ref(h, 4, 2, 0.5)
    assert n.tolist() == [2, 0]
    assert rows(p, 0) == [(2, 2, 3), (5, 6, 2), R.EMPTY, R.EMPTY] and rows(p, 1) == [R.EMPTY] * 4


# ---- the reference of the association, on a scene whose answer is known by construction
def scene():
    from jarvis_hybridnet_amd import synthetic as S
    calib = S.ring_calibration(4, 640, 512, 900.0)
    pts = [(60.0, -40.0, 20.0), (-120.0, 90.0, -30.0)]
    # subject 1 hidden from camera 2; camera 1 holds a distractor with the highest value
    peaks = R.scene_peaks(calib, pts, (200.0, 150.0), 5.0, 4.0, 4, hidden={(2, 1)}, extra=[(1, 100, 20, 250.0)])
    return calib, pts, peaks


def test_ref_association_two_subjects():
    calib, pts, peaks = scene()
    tol = 3 * 5.0 / np.sqrt(2)
    args = [a.numpy() for a in calib]
    ctr, views, mem, err = R.associate_ref(peaks, *args, None, 5.0, 4.0, 3, tol, 2, margin=1e-2)
    assert views.tolist() == [4, 3, 0]
    # camera 1: the distractor is slot 0, the subjects slots 1 and 2; camera 2 sees subject 0 only
    assert mem.tolist() == [[0, 1, 0, 0], [1, 2, -1, 1], [-1, -1, -1, -1]]
    # grid rounding moves a peak by at most (2.5, 2) px: a few millimetres at this range
    assert np.abs(ctr[0] - pts[0]).max() < 6 and np.abs(ctr[1] - pts[1]).max() < 6 and np.isnan(ctr[2]).all()
    assert (err[:2] < 5.0 / np.sqrt(2)).all() and np.isnan(err[2])
    # three views are required: the second subject is still found, a pair-only one would not be
    assert R.associate_ref(peaks, *args, None, 5.0, 4.0, 3, tol, 3)[1].tolist() == [4, 3, 0]
    assert R.associate_ref(peaks, *args, None, 5.0, 4.0, 3, tol, 4)[1].tolist() == [4, 0, 0]
    # a masked camera takes no part, whatever its slots hold
    bad = peaks.copy()
    bad[3] = np.nan
    _, views, mem, _ = R.associate_ref(bad, *args, [1, 1, 1, 0], 5.0, 4.0, 2, tol, 2, margin=1e-2)
    assert views.tolist() == [3, 2] and mem.tolist() == [[0, 1, 0, -1], [1, 2, -1, -1]]


# ---- the Python surface that needs no device
def test_subjects_params_rejections():
    from jarvis_hybridnet_amd import _native as N
    p = N.subjects_params(2)
    assert (p.max_subjects, p.max_peaks, p.nms_radius, p.min_views) == (2, 4, 4, 2)
    assert (p.min_peak, p.max_error_px) == (50.0, 24.0)
    assert N.subjects_params(8).max_peaks == 8 and N.subjects_params(1, min_peak=-INF, max_error_px=INF).max_peaks == 2
    bad = [dict(max_subjects=0), dict(max_subjects=9), dict(max_subjects=2, max_peaks=0),
           dict(max_subjects=2, max_peaks=9), dict(max_subjects=1, nms_radius=0), dict(max_subjects=1, nms_radius=17),
           dict(max_subjects=1, min_views=1), dict(max_subjects=1, min_peak=float("nan")),
           dict(max_subjects=1, min_peak=INF), dict(max_subjects=1, max_error_px=-1.0),
           dict(max_subjects=1, max_error_px=float("nan")), dict(max_subjects=1.5), dict(max_subjects=True),
           dict(max_subjects=1, nms_radius="4"), dict(max_subjects=1, min_peak="high"), dict(max_subjects=2 ** 40)]
    for kw in bad:
        with pytest.raises(ValueError):
            N.subjects_params(**kw)
    with pytest.raises(TypeError):
        N.subjects_params(1, radius=3)


def test_subjects_exported_without_loading_the_library():
    import subprocess
    import sys
    code = ("import sys; import jarvis_hybridnet_amd as p; from jarvis_hybridnet_amd import _native as N; "
            "assert p.Subjects._fields == ('centers', 'views', 'members', 'error'); "
            "from jarvis_hybridnet_amd._predictor import Subjects; assert Subjects is p.Subjects; "
            "assert N._lib is None")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    assert callable(JarvisPredictor3D.detect_subjects) and callable(JarvisPredictor3D.forward_subjects)


def test_symbols_in_header_ctypes_table_and_library():
    from jarvis_hybridnet_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jarvis_hip.h")).read(), flags=re.S)
    assert re.search(r"typedef struct jh_subjects_params \{\s*int32_t max_subjects, max_peaks, nms_radius, min_views;"
                     r"\s*float min_peak, max_error_px;\s*\} jh_subjects_params;", text)
    lib = N.lib()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/jarvis_hip.h does not declare %s" % name
        res, args = N._SIGS[name]
        assert res is N.c_int and len(args) == len([p for p in m.group(1).split(",") if p.strip()]), name
        assert name in N.symbols() and hasattr(lib, name)
    # validation needs no GPU: nothing is enqueued for a null predictor or parameters out of range
    p = N.subjects_params(2)
    assert lib.jh_predictor_detect_subjects(None, None, None, 0, 0, None, None, None, p, None, None, None, None, None,
                                            None) != 0
    assert b"null predictor" in lib.jh_last_error()
    p.max_peaks = 9
    assert lib.jh_op_center_peaks(None, 1, 8, 8, 8, p, None, None, None) != 0 and b"max_peaks" in lib.jh_last_error()
    assert lib.jh_op_associate_subjects(None, 1, 4, None, None, None, 0, None, 5.0, 4.0, p, None, None, None, None,
                                        None) != 0 and b"max_peaks" in lib.jh_last_error()
