"""CPU: per-joint robust triangulation (jh_joints3d_params, jh_op_joint_peaks_refine, jh_op_triangulate_joints,
jh_predictor_triangulate_joints) -- the new symbols in the header, the ctypes table and the built library, the parameter
check, the CSV row and header, `Triangulated3D` and its place in the return value, and self-tests of the numpy reference
(tests/joints3d_ref.py) on scenes whose answer is known by construction.  Every test uses a name this feature adds.

The scenes' seeds are fixed: they were chosen, on the CPU, so that the reference's margin assertions (no support
distance within 1e-2 px of max_error_px, no choice resting on a cost difference below 1e-2 px, over every candidate
pair) hold on every one of them; about 3 % of random joints trip "a support distance on the bound" by chance."""
import csv
import io
import os
import re

import numpy as np
import pytest
import torch

from tests import joints3d_ref as JR

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("jh_joints3d_params_check", "jh_op_joint_peaks_refine", "jh_op_triangulate_joints",
       "jh_predictor_triangulate_joints")
INF = float("inf")


def kw(**params):
    """The reference's keywords for parameters that went through the library's own check (jh_joints3d_params_check, by
    _native.joints3d_params): the reference and the kernels are given the same, checked, numbers."""
    from jarvis_hybridnet_amd import _native as N
    p = N.joints3d_params(**params)
    assert N.lib().jh_joints3d_params_check(p) == 0
    return dict(min_views=p.min_views, min_conf=p.min_conf, max_error_px=p.max_error_px)


# rig of C cameras -> seeds of its self-test scenes (one outlier camera for C >= 4)
SCENE_SEEDS = {3: (300, 301, 302, 303), 4: (400, 401, 402, 403), 6: (600, 601, 602, 603), 12: (1200, 1201, 1202, 1203)}


def test_symbols_in_header_ctypes_table_and_library():
    from jarvis_hybridnet_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jarvis_hip.h")).read(), flags=re.S)
    assert re.search(r"typedef struct jh_joints3d_params \{\s*int32_t min_views, refine_radius;"
                     r"\s*float min_conf, max_error_px;\s*\} jh_joints3d_params;", text)
    assert re.search(r"#define JH_ABI_VERSION\s+4\b", text)
    lib = N.lib()
    assert lib.jh_abi_version() == N.ABI_VERSION == 4
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/jarvis_hip.h does not declare %s" % name
        res, args = N._SIGS[name]
        assert res is N.c_int and len(args) == len([p for p in m.group(1).split(",") if p.strip()]), name
        assert name in N.symbols() and hasattr(lib, name)
    # validation needs no GPU: nothing is enqueued for a null predictor or parameters out of range
    p = N.joints3d_params()
    assert lib.jh_predictor_triangulate_joints(None, None, 0, None, p, None, None, None, None, None, None) != 0
    assert b"null predictor" in lib.jh_last_error()
    p.refine_radius = 4
    assert lib.jh_op_triangulate_joints(None, 1, 4, 1, None, None, None, 0, p, None, None, None, None, None) != 0
    assert b"refine_radius" in lib.jh_last_error()
    assert lib.jh_op_joint_peaks_refine(None, 1, 8, 8, 8, None, 1, 4, None, None) != 0


def test_params_check_accepts_the_defaults_and_rejects_each_field():
    from jarvis_hybridnet_amd import _native as N
    p = N.joints3d_params()
    assert (p.min_views, p.refine_radius) == (2, 1) and p.max_error_px == 8.0
    assert p.min_conf == np.float32(0.1)
    assert N.lib().jh_joints3d_params_check(p) == 0
    assert N.lib().jh_joints3d_params_check(None) != 0
    ok = [dict(refine_radius=0), dict(refine_radius=3), dict(min_conf=0.0), dict(min_conf=1.0), dict(max_error_px=0.0),
          dict(max_error_px=INF), dict(min_views=64)]
    for kw in ok:
        N.joints3d_params(**kw)
    bad = [dict(min_views=1), dict(min_views=0), dict(refine_radius=-1), dict(refine_radius=4), dict(min_conf=-0.1),
           dict(min_conf=1.5), dict(min_conf=float("nan")), dict(max_error_px=-1.0), dict(max_error_px=float("nan")),
           dict(min_views=2.0), dict(refine_radius=True), dict(min_conf="high"), dict(min_views=2 ** 40)]
    for kw in bad:
        with pytest.raises(ValueError):
            N.joints3d_params(**kw)
    # the library's own check says the same of the raw struct, field by field
    for field, value in (("min_views", 1), ("refine_radius", -1), ("refine_radius", 4), ("min_conf", -0.1),
                         ("min_conf", 1.5), ("min_conf", float("nan")), ("max_error_px", -1.0),
                         ("max_error_px", float("nan"))):
        q = N.joints3d_params()
        setattr(q, field, value)
        assert N.lib().jh_joints3d_params_check(q) != 0, (field, value)
        assert b"jh_joints3d_params" in N.lib().jh_last_error() and field.encode() in N.lib().jh_last_error()
    with pytest.raises(TypeError):
        N.joints3d_params(radius=1)
    # what return_triangulated= accepts
    assert N.triangulation_params(False) is None and N.triangulation_params(None) is None
    assert N.triangulation_params(True).refine_radius == 1
    assert N.triangulation_params(dict(refine_radius=0, max_error_px=INF)).max_error_px == INF
    q = N.joints3d_params(refine_radius=2)
    assert N.triangulation_params(q) is q
    q.min_views = 1
    for value in (q, 1, "yes"):
        with pytest.raises(ValueError):
            N.triangulation_params(value)


def test_csv_row_and_header():
    from types import SimpleNamespace as NS
    from jarvis_hybridnet_amd.prediction import predict3D as P
    pts = torch.tensor([[1.5, -2.25, 3.0], [float("nan")] * 3])
    row = P.triangulated_row(pts, torch.tensor([3, 0], dtype=torch.int32), torch.tensor([0.5, float("nan")]), 2)
    assert row == [1.5, -2.25, 3.0, 3, 0.5, "NaN", "NaN", "NaN", 0, "NaN"]
    assert all(isinstance(v, np.float32) for v in row[:3] + row[4:5]) and isinstance(row[3], int)
    assert P.triangulated_row(None, None, None, 2) == ["NaN"] * 10
    buf = io.StringIO()
    w = csv.writer(buf)
    P.create_header_triangulated(w, NS(KEYPOINT_NAMES=["nose", "tail"]))
    w.writerow(row)
    lines = buf.getvalue().splitlines()
    assert lines[0] == "nose,nose,nose,nose,nose,tail,tail,tail,tail,tail"
    assert lines[1] == "x,y,z,views,error,x,y,z,views,error"
    assert lines[2] == "1.5,-2.25,3.0,3,0.5,NaN,NaN,NaN,0,NaN"
    assert P.TRIANGULATED_COLUMNS == ("x", "y", "z", "views", "error")


def test_triangulated3d_exported_and_last_in_the_return_value():
    import inspect
    import subprocess
    import sys
    code = ("import jarvis_hybridnet_amd as p; from jarvis_hybridnet_amd import _native as N; "
            "assert p.Triangulated3D._fields == ('points', 'views', 'members', 'error', 'observations'); "
            "from jarvis_hybridnet_amd._predictor import Triangulated3D; assert Triangulated3D is p.Triangulated3D; "
            "assert N._lib is None")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    from jarvis_hybridnet_amd._predictor import MultiStreamPredictor, NativePredictor
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    for name in ("forward", "forward_uint8", "forward_yuv", "forward_surface", "forward_batch", "forward_images",
                 "forward_subjects"):
        sig = inspect.signature(getattr(JarvisPredictor3D, name)).parameters
        assert sig["return_triangulated"].default is False and "return_2d" in sig, name
    assert inspect.signature(MultiStreamPredictor.forward).parameters["return_triangulated"].default is False
    assert inspect.signature(predict3D_frames).parameters["output_triangulated"].default is False
    assert list(inspect.signature(NativePredictor.triangulate_joints).parameters) == ["self", "heat", "t0",
                                                                                      "camera_mask", "params"]

    # the place in the return value, with a predictor that records what it is asked for
    class Fake:
        T3, C, J = 1, 4, 2

        def views2d(self, points, camera_mask=None):
            return "views"

        def triangulate_joints(self, camera_mask=None, params=None):
            return ("tri", params.refine_radius)
    from jarvis_hybridnet_amd import _native as N
    res = ("points", "conf", torch.ones(1, dtype=torch.int32), "spread")
    tri = N.joints3d_params(refine_radius=2)
    assert JarvisPredictor3D._batch(Fake(), res, None, True, tri) == res[:3] + ("views", "spread", ("tri", 2))
    assert JarvisPredictor3D._batch(Fake(), res[:3], None, False, tri) == res[:3] + (("tri", 2),)
    assert JarvisPredictor3D._batch(Fake(), res[:3], None, False) == res[:3]
    assert JarvisPredictor3D._single(Fake(), res, None, True, tri) == ("points", "conf", "views", "spread", ("tri", 2))
    invalid = ("points", "conf", torch.zeros(1, dtype=torch.int32))
    assert JarvisPredictor3D._single(Fake(), invalid, None, True, tri) == (None,) * 4


# ---- the reference, on scenes whose answer is known
@pytest.mark.parametrize("C", sorted(SCENE_SEEDS))
def test_ref_leaves_the_outlier_camera_out(C):
    calib = JR.rig(C)
    for seed in SCENE_SEEDS[C]:
        obs, X, out = JR.joint_scene(calib, np.random.RandomState(seed), "outlier" if C >= 4 else "clean")
        pt, views, mem, err = JR.joint_ref(obs, *calib, **kw(max_error_px=6.0))
        if C >= 4:
            assert len(out) == 1 and mem[out[0]] == 0 and views == C - 1, (seed, out, mem)
        else:
            assert out == [] and views == 3 and mem.tolist() == [1, 1, 1], (seed, mem)
        assert mem.sum() == views and err < 2.0, (seed, err)
        # the +-1 px of the grid is a millimetre or two at this range; the outlier's 50 px would be 80
        assert np.abs(pt - X).max() < 4.0, (seed, pt, X)
        # the point is the weighted DLT over the members
        want = JR.R.dlt64([(c, obs[c, 0], obs[c, 1], obs[c, 2]) for c in range(C) if mem[c]], *calib)
        assert np.abs(pt - want).max() < 1e-6
        # without the bound every camera in front of which the point lies is a member
        _, views_inf, mem_inf, _ = JR.joint_ref(obs, *calib, margin=None, **kw(min_conf=0.0, max_error_px=INF))
        assert views_inf == C and mem_inf.all()


def test_ref_kinds_and_the_camera_behind_the_point():
    calib = JR.rig(4)
    g = np.random.RandomState(4100)
    obs, X, out = JR.joint_scene(calib, g, "low_conf")
    _, views, mem, _ = JR.joint_ref(obs, *calib, **kw(max_error_px=6.0))
    assert views == 3 and mem[out[0]] == 0
    assert JR.joint_ref(obs, *calib, **kw(min_conf=0.0, max_error_px=6.0))[1] == 3      # (its pixel is 35 px off as well)
    obs, X, out = JR.joint_scene(calib, g, "unused")
    _, views, mem, _ = JR.joint_ref(obs, *calib, **kw(max_error_px=6.0))
    assert views == 3 and mem[out[0]] == 0 and np.isnan(obs[out[0], 0])
    obs, X, out = JR.joint_scene(calib, g, "too_few")
    pt, views, mem, err = JR.joint_ref(obs, *calib, **kw(max_error_px=6.0))
    assert views == 0 and not mem.any() and np.isnan(pt).all() and np.isnan(err)
    # three views required of a joint two cameras agree on: empty
    obs, X, out = JR.joint_scene(JR.rig(3), g, "unused")
    assert JR.joint_ref(obs, *JR.rig(3), **kw(max_error_px=6.0))[1] == 2
    assert JR.joint_ref(obs, *JR.rig(3), **kw(min_views=3, max_error_px=6.0))[1] == 0
    # a camera whose matrix is negated sees the same pixels from behind: never a member, with or without the bound
    obs, X, _ = JR.joint_scene(calib, g, "clean")
    back = JR.flipped(calib, 2)
    for params, margin in ((dict(max_error_px=6.0), JR.MARGIN), (dict(max_error_px=INF, min_conf=0.0), None)):
        _, views, mem, _ = JR.joint_ref(obs, *back, margin=margin, **kw(**params))
        assert views == 3 and mem.tolist() == [1, 1, 0, 1]


def test_ref_refined_peak_finds_the_subpixel_centre():
    from jarvis_hybridnet_amd import _native as N
    # the radii the library takes: 1 .. 3 refine, 0 does not, 4 is refused
    RADII = [r for r in range(1, 8) if N.lib().jh_joints3d_params_check(N.Joints3dParamsStruct(2, r, 0.1, 8.0)) == 0]
    assert RADII == [1, 2, 3] and N.joints3d_params(refine_radius=0).refine_radius == 0
    g = np.random.RandomState(7)
    worst_int, worst_ref = 0.0, 0.0
    for _ in range(40):
        cx, cy = g.uniform(4.0, 19.0, 2)
        img = JR.blob(24, 24, cx, cy)
        m = int(np.argmax(img))
        mx, my = m % 24, m // 24
        for r in RADII:
            ox, oy = JR.offset_ref(img, mx, my, r)
            worst_ref = max(worst_ref, abs(mx + float(ox) - cx), abs(my + float(oy) - cy))
            assert abs(float(ox)) <= r and abs(float(oy)) <= r
        worst_int = max(worst_int, abs(mx - cx), abs(my - cy))
    assert worst_ref < 0.1 and 0.4 < worst_int <= 0.5, (worst_ref, worst_int)
    # the emulation's corner cases: the window is clipped at the edge, NaN and negative pixels count as 0, a
    # non-positive window has no centroid
    img = np.zeros((8, 8), np.float32)
    img[0, 0], img[0, 1], img[1, 0] = 4.0, 2.0, 2.0
    assert JR.offset_ref(img, 0, 0, 1) == (np.float32(0.25), np.float32(0.25))
    img[1, 1], img[0, 1] = np.nan, -3.0
    assert JR.offset_ref(img, 0, 0, 1) == (np.float32(0.0), np.float32(2.0) / np.float32(6.0))
    assert JR.offset_ref(np.full((8, 8), -1.0, np.float32), 3, 3, 2) == (0.0, 0.0)
    assert JR.offset_ref(np.zeros((8, 8), np.float32), 7, 7, 3) == (0.0, 0.0)
    idx = np.array([[0, 99]], np.int32)
    heat = np.stack([img, img], -1)[None]
    assert JR.refine_ref(heat, idx, 1)[0].tolist() == [[0.0, float(np.float32(2.0) / np.float32(6.0))], [0.0, 0.0]]
    # u = (float)x2d + 2 * ox
    obs = JR.observations_ref(np.array([[300, 200]]), np.array([0.5], np.float32), np.array([[0.25, -0.125]], np.float32))
    assert obs.tolist() == [[300.5, 199.75, 0.5]]
