"""GPU: per-frame-set calibration (jh_predictor_set_calibration_frames).  The claim: row t of a batch run with one
calibration per frame set equals, BIT FOR BIT, row t of the same batch -- same predictor, frames and mask row -- run with
calibration k(t) as the shared calibration (the existing, pinned code path, which is the reference here).

Calibration sets, all derived from the case's own set A (tests/cases.py, cfg2: 4 cameras 640 x 512, 48^3 grid):
  B  A in a world frame translated by d = (30, -20, 10) mm: row 3 of every (4,3) camera matrix becomes
     row3 - d @ rows[0:3].  Projections are unchanged, so a frame is valid exactly when it is under A; the integer
     centre moves.
  D  A with k1, k2 of every camera halved: the `dist` stride, and an intr / dist pair that differs from cam's.
Validity is decided in stage 1, which reads no calibration; the tests still assert valid == 1 on every row they compare
(nothing passes vacuously) and that the A, B and D rows of a batch are pairwise NOT equal.
Every test passes a per-frame calibration or calls the new entry point, so every one fails on a build without the
feature."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import cases
from tests.gpu_util import cuda

pytestmark = pytest.mark.gpu

TAG = "cfg2"
KEYS = ("cam", "intr", "dist")


def make_cfg(c):
    from jarvis_hybridnet_amd import synthetic as S
    return NS(PARENT_DIR="/nonexistent", PROJECT_NAME="none",
              DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
              CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center_size"]),
              KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
              HYBRIDNET=NS(NUM_CAMERAS=c["C"], ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))


def derived_sets(cam, intr, dist):
    """{"A", "B", "D"} -> (cam, intr, dist) CPU tensors, as the module docstring derives them."""
    d = torch.tensor([30.0, -20.0, 10.0])
    cam_b = cam.clone()
    cam_b[:, 3] = cam[:, 3] - torch.einsum("k,ckj->cj", d, cam[:, 0:3])
    dist_d = dist.clone()
    dist_d[:, 0, 0:2] *= 0.5
    return {"A": (cam, intr, dist), "B": (cam_b, intr.clone(), dist.clone()), "D": (cam.clone(), intr.clone(), dist_d)}


@functools.lru_cache(maxsize=None)
def setup():
    """The cfg2 predictor, its calibration sets on the device and 8 frame sets; shared, never changed.  The frame sets
    alternate between the two that tests/test_hip_views2d.py pins as valid, so rows "ABDABD.." meet every pairing of
    frame set and calibration."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES[TAG]
    inp = cases.predictor_inputs(TAG)
    calib = tuple(inp[k] for k in KEYS)
    sets = {k: tuple(cuda(t) for t in v) for k, v in derived_sets(*calib).items()}
    two = [inp["imgs"], S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"] + 100)[0]]
    frames = torch.stack([two[t % 2] for t in range(8)])
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    return c, inp, pred, sets, frames


def stacked(sets, rows):
    """Per-frame calibration of the rows named by `rows` ("ABD...") -> three (T,C,...) device tensors."""
    return tuple(torch.stack([sets[k][i] for k in rows]) for i in range(3))


def bits(t):
    """A tensor as integers: NaN rows (unused cameras of the 2D views) compare by their bits."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def run(pred, c, x, calib, call="forward_batch", **kw):
    """One batched forward and the predictor's debug tensors -> dict of clones (the predictor's buffers are reused)."""
    T = len(x)
    res = getattr(pred, call)(x, *calib, **kw)
    pr = pred.native(c["H"], c["W"], time_batch=T)
    out = dict(points=res[0], conf=res[1], valid=res[2])
    dbg = pr.debug("cuda")
    out.update(center3d=dbg["center3d"], center3d_int=dbg["center3d_int"], center_hm=dbg["center_hm"])
    if kw.get("return_2d"):
        out.update(res[3]._asdict())
    if kw.get("camera_mask") is not None:
        out.update(pr.debug_mask("cuda"))
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def check_rows(got, shared, rows, what=""):
    """Row t of `got` == row t of shared[rows[t]] in every tensor; all rows valid; A, B, D rows pairwise different."""
    assert got["valid"].tolist() == [1] * len(rows), what
    for k in set(rows):
        assert shared[k]["valid"].tolist() == [1] * len(rows), (what, k)
    for t, k in enumerate(rows):
        for name, v in got.items():
            assert same(v[t], shared[k][name][t]), (what, t, k, name)
        for other in set("ABD") - {k}:                 # ... and the row really is its own calibration's
            assert not torch.equal(got["points"][t], shared[other]["points"][t]), (what, t, k, other)
            assert not torch.equal(got["center3d"][t], shared[other]["center3d"][t]), (what, t, k, other)
    # the integer centre moves with the world frame (B), not with the distortion alone (D is within a voxel of A)
    for t, k in enumerate(rows):
        if k == "B":
            assert not torch.equal(got["center3d_int"][t], shared["A"]["center3d_int"][t]), (what, t)


@functools.lru_cache(maxsize=None)
def shared_runs(T, u8=False):
    """The batch of T frame sets under each of A, B, D as the SHARED calibration: the reference, computed once."""
    c, inp, pred, sets, frames = setup()
    x = cuda(to_u8(frames[:T]) if u8 else frames[:T])
    return x, {k: run(pred, c, x, sets[k]) for k in "ABD"}


def to_u8(imgs):
    return (imgs.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).contiguous()


@pytest.mark.parametrize("T,rows,u8", [(3, "ABD", False), (8, "ABDABDAB", False), (3, "ABD", True)])
def test_forward_batch_rows_equal_shared_runs(T, rows, u8):
    """Item 1: fp32 frames at T = 3 and T = 8 (the other time-batch class), uint8 BGR at T = 3."""
    c, inp, pred, sets, _ = setup()
    x, shared = shared_runs(T, u8)
    got = run(pred, c, x, stacked(sets, rows))
    check_rows(got, shared, rows, "T=%d u8=%d" % (T, u8))
    # back to the shared form on the same predictor: today's bits
    again = run(pred, c, x, sets["A"])
    for name, v in again.items():
        assert same(v, shared["A"][name]), name


def test_masks_and_2d_views_compose():
    """Item 2: one mask per row and return_2d -- the five Views2D tensors and the counts of the masked triangulation."""
    c, inp, pred, sets, frames = setup()
    rows = "ABD"
    x = cuda(frames[:3])
    mask = torch.tensor([[1, 1, 0, 1], [1, 1, 1, 1], [1, 1, 1, 0]], dtype=torch.uint8)
    shared = {k: run(pred, c, x, sets[k], camera_mask=mask, return_2d=True) for k in rows}
    got = run(pred, c, x, stacked(sets, rows), camera_mask=mask, return_2d=True)
    for name in ("points2D", "confidences2D", "reprojections", "errors", "used", "n_active", "num_cams_detect"):
        assert name in got
    check_rows(got, shared, rows, "masked")
    assert got["used"].tolist() == mask.tolist() and got["n_active"].tolist() == [3, 4, 3]
    # the reprojections of row t are made with row t's calibration: B's differ from D's on the same points' row
    assert not torch.equal(bits(got["reprojections"][1]), bits(shared["D"]["reprojections"][1]))
    # return_2d without a mask
    shared = {k: run(pred, c, x, sets[k], return_2d=True) for k in rows}
    got = run(pred, c, x, stacked(sets, rows), return_2d=True)
    check_rows(got, shared, rows, "views")


def test_forward_images_equals_forward_batch():
    """Item 3."""
    c, inp, pred, sets, frames = setup()
    rows = "BDA"
    x = cuda(frames[:3])
    calib = stacked(sets, rows)
    want = run(pred, c, x, calib)
    images = [[x[t, cam].clone() for cam in range(c["C"])] for t in range(3)]
    got = run(pred, c, images, calib, call="forward_images")
    assert got["valid"].tolist() == [1, 1, 1]
    for name, v in got.items():
        assert same(v, want[name]), name
    _, shared = shared_runs(3, False)
    check_rows(got, shared, rows, "images")


def native(T, **kw):
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, _, _, _ = setup()
    return NativePredictor(inp["sd_center"], inp["sd_hybrid"], num_cameras=c["C"], num_joints=c["J"],
                           center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
                           grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD, time_batch=T,
                           **kw)


def test_graph_replay_across_forms_and_values():
    """Item 4: graph replay on at T = 3.  Shared A, per-frame (A,B,D), per-frame (B,D,A) -- new values in the same form:
    the one recording keeps replaying --, shared B -- the form changes back: recorded again.  Each equals the plain
    launches (graph_replay = False) of the same call."""
    c, inp, pred, sets, frames = setup()
    x = cuda(frames[:3])
    g, e = native(3), native(3)
    g.graph_replay = True
    assert g.graph_replay and not e.graph_replay
    steps = [("shared", sets["A"]), ("frames", stacked(sets, "ABD")), ("frames", stacked(sets, "BDA")),
             ("shared", sets["B"])]
    results = []
    for form, calib in steps:
        outs = []
        for p in (g, e):
            (p.set_calibration_frames if form == "frames" else p.set_calibration)(*calib)
            outs.append([t.clone() for t in p.forward(x)])
        torch.cuda.synchronize()
        assert outs[0][2].tolist() == [1, 1, 1]
        for a, b in zip(*outs):
            assert torch.equal(a, b), form
        results.append(outs[0])
    # the steps are told apart by their results: (A,B,D) against (B,D,A) row 0, shared A against shared B
    assert not torch.equal(results[1][0][0], results[2][0][0]) and not torch.equal(results[0][0], results[3][0])
    assert torch.equal(results[1][0][0], results[0][0][0]) and torch.equal(results[2][0][0], results[3][0][0])


def test_staged_calls_read_rows_from_t0():
    """Item 5: stage_center, stage_keypoints, then stage_3d and views2d with time_batch_3d = 1 over t0 = 0, 1, 2 after
    set_calibration_frames equal the rows of the whole-path forward."""
    c, inp, pred, sets, frames = setup()
    rows = "ABD"
    T, C, J = 3, c["C"], c["J"]
    x = cuda(frames[:T])
    calib = stacked(sets, rows)
    want = run(pred, c, x, calib, return_2d=True)
    assert want["valid"].tolist() == [1, 1, 1]
    pr = native(T, time_batch_3d=1)
    pr.set_calibration_frames(*calib)
    det = torch.empty((T, C, 3), device="cuda")
    heat = torch.empty((T, C, pr.Hh, pr.Hh, pr.Jp), device="cuda")
    pr.stage_center(x, det)
    pr.stage_keypoints(x, det, heat)
    dbg = pr.debug("cuda")
    for name in ("center3d", "center3d_int", "center_hm"):
        assert torch.equal(dbg[name], want[name]), name
    for t0 in range(T):
        pts, conf = torch.empty((1, J, 3), device="cuda"), torch.empty((1, J), device="cuda")
        valid = torch.empty((1,), device="cuda", dtype=torch.int32)
        pr.stage_3d(heat[t0:t0 + 1], t0, pts, conf, valid)
        views = pr.views2d(pts, heat=heat[t0:t0 + 1], t0=t0)
        torch.cuda.synchronize()
        assert int(valid[0]) == 1
        assert torch.equal(pts[0], want["points"][t0]) and torch.equal(conf[0], want["conf"][t0]), t0
        for name, v in views._asdict().items():
            assert same(v[0], want[name][t0]), (t0, name)


def test_analyze_frames_time_batch_with_the_hip_predictor(tmp_path):
    """Item 6: six samples from two dataset names (A, B interleaved) at time_batch = 4 -- one full group and a padded
    tail -- write the three files of the time_batch = 1 run, byte for byte.  One sample is rejected by the network:
    frame set 2 of cases.analysis_gpu_samples, whose centre weights are scaled so that one camera alone passes the
    `> 50` gate (the construction of the cfg2_one case that test_masked_invalid_like_the_reference uses; this predictor
    needs its other frame sets valid under the SAME weights, which cases.ANALYSIS_GPU_VALID pins)."""
    from torch.utils.data import DataLoader
    from jarvis_hybridnet_amd.analysis.analyze import analyze_frames
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c, inp, samples, _ = cases.analysis_gpu_samples()
    samples = [list(s) for s in samples] + [list(samples[0])]
    valid = list(cases.ANALYSIS_GPU_VALID) + [cases.ANALYSIS_GPU_VALID[0]]
    for i, s in enumerate(samples):
        s[-2], s[-1] = ("ringA", "ringB")[i % 2], "Frame_%03d.jpg" % i
    two = derived_sets(*(inp[k] for k in KEYS))
    tools = {name: NS(cameraMatrices=two[k][0], intrinsicMatrices=two[k][1], distortionCoefficients=two[k][2])
             for name, k in (("ringA", "A"), ("ringB", "B"))}
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    files = {}
    for T in (1, 4):
        out = tmp_path / ("t%d" % T)
        seen, done = analyze_frames(pred, DataLoader(samples, batch_size=1, shuffle=False), tools, str(out), c["J"],
                                    time_batch=T)
        assert (seen, done) == (len(samples), sum(valid)) == (6, 5)
        files[T] = [open(out / f, "rb").read() for f in ("frame_names.csv", "points_HybridNet.csv",
                                                         "points_GroundTruth.csv")]
    assert files[4] == files[1]
    assert files[1][0].decode().split() == ["Frame_%03d.jpg" % i for i, v in enumerate(valid) if v]
    # samples 0 (ringA) and 5 (ringB) hold the same frames: the two calibrations give different rows
    net = np.loadtxt(tmp_path / "t4" / "points_HybridNet.csv", delimiter=",")
    assert net.shape == (5, c["J"] * 3) and not np.array_equal(net[0], net[4])


def test_device_bytes_and_null_pointers():
    """Item 7: nothing is allocated for a predictor that never uses the per-frame form (jh_predictor_device_bytes is the
    figure of creation until the first call, which is what allocates); a NULL pointer is refused with a message."""
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, sets, frames = setup()
    pr = native(3)
    lib = N.lib()
    created = pr.device_bytes
    assert created > 0 and lib.jh_predictor_device_bytes(pr.handle) == created
    pr.set_calibration(*sets["A"])
    x = cuda(frames[:3])
    before = [t.clone() for t in pr.forward(x)]
    assert lib.jh_predictor_device_bytes(pr.handle) == created
    cam, intr, dist = stacked(sets, "ABD")
    for args in ((None, N.ptr(intr), N.ptr(dist)), (N.ptr(cam), None, N.ptr(dist)), (N.ptr(cam), N.ptr(intr), None)):
        assert lib.jh_predictor_set_calibration_frames(pr.handle, *args, N.stream()) != 0
        assert b"null calibration pointer" in lib.jh_last_error()
    assert lib.jh_predictor_set_calibration_frames(None, N.ptr(cam), N.ptr(intr), N.ptr(dist), N.stream()) != 0
    assert b"null predictor" in lib.jh_last_error()
    # the refused calls changed nothing: still the shared form, still the same bits
    after = pr.forward(x)
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    # the Python handle refuses what is not (T,C,...)
    with pytest.raises(ValueError):
        pr.set_calibration_frames(*sets["A"])
    with pytest.raises(ValueError):
        pr.set_calibration_frames(cam[:2], intr[:2], dist[:2])
    with pytest.raises(ValueError):
        pred.forward_batch(x, cam, sets["A"][1], sets["A"][2])           # mixed forms
    pr.set_calibration_frames(cam, intr, dist)
    got = pr.forward(x)
    torch.cuda.synchronize()
    _, shared = shared_runs(3, False)
    for t, k in enumerate("ABD"):
        assert torch.equal(got[0][t], shared[k]["points"][t]), t
