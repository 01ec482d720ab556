"""GPU: caller-supplied 3D centres (jh_predictor_set_centers): the 3D path without CenterDetect.

The main claim: a centred batch whose centres are the float centres of a detected run (jh_predictor_debug's center3d of
the same frames, calibration and mask) is that run BIT FOR BIT -- points, confidences, valid, the integer centre, the
crop centres and the five Views2D tensors.  Beside it: the reference's own centre (the fixture's, up to 3.3e-3 mm from
the HIP eigen-solve's) gives the reference's keypoints within the project's 1e-3 mm; centres the detector would not have
chosen give the oracle's integer path exactly and the keypoints of the pinned jh_predictor_hybridnet_forward on crops cut
on the CPU; invalid rows; composition with masks, per-frame-set calibration, per-image frames, YUV and sensor frames;
graph replay; the staged form; the driver.

All on cfg2 (tests/cases.py: 4 cameras 640 x 512, small / small, 48^3 grid).  Test centres (world mm), K0 the fixture's
cfg2.center3d; checked with oracle.reproject_point in fp32 (fp64 differs by <= 6e-5 px), every projection >= 0.027 px
and every coordinate >= 0.0118 mm from an integer -- the tests recompute the integers with the oracle and assert margins
>= 1e-2 before they compare, so nothing rests on a truncation tie:
  K1 = K0 + (7.3, -4.6, 2.2)        int (110, 70, -20)   center_hm [[365,269],[250,255],[280,267],[382,255]]
  K2 = K0 + (-12.4, 9.7, -6.3)      int (90, 84, -29)    center_hm [[373,274],[262,257],[272,272],[371,257]]
  K5 = K0 + (-130.2, -95.4, 40.6)   int (-27, -20, 17)   center_hm [[307,245],[336,249],[332,245],[303,249]]  (negative
                                    coordinates: truncation toward zero)
  K3 = K0 + (400, 0, 0)             int (502, 74, -22)   center_hm [[387,276],[128,255],[286,266],[512,255]]  (clamps
                                    active on two cameras: x = 128 and x = 512)
Every test passes `centers=` or calls set_centers, so every one fails on a build without the feature."""
import csv
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import cases
from tests.gpu_util import cuda, max_err, report

pytestmark = pytest.mark.gpu

TAG = "cfg2"
KEYS = ("cam", "intr", "dist")
OFFSETS = {"K1": (7.3, -4.6, 2.2), "K2": (-12.4, 9.7, -6.3), "K5": (-130.2, -95.4, 40.6), "K3": (400.0, 0.0, 0.0)}
TABLE = {"K1": ((110, 70, -20), [[365, 269], [250, 255], [280, 267], [382, 255]]),
         "K2": ((90, 84, -29), [[373, 274], [262, 257], [272, 272], [371, 257]]),
         "K5": ((-27, -20, 17), [[307, 245], [336, 249], [332, 245], [303, 249]]),
         "K3": ((502, 74, -22), [[387, 276], [128, 255], [286, 266], [512, 255]])}
NAMES = ("points", "conf", "valid", "center3d_int", "center_hm")
VIEWS = ("points2D", "confidences2D", "reprojections", "errors", "used")


def make_cfg(c):
    from jarvis_hybridnet_amd import synthetic as S
    return NS(PARENT_DIR="/nonexistent", PROJECT_NAME="none",
              DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
              CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center_size"]),
              KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
              HYBRIDNET=NS(NUM_CAMERAS=c["C"], ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))


def derived_sets(cam, intr, dist):
    """The calibration sets of tests/test_hip_calibration_frames.py: A the case's own; B the world frame translated by
    (30, -20, 10) mm (same projections, another integer centre); D with k1, k2 halved."""
    d = torch.tensor([30.0, -20.0, 10.0])
    cam_b = cam.clone()
    cam_b[:, 3] = cam[:, 3] - torch.einsum("k,ckj->cj", d, cam[:, 0:3])
    dist_d = dist.clone()
    dist_d[:, 0, 0:2] *= 0.5
    return {"A": (cam, intr, dist), "B": (cam_b, intr.clone(), dist.clone()), "D": (cam.clone(), intr.clone(), dist_d)}


@functools.lru_cache(maxsize=None)
def setup():
    """The cfg2 predictor (one native predictor per time batch behind it), its calibration on the device and 8 frame
    sets alternating between the two that tests/test_hip_views2d.py pins as valid; shared, never changed."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES[TAG]
    inp = cases.predictor_inputs(TAG)
    calib = tuple(inp[k] for k in KEYS)
    two = [inp["imgs"], S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"] + 100)[0]]
    frames = torch.stack([two[t % 2] for t in range(8)])
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    return c, inp, pred, tuple(cuda(t) for t in calib), frames


@functools.lru_cache(maxsize=None)
def centres():
    """K0 and the table's centres as fp32 CPU tensors, with the oracle's integer path for each -> {name: (K, int3,
    center_hm)}; margins asserted here, once."""
    from oracle import hybridnet_oracle as O
    c, inp, _, _, _ = setup()
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predictor.npz")))
    K0 = torch.from_numpy(g[TAG + ".center3d"]).float().reshape(3)
    hw = c["bbox"] // 2
    out = {}
    for name, off in dict(K0=(0.0, 0.0, 0.0), **OFFSETS).items():
        K = K0 + torch.tensor(off, dtype=torch.float32)
        uv = O.reproject_point(K[None], inp["cam"], inp["intr"], inp["dist"])
        assert float((uv - uv.round()).abs().min()) >= 1e-2 and float((K - K.round()).abs().min()) >= 1e-2, name
        chm = uv.int()
        chm[:, 0] = chm[:, 0].clamp(hw, c["W"] - hw)
        chm[:, 1] = chm[:, 1].clamp(hw, c["H"] - hw)
        out[name] = (K, K.int(), chm)
    for name, (i3, chm) in TABLE.items():
        assert out[name][1].tolist() == list(i3) and out[name][2].tolist() == chm, name
    assert out["K0"][2].tolist() == g[TAG + ".center_hm"].tolist()
    return out, g


def bits(t):
    """A tensor as integers: NaN rows (unused cameras of the 2D views) compare by their bits."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def to_u8(imgs):
    return (imgs.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).contiguous()


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


@functools.lru_cache(maxsize=None)
def detected(T, u8=False):
    """The first T frame sets run DETECTED: the reference of the bit comparisons, computed once."""
    c, inp, pred, calib, frames = setup()
    x = cuda(to_u8(frames[:T]) if u8 else frames[:T])
    return x, run(pred, c, x, calib)


@functools.lru_cache(maxsize=None)
def centred_single(name):
    """cfg2's frame at T = 1 from the table's centre `name`."""
    c, inp, pred, calib, frames = setup()
    return run(pred, c, cuda(frames[:1]), calib, centers=centres()[0][name][0][None])


def native(T, center=True, **kw):
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, _, calib, _ = setup()
    pr = NativePredictor(inp["sd_center"] if center else None, inp["sd_hybrid"], num_cameras=c["C"],
                         num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
                         grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD, time_batch=T,
                         **kw)
    pr.set_calibration(*calib)
    return pr


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,graph,u8", [(1, True, False), (1, False, False), (3, None, False), (8, None, False),
                                        (3, None, True)])
def test_equals_detection_bit_for_bit(T, graph, u8):
    c, inp, pred, calib, _ = setup()
    x, det = detected(T, u8)
    assert det["valid"].tolist() == [1] * T
    pr = pred.native(c["H"], c["W"], time_batch=T)
    if graph is not None:
        assert pr.graph_replay                              # the default at T = 1
        pr.graph_replay = graph
    try:
        for centers in (det["center3d"].cpu(), det["center3d"].clone()):      # a host tensor, a device tensor
            got = run(pred, c, x, calib, centers=centers)
            assert got["valid"].tolist() == [1] * T
            assert same(got["center3d"], det["center3d"])
            for name in NAMES:
                assert same(got[name], det[name]), (name, centers.device)
        again = run(pred, c, x, calib)                      # ... and back: today's bits
        for name in NAMES + ("center3d",):
            assert same(again[name], det[name]), name
    finally:
        if graph is not None:
            pr.graph_replay = True


# ---- 2 -------------------------------------------------------------------------------------------------------------
def test_reference_centre_gives_the_reference_result():
    c, inp, pred, calib, frames = setup()
    table, g = centres()
    K0 = table["K0"][0]
    pts, conf = pred(cuda(inp["imgs"]), *calib, centers=K0)
    dbg = pred.native(c["H"], c["W"]).debug("cuda")
    torch.cuda.synchronize()
    assert pts is not None
    assert torch.equal(dbg["center3d"][0].cpu(), K0)
    assert torch.equal(dbg["center_hm"][0].cpu(), torch.from_numpy(g[TAG + ".center_hm"]))
    assert torch.equal(dbg["center3d_int"][0].cpu(), torch.from_numpy(g[TAG + ".center3d"]).int().reshape(3))
    ep = max_err(pts, torch.from_numpy(g[TAG + ".points3D"]))
    ec = max_err(conf, torch.from_numpy(g[TAG + ".confidences"]))
    # (the HIP path's own detected centre, for the record: not the fixture's)
    e3 = max_err(detected(1)[1]["center3d"][0], K0)
    report("centers_vs_fixture", tag=TAG, points_mm=ep, conf=ec, detected_center_vs_fixture_mm=e3)
    print("centred with the fixture's centre: points %.3g mm, conf %.3g; HIP detected centre %.3g mm off" % (ep, ec, e3))
    assert ep < 1e-3, "3D keypoints must be within 1e-3 mm of the reference"
    assert ec < 1e-4


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_centres_the_detector_would_not_have_chosen():
    from jarvis_hybridnet_amd import synthetic as S
    c, inp, pred, calib, frames = setup()
    table, _ = centres()
    order = ("K1", "K2", "K5", "K3")
    x = cuda(torch.stack([inp["imgs"]] * 4))
    got = run(pred, c, x, calib, centers=torch.stack([table[k][0] for k in order]))
    assert got["valid"].tolist() == [1, 1, 1, 1]
    for t, k in enumerate(order):
        assert got["center3d_int"][t].cpu().tolist() == table[k][1].tolist(), k
        assert got["center_hm"][t].cpu().tolist() == table[k][2].tolist(), k
    assert bool(torch.isfinite(got["points"]).all()) and bool(torch.isfinite(got["conf"]).all())
    # K1, K2: the pinned entry point on crops cut and normalised on the CPU at those integers
    ref = native(1, center=False)
    hw = c["bbox"] // 2
    mean, std = torch.tensor(S.MEAN).view(3, 1, 1), torch.tensor(S.STD).view(3, 1, 1)
    for t, k in enumerate(order[:2]):
        _, i3, chm = table[k]
        crops = torch.stack([inp["imgs"][i, :, int(chm[i, 1]) - hw:int(chm[i, 1]) + hw,
                                         int(chm[i, 0]) - hw:int(chm[i, 0]) + hw] for i in range(c["C"])])
        crops = ((crops - mean) / std)[None].contiguous()
        _, _, rp, rc = ref.hybridnet_forward(cuda(crops), cuda(chm[None].int()), cuda(i3[None].int()),
                                             want_final=False, want_padded=False)
        torch.cuda.synchronize()
        e = max_err(got["points"][t], rp[0])
        report("centers_vs_hybridnet_forward", centre=k, points_mm=e, conf=max_err(got["conf"][t], rc[0]))
        print("%s: %.3g mm from hybridnet_forward on CPU-cut crops" % (k, e))
        assert e < 1e-3, k


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_stage_1_does_not_run():
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, frames = setup()
    x, det = detected(1)
    pr = native(1)
    K = det["center3d"].clone()
    prof_c = N.profile(lambda: pr.forward(x, centers=K))
    prof_d = N.profile(lambda: pr.forward(x))
    torch.cuda.synchronize()
    names_c, names_d = [r[0] for r in prof_c], [r[0] for r in prof_d]
    assert names_c.count("centers") == 1 and "centers" not in names_d
    for n in names_c:
        assert n != "center_argmax" and not n.startswith("triangulate") and n != "preprocess_resize", n
    assert "center_argmax" in names_d and "triangulate" in names_d
    assert len(names_c) < len(names_d)
    # a predictor without CenterDetect weights: centred forwards run, detected ones still refuse
    bare = native(1, center=False)
    got = [t.clone() for t in bare.forward(x, centers=K)]
    dbg = bare.debug("cuda")
    torch.cuda.synchronize()
    assert int(got[2][0]) == 1
    for a, name in zip(got, ("points", "conf", "valid")):
        assert same(a, det[name]), name
    assert same(dbg["center3d_int"], det["center3d_int"]) and same(dbg["center_hm"], det["center_hm"])
    with pytest.raises(RuntimeError, match="without CenterDetect weights"):
        bare.forward(x)
    assert bare.device_bytes < pr.device_bytes


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_invalid_rows():
    c, inp, pred, calib, frames = setup()
    table, _ = centres()
    x = cuda(torch.stack([inp["imgs"]] * 4))
    before = run(pred, c, x, calib)
    K1 = table["K1"][0]
    rows = torch.stack([K1, torch.tensor([float("nan"), 0.0, 0.0]), torch.tensor([0.0, float("inf"), 0.0]),
                        torch.tensor([3e7, 0.0, 0.0])])
    got = run(pred, c, x, calib, centers=rows)
    assert got["valid"].tolist() == [1, 0, 0, 0]
    one = centred_single("K1")
    for name in NAMES:
        assert same(got[name][0], one[name][0]), name
    hw = c["bbox"] // 2
    chm = got["center_hm"][1:].cpu()
    assert int(chm[..., 0].min()) >= hw and int(chm[..., 0].max()) <= c["W"] - hw
    assert int(chm[..., 1].min()) >= hw and int(chm[..., 1].max()) <= c["H"] - hw
    assert got["center3d_int"][1:].cpu().tolist() == [[0, 0, 0]] * 3
    # the float centre is reported as it was supplied
    assert same(got["center3d"].cpu(), rows)
    after = run(pred, c, x, calib)
    assert after["valid"].tolist() == [1, 1, 1, 1]
    for name in NAMES + ("center3d",):
        assert same(after[name], before[name]), name
    # the single-frame form
    assert pred(cuda(inp["imgs"]), *calib, centers=[float("nan"), 0.0, 0.0]) == (None, None)
    assert pred(cuda(inp["imgs"]), *calib, centers=K1, return_2d=True)[0] is not None
    assert pred(cuda(inp["imgs"]), *calib, centers=[0.0, float("-inf"), 0.0], return_2d=True) == (None, None, None)


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_composes_with_camera_masks_and_2d_views():
    c, inp, pred, calib, frames = setup()
    table, _ = centres()
    x = cuda(frames[:4])
    mask = torch.tensor([[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 0], [0, 0, 0, 0]], dtype=torch.uint8)
    det = run(pred, c, x, calib, camera_mask=mask, return_2d=True)
    assert det["valid"].tolist() == [1, 1, 0, 0]
    centers = torch.stack([det["center3d"][t].cpu() if det["valid"][t] else table["K1"][0] for t in range(4)])
    got = run(pred, c, x, calib, camera_mask=mask, return_2d=True, centers=centers)
    assert got["valid"].tolist() == [1, 1, 1, 0]            # one camera is enough here; none is not
    assert got["n_active"].tolist() == [4, 3, 1, 0] == det["n_active"].tolist()
    assert got["num_cams_detect"].tolist() == [0, 0, 0, 0]
    for t in (0, 1):
        for name in NAMES + VIEWS:
            assert same(got[name][t], det[name][t]), (t, name)
    assert got["used"].tolist() == [[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert got["center3d_int"][2].cpu().tolist() == table["K1"][1].tolist()


def test_composes_with_per_frame_set_calibration():
    c, inp, pred, calib, frames = setup()
    sets = {k: tuple(cuda(t) for t in v) for k, v in derived_sets(*(inp[k] for k in KEYS)).items()}
    per_frame = tuple(torch.stack([sets[k][i] for k in "ABD"]) for i in range(3))
    x = cuda(frames[:3])
    det = run(pred, c, x, per_frame)
    assert det["valid"].tolist() == [1, 1, 1]
    got = run(pred, c, x, per_frame, centers=det["center3d"].clone())
    for name in NAMES:
        assert same(got[name], det[name]), name
    # ... and row 1 really is projected with B's calibration: under the shared A the same centre gives other integers
    shared = run(pred, c, x, calib, centers=det["center3d"].clone())
    assert same(shared["center3d_int"], det["center3d_int"]) and not same(shared["points"][1], det["points"][1])


def test_forward_images_rows_are_different_subjects():
    c, inp, pred, calib, frames = setup()
    table, _ = centres()
    images = [cuda(inp["imgs"][cam]) for cam in range(c["C"])]
    got = run(pred, c, [images, images], calib, call="forward_images",
              centers=torch.stack([table["K1"][0], table["K2"][0]]))
    assert got["valid"].tolist() == [1, 1]
    for t, k in enumerate(("K1", "K2")):
        one = centred_single(k)
        for name in NAMES:
            assert same(got[name][t], one[name][0]), (k, name)
    assert not torch.equal(got["points"][0], got["points"][1])
    assert not torch.equal(got["center_hm"][0], got["center_hm"][1])


def test_composes_with_yuv_and_sensor_frames():
    from jarvis_hybridnet_amd import SensorSurface
    from jarvis_hybridnet_amd import synthetic as S
    c, inp, pred, calib, frames = setup()
    bgr = to_u8(frames[:1]).numpy()
    surface = SensorSurface(c["H"], c["W"], "rggb")
    raw = torch.from_numpy(S.pack_sensor_surface(S.mosaic(bgr, "rggb"), surface, 0xA5))
    for x, kw in ((torch.from_numpy(S.bgr_to_yuv420(bgr, "nv12")), dict(frame_format="nv12")),
                  (raw, dict(frame_layout=surface))):
        x = cuda(x)
        det = run(pred, c, x, calib, **kw)
        assert det["valid"].tolist() == [1], kw
        got = run(pred, c, x, calib, centers=det["center3d"].clone(), **kw)
        for name in NAMES:
            assert same(got[name], det[name]), (name, kw)


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_graph_replay_and_alternation():
    c, inp, pred, calib, frames = setup()
    table, _ = centres()
    x = cuda(frames[:1])
    g, e = native(1), native(1)
    e.graph_replay = False
    assert g.graph_replay and not e.graph_replay
    results = []
    for k in ("K1", None, "K2", "K1", None):
        centers = None if k is None else cuda(table[k][0][None])
        outs = [[t.clone() for t in p.forward(x, centers=centers)] for p in (g, e)]
        torch.cuda.synchronize()
        assert int(outs[0][2][0]) == 1
        for a, b in zip(*outs):
            assert torch.equal(a, b), k
        results.append(outs[0][0])
    # the calls are told apart by their results, and equal calls repeat theirs
    assert torch.equal(results[0], results[3]) and torch.equal(results[1], results[4])
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[0], results[2])
    assert torch.equal(results[1], detected(1)[1]["points"])


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_staged_form():
    c, inp, pred, calib, frames = setup()
    x, det = detected(3)
    K = det["center3d"].clone()
    T, C, J = 3, c["C"], c["J"]
    pr = native(T)
    heat = torch.empty((T, C, pr.Hh, pr.Hh, pr.Jp), device="cuda")
    with pytest.raises(ValueError):
        pr.stage_keypoints(x, None, heat)                   # no detections and no centres
    pr.set_centers(K)
    pr.stage_keypoints(x, None, heat)
    pts, conf = torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda")
    valid = torch.empty((T,), device="cuda", dtype=torch.int32)
    pr.stage_3d(heat, 0, pts, conf, valid)
    dbg = pr.debug("cuda")
    torch.cuda.synchronize()
    want = run(pred, c, x, calib, centers=K)
    assert valid.tolist() == [1, 1, 1]
    assert same(pts, want["points"]) and same(conf, want["conf"]) and same(valid, want["valid"])
    assert same(dbg["center3d_int"], want["center3d_int"]) and same(dbg["center_hm"], want["center_hm"])
    assert same(pts, det["points"])


# ---- 9 -------------------------------------------------------------------------------------------------------------
def test_driver(tmp_path):
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, pred, calib, frames = setup()
    cfg = make_cfg(c)
    _, det = detected(3)
    K = [det["center3d"][t % 2].cpu() for t in range(5)]
    sets = [frames[t].numpy() for t in range(5)]

    def lines(name, **kw):
        out = str(tmp_path / name)
        assert predict3D_frames(pred, iter(sets), *calib, cfg, out, time_batch=2, **kw) == 5
        return open(os.path.join(out, "data3D.csv"), "rb").read().splitlines()
    plain = lines("detected")
    got = lines("centred", centers=iter([K[0], K[1], K[2], None, K[4]]))
    assert len(plain) == len(got) == 5
    for t in (0, 1, 2, 4):
        assert got[t] == plain[t] and b"NaN" not in got[t], t
    assert list(csv.reader([got[3].decode()]))[0] == ["NaN"] * (4 * c["J"])
    fixed = lines("fixed", centers=K[0])
    assert len(fixed) == 5 and all(b"NaN" not in r for r in fixed)
    assert fixed[0] == plain[0] and fixed[1] != plain[1]
