"""GPU: centre keyframes (jh_predictor_set_center_keyframes): CenterDetect on the key rows of a time batch, the rows in
between on a centre interpolated between their two key rows.

Everything is bit for bit.  The feature is defined through two things that are tested already -- a key row's detection
has the bits of the detected call, and a centred call equals the detected one on its centres -- so a keyframe call must
equal the centred call on the centres tests/center_keys_ref.py builds, in numpy float32, from the DETECTED call's float
centres at the key rows.

All on cfg2 (tests/cases.py: 4 cameras 640 x 512, small / small, 48^3 grid) at T = 8, on the eight frame sets of
tests/test_hip_centers.py (two valid frame sets alternating).  Every test passes `center_every=` or calls
set_center_keyframes, so every one fails on a build without the feature."""
import csv
import functools
import io
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import cases
from tests import center_keys_ref as R
from tests.gpu_util import cuda

pytestmark = pytest.mark.gpu

TAG, T = "cfg2", 8
KEYS = ("cam", "intr", "dist")
NAMES = ("points", "conf", "valid", "center3d_int", "center_hm")
VIEWS = ("points2D", "confidences2D", "reprojections", "errors", "used")


def make_cfg(c):
    from jarvis_hybridnet_amd import synthetic as S
    return NS(PARENT_DIR="/nonexistent", PROJECT_NAME="none",
              DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
              CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center_size"]),
              KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
              HYBRIDNET=NS(NUM_CAMERAS=c["C"], ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))


@functools.lru_cache(maxsize=None)
def setup():
    """The cfg2 predictor, its calibration on the device and the 8 frame sets (fp32, host); shared, never changed."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES[TAG]
    inp = cases.predictor_inputs(TAG)
    calib = tuple(inp[k] for k in KEYS)
    two = [inp["imgs"], S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"] + 100)[0]]
    frames = torch.stack([two[t % 2] for t in range(T)])
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    return c, inp, pred, tuple(cuda(t) for t in calib), frames


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def to_u8(imgs):
    return (imgs.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).contiguous()


def run(pred, c, x, calib, call="forward_batch", **kw):
    """One batched forward and the predictor's debug tensors -> dict of clones.  The extras of the result are taken in
    their order: Views2D, Spread3D, JointMask, CenterKeyframes."""
    res = getattr(pred, call)(x, *calib, **kw)
    pr = pred.native(c["H"], c["W"], time_batch=len(x))
    out = dict(points=res[0], conf=res[1], valid=res[2])
    rest = list(res[3:])
    if kw.get("return_2d"):
        out.update(rest.pop(0)._asdict())
    if kw.get("return_spread"):
        out.update({"spread_" + k: v for k, v in rest.pop(0)._asdict().items()})
    if kw.get("joint_mask") is not None:
        out.update({"jm_" + k: v for k, v in rest.pop(0)._asdict().items()})
    if kw.get("center_every") is not None:
        kf = rest.pop(0)
        out.update(kf_centers=kf.centers, kf_source=kf.source)
    assert not rest
    dbg = pr.debug("cuda")
    out.update(center3d=dbg["center3d"], center3d_int=dbg["center3d_int"], center_hm=dbg["center_hm"], det=dbg["det"])
    if kw.get("camera_mask") is not None:
        out.update(pr.debug_mask("cuda"))
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def ref_centres(det, every, n_rows=T, valid=None):
    """The reference fill of the detected call's float centres at the key rows -> (centers (T,3) tensor, source list)."""
    keys = R.key_rows(T, every, n_rows)
    c3f, ok = det["center3d"].cpu().numpy(), det["valid"].cpu().numpy() if valid is None else valid
    centers, source = R.fill(T, every, n_rows, {k: c3f[k] for k in keys}, {k: bool(ok[k]) for k in keys})
    return torch.from_numpy(centers), source.tolist()


def compare(got, want, names, rows=None):
    for name in names:
        a, b = (got[name], want[name]) if rows is None else (got[name][rows], want[name][rows])
        assert same(a, b), name


@functools.lru_cache(maxsize=None)
def detected():
    """The 8 frame sets run DETECTED: computed once."""
    c, inp, pred, calib, frames = setup()
    x = cuda(frames)
    det = run(pred, c, x, calib)
    assert det["valid"].tolist() == [1] * T
    # the precondition: the two frame sets' centres differ by more than 1 mm, so the interpolation is not trivial
    assert float((det["center3d"][0] - det["center3d"][1]).abs().max()) > 1.0
    return x, det


def native(time_batch, center=True, **kw):
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, _, calib, _ = setup()
    pr = NativePredictor(inp["sd_center"] if center else None, inp["sd_hybrid"], num_cameras=c["C"],
                         num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
                         grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD,
                         time_batch=time_batch, **kw)
    if kw.get("cam_n") is None:
        pr.set_calibration(*calib)
    return pr


# ---- 1 -------------------------------------------------------------------------------------------------------------
def test_every_1_is_the_detected_call():
    c, inp, pred, calib, _ = setup()
    x, det = detected()
    got = run(pred, c, x, calib, center_every=1)
    compare(got, det, NAMES + ("center3d", "det"))
    assert got["kf_source"].tolist() == [0] * T and same(got["kf_centers"], det["center3d"])


# ---- 2 -------------------------------------------------------------------------------------------------------------
def test_every_3_equals_the_centred_call_on_the_reference_centres():
    c, inp, pred, calib, _ = setup()
    x, det = detected()
    ref, source = ref_centres(det, 3)
    assert source == [0, 1, 1, 0, 1, 1, 0, 0]
    want = run(pred, c, x, calib, centers=ref, return_2d=True)
    got = run(pred, c, x, calib, center_every=3, return_2d=True)
    assert got["valid"].tolist() == [1] * T
    compare(got, want, NAMES + VIEWS + ("center3d",))
    keys = [0, 3, 6, 7]
    compare(got, det, NAMES + ("center3d", "det"), rows=keys)    # a key row is the detected call's row
    assert same(got["kf_centers"].cpu(), ref) and got["kf_source"].tolist() == source
    assert not got["det"][[1, 2, 4, 5]].any()
    # rows 1 and 2 lie between two different centres: they are NOT the detected call's rows
    assert not same(got["center3d"][1], det["center3d"][1]) and not same(got["points"][1], det["points"][1])


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invalid,valid,source", [
    ((3,), [1, 1, 1, 0, 1, 1, 1, 1], [0, 2, 2, -1, 2, 2, 0, 0]),
    ((3, 6), [1, 1, 1, 0, 0, 0, 0, 1], [0, 2, 2, -1, -1, -1, -1, 0]),
])
def test_invalid_keys_by_camera_mask(invalid, valid, source):
    c, inp, pred, calib, _ = setup()
    x, det = detected()
    mask = torch.ones((T, c["C"]), dtype=torch.uint8)
    for t in invalid:
        mask[t] = torch.tensor([1, 0, 0, 0])                    # one camera: no detection there
    ok = np.ones(T, bool)
    ok[list(invalid)] = False
    ref, ref_source = ref_centres(det, 3, valid=ok)             # (a full mask row has the unmasked call's centre)
    assert ref_source == source
    want = run(pred, c, x, calib, centers=ref, camera_mask=mask)
    got = run(pred, c, x, calib, center_every=3, camera_mask=mask)
    assert got["valid"].tolist() == valid == want["valid"].tolist()
    assert got["kf_source"].tolist() == source and same(got["kf_centers"].cpu(), ref)
    live = [t for t in range(T) if valid[t]]
    compare(got, want, ("points", "conf"), rows=live)
    compare(got, want, ("valid", "center3d_int", "center_hm", "center3d", "n_active", "num_cams_detect"))
    # held rows: key 0's centre in rows 1 and 2
    assert same(got["center3d"][1], det["center3d"][0]) and same(got["center3d"][2], det["center3d"][0])
    if invalid == (3,):
        assert same(got["center3d"][4], det["center3d"][6]) and same(got["center3d"][5], det["center3d"][6])


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_n_rows_6_every_4():
    c, inp, pred, calib, _ = setup()
    x, det = detected()
    ref, source = ref_centres(det, 4, 6)
    assert source == [0, 1, 1, 1, 0, 0, 2, 2]
    want = run(pred, c, x, calib, centers=ref)
    got = run(pred, c, x, calib, center_every=(4, 6))
    compare(got, want, NAMES + ("center3d",))
    assert same(got["kf_centers"].cpu(), ref) and got["kf_source"].tolist() == source
    for t in (6, 7):
        assert same(got["center3d"][t], det["center3d"][5])
    compare(got, det, NAMES + ("det",), rows=[0, 4, 5])
    assert not got["det"][[1, 2, 3, 6, 7]].any()


# ---- 5 -------------------------------------------------------------------------------------------------------------
def derived_b(cam, intr, dist):
    """Set B of tests/test_hip_calibration_frames.py: the world frame translated by (30, -20, 10) mm."""
    d = torch.tensor([30.0, -20.0, 10.0])
    cam_b = cam.clone()
    cam_b[:, 3] = cam[:, 3] - torch.einsum("k,ckj->cj", d, cam[:, 0:3])
    return cam_b, intr.clone(), dist.clone()


@pytest.mark.parametrize("case", ["u8", "images", "nv12_tone", "calibration_frames", "spread", "consensus"])
def test_composition(case):
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd.tone import ToneTables
    c, inp, pred, calib, frames = setup()
    call, kw, extra, tone = "forward_batch", {}, (), None
    x = cuda(frames)
    if case == "u8":
        x = cuda(to_u8(frames))
    elif case == "images":
        # every image a tensor of its own, allocated in reverse order: nothing is contiguous or ascending
        flat = [cuda(to_u8(frames)[t, cam]).clone() for t in reversed(range(T)) for cam in reversed(range(c["C"]))][::-1]
        x, call = [flat[t * c["C"]:(t + 1) * c["C"]] for t in range(T)], "forward_images"
    elif case == "nv12_tone":
        x, kw = cuda(torch.from_numpy(S.bgr_to_yuv420(to_u8(frames).numpy(), "nv12"))), dict(frame_format="nv12")
        tone = ToneTables.from_curve(c["C"], black=(0, 1, 2, 3), gamma=(1.0, 1.05, 0.95, 1.0))
    elif case == "calibration_frames":
        a = tuple(inp[k] for k in KEYS)
        sets = (tuple(cuda(t) for t in a), tuple(cuda(t) for t in derived_b(*a)))
        calib = tuple(torch.stack([sets[t % 2][i] for t in range(T)]) for i in range(3))
    elif case == "spread":
        kw, extra = dict(return_spread=True), ("spread_cov", "spread_peak", "spread_mass")
    elif case == "consensus":
        kw, extra = dict(joint_mask="consensus"), ("jm_cameras", "jm_count")
    try:
        if tone is not None:
            pred.set_tone(tone)
        det = run(pred, c, x, calib, call, **kw)
        assert det["valid"].tolist() == [1] * T, case
        ref, source = ref_centres(det, 3)
        want = run(pred, c, x, calib, call, centers=ref, **kw)
        got = run(pred, c, x, calib, call, center_every=3, **kw)
    finally:
        if tone is not None:
            pred.set_tone(None)
    assert got["valid"].tolist() == [1] * T
    compare(got, want, NAMES + ("center3d",) + extra)
    assert same(got["kf_centers"].cpu(), ref) and got["kf_source"].tolist() == source
    compare(got, det, NAMES + ("det",), rows=[0, 3, 6, 7])


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_leaves_things_alone():
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, _ = setup()
    x, det = detected()
    pr = native(T)
    before = pr.device_bytes
    first = [t.clone() for t in pr.forward(x)]
    assert N.lib().jh_predictor_device_bytes(pr.handle) == before          # a predictor that does not ask
    pr.set_center_keyframes(3)
    assert pr.device_bytes > before and N.lib().jh_predictor_device_bytes(pr.handle) == pr.device_bytes
    grown = pr.device_bytes
    pr.set_center_keyframes(3, 5)                                          # n_rows alone: nothing is built
    assert pr.device_bytes == grown
    pr.forward(x, center_every=3)
    again = [t.clone() for t in pr.forward(x)]                             # a plain detected call afterwards
    torch.cuda.synchronize()
    for a, b, name in zip(again, first, ("points", "conf", "valid")):
        assert same(a, b) and same(a, det[name]), name
    # time_batch 1: one key slot, the detected call, and the graphs are not touched
    one = native(1)
    assert one.graph_replay
    x1 = x[:1]
    plain = [t.clone() for t in one.forward(x1)]
    records = one.graph_records
    assert records == 1
    res = one.forward(x1, center_every=1)
    keyed, kf = [t.clone() for t in res[:3]], res[3]
    replay = [t.clone() for t in one.forward(x1)]
    torch.cuda.synchronize()
    assert one.graph_records == records
    assert kf.source.tolist() == [0]
    # (the T = 1 predictor's own detected call: time batches below 8 are another class than the T = 8 reference)
    assert int(plain[2][0]) == 1
    for a, b, d in zip(keyed, replay, plain):
        assert same(a, d) and same(b, d)


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, _ = setup()
    x, det = detected()
    pr = native(T)
    for every, n_rows, what in ((3, 0, "n_rows"), (3, T + 1, "n_rows"), (-1, T, "every")):
        with pytest.raises(RuntimeError, match=what):
            pr.set_center_keyframes(every, n_rows)
        assert not pr._keyframed
    with pytest.raises(RuntimeError, match="without CenterDetect weights"):
        native(T, center=False).set_center_keyframes(3)
    with pytest.raises(RuntimeError, match="all cameras local"):
        native(T, cam_lo=0, cam_n=2).set_center_keyframes(3)
    # centres and keyframes both in force: the forward names both and enqueues nothing
    pr.set_centers(det["center3d"].clone())
    pr.set_center_keyframes(3)
    out = (torch.full((T, c["J"], 3), 7.0, device="cuda"), torch.full((T, c["J"]), 7.0, device="cuda"),
           torch.full((T,), 7, device="cuda", dtype=torch.int32))
    with pytest.raises(RuntimeError) as e:
        N.call_forward("jh_predictor", pr.handle, pr._describe(x), None, out)
    assert "jh_predictor_set_centers" in str(e.value) and "jh_predictor_set_center_keyframes" in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)
    # ... and the predictor is as good as before: the next plain call clears both and detects
    got = [t.clone() for t in pr.forward(x)]
    torch.cuda.synchronize()
    for a, name in zip(got, ("points", "conf", "valid")):
        assert same(a, det[name]), name
    # the public forms refuse before anything is touched
    for bad in (dict(center_every=(3, T + 1)), dict(center_every=0), dict(center_every=3, centers=det["center3d"])):
        with pytest.raises(ValueError):
            pred.forward_batch(x, *calib, **bad)


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_driver(tmp_path):
    from jarvis_hybridnet_amd.prediction.predict3D import frame_row, predict3D_frames
    c, inp, pred, calib, frames = setup()
    cfg = make_cfg(c)
    n = 13
    sets = [frames[t % T].numpy() for t in range(n)]

    def data3d(name, streams):
        out = str(tmp_path / name)
        assert predict3D_frames(pred, iter(sets), *calib, cfg, out, time_batch=T, streams=streams, center_every=3) == n
        return open(os.path.join(out, "data3D.csv"), "rb").read()
    # the CSV assembled from forward_batch per group: the short last group has 5 real rows behind which its last frame
    # set repeats
    text = io.StringIO(newline="")
    writer = csv.writer(text, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)
    for t0 in range(0, n, T):
        real = min(T, n - t0)
        group = [frames[t % T] for t in range(t0, t0 + real)]
        x = cuda(torch.stack(group + [group[-1]] * (T - real)))
        pts, conf, valid, kf = pred.forward_batch(x, *calib, center_every=(3, real))
        torch.cuda.synchronize()
        assert kf.source.tolist() == ([0, 1, 1, 0, 1, 1, 0, 0] if real == T else [0, 1, 1, 0, 0, 2, 2, 2])
        for t in range(real):
            assert int(valid[t]) == 1
            writer.writerow(frame_row(pts[t].cpu(), conf[t].cpu(), c["J"]))
    want = text.getvalue().encode()
    two = data3d("two", 2)
    assert two == want and len(two.splitlines()) == n
    assert data3d("one", 1) == two
