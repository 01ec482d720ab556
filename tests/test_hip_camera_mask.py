"""GPU: per-frame camera masks.  A C-camera JarvisPredictor3D given camera_mask computes, for every frame set, what
the reference computes for the unmasked cameras alone.  References, neither of them the code under test:
  R1  the CPU oracle on the sliced inputs, oracle.predictor3d_forward(imgs[S], cam[S], intr[S], dist[S]);
  R2  a second JarvisPredictor3D built with NUM_CAMERAS = |S| from the same state dicts, given the sliced frames and
      calibration (the existing, pinned code path).
Every test here passes a mask, so every one fails on a build without the feature (no such argument)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import pytest
import torch

from tests import cases
from tests.gpu_util import cuda, max_err, report

pytestmark = pytest.mark.gpu


def make_cfg(c, cams=None):
    from jarvis_hybridnet_amd import synthetic as S
    return NS(PARENT_DIR="/nonexistent", PROJECT_NAME="none",
              DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
              CENTERDETECT=NS(MODEL_SIZE=c.get("size", "small"), NUM_JOINTS=1, IMAGE_SIZE=c["center_size"]),
              KEYPOINTDETECT=NS(MODEL_SIZE=c.get("size", "small"), NUM_JOINTS=c["J"],
                                BOUNDING_BOX_SIZE=c["bbox"]),
              HYBRIDNET=NS(NUM_CAMERAS=c["C"] if cams is None else cams, ROI_CUBE_SIZE=c["roi"],
                           GRID_SPACING=c["spacing"]))


def predictor(tag, cams=None):
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES[tag]
    inp = cases.predictor_inputs(tag)
    return JarvisPredictor3D(make_cfg(c, cams), inp["sd_center"], inp["sd_hybrid"]), c, inp


def keep(mask):
    return [i for i, m in enumerate(mask) if m]


def to_u8(imgs):
    return (imgs.permute(0, 2, 3, 1)[..., [2, 1, 0]] * 255).round().to(torch.uint8).contiguous()


def oracle(c, inp, S_idx, inter=None):
    from jarvis_hybridnet_amd import synthetic as S
    from oracle import hybridnet_oracle as O
    with torch.no_grad():
        return O.predictor3d_forward(inp["sd_center"], inp["sd_hybrid"], inp["imgs"][S_idx].contiguous(),
                                     inp["cam"][S_idx].contiguous(), inp["intr"][S_idx].contiguous(),
                                     inp["dist"][S_idx].contiguous(), center_size=c["center_size"], bbox=c["bbox"],
                                     roi_cube_size=c["roi"], grid_spacing=c["spacing"], mean=S.MEAN, std=S.STD,
                                     intermediates=inter)


# (tag, mask): "drop one", "keep exactly two", 8 of 12, "drop the dead camera of the dead-camera case".  All of these
# are valid frames for R1 (at least two of the kept cameras pass maxval > 50: asserted below from R1 itself).
# "Keep exactly two" keeps two NEIGHBOURS of the four-camera ring (90 degrees apart).  Two OPPOSITE cameras (1 and 3)
# look at the subject along nearly the same line: the two-view DLT is then ill-conditioned, R1 itself puts the centre
# 26 m away and its float32 SVD is not reproducible to the integer (the situation tests/cases.py describes for the
# dead-camera cases), so that subset is no reference for the integer paths; it is held against the |S|-camera
# predictor instead (test_masked_same_bits_as_subset_predictor).
ORACLE_SUBSETS = [
    ("cfg2", [1, 1, 0, 1]),
    ("cfg2", [1, 1, 0, 0]),
    ("cfg3", [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]),
    ("cfg3", [1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1]),
    ("cfg3_cam_black", [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]),
]


@pytest.mark.parametrize("tag,mask", ORACLE_SUBSETS)
def test_masked_vs_oracle_on_sliced_inputs(tag, mask):
    """Items 1 and 2: 3D keypoints within 1e-3 mm of R1, confidences within 1e-4 (the tolerance of
    tests/test_hip_predictor.py); center3D.int(), the clamped crop centres of the unmasked cameras and
    num_cams_detect equal R1's, the active count equals |S|."""
    pred, c, inp = predictor(tag)
    S_idx = keep(mask)
    inter = {}
    rp, rc = oracle(c, inp, S_idx, inter)
    assert rp is not None, "subset chosen so that the reference returns a valid frame"
    calib = (cuda(inp["cam"]), cuda(inp["intr"]), cuda(inp["dist"]))
    pts, conf = pred(cuda(inp["imgs"]), *calib, camera_mask=mask)
    torch.cuda.synchronize()
    assert pts is not None
    # R1 runs on THIS host's CPU, whose torch kernels may flip a few of the reference's own gather indices against
    # the fixtures' host (a truncation of u/2, v/2 within an ulp of an integer).  As in
    # __graft_entry__.smoke(), the comparison is made host-independent instead of loose: the oracle is re-run from
    # the gather on with the HIP path's indices for the oracle's own heat maps and centres (the |S|-camera
    # reprojection kernel, pinned bit for bit by tests/test_hip_stages.py::test_reprojection) and held to the
    # 1e-3 mm bar; the raw distance and the flips are reported, and every flip must be a truncation tie.
    from jarvis_hybridnet_amd.hybridnet.repro_layer import ReprojectionLayer
    from oracle import hybridnet_oracle as O
    sub_calib = tuple(inp[k][S_idx].contiguous() for k in ("cam", "intr", "dist"))
    c3i, chm = inter["center3d"].int()[None], inter["center_hm"][None]
    idx = ReprojectionLayer(make_cfg(c, len(S_idx))).gather_indices(
        cuda(inter["heatmaps_padded"]), cuda(c3i), cuda(chm), *(cuda(t)[None] for t in sub_calib)).cpu()
    hp = O.host_parity(inp["sd_hybrid"], inter, idx, pts.cpu(), rp, sub_calib, c["roi"], c["spacing"], c["bbox"])
    ref_conf = rc
    if hp["flips"]:
        with torch.no_grad():
            _, ref_conf = O.tail_with_indices(inp["sd_hybrid"], inter["heatmaps_padded"],
                                              idx.reshape((len(S_idx),) + (int(c["roi"] / c["spacing"]),) * 3).long(),
                                              c3i, c["roi"], c["spacing"])
    ep, ec = hp["same_indices_mm"], max_err(conf, ref_conf)
    pr = pred.native(c["H"], c["W"])
    dbg, dm = pr.debug("cuda"), pr.debug_mask("cuda")
    n_det_ref = int((inter["maxvals"] * 255. > 50).sum())
    e3 = max_err(dbg["center3d"][0], inter["center3d"].reshape(3))
    report("camera_mask_vs_oracle", tag=tag, cameras=len(S_idx), points_mm=ep, conf=ec, center3d_mm=e3,
           raw_points_mm=hp["raw_mm"], host_index_flips=hp["flips"], of=hp["of"],
           n_active=int(dm["n_active"][0]), num_cams_detect=int(dm["num_cams_detect"][0]), ref_detect=n_det_ref)
    print("camera_mask_vs_oracle", tag, mask, "points_mm %.3g (raw %.3g, %d host index flips of %d) conf %.3g "
          "center3d_mm %.3g" % (ep, hp["raw_mm"], hp["flips"], hp["of"], ec, e3))
    assert int(dm["n_active"][0]) == len(S_idx)
    assert int(dm["num_cams_detect"][0]) == n_det_ref
    assert torch.equal(dbg["center3d_int"][0].cpu(), inter["center3d"].reshape(3).int())
    assert torch.equal(dbg["center_hm"][0].cpu()[S_idx], inter["center_hm"].reshape(len(S_idx), 2).int())
    assert ep < 1e-3, "3D keypoints must be within 1e-3 mm of the reference on the camera subset"
    assert ec < 1e-4
    assert all(r["dist_to_integer"] <= 2.5e-4 for r in hp["flip_voxels"]), "an index flip that is not a truncation tie"


def test_masked_invalid_like_the_reference():
    """cfg2_one: one camera of four detects.  Dropping camera 3 leaves at most one detecting camera: R1 returns
    (None, None), and so does the masked predictor; so does any frame with fewer than two cameras left."""
    pred, c, inp = predictor("cfg2_one")
    mask = [1, 1, 1, 0]
    rp, rc = oracle(c, inp, keep(mask))
    assert rp is None and rc is None
    calib = (cuda(inp["cam"]), cuda(inp["intr"]), cuda(inp["dist"]))
    assert pred(cuda(inp["imgs"]), *calib, camera_mask=mask) == (None, None)
    pred2, c2, inp2 = predictor("cfg2")
    calib2 = (cuda(inp2["cam"]), cuda(inp2["intr"]), cuda(inp2["dist"]))
    assert pred2(cuda(inp2["imgs"]), *calib2, camera_mask=[0, 0, 1, 0]) == (None, None)
    assert pred2(cuda(inp2["imgs"]), *calib2, camera_mask=[0, 0, 0, 0]) == (None, None)
    dm = pred2.native(c2["H"], c2["W"]).debug_mask("cuda")
    assert int(dm["n_active"][0]) == 0 and int(dm["num_cams_detect"][0]) == 0


# cfg5 (30 joints: 32 channels, 4-thick cubes on 1024 threads) and ex72 (the ragged 72^3 grid) take other
# instantiations of the masked cube gather than the 24-channel 8-thick one of cfg2 / cfg3
@pytest.mark.parametrize("tag,mask", [("cfg2", [1, 1, 0, 1]), ("cfg2", [0, 1, 0, 1]),
                                      ("cfg3", [1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1]),
                                      ("cfg5", [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0]),
                                      ("ex72", [0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0])])
def test_masked_same_bits_as_subset_predictor(tag, mask):
    """Item 3: time_batch = 1, the masked C-camera predictor against R2, through the fp32, uint8 and I420 forms.
    One image per launch more or less does not change a kernel's arithmetic inside the time_batch < 8 class
    (DESIGN.md section 1), so the bits are equal."""
    pred, c, inp = predictor(tag)
    S_idx = keep(mask)
    sub, _, _ = predictor(tag, cams=len(S_idx))
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    calib_s = tuple(cuda(inp[k][S_idx]) for k in ("cam", "intr", "dist"))
    imgs = inp["imgs"]
    u8 = to_u8(imgs)
    forms = [("f32", lambda p, x, cal, **kw: p(cuda(x), *cal, **kw), imgs),
             ("u8", lambda p, x, cal, **kw: p.forward_uint8(cuda(x), *cal, **kw), u8)]
    forms.append(("i420", lambda p, x, cal, **kw: p.forward_yuv(cuda(x), "i420", *cal, **kw), _i420_of(u8)))
    for name, call, x in forms:
        got = call(pred, x, calib, camera_mask=mask)
        want = call(sub, x[S_idx].contiguous(), calib_s)
        torch.cuda.synchronize()
        assert got[0] is not None and want[0] is not None, name
        report("camera_mask_vs_subset_predictor", tag=tag, form=name, cameras=len(S_idx),
               points_mm=max_err(got[0], want[0]), conf=max_err(got[1], want[1]))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name


def _i420_of(u8):
    """(C,H,W,3) uint8 BGR -> (C,3H/2,W) uint8 I420 with plain BT.601 arithmetic (any valid YUV bytes do: both
    predictors convert the same bytes)."""
    b, g, r = (u8[..., k].float() for k in range(3))
    y = (16 + 0.257 * r + 0.504 * g + 0.098 * b).round().clamp(0, 255)
    u = (128 - 0.148 * r - 0.291 * g + 0.439 * b).round().clamp(0, 255)[:, ::2, ::2]
    v = (128 + 0.439 * r - 0.368 * g - 0.071 * b).round().clamp(0, 255)[:, ::2, ::2]
    C, H, W = y.shape
    return torch.cat([y.reshape(C, -1), u.reshape(C, -1), v.reshape(C, -1)], 1).to(torch.uint8).reshape(
        C, H * 3 // 2, W).contiguous()


@pytest.mark.parametrize("T", [1, 8])
def test_all_ones_equals_no_mask(T):
    """Item 4: at time_batch 1 (graph replay on) and 8."""
    pred, c, inp = predictor("cfg2")
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    x = cuda(torch.stack([inp["imgs"]] * T))
    ref = [t.clone() for t in pred.forward_batch(x, *calib)]
    got = pred.forward_batch(x, *calib, camera_mask=torch.ones(T, c["C"], dtype=torch.bool))
    torch.cuda.synchronize()
    pr = pred.native(c["H"], c["W"], time_batch=T)
    assert pr.graph_replay == (T == 1)
    assert int(ref[2].sum()) == T
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def _frame_sets(tag, n):
    """n distinct frame sets on the rig of `tag` (other subjects: other frame seeds)."""
    from jarvis_hybridnet_amd import synthetic as S
    c = cases.PREDICTOR_CASES[tag]
    calib = S.ring_calibration(c["C"], c["W"], c["H"], c["focal"])
    return torch.stack([S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"] + 100 * k)[0] for k in range(n)])


def test_per_frame_masks_in_one_batch():
    """Item 5: T = 8 distinct frame sets, a different mask in every row (an all-ones row, a one-camera row): each
    row equals, bit for bit, the same time batch run with that row's mask in every row.  The one-camera row is
    invalid; its neighbours are unaffected."""
    pred, c, inp = predictor("cfg2")
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    T = 8
    x = cuda(_frame_sets("cfg2", T))
    rows = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 1], [0, 0, 1, 0], [1, 0, 1, 1], [0, 1, 1, 1], [1, 1, 1, 0],
                         [0, 1, 0, 1], [1, 0, 1, 0]], dtype=torch.uint8)
    got = [t.clone() for t in pred.forward_batch(x, *calib, camera_mask=rows)]
    torch.cuda.synchronize()
    assert int(got[2][2]) == 0, "one camera left: an invalid frame"
    for t in range(T):
        one = pred.forward_batch(x, *calib, camera_mask=rows[t].expand(T, -1))
        torch.cuda.synchronize()
        assert int(one[2][t]) == int(got[2][t])
        if int(got[2][t]):
            assert torch.equal(one[0][t], got[0][t]) and torch.equal(one[1][t], got[1][t]), t
    plain = pred.forward_batch(x, *calib)
    torch.cuda.synchronize()
    assert torch.equal(plain[0][0], got[0][0]) and torch.equal(plain[1][0], got[1][0])     # the all-ones row
    assert int(got[2].sum()) >= T - 2


def test_garbage_in_masked_slots():
    """Item 6: NaN (fp32) resp. 0xFF (uint8, I420) in the masked cameras' frame slots: same bits as clean frames."""
    pred, c, inp = predictor("cfg3")
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    mask = torch.tensor([1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1], dtype=torch.bool)
    dead = (~mask).nonzero().flatten()
    imgs = inp["imgs"]
    u8 = to_u8(imgs)
    yuv = _i420_of(u8)
    for name, clean, fill, call in (
            ("f32", imgs, float("nan"), lambda x: pred(cuda(x), *calib, camera_mask=mask)),
            ("f32_inf", imgs, float("inf"), lambda x: pred(cuda(x), *calib, camera_mask=mask)),
            ("u8", u8, 255, lambda x: pred.forward_uint8(cuda(x), *calib, camera_mask=mask)),
            ("i420", yuv, 255, lambda x: pred.forward_yuv(cuda(x), "i420", *calib, camera_mask=mask))):
        want = call(clean)
        dirty = clean.clone()
        dirty[dead] = fill
        got = call(dirty)
        torch.cuda.synchronize()
        assert want[0] is not None and got[0] is not None, name
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
    # time batch 8 (the row-streaming BiFPN nodes and >= 64 KB statistic blocks) with NaN slots
    T = 8
    x = torch.stack([imgs] * T)
    rows = mask.expand(T, -1)
    want = [t.clone() for t in pred.forward_batch(cuda(x), *calib, camera_mask=rows)]
    x[:, dead] = float("nan")
    got = pred.forward_batch(cuda(x), *calib, camera_mask=rows)
    torch.cuda.synchronize()
    assert int(want[2].sum()) == T
    for a, b in zip(want, got):
        assert torch.equal(a, b)


def test_graph_replay_with_changing_masks():
    """Item 7: one predictor, time_batch 1, three masks and then None; each equals its fresh-predictor result."""
    pred, c, inp = predictor("cfg2")
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    x = cuda(inp["imgs"])
    masks = [[1, 1, 0, 1], [0, 1, 1, 1], [1, 0, 1, 0], None]
    got = []
    for m in masks:
        p, q = pred(x, *calib, camera_mask=m)
        got.append((p.clone(), q.clone()))
    assert pred.native(c["H"], c["W"]).graph_replay
    for m, (p, q) in zip(masks, got):
        fresh, _, _ = predictor("cfg2")
        fp, fq = fresh(x, *calib, camera_mask=m)
        torch.cuda.synchronize()
        assert torch.equal(p, fp) and torch.equal(q, fq), m


def test_driver_masks(tmp_path):
    """Item 8: predict3D_frames with a (C,) mask writes the CSV of R2 on the sliced frame sets, byte for byte; with
    a per-frame-set mask iterator that leaves one camera for frames 2..4, exactly those rows are NaN and the others
    are the unmasked run's."""
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    pred, c, inp = predictor("cfg2")
    mask = [1, 1, 0, 1]
    S_idx = keep(mask)
    sub, _, _ = predictor("cfg2", cams=len(S_idx))
    sets = [to_u8(f) for f in _frame_sets("cfg2", 6)]
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    calib_s = tuple(cuda(inp[k][S_idx]) for k in ("cam", "intr", "dist"))

    def run(p, frames, cal, name, cams, **kw):
        out = tmp_path / name
        n = predict3D_frames(p, frames, *cal, make_cfg(c, cams), str(out), **kw)
        assert n == len(sets)
        return (out / "data3D.csv").read_bytes()

    a = run(pred, [s.numpy() for s in sets], calib, "masked", None, camera_mask=mask)
    b = run(sub, [s[S_idx].contiguous().numpy() for s in sets], calib_s, "subset", len(S_idx))
    assert a == b
    full = run(pred, [s.numpy() for s in sets], calib, "full", None).splitlines()
    per = [None if not 2 <= k <= 4 else [0, 0, 1, 0] for k in range(len(sets))]
    rows = run(pred, [s.numpy() for s in sets], calib, "per_frame", None, camera_mask=iter(per)).splitlines()
    assert len(rows) == len(full) == len(sets)
    for k, (r, f) in enumerate(zip(rows, full)):
        if 2 <= k <= 4:
            assert set(r.split(b",")) == {b"NaN"}, k
        else:
            assert r == f, k


# ---- the voxel-row form of the masked gather (repro_gather_masked_kernel): what the predictor launches when the grid
# is no multiple of 8, for more than 32 channels, or under JH_REPRO_CUBE=0
def _wide_case():
    """The cfg2 rig with 36 joints: 40 channels, more than the cube form takes, so launch_reproject (given a mask) sends it
    to repro_gather_masked_kernel<10>."""
    from jarvis_hybridnet_amd import synthetic as S
    c = dict(cases.PREDICTOR_CASES["cfg2"], J=36)
    calib = S.ring_calibration(c["C"], c["W"], c["H"], c["focal"])
    imgs, _, _ = S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"])
    return c, dict(sd_center=S.efficienttrack_weights("small", 1, c["cseed"]),
                   sd_hybrid=S.hybridnet_weights("small", c["J"], c["hseed"]), imgs=imgs, cam=calib[0], intr=calib[1],
                   dist=calib[2])


@pytest.mark.parametrize("mask", [[1, 1, 0, 1], [0, 1, 1, 0], [1, 1, 1, 1]])
def test_masked_row_gather_wide_joint_count(mask):
    """40 channels: the row form by geometry.  Masked against the |S|-camera predictor bit for bit (fp32 and uint8),
    NaN / 0xFF in the masked slots without effect, a batch of 8 with one mask per row."""
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c, inp = _wide_case()
    assert (c["J"] + 7) // 8 * 8 > 32
    S_idx = keep(mask)
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    sub = JarvisPredictor3D(make_cfg(c, len(S_idx)), inp["sd_center"], inp["sd_hybrid"])
    calib = tuple(cuda(inp[k]) for k in ("cam", "intr", "dist"))
    calib_s = tuple(cuda(inp[k][S_idx]) for k in ("cam", "intr", "dist"))
    imgs, u8 = inp["imgs"], to_u8(inp["imgs"])
    dead = [i for i, m in enumerate(mask) if not m]
    for name, x, fill, call in (("f32", imgs, float("nan"), lambda p, x, cal, **kw: p(cuda(x), *cal, **kw)),
                                ("u8", u8, 255, lambda p, x, cal, **kw: p.forward_uint8(cuda(x), *cal, **kw))):
        got = call(pred, x, calib, camera_mask=mask)
        want = call(sub, x[S_idx].contiguous(), calib_s)
        dirty = x.clone()
        dirty[dead] = fill
        nan = call(pred, dirty, calib, camera_mask=mask)
        torch.cuda.synchronize()
        assert got[0] is not None and want[0] is not None, name
        report("camera_mask_row_gather", form=name, cameras=len(S_idx), points_mm=max_err(got[0], want[0]))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
        assert torch.equal(got[0], nan[0]) and torch.equal(got[1], nan[1]), name
    T = 8
    rows = torch.tensor([mask, [1, 1, 1, 1], [0, 0, 1, 0], [1, 0, 1, 1]] * 2, dtype=torch.uint8)
    x = cuda(torch.stack([imgs] * T))
    got = [t.clone() for t in pred.forward_batch(x, *calib, camera_mask=rows)]
    assert got[2].tolist() == [int(sum(r) >= 2) for r in rows.tolist()]
    for t in range(4):
        one = pred.forward_batch(x, *calib, camera_mask=rows[t].expand(T, -1))
        torch.cuda.synchronize()
        for u in (t, t + 4):
            if int(got[2][u]):
                assert torch.equal(one[0][u], got[0][u]) and torch.equal(one[1][u], got[1][u]), (t, u)


@pytest.mark.parametrize("tag,mask", [("cfg3", "101101101101"), ("cfg2", "1101")])
def test_masked_row_gather_in_a_child_process(tag, mask):
    """JH_REPRO_CUBE=0 (read once per process: a fresh child, tests/camera_mask_worker.py): the 24-channel row form at
    the cfg2 / cfg3 geometries against the |S|-camera predictor, NaN in the masked slots, all ones against no mask."""
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "camera_mask_worker.py"), tag, mask], cwd=root,
                       env=dict(os.environ, JH_REPRO_CUBE="0"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    report("camera_mask_row_gather_child", **line)
    assert line["subset_equal"] and line["garbage_equal"] and line["ones_equal"], line


def test_masked_staged_calls_equal_the_masked_forward():
    """jh_predictor_stage_keypoints_masked + jh_predictor_stage_3d_masked behind stage_center: the masked forward in
    three calls, bit for bit (T = 2, one mask per row), with the counts of the masked triangulation."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    T, C, J = 2, c["C"], c["J"]
    pr = NativePredictor(inp["sd_center"], inp["sd_hybrid"], num_cameras=C, num_joints=J, center_size=c["center_size"],
                         bbox=c["bbox"], roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"],
                         mean=S.MEAN, std=S.STD, time_batch=T)
    pr.set_calibration(*(cuda(inp[k]) for k in ("cam", "intr", "dist")))
    frames = cuda(_frame_sets("cfg2", T))
    mask = cuda(torch.tensor([[1, 1, 0, 1], [0, 1, 1, 1]], dtype=torch.uint8))
    want = [t.clone() for t in pr.forward(frames, camera_mask=mask)]
    det = torch.empty((T, C, 3), device="cuda")
    heat = torch.empty((T, C, pr.Hh, pr.Hh, pr.Jp), device="cuda")
    pts, conf = torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda")
    valid = torch.empty((T,), device="cuda", dtype=torch.int32)
    pr.stage_center(frames, det)
    pr.stage_keypoints(frames, det, heat, camera_mask=mask)
    pr.stage_3d(heat, 0, pts, conf, valid, camera_mask=mask)
    dm = pr.debug_mask("cuda")
    torch.cuda.synchronize()
    assert int(want[2].sum()) == T and torch.equal(valid, want[2])
    assert torch.equal(pts, want[0]) and torch.equal(conf, want[1])
    assert dm["n_active"].tolist() == [3, 3]
    with pytest.raises(ValueError):
        pr.stage_3d(heat, 0, pts, conf, valid, camera_mask=mask.cpu())
