"""GPU: per-joint camera masks -- the joint-masked voxel gather against its fp32 reference on the pinned gather indices
(tests/joint_mask_ref.py), the predictor's staged and whole-path forms against themselves over the equalities the
definition states (include/jarvis_hip.h), the consensus form against the composition it stands for, graph replay around
it, its composition with centres, spread and per-frame-set calibration, and the driver.

Bounds: everything is compared bit for bit.  The reference sums the tapped values in camera order in fp32 from +0 through
torch.where and divides once in fp32 -- the operations the kernel is defined by --, so no tolerance is needed there
either.  The predictor tests run on cfg2 (tests/cases.py: 4 cameras 640 x 512, 23 joints in 24 channels, 48^3 grid), where
the plain gather is the cube form and the joint-masked one the voxel-row form, and on the 36-joint rig of
tests/test_hip_camera_mask.py, where both are the row form.  Every test passes a joint_mask."""
import csv
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases
from tests import joint_mask_ref as R
from tests import joints3d_ref as JR
from tests import test_hip_centers as HC
from tests import test_hip_joints3d as HJ
from tests.gpu_util import cuda, report

pytestmark = pytest.mark.gpu
same = HC.same

# 3 cameras, 36 joints (40 channels: ten quads per voxel), a 12^3 grid: built like the cases of tests/cases.py
WIDE_REPRO = (3, 36, 12, 4, 28, 160, 128, 300.0, 17)


@pytest.fixture(scope="module", autouse=True)
def shared_scene_left_as_found():
    """tests/test_hip_joints3d.py caches its scene together with the centre set the scene's forward left in the shared
    predictor; the forwards of this file move that set, so the cache goes and that file builds its scene again."""
    yield
    HJ.centred.cache_clear()


def u8(x):
    return cuda(torch.as_tensor(np.asarray(x), dtype=torch.uint8))


# ---- 1: the operator ----------------------------------------------------------------------------------------------------
def repro_case(tag):
    if tag != "wide":
        return cases.REPRO_CASES[tag], cases.repro_inputs(tag)
    from jarvis_hybridnet_amd import synthetic as S
    C, J, G, spacing, bbox, W, H, focal, seed = WIDE_REPRO
    cam, intr, dist, centre, chm = cases.subject_geometry(C, W, H, focal, bbox, seed)
    hm_pad = F.pad(S.smooth_heatmaps(C, J, bbox // 2, seed + 100), [1, 1, 1, 1])[None]
    return WIDE_REPRO, dict(hm_pad=hm_pad.contiguous(), center3d=centre.int()[None], center_hm=chm[None], cam=cam[None],
                            intr=intr[None], dist=dist[None])


def joint_rows(J, C):
    """(J,C): row j has j % (C + 1) cameras, starting at camera 3 j % C -- every size from empty to full."""
    jm = np.zeros((J, C), np.uint8)
    for j in range(J):
        for k in range(j % (C + 1)):
            jm[j, (3 * j + k) % C] = 1
    return jm


@pytest.mark.parametrize("tag", ["tiny", "cfg2", "wide"])
def test_operator_equals_the_reference(tag):
    from types import SimpleNamespace as NS
    from jarvis_hybridnet_amd.hybridnet.repro_layer import ReprojectionLayer
    (C, J, G, spacing, bbox, W, H, focal, seed), inp = repro_case(tag)
    layer = ReprojectionLayer(NS(HYBRIDNET=NS(GRID_SPACING=spacing, ROI_CUBE_SIZE=G * spacing, NUM_CAMERAS=C),
                                 KEYPOINTDETECT=NS(BOUNDING_BOX_SIZE=bbox)))
    keys = ("hm_pad", "center3d", "center_hm", "cam", "intr", "dist")
    args = [cuda(inp[k]) for k in keys]
    idx = layer.gather_indices(*args).cpu()                 # (the pinned existing path)
    jm = joint_rows(J, C)
    sizes = jm.sum(1).tolist()
    assert set(sizes) == set(range(C + 1)) and 0 in sizes and 1 in sizes and C in sizes
    cam_mask = [0 if c == 1 else 1 for c in range(C)]
    for mask in (None, cam_mask):
        e, n = R.effective_sets(jm[None], None if mask is None else [mask])
        want = R.gather_ref(inp["hm_pad"][0], idx, e[0])
        got = layer(*args, joint_mask=jm, camera_mask=mask)
        # the planes that no voxel's sum may touch hold NaN: the volume stays finite and keeps its bits
        dirty = inp["hm_pad"].clone()
        dirty[0].permute(1, 0, 2, 3)[torch.from_numpy(e[0] == 0)] = float("nan")
        assert int(torch.isnan(dirty).sum()) > 0
        nan = layer(cuda(dirty), *args[1:], joint_mask=torch.from_numpy(jm), camera_mask=mask)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (1, J, G, G, G) and bool(torch.isfinite(nan).all())
        diff = (got[0].cpu() - want).abs().max().item()
        print("joint-masked gather %s, camera mask %s: max |got - ref| = %g, max |ref| = %g"
              % (tag, mask, diff, want.abs().max().item()))
        report("joint_mask_operator", case=tag, camera_mask=mask is not None, max_abs_diff=diff)
        assert float(want.abs().max()) > 0
        assert same(got[0].cpu(), want), (tag, mask, diff)
        assert same(nan, got), (tag, mask)
    # all ones is the plain operator wherever the division by C is the same in both forms; a camera mask alone is the
    # uniform joint mask
    ones = layer(*args, joint_mask=np.ones((J, C), np.uint8))
    only = layer(*args, camera_mask=cam_mask)
    rows = layer(*args, joint_mask=np.tile(np.asarray(cam_mask, np.uint8), (J, 1)))
    torch.cuda.synchronize()
    assert same(only, rows)
    if C in (2, 4):                                          # (a power of two: x / C is exact in every form)
        assert same(ones, layer(*args))


# ---- 2: the predictor, staged -------------------------------------------------------------------------------------------
def scene():
    """The cfg2 predictor at T = 2 with the centre set of tests/test_hip_joints3d.py's heat-map scene in force."""
    c, inp, pred, calib, frames = HC.setup()
    pr, centres, chm, calib64, heat, truth, _ = HJ.centred()
    pred.forward_batch(cuda(frames[:2]), *calib, centers=centres)        # (other tests move the centre set)
    return c, pr, chm, calib64, heat


def stage3(pr, heat_dev, camera_mask=None, joint_mask=None, T=2):
    """stage_3d on device heat maps -> points, conf on the host."""
    pts, conf = torch.empty((T, pr.J, 3), device="cuda"), torch.empty((T, pr.J), device="cuda")
    valid = torch.empty((T,), device="cuda", dtype=torch.int32)
    m = None if camera_mask is None else u8(camera_mask)
    jm = None if joint_mask is None else u8(joint_mask)
    pr.stage_3d(heat_dev, 0, pts, conf, valid, camera_mask=m, joint_mask=jm)
    torch.cuda.synchronize()
    assert valid.tolist() == [1] * T
    return pts.cpu(), conf.cpu()


def eq(a, b):
    return same(a[0], b[0]) and same(a[1], b[1])


def batch_rows(T, J, C):
    """(T,J,C): row t is joint_rows shifted by t joints -- the rows of a batch differ."""
    return np.stack([np.roll(joint_rows(J, C), t + 1, axis=0) for t in range(T)])


def test_staged_equalities():
    c, pr, chm, calib64, heat = scene()
    J, C = c["J"], c["C"]
    dev = cuda(torch.from_numpy(heat))
    plain = stage3(pr, dev)
    ones = np.ones((2, J, C), np.uint8)
    # (a) all ones is the plain stage 3 (here the cube form: same indices, same sum order)
    assert eq(stage3(pr, dev, joint_mask=ones), plain)
    got = pr.joint_mask()
    assert got.cameras.cpu().tolist() == ones.tolist() and got.count.cpu().tolist() == [[C] * J] * 2
    # (b) uniform rows are the camera mask
    m = np.array([[1, 1, 0, 1], [0, 1, 1, 1]], np.uint8)
    masked = stage3(pr, dev, camera_mask=m)
    assert not eq(masked, plain)
    assert eq(stage3(pr, dev, joint_mask=np.broadcast_to(m[:, None, :], (2, J, C)).copy()), masked)
    # (c) a camera mask composes as jm & m (on rows that keep a camera)
    jm = batch_rows(2, J, C)
    jm[(jm & m[:, None, :]).sum(-1) == 0] = 1
    both = stage3(pr, dev, camera_mask=m, joint_mask=jm)
    e, n = R.effective_sets(jm, m)
    got = pr.joint_mask()
    assert got.cameras.cpu().tolist() == e.tolist() and got.count.cpu().tolist() == n.tolist()
    assert (n >= 1).all() and (n < 3).any()
    assert eq(stage3(pr, dev, joint_mask=jm & m[:, None, :]), both)
    assert not eq(both, masked)
    # (d) all zero is the plain result (every joint falls back)
    assert eq(stage3(pr, dev, joint_mask=np.zeros((2, J, C), np.uint8)), plain)
    assert pr.joint_mask().cameras.cpu().tolist() == ones.tolist()


def test_staged_selection_and_row_independence():
    c, pr, chm, calib64, heat = scene()
    J, C = c["J"], c["C"]
    jm = batch_rows(2, J, C)
    assert (jm[0] != jm[1]).any() and set(jm.sum(-1).reshape(-1).tolist()) == set(range(C + 1))
    e, n = R.effective_sets(jm)
    got = stage3(pr, cuda(torch.from_numpy(heat)), joint_mask=jm)
    sets = pr.joint_mask()
    assert sets.cameras.cpu().tolist() == e.tolist() and sets.count.cpu().tolist() == n.tolist()
    # (e) NaN wherever a value is selected out changes no bit
    dirty = heat.copy()
    off = np.broadcast_to((e == 0).transpose(0, 2, 1)[:, :, None, None, :], dirty[..., :J].shape)
    dirty[..., :J][off] = np.nan
    assert np.isnan(dirty).any()
    assert eq(stage3(pr, cuda(torch.from_numpy(dirty)), joint_mask=jm), got)
    # (f) row t is row t of the batch with row t's mask on all rows
    dev = cuda(torch.from_numpy(heat))
    for t in range(2):
        one = stage3(pr, dev, joint_mask=np.stack([jm[t]] * 2))
        assert same(one[0][t], got[0][t]) and same(one[1][t], got[1][t]), t
    assert not eq(stage3(pr, dev, joint_mask=np.stack([jm[0]] * 2)), got)


@functools.lru_cache(maxsize=None)
def wide_rig():
    """The 36-joint cfg2 rig of tests/test_hip_camera_mask.py (40 channels: the plain gather is the row form too), one
    frame set taken through the staged calls -> the native predictor, its heat maps."""
    from tests import test_hip_camera_mask as CM
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c, inp = CM._wide_case()
    pred = JarvisPredictor3D(CM.make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    pr = pred.native(c["H"], c["W"], time_batch=1)
    pr.set_calibration(*(cuda(inp[k]) for k in ("cam", "intr", "dist")))
    x = cuda(inp["imgs"][None])
    det = torch.empty((1, c["C"], 3), device="cuda")
    heat = torch.empty((1, c["C"], pr.Hh, pr.Hh, pr.Jp), device="cuda")
    pr.stage_center(x, det)
    pr.stage_keypoints(x, det, heat)
    torch.cuda.synchronize()
    return c, pred, pr, heat


def test_staged_equalities_where_both_gathers_are_the_row_form():
    c, pred, pr, heat = wide_rig()
    J, C = c["J"], c["C"]
    assert pr.Jp == 40
    plain = stage3(pr, heat, T=1)
    assert eq(stage3(pr, heat, joint_mask=np.ones((1, J, C), np.uint8), T=1), plain)
    m = np.array([[1, 0, 1, 1]], np.uint8)
    masked = stage3(pr, heat, camera_mask=m, T=1)
    assert not eq(masked, plain)
    assert eq(stage3(pr, heat, joint_mask=np.broadcast_to(m[:, None, :], (1, J, C)).copy(), T=1), masked)
    jm = batch_rows(1, J, C)
    e, n = R.effective_sets(jm)
    assert not eq(stage3(pr, heat, joint_mask=jm, T=1), plain)
    assert pr.joint_mask().cameras.cpu().tolist() == e.tolist()


# ---- 3: the consensus ---------------------------------------------------------------------------------------------------
def test_consensus_members_as_the_joint_mask_of_stage_3():
    c, pr, chm, calib64, heat = scene()
    J, C = c["J"], c["C"]
    heat = heat.copy()
    dark = 5
    assert dark != HJ.FALSE_PEAK[2]
    heat[:, :, :, :, dark] = 0.0                                  # a joint no camera sees: no members, the fallback
    p = HJ.jparams()
    obs = HJ.observations_of(heat, chm, J, pr.Hh, p.refine_radius)
    want = JR.triangulate_ref(obs, *calib64, False, max_error_px=HJ.MAX_ERR)[2]
    t, cam, j = HJ.FALSE_PEAK
    sizes = want.sum(-1)
    assert want[t, j].tolist() == [0 if k == cam else 1 for k in range(C)]       # exactly one camera left out
    assert (sizes[:, dark] == 0).all() and int((sizes == C).sum()) == 2 * J - 3  # empty rows, and all others full
    dev = cuda(torch.from_numpy(heat))
    tri = pr.triangulate_joints(heat=dev, params=p)
    assert tri.members.cpu().tolist() == want.tolist()
    got = stage3(pr, dev, joint_mask=tri.members.cpu().numpy())
    e, n = R.effective_sets(want)
    sets = pr.joint_mask()
    assert sets.cameras.cpu().tolist() == e.tolist() and sets.count.cpu().tolist() == n.tolist()
    assert e[:, dark].all() and n[t, j] == C - 1
    # the fallback written out gives the same bits, and the one camera left out moves the result
    assert eq(stage3(pr, dev, joint_mask=e), got)
    assert not same(stage3(pr, dev)[0][t], got[0][t])


def partial_share(cameras, C):
    n = cameras.sum(-1)
    return float(((n > 0) & (n < C)).float().mean())


@pytest.mark.parametrize("name,params", [("wide", HJ.WIDE), ("tight", dict(max_error_px=12.0, min_conf=0.0))])
def test_consensus_in_one_call_is_the_two_calls(name, params):
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, frames = HC.setup()
    J, C = c["J"], c["C"]
    x = cuda(frames[:3])
    centre = HC.detected(3)[1]["center3d"].clone()
    centre[1] = float("nan")                                     # frame set 1 is not valid
    plain = [t.clone() for t in pred.forward_batch(x, *calib, centers=centre)]
    first = pred.forward_batch(x, *calib, centers=centre, return_triangulated=params)
    members = first[3].members.clone()
    two = pred.forward_batch(x, *calib, centers=centre, joint_mask=members)
    two = [t.clone() for t in two[:3]] + [type(two[3])(*(t.clone() for t in two[3]))]
    one = pred.forward_batch(x, *calib, centers=centre, joint_mask=N.joints3d_params(**params))
    torch.cuda.synchronize()
    assert len(one) == 4 and type(one[3]).__name__ == "JointMask"
    assert all(same(a, b) for a, b in zip(one[:3], two[:3])) and one[2].tolist() == [1, 0, 1]
    assert same(one[3].cameras, two[3].cameras) and same(one[3].count, two[3].count)
    e, n = R.effective_sets(members.cpu().numpy())
    assert one[3].cameras.cpu().tolist() == e.tolist() and one[3].count.cpu().tolist() == n.tolist()
    # the invalid frame set has no members: it is as in the plain call, and so is its validity
    assert not members[1].any() and e[1].all()
    assert all(same(a[1], b[1]) for a, b in zip(one[:3], plain))
    report("joint_mask_consensus", params=name, partial_rows=partial_share(members.cpu()[[0, 2]], C),
           empty_rows=float((members.cpu()[[0, 2]].sum(-1) == 0).float().mean()))
    # a dict and 'consensus' are accepted like the struct
    d = pred.forward_batch(x, *calib, centers=centre, joint_mask=dict(params))
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(d[:3], one[:3]))


def test_whole_path_is_the_staged_composition():
    c, inp, pred, calib, frames = HC.setup()
    x = cuda(frames[:2])
    pr = HC.native(2)
    p = HJ.jparams(**HJ.WIDE)
    whole = pr.forward(x, joint_mask=p)
    whole = [t.clone() for t in whole[:3]] + [whole[3]]
    det = torch.empty((2, c["C"], 3), device="cuda")
    heat = torch.empty((2, c["C"], pr.Hh, pr.Hh, pr.Jp), device="cuda")
    pr.stage_center(x, det)
    pr.stage_keypoints(x, det, heat)
    tri = pr.triangulate_joints(heat=heat, params=p)
    got = stage3(pr, heat, joint_mask=tri.members.cpu().numpy())
    assert same(got[0], whole[0].cpu()) and same(got[1], whole[1].cpu())
    e, n = R.effective_sets(tri.members.cpu().numpy())
    assert whole[3].cameras.cpu().tolist() == e.tolist() and pr.joint_mask().count.cpu().tolist() == n.tolist()
    pr.close()


# ---- 4: graph replay ----------------------------------------------------------------------------------------------------
def test_graph_replay_keeps_its_bits_around_joint_masked_calls():
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, frames = HC.setup()
    J, C = c["J"], c["C"]
    x = cuda(frames[:1])
    g = HC.native(1)
    assert g.graph_replay
    bytes_before = N.lib().jh_predictor_device_bytes(g.handle)
    before = [t.clone() for t in g.forward(x)]
    jm = batch_rows(1, J, C)
    masked = []
    for _ in range(2):
        res = g.forward(x, joint_mask=jm)
        masked.append([t.clone() for t in res[:3]] + [res[3].cameras.clone()])
        after = [t.clone() for t in g.forward(x)]                 # (the replay again: the mode is off)
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(before, after))
    assert all(same(a, b) for a, b in zip(*masked)) and not same(masked[0][0], before[0])
    assert g.graph_replay and N.lib().jh_predictor_device_bytes(g.handle) == bytes_before
    # the single-frame form is row 0 of the batched one
    batch = pred.forward_batch(x, *calib, joint_mask=jm)
    batch = [t.clone() for t in batch[:3]] + [batch[3].cameras.clone()]
    single = pred(x[0], *calib, joint_mask=jm[0])
    torch.cuda.synchronize()
    assert len(single) == 3 and same(single[0], batch[0]) and same(single[1], batch[1])
    assert same(single[2].cameras, batch[3]) and tuple(single[2].count.shape) == (1, J)
    assert same(batch[0], masked[0][0]) and same(batch[3], masked[0][3])
    assert batch[3].cpu().tolist() == R.effective_sets(jm)[0].tolist()
    # invalid: None with the others; misuse raises before anything is enqueued
    assert pred(x[0], *calib, joint_mask=jm[0], centers=torch.full((3,), float("nan"))) == (None, None, None)
    for bad in ("members", jm[0, :, :3], torch.ones((1, J, C))):
        with pytest.raises(ValueError):
            pred.forward_batch(x, *calib, joint_mask=bad)
    with pytest.raises(RuntimeError, match="mode"):
        N.check(N.lib().jh_predictor_set_joint_mask(g.handle, 3, None, None, None))
    with pytest.raises(RuntimeError, match="needs a mask"):
        N.check(N.lib().jh_predictor_set_joint_mask(g.handle, N.JOINT_MASK_GIVEN, None, None, None))
    again = [t.clone() for t in g.forward(x)]
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(before, again))
    g.close()


# ---- 5: composition -----------------------------------------------------------------------------------------------------
MASK2 = np.array([[1, 1, 0, 1], [0, 1, 1, 1]], np.uint8)


def staged_pair(pr, x, J, C, det=True):
    """Stages 1 and 2 of x on pr, then stage 3 under MASK2 as a camera mask and as a uniform joint mask."""
    heat = torch.empty((2, C, pr.Hh, pr.Hh, pr.Jp), device="cuda")
    d = None
    if det:
        d = torch.empty((2, C, 3), device="cuda")
        pr.stage_center(x, d)
    pr.stage_keypoints(x, d, heat)
    return heat, stage3(pr, heat, camera_mask=MASK2), \
        stage3(pr, heat, joint_mask=np.broadcast_to(MASK2[:, None, :], (2, J, C)).copy())


def test_composes_with_centres():
    c, inp, pred, calib, frames = HC.setup()
    J, C = c["J"], c["C"]
    x = cuda(frames[:2])
    K = HC.detected(3)[1]["center3d"][:2].clone() + 3.0
    want = [t.clone() for t in pred.forward_batch(x, *calib, centers=K)]
    got = pred.forward_batch(x, *calib, centers=K, joint_mask=np.ones((2, J, C), np.uint8))
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(got[:3], want)) and want[2].tolist() == [1, 1]
    pr = HC.native(2)
    pr.set_centers(K)
    _, masked, rows = staged_pair(pr, x, J, C, det=False)
    assert eq(masked, rows)
    pr.close()


def test_composes_with_the_spread():
    c, inp, pred, calib, frames = HC.setup()
    J, C = c["J"], c["C"]
    x = cuda(frames[:2])
    want = pred.forward_batch(x, *calib, return_spread=True)
    want = [t.clone() for t in want[:3]] + [t.clone() for t in want[3]]
    got = pred.forward_batch(x, *calib, return_spread=True, joint_mask=np.ones((2, J, C), np.uint8))
    torch.cuda.synchronize()
    assert len(got) == 5 and type(got[3]).__name__ == "Spread3D" and type(got[4]).__name__ == "JointMask"
    assert all(same(a, b) for a, b in zip(list(got[:3]) + list(got[3]), want))
    pr = HC.native(2)
    pr.set_spread(True)
    heat, masked, _ = staged_pair(pr, x, J, C)
    sp_masked = [t.clone() for t in pr.spread()]
    rows = stage3(pr, heat, joint_mask=np.broadcast_to(MASK2[:, None, :], (2, J, C)).copy())
    sp_rows = pr.spread()
    torch.cuda.synchronize()
    assert eq(masked, rows) and all(same(a, b) for a, b in zip(sp_masked, sp_rows))
    pr.close()


def test_composes_with_per_frame_set_calibration():
    c, inp, pred, calib, frames = HC.setup()
    J, C = c["J"], c["C"]
    x = cuda(frames[:2])
    sets = {k: tuple(cuda(t) for t in v) for k, v in HC.derived_sets(*(inp[k] for k in HC.KEYS)).items()}
    per = tuple(torch.stack([sets[k][i] for k in "BD"]) for i in range(3))
    want = [t.clone() for t in pred.forward_batch(x, *per)]
    got = pred.forward_batch(x, *per, joint_mask=np.ones((2, J, C), np.uint8))
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(got[:3], want)) and want[2].tolist() == [1, 1]
    shared = pred.forward_batch(x, *calib, joint_mask=np.ones((2, J, C), np.uint8))
    torch.cuda.synchronize()
    assert not same(shared[0], got[0])                           # (the calibration is really read per row)
    pr = HC.native(2)
    pr.set_calibration_frames(*per)
    _, masked, rows = staged_pair(pr, x, J, C)
    assert eq(masked, rows)
    pr.close()


def test_forward_subjects_rows_are_centred_consensus_forwards():
    c, inp, pred, calib, frames = HC.setup()
    x = cuda(frames[:2])
    kw = dict(max_peaks=2, min_peak=-float("inf"), max_error_px=float("inf"))
    res = pred.forward_subjects(x, *calib, 2, joint_mask="consensus", **kw)
    torch.cuda.synchronize()
    assert len(res) == 5 and len(res[4]) == 2
    pts, conf, valid, subj = [t.clone() if torch.is_tensor(t) else t for t in res[:4]]
    used = [type(u)(*(t.clone() for t in u)) for u in res[4]]
    rows = 0
    for k in range(2):
        want = pred.forward_batch(x, *calib, centers=subj.centers[:, k], joint_mask="consensus")
        torch.cuda.synchronize()
        assert same(valid[:, k], want[2])
        for t in range(2):
            if int(valid[t, k]):
                assert same(pts[t, k], want[0][t]) and same(conf[t, k], want[1][t]), (t, k)
                assert same(used[k].cameras[t], want[3].cameras[t]) and same(used[k].count[t], want[3].count[t])
                rows += 1
    assert rows >= 2


# ---- 6: the driver ------------------------------------------------------------------------------------------------------
def test_driver_writes_joint_cameras_csv(tmp_path):
    from jarvis_hybridnet_amd.joint_mask import joint_cameras_row
    from jarvis_hybridnet_amd.prediction.predict3D import frame_row, predict3D_frames
    c, inp, pred, calib, frames = HC.setup()
    J = c["J"]
    cfg = HC.make_cfg(c)
    cfg.KEYPOINT_NAMES = ["joint%d" % j for j in range(J)]
    n = 9
    sets = [frames[t % 8].numpy() for t in range(n)]
    files = {}
    for streams in (1, 3):
        out = str(tmp_path / ("s%d" % streams))
        assert predict3D_frames(pred, iter(sets), *calib, cfg, out, time_batch=8, streams=streams,
                                joint_mask="consensus") == n
        files[streams] = tuple(open(os.path.join(out, name), "rb").read() for name in ("data3D.csv", "joint_cameras.csv"))
    assert files[1] == files[3]
    data = list(csv.reader(files[1][0].decode().splitlines()))
    cams = list(csv.reader(files[1][1].decode().splitlines()))
    assert len(data) == len(cams) == 2 + n and cams[1] == ["count", "cameras"] * J and cams[0][:3] == ["joint0"] * 2 + ["joint1"]
    res = pred.forward_batch(cuda(frames), *calib, joint_mask="consensus")
    torch.cuda.synchronize()
    pts, conf, valid = (t.cpu() for t in res[:3])
    used = type(res[3])(*(t.cpu() for t in res[3]))
    assert valid.tolist() == [1] * 8
    for k in range(n):
        t = k % 8
        assert data[2 + k] == [str(v) for v in frame_row(pts[t], conf[t], J)], k
        assert cams[2 + k] == [str(v) for v in joint_cameras_row(used.cameras[t].tolist(), used.count[t].tolist())], k
    report("joint_mask_driver", partial_rows=partial_share(used.cameras, c["C"]))
