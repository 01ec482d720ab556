"""GPU: per-camera 2D views of the 3D predictor (jh_predictor_views2d) and the all-joint argmax behind them.
References, none of them the code under test: torch.argmax / torch.amax on the CPU copy of the same heat maps, the
crop centres of jh_predictor_debug, jh_reproject_point for the projections, torch arithmetic on the CPU for the
errors.  Every test here calls an entry point that a build without the feature does not have."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N
from tests import cases
from tests.gpu_util import cuda, report

pytestmark = pytest.mark.gpu

TAG = "cfg2"
FIELDS = ("points2D", "confidences2D", "reprojections", "errors", "used")


# ------------------------------------------------------------------------------------------------ the scan
def _planted(n, hh, wh, j, jp, seed):
    """randn heat maps with the edge cases planted, one per (image, joint) slot: the maximum at flat index 0 and at
    P-1; three equal maxima, two in neighbouring pixels (two lanes of one wave) and one near the end of the image
    (another row slice wherever the image has more than one); an all-equal map; an all-negative map; with room left,
    two equal maxima far apart on their own.  +1e30 in every padding channel.  -> heat, {slot: expected index}."""
    P = hh * wh
    g = torch.Generator().manual_seed(seed)
    heat = torch.randn(n, P, jp, generator=g)
    slots = [(i, c) for c in range(j) for i in range(n)]
    a, b = P // 3, P - 3
    want = {}

    def first(i, c): heat[i, 0, c] = 50.0; return 0
    def last(i, c): heat[i, P - 1, c] = 50.0; return P - 1
    def tie3(i, c): heat[i, [a, a + 1, b], c] = 60.0; return a
    def equal(i, c): heat[i, :, c] = 0.25; return 0
    def negative(i, c): heat[i, :, c] = -heat[i, :, c].abs() - 1.0; return int(heat[i, :, c].argmax())
    def tie_far(i, c): heat[i, [7, b], c] = 70.0; return 7
    kinds = [first, last, tie3, equal, negative, tie_far]
    assert len(slots) >= 5
    for kind, slot in zip(kinds, slots):
        want[slot] = kind(*slot)
    heat[:, :, j:] = 1e30
    return heat.reshape(n, hh, wh, jp).contiguous(), want


@pytest.mark.parametrize("n,hh,wh,j,jp", [(3, 20, 20, 23, 24), (2, 128, 128, 23, 24), (2, 160, 160, 30, 32),
                                          (5, 8, 8, 1, 8)])
def test_joint_argmax_all_vs_torch(n, hh, wh, j, jp):
    heat, want = _planted(n, hh, wh, j, jp, 1000 + hh + j)
    P = hh * wh
    flat = heat.reshape(n, P, jp)[:, :, :j]
    ref_idx, ref_max = flat.argmax(dim=1), flat.amax(dim=1)
    for (i, c), m in want.items():
        assert int(ref_idx[i, c]) == m                 # the plants are what the reference sees
    lib = N.lib()
    nbytes = lib.jh_joint_argmax_all_workspace_bytes(n, hh, wh, jp)
    assert nbytes > 0
    x = cuda(heat)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    idx = torch.full((n, j), -7, dtype=torch.int32, device="cuda")
    mx = torch.full((n, j), float("nan"), device="cuda")
    N.check(lib.jh_op_joint_argmax_all(N.ptr(x), n, hh, wh, j, jp, N.ptr(idx), N.ptr(mx), N.ptr(ws), nbytes, N.stream()))
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu().long(), ref_idx)
    assert torch.equal(mx.cpu(), ref_max)
    assert float(mx.max()) < 1e30                      # no padding channel in any output
    # a workspace that is too small is refused, not overrun
    assert lib.jh_op_joint_argmax_all(N.ptr(x), n, hh, wh, j, jp, N.ptr(idx), N.ptr(mx), N.ptr(ws), nbytes - 256,
                                      N.stream()) != 0


# ------------------------------------------------------------------------------------------- the predictor
def make_cfg(c):
    from jarvis_hybridnet_amd import synthetic as S
    return NS(PARENT_DIR="/nonexistent", PROJECT_NAME="none",
              DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
              CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center_size"]),
              KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
              HYBRIDNET=NS(NUM_CAMERAS=c["C"], ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))


@functools.lru_cache(maxsize=None)
def inputs():
    """The cfg2 rig, its weights and three frame sets (blob frames with known joints); CPU tensors, never changed."""
    from jarvis_hybridnet_amd import synthetic as S
    c = cases.PREDICTOR_CASES[TAG]
    inp = cases.predictor_inputs(TAG)
    calib = (inp["cam"], inp["intr"], inp["dist"])
    sets = [inp["imgs"]] + [S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"] + 100 * k)[0] for k in (1, 2)]
    return c, inp, calib, torch.stack(sets)


def native(T):
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, calib, _ = inputs()
    pr = NativePredictor(inp["sd_center"], inp["sd_hybrid"], num_cameras=c["C"], num_joints=c["J"],
                         center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
                         grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD, time_batch=T)
    pr.set_calibration(*(cuda(t) for t in calib))
    return pr


def staged(pr, frames, mask=None):
    """stage_center -> stage_keypoints -> stage_3d -> views2d(heat=...): the test owns the heat maps.  CPU copies."""
    c = cases.PREDICTOR_CASES[TAG]
    T, C, J = pr.T, c["C"], c["J"]
    det = torch.empty((T, C, 3), device="cuda")
    heat = torch.empty((T, C, pr.Hh, pr.Hh, pr.Jp), device="cuda")
    pts, conf = torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda")
    valid = torch.empty((T,), device="cuda", dtype=torch.int32)
    pr.stage_center(frames, det)
    pr.stage_keypoints(frames, det, heat, camera_mask=mask)
    pr.stage_3d(heat, 0, pts, conf, valid, camera_mask=mask)
    views = pr.views2d(pts, heat=heat, camera_mask=mask)
    chm = pr.debug("cuda")["center_hm"]
    torch.cuda.synchronize()
    return dict(heat=heat.cpu(), points=pts.cpu(), conf=conf.cpu(), valid=valid.cpu(), center_hm=chm.cpu(),
                views=type(views)(*(t.cpu() for t in views)))


def reproject(points):
    """jh_reproject_point of points (T,J,3) in every camera -> (T,C,J,2) on the CPU."""
    c, _, calib, _ = inputs()
    dev = [cuda(t) for t in calib]
    out = []
    for p in points:
        uv = torch.empty((c["C"], p.shape[0], 2), device="cuda")
        N.check(N.lib().jh_reproject_point(N.ptr(cuda(p)), p.shape[0], c["C"], N.ptr(dev[0]), N.ptr(dev[1]),
                                           N.ptr(dev[2]), N.ptr(uv), N.stream()))
        out.append(uv)
    torch.cuda.synchronize()
    return torch.stack(out).cpu()


def torch_reference(run):
    """points2D, confidences2D from the heat maps and crop centres with torch on the CPU; errors from them and the
    given reprojections."""
    c = cases.PREDICTOR_CASES[TAG]
    J, Hh = c["J"], c["bbox"] // 2
    heat = run["heat"][..., :J]
    T, C = heat.shape[:2]
    flat = heat.reshape(T, C, Hh * Hh, J)
    m, mx = flat.argmax(dim=2), flat.amax(dim=2)
    chm = run["center_hm"].long()
    p2d = torch.stack([(m % Hh) * 2 + chm[..., 0:1] - c["bbox"] // 2, (m // Hh) * 2 + chm[..., 1:2] - c["bbox"] // 2], -1)
    conf = torch.clamp(mx, max=255) / 255
    return p2d, conf


def check_errors(errors, reproj, p2d, where):
    """errors == sqrt(dx*dx + dy*dy) in fp32 on the CPU, to 1 ulp, where `where` (T,C) is set."""
    d = reproj - p2d.float()
    ref = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    lo, hi = torch.nextafter(ref, torch.full_like(ref, -1.0)), torch.nextafter(ref, torch.full_like(ref, float("inf")))
    ok = (errors >= lo) & (errors <= hi)
    assert bool(ok[where].all())


@functools.lru_cache(maxsize=None)
def base():
    """Frame sets 0 and 1 through the staged calls at T = 2, computed once and shared (never changed)."""
    _, _, _, sets = inputs()
    return staged(native(2), cuda(sets[:2]))


def test_views2d_staged_vs_torch():
    c, inp, _, _ = inputs()
    run = base()
    v = run["views"]
    assert run["valid"].tolist() == [1, 1] and v.used.tolist() == [[1] * c["C"]] * 2
    p2d, conf = torch_reference(run)
    assert torch.equal(v.points2D.long(), p2d)
    assert torch.equal(v.confidences2D, conf)
    ref_uv = reproject(run["points"])
    assert torch.equal(v.reprojections, ref_uv)
    assert (v.reprojections.view(torch.int32) == ref_uv.view(torch.int32)).all()
    check_errors(v.errors, ref_uv, p2d, v.used.bool())
    # the blob frames show a subject inside every camera's frame: so do the projected 3D keypoints
    u, w = v.reprojections[..., 0], v.reprojections[..., 1]
    assert bool(((u >= 0) & (u < c["W"]) & (w >= 0) & (w < c["H"])).all())
    med = float(v.errors.median())
    report("views2d_reprojection_error", tag=TAG, median_px=med, max_px=float(v.errors.max()),
           median_conf2d=float(v.confidences2D.median()))
    print("views2d: median reprojection error %.3g px, max %.3g px" % (med, float(v.errors.max())))


def _same(views, ref, t_got, t_ref):
    for name in FIELDS:
        a, b = getattr(views, name)[t_got].cpu(), getattr(ref, name)[t_ref]
        if a.is_floating_point():
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name      # bits: NaN rows included
        else:
            assert torch.equal(a, b), name


def test_whole_path_forms_equal_the_staged_values():
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c, inp, calib, sets = inputs()
    ref = base()
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    dev = [cuda(t) for t in calib]
    # T = 1, graph replay on: forward and forward_batch, then other frames on the same predictor
    for t in (0, 1, 0):
        plain = pred(cuda(sets[t]), *dev)
        pts, conf, views = pred(cuda(sets[t]), *dev, return_2d=True)
        assert torch.equal(pts, plain[0]) and torch.equal(conf, plain[1])
        assert torch.equal(pts[0].cpu(), ref["points"][t])
        assert views.points2D.shape == (1, c["C"], c["J"], 2) and views.used.shape == (1, c["C"])
        _same(views, ref["views"], 0, t)
        bp, bc, bv, bviews = pred.forward_batch(cuda(sets[t:t + 1]), *dev, return_2d=True)
        assert int(bv[0]) == 1 and torch.equal(bp, pts) and torch.equal(bc, conf)
        _same(bviews, ref["views"], 0, t)
    assert pred.native(c["H"], c["W"]).graph_replay
    assert N.lib().jh_predictor_graph_replay(pred.native(c["H"], c["W"]).handle) == 1
    # T = 2: both rows; then the frame sets in the other order
    for order in ([0, 1], [1, 0]):
        x = cuda(sets[order])
        plain = [t.clone() for t in pred.forward_batch(x, *dev)]
        bp, bc, bv, bviews = pred.forward_batch(x, *dev, return_2d=True)
        assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, (bp, bc, bv)))
        for row, t in enumerate(order):
            assert torch.equal(bp[row].cpu(), ref["points"][t])
            _same(bviews, ref["views"], row, t)
    assert not pred.native(c["H"], c["W"], time_batch=2).graph_replay


def test_masks_and_invalid_frames():
    """T = 2.  Frame 0: camera 2 masked, its frame slot NaN.  Frame 1: three cameras masked -- an invalid frame."""
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c, inp, calib, sets = inputs()
    C, J = c["C"], c["J"]
    frames = sets[:2].clone()
    frames[0, 2] = float("nan")
    mask = torch.tensor([[1, 1, 0, 1], [0, 0, 0, 1]], dtype=torch.uint8)
    run = staged(native(2), cuda(frames), cuda(mask))
    v = run["views"]
    assert run["valid"].tolist() == [1, 0]
    assert v.used.tolist() == [[1, 1, 0, 1], [0, 0, 0, 0]]
    p2d, conf = torch_reference(run)
    ref_uv = reproject(run["points"][:1])[0]
    on = [0, 1, 3]
    assert torch.equal(v.points2D[0, on].long(), p2d[0, on]) and torch.equal(v.confidences2D[0, on], conf[0, on])
    # the masked camera of the valid frame: no 2D detection, but its calibration still says where the joints are
    assert bool((v.points2D[0, 2] == -1).all()) and bool((v.confidences2D[0, 2] == 0).all())
    assert bool(v.errors[0, 2].isnan().all())
    assert bool(v.reprojections[0].isfinite().all()) and torch.equal(v.reprojections[0], ref_uv)
    check_errors(v.errors, v.reprojections, p2d, v.used.bool())
    assert bool(v.errors[0, on].isfinite().all())
    # the invalid frame
    assert bool(v.reprojections[1].isnan().all()) and bool(v.errors[1].isnan().all())
    assert bool((v.points2D[1] == -1).all()) and bool((v.confidences2D[1] == 0).all())
    # the whole-path form with the same mask gives the same views; so does the single-frame form
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    dev = [cuda(t) for t in calib]
    bp, bc, bv, bviews = pred.forward_batch(cuda(frames), *dev, camera_mask=mask, return_2d=True)
    assert bv.tolist() == [1, 0]
    for t in (0, 1):
        _same(bviews, v, t, t)
    pts, conf1, views = pred(cuda(frames[0]), *dev, camera_mask=mask[0], return_2d=True)
    _same(views, v, 0, 0)
    assert pred(cuda(frames[1]), *dev, camera_mask=mask[1], return_2d=True) == (None, None, None)


def test_driver_output_2d(tmp_path):
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, calib, sets = inputs()
    C, J = c["C"], c["J"]
    u8 = [(f.permute(0, 2, 3, 1)[..., [2, 1, 0]] * 255).round().to(torch.uint8).contiguous() for f in sets]
    masks = [None, [1, 1, 0, 1], None]
    pred = JarvisPredictor3D(make_cfg(c), inp["sd_center"], inp["sd_hybrid"])
    dev = [cuda(t) for t in calib]

    def run(name, **kw):
        out = tmp_path / name
        n = predict3D_frames(pred, [f.numpy() for f in u8], *dev, make_cfg(c), str(out), time_batch=2,
                             camera_mask=iter(masks), **kw)
        assert n == 3
        return out

    plain, with2d = run("plain"), run("with2d", output_2d=True)
    assert (plain / "data3D.csv").read_bytes() == (with2d / "data3D.csv").read_bytes()
    assert sorted(p.name for p in with2d.iterdir()) == ["data2D_Camera_%d.csv" % i for i in range(C)] + [
        "data3D.csv", "reprojection_error.csv"]
    # the same frame sets through forward_batch: batch 0 = sets 0, 1; batch 1 = set 2 padded with itself
    rows2d, rows_err, rows_used = [], [], []
    for x, m in ((torch.stack(u8[:2]), [[1] * C, masks[1]]), (torch.stack([u8[2], u8[2]]), None)):
        views = pred.forward_batch(cuda(x), *dev, camera_mask=m, return_2d=True)[3]
        for t in range(2 if m else 1):
            rows2d.append((views.points2D[t].cpu(), views.confidences2D[t].cpu()))
            rows_err.append(views.errors[t].cpu())
            rows_used.append(views.used[t].cpu().tolist())
    assert rows_used[0] == [1] * C and rows_used[1] == [1, 1, 0, 1]
    for cam in range(C):
        rows = (with2d / ("data2D_Camera_%d.csv" % cam)).read_text().splitlines()
        assert len(rows) == 3
        for k, r in enumerate(rows):
            cells = r.split(",")
            assert len(cells) == 3 * J
            if not rows_used[k][cam]:
                assert cells == ["NaN"] * (3 * J)
                continue
            p, q = rows2d[k]
            assert [int(v) for v in cells[0::3]] == p[cam, :, 0].tolist()
            assert [int(v) for v in cells[1::3]] == p[cam, :, 1].tolist()
            assert [np.float32(v) for v in cells[2::3]] == list(q[cam].numpy())
    assert (with2d / "data2D_Camera_2.csv").read_text().splitlines()[1] == ",".join(["NaN"] * (3 * J))
    rows = (with2d / "reprojection_error.csv").read_text().splitlines()
    assert len(rows) == 3
    for k, r in enumerate(rows):
        cells = r.split(",")
        want = rows_err[k].reshape(-1).numpy()
        assert len(cells) == C * J
        for cell, w in zip(cells, want):
            assert (cell == "NaN") if np.isnan(w) else (np.float32(cell) == w)
        nan_cams = [cam for cam in range(C) if all(cell == "NaN" for cell in cells[cam * J:(cam + 1) * J])]
        assert nan_cams == [cam for cam in range(C) if not rows_used[k][cam]]
