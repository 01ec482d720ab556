"""GPU: the keypoint head's box.

A whole-path forward whose voxel gather is the only reader of the heat maps projects the grid before stage 2, takes the
box of heat-map pixels each camera can be read at (csrc/reproject.hip: repro_box_kernel) and lets the window form of the
head's ConvTranspose2d compute only the tiles that cover it (csrc/deconv4.hip).  Three claims, all bit for bit:

1. the head op: inside its box an image holds exactly what the box-less launch writes, outside it nothing else is
   written (still NaN, or the box-less value); no box = the launch of before;
2. the box: every index the gather reports lies inside its camera's box or on the virtual border;
3. the predictor: points, confidences and validity do not depend on JH_HEAD_ROI, eagerly, under graph replay and with a
   camera mask; whoever reads whole heat maps after a boxed forward sees what a JH_HEAD_ROI=0 predictor shows.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import head_roi_ref as R
from tests.gpu_util import cuda

pytestmark = pytest.mark.gpu


# ---- 1. the head op ------------------------------------------------------------------------------------------------
def _head(x, w, boxes):
    """jh_op_deconv4_box: x (n, cin, h, w) -> y (n, cout, 2h, 2w) on the CPU; boxes (n, 4) pixel boxes or None.  The
    tensor the kernel stores into starts as NaN, and so does y."""
    from jarvis_hybridnet_amd import _native as N
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    xc = cuda(x)
    y = torch.full((n, cout, 2 * h, 2 * wd), float("nan"), device="cuda")
    wh = w.contiguous()
    bh = torch.tensor(boxes, dtype=torch.int32).contiguous() if boxes is not None else None
    N.check(N.lib().jh_op_deconv4_box(cin, cout, wh.data_ptr(), xc.data_ptr(), n, h, wd,
                                      bh.data_ptr() if bh is not None else None, y.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _window_boxes(H, W):
    """Six boxes in windows (x lo, y lo, x hi, y hi), clipped to the image's windows [0, W] x [0, H]."""
    raw = [(0, 0, W, H),                                   # the whole image, edge windows included
           (5, 3, 20, 12),                                 # not tile-aligned
           (0, 0, 9, 4),                                   # touching the origin
           (W - 5, H - 3, W, H),                           # reaching the last output row and column: edge workgroups run
           (7, 7, 7, 7),                                   # one window
           (W - 10, H - 7, W - 2, H - 1)]                  # the last tile starts 7 rows / 10 columns from the end: clamped
    return [(min(a, W), min(b, H), min(c, W), min(d, H)) for a, b, c, d in raw]


@functools.lru_cache(maxsize=None)
def _head_case(cin, J, H, W):
    g = torch.Generator().manual_seed(3 + cin + H)
    x = torch.randn(3, cin, H, W, generator=g)
    w = torch.randn(cin, J, 4, 4, generator=g) / (cin * 4) ** 0.5
    return x, w, _head(x, w, None)                          # the box-less launch of the same binary: the reference


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("H,W", [(16, 16), (24, 40)])
@pytest.mark.parametrize("cin,J", [(64, 23), (32, 6)])
def test_head_computes_its_box(cin, J, H, W, group, monkeypatch):
    monkeypatch.delenv("JH_DECONV4_WINDOW", raising=False)
    x, w, full = _head_case(cin, J, H, W)
    assert not torch.isnan(full).any()
    wins = _window_boxes(H, W)[3 * group:3 * group + 3]     # three images, a box each
    boxes = [R.pixel_box(*b, H, W) for b in wins]
    y = _head(x, w, boxes)
    for n, (x0, y0, x1, y1) in enumerate(boxes):
        assert 0 <= x0 <= x1 < 2 * W and 0 <= y0 <= y1 < 2 * H
        inside = torch.zeros(2 * H, 2 * W, dtype=torch.bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        assert torch.equal(y[n][:, inside], full[n][:, inside]), ("inside the box", wins[n])
        out, ref = y[n][:, ~inside], full[n][:, ~inside]
        assert bool((torch.isnan(out) | (out == ref)).all()), ("outside the box", wins[n])
        # what the box leaves out is really left out: only whole tiles around the box are computed
        n_tiles, n_edge = R.workgroups(boxes[n], H, W)
        if (n_tiles, n_edge) != R.all_workgroups(H, W):
            assert int(torch.isnan(y[n]).sum()) > 0, ("nothing was skipped", wins[n])
        written = ~torch.isnan(y[n][0])
        assert int(written.sum()) <= n_tiles * (2 * R.TILE_Y) * (2 * R.TILE_X) + n_edge * 2 * R.EDGE_WINDOWS


@pytest.mark.parametrize("cin,J,H,W", [(64, 23, 16, 16), (32, 6, 24, 40)])
def test_no_box_is_the_window_form_of_before(cin, J, H, W, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    monkeypatch.delenv("JH_DECONV4_WINDOW", raising=False)
    x, w, full = _head_case(cin, J, H, W)

    def op_conv():
        y = torch.full((3, J, 2 * H, 2 * W), float("nan"), device="cuda")
        before = N.lib().jh_deconv4_window_launches()
        N.check(N.lib().jh_op_conv(2, 1, 4, 2, 1, cin, J, w.contiguous().data_ptr(), None, cuda(x).data_ptr(), 3, 1, H,
                                   W, None, -1, y.data_ptr(), N.stream()))
        torch.cuda.synchronize()
        return y.cpu(), N.lib().jh_deconv4_window_launches() - before

    y_w, ran_w = op_conv()
    monkeypatch.setenv("JH_DECONV4_WINDOW", "0")
    y_p, ran_p = op_conv()
    assert ran_w == 1 and ran_p == 0
    assert torch.equal(full, y_w) and torch.equal(full, y_p)
    # ... and a layer of another form refuses a box instead of ignoring it silently
    with pytest.raises(RuntimeError, match="window form"):
        _head(x, w, [R.pixel_box(0, 0, W, H, H, W)] * 3)


# ---- 2. the box against the gather's indices -----------------------------------------------------------------------
def _repro_box(g, heat_pad, J=3, valid=None, mask=None):
    from jarvis_hybridnet_amd import _native as N
    T, C, G, hs = g["T"], g["C"], g["G"], g["hs"]
    dev = {k: cuda(g[k]) for k in ("cam", "intr", "dist", "center3d", "center_hm")}
    box = torch.full((T, C, 4), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((T, C, G ** 3), -7, dtype=torch.int32, device="cuda")
    vd = cuda(torch.tensor(valid, dtype=torch.int32)) if valid is not None else None
    md = cuda(torch.tensor(mask, dtype=torch.uint8)) if mask is not None else None
    N.check(N.lib().jh_op_repro_box(dev["cam"].data_ptr(), dev["intr"].data_ptr(), dev["dist"].data_ptr(), 1,
                                    dev["center3d"].data_ptr(), dev["center_hm"].data_ptr(), N.ptr(vd), N.ptr(md), T, C,
                                    J, hs, heat_pad, G, float(g["spacing"]), box.data_ptr(), idx.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    return box.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("heat_pad", [0, 1])
@pytest.mark.parametrize("tag", sorted(R.GEOMETRIES))
def test_gather_reads_inside_the_box(tag, heat_pad):
    g = R.geometry(tag)
    box, idx = _repro_box(g, heat_pad)
    hs, Hh = g["hs"], g["hs"] - 2 + 2 * heat_pad
    assert (idx >= 0).all() and (idx < hs * hs).all()
    full = (box == np.asarray([0, 0, Hh - 1, Hh - 1])).all(-1)
    assert not full.all(), "a case whose boxes are all the full map checks nothing"
    assert (box[..., 0] <= box[..., 2]).all() and (box[..., 1] <= box[..., 3]).all(), "an empty box"
    assert (box >= 0).all() and (box <= Hh - 1).all()
    # stored pixel of an index: padded (iu, iv) - 1 + heat_pad; outside the stored map = the virtual zero border
    hx, hy = idx % hs - 1 + heat_pad, idx // hs - 1 + heat_pad
    border = (hx < 0) | (hy < 0) | (hx >= Hh) | (hy >= Hh)
    b = box[:, :, None, :]
    inside = (hx >= b[..., 0]) & (hx <= b[..., 2]) & (hy >= b[..., 1]) & (hy <= b[..., 3])
    assert (inside | border).all(), "the gather reads a heat-map pixel outside its camera's box"
    # the box is no looser than its rule says: the pixels read span it up to the rule's margins (2 px a side: the one
    # pixel of margin, and one of the hull of the coarse field over the fine one)
    for t in range(g["T"]):
        for c in range(g["C"]):
            rd = ~border[t, c]
            assert rd.any()
            lo = np.asarray([hx[t, c][rd].min(), hy[t, c][rd].min()])
            hi = np.asarray([hx[t, c][rd].max(), hy[t, c][rd].max()])
            assert (lo - box[t, c, :2] <= 3).all() and (box[t, c, 2:] - hi <= 3).all(), (t, c, box[t, c], lo, hi)
    # ... and agrees with the numpy mirror up to the rounding of an fp32 field against a float64 one
    mirror, _ = R.geometry_boxes(g, heat_pad)
    assert np.abs(box - mirror).max() <= 1
    if tag == "clamp":
        assert border.any() or (box[..., :2] == 0).any()


def test_invalid_frames_and_masked_cameras_get_the_full_map():
    g = R.geometry("frames")
    ref, _ = _repro_box(g, 0)
    mask = [[1, 0, 1, 1], [1, 1, 1, 1]]
    box, idx = _repro_box(g, 0, valid=[1, 0], mask=mask)
    Hh = g["Hh"]
    full = np.asarray([0, 0, Hh - 1, Hh - 1])
    assert (box[1] == full).all() and (box[0, 1] == full).all()
    assert np.array_equal(box[0, [0, 2, 3]], ref[0, [0, 2, 3]])


# ---- 3. the predictor ----------------------------------------------------------------------------------------------
TAG = "cfg2"


@functools.lru_cache(maxsize=None)
def _setup():
    from jarvis_hybridnet_amd import synthetic as S
    c = cases.PREDICTOR_CASES[TAG]
    inp = cases.predictor_inputs(TAG)
    calib = tuple(inp[k] for k in ("cam", "intr", "dist"))
    other = S.blob_frames(calib, c["W"], c["H"], c["J"], c["fseed"] + 100)[0]
    a = cuda(torch.stack([inp["imgs"], other]))
    b = cuda(torch.stack([other, inp["imgs"]]).flip(-1).contiguous())       # other pictures: other heat maps
    return c, inp, tuple(cuda(t) for t in calib), a, b


@functools.lru_cache(maxsize=None)
def _native(roi):
    """The cfg2 predictor at T = 2, created with JH_HEAD_ROI unset (roi) or 0."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, calib, _, _ = _setup()
    old = os.environ.pop("JH_HEAD_ROI", None)
    if not roi:
        os.environ["JH_HEAD_ROI"] = "0"
    try:
        pr = NativePredictor(inp["sd_center"], inp["sd_hybrid"], num_cameras=c["C"], num_joints=c["J"],
                             center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
                             grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD, time_batch=2)
    finally:
        os.environ.pop("JH_HEAD_ROI", None)
        if old is not None:
            os.environ["JH_HEAD_ROI"] = old
    pr.set_calibration(*calib)
    return pr


def _boxes(pr):
    from jarvis_hybridnet_amd import _native as N
    box = torch.zeros((pr.T, pr.C, 4), dtype=torch.int32, device="cuda")
    boxed = ctypes.c_int32(-1)
    N.check(N.lib().jh_predictor_debug_head_boxes(pr.handle, box.data_ptr(), ctypes.byref(boxed), N.stream()))
    torch.cuda.synchronize()
    return box.cpu().numpy(), boxed.value


def _forward(pr, x, **kw):
    res = pr.forward(x, **kw)
    torch.cuda.synchronize()
    return [t.clone() for t in res[:3]]


def _same(got, want):
    return all(a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(got, want))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_forward_does_not_depend_on_the_box(graph, masked):
    c, inp, calib, a, b = _setup()
    on, off = _native(True), _native(False)
    mask = torch.tensor([[1, 1, 0, 1], [1, 1, 1, 1]], dtype=torch.bool) if masked else None
    for pr in (on, off):
        pr.graph_replay = graph
    try:
        want = _forward(off, a, camera_mask=mask)
        assert _boxes(off)[1] == 0
        assert want[2].tolist() == [1, 1], "the case must be valid, or stage 3 checks nothing"
        got = _forward(on, a, camera_mask=mask)
        box, boxed = _boxes(on)
        assert boxed == 1, "the default predictor's head did not take its box"
        Hh = c["bbox"] // 2
        full = (box == np.asarray([0, 0, Hh - 1, Hh - 1])).all(-1)
        assert not full.all() and (box[..., 0] <= box[..., 2]).all() and (box[..., 1] <= box[..., 3]).all()
        if masked:
            assert full[0, 2], "a masked camera keeps the full map"
        assert _same(got, want)
        # other frames in between (the heat maps outside the boxes now hold their pixels), then the first ones again:
        # a replay under graph replay
        _forward(on, b, camera_mask=mask)
        assert _same(_forward(on, a, camera_mask=mask), want)
    finally:
        for pr in (on, off):
            pr.graph_replay = False


def _variants(c, calib, pr_off, a):
    """Call forms the box is kept under, beyond mask and graph replay: name -> (prepare(pr), forward keywords)."""
    cam, intr, dist = calib
    dist2 = dist.clone()
    dist2[:, 0, 0:2] *= 0.5                                 # frame set 1: another lens (k1, k2 halved)
    frames = (torch.stack([cam, cam]), torch.stack([intr, intr]), torch.stack([dist, dist2]))
    jm = torch.ones((2, c["J"], c["C"]), dtype=torch.uint8)
    jm[0, ::2, 1] = 0                                       # every other joint of frame set 0 without camera 1
    jm[1, 3, :] = 0                                         # a joint without any camera: falls back
    _forward(pr_off, a)
    centres = pr_off.debug("cuda")["center3d"].clone() + torch.tensor([7.3, -4.6, 2.2], device="cuda")
    return {"calibration_frames": (lambda pr: pr.set_calibration_frames(*frames), {}),
            "joint_mask": (lambda pr: None, dict(joint_mask=jm)),
            "centres": (lambda pr: None, dict(centers=centres)),
            "center_keyframes": (lambda pr: None, dict(center_every=2))}


@pytest.mark.parametrize("name", ["calibration_frames", "joint_mask", "centres", "center_keyframes"])
def test_call_forms_that_keep_the_box(name):
    c, inp, calib, a, b = _setup()
    on, off = _native(True), _native(False)
    prepare, kw = _variants(c, calib, off, a)[name]
    try:
        for pr in (on, off):
            prepare(pr)
        want = _forward(off, a, **kw)
        assert _boxes(off)[1] == 0
        _forward(on, b, **kw)                               # other heat maps outside the boxes first
        got = _forward(on, a, **kw)
        box, boxed = _boxes(on)
        assert boxed == 1, "this call form keeps the head's box"
        Hh = c["bbox"] // 2
        assert not (box == np.asarray([0, 0, Hh - 1, Hh - 1])).all(-1).all()
        assert want[2].tolist() == [1, 1]
        assert _same(got, want)
    finally:
        for pr in (on, off):
            pr.set_calibration(*calib)
            _forward(pr, a)                                 # (clears the joint mask, the centres and the keyframes)


def test_consensus_keeps_the_full_map():
    """The joint-mask consensus scans whole heat maps between stage 2 and stage 3: no box, the same results."""
    c, inp, calib, a, b = _setup()
    on, off = _native(True), _native(False)
    try:
        want = _forward(off, a, joint_mask="consensus")
        _forward(on, b)
        assert _boxes(on)[1] == 1
        got = _forward(on, a, joint_mask="consensus")
        assert _boxes(on)[1] == 0
        assert _same(got, want)
    finally:
        for pr in (on, off):
            _forward(pr, a)


def _fresh(roi=True):
    from jarvis_hybridnet_amd._predictor import NativePredictor
    from jarvis_hybridnet_amd import synthetic as S
    c, inp, calib, _, _ = _setup()
    old = os.environ.pop("JH_HEAD_ROI", None)
    assert old is None
    if not roi:
        os.environ["JH_HEAD_ROI"] = "0"
    try:
        pr = NativePredictor(inp["sd_center"], inp["sd_hybrid"], num_cameras=c["C"], num_joints=c["J"],
                             center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
                             grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD, time_batch=2)
    finally:
        os.environ.pop("JH_HEAD_ROI", None)
    pr.set_calibration(*calib)
    return pr


def test_full_heat_maps_after_a_boxed_forward():
    """2D views read the predictor's own heat maps; the staged stage 2 hands heat maps to the caller.  Behind a boxed
    forward both give what a JH_HEAD_ROI=0 predictor gives -- nothing of the stale pixels outside the boxes -- and
    they do so every time, not only the first."""
    c, inp, calib, a, b = _setup()
    off = _native(False)
    on = _fresh()
    try:
        want = _forward(off, a)
        want_views = [t.clone() for t in off.views2d(want[0])]
        want_b = _forward(off, b)
        want_views_b = [t.clone() for t in off.views2d(want_b[0])]
        for x, w, wv in ((b, want_b, want_views_b), (a, want, want_views), (b, want_b, want_views_b)):
            got = _forward(on, x)
            assert _boxes(on)[1] == 1, "the forwards keep their box after a reader has come"
            got_views = [t.clone() for t in on.views2d(got[0])]
            torch.cuda.synchronize()
            assert _boxes(on)[1] == 0, "the heat maps were completed for their reader"
            assert _same(got, w) and _same(got_views, wv)
            # a second reader of the same maps finds them complete
            again = [t.clone() for t in on.views2d(got[0])]
            torch.cuda.synchronize()
            assert _same(again, wv)
        # the staged stage 2 writes whole heat maps for its caller, on either predictor
        _forward(on, b)
        heats = []
        for pr in (on, off):
            det = torch.zeros((2, c["C"], 3), device="cuda")
            heat = torch.full((2, c["C"], pr.Hh, pr.Hh, pr.Jp), float("nan"), device="cuda")
            pr.stage_center(a, det)
            pr.stage_keypoints(a, det, heat)
            torch.cuda.synchronize()
            heats.append(heat.clone())
        assert not torch.isnan(heats[0]).any() and torch.equal(heats[0], heats[1])
    finally:
        on.close()


def test_forward_captured_by_the_caller_keeps_the_full_map():
    """A forward inside the caller's stream capture runs again at every replay without the predictor's host code, so
    it never boxes the head: replay on other frames, 2D views, replay, 2D views again -- each equal to a JH_HEAD_ROI=0
    predictor's.  (With a boxed head inside the graph the second views2d would scan stale pixels.)"""
    c, inp, calib, a, b = _setup()
    off = _native(False)
    on = _fresh()
    try:
        want = {}
        for key, x in (("a", a), ("b", b)):
            res = _forward(off, x)
            want[key] = (res, [t.clone() for t in off.views2d(res[0])])
        x = a.clone()
        out = (torch.empty((2, c["J"], 3), device="cuda"), torch.empty((2, c["J"]), device="cuda"),
               torch.empty((2,), device="cuda", dtype=torch.int32))
        first = _forward(on, x)                             # eager and boxed first: allocations, and a boxed state
        assert _boxes(on)[1] == 1
        on.views2d(first[0])                                # (the views' workspace is allocated outside a capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            on.forward(x, out=out)
        assert _boxes(on)[1] == 0, "a forward the caller captures does not box the head"
        for key, frames in (("b", b), ("a", a), ("b", b)):
            x.copy_(frames)
            graph.replay()
            views = [t.clone() for t in on.views2d(out[0])]
            torch.cuda.synchronize()
            assert _same([t.clone() for t in out], want[key][0]), key
            assert _same(views, want[key][1]), key
        # an eager (boxed) forward between replays changes nothing for the replays' readers
        _forward(on, b)
        assert _boxes(on)[1] == 1
        x.copy_(a)
        graph.replay()
        views = [t.clone() for t in on.views2d(out[0])]
        torch.cuda.synchronize()
        assert _same(views, want["a"][1])
    finally:
        on.close()
