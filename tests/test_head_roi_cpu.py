"""CPU: the keypoint head's box -- who gets one, and the box rule in numpy.

1. The dispatch rule (jh_head_roi_form -> conv_takes_box / head_box_allowed, csrc/conv_layer.hip): the
   head takes a box only in a whole-path forward whose voxel gather is the one reader of the heat maps, only as a layer
   of the window form, and never with JH_HEAD_ROI=0.  Pure host arithmetic; no kernel runs here.
2. tests/head_roi_ref.py, the numpy mirror the GPU tests use: the rule by hand, the window / tile arithmetic, and the
   conditions the box-against-gather geometries have to meet (no case whose boxes are all the full map, no empty box,
   the clamp case really clamps).
"""
import ctypes

import numpy as np
import pytest

from jarvis_hybridnet_amd import _native as N
from tests import head_roi_ref as R
from tests.test_native_abi import header_symbols

KNOBS = ("JH_HEAD_ROI", "JH_DECONV4_WINDOW")
FORWARD, STAGED, HYBRIDNET, CAPTURED = 0, 1, 2, 3


def takes_box(kind=FORWARD, consensus=False, sharded=False, res1=False, cin=64, cout=23, prec=0):
    out = ctypes.c_int32(-1)
    N.check(N.lib().jh_head_roi_form(kind, int(consensus), int(sharded), int(res1), cin, cout, prec, ctypes.byref(out)))
    assert out.value in (0, 1)
    return bool(out.value)


def test_symbols_in_header_and_ctypes_table():
    for name in ("jh_head_roi_form", "jh_op_deconv4_box", "jh_op_repro_box", "jh_predictor_debug_head_boxes"):
        assert name in header_symbols() and name in N.symbols() and hasattr(N.lib(), name), name


# call form -> box?
ROWS = [
    (dict(), {}, True),                                         # the benchmark's call: cfg3's head, 64 -> 23
    (dict(cin=32, cout=6), {}, True),                           # <2, 2>
    (dict(cin=88, cout=23), {}, True),                          # the medium model's head
    (dict(cin=160, cout=23), {}, True),                         # the large model's
    (dict(), {"JH_HEAD_ROI": "0"}, False),                      # the A/B arm
    (dict(), {"JH_HEAD_ROI": "1"}, True),
    (dict(), {"JH_DECONV4_WINDOW": "0"}, False),                # the four-parity kernel computes everything
    (dict(cout=30), {}, False),                                 # cfg5: J = 30 stays with the four parities
    (dict(cout=30), {"JH_DECONV4_WINDOW": "2"}, True),          # ... unless the measurement knob gives it the window form
    (dict(cout=40), {}, False),                                 # the general path
    (dict(cout=1), {}, False),                                  # a one-channel head (deconv_c1)
    (dict(prec=1), {}, False),                                  # the split-bf16 head
    (dict(kind=STAGED), {}, False),                             # heat_dev copy / the camera-sharded exchange
    (dict(kind=HYBRIDNET), {}, False),                          # heat maps exported to the caller
    (dict(consensus=True), {}, False),                          # the consensus scans whole heat maps
    (dict(kind=CAPTURED), {}, False),                           # the caller's graph replays it without the host code
    (dict(sharded=True), {}, False),
    (dict(res1=True), {}, False),
]


@pytest.mark.parametrize("call,env,want", ROWS)
def test_dispatch_rule(call, env, want, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert takes_box(**call) is want


def test_dispatch_rule_rejects_bad_arguments():
    out = ctypes.c_int32(0)
    f = N.lib().jh_head_roi_form
    assert f(4, 0, 0, 0, 64, 23, 0, ctypes.byref(out)) != 0
    assert f(0, 0, 0, 0, 0, 23, 0, ctypes.byref(out)) != 0
    assert f(0, 0, 0, 0, 64, 23, 3, ctypes.byref(out)) != 0
    assert f(0, 0, 0, 0, 64, 23, 0, None) != 0


# ---- the numpy mirror
def test_box_rule_by_hand():
    # heat_pad 0 (the predictor): stored pixel = trunc(u / 2) - 1, one pixel of margin on either side
    assert R.box_rule(40.0, 101.9, 63.9, 64.1, 128, 0) == (18, 29, 50, 32)
    # heat_pad 1 (the stand-alone reprojection operator): stored = padded
    assert R.box_rule(40.0, 101.9, 63.9, 64.1, 130, 1) == (19, 30, 51, 33)
    # clipped to the map at both ends; a field clamped to the crop's first / last pixel
    assert R.box_rule(0.0, 257.0, 0.0, 3.9, 128, 0) == (0, 0, 127, 1)
    # a degenerate field (every voxel clamped to one pixel) still gives a box that is not empty
    assert R.box_rule(0.0, 0.0, 257.0, 257.0, 128, 0) == (0, 126, 0, 127)


def test_window_and_tile_arithmetic():
    H, W = 24, 40
    assert R.all_workgroups(H, W) == (9, 1) and R.all_workgroups(64, 64) == (32, 2)
    whole = R.pixel_box(0, 0, W, H, H, W)
    assert whole == (0, 0, 2 * W - 1, 2 * H - 1) and R.workgroups(whole, H, W) == R.all_workgroups(H, W)
    b = R.pixel_box(5, 3, 20, 12, H, W)                    # windows [5..20] x [3..12], not tile-aligned
    assert b == (9, 5, 40, 24) and R.windows(b) == (5, 3, 20, 12)
    assert R.workgroups(b, H, W) == (2, 0)                 # 10 rows -> 2 tiles, 16 columns -> 1; no edge
    assert R.workgroups(R.pixel_box(7, 7, 7, 7, H, W), H, W) == (1, 0)
    assert R.workgroups(R.pixel_box(30, 20, W, H, H, W), H, W) == (1, 1)       # reaches the last row and column
    assert R.workgroups(R.pixel_box(0, 0, W - 1, H - 1, H, W), H, W) == (9, 0)  # all but the last row and column
    # every window of a box lies in one of its tiles, also where the last tile is clamped back into the image
    for box in (b, R.pixel_box(30, 20, W, H, H, W), R.pixel_box(33, 17, 38, 23, H, W)):
        wx_lo, wy_lo, wx_hi, wy_hi = R.windows(box)
        nt, _ = R.workgroups(box, H, W)
        covered = np.zeros((H, W), bool)
        tiles_x = -(-W // R.TILE_X)
        for unit in range(R.all_workgroups(H, W)[0]):
            wy0, wx0 = wy_lo + (unit // tiles_x) * R.TILE_Y, wx_lo + (unit % tiles_x) * R.TILE_X
            if wy0 > min(wy_hi, H - 1) or wx0 > min(wx_hi, W - 1):
                continue
            wy0, wx0 = min(wy0, max(H - R.TILE_Y, 0)), min(wx0, max(W - R.TILE_X, 0))
            covered[wy0:wy0 + R.TILE_Y, wx0:wx0 + R.TILE_X] = True
        assert covered[wy_lo:min(wy_hi, H - 1) + 1, wx_lo:min(wx_hi, W - 1) + 1].all()
        assert nt <= R.all_workgroups(H, W)[0]


@pytest.mark.parametrize("tag", sorted(R.GEOMETRIES))
def test_geometries_meet_their_conditions(tag):
    g = R.geometry(tag)
    b, fields = R.geometry_boxes(g)
    Hh = g["Hh"]
    assert b.shape == (g["T"], g["C"], 4)
    full = (b == np.asarray([0, 0, Hh - 1, Hh - 1])).all(-1)
    assert not full.all(), "a case whose boxes are all the full map checks nothing"
    assert (b[..., 0] <= b[..., 2]).all() and (b[..., 1] <= b[..., 3]).all(), "an empty box"
    assert (b >= 0).all() and (b <= Hh - 1).all()
    hit = sum(int((f[..., 0] <= 0).sum() + (f[..., 1] <= 0).sum() + (f >= 2 * g["hs"] - 3).sum()) for f in fields)
    if tag == "clamp":
        assert hit > 0, "the clamp case must have voxels outside the crop"
        assert (b[..., :2] == 0).any(), "... so a box touches the map's border"
    else:
        assert hit == 0
    if tag == "frames":
        assert g["T"] == 2 and not np.array_equal(g["cam"][0].numpy(), g["cam"][1].numpy())
        assert not np.array_equal(b[0], b[1])


def test_estimate_of_the_tile_fraction():
    """The issue's CPU estimate for the benchmark geometry (12 cameras 1280 x 1024, focal 1800, 128 mm cube, 64^3):
    boxes from the coarse hull cover roughly half the map and 0.6 - 0.85 of the 32 + 2 workgroups of an image."""
    import torch
    from jarvis_hybridnet_amd import synthetic as S
    cam, intr, dist = S.ring_calibration(12, 1280, 1024, 1800.0)
    rng = np.random.RandomState(5)
    area, wgs = [], []
    for _ in range(4):
        centre = rng.uniform(-100, 100, 3)
        uv = torch.from_numpy(S.project(centre[None], cam, intr, dist))[:, 0].int()
        uv[:, 0] = uv[:, 0].clamp(128, 1280 - 128)
        uv[:, 1] = uv[:, 1].clamp(128, 1024 - 128)
        f = R.coarse_field(cam.numpy(), intr.numpy(), dist.numpy(), centre.astype(np.int32), uv.numpy(), 64, 2, 130)
        for b in R.boxes(f, 128, 0):
            area.append((b[2] - b[0] + 1) * (b[3] - b[1] + 1) / 128.0 ** 2)
            wgs.append(sum(R.workgroups(b, 64, 64)) / 34.0)
    assert 0.4 < np.mean(area) < 0.7, np.mean(area)
    assert 0.55 < np.mean(wgs) < 0.9, np.mean(wgs)
