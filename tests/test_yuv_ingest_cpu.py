"""CPU: YUV 4:2:0 ingest (I420 / NV12) on the host side -- the numpy reference of the conversion contract
(BT.601 limited range, fixed-point arithmetic of OpenCV's cvtColor COLOR_YUV2BGR_I420 / _NV12), the frame
layouts, and the drivers' handling of the `frame_format` argument with stub predictors.  No compute call."""
import csv
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20
HALF = 1 << (SHIFT - 1)


def yuv420_to_bgr(frames, fmt):
    """(..., 3H/2, W) uint8 YUV 4:2:0 in layout `fmt` ('i420' | 'nv12') -> (..., H, W, 3) uint8 BGR, written from
    the contract: u = U - 128, v = V - 128, yy = max(0, Y - 16) * CY, channel = clamp((yy + HALF + ...) >> 20),
    chroma of pixel (y, x) at (y/2, x/2)."""
    f = np.asarray(frames, np.uint8)
    lead, rows, W = f.shape[:-2], f.shape[-2], f.shape[-1]
    H = rows // 3 * 2
    Y = f[..., :H, :].astype(np.int64)
    c = f[..., H:, :]
    if fmt == "i420":
        flat = c.reshape(lead + (-1,))
        U = flat[..., :H * W // 4].reshape(lead + (H // 2, W // 2))
        V = flat[..., H * W // 4:].reshape(lead + (H // 2, W // 2))
    elif fmt == "nv12":
        U, V = c[..., 0::2], c[..., 1::2]
    else:
        raise ValueError(fmt)
    u = np.repeat(np.repeat(U.astype(np.int64) - 128, 2, -2), 2, -1)
    v = np.repeat(np.repeat(V.astype(np.int64) - 128, 2, -2), 2, -1)
    yy = np.maximum(Y - 16, 0) * CY + HALF
    for t in (yy + CVR * v, yy + CVG * v + CUG * u, yy + CUB * u):
        assert np.abs(t).max() < (1 << 30)                      # int32 arithmetic in the kernels: no overflow
    r = np.clip((yy + CVR * v) >> SHIFT, 0, 255)
    g = np.clip((yy + CVG * v + CUG * u) >> SHIFT, 0, 255)
    b = np.clip((yy + CUB * u) >> SHIFT, 0, 255)
    return np.stack([b, g, r], -1).astype(np.uint8)


def planes(y, u, v, fmt):
    from jarvis_hybridnet_amd.synthetic import pack_yuv420
    return pack_yuv420(y, u, v, fmt)


def test_grey_and_extreme_values():
    H, W = 4, 6
    u = np.full((H // 2, W // 2), 128, np.uint8)
    for Y, want in ((16, 0), (0, 0), (235, 255), (255, 255)):
        for fmt in ("i420", "nv12"):
            out = yuv420_to_bgr(planes(np.full((H, W), Y, np.uint8), u, u, fmt), fmt)
            assert out.shape == (H, W, 3) and (out == want).all(), (Y, fmt)
    # neutral chroma: grey, monotone in Y, the BT.601 luma scale 255 / 219
    ys = np.arange(256, dtype=np.uint8).reshape(16, 16)
    out = yuv420_to_bgr(planes(ys, np.full((8, 8), 128, np.uint8), np.full((8, 8), 128, np.uint8), "i420"), "i420")
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()
    grey = out[..., 0].reshape(-1).astype(int)
    assert (np.diff(grey) >= 0).all()
    assert np.abs(grey - np.clip(np.round((np.arange(256) - 16) * 255.0 / 219.0), 0, 255)).max() <= 1
    # clamping at both ends: full blue / red chroma on black and white luma
    lo = np.full((2, 2), 16, np.uint8)
    hi = np.full((2, 2), 235, np.uint8)
    one = lambda x: np.full((1, 1), x, np.uint8)  # noqa: E731
    b = yuv420_to_bgr(planes(lo, one(0), one(0), "i420"), "i420")[0, 0]       # U = V = 0 on black
    assert b[0] == 0 and b[2] == 0 and b[1] > 100                               # B, R clamp low; G high
    w = yuv420_to_bgr(planes(hi, one(255), one(255), "i420"), "i420")[0, 0]   # U = V = 255 on white
    assert w[0] == 255 and w[2] == 255 and w[1] < 200


def test_against_floating_point_bt601():
    """The fixed-point constants are BT.601 limited range: within 1 of the real-valued matrix everywhere."""
    g = np.random.default_rng(3)
    Y = g.integers(0, 256, (64, 64), dtype=np.uint8)
    U = g.integers(0, 256, (32, 32), dtype=np.uint8)
    V = g.integers(0, 256, (32, 32), dtype=np.uint8)
    out = yuv420_to_bgr(planes(Y, U, V, "nv12"), "nv12").astype(np.float64)
    yf = np.maximum(Y.astype(np.float64) - 16, 0) * 255.0 / 219.0
    uf = np.repeat(np.repeat(U.astype(np.float64) - 128, 2, 0), 2, 1) * 255.0 / 224.0
    vf = np.repeat(np.repeat(V.astype(np.float64) - 128, 2, 0), 2, 1) * 255.0 / 224.0
    r = yf + 1.402 * vf
    gg = yf - 0.344136 * uf - 0.714136 * vf
    b = yf + 1.772 * uf
    for k, ref in ((0, b), (1, gg), (2, r)):
        assert np.abs(out[..., k] - np.clip(ref, 0, 255)).max() <= 1.0 + 1e-9


def test_i420_and_nv12_agree():
    g = np.random.default_rng(5)
    Y = g.integers(0, 256, (3, 2, 8, 10), dtype=np.uint8)
    U = g.integers(0, 256, (3, 2, 4, 5), dtype=np.uint8)
    V = g.integers(0, 256, (3, 2, 4, 5), dtype=np.uint8)
    a, b = planes(Y, U, V, "i420"), planes(Y, U, V, "nv12")
    assert a.shape == b.shape == (3, 2, 12, 10) and not np.array_equal(a, b)
    ba, bb = yuv420_to_bgr(a, "i420"), yuv420_to_bgr(b, "nv12")
    assert ba.shape == (3, 2, 8, 10, 3) and np.array_equal(ba, bb)
    # the 2 x 2 blocks share their chroma: pixels with equal Y inside a block are equal
    Y2 = np.repeat(np.repeat(Y[..., ::2, ::2], 2, -2), 2, -1)
    out = yuv420_to_bgr(planes(Y2, U, V, "i420"), "i420")
    assert (out[..., 0::2, :, :] == out[..., 1::2, :, :]).all() and (out[..., 0::2, :] == out[..., 1::2, :]).all()


def test_forward_transform_round_trip():
    """synthetic.bgr_to_yuv420 (the test data's forward BT.601) is close to the contract's inverse on smooth images."""
    from jarvis_hybridnet_amd import synthetic as S
    yy, xx = np.meshgrid(np.arange(32), np.arange(48), indexing="ij")
    bgr = np.stack([40 + 4 * xx, 60 + 3 * yy, 200 - 2 * xx - yy], -1).clip(0, 255).astype(np.uint8)
    for fmt in ("i420", "nv12"):
        yuv = S.bgr_to_yuv420(bgr, fmt)
        assert yuv.shape == (48, 48) and yuv.dtype == np.uint8
        assert np.abs(yuv420_to_bgr(yuv, fmt).astype(int) - bgr).max() <= 8


def test_matches_cv2_cvtcolor():
    cv2 = pytest.importorskip("cv2")
    g = np.random.default_rng(7)
    for H, W in ((4, 6), (64, 96), (30, 42)):
        for fmt, code in (("i420", cv2.COLOR_YUV2BGR_I420), ("nv12", cv2.COLOR_YUV2BGR_NV12)):
            yuv = g.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
            assert np.array_equal(yuv420_to_bgr(yuv, fmt), cv2.cvtColor(yuv, code)), (H, W, fmt)


def test_frame_format_names():
    from jarvis_hybridnet_amd import _native as N
    def hw(shape, fmt="i420"):
        d = N.describe_shape(shape, torch.uint8, (None,) * (len(shape) - 2), fmt)
        return d.height, d.width
    assert N.describe_shape((4, 6, 3), torch.uint8, (), None).fmt == 1 and hw((12, 10), "i420") == (8, 10)
    assert N.FRAME_FORMATS == {"bgr": 1, "i420": 2, "nv12": 3}
    for bad in ("I420", "yuv420p", "rgb", 2):
        with pytest.raises(ValueError):
            hw((12, 10), bad)
    assert hw((12, 10)) == (8, 10) and hw((2, 3, 1536, 1280)) == (1024, 1280)
    for bad in ((7, 10), (12, 9), (0, 4)):
        with pytest.raises(ValueError):
            hw(bad)
    # the C ABI's codes (include/jarvis_hip.h)
    import re
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    text = open(os.path.join(root, "include", "jarvis_hip.h")).read()
    codes = dict(re.findall(r"#define JH_FRAME_(\w+) (\d+)", text))
    assert codes == {"RGB_F32": "0", "BGR_U8": "1", "I420": "2", "NV12": "3"}


class Stub3D:
    """points = first byte of the frame set + joint index; frame sets whose first byte is 255 are `not detected`;
    records the frame_format of every call"""
    J = 3

    def __init__(self):
        self.formats, self.shapes = [], []

    def forward_batch(self, x, *calib, frame_format=None):
        self.formats.append(frame_format)
        self.shapes.append(tuple(x.shape))
        ids = x.reshape(x.shape[0], -1)[:, 0].float()
        pts = ids[:, None, None] + torch.arange(self.J).float()[None, :, None] + torch.zeros(1, 1, 3)
        return pts, torch.full((x.shape[0], self.J), 0.5), (ids != 255).int()


def _rows(path, name="data3D.csv"):
    return list(csv.reader(open(os.path.join(path, name))))[2:]


def test_predict3D_frames_yuv_host_logic(tmp_path):
    """YUV frame sets (C, 3H/2, W) through the driver's staging pipeline: rows in frame order with a short last
    time batch, the format handed to the predictor, fill callables with frame_spec, ValueError for an unknown
    format and for frame sets that cannot be 4:2:0 with even H and W."""
    from jarvis_hybridnet_amd.prediction import predict3D as P
    C, H, W, J = 2, 4, 6, 3
    cfg = NS(KEYPOINT_NAMES=["a", "b", "c"], KEYPOINTDETECT=NS(NUM_JOINTS=J))
    sets = [np.full((C, H * 3 // 2, W), 255 if i == 2 else i, np.uint8) for i in range(7)]
    for fmt in ("i420", "nv12"):
        for tb, st in ((1, 1), (3, 2), (4, 1)):
            pred = Stub3D()
            out = str(tmp_path / ("%s_%d_%d" % (fmt, tb, st)))
            assert P.predict3D_frames(pred, iter(sets), None, None, None, cfg, out, time_batch=tb, streams=st,
                                      frame_format=fmt) == 7
            got = _rows(out)
            assert len(got) == 7 and got[2] == ["NaN"] * (4 * J)
            assert [float(r[0]) for i, r in enumerate(got) if i != 2] == [0.0, 1.0, 3.0, 4.0, 5.0, 6.0]
            assert set(pred.formats) == {fmt} and set(pred.shapes) == {(tb, C, H * 3 // 2, W)}
            assert len(pred.formats) == -(-7 // tb)
    # fill callables decode in place into the (C, 3H/2, W) staging buffer
    pred = Stub3D()
    fills = [(lambda dst, i=i: dst.fill(i)) for i in (4, 5, 6)]
    out = str(tmp_path / "fill")
    assert P.predict3D_frames(pred, fills, None, None, None, cfg, out, time_batch=2, frame_format="nv12",
                              frame_spec=((C, H * 3 // 2, W), torch.uint8)) == 3
    assert [r[0] for r in _rows(out)] == ["4.0", "5.0", "6.0"] and pred.formats == ["nv12", "nv12"]
    # the default stays the BGR behaviour: no frame_format reaches a predictor that does not know the argument
    pred = Stub3D()
    bgr = [np.full((C, H, W, 3), i, np.uint8) for i in range(3)]
    assert P.predict3D_frames(pred, bgr, None, None, None, cfg, str(tmp_path / "bgr"), time_batch=2) == 3
    assert pred.formats == [None, None]
    # errors before anything is written or run
    for bad in ("yuv420p", "I420", "rgb"):
        with pytest.raises(ValueError, match="frame_format"):
            P.predict3D_frames(Stub3D(), sets, None, None, None, cfg, str(tmp_path / "bad"), frame_format=bad)
    assert not os.path.exists(tmp_path / "bad")
    for shape in ((C, 7, W), (C, 6, 5), (C, H, W, 3)):                 # odd H (3H/2 no integer), odd W, BGR bytes
        pred = Stub3D()
        with pytest.raises(ValueError):
            P.predict3D_frames(pred, [np.zeros(shape, np.uint8)], None, None, None, cfg, str(tmp_path / "odd"),
                               frame_format="i420")
        assert pred.formats == []
    with pytest.raises(ValueError):
        P.predict3D_frames(Stub3D(), [np.zeros((C, 6, W), np.float32)], None, None, None, cfg,
                           str(tmp_path / "f32"), frame_format="i420")
    for spec in (((C, 7, W), torch.uint8), ((C, 6, 5), torch.uint8), ((C, 6, W), torch.float32)):
        with pytest.raises(ValueError):
            P.predict3D_frames(Stub3D(), fills, None, None, None, cfg, str(tmp_path / "spec"), frame_format="i420",
                               frame_spec=spec)


def test_predict2D_frames_yuv_host_logic(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict2D as P
    J = 2
    cfg = NS(KEYPOINT_NAMES=["a", "b"], KEYPOINTDETECT=NS(NUM_JOINTS=J))

    class Stub2D:
        def __init__(self):
            self.formats = []

        def forward_batch(self, x, frame_format=None):
            self.formats.append(frame_format)
            ids = x.reshape(x.shape[0], -1)[:, 0].int()
            pts = ids[:, None, None] + torch.zeros(1, J, 2, dtype=torch.int32)
            return pts, torch.full((x.shape[0], J), 0.25), (ids != 255).int()

    frames = [np.full((6, 4), 255 if i == 1 else i, np.uint8) for i in range(5)]
    for fmt in ("i420", "nv12"):
        pred = Stub2D()
        out = tmp_path / fmt
        assert P.predict2D_frames(pred, frames, cfg, str(out), time_batch=2, frame_format=fmt) == 5
        rows = _rows(out, "data2D.csv")
        assert [r[0] for r in rows] == ["0", "NaN", "2", "3", "4"] and pred.formats == [fmt] * 3
    pred = Stub2D()
    fills = [(lambda dst, i=i: dst.fill(i)) for i in (7, 8, 9)]
    assert P.predict2D_frames(pred, fills, cfg, str(tmp_path / "fill"), time_batch=2, frame_format="i420",
                              frame_spec=((6, 4), torch.uint8)) == 3
    assert [r[0] for r in _rows(tmp_path / "fill", "data2D.csv")] == ["7", "8", "9"]
    with pytest.raises(ValueError, match="frame_format"):
        P.predict2D_frames(Stub2D(), frames, cfg, str(tmp_path / "bad"), frame_format="yv12")
    for shape in ((7, 4), (6, 3)):
        with pytest.raises(ValueError):
            P.predict2D_frames(Stub2D(), [np.zeros(shape, np.uint8)], cfg, str(tmp_path / "odd"),
                               frame_format="nv12")


def test_predictor_entry_points_refuse_bad_yuv_arguments():
    """The public forms validate format, dtype and shape before anything reaches the GPU (no GPU needed: the
    checks run first)."""
    from jarvis_hybridnet_amd.distributed import ShardedPredictor
    from jarvis_hybridnet_amd import _native as N

    def _yuv_frames(frames, frame_format, ndim):            # (forward_yuv's check of a (C, 3H/2, W) frame set)
        assert ndim == 3
        return N.describe_frames(frames, (2,), N.yuv_format(frame_format))
    ok = torch.zeros((2, 6, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="frame_format"):
        _yuv_frames(ok, "bgr", 3)
    with pytest.raises(ValueError):
        _yuv_frames(ok.float(), "i420", 3)
    with pytest.raises(ValueError):
        _yuv_frames(ok[None], "i420", 3)
    with pytest.raises(ValueError):
        _yuv_frames(torch.zeros((2, 7, 4), dtype=torch.uint8), "nv12", 3)
    with pytest.raises(ValueError):
        _yuv_frames(torch.zeros((2, 6, 5), dtype=torch.uint8), "nv12", 3)
    # the camera-sharded path refuses YUV outright (it would misread the bytes as BGR)
    for fmt in ("i420", "nv12"):
        with pytest.raises(ValueError, match="camera-sharded"):
            ShardedPredictor.submit(NS(), ok[None], fmt)
