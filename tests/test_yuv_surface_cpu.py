"""CPU: described YUV 4:2:0 surfaces (jh_yuv_surface / YuvSurface) on the host side -- the numpy reference of the
contract (plane addressing and the four fixed-point constant rows, include/jarvis_hip.h), the validation rules in
Python and in C (the library is loaded, no kernel runs), and the drivers' handling of `frame_layout` with stub
predictors."""
import csv
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests.test_yuv_ingest_cpu import yuv420_to_bgr

# the contract's table (ISSUE / include/jarvis_hip.h), written out here on purpose: Y0, CY, CVR, CUB, CUG, CVG
ROWS = {
    ("bt601", "limited"): (16, 1220542, 1673527, 2116026, -409993, -852492),
    ("bt601", "full"): (0, 1048576, 1470104, 1858077, -360853, -748826),
    ("bt709", "limited"): (16, 1220945, 1879825, 2215014, -223607, -558796),
    ("bt709", "full"): (0, 1048576, 1651297, 1945738, -196424, -490864),
}
ORDERS = ("i420", "yv12", "nv12", "nv21")


def convert(Y, U, V, matrix, rng):
    """int64 arrays Y, U, V (same shape) -> (b, g, r) by the contract's arithmetic; asserts the int32 headroom."""
    y0, cy, cvr, cub, cug, cvg = ROWS[(matrix, rng)]
    u, v = U - 128, V - 128
    yy = np.maximum(Y - y0, 0) * cy + (1 << 19)
    sums = (yy + cvr * v, yy + cvg * v + cug * u, yy + cub * u)
    for t in (yy, cvg * v) + sums:
        assert np.abs(t).max() < (1 << 30)
    r, g, b = (np.clip(t >> 20, 0, 255) for t in sums)
    return b, g, r


def surface_to_bgr(buf, s):
    """(..., image_stride) uint8 images of the YuvSurface `s` -> (..., H, W, 3) uint8 BGR: Y(y, x) at
    y_offset + y * y_pitch + x, U / V of block (y/2, x/2) at *_offset + (y/2) * c_pitch + (x/2) * c_step."""
    buf = np.asarray(buf, np.uint8)
    assert buf.shape[-1] == s.image_stride
    yy, xx = np.meshgrid(np.arange(s.height), np.arange(s.width), indexing="ij")
    c = (yy // 2) * s.c_pitch + (xx // 2) * s.c_step
    Y = buf[..., s.y_offset + yy * s.y_pitch + xx].astype(np.int64)
    U = buf[..., s.u_offset + c].astype(np.int64)
    V = buf[..., s.v_offset + c].astype(np.int64)
    return np.stack(convert(Y, U, V, s.matrix, s.range), -1).astype(np.uint8)


def random_planes(g, lead, H, W):
    return (g.integers(0, 256, lead + (H, W), dtype=np.uint8), g.integers(0, 256, lead + (H // 2, W // 2), dtype=np.uint8),
            g.integers(0, 256, lead + (H // 2, W // 2), dtype=np.uint8))


@pytest.mark.parametrize("H,W", [(4, 6), (30, 42)])
def test_reference_equals_the_tight_formats(H, W):
    g = np.random.default_rng(H)
    y, u, v = random_planes(g, (3,), H, W)
    for fmt, swapped in (("i420", "yv12"), ("nv12", "nv21")):
        s = YuvSurface(H, W, fmt)
        assert s.image_stride == H * W * 3 // 2
        tight = S.pack_yuv420(y, u, v, fmt)
        buf = S.pack_yuv_surface(y, u, v, s, fill=0xEE)
        assert np.array_equal(buf, tight.reshape(3, -1))                    # tight: no byte outside the planes
        want = yuv420_to_bgr(tight, fmt)
        assert np.array_equal(surface_to_bgr(buf, s), want)
        # the V-first orders: the same bytes with U and V swapped
        s2 = YuvSurface(H, W, swapped)
        assert np.array_equal(surface_to_bgr(S.pack_yuv420(y, v, u, fmt).reshape(3, -1), s2), want)
        assert np.array_equal(S.pack_yuv_surface(y, u, v, s2), S.pack_yuv420(y, v, u, fmt).reshape(3, -1))


def test_padding_never_influences_the_reference():
    g = np.random.default_rng(11)
    H, W = 6, 10
    y, u, v = random_planes(g, (2,), H, W)
    want = surface_to_bgr(S.pack_yuv_surface(y, u, v, YuvSurface(H, W, "i420")), YuvSurface(H, W, "i420"))
    for order in ORDERS:
        semi = order.startswith("nv")
        probe = YuvSurface(H, W, order, y_pitch=W + 6, c_pitch=(W + 6) if semi else W // 2 + 4, luma_rows=H + 3)
        s = YuvSurface(H, W, order, y_pitch=W + 6, c_pitch=probe.c_pitch, luma_rows=H + 3,
                       image_stride=probe.image_stride + 10)
        a = S.pack_yuv_surface(y, u, v, s, fill=0xA5)
        b = S.pack_yuv_surface(y, u, v, s, fill=0x5A)
        assert not np.array_equal(a, b)
        assert np.array_equal(surface_to_bgr(a, s), want) and np.array_equal(surface_to_bgr(b, s), want)


def real_matrix(matrix, rng):
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    kg = 1.0 - kr - kb
    sy, sc, y0 = (255.0 / 219.0, 255.0 / 224.0, 16) if rng == "limited" else (1.0, 1.0, 0)
    return y0, sy, 2 * (1 - kr) * sc, 2 * (1 - kb) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc


@pytest.mark.parametrize("matrix,rng", list(ROWS))
def test_constant_rows(matrix, rng):
    assert YuvSurface(2, 2, matrix=matrix, range=rng).coefficients == ROWS[(matrix, rng)]
    y0, sy, cvr, cub, cug, cvg = real_matrix(matrix, rng)
    if (matrix, rng) != ("bt601", "limited"):                     # (that row keeps OpenCV's three-decimal literals)
        want = (y0,) + tuple(int(round(x * (1 << 20))) for x in (sy, cvr, cub, cug, cvg))
        assert ROWS[(matrix, rng)] == want
    # neutral chroma: grey, monotone in Y, the end points of the range
    Y = np.arange(256, dtype=np.int64)
    b, g, r = convert(Y, np.full(256, 128), np.full(256, 128), matrix, rng)
    assert np.array_equal(b, g) and np.array_equal(g, r) and (np.diff(g) >= 0).all()
    if rng == "limited":
        assert g[16] == 0 and g[235] == 255 and g[0] == 0 and g[255] == 255
    else:
        assert np.array_equal(g, Y)
    # every partial sum below 2^30 (asserted inside convert) and, for the derived rows, within 0.51 of the float64
    # matrix: 0.5 for the shift + 511 * 2^-21 for the rounding of the coefficients (< 0.5003), over every Y and
    # every U, V in steps of 3
    c = np.arange(0, 256, 3, dtype=np.int64)
    Yg, Ug, Vg = np.meshgrid(Y, c, c, indexing="ij")
    got = convert(Yg, Ug, Vg, matrix, rng)
    if (matrix, rng) == ("bt601", "limited"):
        return
    yf = np.maximum(Yg - y0, 0) * sy
    uf, vf = (Ug - 128).astype(np.float64), (Vg - 128).astype(np.float64)
    ref = (yf + cub * uf, yf + cug * uf + cvg * vf, yf + cvr * vf)
    for k in range(3):
        err = np.abs(got[k] - np.clip(ref[k], 0, 255)).max()
        assert err <= 0.51, (matrix, rng, k, err)


def test_forward_transform_round_trip():
    """synthetic.bgr_to_yuv with the matching matrix and range is close to the contract's inverse on smooth images."""
    yy, xx = np.meshgrid(np.arange(32), np.arange(48), indexing="ij")
    bgr = np.stack([40 + 4 * xx, 60 + 3 * yy, 200 - 2 * xx - yy], -1).clip(0, 255).astype(np.uint8)
    for (matrix, rng) in ROWS:
        s = YuvSurface(32, 48, "nv21", matrix=matrix, range=rng, y_pitch=64)
        back = surface_to_bgr(S.pack_yuv_surface(*S.bgr_to_yuv(bgr, matrix, rng), s, fill=7), s)
        assert np.abs(back.astype(int) - bgr).max() <= 8, (matrix, rng)
    # the wrong matrix shifts the colours: what the description is for
    s = YuvSurface(32, 48, "nv12", matrix="bt601", range="limited")
    wrong = surface_to_bgr(S.pack_yuv_surface(*S.bgr_to_yuv(bgr, "bt709", "full"), s), s)
    assert np.abs(wrong.astype(int) - bgr).max() > 16


# (height, width, y_offset, y_pitch, u_offset, v_offset, c_pitch, c_step, image_stride, matrix, range) and whether it is good
H, W = 6, 10
DESCRIPTIONS = [
    ((H, W, 0, 10, 60, 75, 5, 1, 90, 0, 0), True),               # tight I420
    ((H, W, 0, 10, 75, 60, 5, 1, 90, 1, 1), True),               # tight YV12, BT.709 full
    ((H, W, 0, 16, 144, 145, 16, 2, 200, 1, 0), True),           # pitched NV12, luma_rows 9, a gap at the end
    ((H, W, 0, 10, 61, 60, 10, 2, 90, 0, 1), True),              # tight NV21
    ((H, W, 4, 10, 64, 80, 5, 1, 95, 0, 0), True),               # planes at explicit offsets; U ends at 79, V at 95
    ((H, W, 0, 10, 60, 75, 5, 1, 1 << 40, 0, 0), True),          # a huge stride is no error
    ((5, W, 0, 10, 60, 75, 5, 1, 90, 0, 0), False),              # odd height
    ((H, 9, 0, 10, 60, 75, 5, 1, 90, 0, 0), False),              # odd width
    ((0, W, 0, 10, 60, 75, 5, 1, 90, 0, 0), False),              # no height
    ((H, W, 0, 10, 60, 75, 5, 3, 90, 0, 0), False),              # c_step
    ((H, W, 0, 9, 60, 75, 5, 1, 90, 0, 0), False),               # y_pitch < w
    ((H, W, 0, 10, 60, 75, 4, 1, 90, 0, 0), False),              # c_pitch < w/2
    ((H, W, 0, 10, 60, 61, 8, 2, 90, 0, 0), False),              # c_pitch < (w/2) * 2
    ((H, W, -2, 10, 60, 75, 5, 1, 90, 0, 0), False),             # negative offset
    ((H, W, 0, 10, 60, 75, 5, 1, -90, 0, 0), False),             # negative stride
    ((H, W, 0, 10, 60, 62, 10, 2, 95, 0, 0), False),             # semi-planar: U and V two bytes apart
    ((H, W, 0, 10, 61, 62, 10, 2, 95, 0, 0), False),             # semi-planar: the pair starts at an odd offset
    ((H, W, 0, 12, 72, 73, 11, 2, 110, 0, 0), False),            # semi-planar: odd c_pitch
    ((H, W, 0, 10, 60, 75, 5, 1, 59, 0, 0), False),              # Y ends beyond the stride
    ((H, W, 0, 10, 60, 75, 5, 1, 74, 0, 0), False),              # U does
    ((H, W, 0, 10, 60, 75, 5, 1, 89, 0, 0), False),              # V does, by one byte
    ((H, W, 0, 1 << 62, 60, 75, 5, 1, 90, 0, 0), False),         # a pitch that would wrap int64
    ((H, W, 0, 10, 60, 75, 5, 1, 90, 2, 0), False),              # unknown matrix
    ((H, W, 0, 10, 60, 75, 5, 1, 90, 0, 2), False),              # unknown range
]


def test_python_and_c_validation_agree():
    """YuvSurface.from_planes and jh_yuv_surface_check (through ctypes; the library loads without a GPU) give the
    same verdict on every description."""
    from jarvis_hybridnet_amd import _native as N
    lib = N.lib()
    mnames, rnames = {0: "bt601", 1: "bt709"}, {0: "limited", 1: "full"}
    for d, good in DESCRIPTIONS:
        h, w, yo, yp, uo, vo, cp, cs, stride, m, r = d
        st = N.YuvSurfaceStruct(stride, yo, yp, uo, vo, cp, cs, m, r, 0)
        rc = lib.jh_yuv_surface_check(st, h, w)
        assert (rc == 0) == good, (d, lib.jh_last_error())
        if not good:
            assert lib.jh_last_error()
        try:
            s = YuvSurface.from_planes(h, w, yo, yp, uo, vo, cp, cs, stride, matrix=mnames.get(m, "bt2020"),
                                       range=rnames.get(r, "studio"))
            ok = True
        except ValueError:
            ok = False
        assert ok == good, d
        if good:
            q = s.struct()
            assert [getattr(q, f) for f, _ in q._fields_] == [stride, yo, yp, uo, vo, cp, cs, m, r, 0]
            assert s.image_stride == stride
    # reserved must be 0, and a null description is refused
    st = YuvSurface(H, W).struct()
    assert lib.jh_yuv_surface_check(st, H, W) == 0
    st.reserved = 1
    assert lib.jh_yuv_surface_check(st, H, W) != 0 and b"reserved" in lib.jh_last_error()
    assert lib.jh_yuv_surface_check(None, H, W) != 0
    # the same description, another frame size
    assert lib.jh_yuv_surface_check(YuvSurface(H, W).struct(), H + 2, W) != 0


def test_yuv_surface_constructor():
    s = YuvSurface(1024, 1280, "nv12", matrix="bt709", y_pitch=1536, c_pitch=1536, luma_rows=1088)
    assert (s.u_offset, s.v_offset, s.c_step, s.image_stride) == (1088 * 1536, 1088 * 1536 + 1, 2, 1088 * 1536 + 512 * 1536)
    assert (YuvSurface(4, 6).u_offset, YuvSurface(4, 6).c_step, YuvSurface(4, 6).image_stride) == (24, 2, 36)
    t = YuvSurface(4, 6, "yv12")
    assert (t.v_offset, t.u_offset, t.c_pitch, t.c_step) == (24, 30, 3, 1)
    assert YuvSurface(4, 6, "nv21").u_offset == 25 and YuvSurface(4, 6, "nv21").v_offset == 24
    assert s == YuvSurface(1024, 1280, "nv12", matrix="bt709", y_pitch=1536, c_pitch=1536, luma_rows=1088)
    assert s != YuvSurface(1024, 1280, "nv12", y_pitch=1536, c_pitch=1536, luma_rows=1088) and len({s, t}) == 2
    with pytest.raises(AttributeError):
        s.y_pitch = 1280
    for kw in (dict(order="yuv420p"), dict(matrix="bt2020"), dict(range="studio"), dict(luma_rows=2), dict(y_pitch=5),
               dict(c_pitch=4), dict(order="i420", c_pitch=2), dict(order="nv12", c_pitch=7), dict(image_stride=35),
               dict(y_pitch=6.0)):
        with pytest.raises(ValueError):
            YuvSurface(4, 6, **kw)
    with pytest.raises(ValueError):
        YuvSurface(5, 6)


class Stub3D:
    """As tests/test_yuv_ingest_cpu.py's: points = first byte of the frame set + joint index; first byte 255 = `not
    detected`; records what every call was given."""
    J = 3

    def __init__(self):
        self.kwargs, self.shapes = [], []

    def forward_batch(self, x, *calib, **kw):
        self.kwargs.append(kw)
        self.shapes.append(tuple(x.shape))
        ids = x.reshape(x.shape[0], -1)[:, 0].float()
        pts = ids[:, None, None] + torch.arange(self.J).float()[None, :, None] + torch.zeros(1, 1, 3)
        return pts, torch.full((x.shape[0], self.J), 0.5), (ids != 255).int()


class StubOld3D:
    """A predictor that knows `frame_format=` only (the stubs of the existing tests)."""

    def forward_batch(self, x, *calib, frame_format=None):
        return Stub3D().forward_batch(x)


def _rows(path, name="data3D.csv"):
    return list(csv.reader(open(os.path.join(path, name))))[2:]


def test_predict3D_frames_layout_host_logic(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    C, J = 2, 3
    s = YuvSurface(4, 6, "nv12", matrix="bt709", y_pitch=8, c_pitch=8, luma_rows=5)
    cfg = NS(KEYPOINT_NAMES=["a", "b", "c"], KEYPOINTDETECT=NS(NUM_JOINTS=J))
    sets = [np.full((C, s.image_stride), 255 if i == 2 else i, np.uint8) for i in range(7)]
    for tb, st in ((1, 1), (3, 2), (4, 1)):
        pred = Stub3D()
        out = str(tmp_path / ("l_%d_%d" % (tb, st)))
        assert P.predict3D_frames(pred, iter(sets), None, None, None, cfg, out, time_batch=tb, streams=st,
                                  frame_layout=s) == 7
        got = _rows(out)
        assert len(got) == 7 and got[2] == ["NaN"] * (4 * J)
        assert [float(r[0]) for i, r in enumerate(got) if i != 2] == [0.0, 1.0, 3.0, 4.0, 5.0, 6.0]
        assert set(pred.shapes) == {(tb, C, s.image_stride)}                 # staging (tb, C, image_stride)
        assert all(kw == {"frame_layout": s} for kw in pred.kwargs) and len(pred.kwargs) == -(-7 // tb)
    # fill callables decode into the (C, image_stride) staging buffer
    pred = Stub3D()
    fills = [(lambda dst, i=i: dst.fill(i)) for i in (4, 5, 6)]
    out = str(tmp_path / "fill")
    assert P.predict3D_frames(pred, fills, None, None, None, cfg, out, time_batch=2, frame_layout=s,
                              frame_spec=((C, s.image_stride), torch.uint8)) == 3
    assert [r[0] for r in _rows(out)] == ["4.0", "5.0", "6.0"] and set(pred.shapes) == {(2, C, s.image_stride)}
    # the layout reaches the predictor only when given: a predictor that does not know the keyword keeps working
    bgr = [np.full((C, 4, 6, 3), i, np.uint8) for i in range(3)]
    assert P.predict3D_frames(StubOld3D(), bgr, None, None, None, cfg, str(tmp_path / "bgr"), time_batch=2) == 3
    pred = Stub3D()
    assert P.predict3D_frames(pred, bgr, None, None, None, cfg, str(tmp_path / "bgr2"), time_batch=2) == 3
    assert pred.kwargs == [{}, {}]
    # errors, before anything is written or run
    for fmt in ("i420", "nv12"):
        with pytest.raises(ValueError, match="frame_layout"):
            P.predict3D_frames(Stub3D(), sets, None, None, None, cfg, str(tmp_path / "bad"), frame_format=fmt,
                               frame_layout=s)
    with pytest.raises(ValueError, match="frame_format"):
        P.predict3D_frames(Stub3D(), sets, None, None, None, cfg, str(tmp_path / "bad"), frame_format="yv12",
                           frame_layout=s)
    with pytest.raises(ValueError, match="YuvSurface"):
        P.predict3D_frames(Stub3D(), sets, None, None, None, cfg, str(tmp_path / "bad"), frame_layout="nv12")
    for spec in (((C, s.image_stride + 1), torch.uint8), ((C, 6, 6), torch.uint8), ((C, s.image_stride), torch.float32)):
        with pytest.raises(ValueError):
            P.predict3D_frames(Stub3D(), fills, None, None, None, cfg, str(tmp_path / "bad"), frame_layout=s,
                               frame_spec=spec)
    assert not os.path.exists(tmp_path / "bad")
    for bad in (np.zeros((C, s.image_stride - 1), np.uint8), np.zeros((C, 6, 6), np.uint8),
                np.zeros((C, s.image_stride), np.float32)):
        pred = Stub3D()
        with pytest.raises(ValueError):
            P.predict3D_frames(pred, [bad], None, None, None, cfg, str(tmp_path / "odd"), frame_layout=s)
        assert pred.kwargs == []


def test_predict2D_frames_layout_host_logic(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict2D as P
    J = 2
    s = YuvSurface(4, 4, "yv12", range="full", y_pitch=6)
    cfg = NS(KEYPOINT_NAMES=["a", "b"], KEYPOINTDETECT=NS(NUM_JOINTS=J))

    class Stub2D:
        def __init__(self):
            self.kwargs, self.shapes = [], []

        def forward_batch(self, x, **kw):
            self.kwargs.append(kw)
            self.shapes.append(tuple(x.shape))
            ids = x.reshape(x.shape[0], -1)[:, 0].int()
            return ids[:, None, None] + torch.zeros(1, J, 2, dtype=torch.int32), torch.full((x.shape[0], J), 0.25), \
                (ids != 255).int()

    frames = [np.full((s.image_stride,), 255 if i == 1 else i, np.uint8) for i in range(5)]
    pred = Stub2D()
    assert P.predict2D_frames(pred, frames, cfg, str(tmp_path / "a"), time_batch=2, frame_layout=s) == 5
    assert [r[0] for r in _rows(tmp_path / "a", "data2D.csv")] == ["0", "NaN", "2", "3", "4"]
    assert pred.kwargs == [{"frame_layout": s}] * 3 and set(pred.shapes) == {(2, s.image_stride)}
    pred = Stub2D()
    done = P.predict2D_recordings(pred, {"v.mp4": frames}, cfg, str(tmp_path / "r"), time_batch=5, frame_layout=s)
    assert done == {"data2D.csv": 5} and pred.kwargs == [{"frame_layout": s}]
    fills = [(lambda dst, i=i: dst.fill(i)) for i in (7, 8, 9)]
    assert P.predict2D_frames(Stub2D(), fills, cfg, str(tmp_path / "fill"), time_batch=2, frame_layout=s,
                              frame_spec=((s.image_stride,), torch.uint8)) == 3
    assert [r[0] for r in _rows(tmp_path / "fill", "data2D.csv")] == ["7", "8", "9"]
    with pytest.raises(ValueError, match="frame_layout"):
        P.predict2D_frames(Stub2D(), frames, cfg, str(tmp_path / "bad"), frame_format="nv12", frame_layout=s)
    with pytest.raises(ValueError):
        P.predict2D_frames(Stub2D(), [np.zeros((6, 4), np.uint8)], cfg, str(tmp_path / "odd"), frame_layout=s)


def test_pipeline_keys_on_the_layout():
    """One cached ingest pipeline per format AND layout: the same byte count under another description is another
    pipeline."""
    from jarvis_hybridnet_amd.prediction import _ingest as I
    a = YuvSurface(4, 6, "nv12")
    b = YuvSurface(4, 6, "nv21")
    owner = NS()
    f = np.zeros((2, a.image_stride), np.uint8)
    noop = lambda *x: None  # noqa: E731
    p1 = I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=a)
    assert I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=a) is p1
    assert p1.host[0].shape == (2, 2, a.image_stride) and p1.host[0].dtype == torch.uint8
    p2 = I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=b)
    assert p2 is not p1 and len(owner._ingest_cache) == 1
    I.release_ingest_buffers(owner)


def test_entry_points_refuse_bad_layout_arguments():
    """dtype, rank, byte count and the frame_format combination are checked before anything reaches the GPU."""
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd.distributed import ShardedPredictor
    s = YuvSurface(4, 6, "nv12")
    ok = torch.zeros((3, 2, s.image_stride), dtype=torch.uint8)
    assert N.check_layout(None, "nv12") is None
    def frame_layout(layout, fmt, lead, hw, frames):
        return N.describe_frames(frames, lead, fmt, layout, hw)
    assert N.describe_shape(ok.shape, ok.dtype, (3, 2), None, s, (4, 6)).layout is s
    assert N.describe_shape(ok.shape, ok.dtype, (None, 2), "bgr", s).layout is s
    for fmt in ("i420", "nv12"):
        with pytest.raises(ValueError, match="frame_layout"):
            frame_layout(s, fmt, (3, 2), (4, 6), ok)
    for bad in (ok.float(), ok[0], ok[..., :-1], torch.zeros((3, 1, s.image_stride), dtype=torch.uint8), ok.numpy()):
        with pytest.raises(ValueError):
            frame_layout(s, None, (3, 2), (4, 6), bad)
    with pytest.raises(ValueError, match="4 x 6"):
        frame_layout(s, None, (3, 2), (8, 6), ok)
    with pytest.raises(ValueError, match="YuvSurface"):
        frame_layout(s.struct(), None, (3, 2), (4, 6), ok)
    with pytest.raises(ValueError, match="frame_layout"):
        ShardedPredictor.submit(NS(), ok, None, None, False, s)
    with pytest.raises(ValueError, match="camera-sharded"):
        ShardedPredictor.submit(NS(), ok, frame_layout=s)


def test_new_symbols_in_header_and_ctypes_table():
    import re
    from jarvis_hybridnet_amd import _native as N
    from tests.test_native_abi import ROOT, header_symbols
    for name in ("jh_yuv_surface_check", "jh_predictor_forward_surface", "jh_predictor2d_forward_surface",
                 "jh_op_yuv_surface_to_bgr"):
        assert name in header_symbols() and name in N.symbols() and hasattr(N.lib(), name), name
    assert N.lib().jh_abi_version() == 4
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    codes = dict(re.findall(r"#define JH_YUV_(\w+) (\d+)", text))
    assert codes == {"BT601": "0", "BT709": "1", "LIMITED": "0", "FULL": "1"}
