"""No GPU: raw sensor surfaces (SensorSurface / jh_sensor_surface).  The rules of the description, in Python and
through jh_sensor_surface_check (the library loads without a GPU); the properties of the numpy reference of the
demosaic (synthetic.sensor_to_bgr), which the GPU tests compare the kernels with bit for bit; and the drivers' host
logic with stub predictors."""
import csv
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import synthetic as S

BAYER = ("rggb", "bggr", "grbg", "gbrg")
PATTERNS = ("mono",) + BAYER
SIZES = ((4, 4), (6, 10), (34, 66))
CODES = {"mono": 0, "rggb": 1, "bggr": 2, "grbg": 3, "gbrg": 4}

# (h, w, image_stride, offset, pitch, pattern code, reserved), valid?
DESCRIPTIONS = [
    ((6, 10, 60, 0, 10, 0, 0), True),                   # tight mono
    ((6, 10, 60, 0, 10, 1, 0), True),                   # tight rggb
    ((6, 10, 7 + 5 * 16 + 10, 7, 16, 4, 0), True),      # pitched, with an offset: the last sample is the last byte
    ((6, 10, 1 << 40, 3, 1 << 20, 2, 0), True),         # a huge stride is no error
    ((5, 9, 45, 0, 9, 0, 0), True),                     # mono takes odd sizes
    ((1, 1, 1, 0, 1, 0, 0), True),                      # ... and a single pixel
    ((4, 4, 16, 0, 4, 3, 0), True),                     # the smallest Bayer image
    ((0, 10, 60, 0, 10, 0, 0), False),                  # no height
    ((6, -2, 60, 0, 10, 0, 0), False),                  # negative width
    ((5, 10, 60, 0, 10, 1, 0), False),                  # Bayer: odd height
    ((6, 9, 60, 0, 10, 2, 0), False),                   # Bayer: odd width
    ((2, 10, 60, 0, 10, 3, 0), False),                  # Bayer: fewer than 4 rows
    ((6, 2, 60, 0, 10, 4, 0), False),                   # Bayer: fewer than 4 columns
    ((6, 10, 60, 0, 9, 0, 0), False),                   # pitch < w
    ((6, 10, 60, -1, 10, 0, 0), False),                 # negative offset
    ((6, 10, 59, 0, 10, 0, 0), False),                  # the image ends beyond the stride, by one byte
    ((6, 10, 7 + 5 * 16 + 9, 7, 16, 4, 0), False),      # ... the pitched one too
    ((6, 10, 60, 0, 1 << 62, 0, 0), False),             # a pitch that would wrap int64
    ((6, 10, 60, 0, 10, 5, 0), False),                  # unknown pattern
    ((6, 10, 60, 0, 10, -1, 0), False),                 # unknown pattern
    ((6, 10, 60, 0, 10, 1, 1), False),                  # reserved
]


def test_python_and_c_validation_agree():
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd import sensor_surface as M
    lib = N.lib()
    names = {v: k for k, v in CODES.items()}
    for d, good in DESCRIPTIONS:
        h, w, stride, off, pitch, pat, res = d
        st = N.SensorSurfaceStruct(stride, off, pitch, pat, res)
        rc = lib.jh_sensor_surface_check(st, h, w)
        assert (rc == 0) == good, (d, lib.jh_last_error())
        if not good:
            assert lib.jh_last_error()
        if res:
            continue                                     # (Python has no `reserved`: struct() writes the 0)
        try:
            s = SensorSurface(h, w, names.get(pat, "rgbw"), pitch=pitch, offset=off, image_stride=stride)
            ok = True
        except ValueError:
            ok = False
        assert ok == good, d
        if good:
            q = s.struct()
            assert [getattr(q, f) for f, _ in q._fields_] == [stride, off, pitch, pat, 0]
            assert s.check() is s
            M.check(h, w, names[pat], pitch, off, stride)
    assert lib.jh_sensor_surface_check(None, 6, 10) != 0
    # the same description, another frame size
    assert lib.jh_sensor_surface_check(SensorSurface(6, 10, "rggb").struct(), 8, 10) != 0
    # every rule has its own text
    texts = set()
    for d in ((0, 10, 60, 0, 10, 0, 0), (5, 10, 60, 0, 10, 1, 0), (6, 10, 60, 0, 9, 0, 0), (6, 10, 60, -1, 10, 0, 0),
              (6, 10, 59, 0, 10, 0, 0), (6, 10, 60, 0, 10, 5, 0), (6, 10, 60, 0, 10, 1, 1)):
        assert lib.jh_sensor_surface_check(N.SensorSurfaceStruct(*d[2:]), d[0], d[1]) != 0
        texts.add(lib.jh_last_error())
    assert len(texts) == 7


def test_sensor_surface_constructor():
    s = SensorSurface(1024, 1280, "rggb", pitch=1536, offset=64)
    assert (s.image_stride, s.pitch, s.offset, s.pattern) == (64 + 1024 * 1536, 1536, 64, "rggb")
    t = SensorSurface(4, 6)
    assert (t.pattern, t.pitch, t.offset, t.image_stride) == ("mono", 6, 0, 24)
    assert s == SensorSurface(1024, 1280, "rggb", pitch=1536, offset=64)
    assert s != SensorSurface(1024, 1280, "bggr", pitch=1536, offset=64) and len({s, t}) == 2
    assert s != YuvSurface(1024, 1280) and "rggb" in repr(s)
    with pytest.raises(AttributeError):
        s.pitch = 1280
    msgs = set()
    for kw in (dict(pattern="rgbw"), dict(pitch=5), dict(offset=-1), dict(image_stride=23), dict(pitch=6.0),
               dict(offset=True)):
        with pytest.raises(ValueError) as e:
            SensorSurface(4, 6, **kw)
        msgs.add(str(e.value).split(",")[0].split("(")[0])
    assert len(msgs) >= 5                                # one text per rule
    for hw in ((0, 6), (4, -6), (5, 6), (4, 7), (2, 6), (4, 2)):
        with pytest.raises(ValueError):
            SensorSurface(*hw, "grbg")
    assert SensorSurface(5, 7).image_stride == 35        # mono: any positive size


@pytest.mark.parametrize("H,W", SIZES)
def test_reference_properties(H, W):
    g = np.random.default_rng(H * 100 + W)
    raw = g.integers(0, 256, (2, H, W), dtype=np.uint8)
    # mono triplicates the byte
    m = S.sensor_to_bgr(raw, "mono")
    assert m.shape == (2, H, W, 3) and m.dtype == np.uint8 and all(np.array_equal(m[..., c], raw) for c in range(3))
    for p in BAYER:
        # a constant colour comes back exactly at EVERY pixel, borders included: (4a + 2) >> 2 == a, (2a + 1) >> 1 == a
        for colour in ((0, 0, 0), (255, 255, 255), (255, 0, 1), (3, 254, 129)):
            img = np.broadcast_to(np.array(colour, np.uint8), (H, W, 3))
            assert np.array_equal(S.sensor_to_bgr(S.mosaic(img, p), p), img), (p, colour)
        out = S.sensor_to_bgr(raw, p)
        # border pixels equal their clamped interior neighbour
        yc, xc = np.clip(np.arange(H), 1, H - 2), np.clip(np.arange(W), 1, W - 2)
        assert np.array_equal(out, out[:, yc][:, :, xc]), p
        assert np.array_equal(out[:, 0, 0], out[:, 1, 1]) and np.array_equal(out[:, H - 1, W - 1], out[:, H - 2, W - 2])
        # the sample of a site is its own colour there (interior), and mosaic() inverts it
        assert np.array_equal(S.mosaic(out, p)[:, 1:-1, 1:-1], raw[:, 1:-1, 1:-1]), p
    # an interior pixel by hand: rggb, (1, 1) is a blue site, (1, 2) a green site of a blue row
    r = raw[0].astype(np.int64)
    o = S.sensor_to_bgr(raw[0], "rggb")
    assert tuple(o[1, 1]) == (r[1, 1], (r[0, 1] + r[2, 1] + r[1, 0] + r[1, 2] + 2) >> 2,
                              (r[0, 0] + r[0, 2] + r[2, 0] + r[2, 2] + 2) >> 2)
    assert tuple(o[1, 2]) == ((r[1, 1] + r[1, 3] + 1) >> 1, r[1, 2], (r[0, 2] + r[2, 2] + 1) >> 1)


@pytest.mark.parametrize("H,W", SIZES)
def test_reference_shift_equivalence(H, W):
    """Dropping the first row turns rggb into gbrg (and bggr into grbg); dropping the first column turns rggb into
    grbg: the demosaics agree on the common interior."""
    g = np.random.default_rng(W)
    raw = g.integers(0, 256, (H + 2, W + 2), dtype=np.uint8)
    for full, rows in (("rggb", "gbrg"), ("bggr", "grbg"), ("grbg", "bggr"), ("gbrg", "rggb")):
        a = S.sensor_to_bgr(raw[:H, :W], full)
        b = S.sensor_to_bgr(raw[1:H + 1, :W], rows)
        # row y of `a` is row y - 1 of `b`: the interior rows of both, the interior columns
        assert np.array_equal(a[2:H - 1, 1:W - 1], b[1:H - 2, 1:W - 1]), (full, rows)
    a = S.sensor_to_bgr(raw[:H, :W], "rggb")
    c = S.sensor_to_bgr(raw[:H, 1:W + 1], "grbg")
    assert np.array_equal(a[1:H - 1, 2:W - 1], c[1:H - 1, 1:W - 2])


def test_mosaic_and_pack():
    g = np.random.default_rng(5)
    bgr = g.integers(0, 256, (3, 6, 10, 3), dtype=np.uint8)
    assert np.array_equal(S.mosaic(bgr, "mono"), bgr[..., 1])
    raw = S.mosaic(bgr, "grbg")                          # G R / B G
    for (y0, x0), ch in (((0, 0), 1), ((0, 1), 2), ((1, 0), 0), ((1, 1), 1)):
        assert np.array_equal(raw[:, y0::2, x0::2], bgr[:, y0::2, x0::2, ch]), (y0, x0)
    s = SensorSurface(6, 10, "grbg", pitch=16, offset=7, image_stride=7 + 6 * 16 + 5)
    buf = S.pack_sensor_surface(raw, s, 0xA5)
    assert buf.shape == (3, s.image_stride) and int((buf != 0xA5).sum()) <= 3 * 60
    rows = buf[:, 7:7 + 6 * 16].reshape(3, 6, 16)
    assert np.array_equal(rows[:, :, :10], raw) and (rows[:, :, 10:] == 0xA5).all() and (buf[:, :7] == 0xA5).all()
    with pytest.raises(ValueError):
        S.pack_sensor_surface(raw[:, :4], s)
    with pytest.raises(ValueError):
        S.sensor_to_bgr(raw[:, :3], "rggb")


class Stub3D:
    """As tests/test_yuv_surface_cpu.py's: points = first byte of the frame set + joint index; first byte 255 = `not
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


def _rows(path, name="data3D.csv"):
    return list(csv.reader(open(os.path.join(path, name))))[2:]


def test_predict3D_frames_layout_host_logic(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    C, J = 2, 3
    s = SensorSurface(4, 6, "rggb", pitch=8, offset=3, image_stride=40)
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
    # errors, before anything is written or run
    for fmt in ("i420", "nv12"):
        with pytest.raises(ValueError, match="frame_layout"):
            P.predict3D_frames(Stub3D(), sets, None, None, None, cfg, str(tmp_path / "bad"), frame_format=fmt,
                               frame_layout=s)
    with pytest.raises(ValueError, match="SensorSurface"):
        P.predict3D_frames(Stub3D(), sets, None, None, None, cfg, str(tmp_path / "bad"), frame_layout="rggb")
    for spec in (((C, s.image_stride + 1), torch.uint8), ((C, 4, 6), torch.uint8),
                 ((C, s.image_stride), torch.float32)):
        with pytest.raises(ValueError):
            P.predict3D_frames(Stub3D(), fills, None, None, None, cfg, str(tmp_path / "bad"), frame_layout=s,
                               frame_spec=spec)
    assert not os.path.exists(tmp_path / "bad")
    for bad in (np.zeros((C, s.image_stride - 1), np.uint8), np.zeros((C, 4, 6), np.uint8),
                np.zeros((C, s.image_stride), np.float32)):
        pred = Stub3D()
        with pytest.raises(ValueError):
            P.predict3D_frames(pred, [bad], None, None, None, cfg, str(tmp_path / "odd"), frame_layout=s)
        assert pred.kwargs == []


def test_predict2D_frames_layout_host_logic(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict2D as P
    J = 2
    s = SensorSurface(4, 4, "mono", pitch=6)
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
    done = P.predict2D_recordings(pred, {"v.raw": frames}, cfg, str(tmp_path / "r"), time_batch=5, frame_layout=s)
    assert done == {"data2D.csv": 5} and pred.kwargs == [{"frame_layout": s}]
    fills = [(lambda dst, i=i: dst.fill(i)) for i in (7, 8, 9)]
    assert P.predict2D_frames(Stub2D(), fills, cfg, str(tmp_path / "fill"), time_batch=2, frame_layout=s,
                              frame_spec=((s.image_stride,), torch.uint8)) == 3
    assert [r[0] for r in _rows(tmp_path / "fill", "data2D.csv")] == ["7", "8", "9"]
    with pytest.raises(ValueError, match="frame_layout"):
        P.predict2D_frames(Stub2D(), frames, cfg, str(tmp_path / "bad"), frame_format="nv12", frame_layout=s)
    for bad in (np.zeros((4, 6), np.uint8), np.zeros((s.image_stride + 1,), np.uint8),
                np.zeros((s.image_stride,), np.int8)):
        pred = Stub2D()
        with pytest.raises(ValueError):
            P.predict2D_frames(pred, [bad], cfg, str(tmp_path / "odd"), frame_layout=s)
        assert pred.kwargs == []
    assert not os.path.exists(tmp_path / "bad")


def test_pipeline_keys_on_the_layout():
    """The same byte count under another description (another pattern, or a YUV surface) is another pipeline."""
    from jarvis_hybridnet_amd.prediction import _ingest as I
    a = SensorSurface(4, 6, "rggb", image_stride=36)
    b = SensorSurface(4, 6, "bggr", image_stride=36)
    y = YuvSurface(4, 6, "nv12")
    assert y.image_stride == 36
    owner = NS()
    f = np.zeros((2, 36), np.uint8)
    noop = lambda *x: None  # noqa: E731
    p1 = I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=a)
    assert I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=a) is p1
    assert I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=SensorSurface(4, 6, "rggb", image_stride=36)) is p1
    assert p1.host[0].shape == (2, 2, 36) and p1.host[0].dtype == torch.uint8
    p2 = I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=b)
    assert p2 is not p1 and len(owner._ingest_cache) == 1
    p3 = I.pipeline_for(owner, f, 2, 1, noop, noop, frame_layout=y)
    assert p3 is not p2
    I.release_ingest_buffers(owner)


def test_entry_points_refuse_bad_layout_arguments():
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd.distributed import ShardedPredictor
    from jarvis_hybridnet_amd.prediction import _ingest as I
    s = SensorSurface(4, 6, "gbrg", pitch=8)
    ok = torch.zeros((3, 2, s.image_stride), dtype=torch.uint8)
    def frame_layout(layout, fmt, lead, hw, frames):
        return N.describe_frames(frames, lead, fmt, layout, hw)
    assert N.describe_shape(ok.shape, ok.dtype, (3, 2), None, s, (4, 6)).layout is s
    assert N.describe_shape(ok.shape, ok.dtype, (None, 2), "bgr", s).layout is s
    assert N.check_layout(s) is s and N.check_layout(YuvSurface(4, 6)) is not None
    for fmt in ("i420", "nv12"):
        with pytest.raises(ValueError, match="frame_layout"):
            frame_layout(s, fmt, (3, 2), (4, 6), ok)
    for bad in (ok.float(), ok[0], ok[..., :-1], torch.zeros((3, 1, s.image_stride), dtype=torch.uint8), ok.numpy()):
        with pytest.raises(ValueError, match="SensorSurface"):
            frame_layout(s, None, (3, 2), (4, 6), bad)
    with pytest.raises(ValueError, match="4 x 6"):
        frame_layout(s, None, (3, 2), (8, 6), ok)
    with pytest.raises(ValueError, match="a YuvSurface or a SensorSurface"):
        frame_layout(s.struct(), None, (3, 2), (4, 6), ok)
    with pytest.raises(ValueError, match="camera-sharded"):
        ShardedPredictor.submit(NS(), ok, frame_layout=s)
    assert I.driver_format("bgr", ((2, s.image_stride), torch.uint8), 3, s) is False
    with pytest.raises(ValueError, match="frame_layout"):
        I.driver_format("nv12", None, 3, s)
    with pytest.raises(ValueError, match="SensorSurface"):
        I.driver_format("bgr", ((2, 4, 6), torch.uint8), 3, s)


def test_new_symbols_in_header_and_ctypes_table():
    import re
    from jarvis_hybridnet_amd import _native as N
    from tests.test_native_abi import ROOT, header_symbols
    for name in ("jh_sensor_surface_check", "jh_predictor_forward_sensor", "jh_predictor2d_forward_sensor",
                 "jh_op_sensor_to_bgr"):
        assert name in header_symbols() and name in N.symbols() and hasattr(N.lib(), name), name
    assert N.lib().jh_abi_version() == 4
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    codes = dict(re.findall(r"#define JH_SENSOR_(\w+) (\d+)", text))
    assert codes == {k.upper(): str(v) for k, v in CODES.items()}
    from jarvis_hybridnet_amd.sensor_surface import PATTERNS as P
    assert P == CODES
