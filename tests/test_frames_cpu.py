"""No GPU: the one description of a call's frames (_native.Frames: describe_shape / describe_frames / frame_images) and
the one call site into the library (_native.forward_symbol / call_forward) -- which entry point every form calls, what
every input is taken for, every refusal, and that the public predictors check their arguments before they touch
anything else."""
from types import MethodType

import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import _native as N
from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D

H, W, T, C = 4, 6, 2, 3
U8 = torch.uint8
CODES = {"rgb": 0, "bgr": 1, "i420": 2, "nv12": 3, "surface": 4, "sensor": 5}
YUV, SENSOR = YuvSurface(H, W, "nv12"), SensorSurface(H, W, "rggb")


def test_codes_are_the_headers():
    import re
    text = open(N.os.path.join(N._HERE, "..", "include", "jarvis_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define JH_FRAME_(\w+)\s+(\d+)", text)}
    assert codes == {"RGB_F32": 0, "BGR_U8": 1, "I420": 2, "NV12": 3, "SURFACE": 4, "SENSOR": 5}
    assert N.FRAME_CODES == CODES and N.FRAME_FORMATS == {"bgr": 1, "i420": 2, "nv12": 3}


# The table of the C entry points, measured on the commit before this module existed (forward_entry and the two
# forward_images call expressions, driven with a recording library) and held here: (3D symbol, 2D symbol) per format
# without a mask; the 3D predictor's masked call of a fixed format goes through forward_masked.
PLAIN = {"rgb": "_forward", "bgr": "_forward_u8", "i420": "_forward_yuv", "nv12": "_forward_yuv",
         "surface": "_forward_surface", "sensor": "_forward_sensor"}


@pytest.mark.parametrize("name", sorted(CODES))
def test_entry_point_table(name):
    fmt = CODES[name]
    for which in ("jh_predictor", "jh_predictor2d"):
        assert N.forward_symbol(which, fmt) == which + PLAIN[name]
        assert N.forward_symbol(which, fmt, per_image=True) == which + "_forward_images"
    masked = "jh_predictor_forward_masked" if fmt < 4 else "jh_predictor" + PLAIN[name]
    assert N.forward_symbol("jh_predictor", fmt, masked=True) == masked
    assert N.forward_symbol("jh_predictor", fmt, masked=True, per_image=True) == "jh_predictor_forward_images"
    assert N.forward_symbol("jh_predictor", fmt) in N.symbols() and N.forward_symbol("jh_predictor2d", fmt) in N.symbols()


class _Recorder:
    """Stands in for the loaded library: every symbol is a function that records its name and arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture()
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(N, "lib", lambda: rec)
    monkeypatch.setattr(N, "stream", lambda: 77)
    return rec


def _frames(name, per_image):
    layout = {"surface": YUV, "sensor": SENSOR}.get(name)
    one = {"rgb": torch.zeros(3, H, W), "bgr": torch.zeros(H, W, 3, dtype=U8)}.get(
        name, torch.zeros(layout.image_stride if layout else (H * 3 // 2, W), dtype=U8))
    if per_image:
        return N.Frames(CODES[name], H, W, layout, (2,), images=[one, one.clone()])
    return N.Frames(CODES[name], H, W, layout, (1, 2), data=torch.stack([one, one])[None])


@pytest.mark.parametrize("name", sorted(CODES))
def test_call_forward_arguments(recorder, name):
    """The arguments between the handle and the outputs, per row of the table (include/jarvis_hip.h)."""
    fmt, outs, mask = CODES[name], (torch.zeros(1), torch.zeros(2), torch.zeros(3)), torch.ones(1, 2, dtype=U8)
    tail = tuple(t.data_ptr() for t in outs) + (77,)
    struct = {"surface": N.YuvSurfaceStruct, "sensor": N.SensorSurfaceStruct}.get(name)
    for which, m in (("jh_predictor", None), ("jh_predictor", mask), ("jh_predictor2d", None)):
        mp = ((None if m is None else m.data_ptr(),) if which == "jh_predictor" else ())
        # one tensor
        f = _frames(name, False)
        del recorder.calls[:]
        N.call_forward(which, 5, f, m, outs)
        (sym, args), = recorder.calls
        assert sym == N.forward_symbol(which, fmt, m is not None) and args[0] == 5 and args[1] == f.data.data_ptr()
        assert args[-4:] == tail
        mid = args[2:-4]
        if struct is not None:
            assert isinstance(mid[0], struct) and mid[1:] == mp
        elif m is not None:
            assert mid == (fmt, m.data_ptr())
        else:
            assert mid == ((fmt,) if name in ("i420", "nv12") else ())
        # per-image
        f = _frames(name, True)
        del recorder.calls[:]
        N.call_forward(which, 5, f, m, outs)
        (sym, args), = recorder.calls
        assert sym == which + "_forward_images" and args[0] == 5 and args[-4:] == tail
        assert [args[1][i] for i in range(2)] == [t.data_ptr() for t in f.images] and args[2:4] == (2, fmt)
        yuv, sensor = args[4:6]
        assert (isinstance(yuv, N.YuvSurfaceStruct) if name == "surface" else yuv is None)
        assert (isinstance(sensor, N.SensorSurfaceStruct) if name == "sensor" else sensor is None)
        assert args[6:-4] == mp
    with pytest.raises(ValueError, match="no camera mask"):
        N.call_forward("jh_predictor2d", 5, _frames(name, False), mask, outs)


def _key(d):
    return d.fmt, d.height, d.width, d.lead, d.layout


def _cases(h=H):
    """(label, tensor, lead argument, frame_format, frame_layout, the expected (fmt, height, width, lead, layout))."""
    rows, y, s = h * 3 // 2, YuvSurface(h, W, "nv12"), SensorSurface(h, W, "rggb")
    z = torch.zeros
    out = []
    for dim, lead_arg, lead in (("3D", (None, C), (T, C)), ("2D", (None,), (T,)), ("3D single", (C,), (C,)),
                                ("3D fixed", (T, C), (T, C))):
        out += [(dim + " fp32", z(lead + (3, h, W)), lead_arg, None, None, (0, h, W, lead, None)),
                (dim + " uint8", z(lead + (h, W, 3), dtype=U8), lead_arg, None, None, (1, h, W, lead, None)),
                (dim + " uint8 'bgr'", z(lead + (h, W, 3), dtype=U8), lead_arg, "bgr", None, (1, h, W, lead, None)),
                (dim + " i420", z(lead + (rows, W), dtype=U8), lead_arg, "i420", None, (2, h, W, lead, None)),
                (dim + " nv12", z(lead + (rows, W), dtype=U8), lead_arg, "nv12", None, (3, h, W, lead, None)),
                (dim + " surface", z(lead + (y.image_stride,), dtype=U8), lead_arg, None, y, (4, h, W, lead, y)),
                (dim + " sensor", z(lead + (s.image_stride,), dtype=U8), lead_arg, "bgr", s, (5, h, W, lead, s))]
    return out


@pytest.mark.parametrize("h", [H, 6])                           # 6: 3H/2 = 9 rows, odd, with H and W even
def test_description_table(h):
    for label, x, lead, ff, layout, want in _cases(h):
        for kw in ({}, {"hw": (h, W)}, {"hw": (h, W), "error": RuntimeError, "in_place": True}):
            d = N.describe_shape(x.shape, x.dtype, lead, ff, layout, **kw)
            assert _key(d) == want and d.data is None and d.images is None, (label, kw)
        # the device comes last: every rule above has passed when a CPU tensor is refused
        with pytest.raises(RuntimeError, match="CPU tensor"):
            N.describe_frames(x, lead, ff, layout)
        with pytest.raises(RuntimeError, match="contiguous CUDA"):
            N.describe_frames(x, lead, ff, layout, (h, W), error=RuntimeError, in_place=True)
    # any other dtype is the fp32 form's, to be converted -- unless the bytes are read in place
    x = torch.zeros((T, C, 3, h, W), dtype=torch.float64)
    assert _key(N.describe_shape(x.shape, x.dtype, (None, C))) == (0, h, W, (T, C), None)
    with pytest.raises(RuntimeError, match="dtype"):
        N.describe_shape(x.shape, x.dtype, (None, C), error=RuntimeError, in_place=True)
    with pytest.raises(ValueError, match="dtype"):
        N.frame_images([x[0, 0]] * 2, 2)


def test_frame_images_description():
    y = YuvSurface(H, W, "nv12")
    for one, ff, layout, want in ((torch.zeros(3, H, W), None, None, (0, H, W, (T, C), None)),
                                  (torch.zeros(H, W, 3, dtype=U8), None, None, (1, H, W, (T, C), None)),
                                  (torch.zeros(6, W, dtype=U8), "i420", None, (2, H, W, (T, C), None)),
                                  (torch.zeros(y.image_stride + 5, dtype=U8), None, y, (4, H, W, (T, C), y))):
        d = N.describe_shape(one.shape, one.dtype, (), ff, layout, in_place=True, at_least=True)
        assert _key(d) == want[:3] + ((), want[4])
        with pytest.raises(RuntimeError, match="CPU tensor"):      # (shape rules passed, lead taken from `count`)
            N.frame_images([one] * (T * C), (T, C), ff, layout)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            N.frame_images([one] * T, T, ff, layout)


def test_refusals():
    """Every refusal of the helpers this description replaced (frame_format, yuv_frame_hw, frame_layout,
    NativePredictor._check_frames, _yuv_frames, _need_surface), with the class each caller gets."""
    z = torch.zeros
    yuv = z((T, C, 6, W), dtype=U8)
    for err, kw in ((ValueError, {}), (RuntimeError, {"hw": (H, W), "error": RuntimeError, "in_place": True})):
        def refuse(x, match, ff=None, layout=None, cls=err, lead=(T, C)):
            with pytest.raises(cls, match=match):
                N.describe_frames(x, lead, ff, layout, **kw)
        for bad in ("I420", "yuv420p", "rgb", "yuyv", 2):                               # unknown format
            refuse(yuv, "frame_format must be one of", bad, cls=ValueError)
        refuse(z((T, C, 3, H, W)), "'bgr' needs uint8", "bgr")                          # 'bgr' with fp32
        refuse(yuv, r"pass frame_format='i420' or 'nv12'")                             # uint8 4-D, no format
        refuse(yuv.float(), "uint8", "i420")                                            # YUV dtype
        refuse(yuv[0], "shape", "i420")                                                 # wrong rank
        refuse(z((T, C, 3, H)), "shape")
        refuse(z((T, C, H, W, 4), dtype=U8), "shape")
        refuse(z((T, C + 1, 3, H, W)), "shape")                                         # another camera count
        refuse(z((T, C, H, W, 3), dtype=U8), "shape", lead=(T + 1, C))
        refuse(list(range(4)), "list")                                                  # no tensor
        for layout in (YUV, SENSOR):
            ok = z((T, C, layout.image_stride), dtype=U8)
            name = type(layout).__name__
            for ff in ("i420", "nv12"):                                                 # layout with a YUV format
                refuse(ok, "do not combine", ff, layout, cls=ValueError)
            for bad in (ok.float(), ok[0], ok[..., :-1], z((T, 1, layout.image_stride), dtype=U8), ok.numpy()):
                refuse(bad, name, None, layout, cls=ValueError)                         # dtype, rank, image_stride
            refuse(ok, "a YuvSurface or a SensorSurface", None, layout.struct(), cls=ValueError)
            refuse(ok, "a YuvSurface or a SensorSurface", None, "nv12", cls=ValueError)
    # sizes that cannot be 4:2:0: odd H (rows no multiple of 3), odd W, nothing -- from the shape, and of a predictor
    for shape in ((7, 10), (12, 9), (0, 4), (2, 3, 7, 4), (2, 6, 5)):
        with pytest.raises(ValueError, match="3H/2"):
            N.describe_shape(shape, U8, (None,) * (len(shape) - 2), "nv12")
    assert tuple(N.describe_shape((12, 10), U8, (), "i420")[:3]) == (2, 8, 10)
    assert tuple(N.describe_shape((2, 3, 1536, 1280), U8, (None, 3), "nv12")[:3]) == (3, 1024, 1280)
    for hw in ((5, 6), (4, 7)):
        with pytest.raises(ValueError, match="even height and width"):
            N.describe_shape((T, C, 6, W), U8, (T, C), "i420", hw=hw)
    for layout in (YUV, SENSOR):                                                        # a layout of another size
        with pytest.raises(ValueError, match="4 x 6"):
            N.describe_shape((T, C, layout.image_stride), U8, (T, C), None, layout, hw=(8, 6))
        assert N.check_layout(layout) is layout and N.check_layout(layout, "bgr", (4, 6)) is layout
        with pytest.raises(ValueError, match="4 x 6"):
            N.check_layout(layout, None, (8, 6))
        with pytest.raises(ValueError, match="a YuvSurface or a SensorSurface"):
            N.check_layout(layout.struct())
    assert N.check_layout(None, "nv12") is None
    # the forms that take one kind of frames only
    assert N.yuv_format("i420") == "i420" and N.surface(YUV) is YUV
    for bad in ("bgr", None, "yv12"):
        with pytest.raises(ValueError, match="frame_format"):
            N.yuv_format(bad)
    with pytest.raises(ValueError, match="surface must be"):
        N.surface(None)


class _Owner:
    """What a public method may touch of its predictor before its checks are through: `num_cameras`.  Reaching for
    anything else, the native predictor included, fails the test."""
    num_cameras = C

    def __getattr__(self, name):
        raise AssertionError("reached for %r before the arguments were checked" % name)


@pytest.fixture()
def owners(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a native call was made before the arguments were checked")
    monkeypatch.setattr(N, "lib", boom)
    p3, p2 = _Owner(), _Owner()
    for name in ("forward", "forward_uint8", "forward_yuv", "forward_surface", "forward_batch"):
        setattr(p3, name, MethodType(getattr(JarvisPredictor3D, name), p3))
        if hasattr(JarvisPredictor2D, name):
            setattr(p2, name, MethodType(getattr(JarvisPredictor2D, name), p2))
    p3._frame_mask = MethodType(JarvisPredictor3D._frame_mask, p3)
    return p3, p2


def test_checks_come_first(owners):
    p3, p2 = owners
    z, calib = torch.zeros, (None, None, None)
    ok3, ok2 = z((T, C, 6, W), dtype=U8), z((T, 6, W), dtype=U8)
    sur3, sur2 = z((T, C, YUV.image_stride), dtype=U8), z((T, YUV.image_stride), dtype=U8)
    # forward_batch
    with pytest.raises(ValueError, match="frame_format must be one of"):
        p3.forward_batch(ok3, *calib, frame_format="yuyv")
    with pytest.raises(ValueError, match="pass frame_format='i420' or 'nv12'"):
        p3.forward_batch(ok3, *calib)
    with pytest.raises(ValueError, match="'bgr' needs uint8"):
        p3.forward_batch(z((T, C, 3, H, W)), *calib, frame_format="bgr")
    with pytest.raises(ValueError, match="shape"):
        p3.forward_batch(z((T, C + 1, 3, H, W)), *calib)
    with pytest.raises(ValueError, match="3H/2"):
        p3.forward_batch(z((T, C, 7, W), dtype=U8), *calib, frame_format="i420")
    with pytest.raises(ValueError, match="do not combine"):
        p3.forward_batch(sur3, *calib, frame_format="nv12", frame_layout=YUV)
    with pytest.raises(ValueError, match="YuvSurface"):
        p3.forward_batch(sur3[..., :-1], *calib, frame_layout=YUV)
    with pytest.raises(ValueError, match="camera_mask"):
        p3.forward_batch(ok3, *calib, frame_format="i420", camera_mask=[[1, 1]])
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p3.forward_batch(ok3, *calib, frame_format="i420", camera_mask=[[1, 1, 0]] * T)
    with pytest.raises(ValueError, match="pass frame_format='i420' or 'nv12'"):
        p2.forward_batch(ok2)
    with pytest.raises(ValueError, match="'bgr' needs uint8"):
        p2.forward_batch(z((T, 3, H, W)), frame_format="bgr")
    with pytest.raises(ValueError, match="do not combine"):
        p2.forward_batch(sur2, frame_format="i420", frame_layout=YUV)
    with pytest.raises(ValueError, match="SensorSurface"):
        p2.forward_batch(sur2, frame_layout=SENSOR.struct())
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p2.forward_batch(ok2, frame_format="nv12")
    # forward_yuv
    with pytest.raises(ValueError, match="frame_format"):
        p3.forward_yuv(ok3[0], "bgr", *calib)
    with pytest.raises(ValueError, match="uint8"):
        p3.forward_yuv(ok3[0].float(), "i420", *calib)
    with pytest.raises(ValueError, match="shape"):
        p3.forward_yuv(ok3, "i420", *calib)
    with pytest.raises(ValueError, match="3H/2"):
        p3.forward_yuv(z((C, 6, 5), dtype=U8), "nv12", *calib)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p3.forward_yuv(ok3[0], "nv12", *calib)
    with pytest.raises(ValueError, match="frame_format"):
        p2.forward_yuv(ok2[0], "bgr")
    with pytest.raises(ValueError, match="3H/2"):
        p2.forward_yuv(z((7, W), dtype=U8), "i420")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p2.forward_yuv(ok2[0], "i420")
    # forward_surface
    with pytest.raises(ValueError, match="surface must be"):
        p3.forward_surface(sur3[0], None, *calib)
    with pytest.raises(ValueError, match="a YuvSurface or a SensorSurface"):
        p3.forward_surface(sur3[0], YUV.struct(), *calib)
    with pytest.raises(ValueError, match="YuvSurface"):
        p3.forward_surface(sur3[0, :-1], YUV, *calib)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p3.forward_surface(sur3[0], YUV, *calib)
    with pytest.raises(ValueError, match="surface must be"):
        p2.forward_surface(sur2[0], None)
    with pytest.raises(ValueError, match="SensorSurface"):
        p2.forward_surface(sur2, SENSOR)                                # (T, image_stride): one image only
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p2.forward_surface(sur2[0], YUV)
    # the single-frame fp32 / uint8 forms
    with pytest.raises(ValueError, match="shape"):
        p3.forward(z((C + 1, 3, H, W)), *calib)
    with pytest.raises(ValueError, match="'bgr' needs uint8"):
        p3.forward_uint8(z((C, H, W, 3)), *calib)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p3.forward(z((C, 3, H, W)), *calib)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p2.forward(z((1, 3, H, W)))
