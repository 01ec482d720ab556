"""No GPU: the per-image frame pointers (jh_predictor_forward_images / JarvisPredictor*.forward_images) at the two
places that need none -- the ABI tables, and the Python checks, which raise before any native call is made."""
import re

import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import _native as N
from jarvis_hybridnet_amd import synthetic as S
from tests.test_native_abi import header_symbols

NEW = ("jh_predictor_forward_images", "jh_predictor2d_forward_images")
H, W, C = 32, 48, 3


def test_symbols_in_header_and_ctypes_table():
    names = header_symbols()
    for name in NEW:
        assert name in names and name in N.symbols(), name
    lib = N.lib()
    assert lib.jh_abi_version() == N.ABI_VERSION == 4
    for name in NEW:
        assert hasattr(lib, name), name
    text = open(N.os.path.join(N._HERE, "..", "include", "jarvis_hip.h")).read()
    codes = dict(re.findall(r"#define JH_FRAME_(\w+)\s+(\d+)", text))
    assert codes["SURFACE"] == "4" and codes["SENSOR"] == "5" and len(codes) == 6
    assert (N.FRAME_SURFACE, N.FRAME_SENSOR) == (4, 5)


@pytest.fixture()
def no_native(monkeypatch):
    """Any use of the library from here on fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("a native call was made before the arguments were checked")
    monkeypatch.setattr(N, "lib", boom)


def bgr(n, h=H, w=W):
    return [torch.zeros((h, w, 3), dtype=torch.uint8) for _ in range(n)]


def test_frame_images_checks(no_native):
    with pytest.raises(ValueError, match="sequence of 3 images"):
        N.frame_images(bgr(2), 3)
    with pytest.raises(ValueError, match="sequence of 3 images"):
        N.frame_images(torch.zeros((3, H, W, 3), dtype=torch.uint8), 3)
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        N.frame_images(bgr(2) + bgr(1, H + 2), 3)
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        N.frame_images(bgr(2) + [torch.zeros((H, W, 3), dtype=torch.int8)], 3)
    with pytest.raises(ValueError, match="not a tensor"):
        N.frame_images(bgr(2) + [None], 3)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        N.frame_images(bgr(3), 3)
    nc = [torch.zeros((H, 2 * W, 3), dtype=torch.uint8)[:, ::2] for _ in range(3)]
    assert not nc[0].is_contiguous()
    with pytest.raises(RuntimeError, match="not contiguous"):
        N.frame_images(nc, 3)
    for layout in (YuvSurface(H, W, "nv12"), SensorSurface(H, W, "rggb")):
        with pytest.raises(ValueError, match="do not combine"):
            N.frame_images([torch.zeros(layout.image_stride, dtype=torch.uint8)] * 3, 3, "nv12", layout)
        with pytest.raises(ValueError, match="at least image_stride"):
            N.frame_images([torch.zeros(layout.image_stride - 1, dtype=torch.uint8)] * 3, 3, None, layout)
    with pytest.raises(ValueError, match="frame_format must be one of"):
        N.frame_images(bgr(3), 3, "yuyv")
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        N.frame_images([torch.zeros((H * 3 // 2, W), dtype=torch.uint8)] * 3, 3)
    with pytest.raises(ValueError, match="3H/2"):
        N.frame_images([torch.zeros((H * 3 // 2 + 1, W), dtype=torch.uint8)] * 3, 3, "i420")
    with pytest.raises(ValueError, match="'bgr' needs uint8"):
        N.frame_images([torch.zeros((3, H, W))] * 3, 3, "bgr")
    with pytest.raises(ValueError, match=r"\(3, H, W\)"):
        N.frame_images([torch.zeros((H, W, 3))] * 3, 3)


def test_layout_args_and_table(monkeypatch):
    """(table, n, fmt, yuv, sensor) of jh_predictor*_forward_images as _native.call_forward hands them over: the
    struct the format needs, NULL for the other, and the images' own addresses."""
    seen = []
    monkeypatch.setattr(N, "lib", lambda: type("L", (), {"__getattr__": lambda self, name: lambda *a: seen.append(a) or 0})())
    monkeypatch.setattr(N, "stream", lambda: 0)

    def layout_args(fmt, layout, imgs):
        del seen[:]
        N.call_forward("jh_predictor2d", None, N.Frames(fmt, H, W, layout, (len(imgs),), images=imgs), None, ())
        assert seen[0][2:4] == (len(imgs), fmt)
        return seen[0][1], seen[0][4:6]
    y, s = YuvSurface(H, W, "nv12"), SensorSurface(H, W, "mono")
    imgs = bgr(3)
    tab, a = layout_args(N.FRAME_SURFACE, y, imgs)
    assert isinstance(a[0], N.YuvSurfaceStruct) and a[1] is None
    _, a = layout_args(N.FRAME_SENSOR, s, imgs)
    assert a[0] is None and isinstance(a[1], N.SensorSurfaceStruct)
    assert layout_args(N.FRAME_FORMATS["bgr"], None, imgs)[1] == (None, None)
    assert [tab[i] for i in range(3)] == [t.data_ptr() for t in imgs]


class _Owner:
    """What forward_images touches of a predictor before its checks are through (a predictor itself needs a GPU to be
    built): reaching for anything else, the native predictor included, fails the test."""
    num_cameras = C

    def __getattr__(self, name):
        raise AssertionError("forward_images reached for %r before the arguments were checked" % name)


@pytest.fixture()
def predictors():
    from types import MethodType

    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    p3, p2 = _Owner(), _Owner()
    p3.forward_images = MethodType(JarvisPredictor3D.forward_images, p3)
    p2.forward_images = MethodType(JarvisPredictor2D.forward_images, p2)
    return p3, p2


def test_predictor_checks_come_before_any_native_call(predictors, no_native):
    p3, p2 = predictors
    calib = S.ring_calibration(C, W, H, 100.0)
    with pytest.raises(ValueError, match="one per camera"):
        p3.forward_images(bgr(C - 1), *calib)
    with pytest.raises(ValueError, match="one per camera"):
        p3.forward_images([bgr(C), bgr(C + 1)], *calib)
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        p3.forward_images([bgr(C), bgr(C - 1) + bgr(1, H, W + 2)], *calib)
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        p3.forward_images(bgr(C - 1) + [torch.zeros((H, W, 3))], *calib)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p3.forward_images(bgr(C), *calib)
    with pytest.raises(RuntimeError, match="not contiguous"):
        p3.forward_images([torch.zeros((H, 2 * W, 3), dtype=torch.uint8)[:, ::2] for _ in range(C)], *calib)
    layout = YuvSurface(H, W, "nv12")
    flat = [torch.zeros(layout.image_stride, dtype=torch.uint8) for _ in range(C)]
    with pytest.raises(ValueError, match="do not combine"):
        p3.forward_images(flat, *calib, frame_format="nv12", frame_layout=layout)
    with pytest.raises(ValueError, match="sequence"):
        p3.forward_images(torch.zeros((C, H, W, 3), dtype=torch.uint8), *calib)
    # the 2D predictor: T images
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        p2.forward_images(bgr(2) + bgr(1, H + 2))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        p2.forward_images(bgr(3))
    with pytest.raises(ValueError, match="do not combine"):
        p2.forward_images(flat, frame_format="nv12", frame_layout=layout)
    with pytest.raises(ValueError, match="non-empty sequence"):
        p2.forward_images([])
