"""CPU: pixel surfaces (PixelSurface / jh_pixel_surface).  The description's rules in Python and in the library's own
check, the FFmpeg names against hand-written field values, the numpy reference (synthetic.pixels_to_bgr) and the packer
(synthetic.pack_pixel_surface) the GPU tests compare against, and the shape rules of the frames."""
import ctypes
import os

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import PixelSurface, YuvSurface
from jarvis_hybridnet_amd import pixel_surface as M
from jarvis_hybridnet_amd import synthetic as S
from tests.test_yuv_surface_cpu import ROWS, surface_to_bgr

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)

# A good 6 x 10 description of each colour, as from_components' keywords
RGB = dict(height=6, width=10, image_stride=180, offset=(0, 1, 2), pitch=(30, 30, 30), step=(3, 3, 3))
YUV = dict(height=6, width=10, image_stride=120, offset=(0, 1, 3), pitch=(20, 20, 20), step=(2, 4, 4), xs=(0, 1, 1),
           ys=(0, 0, 0), colour="yuv", matrix="bt601", range="limited")

# (base, what changes in Python, what the same change is in the C struct (None: the same), the rule's words in the
#  Python message, in the C message).  Every row breaks exactly one rule.
BAD = [
    (RGB, dict(height=0), None, "positive height and width", "positive height and width"),
    (RGB, dict(width=-3), None, "positive height and width", "positive height and width"),
    (RGB, dict(colour="cmyk"), dict(colour=7), "colour must be", "colour: unknown"),
    (YUV, dict(matrix="bt2020"), dict(matrix=5), "matrix must be", "matrix: unknown"),
    (YUV, dict(range="video"), dict(range=-1), "range must be", "range: unknown"),
    (RGB, dict(matrix="bt709", range="limited"), dict(matrix=1), "must be None for 'rgb'", "must be 0 for JH_PIXEL_RGB"),
    (RGB, dict(range="full", matrix="bt601"), dict(range=1), "must be None for 'rgb'", "must be 0 for JH_PIXEL_RGB"),
    (RGB, dict(sample=0x102), None, "sample must be 0", "sample must be JH_SAMPLE_U8"),
    (RGB, dict(sample=0x200), None, "sample must be 0", "sample must be JH_SAMPLE_U8"),
    (RGB, dict(step=(3, 0, 3)), None, "step must be 1 .. 8", "step must be 1 .. 8"),
    (RGB, dict(step=(9, 3, 3), pitch=(100, 30, 30), image_stride=1000), None, "step must be 1 .. 8", "step must be 1 .. 8"),
    (YUV, dict(xs=(0, 3, 3)), None, "xs and ys must be 0 .. 2", "xs and ys must be 0 .. 2"),
    (YUV, dict(ys=(0, -1, -1)), None, "xs and ys must be 0 .. 2", "xs and ys must be 0 .. 2"),
    (RGB, dict(xs=(0, 1, 1)), None, "R, G and B are not subsampled", "R, G and B are not subsampled"),
    (RGB, dict(ys=(1, 1, 1)), None, "R, G and B are not subsampled", "R, G and B are not subsampled"),
    (YUV, dict(xs=(1, 1, 1)), None, "Y is not subsampled", "Y is not subsampled"),
    (YUV, dict(xs=(0, 1, 0), pitch=(20, 20, 40)), None, "subsampled alike", "subsampled alike"),
    (YUV, dict(ys=(0, 0, 1)), None, "subsampled alike", "subsampled alike"),
    (RGB, dict(offset=(0, -1, 2)), None, "offsets must not be negative", "offset must not be negative"),
    (RGB, dict(offset=(I64_MIN, 1, 2)), None, "offsets must not be negative", "offset must not be negative"),
    (RGB, dict(pitch=(30, 27, 30)), None, "smaller than a row", "smaller than a row"),
    (YUV, dict(pitch=(20, 16, 20)), None, "smaller than a row", "smaller than a row"),
    (RGB, dict(pitch=(30, I64_MIN, 30)), None, "smaller than a row", "smaller than a row"),
    (RGB, dict(image_stride=179), None, "ends beyond image_stride", "ends beyond image_stride"),
    (RGB, dict(offset=(0, 1, 3)), None, "ends beyond image_stride", "ends beyond image_stride"),
    (RGB, dict(image_stride=I64_MIN), None, "ends beyond image_stride", "ends beyond image_stride"),
    # (spans that wrap in 64 bits: the check may not)
    (RGB, dict(pitch=(I64_MAX,) * 3, image_stride=I64_MAX), None, "ends beyond image_stride", "ends beyond image_stride"),
    (RGB, dict(offset=(I64_MAX, 1, 2), image_stride=I64_MAX), None, "ends beyond image_stride", "ends beyond image_stride"),
]
GOOD = [
    (RGB, {}), (YUV, {}),
    (RGB, dict(image_stride=I64_MAX)),
    (RGB, dict(height=1, width=1, pitch=(1, 1, 1), offset=(I64_MAX - 1,) * 3, image_stride=I64_MAX)),
    (RGB, dict(height=1, pitch=(I64_MAX,) * 3)),            # (a pitch no row is ever stepped by)
    (YUV, dict(height=5, width=9)),                         # odd sizes: the planes are ceil wide / high
    (YUV, dict(xs=(0, 2, 2), ys=(0, 2, 2), step=(2, 8, 8))),
]


def c_struct(kw, c_over):
    """The jh_pixel_surface of from_components' keywords `kw`, the fields of c_over replaced -- built field by field,
    so that a description Python refuses can still be shown to the C check."""
    from jarvis_hybridnet_amd import _native as N
    st = N.PixelSurfaceStruct()
    st.image_stride = kw["image_stride"]
    for k in range(3):
        st.offset[k], st.pitch[k], st.step[k] = kw["offset"][k], kw["pitch"][k], kw["step"][k]
        st.xs[k], st.ys[k] = kw.get("xs", (0, 0, 0))[k], kw.get("ys", (0, 0, 0))[k]
    st.colour = M.COLOURS.get(kw.get("colour", "rgb"), 0)
    st.matrix = M.MATRICES.get(kw.get("matrix"), 0)
    st.range = M.RANGES.get(kw.get("range"), 0)
    st.sample = kw.get("sample", 0)
    for name, v in (c_over or {}).items():
        setattr(st, name, v)
    return st


def test_python_and_c_validation_agree():
    from jarvis_hybridnet_amd import _native as N
    lib = N.lib()
    for base, change in GOOD:
        kw = dict(base, **change)
        s = PixelSurface.from_components(**kw)
        assert lib.jh_pixel_surface_check(ctypes.byref(s.struct()), kw["height"], kw["width"]) == 0, \
            (kw, lib.jh_last_error())
        assert bytes(s.struct()) == bytes(c_struct(kw, None))
    seen_py, seen_c = set(), set()
    for base, change, c_over, py_words, c_words in BAD:
        kw = dict(base, **change)
        with pytest.raises(ValueError, match=py_words):
            PixelSurface.from_components(**kw)
        st = c_struct(kw, c_over)
        assert lib.jh_pixel_surface_check(ctypes.byref(st), kw["height"], kw["width"]) != 0, kw
        assert c_words in lib.jh_last_error().decode(), (kw, lib.jh_last_error())
        seen_py.add(py_words)
        seen_c.add(c_words)
    # every rule of the header's list has its row: 13 rules, the one on the YUV shifts quoted by either half
    assert len(seen_c) == 14 and len(seen_py) == 14
    assert lib.jh_pixel_surface_check(None, 6, 10) != 0 and b"null" in lib.jh_last_error()


def test_what_only_python_can_refuse():
    for change in (dict(image_stride=1 << 63), dict(offset=(0, 1.5, 2)), dict(pitch=(30, 30)), dict(step=(3, 3, 1 << 31)),
                   dict(height=True), dict(width=2.0), dict(sample=None), dict(offset=(0, 1, True))):
        with pytest.raises(ValueError):
            PixelSurface.from_components(**dict(RGB, **change))
    with pytest.raises(TypeError):
        PixelSurface(6, 10)


# name -> (offset, pitch, step, xs, ys, colour, range, image_stride) of a tight 5 x 7 image, written by hand:
# 35 = 5 * 7 luma bytes; ceil(7/2) = 4, ceil(7/4) = 2, ceil(5/2) = 3
Z = (0, 0, 0)
PIX_FMT_5x7 = {
    "rgb24": ((0, 1, 2), (21,) * 3, (3,) * 3, Z, Z, "rgb", None, 105),
    "bgr24": ((2, 1, 0), (21,) * 3, (3,) * 3, Z, Z, "rgb", None, 105),
    "rgba": ((0, 1, 2), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "bgra": ((2, 1, 0), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "argb": ((1, 2, 3), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "abgr": ((3, 2, 1), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "rgb0": ((0, 1, 2), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "bgr0": ((2, 1, 0), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "0rgb": ((1, 2, 3), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "0bgr": ((3, 2, 1), (28,) * 3, (4,) * 3, Z, Z, "rgb", None, 140),
    "gbrp": ((70, 0, 35), (7,) * 3, (1,) * 3, Z, Z, "rgb", None, 105),
    "gray": ((0, 0, 0), (7,) * 3, (1,) * 3, Z, Z, "rgb", None, 35),
    "yuyv422": ((0, 1, 3), (16,) * 3, (2, 4, 4), (0, 1, 1), Z, "yuv", "limited", 80),
    "uyvy422": ((1, 0, 2), (16,) * 3, (2, 4, 4), (0, 1, 1), Z, "yuv", "limited", 80),
    "yvyu422": ((0, 3, 1), (16,) * 3, (2, 4, 4), (0, 1, 1), Z, "yuv", "limited", 80),
    "yuv422p": ((0, 35, 55), (7, 4, 4), (1,) * 3, (0, 1, 1), Z, "yuv", "limited", 75),
    "yuvj422p": ((0, 35, 55), (7, 4, 4), (1,) * 3, (0, 1, 1), Z, "yuv", "full", 75),
    "nv16": ((0, 35, 36), (7, 8, 8), (1, 2, 2), (0, 1, 1), Z, "yuv", "limited", 75),
    "yuv444p": ((0, 35, 70), (7,) * 3, (1,) * 3, Z, Z, "yuv", "limited", 105),
    "yuvj444p": ((0, 35, 70), (7,) * 3, (1,) * 3, Z, Z, "yuv", "full", 105),
    "nv24": ((0, 35, 36), (7, 14, 14), (1, 2, 2), Z, Z, "yuv", "limited", 105),
    "yuv440p": ((0, 35, 56), (7,) * 3, (1,) * 3, Z, (0, 1, 1), "yuv", "limited", 77),
    "yuvj440p": ((0, 35, 56), (7,) * 3, (1,) * 3, Z, (0, 1, 1), "yuv", "full", 77),
    "yuv411p": ((0, 35, 45), (7, 2, 2), (1,) * 3, (0, 2, 2), Z, "yuv", "limited", 55),
    "yuv420p": ((0, 35, 47), (7, 4, 4), (1,) * 3, (0, 1, 1), (0, 1, 1), "yuv", "limited", 59),
    "yuvj420p": ((0, 35, 47), (7, 4, 4), (1,) * 3, (0, 1, 1), (0, 1, 1), "yuv", "full", 59),
    "nv12": ((0, 35, 36), (7, 8, 8), (1, 2, 2), (0, 1, 1), (0, 1, 1), "yuv", "limited", 59),
    "nv21": ((0, 36, 35), (7, 8, 8), (1, 2, 2), (0, 1, 1), (0, 1, 1), "yuv", "limited", 59),
}


def test_from_pix_fmt_field_values():
    assert set(PIX_FMT_5x7) == set(M.PIX_FMTS)
    for name, (off, pitch, step, xs, ys, colour, rng, stride) in PIX_FMT_5x7.items():
        s = PixelSurface.from_pix_fmt(5, 7, name)
        assert (s.offset, s.pitch, s.step, s.xs, s.ys, s.colour, s.range, s.image_stride) == \
            (off, pitch, step, xs, ys, colour, rng, stride), name
        assert s.matrix == ("bt601" if colour == "yuv" else None) and (s.height, s.width, s.sample) == (5, 7, 0)
    # linesize: an AVFrame copied plane by plane
    s = PixelSurface.from_pix_fmt(5, 7, "yuv422p", linesize=(32, 16, 16))
    assert (s.offset, s.pitch, s.image_stride) == ((0, 160, 240), (32, 16, 16), 320)
    s = PixelSurface.from_pix_fmt(5, 7, "nv16", linesize=(32, 32))
    assert (s.offset, s.pitch, s.image_stride) == ((0, 160, 161), (32, 32, 32), 320)
    s = PixelSurface.from_pix_fmt(5, 7, "bgra", linesize=[64])
    assert (s.offset, s.pitch, s.image_stride) == ((2, 1, 0), (64, 64, 64), 320)
    with pytest.raises(ValueError, match="known: .*yuyv422"):
        PixelSurface.from_pix_fmt(5, 7, "yuv420p10le")
    for name, ls in (("yuv422p", (32, 16)), ("yuv422p", (32, 16, 32)), ("gbrp", (8, 8, 16)), ("rgb24", (20,)),
                     ("rgb24", 21)):
        with pytest.raises(ValueError):
            PixelSurface.from_pix_fmt(5, 7, name, linesize=ls)


def test_constructors():
    P = PixelSurface
    assert P.packed(5, 7, "rgb") == P.from_pix_fmt(5, 7, "rgb24") != P.packed(5, 7, "bgr")
    s = P.packed(6, 10, "bgra", pitch=46, offset=9, image_stride=9 + 6 * 46 + 10)
    assert (s.offset, s.pitch, s.step, s.image_stride) == ((11, 10, 9), (46,) * 3, (4,) * 3, 295)
    assert P.packed(6, 10, "xbgr").offset == (3, 2, 1)
    s = P.planar(6, 10, "rgb", pitch=16, plane_rows=8, offset=4)
    assert (s.offset, s.pitch, s.image_stride) == ((4, 132, 260), (16,) * 3, 4 + 3 * 128)
    assert P.planar(5, 7, "gbr") == P.from_pix_fmt(5, 7, "gbrp")
    assert P.gray(6, 10, pitch=12, offset=3).offset == (3, 3, 3)
    s = P.yuv_packed(6, 9, "uyvy", matrix="bt709", range="full", pitch=24, offset=2)
    assert (s.offset, s.pitch, s.matrix, s.range, s.image_stride) == ((3, 2, 4), (24,) * 3, "bt709", "full", 2 + 144)
    s = P.yuv_planar(6, 10, "420", semi="vu", y_pitch=16, c_pitch=12, luma_rows=8)
    assert (s.offset, s.pitch, s.step, s.image_stride) == ((0, 129, 128), (16, 12, 12), (1, 2, 2), 128 + 36)
    for bad in (lambda: P.packed(6, 10, "rgbb"), lambda: P.packed(6, 10, "rg"), lambda: P.packed(6, 10, "rgbaa"),
                lambda: P.packed(6, 10, "rgbq"), lambda: P.planar(6, 10, "rgba"), lambda: P.planar(6, 10, plane_rows=5),
                lambda: P.yuv_packed(6, 10, "vyuy"), lambda: P.yuv_planar(6, 10, "410"),
                lambda: P.yuv_planar(6, 10, "422", semi="u"), lambda: P.yuv_planar(6, 10, luma_rows=5),
                lambda: P.packed(6, 10, "rgb", pitch=29), lambda: P.gray(6, 10, pitch=1.5),
                lambda: P.yuv_packed(6, 10, matrix="bt2020")):
        with pytest.raises(ValueError):
            bad()


def test_immutable_hashable_fieldwise_equal():
    a, b = PixelSurface.packed(6, 10, "bgra"), PixelSurface.from_pix_fmt(6, 10, "bgra")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and a is not b
    assert a != PixelSurface.packed(6, 10, "rgba") and a != PixelSurface.packed(6, 12, "bgra") and a != "bgra"
    assert a != PixelSurface.packed(6, 10, "bgra", image_stride=241)
    y = PixelSurface.yuv_packed(6, 10)
    assert y != PixelSurface.yuv_packed(6, 10, range="full") and y != PixelSurface.yuv_packed(6, 10, matrix="bt709")
    for name in M._FIELDS:
        with pytest.raises(AttributeError):
            setattr(a, name, getattr(a, name))
    with pytest.raises(AttributeError):
        del a.height
    with pytest.raises(AttributeError):
        a.extra = 1
    assert "offset=(2, 1, 0)" in repr(a)


def named_layouts(H, W):
    """Every named layout (the FFmpeg names), tight and pitched: pitched is the first byte at offset 9, every pitch
    padded by 6 bytes and a 10-byte tail behind the last row; the pitched YUV layouts are BT.709."""
    P = PixelSurface
    out = {}
    for name, (kind, arg, _) in M.PIX_FMTS.items():
        out[name] = P.from_pix_fmt(H, W, name)
        if kind == "packed":
            pitch = W * len(arg) + 6
            s = P.packed(H, W, arg, pitch=pitch, offset=9, image_stride=9 + H * pitch + 10)
        elif kind == "gray":
            s = P.gray(H, W, pitch=W + 6, offset=9, image_stride=9 + H * (W + 6) + 10)
        elif kind == "yuv_packed":
            pitch = 4 * ((W + 1) // 2) + 6
            s = P.yuv_packed(H, W, arg, matrix="bt709", pitch=pitch, offset=9, image_stride=9 + H * pitch + 10)
        elif kind == "planar":
            s = P.planar(H, W, arg, pitch=W + 6, offset=9, image_stride=9 + 3 * H * (W + 6) + 10)
        else:
            sub, semi, rng = arg
            kw = dict(subsampling=sub, semi=semi, matrix="bt709", range=rng, y_pitch=W + 6,
                      c_pitch=out[name].pitch[1] + 6, offset=9)
            s = P.yuv_planar(H, W, image_stride=P.yuv_planar(H, W, **kw).image_stride + 10, **kw)
        out[name + "_pitched"] = s
    return out


def random_content(g, s, n=3):
    """Random content for a description: BGR (n,H,W,3) for 'rgb' (grey: one value per pixel), planes for 'yuv'."""
    H, W = s.height, s.width
    if s.colour == "rgb":
        bgr = g.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        if len(set(s.offset)) == 1:
            bgr[..., 0] = bgr[..., 2] = bgr[..., 1]
        return bgr
    return [g.integers(0, 256, (n, ((H - 1) >> s.ys[k]) + 1, ((W - 1) >> s.xs[k]) + 1), dtype=np.uint8)
            for k in range(3)]


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (6, 10)])
def test_named_layouts_are_valid_and_disjoint(H, W):
    for name, s in named_layouts(H, W).items():
        idx = [S._component_index(s, k) for k in range(3)]
        assert all(i.min() >= 0 and i.max() < s.image_stride for i in idx), name
        if name.endswith("_pitched"):
            assert min(i.min() for i in idx) in (9, 10) and max(i.max() for i in idx) < s.image_stride - 10, name
        if not name.startswith("gray"):                     # no byte belongs to two components
            planes = [np.unique(i) for i in idx]
            assert len(np.unique(np.concatenate(planes))) == sum(len(p) for p in planes), name


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (6, 10)])
def test_pack_then_convert_is_the_identity_for_rgb(H, W):
    g = np.random.default_rng(H * 100 + W)
    n = 0
    for name, s in named_layouts(H, W).items():
        if s.colour != "rgb":
            continue
        bgr = random_content(g, s)
        for fill in (0xA5, 0x5A):
            assert np.array_equal(S.pixels_to_bgr(S.pack_pixel_surface(bgr, s, fill), s), bgr), (name, fill)
        n += 1
    assert n == 24
    with pytest.raises(ValueError):
        S.pack_pixel_surface(np.zeros((H + 1, W, 3), np.uint8), PixelSurface.packed(H, W, "rgb"))
    with pytest.raises(ValueError):
        S.pixels_to_bgr(np.zeros((7,), np.uint8), PixelSurface.packed(2, 2, "rgb"))


@pytest.mark.parametrize("matrix,rng", list(ROWS))
def test_444_equals_the_per_pixel_yuv_surface_conversion(matrix, rng):
    """A 4:4:4 image converts as the 4:2:0 surface does whose 2 x 2 blocks hold the same (Y, U, V): the YuvSurface
    reference (tests/test_yuv_surface_cpu.py) on the twice-as-large I420 image, every second pixel taken."""
    H, W = 8, 12
    g = np.random.default_rng(5)
    y, u, v = g.integers(0, 256, (3, 2, H, W), dtype=np.uint8)
    y[0, 0, :4], u[0, 0, :4], v[0, 0, :4] = (0, 255, 16, 235), (0, 255, 255, 0), (255, 0, 255, 0)    # the clamps
    s = PixelSurface.yuv_planar(H, W, "444", matrix=matrix, range=rng)
    got = S.pixels_to_bgr(S.pack_pixel_surface((y, u, v), s), s)
    big = YuvSurface(2 * H, 2 * W, "i420", matrix=matrix, range=rng)
    y2 = np.repeat(np.repeat(y, 2, axis=-2), 2, axis=-1)
    want = surface_to_bgr(S.pack_yuv_surface(y2, u, v, big), big)[..., ::2, ::2, :]
    assert np.array_equal(got, want)
    assert s.coefficients == big.coefficients
    # the same triples through a packed 4:2:2 and a 4:1:1 description whose chroma is constant per group
    for sub, k in (("422", 2), ("411", 4)):
        s2 = PixelSurface.yuv_planar(H, W, sub, matrix=matrix, range=rng)
        uu, vv = u[..., ::k], v[..., ::k]
        want2 = S.pixels_to_bgr(S.pack_pixel_surface((y, np.repeat(uu, k, -1), np.repeat(vv, k, -1)), s), s)
        assert np.array_equal(S.pixels_to_bgr(S.pack_pixel_surface((y, uu, vv), s2), s2), want2), sub


def test_odd_sizes_address_ceil_sized_planes():
    """5 x 7: chroma planes of ceil size, and the last row / column's chroma is the last sample of the plane."""
    H, W = 5, 7
    g = np.random.default_rng(11)
    for name, cshape in (("yuv422p", (5, 4)), ("yuv420p", (3, 4)), ("yuv411p", (5, 2)), ("yuv440p", (3, 7)),
                         ("nv16", (5, 4)), ("nv12", (3, 4)), ("yuyv422", (5, 4))):
        s = PixelSurface.from_pix_fmt(H, W, name)
        planes = random_content(g, s, 2)
        assert planes[1].shape[1:] == cshape, name
        buf = S.pack_pixel_surface(planes, s, 0xEE)
        got = S.pixels_to_bgr(buf, s)
        # reference: replicate the chroma to full size, crop to 5 x 7, convert as 4:4:4
        full = PixelSurface.yuv_planar(H, W, "444")
        up = [np.repeat(np.repeat(p, 1 << s.ys[1], -2), 1 << s.xs[1], -1)[..., :H, :W] for p in planes[1:]]
        want = S.pixels_to_bgr(S.pack_pixel_surface((planes[0], up[0], up[1]), full), full)
        assert np.array_equal(got, want), name
        # the corner pixel reads the corner sample of every plane
        p2 = [p.copy() for p in planes]
        p2[1][..., -1, -1] ^= 0x80
        assert not np.array_equal(S.pixels_to_bgr(S.pack_pixel_surface(p2, s), s)[..., -1, -1, :], got[..., -1, -1, :])
    with pytest.raises(ValueError):
        S.pack_pixel_surface([np.zeros((5, 7), np.uint8), np.zeros((5, 3), np.uint8), np.zeros((5, 3), np.uint8)],
                             PixelSurface.from_pix_fmt(5, 7, "yuv422p"))


def test_yuyv_reference_against_the_formula():
    """One YUYV group by hand: BT.601 limited, (Y0, U, Y1, V) = (81, 90, 145, 240) -> both pixels share U and V."""
    s = PixelSurface.yuv_packed(1, 2, "yuyv")
    buf = np.array([[81, 90, 145, 240]], np.uint8)
    y0, cy, cvr, cub, cug, cvg = s.coefficients

    def px(Y):
        yy = max(Y - y0, 0) * cy + (1 << 19)
        u, v = 90 - 128, 240 - 128
        c = lambda x: min(max(x >> 20, 0), 255)             # noqa: E731
        return [c(yy + cub * u), c(yy + cvg * v + cug * u), c(yy + cvr * v)]
    assert S.pixels_to_bgr(buf, s)[0, 0].tolist() == [px(81), px(145)]
    assert S.pixels_to_bgr(buf, PixelSurface.yuv_packed(1, 2, "uyvy"))[0, 0, 0].tolist() != px(81)


def test_frame_shape_rules():
    from jarvis_hybridnet_amd import _native as N
    H, W = 6, 10
    rgb, planar, yuyv = PixelSurface.packed(H, W, "rgb"), PixelSurface.planar(H, W), PixelSurface.yuv_packed(H, W)
    u8 = torch.uint8
    # lead + (image_stride,), and for this layout any trailing shape of exactly image_stride bytes
    for s, shape in ((rgb, (2, 4, 180)), (rgb, (2, 4, H, W, 3)), (planar, (2, 4, 3, H, W)), (yuyv, (2, 4, H, 20)),
                     (PixelSurface.packed(H, W, "bgra"), (2, 4, H, W, 4))):
        d = N.describe_shape(shape, u8, (None, 4), frame_layout=s)
        assert (d.fmt, d.height, d.width, d.layout, d.lead) == (N.FRAME_PIXELS, H, W, s, (2, 4))
    for s, shape, dtype in ((rgb, (2, 4, 179), u8), (rgb, (2, 4, H, W, 4), u8), (rgb, (2, 3, 180), u8),
                            (rgb, (2, 4, 180), torch.float32), (rgb, (2, 4), u8), (rgb, (2, 4, 181), u8)):
        with pytest.raises(ValueError, match="PixelSurface"):
            N.describe_shape(shape, dtype, (None, 4), frame_layout=s)
    # per image: at least image_stride bytes, or exactly image_stride in any shape
    assert N.describe_shape((200,), u8, (), frame_layout=rgb, in_place=True, at_least=True).fmt == N.FRAME_PIXELS
    assert N.describe_shape((H, W, 3), u8, (), frame_layout=rgb, in_place=True, at_least=True).lead == ()
    with pytest.raises(ValueError):
        N.describe_shape((179,), u8, (), frame_layout=rgb, in_place=True, at_least=True)
    # the other layouts' rules did not change: a YuvSurface still wants (image_stride,)
    y = YuvSurface(H, W, "nv12")
    with pytest.raises(ValueError):
        N.describe_shape((2, 4, 9, 10), u8, (None, 4), frame_layout=y)
    assert N.describe_shape((2, 4, 90), u8, (None, 4), frame_layout=y).fmt == N.FRAME_SURFACE
    # checked with the other arguments
    with pytest.raises(ValueError, match="do not combine"):
        N.check_layout(rgb, "nv12")
    with pytest.raises(ValueError, match="this predictor is"):
        N.check_layout(rgb, None, (8, 10))
    with pytest.raises(ValueError, match="PixelSurface"):
        N.check_layout("rgb24")
    assert N.forward_symbol("jh_predictor", N.FRAME_PIXELS) == "jh_predictor_forward_pixels"
    assert N.forward_symbol("jh_predictor", N.FRAME_PIXELS, True, True) == "jh_predictor_forward_pixels"
    assert N.forward_symbol("jh_predictor2d", N.FRAME_PIXELS, False, True) == "jh_predictor2d_forward_pixels"


def test_new_symbols_in_header_and_ctypes_table():
    import re
    from jarvis_hybridnet_amd import _native as N
    from tests.test_native_abi import ROOT, header_symbols
    for name in ("jh_pixel_surface_check", "jh_op_pixels_to_bgr", "jh_predictor_forward_pixels",
                 "jh_predictor2d_forward_pixels", "jh_predictor_detect_subjects_pixels"):
        assert name in header_symbols() and name in N.symbols() and hasattr(N.lib(), name), name
    assert N.lib().jh_abi_version() == 4
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    assert dict(re.findall(r"#define JH_PIXEL_(\w+) (\d+)", text)) == {k.upper(): str(v) for k, v in M.COLOURS.items()}
    assert ctypes.sizeof(N.PixelSurfaceStruct) == 112
