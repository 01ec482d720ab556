"""Description of a pixel surface (jh_pixel_surface of include/jarvis_hip.h): three 8-bit components per pixel -- R G B
or Y U V --, each found by its own address rule inside the `image_stride` bytes of one image.  RGB in any byte order,
4-byte and planar RGB, grey, packed YUYV / UYVY / YVYU and planar or semi-planar YUV 4:2:2 / 4:4:4 / 4:4:0 / 4:1:1 /
4:2:0 are values of this one description.  Pure Python: building and checking a description needs neither the native
library nor a GPU; the rules are those of jh_pixel_surface_check."""
import numbers

from .yuv_surface import COEFFICIENTS, MATRICES, RANGES

COLOURS = {"rgb": 0, "yuv": 1}                      # JH_PIXEL_RGB / JH_PIXEL_YUV
SUBSAMPLINGS = {"444": (0, 0), "422": (1, 0), "440": (0, 1), "411": (2, 0), "420": (1, 1)}     # (xs, ys) of the chroma
# byte of (Y, U, V) inside the 4-byte group of two pixels; the second pixel's Y lies 2 bytes after the first's
YUV_PACKED = {"yuyv": (0, 1, 3), "uyvy": (1, 0, 2), "yvyu": (0, 3, 1)}

_FIELDS = ("height", "width", "image_stride", "offset", "pitch", "step", "xs", "ys", "colour", "matrix", "range",
           "sample")


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _ceil_shift(n, s):
    return ((n - 1) >> s) + 1


class PixelSurface:
    """One image of frames (..., image_stride) uint8, images back to back: component k of pixel (y, x) is the byte at
    offset[k] + (y >> ys[k]) * pitch[k] + (x >> xs[k]) * step[k]; components 0, 1, 2 are R, G, B (colour 'rgb') or
    Y, U, V (colour 'yuv', converted with `matrix` 'bt601' | 'bt709' and `range` 'limited' | 'full' as a YuvSurface
    converts; both are None for 'rgb').  Chroma is replicated, never interpolated.  The (R, G, B) bytes take the uint8
    path: a result equals, bit for bit, that of the uint8 BGR frames pixels_to_bgr (synthetic.py) makes of the bytes.
    Bytes that are no component (an alpha byte, pitch padding, gaps) are never read.

    Built by the constructors packed / planar / gray / yuv_packed / yuv_planar / from_pix_fmt, or from_components
    with every field explicit.  Immutable and hashable; ValueError for a description jh_pixel_surface_check would
    refuse."""
    __slots__ = _FIELDS

    def __init__(self, *args, **kwargs):
        raise TypeError("build a PixelSurface with packed(), planar(), gray(), yuv_packed(), yuv_planar(), "
                        "from_pix_fmt() or from_components()")

    @classmethod
    def from_components(cls, height, width, image_stride, offset, pitch, step, xs=(0, 0, 0), ys=(0, 0, 0),
                        colour="rgb", matrix=None, range=None, sample=0):
        values = (height, width, image_stride, _triple(offset), _triple(pitch), _triple(step), _triple(xs), _triple(ys),
                  colour, matrix, range, sample)
        check(*values)
        self = object.__new__(cls)
        for name, v in zip(_FIELDS, values):
            object.__setattr__(self, name, tuple(int(i) for i in v) if isinstance(v, tuple)
                               else v if v is None or isinstance(v, str) else int(v))
        return self

    @classmethod
    def packed(cls, height, width, order, pitch=None, offset=0, image_stride=None):
        """Interleaved RGB: `order` names the bytes of a pixel over r g b a x 0, three or four of them with r, g and b
        once each -- 'rgb' (rgb24), 'bgr', 'bgra', 'rgba', 'argb', 'abgr', 'rgb0', 'xbgr' ...  pitch: bytes per row
        (default width * len(order)); offset: of the first pixel; image_stride: default offset + height * pitch."""
        _size(height, width)
        if not isinstance(order, str) or len(order) not in (3, 4) or set(order) - set("rgbax0") or \
                any(order.count(c) != 1 for c in "rgb"):
            raise ValueError("order must name 3 or 4 bytes over 'r g b a x 0' with r, g and b once each, got %r"
                             % (order,))
        n = len(order)
        pitch = width * n if pitch is None else pitch
        _ints(pitch=pitch, offset=offset)
        stride = offset + height * pitch if image_stride is None else image_stride
        return cls.from_components(height, width, stride, tuple(offset + order.index(c) for c in "rgb"), (pitch,) * 3,
                                   (n,) * 3)

    @classmethod
    def planar(cls, height, width, order="rgb", pitch=None, plane_rows=None, offset=0, image_stride=None):
        """Three planes of one byte per pixel in the sequence `order` ('rgb': torchcodec / decode_jpeg (3,H,W); 'gbr':
        FFmpeg gbrp).  pitch: bytes per row (default width); plane_rows (>= height): rows from one plane to the next."""
        _size(height, width)
        if not isinstance(order, str) or sorted(order) != ["b", "g", "r"]:
            raise ValueError("order must be a permutation of 'rgb', got %r" % (order,))
        pitch = width if pitch is None else pitch
        plane_rows = height if plane_rows is None else plane_rows
        _ints(pitch=pitch, plane_rows=plane_rows, offset=offset)
        if plane_rows < height:
            raise ValueError("plane_rows (%d) is smaller than the height (%d)" % (plane_rows, height))
        stride = offset + 3 * plane_rows * pitch if image_stride is None else image_stride
        return cls.from_components(height, width, stride,
                                   tuple(offset + order.index(c) * plane_rows * pitch for c in "rgb"), (pitch,) * 3,
                                   (1,) * 3)

    @classmethod
    def gray(cls, height, width, pitch=None, offset=0, image_stride=None):
        """One grey byte per pixel: R = G = B = the byte (the three components share one address rule)."""
        _size(height, width)
        pitch = width if pitch is None else pitch
        _ints(pitch=pitch, offset=offset)
        stride = offset + height * pitch if image_stride is None else image_stride
        return cls.from_components(height, width, stride, (offset,) * 3, (pitch,) * 3, (1,) * 3)

    @classmethod
    def yuv_packed(cls, height, width, order="yuyv", matrix="bt601", range="limited", pitch=None, offset=0,
                   image_stride=None):
        """Packed YUV 4:2:2, two pixels in four bytes: 'yuyv' (YUY2), 'uyvy' or 'yvyu'.  pitch: bytes per row (default
        4 * ceil(width / 2))."""
        _size(height, width)
        if order not in YUV_PACKED:
            raise ValueError("order must be one of %s, got %r" % (sorted(YUV_PACKED), order))
        pitch = 4 * _ceil_shift(width, 1) if pitch is None else pitch
        _ints(pitch=pitch, offset=offset)
        stride = offset + height * pitch if image_stride is None else image_stride
        return cls.from_components(height, width, stride, tuple(offset + b for b in YUV_PACKED[order]), (pitch,) * 3,
                                   (2, 4, 4), (0, 1, 1), (0, 0, 0), "yuv", matrix, range)

    @classmethod
    def yuv_planar(cls, height, width, subsampling="422", semi=None, matrix="bt601", range="limited", y_pitch=None,
                   c_pitch=None, luma_rows=None, offset=0, image_stride=None):
        """The Y plane, then the chroma: two planes U, V (semi None), or one interleaved plane U first (semi 'uv':
        nv16 / nv24 / nv12) or V first ('vu').  subsampling '444' | '422' | '440' | '411' | '420'; a subsampled plane
        is ceil wide / high.  y_pitch / c_pitch: bytes per row (default: tight); luma_rows (>= height): the aligned
        height after which the chroma starts."""
        _size(height, width)
        if subsampling not in SUBSAMPLINGS:
            raise ValueError("subsampling must be one of %s, got %r" % (sorted(SUBSAMPLINGS), subsampling))
        if semi not in (None, "uv", "vu"):
            raise ValueError("semi must be None, 'uv' or 'vu', got %r" % (semi,))
        sx, sy = SUBSAMPLINGS[subsampling]
        cw, ch = _ceil_shift(width, sx), _ceil_shift(height, sy)
        step = 2 if semi else 1
        y_pitch = width if y_pitch is None else y_pitch
        c_pitch = cw * step if c_pitch is None else c_pitch
        luma_rows = height if luma_rows is None else luma_rows
        _ints(y_pitch=y_pitch, c_pitch=c_pitch, luma_rows=luma_rows, offset=offset)
        if luma_rows < height:
            raise ValueError("luma_rows (%d) is smaller than the height (%d)" % (luma_rows, height))
        base = offset + luma_rows * y_pitch
        if semi:
            u, v, end = (base, base + 1, base + ch * c_pitch) if semi == "uv" else (base + 1, base, base + ch * c_pitch)
        else:
            u, v, end = base, base + ch * c_pitch, base + 2 * ch * c_pitch
        return cls.from_components(height, width, end if image_stride is None else image_stride, (offset, u, v),
                                   (y_pitch, c_pitch, c_pitch), (1, step, step), (0, sx, sx), (0, sy, sy), "yuv",
                                   matrix, range)

    @classmethod
    def from_pix_fmt(cls, height, width, name, linesize=None):
        """The layout of an FFmpeg pixel format `name` (PIX_FMTS lists them; the yuvj* names mean full range, BT.601
        as JPEG has it), the planes back to back as an AVFrame copied plane by plane.  linesize: the bytes per row of
        each plane, as AVFrame.linesize gives them (default: tight)."""
        if name not in PIX_FMTS:
            raise ValueError("unknown pixel format %r; known: %s" % (name, ", ".join(sorted(PIX_FMTS))))
        kind, arg, planes = PIX_FMTS[name]
        if linesize is not None:
            if not isinstance(linesize, (tuple, list)) or len(linesize) != planes or not all(_is_int(v) for v in linesize):
                raise ValueError("linesize of %s is %d integers, one per plane; got %r" % (name, planes, linesize))
        ls = (None,) * 3 if linesize is None else tuple(linesize) + (None,) * (3 - planes)
        if kind == "packed":
            return cls.packed(height, width, arg, pitch=ls[0])
        if kind == "gray":
            return cls.gray(height, width, pitch=ls[0])
        if kind == "yuv_packed":
            return cls.yuv_packed(height, width, arg, pitch=ls[0])
        if kind == "planar":
            if linesize is not None and len(set(linesize)) != 1:
                raise ValueError("the three planes of %s have one linesize; got %r" % (name, linesize))
            return cls.planar(height, width, arg, pitch=ls[0])
        sub, semi, rng = arg
        if linesize is not None and semi is None and ls[1] != ls[2]:
            raise ValueError("the U and V planes of %s have one linesize; got %r" % (name, linesize))
        return cls.yuv_planar(height, width, sub, semi, "bt601", rng, y_pitch=ls[0], c_pitch=ls[1])

    def __setattr__(self, name, value):
        raise AttributeError("PixelSurface is immutable")

    def __delattr__(self, name):
        raise AttributeError("PixelSurface is immutable")

    def _key(self):
        return tuple(getattr(self, n) for n in _FIELDS)

    def __eq__(self, other):
        return isinstance(other, PixelSurface) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "PixelSurface(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in _FIELDS)

    @property
    def coefficients(self):
        """(Y0, CY, CVR, CUB, CUG, CVG) of this surface's matrix and range (colour 'yuv')."""
        return COEFFICIENTS[(self.matrix, self.range)]

    def struct(self):
        """The jh_pixel_surface of the C ABI (a new ctypes structure)."""
        from ._native import PixelSurfaceStruct
        s = PixelSurfaceStruct()
        s.image_stride = self.image_stride
        for k in (0, 1, 2):
            s.offset[k], s.pitch[k], s.step[k] = self.offset[k], self.pitch[k], self.step[k]
            s.xs[k], s.ys[k] = self.xs[k], self.ys[k]
        s.colour = COLOURS[self.colour]
        s.matrix = 0 if self.matrix is None else MATRICES[self.matrix]
        s.range = 0 if self.range is None else RANGES[self.range]
        s.sample = self.sample
        return s


# FFmpeg pixel format -> (constructor, its argument, number of planes)
PIX_FMTS = {
    "rgb24": ("packed", "rgb", 1), "bgr24": ("packed", "bgr", 1),
    "rgba": ("packed", "rgba", 1), "bgra": ("packed", "bgra", 1), "argb": ("packed", "argb", 1),
    "abgr": ("packed", "abgr", 1), "rgb0": ("packed", "rgb0", 1), "bgr0": ("packed", "bgr0", 1),
    "0rgb": ("packed", "0rgb", 1), "0bgr": ("packed", "0bgr", 1),
    "gbrp": ("planar", "gbr", 3), "gray": ("gray", None, 1),
    "yuyv422": ("yuv_packed", "yuyv", 1), "uyvy422": ("yuv_packed", "uyvy", 1), "yvyu422": ("yuv_packed", "yvyu", 1),
    "yuv422p": ("yuv", ("422", None, "limited"), 3), "yuvj422p": ("yuv", ("422", None, "full"), 3),
    "yuv444p": ("yuv", ("444", None, "limited"), 3), "yuvj444p": ("yuv", ("444", None, "full"), 3),
    "yuv440p": ("yuv", ("440", None, "limited"), 3), "yuvj440p": ("yuv", ("440", None, "full"), 3),
    "yuv411p": ("yuv", ("411", None, "limited"), 3),
    "yuv420p": ("yuv", ("420", None, "limited"), 3), "yuvj420p": ("yuv", ("420", None, "full"), 3),
    "nv16": ("yuv", ("422", "uv", "limited"), 2), "nv24": ("yuv", ("444", "uv", "limited"), 2),
    "nv12": ("yuv", ("420", "uv", "limited"), 2), "nv21": ("yuv", ("420", "vu", "limited"), 2),
}


def _triple(v):
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return tuple(v)
    raise ValueError("offset, pitch, step, xs and ys are three values each (one per component), got %r" % (v,))


def _size(height, width):
    if not (_is_int(height) and _is_int(width)) or height <= 0 or width <= 0 or height >= 1 << 31 or width >= 1 << 31:
        raise ValueError("pixel surfaces need a positive height and width; got %r x %r" % (height, width))


def _ints(**values):
    for name, v in values.items():
        if not _is_int(v):
            raise ValueError("%s must be an integer, got %r" % (name, v))


def check(height, width, image_stride, offset, pitch, step, xs, ys, colour, matrix, range, sample=0):
    """The rules of jh_pixel_surface_check (include/jarvis_hip.h) in its order, one ValueError per rule."""
    _size(height, width)
    for name, v in (("image_stride", image_stride),) + tuple(("offset", o) for o in offset) + \
            tuple(("pitch", p) for p in pitch):
        if not _is_int(v) or not -(1 << 63) <= v < (1 << 63):
            raise ValueError("%s must be a 64-bit integer, got %r" % (name, v))
    for name, v in tuple(("step", s) for s in step) + tuple(("xs", s) for s in xs) + tuple(("ys", s) for s in ys) + \
            (("sample", sample),):
        if not _is_int(v) or not -(1 << 31) <= v < (1 << 31):
            raise ValueError("%s must be a 32-bit integer, got %r" % (name, v))
    if colour not in COLOURS:
        raise ValueError("colour must be one of %s, got %r" % (sorted(COLOURS), colour))
    if colour == "yuv":
        if matrix not in MATRICES:
            raise ValueError("matrix must be one of %s, got %r" % (sorted(MATRICES), matrix))
        if range not in RANGES:
            raise ValueError("range must be one of %s, got %r" % (sorted(RANGES), range))
    elif matrix is not None or range is not None:
        raise ValueError("matrix and range belong to colour 'yuv': they must be None for 'rgb', got %r, %r"
                         % (matrix, range))
    if sample != 0:
        raise ValueError("sample must be 0 (one byte per component), got %r" % (sample,))
    if any(not 1 <= s <= 8 for s in step):
        raise ValueError("step must be 1 .. 8, got %r" % (step,))
    if any(not 0 <= s <= 2 for s in tuple(xs) + tuple(ys)):
        raise ValueError("xs and ys must be 0 .. 2, got %r, %r" % (xs, ys))
    if colour == "rgb":
        if any(xs) or any(ys):
            raise ValueError("R, G and B are not subsampled: xs and ys must be 0, got %r, %r" % (xs, ys))
    elif xs[0] or ys[0] or xs[1] != xs[2] or ys[1] != ys[2]:
        raise ValueError("Y is not subsampled, and U and V are subsampled alike; got xs %r, ys %r" % (xs, ys))
    if min(offset) < 0:
        raise ValueError("offsets must not be negative, got %r" % (offset,))
    for k in (0, 1, 2):
        if pitch[k] < ((width - 1) >> xs[k]) * step[k] + 1:
            raise ValueError("pitch[%d] (%d) is smaller than a row of the component (%d)"
                             % (k, pitch[k], ((width - 1) >> xs[k]) * step[k] + 1))
    for k in (0, 1, 2):
        if offset[k] + ((height - 1) >> ys[k]) * pitch[k] + ((width - 1) >> xs[k]) * step[k] + 1 > image_stride:
            raise ValueError("component %d ends beyond image_stride (%d)" % (k, image_stride))
