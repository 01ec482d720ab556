"""Description of a YUV 4:2:0 decoder surface (jh_yuv_surface of include/jarvis_hip.h): where the three planes of
one image lie inside `image_stride` bytes and how its colour is coded.  Pure Python: building and checking a
description needs neither the native library nor a GPU; the rules are those of jh_yuv_surface_check."""
import numbers

ORDERS = ("i420", "yv12", "nv12", "nv21")
MATRICES = {"bt601": 0, "bt709": 1}                 # JH_YUV_BT601 / JH_YUV_BT709
RANGES = {"limited": 0, "full": 1}                  # JH_YUV_LIMITED / JH_YUV_FULL

# (Y0, CY, CVR, CUB, CUG, CVG) of the fixed-point conversion, by (matrix, range): BT.601 limited keeps OpenCV's
# literals (the bits of the 'i420' / 'nv12' formats); the others are round(x * 2^20) of the float64 matrix
COEFFICIENTS = {
    ("bt601", "limited"): (16, 1220542, 1673527, 2116026, -409993, -852492),
    ("bt601", "full"): (0, 1048576, 1470104, 1858077, -360853, -748826),
    ("bt709", "limited"): (16, 1220945, 1879825, 2215014, -223607, -558796),
    ("bt709", "full"): (0, 1048576, 1651297, 1945738, -196424, -490864),
}

_FIELDS = ("height", "width", "image_stride", "y_offset", "y_pitch", "u_offset", "v_offset", "c_pitch", "c_step",
           "matrix", "range", "bits", "msb")


def sample_code(bits, msb):
    """JH_SAMPLE_* of include/jarvis_hip.h: 0 for 8-bit planes, else JH_SAMPLE_U16(shift) -- `bits` significant bits
    at the low (shift = bits - 8) or, with msb, the high (shift = 8) end of a little-endian 16-bit word."""
    if not _is_int(bits) or not isinstance(msb, bool):
        raise ValueError("bits must be an integer and msb a bool, got %r, %r" % (bits, msb))
    if bits == 8 and not msb:
        return 0
    if not 9 <= bits <= 16:
        raise ValueError("16-bit planes hold 9..16 bits per sample (8 bits: one byte, msb=False), got bits=%d" % bits)
    return 0x100 | (8 if msb else bits - 8)


class YuvSurface:
    """One image of a pool of decoder surfaces; frames are (..., image_stride) uint8, images back to back.

    YuvSurface(height, width, order) is the tight layout; y_pitch / c_pitch give the row pitches of a pitched
    surface, luma_rows (>= height) the aligned height after which the chroma starts (at luma_rows * y_pitch), and
    image_stride the distance between images when there is a gap behind the last plane.  order: 'i420' (Y, U, V
    planes), 'yv12' (Y, V, U), 'nv12' (Y, interleaved UV), 'nv21' (Y, interleaved VU).  matrix 'bt601' | 'bt709',
    range 'limited' | 'full'.  `from_planes` takes every offset explicitly (an FFmpeg AVFrame copied plane by plane
    with its linesize).  Bytes that belong to no plane are never read.

    Samples wider than a byte: bits=10 (.. 16) says every Y, U and V sample is a little-endian 16-bit word with
    `bits` significant bits at its low end (FFmpeg's yuv420p10le: YuvSurface(h, w, 'i420', bits=10)) or, with
    msb=True, at its high end (P010 / P012 / P016: YuvSurface(h, w, 'nv12', bits=10, msb=True)).  The fetch truncates
    a sample to its top 8 bits, byte = min(sample >> shift, 255), and converts the bytes with the same constants.
    Offsets and pitches stay in bytes (all even), c_step counts samples; the tight pitches double.

    Immutable and hashable; ValueError for a description jh_yuv_surface_check would refuse."""
    __slots__ = _FIELDS

    def __init__(self, height, width, order="nv12", matrix="bt601", range="limited", y_pitch=None, c_pitch=None,
                 luma_rows=None, image_stride=None, *, bits=8, msb=False):
        if order not in ORDERS:
            raise ValueError("order must be one of %s, got %r" % (list(ORDERS), order))
        _even_size(height, width)
        semi = order in ("nv12", "nv21")
        sb = 2 if sample_code(bits, msb) else 1             # bytes per sample
        y_pitch = width * sb if y_pitch is None else y_pitch
        c_pitch = (width if semi else width // 2) * sb if c_pitch is None else c_pitch
        luma_rows = height if luma_rows is None else luma_rows
        for name, v in (("y_pitch", y_pitch), ("c_pitch", c_pitch), ("luma_rows", luma_rows)):
            if not _is_int(v):
                raise ValueError("%s must be an integer, got %r" % (name, v))
        if luma_rows < height:
            raise ValueError("luma_rows (%d) is smaller than the height (%d)" % (luma_rows, height))
        base = luma_rows * y_pitch
        if semi:
            first, second, end = base, base + sb, base + c_pitch * (height // 2)
        else:
            first, second = base, base + c_pitch * (height // 2)
            end = second + c_pitch * (height // 2)
        u_first = order in ("i420", "nv12")
        self._set(height, width, end if image_stride is None else image_stride, 0, y_pitch,
                  first if u_first else second, second if u_first else first, c_pitch, 2 if semi else 1, matrix, range,
                  bits, msb)

    @classmethod
    def from_planes(cls, height, width, y_offset, y_pitch, u_offset, v_offset, c_pitch, c_step, image_stride,
                    matrix="bt601", range="limited", bits=8, msb=False):
        self = object.__new__(cls)
        self._set(height, width, image_stride, y_offset, y_pitch, u_offset, v_offset, c_pitch, c_step, matrix, range,
                  bits, msb)
        return self

    def _set(self, *values):
        check(*values)
        for name, v in zip(_FIELDS, values):
            object.__setattr__(self, name, v if isinstance(v, (str, bool)) else int(v))

    def __setattr__(self, name, value):
        raise AttributeError("YuvSurface is immutable")

    __delattr__ = __setattr__

    def _key(self):
        return tuple(getattr(self, n) for n in _FIELDS)

    def __eq__(self, other):
        return isinstance(other, YuvSurface) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "YuvSurface(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in _FIELDS)

    @property
    def coefficients(self):
        """(Y0, CY, CVR, CUB, CUG, CVG) of this surface's matrix and range."""
        return COEFFICIENTS[(self.matrix, self.range)]

    @property
    def sample(self):
        """The JH_SAMPLE_* code of (bits, msb)."""
        return sample_code(self.bits, self.msb)

    @property
    def shift(self):
        """byte = min(sample >> shift, 255)."""
        return self.sample & 0xff

    def struct(self):
        """The jh_yuv_surface of the C ABI (a new ctypes structure)."""
        from ._native import YuvSurfaceStruct
        return YuvSurfaceStruct(self.image_stride, self.y_offset, self.y_pitch, self.u_offset, self.v_offset,
                                self.c_pitch, self.c_step, MATRICES[self.matrix], RANGES[self.range], self.sample)


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _even_size(height, width):
    if not (_is_int(height) and _is_int(width)) or height <= 0 or width <= 0 or height % 2 or width % 2:
        raise ValueError("YUV 4:2:0 frames need an even, positive height and width; got %r x %r" % (height, width))


def check(height, width, image_stride, y_offset, y_pitch, u_offset, v_offset, c_pitch, c_step, matrix, range, bits=8,
          msb=False):
    """The rules of jh_yuv_surface_check (include/jarvis_hip.h), one ValueError per rule."""
    _even_size(height, width)
    sb = 2 if sample_code(bits, msb) else 1                 # bytes per sample
    for name, v in (("image_stride", image_stride), ("y_offset", y_offset), ("y_pitch", y_pitch),
                    ("u_offset", u_offset), ("v_offset", v_offset), ("c_pitch", c_pitch), ("c_step", c_step)):
        if not _is_int(v) or not -(1 << 63) <= v < (1 << 63):
            raise ValueError("%s must be a 64-bit integer, got %r" % (name, v))
    if c_step not in (1, 2):
        raise ValueError("c_step must be 1 (planar) or 2 (semi-planar), got %r" % (c_step,))
    if y_pitch < width * sb:
        raise ValueError("y_pitch (%d) is smaller than the width (%d bytes)" % (y_pitch, width * sb))
    if c_pitch < (width // 2) * c_step * sb:
        raise ValueError("c_pitch (%d) is smaller than a chroma row (%d)" % (c_pitch, (width // 2) * c_step * sb))
    if min(y_offset, u_offset, v_offset, image_stride) < 0:
        raise ValueError("offsets must not be negative")
    if c_step == 2:
        if abs(u_offset - v_offset) != sb:
            raise ValueError("semi-planar U and V are neighbouring samples: |u_offset - v_offset| must be %d" % sb)
        if min(u_offset, v_offset) % (2 * sb) or c_pitch % (2 * sb):
            raise ValueError("a semi-planar chroma pair starts at a multiple of %d bytes and c_pitch is one" % (2 * sb))
    if sb == 2 and any(v % 2 for v in (image_stride, y_offset, y_pitch, u_offset, v_offset, c_pitch)):
        raise ValueError("16-bit samples need even offsets, pitches and image_stride (every load is aligned)")
    y_end = y_offset + (height - 1) * y_pitch + width * sb
    c_span = (height // 2 - 1) * c_pitch + ((width // 2 - 1) * c_step + 1) * sb
    if max(y_end, u_offset + c_span, v_offset + c_span) > image_stride:
        raise ValueError("a plane ends beyond image_stride (%d)" % image_stride)
    if matrix not in MATRICES:
        raise ValueError("matrix must be one of %s, got %r" % (sorted(MATRICES), matrix))
    if range not in RANGES:
        raise ValueError("range must be one of %s, got %r" % (sorted(RANGES), range))
