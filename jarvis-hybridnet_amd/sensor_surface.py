"""Description of a raw sensor image (jh_sensor_surface of include/jarvis_hip.h): one byte per pixel as a
machine-vision camera delivers it -- Mono8, or an 8-bit Bayer mosaic -- and where its h x w samples lie inside
`image_stride` bytes.  Pure Python: building and checking a description needs neither the native library nor a GPU;
the rules are those of jh_sensor_surface_check."""
import numbers

# pattern name -> JH_SENSOR_* ; a Bayer pattern is named by its top-left 2 x 2 cell (GenICam BayerRG8 = 'rggb',
# BayerBG8 = 'bggr', BayerGR8 = 'grbg', BayerGB8 = 'gbrg')
PATTERNS = {"mono": 0, "rggb": 1, "bggr": 2, "grbg": 3, "gbrg": 4}

_FIELDS = ("height", "width", "pattern", "pitch", "offset", "image_stride")


class SensorSurface:
    """One image of a pool of camera buffers; frames are (..., image_stride) uint8, images back to back.

    SensorSurface(height, width, pattern) is the tight layout: raw(y, x) at byte y * width + x.  `pitch` is the row
    pitch of a padded buffer, `offset` the byte at which the first sample lies (a chunk header in front of the
    image), `image_stride` the distance between images when there is a gap behind the last row.  pattern: 'mono'
    (R = G = B = the byte) or the Bayer cell 'rggb' | 'bggr' | 'grbg' | 'gbrg', demosaiced bilinearly as defined in
    include/jarvis_hip.h.  Bytes that are no sample are never read.  Immutable and hashable; ValueError for a
    description jh_sensor_surface_check would refuse."""
    __slots__ = _FIELDS

    def __init__(self, height, width, pattern="mono", pitch=None, offset=0, image_stride=None):
        _size(height, width)
        pitch = width if pitch is None else pitch
        if image_stride is None:
            if not (_is_int(pitch) and _is_int(offset)):
                raise ValueError("pitch and offset must be integers, got %r, %r" % (pitch, offset))
            image_stride = offset + height * pitch
        values = (height, width, pattern, pitch, offset, image_stride)
        check(*values)
        for name, v in zip(_FIELDS, values):
            object.__setattr__(self, name, v if isinstance(v, str) else int(v))

    def __setattr__(self, name, value):
        raise AttributeError("SensorSurface is immutable")

    __delattr__ = __setattr__

    def _key(self):
        return tuple(getattr(self, n) for n in _FIELDS)

    def __eq__(self, other):
        return isinstance(other, SensorSurface) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "SensorSurface(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in _FIELDS)

    def check(self):
        """The rules of jh_sensor_surface_check on this description (they held when it was built)."""
        check(*self._key())
        return self

    def struct(self):
        """The jh_sensor_surface of the C ABI (a new ctypes structure)."""
        from ._native import SensorSurfaceStruct
        return SensorSurfaceStruct(self.image_stride, self.offset, self.pitch, PATTERNS[self.pattern], 0)


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _size(height, width):
    if not (_is_int(height) and _is_int(width)) or height <= 0 or width <= 0:
        raise ValueError("raw sensor frames need a positive height and width; got %r x %r" % (height, width))


def check(height, width, pattern, pitch, offset, image_stride):
    """The rules of jh_sensor_surface_check (include/jarvis_hip.h), one ValueError per rule."""
    _size(height, width)
    if pattern not in PATTERNS:
        raise ValueError("pattern must be one of %s, got %r" % (list(PATTERNS), pattern))
    if pattern != "mono" and (height % 2 or width % 2 or height < 4 or width < 4):
        raise ValueError("Bayer frames need an even height and width of at least 4; got %d x %d" % (height, width))
    for name, v in (("pitch", pitch), ("offset", offset), ("image_stride", image_stride)):
        if not _is_int(v) or not -(1 << 63) <= v < (1 << 63):
            raise ValueError("%s must be a 64-bit integer, got %r" % (name, v))
    if pitch < width:
        raise ValueError("pitch (%d) is smaller than the width (%d)" % (pitch, width))
    if offset < 0:
        raise ValueError("offset must not be negative, got %d" % offset)
    if offset + (height - 1) * pitch + width > image_stride:
        raise ValueError("the image ends beyond image_stride (%d)" % image_stride)
