"""Description of a raw sensor image (jh_sensor_surface of include/jarvis_hip.h): one sample per pixel as a
machine-vision camera delivers it -- Mono or a Bayer mosaic, in bytes, in 16-bit words or in the GenICam packed
forms 10p / 12p -- and where its h x w samples lie inside `image_stride` bytes.  Pure Python: building and checking a
description needs neither the native library nor a GPU; the rules are those of jh_sensor_surface_check."""
import numbers

# pattern name -> JH_SENSOR_* ; a Bayer pattern is named by its top-left 2 x 2 cell (GenICam BayerRG8 = 'rggb',
# BayerBG8 = 'bggr', BayerGR8 = 'grbg', BayerGB8 = 'gbrg')
PATTERNS = {"mono": 0, "rggb": 1, "bggr": 2, "grbg": 3, "gbrg": 4}

# how a sample is stored: 'u8' one byte; 'u16' / 'u16msb' a little-endian 16-bit word with the `bits` significant
# bits at its low / high end; 'packed' the GenICam PFNC 10p / 12p bit stream of a row
CONTAINERS = ("u8", "u16", "u16msb", "packed")

_FIELDS = ("height", "width", "pattern", "pitch", "offset", "image_stride", "bits", "container")


def sample_code(bits, container):
    """JH_SAMPLE_* of include/jarvis_hip.h for `bits` significant bits in `container`: how the fetch reduces a sample
    to the byte the network sees, byte = min(sample >> shift, 255).  ValueError for a pair the ABI has no code for."""
    if container not in CONTAINERS:
        raise ValueError("container must be one of %s, got %r" % (list(CONTAINERS), container))
    if not _is_int(bits):
        raise ValueError("bits must be an integer, got %r" % (bits,))
    lo, hi = {"u8": (8, 8), "u16": (8, 16), "u16msb": (9, 16), "packed": (10, 12)}[container]
    if not lo <= bits <= hi or (container == "packed" and bits == 11):
        raise ValueError("container %r holds %s bits per sample, got %d"
                         % (container, {"u8": "8", "u16": "8..16", "u16msb": "9..16", "packed": "10 or 12"}[container],
                            bits))
    if container == "u8":
        return 0
    if container == "packed":
        return 0x200 if bits == 10 else 0x300
    return 0x100 | (8 if container == "u16msb" else bits - 8)


def row_bytes(width, code):
    """Bytes the `width` samples of one row occupy under the sample code `code` (JH_SAMPLE_*)."""
    return {0: width, 1: 2 * width, 2: (10 * width + 7) // 8, 3: (12 * width + 7) // 8}[code >> 8]


class SensorSurface:
    """One image of a pool of camera buffers; frames are (..., image_stride) uint8, images back to back.

    SensorSurface(height, width, pattern) is the tight layout: raw(y, x) at byte y * width + x.  `pitch` is the row
    pitch of a padded buffer, `offset` the byte at which the first sample lies (a chunk header in front of the
    image), `image_stride` the distance between images when there is a gap behind the last row.  pattern: 'mono'
    (R = G = B = the byte) or the Bayer cell 'rggb' | 'bggr' | 'grbg' | 'gbrg', demosaiced bilinearly as defined in
    include/jarvis_hip.h.  Bytes that are no sample are never read.

    Samples wider than a byte: `bits` significant bits in `container` 'u16' (LSB-aligned in a little-endian 16-bit
    word: Mono10 / Mono12 / Mono16, BayerRG12 ...), 'u16msb' (MSB-aligned) or 'packed' (GenICam 10p / 12p: every
    row a little-endian bit stream, sample x at bits [bits * x, bits * x + bits) -- NOT the legacy GigE
    Mono12Packed nibble order).  The default container is 'u8' for 8 bits and 'u16' otherwise.  The fetch truncates
    a sample to its top 8 bits, byte = min(sample >> (bits - 8), 255) -- what the camera delivers as Mono8 --, and
    the bytes go the way 8-bit samples go.  pitch, offset and image_stride stay in bytes (even for the 16-bit
    containers); the tight pitch is the bytes of a row.

    Immutable and hashable; ValueError for a description jh_sensor_surface_check would refuse."""
    __slots__ = _FIELDS

    def __init__(self, height, width, pattern="mono", pitch=None, offset=0, image_stride=None, *, bits=8,
                 container=None):
        _size(height, width)
        if container is None:
            container = "u8" if _is_int(bits) and bits == 8 else "u16"
        pitch = row_bytes(width, sample_code(bits, container)) if pitch is None else pitch
        if image_stride is None:
            if not (_is_int(pitch) and _is_int(offset)):
                raise ValueError("pitch and offset must be integers, got %r, %r" % (pitch, offset))
            image_stride = offset + height * pitch
        values = (height, width, pattern, pitch, offset, image_stride, bits, container)
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

    @property
    def sample(self):
        """The JH_SAMPLE_* code of (bits, container)."""
        return sample_code(self.bits, self.container)

    @property
    def shift(self):
        """byte = min(sample >> shift, 255) -- after the packed forms' samples are taken out of the bit stream."""
        return 8 if self.container == "u16msb" else self.bits - 8

    @property
    def row_bytes(self):
        """Bytes the samples of one row occupy."""
        return row_bytes(self.width, self.sample)

    def check(self):
        """The rules of jh_sensor_surface_check on this description (they held when it was built)."""
        check(*self._key())
        return self

    def struct(self):
        """The jh_sensor_surface of the C ABI (a new ctypes structure)."""
        from ._native import SensorSurfaceStruct
        return SensorSurfaceStruct(self.image_stride, self.offset, self.pitch, PATTERNS[self.pattern], self.sample)


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _size(height, width):
    if not (_is_int(height) and _is_int(width)) or height <= 0 or width <= 0:
        raise ValueError("raw sensor frames need a positive height and width; got %r x %r" % (height, width))


def check(height, width, pattern, pitch, offset, image_stride, bits=8, container="u8"):
    """The rules of jh_sensor_surface_check (include/jarvis_hip.h), one ValueError per rule."""
    _size(height, width)
    code = sample_code(bits, container)
    row = row_bytes(width, code)
    if pattern not in PATTERNS:
        raise ValueError("pattern must be one of %s, got %r" % (list(PATTERNS), pattern))
    if pattern != "mono" and (height % 2 or width % 2 or height < 4 or width < 4):
        raise ValueError("Bayer frames need an even height and width of at least 4; got %d x %d" % (height, width))
    for name, v in (("pitch", pitch), ("offset", offset), ("image_stride", image_stride)):
        if not _is_int(v) or not -(1 << 63) <= v < (1 << 63):
            raise ValueError("%s must be a 64-bit integer, got %r" % (name, v))
    if pitch < row:
        raise ValueError("pitch (%d) is smaller than the width (%d samples, %d bytes)" % (pitch, width, row))
    if offset < 0:
        raise ValueError("offset must not be negative, got %d" % offset)
    if offset + (height - 1) * pitch + row > image_stride:
        raise ValueError("the image ends beyond image_stride (%d)" % image_stride)
    if code >> 8 == 1 and (offset % 2 or pitch % 2 or image_stride % 2):
        raise ValueError("16-bit samples need an even offset, pitch and image_stride (every load is aligned); got "
                         "%d, %d, %d" % (offset, pitch, image_stride))
