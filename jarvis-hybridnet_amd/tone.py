"""Per-camera tone tables (jh_predictor_set_tone in include/jarvis_hip.h): black level, gain, white balance and gamma as
ONE byte-to-value lookup inside the resize / crop fetch.  Pure Python: nothing here loads the library.

A table set is (C,3,256) float32: tables[c][ch][k] is the value the networks' pre-processing sees for byte k of channel
ch (0 = R, 1 = G, 2 = B) of camera c, in place of k * (1/255).  A pixel is first converted to its (R, G, B) bytes as
without tables (colour conversion, demosaic, sample reduction); then each byte is looked up."""
import numpy as np


def _per_camera(name, value, cameras, width):
    """A constructor argument that may be a scalar or per camera -> (C, width) float64: a scalar, (width,) for every
    camera (width > 1), (C,) per camera (width == 1), or (C, width)."""
    a = np.asarray(value, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("%s must be finite, got %r" % (name, value))
    shapes = [(), (cameras, width)] + ([(width,)] if width > 1 else [(cameras,)])
    if a.shape not in shapes:
        raise ValueError("%s must be a scalar%s or per camera (%d%s), got shape %s" % (
            name, ", (%d,)" % width if width > 1 else "", cameras, ", %d" % width if width > 1 else "", a.shape))
    if a.shape == (cameras,) and width == 1:
        a = a.reshape(cameras, 1)
    return np.broadcast_to(a, (cameras, width)).copy()


class ToneTables:
    """(C,3,256) float32 tables, checked: `tables` is the array the setters upload (NativePredictor.set_tone,
    JarvisPredictor3D.set_tone, predict3D_frames(..., tone=)); the 2D predictor takes C = 1."""

    def __init__(self, tables):
        a = np.asarray(tables)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (3, 256):
            raise ValueError("tone tables must be (C, 3, 256) (or (3, 256) for one camera), got shape %s"
                             % (np.asarray(tables).shape,))
        if a.dtype.kind not in "fiu":
            raise ValueError("tone tables must be numeric, got dtype %s" % a.dtype)
        if not np.all(np.isfinite(a.astype(np.float64))):
            raise ValueError("tone tables must be finite (no NaN or infinity)")
        with np.errstate(over="ignore"):
            self.tables = np.ascontiguousarray(a, dtype=np.float32)
        if not np.all(np.isfinite(self.tables)):
            raise ValueError("tone tables must be finite in float32")
        self.tables.setflags(write=False)

    @property
    def cameras(self):
        return self.tables.shape[0]

    def __eq__(self, other):
        return isinstance(other, ToneTables) and self.tables.shape == other.tables.shape and \
            np.array_equal(self.tables.view(np.uint32), other.tables.view(np.uint32))

    __hash__ = None

    def __repr__(self):
        return "ToneTables(cameras=%d)" % self.cameras

    @classmethod
    def identity(cls, cameras):
        """fl(fl(k) * fl(1/255)): the bits of the call without tables."""
        cameras = _count(cameras)
        row = np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))
        return cls(np.broadcast_to(row, (cameras, 3, 256)))

    @classmethod
    def from_bytes(cls, lut_u8):
        """A uint8 LUT L (C,3,256) (or (3,256)): fl(fl(L) * fl(1/255)), the bits of the uint8 path on the L-mapped
        bytes."""
        a = np.asarray(lut_u8)
        if a.ndim == 2:
            a = a[None]
        if a.dtype != np.uint8:
            raise ValueError("from_bytes takes a uint8 LUT, got dtype %s" % a.dtype)
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (3, 256):
            raise ValueError("from_bytes takes a (C, 3, 256) or (3, 256) LUT, got shape %s" % (np.asarray(lut_u8).shape,))
        return cls(a.astype(np.float32) * (np.float32(1) / np.float32(255)))

    @classmethod
    def from_curve(cls, cameras, black=0, white=255, gain=(1, 1, 1), gamma=1.0):
        """clip(gain_ch * (k - black) / (white - black), 0, 1) ** (1 / gamma) per entry, in float64, rounded once to
        float32.  black, white, gamma: a scalar or (C,) per camera; gain: a scalar, (3,) = (R, G, B) for every camera,
        or (C,3).  white > black and gamma > 0 (ValueError otherwise)."""
        cameras = _count(cameras)
        b = _per_camera("black", black, cameras, 1)
        w = _per_camera("white", white, cameras, 1)
        gm = _per_camera("gamma", gamma, cameras, 1)
        g = _per_camera("gain", gain, cameras, 3)
        if np.any(w <= b):
            raise ValueError("white must be above black")
        if np.any(gm <= 0):
            raise ValueError("gamma must be positive")
        k = np.arange(256, dtype=np.float64)
        lin = g[:, :, None] * (k[None, None, :] - b[:, :, None]) / (w - b)[:, :, None]
        return cls(np.clip(lin, 0.0, 1.0) ** (1.0 / gm)[:, :, None])


def _count(cameras):
    if isinstance(cameras, bool) or not isinstance(cameras, (int, np.integer)) or cameras < 1:
        raise ValueError("cameras must be a positive integer, got %r" % (cameras,))
    return int(cameras)


def check_tone(tone, cameras):
    """The `tone` argument of the setters and drivers: None stays None; a ToneTables (or an array it accepts) of
    `cameras` cameras -> ToneTables.  ValueError otherwise."""
    if tone is None:
        return None
    if not isinstance(tone, ToneTables):
        tone = ToneTables(tone)
    if tone.cameras != cameras:
        raise ValueError("tone tables of %d cameras given to a predictor of %d" % (tone.cameras, cameras))
    return tone
