"""Samples wider than a byte, without a GPU: the sample codes of jh_sensor_surface / jh_yuv_surface (16-bit words,
GenICam 10p / 12p) -- the Python descriptions and the C validation agree rule by rule --, and the test-data helpers of
synthetic.py: reduce_samples, widen, the bit-stream packer with its inverse, the wide forms of pack_*_surface."""
import numpy as np
import pytest

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import sensor_surface as SM
from jarvis_hybridnet_amd import synthetic as S
from jarvis_hybridnet_amd import yuv_surface as YM

U16 = lambda shift: 0x100 | shift  # noqa: E731
P10, P12 = 0x200, 0x300
PATTERN = {0: "mono", 1: "rggb"}


def py_sample(code):
    """(bits, container) a SensorSurface is built with for the sample code, or None where Python cannot name it."""
    if code == 0:
        return 8, "u8"
    if code in (P10, P12):
        return (10 if code == P10 else 12), "packed"
    if 0x100 <= code <= 0x107:
        return 8 + (code & 0xff), "u16"
    if code == 0x108:
        return 16, "u16"                                  # (the same code as every 'u16msb')
    return None


# (h, w, image_stride, offset, pitch, pattern code, sample code), valid?  w = 7: row_bytes 7, 14, 9, 11
SENSOR = [
    ((3, 7, 42, 0, 14, 0, U16(4)), True),                 # tight Mono12
    ((3, 7, 41, 0, 14, 0, U16(4)), False),                # ... image_stride odd (and one byte short)
    ((3, 7, 40, 0, 14, 0, U16(4)), False),                # ... the last row ends beyond image_stride
    ((3, 7, 42, 0, 12, 0, U16(4)), False),                # ... pitch below 2 w
    ((3, 7, 60, 2, 16, 0, U16(0)), True),                 # pitched, offset 2, 8 bits in 16
    ((3, 7, 60, 3, 16, 0, U16(0)), False),                # odd offset
    ((3, 7, 60, 2, 17, 0, U16(0)), False),                # odd pitch
    ((3, 7, 61, 2, 16, 0, U16(0)), False),                # odd image_stride
    ((3, 7, 48, 2, 16, 0, U16(8)), True),                 # MSB-aligned, the last sample ends at image_stride
    ((3, 7, 46, 2, 16, 0, U16(8)), False),                # ... one 16-bit sample too short
    ((4, 6, 48, 0, 12, 1, U16(2)), True),                 # BayerRG10
    ((3, 7, 27, 0, 9, 0, P10), True),                     # tight Mono10p: ceil(70 / 8) = 9
    ((3, 7, 27, 0, 8, 0, P10), False),                    # ... pitch one byte short
    ((3, 7, 26, 0, 9, 0, P10), False),                    # ... image_stride one byte short
    ((3, 7, 33, 0, 11, 0, P12), True),                    # tight Mono12p: ceil(84 / 8) = 11
    ((3, 7, 33, 0, 10, 0, P12), False),
    ((3, 7, 32, 0, 11, 0, P12), False),
    ((3, 7, 50, 5, 13, 0, P12), True),                    # 5 + 2 * 13 + 11 = 42: a gap behind the last row
    ((3, 7, 42, 5, 13, 0, P12), True),                    # packed rows start at any byte: odd offset, pitch, stride
    ((3, 7, 41, 5, 13, 0, P12), False),                   # ... one byte short
    ((4, 6, 36, 0, 9, 1, P12), True),                     # BayerRG12p, 6 samples = 9 bytes
    ((4, 6, 32, 0, 8, 4, P10), True),                     # BayerGB10p, 6 samples = 8 bytes (7.5 rounded up)
    ((4, 6, 28, 0, 7, 4, P10), False),                    # ... 7 bytes hold 5.6 samples
    ((3, 7, 42, 0, 14, 0, 1), False),                     # unknown codes: 1 was `reserved != 0`
    ((3, 7, 42, 0, 14, 0, 0x109), False),                 # a shift above 8
    ((3, 7, 42, 0, 14, 0, 0x201), False),
    ((3, 7, 42, 0, 14, 0, 0x400), False),
    ((3, 7, 42, 0, 14, 0, -1), False),
]


def test_sensor_python_and_c_validation_agree():
    from jarvis_hybridnet_amd import _native as N
    lib = N.lib()
    for d, good in SENSOR:
        h, w, stride, off, pitch, pat, code = d
        st = N.SensorSurfaceStruct(stride, off, pitch, pat, code)
        assert (lib.jh_sensor_surface_check(st, h, w) == 0) == good, (d, lib.jh_last_error())
        how = py_sample(code)
        if how is None:
            continue
        try:
            s = SensorSurface(h, w, PATTERN.get(pat, "gbrg"), pitch=pitch, offset=off, image_stride=stride, bits=how[0],
                              container=how[1])
            ok = True
        except ValueError:
            ok = False
        assert ok == good, d
        if good:
            q = s.struct()
            assert [getattr(q, f) for f, _ in q._fields_] == [stride, off, pitch, pat, code]
            assert s.check() is s and s.sample == code
    # MSB-aligned: one code for every depth
    for bits in range(9, 17):
        s = SensorSurface(3, 7, bits=bits, container="u16msb")
        assert s.sample == U16(8) and s.shift == 8 and s.struct().reserved == U16(8)
    # every new rule has a text of its own, and the unknown code still says `reserved`
    texts = set()
    for d in ((3, 7, 42, 0, 12, 0, U16(4)), (3, 7, 40, 0, 14, 0, U16(4)), (3, 7, 60, 3, 16, 0, U16(0)),
              (3, 7, 42, 0, 14, 0, 1), (3, 7, 42, -2, 14, 0, U16(4))):
        assert lib.jh_sensor_surface_check(N.SensorSurfaceStruct(*d[2:]), d[0], d[1]) != 0
        texts.add(lib.jh_last_error())
    assert len(texts) == 5
    for code in (1, 0x109, 0x201, 0x400):
        assert lib.jh_sensor_surface_check(N.SensorSurfaceStruct(42, 0, 14, 0, code), 3, 7) != 0
        assert b"reserved" in lib.jh_last_error() and b"sample" in lib.jh_last_error()
    msgs = set()
    for kw in (dict(bits=12, pitch=12), dict(bits=12, image_stride=40), dict(bits=12, offset=1, image_stride=44),
               dict(bits=12, container="packed", pitch=10), dict(bits=8, container="packed"), dict(container="u12")):
        with pytest.raises(ValueError) as e:
            SensorSurface(3, 7, **kw)
        msgs.add(str(e.value).split(",")[0].split("(")[0])
    assert len(msgs) == 5                                 # (the two pitch cases share the pitch rule's text)


def test_sensor_surface_keywords():
    # the defaults are the objects and structs of the 8-bit descriptions
    s = SensorSurface(4, 6, "rggb", pitch=8, offset=2)
    assert (s.bits, s.container, s.sample, s.shift, s.row_bytes) == (8, "u8", 0, 0, 6)
    assert s == SensorSurface(4, 6, "rggb", pitch=8, offset=2, bits=8, container="u8")
    q = s.struct()
    assert [getattr(q, f) for f, _ in q._fields_] == [2 + 4 * 8, 2, 8, 1, 0]
    SM.check(4, 6, "rggb", 8, 2, 34)                      # (the positional form of earlier callers)
    # container defaults and tight pitches
    for kw, cont, pitch, code in ((dict(bits=12), "u16", 14, U16(4)), (dict(bits=16), "u16", 14, U16(8)),
                                  (dict(bits=8, container="u16"), "u16", 14, U16(0)),
                                  (dict(bits=10, container="u16msb"), "u16msb", 14, U16(8)),
                                  (dict(bits=10, container="packed"), "packed", 9, P10),
                                  (dict(bits=12, container="packed"), "packed", 11, P12)):
        t = SensorSurface(3, 7, **kw)
        assert (t.container, t.pitch, t.image_stride, t.sample) == (cont, pitch, 3 * pitch, code), kw
    # bits the container cannot hold
    for kw in (dict(bits=8, container="packed"), dict(bits=16, container="packed"), dict(bits=11, container="packed"),
               dict(bits=12, container="u8"), dict(bits=8, container="u16msb"), dict(bits=17), dict(bits=7),
               dict(bits=12.0), dict(bits=12, container="Packed")):
        with pytest.raises(ValueError):
            SensorSurface(3, 7, **kw)
    # equality, hash and repr see the new fields
    a, b = SensorSurface(3, 7, pitch=14, bits=12), SensorSurface(3, 7, pitch=14, bits=10)
    c = SensorSurface(3, 7, pitch=14, bits=16, container="u16msb")
    assert a != b and len({a, b, c, SensorSurface(3, 7, pitch=14, bits=12)}) == 3
    assert "bits=12" in repr(a) and "container='u16msb'" in repr(c)
    with pytest.raises(AttributeError):
        a.bits = 8


# (h, w, (image_stride, y_offset, y_pitch, u_offset, v_offset, c_pitch, c_step, matrix, range, sample)), valid?
YUV = [
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, U16(8))), True),     # tight P010
    ((4, 6, (72, 0, 12, 50, 48, 12, 2, 1, 1, U16(8))), True),     # the NV21 order
    ((4, 6, (72, 0, 12, 48, 60, 6, 1, 0, 0, U16(2))), True),      # tight yuv420p10le
    ((4, 6, (72, 0, 12, 60, 48, 6, 1, 0, 0, U16(4))), True),      # the YV12 order
    ((4, 6, (72, 0, 10, 48, 50, 12, 2, 0, 0, U16(8))), False),    # y_pitch below 2 w
    ((4, 6, (72, 0, 12, 48, 50, 10, 2, 0, 0, U16(8))), False),    # c_pitch below (w/2) * 2 * 2 (a multiple of 2 only)
    ((4, 6, (72, 0, 12, 48, 60, 4, 1, 0, 0, U16(2))), False),     # planar c_pitch below (w/2) * 2
    ((4, 6, (72, 0, 12, 48, 49, 12, 2, 0, 0, U16(8))), False),    # semi-planar U and V one BYTE apart
    ((4, 6, (76, 0, 12, 50, 52, 12, 2, 0, 0, U16(8))), False),    # the pair at 2 mod 4
    ((4, 6, (80, 0, 12, 48, 50, 14, 2, 0, 0, U16(8))), False),    # semi-planar c_pitch 2 mod 4
    ((4, 6, (80, 0, 12, 48, 64, 8, 1, 0, 0, U16(2))), True),      # (planar: a multiple of 2 is enough)
    ((4, 6, (80, 0, 12, 48, 64, 7, 1, 0, 0, U16(2))), False),     # odd c_pitch
    ((4, 6, (80, 1, 12, 52, 68, 8, 1, 0, 0, U16(2))), False),     # odd y_offset
    ((4, 6, (80, 0, 13, 52, 68, 8, 1, 0, 0, U16(2))), False),     # odd y_pitch
    ((4, 6, (80, 0, 12, 53, 68, 8, 1, 0, 0, U16(2))), False),     # odd u_offset
    ((4, 6, (80, 0, 12, 52, 69, 8, 1, 0, 0, U16(2))), False),     # odd v_offset
    ((4, 6, (73, 0, 12, 48, 60, 6, 1, 0, 0, U16(2))), False),     # odd image_stride
    ((4, 6, (70, 0, 12, 48, 60, 6, 1, 0, 0, U16(2))), False),     # the V plane's last sample ends at 72
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, U16(0))), True),     # 16-bit words that hold 8 bits
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, P10)), False),       # packed YUV
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, P12)), False),
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, 1)), False),         # unknown codes
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, 0x109)), False),
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, 0x201)), False),
    ((4, 6, (72, 0, 12, 48, 50, 12, 2, 0, 0, 0x400)), False),
]


def test_yuv_python_and_c_validation_agree():
    from jarvis_hybridnet_amd import _native as N
    lib = N.lib()
    mats, rngs = {v: k for k, v in YM.MATRICES.items()}, {v: k for k, v in YM.RANGES.items()}
    for (h, w, d), good in YUV:
        assert (lib.jh_yuv_surface_check(N.YuvSurfaceStruct(*d), h, w) == 0) == good, (d, lib.jh_last_error())
        code = d[9]
        if not 0x101 <= code <= 0x108:
            continue                                      # (Python cannot name the code: bits=8 is one byte)
        stride, yo, yp, uo, vo, cp, cs, m, r = d[:9]
        kw = dict(bits=16, msb=True) if code == U16(8) else dict(bits=8 + (code & 0xff))
        try:
            s = YuvSurface.from_planes(h, w, yo, yp, uo, vo, cp, cs, stride, matrix=mats[m], range=rngs[r], **kw)
            ok = True
        except ValueError:
            ok = False
        assert ok == good, d
        if good:
            q = s.struct()
            assert [getattr(q, f) for f, _ in q._fields_] == list(d)
    texts = set()
    for i in (4, 5, 7, 8, 12, 17, 21):                    # one violation per rule
        (h, w, d), good = YUV[i]
        assert not good and lib.jh_yuv_surface_check(N.YuvSurfaceStruct(*d), h, w) != 0
        texts.add(lib.jh_last_error())
    assert len(texts) == 7
    for code in (1, 0x109, 0x201, 0x400, P10, P12):
        assert lib.jh_yuv_surface_check(N.YuvSurfaceStruct(72, 0, 12, 48, 50, 12, 2, 0, 0, code), 4, 6) != 0
        assert b"reserved" in lib.jh_last_error() and b"sample" in lib.jh_last_error()


def test_yuv_surface_keywords():
    s = YuvSurface(4, 6)
    assert (s.bits, s.msb, s.sample) == (8, False, 0) and s == YuvSurface(4, 6, bits=8, msb=False)
    q = s.struct()
    assert [getattr(q, f) for f, _ in q._fields_] == [36, 0, 6, 24, 25, 6, 2, 0, 0, 0]
    YM.check(4, 6, 36, 0, 6, 24, 25, 6, 2, "bt601", "limited")                  # (the positional form)
    p010 = YuvSurface(4, 6, "nv12", bits=10, msb=True)
    assert (p010.y_pitch, p010.c_pitch, p010.u_offset, p010.v_offset, p010.image_stride) == (12, 12, 48, 50, 72)
    assert (p010.sample, p010.shift) == (U16(8), 8)
    le = YuvSurface(4, 6, "i420", bits=10)
    assert (le.y_pitch, le.c_pitch, le.u_offset, le.v_offset, le.image_stride, le.shift) == (12, 6, 48, 60, 72, 2)
    nv21 = YuvSurface(4, 6, "nv21", bits=12, y_pitch=16, c_pitch=16, luma_rows=6)
    assert (nv21.v_offset, nv21.u_offset, nv21.image_stride, nv21.sample) == (96, 98, 96 + 32, U16(4))
    assert p010 != YuvSurface(4, 6, "nv12", bits=12, msb=True) and p010 != YuvSurface(4, 6, "nv12", bits=16)
    assert len({p010, le, YuvSurface(4, 6, "nv12", bits=10, msb=True)}) == 2
    assert "bits=10" in repr(p010) and "msb=True" in repr(p010)
    for kw in (dict(bits=8, msb=True), dict(bits=17), dict(bits=7), dict(bits=10.0), dict(bits=10, msb=1),
               dict(bits=10, y_pitch=10), dict(bits=10, y_pitch=13), dict(bits=10, c_pitch=14)):
        with pytest.raises(ValueError):
            YuvSurface(4, 6, "nv12", **kw)


@pytest.mark.parametrize("bits", [10, 12])
def test_bit_stream_packer_round_trips(bits):
    g = np.random.default_rng(bits)
    for w in range(1, 10):
        a = g.integers(0, 1 << bits, (2, 3, w), dtype=np.uint16)
        p = S.pack_bits(a, bits)
        assert p.dtype == np.uint8 and p.shape == (2, 3, (bits * w + 7) // 8)
        assert np.array_equal(S.unpack_bits(p, bits, w), a)
        # an independent statement of the layout: sample x is bits [bits x, bits x + bits) of the row's integer
        for row, samples in zip(p.reshape(-1, p.shape[-1]), a.reshape(-1, w)):
            n = int.from_bytes(row.tobytes(), "little")
            assert [(n >> (bits * x)) & ((1 << bits) - 1) for x in range(w)] == samples.tolist()
            assert n >> (bits * w) == 0                   # the unused high bits of the last byte
    # PFNC's own example of Mono12p: two samples in three bytes, the low byte of the first sample first
    assert S.pack_bits(np.array([[0xABC, 0x123]]), 12).tolist() == [[0xBC, 0x3A, 0x12]]
    assert S.pack_bits(np.array([[0x3FF, 0, 0x3FF, 0]]), 10).tolist() == [[0xFF, 0x03, 0xF0, 0x3F, 0x00]]


def test_widen_and_reduce():
    g = np.random.default_rng(5)
    b = g.integers(0, 256, (4, 6, 10), dtype=np.uint8)
    b[0, 0] = 255
    b[1, 1] = 0
    for shift in range(9):
        w = S.widen(b, shift, g)
        assert w.dtype == np.uint16 and int(w.max()) < 1 << (8 + shift)
        assert np.array_equal(S.reduce_samples(w, shift), b)
        if shift:
            assert len(np.unique(w & ((1 << shift) - 1))) > 1          # the low bits are not all alike
        sat = S.widen(b, shift, g, saturate=True)
        assert np.array_equal(S.reduce_samples(sat, shift), b)
        if shift < 8:
            over = sat >> (8 + shift) != 0
            assert over.any() and (b[over] == 255).all()                # bits above the declared depth: still 255
    # saturation on its own
    assert S.reduce_samples(np.array([0x0FFF, 0x1000, 0xFFFF, 0x0FF0, 0x0FEF], np.uint16), 4).tolist() == \
        [255, 255, 255, 255, 254]
    assert S.reduce_samples(np.array([0x3FF, 0x400, 0x3FB], np.uint16), 2).tolist() == [255, 255, 254]
    assert S.reduce_samples(np.array([0xFFC0, 0x0040], np.uint16), 8).tolist() == [255, 0]
    with pytest.raises(ValueError):
        S.reduce_samples(np.zeros(3, np.float32), 2)


def test_wide_surface_packers():
    g = np.random.default_rng(9)
    raw = g.integers(0, 1 << 12, (2, 3, 7), dtype=np.uint16)
    # 16-bit words, pitched: little-endian, everything else is fill
    s = SensorSurface(3, 7, pitch=18, offset=4, image_stride=4 + 3 * 18 + 6, bits=12)
    buf = S.pack_sensor_surface(raw, s, 0xA5)
    assert buf.shape == (2, s.image_stride)
    rows = np.stack([buf[:, 4 + y * 18: 4 + y * 18 + 14] for y in range(3)], 1)
    assert np.array_equal(rows.reshape(2, 3, 7, 2)[..., 0] | (rows.reshape(2, 3, 7, 2)[..., 1].astype(np.uint16) << 8), raw)
    mask = np.ones(s.image_stride, bool)
    for y in range(3):
        mask[4 + y * 18: 4 + y * 18 + 14] = False
    assert (buf[:, mask] == 0xA5).all()
    # 12p, 7 samples = 10.5 bytes: the high nibble of a row's 11th byte takes the fill's bits
    p = SensorSurface(3, 7, pitch=13, offset=5, bits=12, container="packed")
    for fill in (0xA5, 0x5A):
        buf = S.pack_sensor_surface(raw, p, fill)
        for y in range(3):
            row = buf[:, 5 + y * 13: 5 + y * 13 + 11]
            assert np.array_equal(S.unpack_bits(row, 12, 7), raw[:, y])
            assert (row[:, 10] >> 4 == fill >> 4).all()
            assert (buf[:, 5 + y * 13 + 11: 5 + (y + 1) * 13] == fill).all()
    with pytest.raises(ValueError):
        S.pack_sensor_surface(raw.astype(np.uint8), p)
    # the 8-bit call is what it was
    r8 = g.integers(0, 256, (3, 7), dtype=np.uint8)
    assert np.array_equal(S.pack_sensor_surface(r8, SensorSurface(3, 7)), r8.reshape(-1))
    # 16-bit YUV: each sample two bytes at offset + row * pitch + column * c_step * 2
    y = g.integers(0, 1 << 10, (4, 6), dtype=np.uint16)
    u, v = g.integers(0, 1 << 10, (2, 2, 3), dtype=np.uint16)
    for order in ("i420", "yv12", "nv12", "nv21"):
        t = YuvSurface(4, 6, order, bits=10, y_pitch=16, c_pitch=16, luma_rows=5)
        buf = S.pack_yuv_surface(y, u, v, t, 0x5A).astype(np.uint16)

        def at(off):
            return buf[off] | (buf[off + 1] << 8)
        assert all(at(t.y_offset + r * 16 + 2 * c) == y[r, c] for r in range(4) for c in range(6))
        assert all(at(t.u_offset + r * 16 + 2 * c * t.c_step) == u[r, c] for r in range(2) for c in range(3))
        assert all(at(t.v_offset + r * 16 + 2 * c * t.c_step) == v[r, c] for r in range(2) for c in range(3))
        assert int((buf != 0x5A).sum()) <= 2 * (24 + 6 + 6)
    with pytest.raises(ValueError):
        S.pack_yuv_surface(y.astype(np.uint8), u, v, YuvSurface(4, 6, bits=10))
