"""CPU: per-camera tone tables (jh_predictor_set_tone) -- the ToneTables constructors and their validation, the new
symbols in the header and the ctypes table, the drivers' `tone=` with stub predictors (the pattern of
tests/test_centers_cpu.py), and the condition the GPU tests rest on: the CPU oracle returns a valid result on the cfg2
and cfg2_edge frames mapped through the tables those tests use."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import ToneTables
from jarvis_hybridnet_amd import _native as N
from jarvis_hybridnet_amd.tone import check_tone
from tests import tone_cases

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
F32 = np.float32


# ---- constructors ----------------------------------------------------------------------------------------------------
def test_identity():
    t = ToneTables.identity(3)
    want = np.arange(256, dtype=F32) * (F32(1) / F32(255))
    assert t.tables.shape == (3, 3, 256) and t.tables.dtype == F32 and t.cameras == 3
    for c in range(3):
        for ch in range(3):
            assert np.array_equal(t.tables[c, ch].view(np.uint32), want.view(np.uint32))
    assert t.tables.flags.c_contiguous and not t.tables.flags.writeable
    assert t == ToneTables.identity(3) and t != ToneTables.identity(2)


def test_from_bytes():
    g = np.random.default_rng(1)
    lut = g.integers(0, 256, (2, 3, 256), dtype=np.uint8)
    t = ToneTables.from_bytes(lut)
    want = lut.astype(F32) * (F32(1) / F32(255))
    assert np.array_equal(t.tables.view(np.uint32), want.view(np.uint32))
    one = ToneTables.from_bytes(lut[0])                                   # (3,256): one camera
    assert one.cameras == 1 and np.array_equal(one.tables[0], t.tables[0])
    ident = ToneTables.from_bytes(np.broadcast_to(np.arange(256, dtype=np.uint8), (2, 3, 256)))
    assert ident == ToneTables.identity(2)
    for bad in (lut.astype(np.int32), lut[:, :2], lut[:, :, :255], np.zeros((0, 3, 256), np.uint8), lut[None]):
        with pytest.raises(ValueError):
            ToneTables.from_bytes(bad)


def test_from_curve():
    t = tone_cases.tables()
    assert t.cameras == 4
    k = np.arange(256, dtype=np.float64)
    for c in range(4):
        for ch in range(3):
            lin = tone_cases.GAIN[c][ch] * (k - tone_cases.BLACK[c]) / (tone_cases.WHITE[c] - tone_cases.BLACK[c])
            want = (np.clip(lin, 0.0, 1.0) ** (1.0 / tone_cases.GAMMA[c])).astype(F32)      # rounded once
            assert np.array_equal(t.tables[c, ch].view(np.uint32), want.view(np.uint32)), (c, ch)
            assert np.all(np.diff(t.tables[c, ch]) >= 0), (c, ch)                            # monotone
            assert t.tables[c, ch].min() >= 0.0 and t.tables[c, ch].max() <= 1.0
    # the cameras differ, and so do the channels of a camera with white-balance gains
    assert not np.array_equal(t.tables[0], t.tables[1]) and not np.array_equal(t.tables[1, 0], t.tables[1, 2])
    # defaults: the identity curve in float64, k / 255 rounded once (not the float32 product of `identity`)
    d = ToneTables.from_curve(2)
    assert np.array_equal(d.tables[1, 2], (k / 255.0).astype(F32))
    # scalars, (3,) gains and per-camera values broadcast alike
    a = ToneTables.from_curve(2, black=3, white=250, gain=(1.1, 1.0, 0.9), gamma=1.2)
    b = ToneTables.from_curve(2, black=[3, 3], white=[250, 250], gain=[[1.1, 1.0, 0.9]] * 2, gamma=[1.2, 1.2])
    assert a == b
    assert ToneTables.from_curve(1, gain=2.0).tables[0, 0, 200] == 1.0                       # clipped


@pytest.mark.parametrize("kw", [
    dict(black=255, white=255), dict(black=10, white=5), dict(gamma=0), dict(gamma=-1.0), dict(gamma=float("nan")),
    dict(gain=float("inf")), dict(gain=(1, 1)), dict(gain=np.ones((3, 3))), dict(black=[1, 2, 3]),
    dict(white=np.ones((2, 2))), dict(gamma=[[1.0, 1.0]]),
])
def test_from_curve_rejects(kw):
    with pytest.raises(ValueError):
        ToneTables.from_curve(2, **kw)


def test_constructor_validation():
    good = np.zeros((2, 3, 256), F32)
    assert ToneTables(good).cameras == 2 and ToneTables(good[0]).cameras == 1
    assert ToneTables(good.astype(np.float64)).tables.dtype == F32
    for bad in (np.zeros((2, 3, 255), F32), np.zeros((2, 4, 256), F32), np.zeros((256,), F32),
                np.zeros((0, 3, 256), F32), np.zeros((1, 2, 3, 256), F32), np.zeros((2, 3, 256), bool),
                np.zeros((2, 3, 256), np.complex64)):
        with pytest.raises(ValueError):
            ToneTables(bad)
    for v in (np.nan, np.inf, -np.inf, 1e39):                                # (1e39: not finite in float32)
        x = good.astype(np.float64)
        x[1, 2, 77] = v
        with pytest.raises(ValueError, match="finite"):
            ToneTables(x)
    for n in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            ToneTables.identity(n)
    assert check_tone(None, 4) is None
    assert check_tone(good, 2).cameras == 2 and check_tone(ToneTables(good), 2).cameras == 2
    with pytest.raises(ValueError, match="2 cameras given to a predictor of 4"):
        check_tone(good, 4)


# ---- symbols ---------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    assert re.search(r"#define JH_ABI_VERSION\s+4\b", text)
    for phrase in ("more than 8 bits", "colour-correction matrix", "before the demosaic",
                   "rounding instead of truncation", "tone tables apply to byte frames"):
        assert phrase in text, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("jh_predictor_set_tone", 3), ("jh_predictor2d_set_tone", 3), ("jh_op_frames_to_rgb_f32", 12)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "include/jarvis_hip.h does not declare %s" % name
        res, args = N._SIGS[name]
        assert res is N.c_int and len(args) == len([p for p in m.group(1).split(",") if p.strip()]) == n_args, name
        assert name in N.symbols() and hasattr(N.lib(), name)
    lib = N.lib()
    assert lib.jh_abi_version() == N.ABI_VERSION == 4
    # validation needs no GPU: a null predictor is refused with a message
    assert lib.jh_predictor_set_tone(None, None, None) != 0 and b"null predictor" in lib.jh_last_error()
    assert lib.jh_predictor2d_set_tone(None, None, None) != 0 and b"null predictor" in lib.jh_last_error()
    assert lib.jh_op_frames_to_rgb_f32(None, 1, None, None, None, 1, 4, 4, None, 0, None, None) != 0
    import jarvis_hybridnet_amd as P
    from jarvis_hybridnet_amd._predictor import MultiStreamPredictor, NativePredictor
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D, _Native2D
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    assert P.ToneTables is ToneTables
    for cls in (NativePredictor, MultiStreamPredictor, JarvisPredictor3D, JarvisPredictor2D, _Native2D):
        assert callable(getattr(cls, "set_tone")), cls


# ---- driver plumbing -------------------------------------------------------------------------------------------------
J, C = 3, 2
CFG = NS(KEYPOINT_NAMES=["a", "b", "c"], KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C))


class Stub3D:
    def __init__(self):
        self.events = []

    def set_tone(self, tone):
        self.events.append(("tone", tone))

    def forward_batch(self, x, *calib, **kw):
        self.events.append(("forward", kw))
        T = x.shape[0]
        return torch.zeros(T, J, 3), torch.full((T, J), 0.5), torch.ones(T, dtype=torch.int32)


class Stub2D(Stub3D):
    def forward_batch(self, x, **kw):
        self.events.append(("forward", kw))
        T = x.shape[0]
        return torch.zeros(T, J, 2, dtype=torch.int32), torch.full((T, J), 0.5), torch.ones(T, dtype=torch.int32)


def test_drivers_pass_tone_through(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict2D as P2
    from jarvis_hybridnet_amd.prediction import predict3D as P3
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    tone = ToneTables.identity(C)
    sets = [np.full((C, 4, 6, 3), i, dtype=np.uint8) for i in range(3)]
    pred = Stub3D()
    assert P3.predict3D_frames(pred, iter(sets), None, None, None, CFG, str(tmp_path / "a"), time_batch=2,
                               tone=tone) == 3
    # the tables are set once, before the first forward; the forwards are called as they always were
    assert pred.events[0] == ("tone", tone) and [e for e in pred.events[1:]] == [("forward", {})] * 2
    pred = Stub3D()
    assert P3.predict3D_frames(pred, iter(sets), None, None, None, CFG, str(tmp_path / "b"), time_batch=2) == 3
    assert pred.events == [("forward", {})] * 2                          # no tone: set_tone is not called at all
    release_ingest_buffers(pred)
    one = ToneTables.identity(1)
    frames = [s[0] for s in sets]
    p2 = Stub2D()
    assert P2.predict2D_frames(p2, iter(frames), CFG, str(tmp_path / "c"), time_batch=2, tone=one) == 3
    assert p2.events[0] == ("tone", one) and p2.events[1:] == [("forward", {})] * 2
    p2 = Stub2D()
    done = P2.predict2D_recordings(p2, {"rec.mp4": iter(frames)}, CFG, str(tmp_path / "d"), time_batch=2, tone=one)
    assert done == {"data2D.csv": 3} and p2.events[0] == ("tone", one)
    p2 = Stub2D()
    P2.predict2D_recordings(p2, {"rec.mp4": iter(frames)}, CFG, str(tmp_path / "e"), time_batch=2)
    assert all(e[0] == "forward" for e in p2.events)
    release_ingest_buffers(p2)


# ---- the tables of the GPU tests are usable --------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["cfg2", "cfg2_edge"])
@pytest.mark.parametrize("which", ["tables", "other_tables"])
def test_oracle_is_valid_on_the_mapped_frames(tag, which):
    """The GPU tests compare a forward under tables with the fp32 forward on the mapped frames: both sides being
    invalid would pass by agreeing.  The reference (CPU oracle) detects the subject on those frames."""
    from jarvis_hybridnet_amd import synthetic as S
    from oracle import hybridnet_oracle as O
    from tests import cases
    from tests.test_hip_yuv_ingest import to_bgr_u8
    c = cases.PREDICTOR_CASES[tag]
    inp = cases.predictor_inputs(tag)
    tone = getattr(tone_cases, which)()
    assert tone.cameras == c["C"]
    imgs = torch.from_numpy(tone_cases.mapped_rgb(to_bgr_u8(inp["imgs"]), tone))
    assert tuple(imgs.shape) == tuple(inp["imgs"].shape)
    with torch.no_grad():
        pts, conf = O.predictor3d_forward(inp["sd_center"], inp["sd_hybrid"], imgs, inp["cam"], inp["intr"],
                                          inp["dist"], center_size=c["center_size"], bbox=c["bbox"],
                                          roi_cube_size=c["roi"], grid_spacing=c["spacing"], mean=S.MEAN, std=S.STD)
    assert pts is not None and torch.isfinite(pts).all() and torch.isfinite(conf).all()
