"""CPU: per-joint 3D spread (jh_softargmax_spread, jh_predictor_set_spread / _get_spread, jh_predictor_debug_v2v) -- the
symbols in the header and the ctypes table, the spread3D.csv row and header, where the Spread3D stands in the return
value of every forward form (a stub native predictor behind the real methods), the driver's output_spread with a stub
predictor, and the camera-sharded path's refusal.  Every test uses a new symbol, function or keyword."""
import csv
import os
import re
from types import MethodType, SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = {"jh_softargmax_spread_workspace_bytes": N.c_int64, "jh_softargmax_spread": N.c_int,
       "jh_predictor_set_spread": N.c_int, "jh_predictor_get_spread": N.c_int, "jh_predictor_debug_v2v": N.c_int}


def test_symbols_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, restype in NEW.items():
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/jarvis_hip.h does not declare %s" % name
        params = [p for p in m.group(1).split(",") if p.strip()]
        res, args = N._SIGS[name]
        assert res is restype and len(args) == len(params), name
        assert name in N.symbols()
    # jh_softargmax_spread is jh_softargmax with three more outputs
    assert len(N._SIGS["jh_softargmax_spread"][1]) == len(N._SIGS["jh_softargmax"][1]) + 3
    lib = N.lib()
    assert lib.jh_abi_version() == N.ABI_VERSION == 4
    # validation needs no GPU: a null predictor is refused with a message
    assert lib.jh_predictor_set_spread(None, 1) != 0 and b"null predictor" in lib.jh_last_error()
    assert lib.jh_predictor_get_spread(None, None, None, None, None) != 0 and b"null predictor" in lib.jh_last_error()
    assert lib.jh_softargmax_spread_workspace_bytes(1, 23, 24) > lib.jh_softargmax_workspace_bytes(1, 23, 24)


def test_exported_from_the_package():
    import jarvis_hybridnet_amd as pkg
    from jarvis_hybridnet_amd._predictor import Spread3D
    assert pkg.Spread3D is Spread3D and Spread3D._fields == ("cov", "peak", "mass")


J, C = 3, 2
CFG = NS(KEYPOINT_NAMES=["a", "b", "c"], KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C))


def spread_of(ids):
    """The stub's Spread3D of frame sets `ids` (T,): cov[t, j] symmetric with entries 100 t + 10 j + (0 .. 5) in the
    order xx xy xz yy yz zz, peak[t, j] = (t, j, 0.5), mass = 1."""
    from jarvis_hybridnet_amd import Spread3D
    T = len(ids)
    six = ids[:, None, None] * 100 + torch.arange(J).float()[None, :, None] * 10 + torch.arange(6).float()
    cov = six[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(T, J, 3, 3)
    peak = torch.stack([ids[:, None].expand(T, J), torch.arange(J).float()[None].expand(T, J), torch.full((T, J), 0.5)], -1)
    return Spread3D(cov, peak, torch.ones(T, J))


def test_spread_row_and_header(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    s = spread_of(torch.tensor([2.0]))
    row = P.spread_row(s.cov[0], s.peak[0], J)
    assert len(row) == 9 * J and all(isinstance(v, np.float32) for v in row)
    assert [float(v) for v in row[:9]] == [200, 201, 202, 203, 204, 205, 2, 0, 0.5]
    assert [float(v) for v in row[9:18]] == [210, 211, 212, 213, 214, 215, 2, 1, 0.5]
    assert P.spread_row(None, None, J) == ["NaN"] * (9 * J)
    # the text: numpy float32 elements, as the confidences of data3D.csv
    third = np.float32(1) / np.float32(3)
    cov = torch.full((J, 3, 3), float(third))
    path = tmp_path / "row.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        P.create_header_spread(w, CFG)
        w.writerow(P.spread_row(cov, torch.zeros(J, 3), J))
    head1, head2, body = list(csv.reader(open(path)))
    assert len(head1) == len(head2) == len(body) == 9 * J
    assert head1 == ["a"] * 9 + ["b"] * 9 + ["c"] * 9
    assert head2 == ["cxx", "cxy", "cxz", "cyy", "cyz", "czz", "px", "py", "pz"] * J
    assert body[0] == str(third) == "0.33333334" and body[6] == "0.0"


# ---- the return value of every forward form --------------------------------------------------------------------------
class StubNative:
    """A native predictor of time batch T whose frame sets are all valid, or all invalid."""

    def __init__(self, T, valid):
        self.T, self.valid, self.calls = T, valid, []

    def set_calibration(self, *calib):
        pass

    set_calibration_frames = set_calibration

    def _forward(self, frames, out, mask, centers=None, spread=False):
        self.calls.append(spread)
        res = (torch.zeros(self.T, J, 3), torch.zeros(self.T, J), torch.full((self.T,), self.valid, dtype=torch.int32))
        return res + (spread_of(torch.arange(self.T).float()),) if spread else res

    def views2d(self, points, camera_mask=None):
        from jarvis_hybridnet_amd._predictor import Views2D
        return Views2D(*"abcde")


@pytest.fixture()
def owner(monkeypatch):
    """The real forward methods of JarvisPredictor3D on an object whose native predictors are StubNatives."""
    from jarvis_hybridnet_amd.prediction import jarvis3D as M
    monkeypatch.setattr(M, "check_native_seam", lambda p: None)
    monkeypatch.setattr(N, "dev", lambda t, dtype=torch.float32: t.to(dtype).contiguous())
    monkeypatch.setattr(N, "frame_images", lambda flat, lead, *a: N.Frames(0, 4, 6, None, tuple(lead), images=flat))
    o = NS(num_cameras=C, reproTool=NS(), natives={}, valid=1)
    o.native = lambda h, w, time_batch=1: o.natives.setdefault(time_batch, StubNative(time_batch, o.valid))
    for name in ("forward", "forward_uint8", "forward_yuv", "forward_surface", "forward_batch", "forward_images",
                 "_run", "_frame_mask"):
        setattr(o, name, MethodType(getattr(M.JarvisPredictor3D, name), o))
    o._single, o._batch = M.JarvisPredictor3D._single, M.JarvisPredictor3D._batch
    return o


def forms(o):
    from jarvis_hybridnet_amd import YuvSurface
    calib = (None, None, None)
    H, W = 4, 6
    surface = YuvSurface(H, W, "nv12")
    yield "forward", True, lambda **kw: o.forward(torch.zeros(C, 3, H, W), *calib, **kw)
    yield "forward_uint8", True, lambda **kw: o.forward_uint8(torch.zeros(C, H, W, 3, dtype=torch.uint8), *calib, **kw)
    yield "forward_yuv", True, lambda **kw: o.forward_yuv(torch.zeros(C, H * 3 // 2, W, dtype=torch.uint8), "nv12",
                                                           *calib, **kw)
    yield "forward_surface", True, lambda **kw: o.forward_surface(
        torch.zeros(C, surface.image_stride, dtype=torch.uint8), surface, *calib, **kw)
    cam, intr, dist = torch.zeros(C, 4, 3), torch.zeros(C, 3, 3), torch.zeros(C, 1, 5)
    yield "forward_batch", False, lambda **kw: o.forward_batch(torch.zeros(2, C, 3, H, W), cam, intr, dist, **kw)
    imgs = [[torch.zeros(3, H, W)] * C] * 2
    yield "forward_images", False, lambda **kw: o.forward_images(imgs, cam, intr, dist, **kw)


def test_return_value_of_every_forward_form(owner):
    from jarvis_hybridnet_amd import Spread3D
    from jarvis_hybridnet_amd._predictor import Views2D
    seen = []
    for name, single, fn in forms(owner):
        seen.append(name)
        lead = 2 if single else 3                               # (points, conf[, valid])
        assert len(fn()) == lead, name
        res = fn(return_spread=True)
        assert len(res) == lead + 1 and isinstance(res[-1], Spread3D), name
        res = fn(return_2d=True, return_spread=True)            # the spread follows Views2D
        assert len(res) == lead + 2 and isinstance(res[-2], Views2D) and isinstance(res[-1], Spread3D), name
        assert len(fn(return_2d=True)) == lead + 1 and isinstance(fn(return_2d=True)[-1], Views2D), name
    assert seen == ["forward", "forward_uint8", "forward_yuv", "forward_surface", "forward_batch", "forward_images"]
    # the flag reaches the native predictor only when it is asked for: a call without it is the call it always was
    assert [n.calls[:4] for n in owner.natives.values()][0] == [False, True, True, False]
    # an invalid frame set: every element of a single-frame form is None
    owner.natives.clear()
    owner.valid = 0
    for name, single, fn in forms(owner):
        if single:
            assert fn(return_spread=True) == (None, None, None), name
            assert fn(return_2d=True, return_spread=True) == (None, None, None, None), name
            assert fn() == (None, None), name


# ---- the driver --------------------------------------------------------------------------------------------------------
class StubBatch:
    """The batch interface: frame set k is valid iff k is even; its spread is spread_of(k)."""

    def __init__(self):
        self.calls = []

    def forward_batch(self, x, *calib, **kw):
        self.calls.append(kw)
        T = x.shape[0]
        ids = x.reshape(T, -1)[:, 0].float()
        pts = ids[:, None, None] + torch.zeros(1, J, 3)
        res = (pts, torch.full((T, J), 0.5), (ids.int() % 2 == 0).int())
        return res + (spread_of(ids),) if kw.get("return_spread") else res


def test_driver_writes_spread3d_csv(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    sets = [np.full((C, 4, 6, 3), i, dtype=np.uint8) for i in range(5)]
    plain, pred = StubBatch(), StubBatch()
    a, b = str(tmp_path / "plain"), str(tmp_path / "spread")
    assert P.predict3D_frames(plain, iter(sets), None, None, None, CFG, a, time_batch=2) == 5
    assert P.predict3D_frames(pred, iter(sets), None, None, None, CFG, b, time_batch=2, output_spread=True) == 5
    assert plain.calls == [{}] * 3 and pred.calls == [{"return_spread": True}] * 3
    assert not os.path.exists(os.path.join(a, "spread3D.csv"))
    assert open(os.path.join(a, "data3D.csv"), "rb").read() == open(os.path.join(b, "data3D.csv"), "rb").read()
    rows = list(csv.reader(open(os.path.join(b, "spread3D.csv"))))
    assert len(rows) == 2 + 5 and all(len(r) == 9 * J for r in rows)
    for k, row in enumerate(rows[2:]):
        if k % 2:
            assert row == ["NaN"] * (9 * J)
        else:
            s = spread_of(torch.tensor([float(k)]))
            assert row == [str(v) for v in P.spread_row(s.cov[0], s.peak[0], J)]
    release_ingest_buffers(plain)
    release_ingest_buffers(pred)


def test_sharded_path_refuses_the_spread():
    from jarvis_hybridnet_amd.distributed import ShardedPredictor

    class Stages:                                   # never reached: the refusal comes first
        def __getattr__(self, name):
            raise AssertionError("stage call %s before the argument check" % name)

    sh = ShardedPredictor(Stages(), num_cameras=4, num_joints=3, time_batch=2, heat_shape=(8, 8, 8), rank=0, world=1,
                          device="cpu")
    x = torch.zeros(2, 4, 3, 16, 16)
    with pytest.raises(ValueError, match="3D spread"):
        sh.submit(x, return_spread=True)
    with pytest.raises(ValueError, match="3D spread"):
        sh.step(x, return_spread=True)
