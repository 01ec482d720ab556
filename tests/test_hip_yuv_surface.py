"""GPU: described YUV 4:2:0 surfaces (YuvSurface / jh_yuv_surface).  The contract is bitwise: what is read through a
description equals the uint8 BGR path on the bytes the numpy reference (tests/test_yuv_surface_cpu.py:
surface_to_bgr) converts the surface to -- the stand-alone conversion over all 2^24 triples of every constant row,
every plane order with padded pitches and poisoned padding, the 3D predictor (fused and stand-alone stems, graph
replay, layout changes under replay, time batches, masks, 2D views), the 2D predictor and the driver."""
import os

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases
from tests.gpu_util import cuda
from tests.test_hip_predictor import make_cfg
from tests.test_hip_yuv_ingest import _assert_same, _debug, to_bgr_u8
from tests.test_yuv_surface_cpu import ORDERS, ROWS, surface_to_bgr

pytestmark = pytest.mark.gpu


def op_to_bgr(buf, s):
    """jh_op_yuv_surface_to_bgr on (n, image_stride) numpy bytes -> (n, H, W, 3) numpy."""
    from jarvis_hybridnet_amd import _native as N
    x = cuda(torch.from_numpy(buf))
    out = torch.empty((buf.shape[0], s.height, s.width, 3), dtype=torch.uint8, device="cuda")
    N.check(N.lib().jh_op_yuv_surface_to_bgr(N.ptr(x), s.struct(), buf.shape[0], s.height, s.width, N.ptr(out),
                                             N.stream()))
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def all_triples():
    """The 64 x 512^2 construction of test_yuv420_to_bgr_op_exhaustive as tight NV12 bytes: the chroma planes
    enumerate the 65 536 (U, V) pairs, the 2 x 2 luma blocks of frame f hold Y = 4f .. 4f+3."""
    F = 64
    cu, cv = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    blk = (4 * np.arange(F, dtype=np.int64))[:, None, None] + np.array([[0, 1], [2, 3]])[None]
    Y = np.tile(blk, (1, 256, 256)).astype(np.uint8)
    buf = S.pack_yuv420(Y, np.broadcast_to(cu, (F, 256, 256)), np.broadcast_to(cv, (F, 256, 256)), "nv12")
    return np.ascontiguousarray(buf.reshape(F, -1))


@pytest.mark.parametrize("matrix,rng", list(ROWS))
def test_surface_to_bgr_op_exhaustive(all_triples, matrix, rng):
    s = YuvSurface(512, 512, "nv12", matrix=matrix, range=rng)
    got = op_to_bgr(all_triples, s)
    for f0 in range(0, 64, 16):
        assert np.array_equal(got[f0:f0 + 16], surface_to_bgr(all_triples[f0:f0 + 16], s)), (matrix, rng, f0)


def padded(H, W, order, **kw):
    """The layout of the issue: y_pitch W + 6, c_pitch minimal + 4 (planar) / + 6 (semi-planar), luma_rows H + 3 and a
    10-byte gap before image_stride."""
    semi = order.startswith("nv")
    args = dict(y_pitch=W + 6, c_pitch=(W + 6) if semi else W // 2 + 4, luma_rows=H + 3, **kw)
    return YuvSurface(H, W, order, image_stride=YuvSurface(H, W, order, **args).image_stride + 10, **args)


@pytest.mark.parametrize("H,W", [(6, 10), (34, 66)])
def test_layouts_and_poisoned_padding(H, W):
    g = np.random.default_rng(W)
    y = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    u, v = g.integers(0, 256, (2, 3, H // 2, W // 2), dtype=np.uint8)
    from jarvis_hybridnet_amd import _native as N
    for i, order in enumerate(ORDERS):
        matrix, rng = list(ROWS)[i]
        s = padded(H, W, order, matrix=matrix, range=rng)
        want = surface_to_bgr(S.pack_yuv_surface(y, u, v, s, 0), s)
        for fill in (0xA5, 0x5A):
            assert np.array_equal(op_to_bgr(S.pack_yuv_surface(y, u, v, s, fill), s), want), (order, fill)
        # an odd image_stride (and with it odd image addresses): the semi-planar pair is fetched byte by byte
        s1 = YuvSurface.from_planes(H, W, s.y_offset, s.y_pitch, s.u_offset, s.v_offset, s.c_pitch, s.c_step,
                                    s.image_stride + 1, matrix=matrix, range=rng)
        assert np.array_equal(op_to_bgr(S.pack_yuv_surface(y, u, v, s1, 0x33), s1), want), (order, "odd stride")
    bad = YuvSurface(H, W).struct()
    bad.c_step = 3
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="c_step"):
        N.check(N.lib().jh_op_yuv_surface_to_bgr(N.ptr(x), bad, 1, H, W, N.ptr(x), N.stream()))


def surface_frames(bgr, s, fill=0xA5):
    """uint8 BGR (..., H, W, 3) -> (frames (..., image_stride) of the surface `s`, the BGR bytes its conversion
    gives) as torch CPU tensors; the content goes through the forward transform of the surface's own matrix."""
    buf = S.pack_yuv_surface(*S.bgr_to_yuv(bgr, s.matrix, s.range), s, fill)
    return torch.from_numpy(buf), torch.from_numpy(surface_to_bgr(buf, s))


@pytest.fixture(scope="module")
def cfg2():
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    bgr = to_bgr_u8(inp["imgs"])
    bgr2 = np.ascontiguousarray(np.roll(bgr, (24, -40), axis=(1, 2)))
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]

    def make():
        return JarvisPredictor3D(make_cfg(c, c["center_size"]), inp["sd_center"], inp["sd_hybrid"])
    return dict(c=c, inp=inp, bgr=bgr, bgr2=bgr2, dev=dev, make=make, H=c["H"], W=c["W"])


def layouts(H, W):
    return {"nv12_pitched_709": YuvSurface(H, W, "nv12", matrix="bt709", y_pitch=768, c_pitch=768, luma_rows=544),
            "yv12_tight_601_full": YuvSurface(H, W, "yv12", range="full"),
            "nv21_709_full_gap": YuvSurface(H, W, "nv21", matrix="bt709", range="full",
                                            image_stride=H * W * 3 // 2 + 1000)}


@pytest.mark.parametrize("name,stem_fuse", [("nv12_pitched_709", None), ("yv12_tight_601_full", None),
                                            ("nv21_709_full_gap", None), ("nv12_pitched_709", "0")])
def test_predictor3d_surface_bitwise(cfg2, name, stem_fuse, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)       # read when a launch plan is built
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    assert (H, W) == (512, 640)
    s = layouts(H, W)[name]
    pred = cfg2["make"]()
    x1, ref1 = surface_frames(cfg2["bgr"], s)
    x2, ref2 = surface_frames(cfg2["bgr2"], s, 0x5A)
    assert pred.native(H, W).graph_replay
    for _ in range(2):                                      # the second call replays the captured graph
        got = pred.forward_surface(cuda(x1), s, *dev)
        torch.cuda.synchronize()
        dbg_s = _debug(pred, H, W)
        want = pred.forward_uint8(cuda(ref1), *dev)
        torch.cuda.synchronize()
        dbg_b = _debug(pred, H, W)
        _assert_same(got, want, (name, "single"))
        assert want[0] is not None                          # two invalid outputs cannot pass by agreeing
        for k in dbg_b:
            assert torch.equal(dbg_s[k], dbg_b[k]), (name, k)
    x = cuda(torch.stack([x1, x2, x2, x1]))
    xb = cuda(torch.stack([ref1, ref2, ref2, ref1]))
    got = [t.clone() for t in pred.forward_batch(x, *dev, frame_layout=s)]
    torch.cuda.synchronize()
    dbg_s = {k: v.clone() for k, v in pred.native(H, W, time_batch=4).debug("cuda").items()}
    want = [t.clone() for t in pred.forward_batch(xb, *dev)]
    torch.cuda.synchronize()
    dbg_b = {k: v.clone() for k, v in pred.native(H, W, time_batch=4).debug("cuda").items()}
    for a, b in zip(got, want):
        assert torch.equal(a, b), (name, "batch")
    for k in dbg_b:
        assert torch.equal(dbg_s[k], dbg_b[k]), (name, "batch", k)
    assert int(want[2].sum()) == 4 and not torch.equal(want[0][0], want[0][1])
    # which path ran: only the stand-alone kernels are launched (and profiled) as preprocess_resize / _crop
    xs = cuda(x1).unsqueeze(0)
    names = {r[0] for r in N.profile(lambda: pred.native(H, W).forward(xs, frame_layout=s))}
    pre = names & {"preprocess_resize", "preprocess_crop"}
    if stem_fuse == "0":
        assert pre == {"preprocess_resize", "preprocess_crop"}, "JH_STEM_FUSE=0 had no effect"
    else:
        assert not pre and any(n.startswith("stem_conv") for n in names), names


def test_tight_nv12_surface_equals_forward_yuv(cfg2):
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    pred = cfg2["make"]()
    yuv = torch.from_numpy(S.bgr_to_yuv420(cfg2["bgr"], "nv12"))
    want = pred.forward_yuv(cuda(yuv), "nv12", *dev)
    got = pred.forward_surface(cuda(yuv.reshape(yuv.shape[0], -1)), YuvSurface(H, W, "nv12"), *dev)
    torch.cuda.synchronize()
    _assert_same(got, want, "tight nv12")
    assert want[0] is not None


def test_layout_change_under_replay(cfg2):
    """One graph-replaying predictor called with layout A, then B (another pitch and matrix), then A: every call
    equals a fresh predictor's result for its layout."""
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    kw = dict(num_cameras=c["C"], num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN, std=S.STD, time_batch=1)
    A = YuvSurface(H, W, "nv12", matrix="bt709", y_pitch=768, c_pitch=768)
    B = YuvSurface(H, W, "nv12", matrix="bt601", y_pitch=704, c_pitch=704)
    frames = {n: cuda(surface_frames(cfg2["bgr"], s)[0]).unsqueeze(0) for n, s in (("A", A), ("B", B))}
    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert g.graph_replay
    g.set_calibration(*dev)
    first = {}
    for n, s in (("A", A), ("B", B), ("A", A)):
        got = [t.clone() for t in g.forward(frames[n].clone(), frame_layout=s)]
        fresh = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
        fresh.set_calibration(*dev)
        want = [t.clone() for t in fresh.forward(frames[n], frame_layout=s)]
        torch.cuda.synchronize()
        fresh.close()
        for a, b in zip(got, want):
            assert torch.equal(a, b), n
        assert int(got[2][0]) == 1
        assert torch.equal(first.setdefault(n, got[0]), got[0])
    assert not torch.equal(first["A"], first["B"])           # (BT.709 bytes read as BT.601: other colours, other points)
    g.close()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_mask_and_views2d_behind_a_surface(cfg2):
    H, W, dev, C = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["c"]["C"]
    s = layouts(H, W)["nv12_pitched_709"]
    pred = cfg2["make"]()
    x, ref = surface_frames(cfg2["bgr"], s)
    mask = [c != 1 for c in range(C)]
    got = pred.forward_surface(cuda(x), s, *dev, camera_mask=mask, return_2d=True)
    want = pred.forward_uint8(cuda(ref), *dev, camera_mask=mask, return_2d=True)
    torch.cuda.synchronize()
    assert want[0] is not None and got[0] is not None
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    for f in want[2]._fields:                                # NaNs compared bitwise
        assert torch.equal(_bits(getattr(got[2], f)), _bits(getattr(want[2], f))), f
    assert int(want[2].used[0, 1]) == 0 and int(want[2].used.sum()) == C - 1
    # the batch form, masked rows differing
    xb = cuda(torch.stack([x, x]))
    rb = cuda(torch.stack([ref, ref]))
    m2 = [mask, [True] * C]
    got = pred.forward_batch(xb, *dev, frame_layout=s, camera_mask=m2, return_2d=True)
    want = pred.forward_batch(rb, *dev, camera_mask=m2, return_2d=True)
    torch.cuda.synchronize()
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(_bits(a), _bits(b))
    for f in want[3]._fields:
        assert torch.equal(_bits(getattr(got[3], f)), _bits(getattr(want[3], f))), f
    assert int(want[2].sum()) == 2


def test_predictor2d_surface_bitwise():
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    tags = ["cam0_j12", "cam2_j12"]
    c = cases.PREDICTOR2D_CASES[tags[0]]
    ins = [cases.predictor2d_inputs(t) for t in tags]
    cfg = make_cfg(dict(J=c["J"], bbox=c["bbox"], C=1, roi=32, spacing=2), c["center_size"])
    pred = JarvisPredictor2D(cfg, ins[0]["sd_center"], ins[0]["sd_kp"])
    bgr = np.concatenate([to_bgr_u8(i["img"]) for i in ins])                  # (2, H, W, 3)
    H, W = bgr.shape[1:3]
    s = YuvSurface(H, W, "i420", matrix="bt709", range="full", y_pitch=W + 64, c_pitch=W // 2 + 32, luma_rows=H + 16)
    x, ref = surface_frames(bgr, s)
    got = [t.clone() for t in pred.forward_batch(cuda(x), frame_layout=s)]
    want = [t.clone() for t in pred.forward_batch(cuda(ref))]
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert int(want[2].sum()) == 2
    p1, c1 = pred.forward_surface(cuda(x[0]), s)
    p2, c2 = pred.forward(cuda(x[:1]), frame_layout=s)
    w1 = pred.forward_batch(cuda(ref[:1]))
    torch.cuda.synchronize()
    assert torch.equal(p1, w1[0][0].long()) and torch.equal(c1, w1[1][0])
    assert torch.equal(p2, p1) and torch.equal(c2, c1)


def _read(path, name):
    return open(os.path.join(path, name), newline="").read()


def test_driver_surface_csv_identical(cfg2, tmp_path):
    """predict3D_frames(frame_layout=s) from numpy frame sets and from device-resident ones writes a data3D.csv
    byte-identical to the BGR run on the reference bytes; info.yaml does not change."""
    from types import SimpleNamespace as NS
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    cfg = make_cfg(c, c["center_size"])
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = (inp["cam"], inp["intr"], inp["dist"])
    pred = cfg2["make"]()
    s = layouts(H, W)["nv12_pitched_709"]
    pairs = [surface_frames(to_bgr_u8(S.blob_frames(calib, W, H, c["J"], 70 + i)[0]), s) for i in range(6)]
    yuv = [p[0].numpy() for p in pairs]
    ref = [p[1].numpy() for p in pairs]
    kw = dict(time_batch=4, streams=2)

    def params():
        return NS(recording_path="rec", dataset_name="d", frame_start=0, number_frames=6)
    assert predict3D_frames(pred, yuv, *dev, cfg, str(tmp_path / "y"), params(), frame_layout=s, **kw) == 6
    assert predict3D_frames(pred, [cuda(torch.from_numpy(a)) for a in yuv], *dev, cfg, str(tmp_path / "d"), params(),
                            frame_layout=s, **kw) == 6
    assert predict3D_frames(pred, ref, *dev, cfg, str(tmp_path / "b"), params(), **kw) == 6
    release_ingest_buffers(pred)
    want = _read(tmp_path / "b", "data3D.csv")
    assert _read(tmp_path / "y", "data3D.csv") == want and _read(tmp_path / "d", "data3D.csv") == want
    assert _read(tmp_path / "y", "info.yaml") == _read(tmp_path / "b", "info.yaml") == _read(tmp_path / "d", "info.yaml")
    rows = want.splitlines()[2:]
    assert len(rows) == 6 and len(set(rows)) == 6 and all(not r.startswith("NaN") for r in rows)
