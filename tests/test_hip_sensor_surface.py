"""GPU: raw sensor surfaces (SensorSurface / jh_sensor_surface).  The contract is bitwise: what is read through a
description equals the uint8 BGR path on the bytes the numpy reference (synthetic.sensor_to_bgr, whose properties
tests/test_sensor_surface_cpu.py checks) demosaics the raw image to -- the stand-alone conversion with poisoned
padding, the 3D predictor (fused and stand-alone stems, graph replay, a pattern change under replay, time batches,
crop windows on the frame's border, masks, 2D views), the 2D predictor and both drivers."""
import os

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases
from tests.gpu_util import cuda
from tests.test_hip_predictor import make_cfg
from tests.test_hip_yuv_ingest import _assert_same, _debug, to_bgr_u8

pytestmark = pytest.mark.gpu

PATTERNS = ("mono", "rggb", "bggr", "grbg", "gbrg")


def op_to_bgr(buf, s):
    """jh_op_sensor_to_bgr on (n, image_stride) numpy bytes -> (n, H, W, 3) numpy."""
    from jarvis_hybridnet_amd import _native as N
    x = cuda(torch.from_numpy(buf))
    out = torch.empty((buf.shape[0], s.height, s.width, 3), dtype=torch.uint8, device="cuda")
    N.check(N.lib().jh_op_sensor_to_bgr(N.ptr(x), s.struct(), buf.shape[0], s.height, s.width, N.ptr(out), N.stream()))
    return out.cpu().numpy()


def pitched(H, W, pattern):
    """Row pitch W + 6, the first sample at byte 9 and a 10-byte gap behind the last row."""
    return SensorSurface(H, W, pattern, pitch=W + 6, offset=9, image_stride=9 + H * (W + 6) + 10)


@pytest.mark.parametrize("H,W", [(4, 4), (6, 10), (34, 66)])
def test_sensor_to_bgr_op(H, W):
    from jarvis_hybridnet_amd import _native as N
    raw = np.random.default_rng(H * 100 + W).integers(0, 256, (3, H, W), dtype=np.uint8)
    for p in PATTERNS:
        want = S.sensor_to_bgr(raw, p)
        tight = SensorSurface(H, W, p)
        assert np.array_equal(op_to_bgr(S.pack_sensor_surface(raw, tight), tight), want), (p, "tight")
        s = pitched(H, W, p)
        for fill in (0xA5, 0x5A):                        # no byte that is not a sample reaches the output
            assert np.array_equal(op_to_bgr(S.pack_sensor_surface(raw, s, fill), s), want), (p, fill)
    bad = SensorSurface(H, W).struct()
    bad.pattern = 7
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="pattern"):
        N.check(N.lib().jh_op_sensor_to_bgr(N.ptr(x), bad, 1, H, W, N.ptr(x), N.stream()))


def sensor_frames(bgr, s, fill=0xA5):
    """uint8 BGR (..., H, W, 3) -> (frames (..., image_stride) of the surface `s`, the BGR bytes its conversion
    gives) as torch CPU tensors: the mosaic of the frames (mono: their green channel)."""
    raw = S.mosaic(bgr, s.pattern)
    return torch.from_numpy(S.pack_sensor_surface(raw, s, fill)), torch.from_numpy(S.sensor_to_bgr(raw, s.pattern))


def _case(tag):
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES[tag]
    inp = cases.predictor_inputs(tag)
    bgr = to_bgr_u8(inp["imgs"])
    bgr2 = np.ascontiguousarray(np.roll(bgr, (24, -40), axis=(1, 2)))
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]

    def make():
        return JarvisPredictor3D(make_cfg(c, c["center_size"]), inp["sd_center"], inp["sd_hybrid"])
    return dict(c=c, inp=inp, bgr=bgr, bgr2=bgr2, dev=dev, make=make, H=c["H"], W=c["W"])


@pytest.fixture(scope="module")
def cfg2():
    return _case("cfg2")


def layouts(H, W):
    return {"mono_tight": SensorSurface(H, W, "mono"),
            "rggb_pitched": SensorSurface(H, W, "rggb", pitch=768, offset=4096, image_stride=4096 + H * 768 + 333),
            "gbrg_tight": SensorSurface(H, W, "gbrg")}


@pytest.mark.parametrize("name,stem_fuse", [("mono_tight", None), ("rggb_pitched", None), ("gbrg_tight", None),
                                            ("rggb_pitched", "0")])
def test_predictor3d_sensor_bitwise(cfg2, name, stem_fuse, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)       # read when a launch plan is built
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    assert (H, W) == (512, 640)
    s = layouts(H, W)[name]
    pred = cfg2["make"]()
    x1, ref1 = sensor_frames(cfg2["bgr"], s)
    x2, ref2 = sensor_frames(cfg2["bgr2"], s, 0x5A)
    assert pred.native(H, W).graph_replay
    firsts = []
    for x, ref in ((x1, ref1), (x2, ref2)):                 # two frame sets, each called twice: the later calls
        for _ in range(2):                                  # replay the captured graph
            got = pred.forward_surface(cuda(x), s, *dev)
            torch.cuda.synchronize()
            dbg_s = _debug(pred, H, W)
            want = pred.forward_uint8(cuda(ref), *dev)
            torch.cuda.synchronize()
            dbg_b = _debug(pred, H, W)
            _assert_same(got, want, (name, "single"))
            assert want[0] is not None                      # two invalid outputs cannot pass by agreeing
            for k in dbg_b:
                assert torch.equal(dbg_s[k], dbg_b[k]), (name, k)
        firsts.append(want[0])
    assert not torch.equal(firsts[0], firsts[1])
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


@pytest.mark.parametrize("stem_fuse", [None, "0"])
def test_crop_windows_on_the_border(stem_fuse, monkeypatch):
    """cfg2_edge: the crop centres are clamped at x low, x high and y low, so crop windows hold the frame's first
    row and its first and last column, where a pixel takes the RGB of its clamped interior neighbour."""
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)
    e = _case("cfg2_edge")
    H, W, dev = e["H"], e["W"], e["dev"]
    pred = e["make"]()
    for s in (SensorSurface(H, W, "bggr", pitch=W + 2, offset=1, image_stride=1 + H * (W + 2)),
              SensorSurface(H, W, "grbg")):
        x, ref = sensor_frames(e["bgr"], s)
        got = pred.forward_surface(cuda(x), s, *dev)
        torch.cuda.synchronize()
        dbg_s = _debug(pred, H, W)
        want = pred.forward_uint8(cuda(ref), *dev)
        torch.cuda.synchronize()
        dbg_b = _debug(pred, H, W)
        _assert_same(got, want, s.pattern)
        assert want[0] is not None
        for k in dbg_b:
            assert torch.equal(dbg_s[k], dbg_b[k]), (s.pattern, k)
        chm = dbg_b["center_hm"].reshape(-1, 2).cpu()
        hw = e["c"]["bbox"] // 2
        assert int((chm[:, 0] == hw).sum()) and int((chm[:, 0] == W - hw).sum()) and int((chm[:, 1] == hw).sum())


def test_pattern_change_under_replay(cfg2):
    """One graph-replaying predictor reads the SAME bytes as rggb, then as bggr, then as rggb: every call equals the
    uint8 path on its own pattern's demosaic (a replay of the other recording would swap red and blue)."""
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    kw = dict(num_cameras=c["C"], num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN, std=S.STD, time_batch=1)
    raw = S.mosaic(cfg2["bgr"], "rggb")
    x = cuda(torch.from_numpy(raw.reshape(raw.shape[0], -1))).unsqueeze(0)
    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert g.graph_replay
    g.set_calibration(*dev)
    ref = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    ref.set_calibration(*dev)
    first = {}
    for p in ("rggb", "bggr", "rggb"):
        got = [t.clone() for t in g.forward(x.clone(), frame_layout=SensorSurface(H, W, p))]
        want = [t.clone() for t in ref.forward(cuda(torch.from_numpy(S.sensor_to_bgr(raw, p))).unsqueeze(0))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), p
        assert int(want[2][0]) == 1
        assert torch.equal(first.setdefault(p, got[0]), got[0])
    assert not torch.equal(first["rggb"], first["bggr"])
    g.close()
    ref.close()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_mask_and_views2d_behind_a_sensor_surface(cfg2):
    H, W, dev, C = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["c"]["C"]
    s = layouts(H, W)["rggb_pitched"]
    pred = cfg2["make"]()
    x, ref = sensor_frames(cfg2["bgr"], s)
    mask = [c != 1 for c in range(C)]
    x, ref = x.clone(), ref.clone()
    x[1] = 0xFF                                              # garbage in the masked slot, of both forms
    ref[1] = 0xFF
    got = pred.forward_surface(cuda(x), s, *dev, camera_mask=mask, return_2d=True)
    want = pred.forward_uint8(cuda(ref), *dev, camera_mask=mask, return_2d=True)
    clean = pred.forward_uint8(cuda(sensor_frames(cfg2["bgr"], s)[1]), *dev, camera_mask=mask)
    torch.cuda.synchronize()
    assert want[0] is not None and got[0] is not None
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    assert torch.equal(_bits(got[0]), _bits(clean[0]))       # the garbage had no effect
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
    assert int(want[2][0]) == 1


def _pred2d():
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    tags = ["cam0_j12", "cam2_j12"]
    c = cases.PREDICTOR2D_CASES[tags[0]]
    ins = [cases.predictor2d_inputs(t) for t in tags]
    cfg = make_cfg(dict(J=c["J"], bbox=c["bbox"], C=1, roi=32, spacing=2), c["center_size"])
    cfg.KEYPOINT_NAMES = ["joint%d" % i for i in range(c["J"])]
    bgr = np.concatenate([to_bgr_u8(i["img"]) for i in ins])                  # (2, H, W, 3)
    return JarvisPredictor2D(cfg, ins[0]["sd_center"], ins[0]["sd_kp"]), cfg, bgr


def test_predictor2d_sensor_bitwise():
    pred, _, bgr = _pred2d()
    H, W = bgr.shape[1:3]
    for s in (SensorSurface(H, W, "mono", pitch=W + 64, offset=32), SensorSurface(H, W, "grbg")):
        x, ref = sensor_frames(bgr, s)
        got = [t.clone() for t in pred.forward_batch(cuda(x), frame_layout=s)]
        want = [t.clone() for t in pred.forward_batch(cuda(ref))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), s.pattern
        assert int(want[2].sum()) == 2
        p1, c1 = pred.forward_surface(cuda(x[0]), s)
        p2, c2 = pred.forward(cuda(x[:1]), frame_layout=s)
        w1 = pred.forward_batch(cuda(ref[:1]))
        torch.cuda.synchronize()
        assert torch.equal(p1, w1[0][0].long()) and torch.equal(c1, w1[1][0])
        assert torch.equal(p2, p1) and torch.equal(c2, c1)


def _read(path, name):
    return open(os.path.join(path, name), newline="").read()


def test_drivers_sensor_csv_identical(cfg2, tmp_path):
    """predict3D_frames (time_batch 3, two streams) and predict2D_frames with frame_layout=SensorSurface write CSVs
    byte-identical to the BGR runs on the demosaiced frames."""
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    from jarvis_hybridnet_amd.prediction.predict2D import predict2D_frames
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    cfg = make_cfg(c, c["center_size"])
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = (inp["cam"], inp["intr"], inp["dist"])
    pred = cfg2["make"]()
    s = layouts(H, W)["rggb_pitched"]
    bgr = [to_bgr_u8(S.blob_frames(calib, W, H, c["J"], 70 + i)[0]) for i in range(5)]
    pairs = [sensor_frames(b, s) for b in bgr]
    raw = [p[0].numpy() for p in pairs]
    ref = [p[1].numpy() for p in pairs]
    kw = dict(time_batch=3, streams=2)
    assert predict3D_frames(pred, raw, *dev, cfg, str(tmp_path / "s"), frame_layout=s, **kw) == 5
    fills = [(lambda dst, a=a: np.copyto(dst, a)) for a in raw]
    assert predict3D_frames(pred, fills, *dev, cfg, str(tmp_path / "f"), frame_layout=s,
                            frame_spec=(raw[0].shape, torch.uint8), **kw) == 5
    assert predict3D_frames(pred, ref, *dev, cfg, str(tmp_path / "b"), **kw) == 5
    release_ingest_buffers(pred)
    want = _read(tmp_path / "b", "data3D.csv")
    assert _read(tmp_path / "s", "data3D.csv") == want and _read(tmp_path / "f", "data3D.csv") == want
    rows = want.splitlines()[2:]
    assert len(rows) == 5 and len(set(rows)) == 5 and all(not r.startswith("NaN") for r in rows)
    # 2D driver: camera 0 of each frame set, Mono8
    p2, cfg2d, _ = _pred2d()
    m = SensorSurface(H, W, "mono", pitch=W + 32)
    pairs = [sensor_frames(b[0], m) for b in bgr]
    assert predict2D_frames(p2, [p[0].numpy() for p in pairs], cfg2d, str(tmp_path / "2s"), time_batch=2,
                            frame_layout=m) == 5
    assert predict2D_frames(p2, [p[1].numpy() for p in pairs], cfg2d, str(tmp_path / "2b"), time_batch=2) == 5
    release_ingest_buffers(p2)
    want = _read(tmp_path / "2b", "data2D.csv")
    assert _read(tmp_path / "2s", "data2D.csv") == want
    assert all(not r.startswith("NaN") for r in want.splitlines()[2:])
