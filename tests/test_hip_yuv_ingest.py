"""GPU: YUV 4:2:0 ingest (I420 / NV12).  The contract is bitwise: a forward on YUV frames equals the uint8 BGR
forward on the frames' conversion by the numpy reference (tests/test_yuv_ingest_cpu.py: yuv420_to_bgr), in the
points, confidences, valid flags and every intermediate debug() exposes -- fused stem and stand-alone kernels,
graph replay and time batches, the 2D predictor and both drivers.  Test frames: synthetic.blob_frames, quantised
to BGR and taken to YUV by any forward BT.601 transform (synthetic.bgr_to_yuv420); only the inverse is a
contract."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.gpu_util import cuda, report
from tests.test_hip_predictor import make_cfg
from tests.test_yuv_ingest_cpu import yuv420_to_bgr

pytestmark = pytest.mark.gpu

FORMATS = ("i420", "nv12")


def to_bgr_u8(imgs):
    """(C,3,H,W) fp32 RGB -> (C,H,W,3) uint8 BGR numpy (as a decoder hands them to cv2)."""
    return (imgs.permute(0, 2, 3, 1)[..., [2, 1, 0]] * 255).round().to(torch.uint8).numpy()


def yuv_and_reference(bgr, fmt):
    """YUV frames of `bgr` and the BGR bytes the contract converts them to (torch CPU tensors)."""
    from jarvis_hybridnet_amd import synthetic as S
    yuv = S.bgr_to_yuv420(bgr, fmt)
    return torch.from_numpy(yuv), torch.from_numpy(yuv420_to_bgr(yuv, fmt))


def test_yuv420_to_bgr_op_exhaustive():
    """jh_op_yuv420_to_bgr against numpy over all 2^24 (Y, U, V) triples, both layouts: 64 frames of 512 x 512
    whose chroma planes enumerate the 65 536 (U, V) pairs and whose 2 x 2 luma blocks hold Y = 4f .. 4f+3."""
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd import synthetic as S
    F, H, W = 64, 512, 512
    cu, cv = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    U = np.broadcast_to(cu, (F, 256, 256))
    V = np.broadcast_to(cv, (F, 256, 256))
    blk = (4 * np.arange(F, dtype=np.int64))[:, None, None] + np.array([[0, 1], [2, 3]])[None]
    Y = np.tile(blk, (1, 256, 256)).astype(np.uint8)
    for fmt in FORMATS:
        yuv = S.pack_yuv420(Y, U, V, fmt)
        assert yuv.shape == (F, H * 3 // 2, W)
        x = cuda(torch.from_numpy(yuv))
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
        N.check(N.lib().jh_op_yuv420_to_bgr(N.ptr(x), N.FRAME_FORMATS[fmt], F, H, W, N.ptr(out), N.stream()))
        got = out.cpu().numpy()
        seen = np.zeros(1 << 24, dtype=bool)
        for f0 in range(0, F, 8):
            assert np.array_equal(got[f0:f0 + 8], yuv420_to_bgr(yuv[f0:f0 + 8], fmt)), (fmt, f0)
            yy = Y[f0:f0 + 8].astype(np.int64)
            uu = np.repeat(np.repeat(U[f0:f0 + 8].astype(np.int64), 2, 1), 2, 2)
            vv = np.repeat(np.repeat(V[f0:f0 + 8].astype(np.int64), 2, 1), 2, 2)
            seen[(yy << 16) | (uu << 8) | vv] = True
        assert seen.all()                       # every (Y, U, V) triple was converted
    with pytest.raises(RuntimeError, match="even"):
        N.check(N.lib().jh_op_yuv420_to_bgr(N.ptr(x), N.FRAME_FORMATS["i420"], 1, 3, 4, N.ptr(out), N.stream()))


def _assert_same(a, b, what):
    assert (a[0] is None) == (b[0] is None), what
    for x, y in zip(a, b):
        if x is not None:
            assert torch.equal(x, y), what


def _debug(pred, H, W):
    return {k: v.clone() for k, v in pred.native(H, W).debug("cuda").items()}


CASES3D = [("cfg2", None, None), ("cfg3", None, None), ("cfg3_medium", None, None), ("cfg2_edge", None, None),
           ("cfg2_none", None, None), ("cfg3", "0", None), ("cfg2", None, "bf16x3")]


@pytest.mark.parametrize("tag,stem_fuse,precision", CASES3D,
                         ids=["cfg2", "cfg3", "cfg3_medium", "cfg2_edge", "cfg2_none", "cfg3_unfused", "cfg2_bf16x3"])
def test_predictor3d_yuv_bitwise(tag, stem_fuse, precision, monkeypatch):
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)       # read when a launch plan is built (nets.hip)
    c = cases.PREDICTOR_CASES[tag]
    inp = cases.predictor_inputs(tag)
    H, W = c["H"], c["W"]
    bgr = to_bgr_u8(inp["imgs"])
    # a second, different frame set for the time batch: the same scene shifted
    bgr2 = np.ascontiguousarray(np.roll(bgr, (24, -40), axis=(1, 2)))
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]
    pred = JarvisPredictor3D(make_cfg(c, c["center_size"]), inp["sd_center"], inp["sd_hybrid"], precision=precision)
    for fmt in FORMATS:
        yuv, ref = yuv_and_reference(bgr, fmt)
        yuv2, ref2 = yuv_and_reference(bgr2, fmt)
        # single frame set: the T = 1 predictor replays one captured graph per format
        assert pred.native(H, W).graph_replay
        for _ in range(2):
            got = pred.forward_yuv(cuda(yuv), fmt, *dev)
            torch.cuda.synchronize()
            dbg_y = _debug(pred, H, W)
            want = pred.forward_uint8(cuda(ref), *dev)
            torch.cuda.synchronize()
            dbg_b = _debug(pred, H, W)
            _assert_same(got, want, (tag, fmt, "single"))
            for k in dbg_b:
                assert torch.equal(dbg_y[k], dbg_b[k]), (tag, fmt, k)
        if c.get("expect_none"):
            assert want[0] is None
        else:
            assert want[0] is not None                     # two invalid outputs cannot pass by agreeing
        # time batch T = 4 of distinct frame sets
        x = cuda(torch.stack([yuv, yuv2, yuv2, yuv]))
        xb = cuda(torch.stack([ref, ref2, ref2, ref]))
        got = [t.clone() for t in pred.forward_batch(x, *dev, frame_format=fmt)]
        torch.cuda.synchronize()
        dbg_y = {k: v.clone() for k, v in pred.native(H, W, time_batch=4).debug("cuda").items()}
        want = [t.clone() for t in pred.forward_batch(xb, *dev)]
        torch.cuda.synchronize()
        dbg_b = {k: v.clone() for k, v in pred.native(H, W, time_batch=4).debug("cuda").items()}
        for a, b in zip(got, want):
            assert torch.equal(a, b), (tag, fmt, "batch")
        for k in dbg_b:
            assert torch.equal(dbg_y[k], dbg_b[k]), (tag, fmt, "batch", k)
        nv = int(want[2].sum())
        assert nv == 0 if c.get("expect_none") else int(want[2][0]) == 1 and int(want[2][3]) == 1
        # which path ran: only the stand-alone kernels are launched (and profiled) as preprocess_resize / _crop
        from jarvis_hybridnet_amd import _native as N
        xs = cuda(yuv).unsqueeze(0)
        names = {r[0] for r in N.profile(lambda: pred.native(H, W).forward(xs, frame_format=fmt))}
        pre = names & {"preprocess_resize", "preprocess_crop"}
        if stem_fuse == "0":
            assert pre == {"preprocess_resize", "preprocess_crop"}, "JH_STEM_FUSE=0 had no effect"
        else:
            assert not pre and any(n.startswith("stem_conv") for n in names), names
        report("yuv_ingest_3d", tag=tag, fmt=fmt, stem_fuse=stem_fuse or "1", precision=precision or "f32",
               valid=nv)


def test_graph_slot_per_format():
    """One graph-replaying predictor called BGR -> I420 -> NV12 -> BGR: every call replays the graph of its own
    format and equals a fresh predictor's result for that format."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    kw = dict(num_cameras=c["C"], num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"],
              mean=S.MEAN, std=S.STD, time_batch=1)
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]
    bgr = to_bgr_u8(inp["imgs"])
    frames = {"bgr": (cuda(torch.from_numpy(bgr)), None)}
    for fmt in FORMATS:
        # (a call that replayed another format's graph would read these bytes in the wrong layout)
        frames[fmt] = (cuda(yuv_and_reference(bgr, fmt)[0]), fmt)
    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert g.graph_replay
    g.set_calibration(*dev)
    outs = {}
    for name in ("bgr", "i420", "nv12", "bgr"):
        x, fmt = frames[name]
        got = [t.clone() for t in g.forward(x.unsqueeze(0).clone(), frame_format=fmt)]
        fresh = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
        fresh.set_calibration(*dev)
        want = [t.clone() for t in fresh.forward(x.unsqueeze(0), frame_format=fmt)]
        torch.cuda.synchronize()
        fresh.close()
        for a, b in zip(got, want):
            assert torch.equal(a, b), name
        assert int(got[2][0]) == 1
        outs.setdefault(name, got[0])
        assert torch.equal(outs[name], got[0])
    # a wrong shape never crosses the ABI
    with pytest.raises(RuntimeError, match="frame_format"):
        g.forward(frames["bgr"][0].unsqueeze(0)[..., 0].contiguous())


def test_predictor2d_yuv_bitwise():
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    tags = ["cam0_j12", "cam2_j12"]
    c = cases.PREDICTOR2D_CASES[tags[0]]
    ins = [cases.predictor2d_inputs(t) for t in tags]
    cfg = make_cfg(dict(J=c["J"], bbox=c["bbox"], C=1, roi=32, spacing=2), c["center_size"])
    pred = JarvisPredictor2D(cfg, ins[0]["sd_center"], ins[0]["sd_kp"])
    bgr = np.concatenate([to_bgr_u8(i["img"]) for i in ins])                  # (2, H, W, 3)
    for fmt in FORMATS:
        yuv, ref = yuv_and_reference(bgr, fmt)
        got = [t.clone() for t in pred.forward_batch(cuda(yuv), frame_format=fmt)]
        want = [t.clone() for t in pred.forward_batch(cuda(ref))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), fmt
        assert int(want[2].sum()) == 2
        p1, c1 = pred.forward_yuv(cuda(yuv[0]), fmt)
        w1 = pred.forward_batch(cuda(ref[:1]))
        torch.cuda.synchronize()
        assert torch.equal(p1, w1[0][0].long()) and torch.equal(c1, w1[1][0])


def _csv(path, name):
    return open(os.path.join(path, name), newline="").read()


def test_drivers_yuv_csv_identical(tmp_path):
    """predict3D_frames / predict2D_frames on YUV frames (arrays and fill callables with frame_spec) write files
    byte-identical to the BGR runs on the converted frames."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    from jarvis_hybridnet_amd.prediction.predict2D import predict2D_frames
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    cfg = make_cfg(c, c["center_size"])
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = (inp["cam"], inp["intr"], inp["dist"])
    dev = [cuda(t) for t in calib]
    pred = JarvisPredictor3D(cfg, inp["sd_center"], inp["sd_hybrid"])
    bgr = [to_bgr_u8(S.blob_frames(calib, c["W"], c["H"], c["J"], 70 + i)[0]) for i in range(10)]
    for fmt in FORMATS:
        pairs = [yuv_and_reference(b, fmt) for b in bgr]
        yuv = [p[0].numpy() for p in pairs]
        ref = [p[1].numpy() for p in pairs]
        kw = dict(time_batch=4, streams=2)
        ny = predict3D_frames(pred, yuv, *dev, cfg, str(tmp_path / (fmt + "_y")), frame_format=fmt, **kw)
        nb = predict3D_frames(pred, ref, *dev, cfg, str(tmp_path / (fmt + "_b")), **kw)
        fills = [(lambda dst, a=a: np.copyto(dst, a)) for a in yuv]
        nf = predict3D_frames(pred, fills, *dev, cfg, str(tmp_path / (fmt + "_f")), frame_format=fmt,
                              frame_spec=(yuv[0].shape, torch.uint8), **kw)
        assert ny == nb == nf == 10
        want = _csv(tmp_path / (fmt + "_b"), "data3D.csv")
        assert _csv(tmp_path / (fmt + "_y"), "data3D.csv") == want
        assert _csv(tmp_path / (fmt + "_f"), "data3D.csv") == want
        rows = list(csv.reader(open(tmp_path / (fmt + "_b") / "data3D.csv")))[2:]
        assert len(rows) == 10 and len({tuple(r) for r in rows}) == 10 and all(r[0] != "NaN" for r in rows)
    release_ingest_buffers(pred)
    # 2D driver: one camera of each frame set
    c2 = cases.PREDICTOR2D_CASES["cam0_j12"]
    i2 = cases.predictor2d_inputs("cam0_j12")
    cfg2 = make_cfg(dict(J=c2["J"], bbox=c2["bbox"], C=1, roi=32, spacing=2), c2["center_size"])
    cfg2.KEYPOINT_NAMES = ["joint%d" % i for i in range(c2["J"])]
    p2 = JarvisPredictor2D(cfg2, i2["sd_center"], i2["sd_kp"])
    for fmt in FORMATS:
        pairs = [yuv_and_reference(b[:1], fmt) for b in bgr[:7]]
        yuv = [p[0][0].numpy() for p in pairs]
        ref = [p[1][0].numpy() for p in pairs]
        ny = predict2D_frames(p2, yuv, cfg2, str(tmp_path / ("2d" + fmt + "_y")), time_batch=3, frame_format=fmt)
        nb = predict2D_frames(p2, ref, cfg2, str(tmp_path / ("2d" + fmt + "_b")), time_batch=3)
        fills = [(lambda dst, a=a: np.copyto(dst, a)) for a in yuv]
        nf = predict2D_frames(p2, fills, cfg2, str(tmp_path / ("2d" + fmt + "_f")), time_batch=3, frame_format=fmt,
                              frame_spec=(yuv[0].shape, torch.uint8))
        assert ny == nb == nf == 7
        want = _csv(tmp_path / ("2d" + fmt + "_b"), "data2D.csv")
        assert _csv(tmp_path / ("2d" + fmt + "_y"), "data2D.csv") == want
        assert _csv(tmp_path / ("2d" + fmt + "_f"), "data2D.csv") == want
    release_ingest_buffers(p2)
