"""GPU: per-camera tone tables (jh_predictor_set_tone).  The contract is bitwise: a call under tables equals the fp32
path on the frames F[c][ch] = tables[c][ch][bytes], the bytes being what the form's to-BGR conversion gives (the numpy
references of the existing tests) -- the stand-alone operator over every source form with poisoned padding, the 3D
predictor (fused and stand-alone stems, graph replay, new table values under one recording, tables off again), identity
and uint8-LUT tables against the uint8 path, crop windows on the frame's border, time batches, per-image pointers,
masks, centres and 2D views, a camera-sharded predictor, the 2D predictor, detect_subjects, the driver and the refusal
of fp32 frames.  The tables are tests/tone_cases.py's: tests/test_tone_cpu.py checks that the reference is valid on the
frames they define.  Every test calls a symbol or argument that does not exist without the feature."""
import os

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import PixelSurface, SensorSurface, ToneTables, YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases, tone_cases
from tests.gpu_util import cuda
from tests.test_hip_pixel_surface import native_kw, pixel_frames, slices
from tests.test_hip_predictor import make_cfg
from tests.test_hip_sample_depth import sensor_layouts, wide_frames, yuv_layouts, yuv_reference
from tests.test_hip_sensor_surface import PATTERNS, pitched, sensor_frames
from tests.test_hip_yuv_ingest import _assert_same, _debug, to_bgr_u8, yuv_and_reference
from tests.test_hip_yuv_surface import padded
from tests.test_pixel_surface_cpu import random_content
from tests.test_yuv_ingest_cpu import yuv420_to_bgr
from tests.test_yuv_surface_cpu import surface_to_bgr

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def frames_to_rgb(x, n, H, W, how, tone=None):
    """jh_op_frames_to_rgb_f32 on n device images -> (n,3,H,W) fp32 device tensor.  how: a format name ('bgr', 'i420',
    'nv12') or a YuvSurface / SensorSurface / PixelSurface; tone: a ToneTables (image i reads camera i % cameras)."""
    from jarvis_hybridnet_amd import _native as N
    yuv = how.struct() if isinstance(how, YuvSurface) else None
    sensor = how.struct() if isinstance(how, SensorSurface) else None
    pixels = how.struct() if isinstance(how, PixelSurface) else None
    fmt = N.FRAME_FORMATS[how] if isinstance(how, str) else \
        N.FRAME_SURFACE if yuv is not None else N.FRAME_SENSOR if sensor is not None else N.FRAME_PIXELS
    tab = None if tone is None else cuda(torch.tensor(tone.tables))
    out = torch.empty((n, 3, H, W), device="cuda")
    N.check(N.lib().jh_op_frames_to_rgb_f32(N.ptr(x), fmt, yuv, sensor, pixels, n, H, W, N.ptr(tab),
                                            0 if tone is None else tone.cameras, N.ptr(out), N.stream()))
    return out


# ---- 1: the operator -------------------------------------------------------------------------------------------------
def op_forms(H, W, g):
    """name -> (description, [(packed frames (3, bytes) numpy, fill), ...], the BGR bytes (3,H,W,3) of the references)
    for every source form at H x W (even); the pixel surfaces at the odd size (H-1) x (W-1)."""
    forms = {}
    bgr = g.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    forms["bgr"] = ("bgr", [(bgr.reshape(3, -1), None)], bgr)
    y = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    u, v = g.integers(0, 256, (2, 3, H // 2, W // 2), dtype=np.uint8)
    for fmt in ("i420", "nv12"):
        yuv = S.pack_yuv420(y, u, v, fmt)
        forms[fmt] = (fmt, [(yuv.reshape(3, -1), None)], yuv420_to_bgr(yuv, fmt))
    ys = padded(H, W, "nv21", matrix="bt709", range="full")
    forms["yuv_surface"] = (ys, [(S.pack_yuv_surface(y, u, v, ys, f), f) for f in (0xA5, 0x5A)],
                            surface_to_bgr(S.pack_yuv_surface(y, u, v, ys, 0), ys))
    p010 = yuv_layouts(H, W, "nv12", bits=10, msb=True)[1]
    wide = [S.widen(p, p010.shift, g, saturate=True) for p in (y, u, v)]
    forms["p010"] = (p010, [(S.pack_yuv_surface(*wide, p010, f), f) for f in (0xA5, 0x5A)],
                     yuv_reference(y, u, v, p010))
    raw = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    for p in PATTERNS:
        s = pitched(H, W, p)
        forms[p] = (s, [(S.pack_sensor_surface(raw, s, f), f) for f in (0xA5, 0x5A)], S.sensor_to_bgr(raw, p))
    m12 = sensor_layouts(H, W, "mono", 12, "packed")[1]
    w12 = S.widen(raw, m12.shift, g)
    forms["mono12p"] = (m12, [(S.pack_sensor_surface(w12, m12, f), f) for f in (0xA5, 0x5A)],
                        S.sensor_to_bgr(raw, "mono"))
    h, w = H - 1, W - 1
    P = PixelSurface
    for name, s in (("rgb24", P.packed(h, w, "rgb")),
                    ("bgra", P.packed(h, w, "bgra", pitch=4 * w + 6, offset=5, image_stride=5 + h * (4 * w + 6) + 9)),
                    ("yuyv422", P.yuv_packed(h, w, "yuyv", pitch=2 * (w + 1) + 6)),
                    ("yuv444p", P.yuv_planar(h, w, "444"))):
        content = random_content(g, s)
        forms[name] = (s, [(S.pack_pixel_surface(content, s, f), f) for f in (0xA5, 0x5A)],
                       S.pixels_to_bgr(S.pack_pixel_surface(content, s, 0), s))
    return forms


@pytest.mark.parametrize("H,W", [(4, 4), (6, 10), (34, 66)])
def test_frames_to_rgb_f32_op(H, W):
    g = np.random.default_rng(H * 1000 + W)
    # a different random table per camera and channel: any (camera, channel, byte) mix-up changes a value
    tone = ToneTables(g.random((3, 3, 256), dtype=np.float32) * 4 - 2)
    forms = op_forms(H, W, g)
    assert len(forms) == 15
    k255 = np.float32(1) / np.float32(255)
    for name, (how, packed, want_bgr) in forms.items():
        h, w = want_bgr.shape[1:3]
        want = tone_cases.mapped_rgb(want_bgr, tone)                     # image i: camera i % 3 = i
        plain = np.ascontiguousarray(want_bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) * k255
        for buf, fill in packed:
            x = cuda(torch.from_numpy(np.ascontiguousarray(buf)))
            got = frames_to_rgb(x, 3, h, w, how, tone).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, fill, "tables")
            got = frames_to_rgb(x, 3, h, w, how).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), (name, fill, "NULL tables")
    # image i reads camera i % cams: two cameras' tables over three images
    two = ToneTables(tone.tables[:2])
    how, packed, want_bgr = forms["bgr"]
    got = frames_to_rgb(cuda(torch.from_numpy(packed[0][0])), 3, H, W, how, two).cpu().numpy()
    want = tone_cases.mapped_rgb(want_bgr, ToneTables(tone.tables[[0, 1, 0]]))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_frames_to_rgb_f32_op_validation():
    from jarvis_hybridnet_amd import _native as N
    x = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, device="cuda")
    fn = N.lib().jh_op_frames_to_rgb_f32
    bgr, s = N.FRAME_FORMATS["bgr"], SensorSurface(4, 4).struct()
    for args, msg in (((N.ptr(x), 0, None, None, None, 1, 4, 4, None, 0), "byte frames"),       # fp32 frames
                      ((N.ptr(x), bgr, None, s, None, 1, 4, 4, None, 0), "jh_sensor_surface"),  # a stray description
                      ((N.ptr(x), N.FRAME_SENSOR, None, None, None, 1, 4, 4, None, 0), "jh_sensor_surface"),
                      ((N.ptr(x), N.FRAME_FORMATS["nv12"], None, None, None, 1, 3, 4, None, 0), "even"),
                      ((N.ptr(x), bgr, None, None, None, 1, 4, 4, N.ptr(out), 0), "camera count"),
                      ((None, bgr, None, None, None, 1, 4, 4, None, 0), "null")):
        with pytest.raises(RuntimeError, match=msg):
            N.check(fn(*args, N.ptr(out), N.stream()))


# ---- the predictors --------------------------------------------------------------------------------------------------
def _case(tag):
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c = cases.PREDICTOR_CASES[tag]
    inp = cases.predictor_inputs(tag)
    bgr = to_bgr_u8(inp["imgs"])
    bgr2 = np.ascontiguousarray(np.roll(bgr, (24, -40), axis=(1, 2)))
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]

    def make():
        return JarvisPredictor3D(make_cfg(c, c["center_size"]), inp["sd_center"], inp["sd_hybrid"])
    return dict(c=c, inp=inp, bgr=bgr, bgr2=bgr2, dev=dev, make=make, H=c["H"], W=c["W"], ref=make(),
                tone=tone_cases.tables(), tone2=tone_cases.other_tables())


@pytest.fixture(scope="module")
def cfg2():
    """cfg2 with `ref`, a predictor that is never given tables: the fp32 side of every comparison."""
    return _case("cfg2")


def form_frames(name, bgr, H, W, fill=0xA5, seed=0):
    """-> (how forward_X is called: (method name, args behind the frames), frames, the BGR bytes of the reference,
    the description for the operator)."""
    if name == "bgr":
        return ("forward_uint8", ()), torch.from_numpy(bgr), torch.from_numpy(bgr), "bgr"
    if name == "nv12":
        x, ref = yuv_and_reference(bgr, "nv12")
        return ("forward_yuv", ("nv12",)), x, ref, "nv12"
    if name == "rggb_pitched":
        s = SensorSurface(H, W, "rggb", pitch=768, offset=4096, image_stride=4096 + H * 768 + 333)
        x, ref = sensor_frames(bgr, s, fill)
    elif name == "mono12p":
        s = SensorSurface(H, W, "mono", bits=12, container="packed")
        x, ref = wide_frames(bgr, s, fill, seed)
    else:
        assert name == "yuyv422"
        s = PixelSurface.yuv_packed(H, W, "yuyv", pitch=2 * W + 64)
        x, ref = pixel_frames(bgr, s, fill)
    return ("forward_surface", (s,)), x, ref, s


def fp32_frames(x, how, ref_bgr, tone, H, W):
    """The fp32 frames a call under `tone` is defined by, built by the operator from the frames themselves (item 1
    checks it over every form) and checked against the numpy definition on the reference bytes."""
    C = ref_bgr.shape[0]
    f = frames_to_rgb(cuda(x).reshape(C, -1), C, H, W, how, tone)
    want = tone_cases.mapped_rgb(ref_bgr.numpy(), tone)
    assert np.array_equal(f.cpu().numpy().view(np.uint32), want.view(np.uint32))
    return f


@pytest.mark.parametrize("name,stem_fuse", [("bgr", None), ("nv12", None), ("rggb_pitched", None), ("mono12p", None),
                                            ("yuyv422", None), ("rggb_pitched", "0")])
def test_predictor3d_tone_bitwise(cfg2, name, stem_fuse, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)       # read when a launch plan is built
    H, W, dev, ref_pred, tone, tone2 = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["ref"], cfg2["tone"], cfg2["tone2"]
    assert (H, W) == (512, 640)
    pred = cfg2["make"]()
    pred.set_tone(tone)
    nat = pred.native(H, W)
    assert nat.graph_replay and nat.graph_records == 0
    bytes_before = nat.device_bytes
    (method, args), x1, ref1, how = form_frames(name, cfg2["bgr"], H, W)
    _, x2, ref2, _ = form_frames(name, cfg2["bgr2"], H, W, 0x5A, 1)
    call = getattr(pred, method)
    firsts = []
    for x, ref in ((x1, ref1), (x2, ref2)):                 # two frame sets, each called twice: the later calls
        f = fp32_frames(x, how, ref, tone, H, W)            # replay the captured graph
        want = ref_pred.forward(f, *dev)
        torch.cuda.synchronize()
        dbg_f = _debug(ref_pred, H, W)
        assert want[0] is not None                          # two invalid outputs cannot pass by agreeing
        for _ in range(2):
            got = call(cuda(x), *args, *dev)
            torch.cuda.synchronize()
            dbg_t = _debug(pred, H, W)
            _assert_same(got, want, (name, "tables"))
            for k in dbg_f:
                assert torch.equal(dbg_t[k], dbg_f[k]), (name, k)
        firsts.append(want[0])
    assert not torch.equal(firsts[0], firsts[1])
    assert nat.graph_records == 1                           # one recording, three replays
    # the tables matter: the same frames without them give another result
    plain = getattr(ref_pred, method)(cuda(x2), *args, *dev)
    torch.cuda.synchronize()
    assert plain[0] is not None and not torch.equal(plain[0], firsts[1])
    # new table VALUES under the same recording: the result follows, and the call was a replay
    pred.set_tone(tone2)
    got = call(cuda(x2), *args, *dev)
    want = ref_pred.forward(fp32_frames(x2, how, ref2, tone2, H, W), *dev)
    torch.cuda.synchronize()
    _assert_same(got, want, (name, "second tables"))
    assert want[0] is not None and not torch.equal(want[0], firsts[1])
    assert nat.graph_records == 1
    assert pred.native(H, W) is nat and nat.device_bytes == bytes_before      # (allocated by the first set_tone)
    # which path ran: only the stand-alone kernels are launched (and profiled) as preprocess_resize / _crop
    names = {r[0] for r in N.profile(lambda: call(cuda(x2), *args, *dev))}
    pre = names & {"preprocess_resize", "preprocess_crop"}
    if stem_fuse == "0":
        assert pre == {"preprocess_resize", "preprocess_crop"}, "JH_STEM_FUSE=0 had no effect"
    else:
        assert not pre and any(n.startswith("stem_conv") for n in names), names
    # tables off again: the bits of the plain call (another recording: the tone form is part of the description)
    pred.set_tone(None)
    for _ in range(2):
        got = call(cuda(x2), *args, *dev)
        torch.cuda.synchronize()
        _assert_same(got, plain, (name, "off"))
    assert nat.graph_records == 2


def test_device_bytes_grow_with_the_first_set_tone(cfg2):
    H, W = cfg2["H"], cfg2["W"]
    pred = cfg2["make"]()
    nat = pred.native(H, W)
    before = nat.device_bytes
    nat.set_tone(cfg2["tone"])
    assert nat.device_bytes == before + 4 * 3 * 256 * 4
    nat.set_tone(cfg2["tone2"])
    nat.set_tone(None)
    assert nat.device_bytes == before + 4 * 3 * 256 * 4
    with pytest.raises(ValueError, match="cameras"):
        nat.set_tone(ToneTables.identity(3))


# ---- 3: identity and uint8 LUTs --------------------------------------------------------------------------------------
def test_identity_and_from_bytes_are_the_uint8_path(cfg2):
    H, W, dev, ref_pred = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["ref"]
    bgr, bgr2 = cfg2["bgr"], cfg2["bgr2"]
    g = np.random.default_rng(5)
    # per camera and channel a monotone LUT near the identity: k -> clip(k + d(k)), d a small smooth offset
    k = np.arange(256)
    lut = np.empty((4, 3, 256), np.uint8)
    for c in range(4):
        for ch in range(3):
            a, b = g.uniform(0.9, 1.1), g.integers(-6, 7)
            lut[c, ch] = np.clip(np.rint(a * k + b), 0, 255)
    mapped = [np.stack([np.stack([lut[c, 2 - j][b[c, ..., j]] for j in range(3)], -1) for c in range(4)])
              for b in (bgr, bgr2)]                                            # BGR order: channel j is table 2 - j
    assert not np.array_equal(mapped[0], bgr)
    pred = cfg2["make"]()
    for tone, frames in ((ToneTables.identity(4), (bgr, bgr2)), (ToneTables.from_bytes(lut), mapped)):
        pred.set_tone(tone)
        got = pred.forward_uint8(cuda(torch.from_numpy(bgr)), *dev)
        want = ref_pred.forward_uint8(cuda(torch.from_numpy(frames[0])), *dev)
        torch.cuda.synchronize()
        _assert_same(got, want, "T=1")
        assert want[0] is not None
        for k_, v in _debug(ref_pred, H, W).items():
            assert torch.equal(_debug(pred, H, W)[k_], v), k_
        x = cuda(torch.from_numpy(np.stack([bgr, bgr2, bgr2, bgr])))
        xr = cuda(torch.from_numpy(np.stack([frames[0], frames[1], frames[1], frames[0]])))
        got = [t.clone() for t in pred.forward_batch(x, *dev)]
        want = [t.clone() for t in ref_pred.forward_batch(xr, *dev)]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), "T=4"
        assert int(want[2].sum()) == 4 and not torch.equal(want[0][0], want[0][1])


# ---- 4: crop windows on the border -----------------------------------------------------------------------------------
@pytest.mark.parametrize("stem_fuse", [None, "0"])
def test_crop_windows_on_the_border(stem_fuse, monkeypatch):
    """cfg2_edge: the crop centres are clamped at x low, x high and y low, so crop windows hold the frame's first row
    and its first and last column, where a Bayer pixel takes the RGB of its clamped interior neighbour."""
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)
    e = _case("cfg2_edge")
    H, W, dev, tone = e["H"], e["W"], e["dev"], e["tone"]
    pred = e["make"]()
    pred.set_tone(tone)
    s = SensorSurface(H, W, "bggr", pitch=W + 6, offset=9, image_stride=9 + H * (W + 6) + 10)
    x, ref = sensor_frames(e["bgr"], s)
    want = e["ref"].forward(fp32_frames(x, s, ref, tone, H, W), *dev)
    torch.cuda.synchronize()
    dbg_f = _debug(e["ref"], H, W)
    got = pred.forward_surface(cuda(x), s, *dev)
    torch.cuda.synchronize()
    dbg_t = _debug(pred, H, W)
    _assert_same(got, want, "bggr")
    assert want[0] is not None
    for k in dbg_f:
        assert torch.equal(dbg_t[k], dbg_f[k]), k
    chm = dbg_f["center_hm"].reshape(-1, 2).cpu()
    hw = e["c"]["bbox"] // 2
    assert int((chm[:, 0] == hw).sum()) and int((chm[:, 0] == W - hw).sum()) and int((chm[:, 1] == hw).sum())


# ---- 5: composition --------------------------------------------------------------------------------------------------
def test_composition(cfg2):
    """forward_batch at T = 4, per-image pointers, a camera mask whose masked slot holds 0xFF bytes, centres and the 2D
    views: each call under tables equals the same call on the fp32 frames."""
    H, W, dev, ref_pred, tone = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["ref"], cfg2["tone"]
    C = cfg2["c"]["C"]
    pred = cfg2["make"]()
    pred.set_tone(tone)
    b1, b2 = cfg2["bgr"], cfg2["bgr2"].copy()
    b2[1] = 0xFF                                             # the slot of the camera the mask leaves out
    xb = np.stack([b1, b2, b2, b1])
    f = cuda(torch.from_numpy(tone_cases.mapped_rgb(xb, tone)))
    x = cuda(torch.from_numpy(xb))
    mask = [[True] * C, [c != 1 for c in range(C)], [c != 1 for c in range(C)], [True] * C]
    # plain batch, then mask + 2D views
    for kw in ({}, dict(camera_mask=mask, return_2d=True)):
        got = pred.forward_batch(x, *dev, **kw)
        want = ref_pred.forward_batch(f, *dev, **kw)
        torch.cuda.synchronize()
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(_bits(a), _bits(b)), kw
        assert int(want[2].sum()) == 4 and not torch.equal(want[0][0], want[0][1])
        if kw:
            for name in want[3]._fields:                     # NaNs compared bitwise
                assert torch.equal(_bits(getattr(got[3], name)), _bits(getattr(want[3], name))), name
            assert int(want[3].used[1, 1]) == 0 and int(want[3].used.sum()) == 4 * C - 2
    # centres of the detected run put back in: stage 1 does not run, the crops still go through the tables
    centres = ref_pred.native(H, W, time_batch=4).debug("cuda")["center3d"].clone()
    got = pred.forward_batch(x, *dev, centers=centres, return_2d=True)
    want = ref_pred.forward_batch(f, *dev, centers=centres, return_2d=True)
    torch.cuda.synchronize()
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(_bits(a), _bits(b)), "centres"
    for name in want[3]._fields:
        assert torch.equal(_bits(getattr(got[3], name)), _bits(getattr(want[3], name))), name
    assert int(want[2].sum()) == 4
    # per-image pointers at odd and 4-aligned addresses, two frame sets; the fp32 side from its own per-image list
    imgs = [slices(torch.from_numpy(b).reshape(C, -1), i) for i, b in enumerate((b1, b2))]
    imgs = [[v.view(H, W, 3) for v in row] for row in imgs]
    got = pred.forward_images(imgs, *dev, camera_mask=mask[:2])
    want = ref_pred.forward_images([[f[t, c] for c in range(C)] for t in range(2)], *dev, camera_mask=mask[:2])
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b)), "images"
    assert int(want[2].sum()) == 2


# ---- 6: a camera-sharded predictor -----------------------------------------------------------------------------------
def test_sharded_predictor_reads_its_own_cameras_tables(cfg2):
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, dev, tone = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["tone"]
    kw = native_kw(c)
    x = cuda(torch.from_numpy(cfg2["bgr"])).unsqueeze(0)                       # (1,4,H,W,3)
    dets = {}
    for name, shard in (("full", {}), ("shard", dict(cam_lo=2, cam_n=2))):
        p = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw, **shard)
        p.set_calibration(*dev)
        p.set_tone(tone)                                                       # all four cameras' tables, both times
        n = shard.get("cam_n", 4)
        lo = shard.get("cam_lo", 0)
        det = torch.empty((1, n, 3), device="cuda")
        p.stage_center(x[:, lo:lo + n].contiguous(), det)
        torch.cuda.synchronize()
        dets[name] = det.cpu()
        p.close()
    assert torch.equal(dets["shard"], dets["full"][:, 2:4])
    # ... and the full predictor's are those of the fp32 frames
    p = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    p.set_calibration(*dev)
    det = torch.empty((1, 4, 3), device="cuda")
    p.stage_center(cuda(torch.from_numpy(tone_cases.mapped_rgb(cfg2["bgr"], tone))).unsqueeze(0), det)
    torch.cuda.synchronize()
    assert torch.equal(det.cpu(), dets["full"])
    # cameras 2, 3 under cameras 0, 1's tables would detect something else
    q = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    q.set_calibration(*dev)
    q.stage_center(cuda(torch.from_numpy(tone_cases.mapped_rgb(
        cfg2["bgr"], ToneTables(tone.tables[[0, 1, 0, 1]])))).unsqueeze(0), det)
    torch.cuda.synchronize()
    assert not torch.equal(det.cpu()[:, 2:4], dets["shard"])
    p.close()
    q.close()


# ---- 7: the 2D predictor and detect_subjects -------------------------------------------------------------------------
def test_predictor2d_tone_bitwise():
    from tests.test_hip_pixel_surface import _pred2d
    pred, _, bgr = _pred2d()
    ref_pred, _, _ = _pred2d()
    tone = ToneTables(tone_cases.tables().tables[1:2])                         # one camera's table
    pred.set_tone(tone)
    f = tone_cases.mapped_rgb(bgr[:, None], tone)[:, 0]                        # every image: camera 0 of the table
    got = [t.clone() for t in pred.forward_batch(cuda(torch.from_numpy(bgr)))]
    want = [t.clone() for t in ref_pred.forward_batch(cuda(torch.from_numpy(f)))]
    plain = [t.clone() for t in ref_pred.forward_batch(cuda(torch.from_numpy(bgr)))]
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert int(want[2].sum()) == 2 and not torch.equal(plain[1], want[1])
    with pytest.raises(RuntimeError, match="tone tables"):
        pred.forward_batch(cuda(torch.from_numpy(f)))
    pred.set_tone(None)
    got = pred.forward_batch(cuda(torch.from_numpy(bgr)))
    torch.cuda.synchronize()
    for a, b in zip(got, plain):
        assert torch.equal(a, b)


def test_detect_subjects_under_tables(cfg2):
    from tests.test_hip_subjects import same_subjects
    dev, ref_pred, tone = cfg2["dev"], cfg2["ref"], cfg2["tone"]
    pred = cfg2["make"]()
    pred.set_tone(tone)
    xb = np.stack([cfg2["bgr"], cfg2["bgr2"]])
    got, gp = pred.detect_subjects(cuda(torch.from_numpy(xb)), *dev, 2, return_peaks=True)
    want, wp = ref_pred.detect_subjects(cuda(torch.from_numpy(tone_cases.mapped_rgb(xb, tone))), *dev, 2,
                                        return_peaks=True)
    torch.cuda.synchronize()
    assert same_subjects(got, want) and torch.equal(_bits(gp), _bits(wp))
    assert int(want.views[:, 0].min()) >= 2                  # a subject was found in both frame sets


# ---- 8: the driver ---------------------------------------------------------------------------------------------------
def test_driver_tone_csv_identical(cfg2, tmp_path):
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, dev, H, W, tone = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"], cfg2["tone"]
    cfg = make_cfg(c, c["center_size"])
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = (inp["cam"], inp["intr"], inp["dist"])
    pred = cfg2["make"]()
    bgr = [to_bgr_u8(S.blob_frames(calib, W, H, c["J"], 70 + i)[0]) for i in range(6)]
    f32 = [tone_cases.mapped_rgb(b, tone) for b in bgr]
    kw = dict(time_batch=4, streams=3)
    assert predict3D_frames(pred, bgr, *dev, cfg, str(tmp_path / "t"), tone=tone, **kw) == 6
    release_ingest_buffers(pred)
    assert predict3D_frames(cfg2["ref"], f32, *dev, cfg, str(tmp_path / "f"), **kw) == 6
    assert predict3D_frames(cfg2["ref"], bgr, *dev, cfg, str(tmp_path / "p"), **kw) == 6
    release_ingest_buffers(cfg2["ref"])
    read = lambda d: open(os.path.join(str(tmp_path / d), "data3D.csv"), newline="").read()  # noqa: E731
    want = read("f")
    assert read("t") == want and read("p") != want
    rows = want.splitlines()[2:]
    assert len(rows) == 6 and len(set(rows)) == 6 and all(not r.startswith("NaN") for r in rows)


# ---- 9: refusal ------------------------------------------------------------------------------------------------------
def test_fp32_frames_are_refused_under_tables(cfg2):
    H, W, dev, tone = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["tone"]
    pred = cfg2["make"]()
    x = cuda(torch.from_numpy(cfg2["bgr"]))
    f = cuda(cfg2["inp"]["imgs"])
    plain = pred.forward_uint8(x, *dev)
    torch.cuda.synchronize()
    pred.set_tone(tone)
    toned = pred.forward_uint8(x, *dev)
    for call in (lambda: pred.forward(f, *dev), lambda: pred.forward_batch(f.unsqueeze(0), *dev),
                 lambda: pred.detect_subjects(f.unsqueeze(0), *dev, 2)):
        with pytest.raises(RuntimeError, match="tone tables apply to byte frames"):
            call()
    det = torch.empty((1, 4, 3), device="cuda")
    with pytest.raises(RuntimeError, match="tone tables"):
        pred.native(H, W).stage_center(f.unsqueeze(0), det)
    again = pred.forward_uint8(x, *dev)                      # the refusals left the predictor as it was
    torch.cuda.synchronize()
    _assert_same(again, toned, "after the refusals")
    pred.set_tone(None)
    got = pred.forward_uint8(x, *dev)
    torch.cuda.synchronize()
    _assert_same(got, plain, "plain")
    assert plain[0] is not None and not torch.equal(plain[0], toned[0])
