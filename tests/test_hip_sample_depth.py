"""GPU: samples wider than a byte (16-bit words, GenICam 10p / 12p, P010 / yuv420p10le).  The contract is the bitwise
one of the 8-bit descriptions: a frame read through a wide description equals the 8-bit description on the reduced
bytes, min(sample >> shift, 255), and therefore the uint8 BGR path on the demosaiced resp. converted bytes -- the
stand-alone conversions with poisoned non-sample bytes and bits, the 3D predictor (fused and stand-alone stems, graph
replay, a change of sample width under replay, time batches, crop windows on the border, per-image pointers, masks, 2D
views), the 2D predictor and both drivers."""
import os

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases
from tests.gpu_util import cuda
from tests.test_hip_predictor import make_cfg
from tests.test_hip_sensor_surface import _bits, _pred2d, op_to_bgr as sensor_op
from tests.test_hip_yuv_ingest import _assert_same, _debug, to_bgr_u8
from tests.test_hip_yuv_surface import op_to_bgr as yuv_op
from tests.test_yuv_surface_cpu import ORDERS, ROWS, surface_to_bgr

pytestmark = pytest.mark.gpu

BAYER = ("rggb", "bggr", "grbg", "gbrg")
# (bits, container, samples above the declared depth?)
SAMPLES = ((12, "u16", False), (10, "u16", True), (16, "u16", False), (10, "u16msb", False), (10, "packed", False),
           (12, "packed", False))


def sensor_layouts(H, W, pattern, bits, container):
    """The tight layout and a pitched one: rows 5 (packed) or 6 bytes longer, the first sample at byte 9 resp. 10 and
    a 10-byte gap behind the last row."""
    tight = SensorSurface(H, W, pattern, bits=bits, container=container)
    pad, off = (5, 9) if container == "packed" else (6, 10)
    pitch = tight.row_bytes + pad
    return tight, SensorSurface(H, W, pattern, pitch=pitch, offset=off, image_stride=off + H * pitch + 10, bits=bits,
                                container=container)


def check_sensor_op(H, W, patterns):
    g = np.random.default_rng(H * 100 + W)
    raw8 = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    raw8[0, 0, -1] = 255                                   # the last sample of a row, at the top of the range
    for p in patterns:
        want = S.sensor_to_bgr(raw8, p)
        for bits, container, over in SAMPLES:
            tight, pitched = sensor_layouts(H, W, p, bits, container)
            wide = S.widen(raw8, tight.shift, g, saturate=over)
            assert np.array_equal(S.reduce_samples(wide, tight.shift), raw8)
            assert np.array_equal(sensor_op(S.pack_sensor_surface(wide, tight), tight), want), (p, bits, container)
            for fill in (0xA5, 0x5A):                      # no byte and no bit that is not a sample reaches the output
                got = sensor_op(S.pack_sensor_surface(wide, pitched, fill), pitched)
                assert np.array_equal(got, want), (p, bits, container, fill)


@pytest.mark.parametrize("H,W", [(4, 4), (6, 10), (34, 66)])
def test_bayer_to_bgr_op(H, W):
    check_sensor_op(H, W, BAYER)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 7), (5, 9), (2, 6), (6, 10)])
def test_mono_to_bgr_op(H, W):
    """W % 4 = 1, 3, 1, 2, 2: with (4, 4) of the Bayer case every 10p phase and both 12p phases end a row."""
    check_sensor_op(H, W, ("mono",))


def test_sensor_op_refuses_unknown_codes():
    from jarvis_hybridnet_amd import _native as N
    x = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for code in (1, 0x109, 0x201, 0x400):
        bad = SensorSurface(4, 4).struct()
        bad.reserved = code
        with pytest.raises(RuntimeError, match="sample"):
            N.check(N.lib().jh_op_sensor_to_bgr(N.ptr(x), bad, 1, 4, 4, N.ptr(x), N.stream()))
    bad = YuvSurface(4, 4).struct()
    bad.reserved = 0x200
    with pytest.raises(RuntimeError, match="sample"):
        N.check(N.lib().jh_op_yuv_surface_to_bgr(N.ptr(x), bad, 1, 4, 4, N.ptr(x), N.stream()))


def order_of(s):
    semi, u_first = s.c_step == 2, s.u_offset < s.v_offset
    return ("nv12" if u_first else "nv21") if semi else ("i420" if u_first else "yv12")


def yuv_reference(y8, u8, v8, s):
    """The BGR bytes of the 8-bit description (tight, same order, matrix and range) on the reduced planes."""
    t = YuvSurface(s.height, s.width, order_of(s), matrix=s.matrix, range=s.range)
    return surface_to_bgr(S.pack_yuv_surface(y8, u8, v8, t), t)


def yuv_layouts(H, W, order, **kw):
    """Tight, and pitched: luma rows 12 bytes longer, chroma rows 12 (semi-planar) or 8, three unused luma rows and
    a 10-byte gap before image_stride."""
    semi = order.startswith("nv")
    tight = YuvSurface(H, W, order, **kw)
    args = dict(y_pitch=2 * W + 12, c_pitch=(2 * W + 12) if semi else W + 8, luma_rows=H + 3, **kw)
    return tight, YuvSurface(H, W, order, image_stride=YuvSurface(H, W, order, **args).image_stride + 10, **args)


@pytest.mark.parametrize("H,W", [(4, 4), (6, 10), (34, 66)])
def test_yuv16_to_bgr_op(H, W):
    g = np.random.default_rng(W)
    y8 = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    u8, v8 = g.integers(0, 256, (2, 3, H // 2, W // 2), dtype=np.uint8)
    y8[0, 0, -1], u8[0, 0, -1], v8[0, -1, -1] = 255, 255, 255
    for i, order in enumerate(ORDERS):
        matrix, rng = list(ROWS)[i]
        for kw in (dict(bits=10), dict(bits=10, msb=True)):                     # shift 2 and shift 8
            tight, pitched = yuv_layouts(H, W, order, matrix=matrix, range=rng, **kw)
            assert tight.shift == (8 if kw.get("msb") else 2)
            y, u, v = (S.widen(p, tight.shift, g, saturate=True) for p in (y8, u8, v8))
            want = yuv_reference(y8, u8, v8, tight)
            assert np.array_equal(yuv_op(S.pack_yuv_surface(y, u, v, tight), tight), want), (order, kw, "tight")
            for fill in (0xA5, 0x5A):
                got = yuv_op(S.pack_yuv_surface(y, u, v, pitched, fill), pitched)
                assert np.array_equal(got, want), (order, kw, fill)
            # an image_stride that is 2 mod 4: every second image's chroma pair is fetched as two 16-bit loads
            q = pitched
            s2 = YuvSurface.from_planes(H, W, q.y_offset, q.y_pitch, q.u_offset, q.v_offset, q.c_pitch, q.c_step,
                                        q.image_stride + 2 * (q.image_stride % 4 == 0), matrix=matrix, range=rng, **kw)
            assert s2.image_stride % 4 == 2
            assert np.array_equal(yuv_op(S.pack_yuv_surface(y, u, v, s2, 0x33), s2), want), (order, kw, "2 mod 4")


# ------------------------------------------------------------------------------------------------- predictor level
def wide_frames(bgr, s, fill=0xA5, seed=0):
    """uint8 BGR (..., H, W, 3) -> (frames (..., image_stride) of the wide description `s`, the BGR bytes the 8-bit
    description gives on the reduced samples) as torch CPU tensors."""
    g = np.random.default_rng(seed)
    if isinstance(s, SensorSurface):
        wide = S.widen(S.mosaic(bgr, s.pattern), s.shift, g, saturate=s.container == "u16")
        ref = S.sensor_to_bgr(S.reduce_samples(wide, s.shift), s.pattern)
        return torch.from_numpy(S.pack_sensor_surface(wide, s, fill)), torch.from_numpy(ref)
    planes = [S.widen(p, s.shift, g, saturate=True) for p in S.bgr_to_yuv(bgr, s.matrix, s.range)]
    ref = yuv_reference(*(S.reduce_samples(p, s.shift) for p in planes), s)
    return torch.from_numpy(S.pack_yuv_surface(*planes, s, fill)), torch.from_numpy(ref)


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
    row12 = (12 * W + 7) // 8
    return {"mono12_u16": SensorSurface(H, W, "mono", bits=12),
            "rggb12p_pitched": SensorSurface(H, W, "rggb", pitch=row12 + 43, offset=4097,
                                             image_stride=4097 + H * (row12 + 43) + 333, bits=12, container="packed"),
            "gbrg10p": SensorSurface(H, W, "gbrg", bits=10, container="packed"),
            "p010_pitched": YuvSurface(H, W, "nv12", bits=10, msb=True, y_pitch=1536, c_pitch=1536, luma_rows=544),
            "yuv420p10le": YuvSurface(H, W, "i420", bits=10)}


@pytest.mark.parametrize("name,stem_fuse", [("mono12_u16", None), ("rggb12p_pitched", None), ("gbrg10p", None),
                                            ("p010_pitched", None), ("yuv420p10le", None), ("rggb12p_pitched", "0")])
def test_predictor3d_wide_bitwise(cfg2, name, stem_fuse, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)       # read when a launch plan is built
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    assert (H, W) == (512, 640)
    s = layouts(H, W)[name]
    pred = cfg2["make"]()
    x1, ref1 = wide_frames(cfg2["bgr"], s)
    x2, ref2 = wide_frames(cfg2["bgr2"], s, 0x5A, 1)
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


def test_crop_windows_on_the_border():
    """cfg2_edge: crop windows hold the frame's first row and its first and last column, where a Bayer pixel takes the
    RGB of its clamped interior neighbour -- and where a packed row begins and ends."""
    e = _case("cfg2_edge")
    H, W, dev = e["H"], e["W"], e["dev"]
    pred = e["make"]()
    row12 = (12 * W + 7) // 8
    for s in (SensorSurface(H, W, "bggr", pitch=row12 + 3, offset=1, image_stride=1 + H * (row12 + 3), bits=12,
                            container="packed"),
              SensorSurface(H, W, "grbg", bits=10, container="packed")):
        x, ref = wide_frames(e["bgr"], s)
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


def _native_pair(cfg2):
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    kw = dict(num_cameras=c["C"], num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN, std=S.STD, time_batch=1)
    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    ref = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    for p in (g, ref):
        p.set_calibration(*dev)
    return g, ref


def test_sample_width_change_under_replay(cfg2):
    """One graph-replaying predictor reads the SAME bytes as Mono8, then as Mono12p, then as Mono8: rows of 960 bytes,
    the 12p stream of a frame set; Mono8 takes the first 640 bytes of each row as its pixels (no picture, but a
    definite one).  Every call equals the uint8 path on its own reading, bit for bit, and the two readings differ: a
    replay of the other recording would give the other one's result."""
    H, W = cfg2["H"], cfg2["W"]
    g, ref = _native_pair(cfg2)
    assert g.graph_replay
    row12 = 12 * W // 8
    p12 = SensorSurface(H, W, "mono", bits=12, container="packed")
    m8 = SensorSurface(H, W, "mono", pitch=row12)
    assert p12.image_stride == m8.image_stride == H * row12
    green = S.mosaic(cfg2["bgr"], "mono")
    wide = S.widen(green, 4, np.random.default_rng(3))
    buf = S.pack_sensor_surface(wide, p12)
    refs = {"m8": np.repeat(buf.reshape(-1, H, row12)[..., :W, None], 3, -1),
            "p12": S.sensor_to_bgr(S.reduce_samples(wide, 4), "mono")}
    x = cuda(torch.from_numpy(buf)).unsqueeze(0)
    first = {}
    for k in ("m8", "p12", "m8"):
        got = [t.clone() for t in g.forward(x.clone(), frame_layout=m8 if k == "m8" else p12)]
        want = [t.clone() for t in ref.forward(cuda(torch.from_numpy(refs[k])).unsqueeze(0))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(_bits(a), _bits(b)), k
        if k == "p12":
            assert int(want[2][0]) == 1
        got = torch.cat([_bits(t).reshape(-1) for t in got[:2]])
        assert torch.equal(first.setdefault(k, got), got)
    assert not torch.equal(first["m8"], first["p12"])
    g.close()
    ref.close()


def test_forward_images_alignment(cfg2):
    """Packed images at odd addresses equal the contiguous call; an image of 16-bit samples at an odd address is an
    error before anything is enqueued, at an even address it equals the contiguous call."""
    from jarvis_hybridnet_amd import _native as N
    H, W, dev, C = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["c"]["C"]
    pred = cfg2["make"]()
    L = layouts(H, W)

    def pool_views(x, starts):
        """The C images of x in one 0xFF-filled pool, image i at byte starts[i] behind the end of image i - 1."""
        n = x.shape[1]
        pool = torch.full((C * (n + 64),), 0xFF, dtype=torch.uint8, device="cuda")
        assert pool.data_ptr() % 16 == 0
        views, cur = [], 0
        for i in range(C):
            cur += starts[i]
            views.append(pool[cur:cur + n])
            views[-1].copy_(cuda(x[i]))
            cur += n
        return views

    for name, starts, packed in (("rggb12p_pitched", [1, 2, 3, 5], True), ("gbrg10p", [3, 1, 1, 2], True),
                                 ("mono12_u16", [2, 6, 4, 10], False), ("p010_pitched", [4, 2, 2, 6], False),
                                 ("yuv420p10le", [2, 2, 4, 2], False)):
        s = L[name]
        x, _ = wide_frames(cfg2["bgr"], s)
        assert x.shape[0] == C == 4
        want = [t.clone() for t in pred.forward_batch(cuda(x.unsqueeze(0)), *dev, frame_layout=s)]
        views = pool_views(x, starts)
        assert sum(v.data_ptr() % 2 for v in views) == (3 if packed else 0)
        got = pred.forward_images(views, *dev, frame_layout=s)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), name
        assert int(want[2][0]) == 1
    # 16-bit samples at an odd address: refused on the host, image 2 named, the outputs untouched
    nat = pred.native(H, W)
    J = cfg2["c"]["J"]
    for name in ("mono12_u16", "p010_pitched"):
        s = L[name]
        x, _ = wide_frames(cfg2["bgr"], s)
        views = pool_views(x, [2, 2, 3, 3])
        assert [v.data_ptr() % 2 for v in views] == [0, 0, 1, 0]
        with pytest.raises(RuntimeError, match="image 2 .*2-byte aligned"):
            pred.forward_images(views, *dev, frame_layout=s)
        out = (torch.full((1, J, 3), -7.0, device="cuda"), torch.full((1, J), -7.0, device="cuda"),
               torch.full((1,), -7, device="cuda", dtype=torch.int32))
        table = (N.c_void_p * C)(*[v.data_ptr() for v in views])
        yuv, sensor = (None, s.struct()) if isinstance(s, SensorSurface) else (s.struct(), None)
        fmt = N.FRAME_SENSOR if sensor is not None else N.FRAME_SURFACE
        assert N.lib().jh_predictor_forward_images(nat.handle, table, C, fmt, yuv, sensor, None,
                                                   *(N.ptr(t) for t in out), N.stream()) != 0
        assert b"image 2" in N.lib().jh_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out)


def test_mask_and_views2d_behind_a_packed_surface(cfg2):
    H, W, dev, C = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["c"]["C"]
    s = layouts(H, W)["rggb12p_pitched"]
    pred = cfg2["make"]()
    x, ref = wide_frames(cfg2["bgr"], s)
    clean_ref = ref.clone()
    mask = [c != 1 for c in range(C)]
    x, ref = x.clone(), ref.clone()
    x[1] = 0xFF                                              # garbage in the masked slot, of both forms
    ref[1] = 0xFF
    got = pred.forward_surface(cuda(x), s, *dev, camera_mask=mask, return_2d=True)
    want = pred.forward_uint8(cuda(ref), *dev, camera_mask=mask, return_2d=True)
    clean = pred.forward_uint8(cuda(clean_ref), *dev, camera_mask=mask)
    torch.cuda.synchronize()
    assert want[0] is not None and got[0] is not None
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    assert torch.equal(_bits(got[0]), _bits(clean[0]))       # the garbage had no effect
    for f in want[2]._fields:                                # NaNs compared bitwise
        assert torch.equal(_bits(getattr(got[2], f)), _bits(getattr(want[2], f))), f
    assert int(want[2].used[0, 1]) == 0 and int(want[2].used.sum()) == C - 1


def test_predictor2d_wide_bitwise():
    pred, _, bgr = _pred2d()
    H, W = bgr.shape[1:3]
    row10 = (10 * W + 7) // 8
    for s in (SensorSurface(H, W, "mono", pitch=row10 + 61, offset=33, bits=10, container="packed"),
              YuvSurface(H, W, "nv12", bits=10, msb=True)):
        x, ref = wide_frames(bgr, s)
        got = [t.clone() for t in pred.forward_batch(cuda(x), frame_layout=s)]
        want = [t.clone() for t in pred.forward_batch(cuda(ref))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), s
        assert int(want[2].sum()) == 2
        p1, c1 = pred.forward_surface(cuda(x[0]), s)
        w1 = pred.forward_batch(cuda(ref[:1]))
        torch.cuda.synchronize()
        assert torch.equal(p1, w1[0][0].long()) and torch.equal(c1, w1[1][0])


def _read(path, name):
    return open(os.path.join(path, name), newline="").read()


def test_drivers_packed_csv_identical(cfg2, tmp_path):
    """predict3D_frames (time_batch 3, two streams) and predict2D_frames with a packed layout write CSVs byte-identical
    to the BGR runs on the reduced, demosaiced frames; plain arrays and `fill` callables."""
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    from jarvis_hybridnet_amd.prediction.predict2D import predict2D_frames
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    cfg = make_cfg(c, c["center_size"])
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = (inp["cam"], inp["intr"], inp["dist"])
    pred = cfg2["make"]()
    s = layouts(H, W)["rggb12p_pitched"]
    bgr = [to_bgr_u8(S.blob_frames(calib, W, H, c["J"], 70 + i)[0]) for i in range(5)]
    pairs = [wide_frames(b, s, seed=i) for i, b in enumerate(bgr)]
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
    # 2D driver: camera 0 of each frame set, BayerRG12p in padded rows
    p2, cfg2d, _ = _pred2d()
    m = SensorSurface(H, W, "rggb", pitch=(12 * W + 7) // 8 + 31, bits=12, container="packed")
    pairs = [wide_frames(b[0], m, seed=i) for i, b in enumerate(bgr)]
    assert predict2D_frames(p2, [p[0].numpy() for p in pairs], cfg2d, str(tmp_path / "2s"), time_batch=2,
                            frame_layout=m) == 5
    assert predict2D_frames(p2, [p[1].numpy() for p in pairs], cfg2d, str(tmp_path / "2b"), time_batch=2) == 5
    release_ingest_buffers(p2)
    want = _read(tmp_path / "2b", "data2D.csv")
    assert _read(tmp_path / "2s", "data2D.csv") == want
    assert all(not r.startswith("NaN") for r in want.splitlines()[2:])
