"""GPU: pixel surfaces (PixelSurface / jh_pixel_surface).  The contract is bitwise: what is read through a description
equals the uint8 BGR path on the bytes the numpy reference (synthetic.pixels_to_bgr, whose properties
tests/test_pixel_surface_cpu.py checks) converts the image to -- the stand-alone conversion of every named layout with
poisoned padding, anchors against the existing forms (BGR, YuvSurface, Mono8) that need no new reference, the 3D
predictor (fused and stand-alone stems, graph replay, a description change under replay, alternation with other
formats, time batches, crop windows on the frame's border, per-image pointers at odd and 4-aligned addresses, masks,
2D views), the 2D predictor, detect_subjects and both drivers."""
import os

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import PixelSurface, SensorSurface, YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases
from tests.gpu_util import cuda
from tests.test_hip_predictor import make_cfg
from tests.test_hip_yuv_ingest import _assert_same, _debug, to_bgr_u8
from tests.test_pixel_surface_cpu import named_layouts, random_content

pytestmark = pytest.mark.gpu


def op_to_bgr(buf, s):
    """jh_op_pixels_to_bgr on (n, image_stride) numpy bytes -> (n, H, W, 3) numpy."""
    from jarvis_hybridnet_amd import _native as N
    x = cuda(torch.from_numpy(buf))
    out = torch.empty((buf.shape[0], s.height, s.width, 3), dtype=torch.uint8, device="cuda")
    N.check(N.lib().jh_op_pixels_to_bgr(N.ptr(x), s.struct(), buf.shape[0], s.height, s.width, N.ptr(out), N.stream()))
    return out.cpu().numpy()


# ---- 1: the operator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (6, 10), (34, 66), (5, 259)])
def test_pixels_to_bgr_op(H, W):
    from jarvis_hybridnet_amd import _native as N
    g = np.random.default_rng(H * 1000 + W)
    layouts = named_layouts(H, W)
    assert len(layouts) == 56
    for name, s in layouts.items():
        content = random_content(g, s)
        want = S.pixels_to_bgr(S.pack_pixel_surface(content, s, 0), s)
        for fill in (0xA5, 0x5A):                            # no byte that is no component reaches the output
            assert np.array_equal(op_to_bgr(S.pack_pixel_surface(content, s, fill), s), want), (name, fill)
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    bad = PixelSurface.packed(H, W, "rgb").struct()
    bad.step[1] = 0
    with pytest.raises(RuntimeError, match="step must be 1 .. 8"):
        N.check(N.lib().jh_op_pixels_to_bgr(N.ptr(x), bad, 1, H, W, N.ptr(x), N.stream()))
    bad = PixelSurface.packed(H, W, "rgb").struct()
    bad.sample = 0x100 | 2                                   # JH_SAMPLE_U16(2)
    with pytest.raises(RuntimeError, match="sample must be JH_SAMPLE_U8"):
        N.check(N.lib().jh_op_pixels_to_bgr(N.ptr(x), bad, 1, H, W, N.ptr(x), N.stream()))


# ---- 2: anchors that need no new reference ---------------------------------------------------------------------------
def as_pixels(y):
    """The PixelSurface that describes the same bytes as the 8-bit YuvSurface `y`."""
    return PixelSurface.from_components(y.height, y.width, y.image_stride, (y.y_offset, y.u_offset, y.v_offset),
                                        (y.y_pitch, y.c_pitch, y.c_pitch), (1, y.c_step, y.c_step), (0, 1, 1), (0, 1, 1),
                                        "yuv", y.matrix, y.range)


@pytest.mark.parametrize("H,W", [(6, 10), (34, 66)])
def test_anchors_op(H, W):
    from tests.test_hip_sensor_surface import op_to_bgr as sensor_op
    from tests.test_hip_yuv_surface import op_to_bgr as yuv_op
    from tests.test_hip_yuv_surface import padded
    g = np.random.default_rng(W)
    bgr = g.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    assert np.array_equal(op_to_bgr(bgr.reshape(3, -1), PixelSurface.packed(H, W, "bgr")), bgr)
    y = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    u, v = g.integers(0, 256, (2, 3, H // 2, W // 2), dtype=np.uint8)
    for ys in (YuvSurface(H, W, "i420"), YuvSurface(H, W, "nv12"),
               padded(H, W, "nv21", matrix="bt709", range="full")):
        buf = S.pack_yuv_surface(y, u, v, ys, 0xA5)
        assert np.array_equal(op_to_bgr(buf, as_pixels(ys)), yuv_op(buf, ys)), ys
    assert as_pixels(YuvSurface(H, W, "i420")) == PixelSurface.from_pix_fmt(H, W, "yuv420p")
    assert as_pixels(YuvSurface(H, W, "nv12")) == PixelSurface.from_pix_fmt(H, W, "nv12")
    raw = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    m = SensorSurface(H, W, "mono", pitch=W + 6, offset=9, image_stride=9 + H * (W + 6) + 10)
    buf = S.pack_sensor_surface(raw, m, 0x5A)
    p = PixelSurface.gray(H, W, pitch=W + 6, offset=9, image_stride=m.image_stride)
    assert np.array_equal(op_to_bgr(buf, p), sensor_op(buf, m))


# ---- 3 .. 8: the predictors ------------------------------------------------------------------------------------------
def yuv_planes(bgr, s):
    """uint8 BGR (..., H, W, 3) -> the (Y, U, V) planes of the description `s`: the forward transform of its matrix and
    range in float64 at full resolution, the chroma then taken at every (2^ys, 2^xs)-th pixel (test data: only the
    inverse is a contract)."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[s.matrix]
    sy, sc, y0 = {"limited": (219.0 / 255.0, 224.0 / 255.0, 16.0), "full": (1.0, 1.0, 0.0)}[s.range]
    x = np.asarray(bgr, np.float64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    luma = kr * r + (1.0 - kr - kb) * g + kb * b
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)  # noqa: E731
    u = q(128.0 + sc * (b - luma) / (2.0 * (1.0 - kb)))[..., ::1 << s.ys[1], ::1 << s.xs[1]]
    v = q(128.0 + sc * (r - luma) / (2.0 * (1.0 - kr)))[..., ::1 << s.ys[1], ::1 << s.xs[1]]
    return q(y0 + sy * luma), np.ascontiguousarray(u), np.ascontiguousarray(v)


def pixel_frames(bgr, s, fill=0xA5):
    """uint8 BGR (..., H, W, 3) -> (frames (..., image_stride) of the surface `s`, the BGR bytes its conversion gives)
    as torch CPU tensors."""
    buf = S.pack_pixel_surface(bgr if s.colour == "rgb" else yuv_planes(bgr, s), s, fill)
    return torch.from_numpy(buf), torch.from_numpy(S.pixels_to_bgr(buf, s))


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
    P = PixelSurface
    bgra_pitch = 4 * W + 64
    return {"rgb24": P.packed(H, W, "rgb"),
            "bgra_pitched": P.packed(H, W, "bgra", pitch=bgra_pitch, offset=32, image_stride=32 + H * bgra_pitch + 100),
            "gbrp": P.from_pix_fmt(H, W, "gbrp"),
            "yuyv_pitched": P.yuv_packed(H, W, "yuyv", pitch=2 * W + 64),
            "yuvj422p": P.from_pix_fmt(H, W, "yuvj422p"),
            "yuv444p_709_full": P.yuv_planar(H, W, "444", matrix="bt709", range="full"),
            "nv16": P.from_pix_fmt(H, W, "nv16")}


def native_kw(c):
    return dict(num_cameras=c["C"], num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
                roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN, std=S.STD,
                time_batch=1)


@pytest.mark.parametrize("name,stem_fuse", [("rgb24", None), ("bgra_pitched", None), ("gbrp", None),
                                            ("yuyv_pitched", None), ("yuvj422p", None), ("yuv444p_709_full", None),
                                            ("nv16", None), ("yuyv_pitched", "0")])
def test_predictor3d_pixels_bitwise(cfg2, name, stem_fuse, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)       # read when a launch plan is built
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    assert (H, W) == (512, 640)
    s = layouts(H, W)[name]
    pred = cfg2["make"]()
    x1, ref1 = pixel_frames(cfg2["bgr"], s)
    x2, ref2 = pixel_frames(cfg2["bgr2"], s, 0x5A)
    if name == "rgb24":                                     # any trailing shape of image_stride bytes: (C,H,W,3) as it is
        x1, x2 = x1.view(-1, H, W, 3), x2.view(-1, H, W, 3)
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
    if stem_fuse is None and name != "yuyv_pitched":
        return
    # which path ran: only the stand-alone kernels are launched (and profiled) as preprocess_resize / _crop
    xs = cuda(x1).unsqueeze(0)
    names = {r[0] for r in N.profile(lambda: pred.native(H, W).forward(xs, frame_layout=s))}
    pre = names & {"preprocess_resize", "preprocess_crop"}
    if stem_fuse == "0":
        assert pre == {"preprocess_resize", "preprocess_crop"}, "JH_STEM_FUSE=0 had no effect"
    else:
        assert not pre and any(n.startswith("stem_conv") for n in names), names


def test_packed_bgr_is_the_uint8_path(cfg2):
    """packed('bgr') over the (C,H,W,3) BGR tensor itself: the same tensor through both entry points."""
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    pred = cfg2["make"]()
    x = cuda(torch.from_numpy(cfg2["bgr"]))
    for _ in range(2):
        got = pred.forward_surface(x, PixelSurface.packed(H, W, "bgr"), *dev)
        want = pred.forward_uint8(x, *dev)
        torch.cuda.synchronize()
        _assert_same(got, want, "bgr")
        assert want[0] is not None


def test_description_change_under_replay(cfg2):
    """One graph-replaying predictor reads the SAME bytes as bgra, then as rgba, then as bgra: every call equals the
    uint8 path on its own description's bytes (a replay of the other recording would swap red and blue)."""
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    kw = native_kw(c)
    descs = {o: PixelSurface.packed(H, W, o) for o in ("bgra", "rgba")}
    buf = S.pack_pixel_surface(cfg2["bgr"], descs["bgra"], 0xA5)
    x = cuda(torch.from_numpy(buf)).unsqueeze(0)
    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert g.graph_replay
    g.set_calibration(*dev)
    ref = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    ref.set_calibration(*dev)
    first = {}
    for o in ("bgra", "rgba", "bgra", "bgra", "rgba"):
        got = [t.clone() for t in g.forward(x.clone(), frame_layout=descs[o])]
        want = [t.clone() for t in ref.forward(cuda(torch.from_numpy(S.pixels_to_bgr(buf, descs[o]))).unsqueeze(0))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), o
        assert int(want[2][0]) == 1
        assert torch.equal(first.setdefault(o, got[0]), got[0])
    assert not torch.equal(first["bgra"][0], first["rgba"][0])
    g.close()
    ref.close()


SEQUENCE = ("bgr", "P", "Y", "P", "bgr", "Q", "Y", "P", "bgr", "Y")


def test_pixels_alternate_with_other_formats_under_replay(cfg2):
    """A pixel-surface call alternating with 'bgr' and YuvSurface calls on ONE graph-replaying predictor, unmasked and
    masked: every call equals the eager uint8 path on its own bytes, and every later call of a form equals its first
    (the form's own graph slot: a recording replayed for another form, or a stale one, would show)."""
    from jarvis_hybridnet_amd._predictor import NativePredictor
    from tests.test_hip_yuv_surface import surface_frames
    c, inp, dev, H, W, bgr = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"], cfg2["bgr"]
    C = c["C"]
    kw = native_kw(c)
    src = {"bgr": (torch.from_numpy(bgr), {}, torch.from_numpy(bgr))}
    for name, s in (("P", layouts(H, W)["yuyv_pitched"]), ("Q", layouts(H, W)["bgra_pitched"])):
        x, ref = pixel_frames(bgr, s)
        src[name] = (x, dict(frame_layout=s), ref)
    ys = YuvSurface(H, W, "nv12", matrix="bt709", y_pitch=768, c_pitch=768)
    x, ref = surface_frames(bgr, ys)
    src["Y"] = (x, dict(frame_layout=ys), ref)
    src = {k: (cuda(x).unsqueeze(0), how, cuda(ref).unsqueeze(0)) for k, (x, how, ref) in src.items()}
    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert g.graph_replay
    g.set_calibration(*dev)
    eager = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    eager.graph_replay = False
    eager.set_calibration(*dev)
    for mask in (None, [[cam != 1 for cam in range(C)]]):
        want = {k: [t.clone() for t in eager.forward(ref, camera_mask=mask)] for k, (_, _, ref) in src.items()}
        first = {}
        for step, name in enumerate(SEQUENCE):
            x, how, _ = src[name]
            got = [t.clone() for t in g.forward(x.clone(), camera_mask=mask, **how)]
            torch.cuda.synchronize()
            for a, b in zip(got, want[name]):
                assert torch.equal(a, b), (mask is not None, step, name)
            assert int(got[2][0]) == 1, (mask is not None, step, name)
            for a, b in zip(first.setdefault(name, got), got):
                assert torch.equal(a, b), (mask is not None, step, name)
        assert not torch.equal(first["P"][0], first["bgr"][0])
    g.close()
    eager.close()


@pytest.mark.parametrize("stem_fuse", [None, "0"])
def test_crop_windows_on_the_border(stem_fuse, monkeypatch):
    """cfg2_edge: the crop centres are clamped at x low, x high and y low, so crop windows hold the frame's first row
    and its first and last column -- the first and the last group of a packed row."""
    if stem_fuse is not None:
        monkeypatch.setenv("JH_STEM_FUSE", stem_fuse)
    e = _case("cfg2_edge")
    H, W, dev = e["H"], e["W"], e["dev"]
    pred = e["make"]()
    for name, s in (("bgra", PixelSurface.packed(H, W, "bgra", pitch=4 * W + 2, offset=1,
                                                 image_stride=1 + H * (4 * W + 2))),
                    ("yuyv", PixelSurface.yuv_packed(H, W, "yuyv"))):
        x, ref = pixel_frames(e["bgr"], s)
        got = pred.forward_surface(cuda(x), s, *dev)
        torch.cuda.synchronize()
        dbg_s = _debug(pred, H, W)
        want = pred.forward_uint8(cuda(ref), *dev)
        torch.cuda.synchronize()
        dbg_b = _debug(pred, H, W)
        _assert_same(got, want, name)
        assert want[0] is not None
        for k in dbg_b:
            assert torch.equal(dbg_s[k], dbg_b[k]), (name, k)
        chm = dbg_b["center_hm"].reshape(-1, 2).cpu()
        hw = e["c"]["bbox"] // 2
        assert int((chm[:, 0] == hw).sum()) and int((chm[:, 0] == W - hw).sum()) and int((chm[:, 1] == hw).sum())


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def slices(images, first=0):
    """CPU images (n, image_stride) -> device views, image i a slice at byte offset 1 (odd) or 4 (4-aligned) of a
    larger 0xFF-filled buffer of its own, alternating."""
    views = []
    for i, img in enumerate(images):
        off = (1, 4)[(i + first) % 2]
        pool = torch.full((img.numel() + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        assert pool.data_ptr() % 16 == 0
        v = pool[off:off + img.numel()]
        v.copy_(cuda(img))
        assert v.data_ptr() % 4 == off % 4 and v.is_contiguous()
        views.append(v)
    return views


@pytest.mark.parametrize("name", ["yuyv_pitched", "bgra_pitched"])
def test_forward_images(cfg2, name):
    H, W, dev, C = cfg2["H"], cfg2["W"], cfg2["dev"], cfg2["c"]["C"]
    s = layouts(H, W)[name]
    pred = cfg2["make"]()
    x1, ref1 = pixel_frames(cfg2["bgr"], s)
    x2, _ = pixel_frames(cfg2["bgr2"], s, 0x5A)
    for x, first in ((x1, 0), (x2, 1), (x1, 1)):            # (the third call: every image at the other alignment)
        want = [t.clone() for t in pred.forward_batch(cuda(x).unsqueeze(0), *dev, frame_layout=s)]
        got = [t.clone() for t in pred.forward_images(slices(x, first), *dev, frame_layout=s)]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, first)
        assert int(want[2][0]) == 1
    # two frame sets in one call, against the uint8 path
    got = pred.forward_images([slices(x1), slices(x2, 1)], *dev, frame_layout=s)
    want = pred.forward_batch(cuda(torch.stack([x1, x2])), *dev, frame_layout=s)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b), (name, "T=2")
    assert int(want[2].sum()) == 2 and not torch.equal(want[0][0], want[0][1])
    if name != "yuyv_pitched":
        return
    # with a camera mask and the 2D views, against the uint8 path on the converted bytes
    mask = [[c != 1 for c in range(C)]]
    got = pred.forward_images(slices(x1, 1), *dev, frame_layout=s, camera_mask=mask, return_2d=True)
    want = pred.forward_batch(cuda(ref1).unsqueeze(0), *dev, camera_mask=mask, return_2d=True)
    torch.cuda.synchronize()
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(_bits(a), _bits(b))
    for f in want[3]._fields:                                # NaNs compared bitwise
        assert torch.equal(_bits(getattr(got[3], f)), _bits(getattr(want[3], f))), f
    assert int(want[2][0]) == 1 and int(want[3].used[0, 1]) == 0 and int(want[3].used.sum()) == C - 1


def _pred2d():
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    tags = ["cam0_j12", "cam2_j12"]
    c = cases.PREDICTOR2D_CASES[tags[0]]
    ins = [cases.predictor2d_inputs(t) for t in tags]
    cfg = make_cfg(dict(J=c["J"], bbox=c["bbox"], C=1, roi=32, spacing=2), c["center_size"])
    cfg.KEYPOINT_NAMES = ["joint%d" % i for i in range(c["J"])]
    bgr = np.concatenate([to_bgr_u8(i["img"]) for i in ins])                  # (2, H, W, 3)
    return JarvisPredictor2D(cfg, ins[0]["sd_center"], ins[0]["sd_kp"]), cfg, bgr


def test_predictor2d_pixels_bitwise():
    pred, _, bgr = _pred2d()
    H, W = bgr.shape[1:3]
    for name, s in (("rgb24", PixelSurface.packed(H, W, "rgb")),
                    ("uyvy", PixelSurface.yuv_packed(H, W, "uyvy", pitch=2 * W + 64, offset=32))):
        x, ref = pixel_frames(bgr, s)
        if name == "rgb24":
            x = x.view(-1, H, W, 3)
        got = [t.clone() for t in pred.forward_batch(cuda(x), frame_layout=s)]
        want = [t.clone() for t in pred.forward_batch(cuda(ref))]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), name
        assert int(want[2].sum()) == 2
        p1, c1 = pred.forward_surface(cuda(x[0]), s)
        p2, c2 = pred.forward(cuda(x[:1]), frame_layout=s)
        w1 = pred.forward_batch(cuda(ref[:1]))
        torch.cuda.synchronize()
        assert torch.equal(p1, w1[0][0].long()) and torch.equal(c1, w1[1][0])
        assert torch.equal(p2, p1) and torch.equal(c2, c1)
        got = [t.clone() for t in pred.forward_images(slices(x.reshape(2, -1)), frame_layout=s)]
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, "images")


def test_detect_subjects_pixels(cfg2):
    from tests.test_hip_subjects import same_subjects
    H, W, dev = cfg2["H"], cfg2["W"], cfg2["dev"]
    s = layouts(H, W)["yuyv_pitched"]
    pred = cfg2["make"]()
    x1, ref1 = pixel_frames(cfg2["bgr"], s)
    x2, ref2 = pixel_frames(cfg2["bgr2"], s)
    x, ref = cuda(torch.stack([x1, x2])), cuda(torch.stack([ref1, ref2]))
    got, gp = pred.detect_subjects(x, *dev, 2, frame_layout=s, return_peaks=True)
    want, wp = pred.detect_subjects(ref, *dev, 2, return_peaks=True)
    torch.cuda.synchronize()
    assert same_subjects(got, want) and torch.equal(_bits(gp), _bits(wp))
    assert int(want.views[:, 0].min()) >= 2                  # a subject was found in both frame sets
    img, _ = pred.detect_subjects([slices(x1), slices(x2, 1)], *dev, 2, frame_layout=s, images=True, return_peaks=True)
    torch.cuda.synchronize()
    assert same_subjects(img, want)


def _read(path, name):
    return open(os.path.join(path, name), newline="").read()


@pytest.mark.parametrize("streams", [1, 3])
def test_drivers_pixels_csv_identical(cfg2, tmp_path, streams):
    """predict3D_frames and predict2D_frames with frame_layout=PixelSurface at time_batch 4 write CSVs byte-identical
    to the BGR runs on the converted frames."""
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    from jarvis_hybridnet_amd.prediction.predict2D import predict2D_frames
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    c, inp, dev, H, W = cfg2["c"], cfg2["inp"], cfg2["dev"], cfg2["H"], cfg2["W"]
    cfg = make_cfg(c, c["center_size"])
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = (inp["cam"], inp["intr"], inp["dist"])
    pred = cfg2["make"]()
    s = layouts(H, W)["yuyv_pitched"]
    bgr = [to_bgr_u8(S.blob_frames(calib, W, H, c["J"], 70 + i)[0]) for i in range(6)]
    pairs = [pixel_frames(b, s) for b in bgr]
    raw = [p[0].numpy() for p in pairs]
    ref = [p[1].numpy() for p in pairs]
    kw = dict(time_batch=4, streams=streams)
    assert predict3D_frames(pred, raw, *dev, cfg, str(tmp_path / "s"), frame_layout=s, **kw) == 6
    assert predict3D_frames(pred, ref, *dev, cfg, str(tmp_path / "b"), **kw) == 6
    release_ingest_buffers(pred)
    want = _read(tmp_path / "b", "data3D.csv")
    assert _read(tmp_path / "s", "data3D.csv") == want
    rows = want.splitlines()[2:]
    assert len(rows) == 6 and len(set(rows)) == 6 and all(not r.startswith("NaN") for r in rows)
    # 2D driver: camera 0 of each frame set, (H,W,3) RGB arrays as PIL / imageio hand them out
    p2, cfg2d, _ = _pred2d()
    m = PixelSurface.packed(H, W, "rgb")
    rgb = [np.ascontiguousarray(b[0][..., ::-1]) for b in bgr]
    assert predict2D_frames(p2, rgb, cfg2d, str(tmp_path / "2s"), frame_layout=m, time_batch=4) == 6
    assert predict2D_frames(p2, [b[0] for b in bgr], cfg2d, str(tmp_path / "2b"), time_batch=4) == 6
    release_ingest_buffers(p2)
    want = _read(tmp_path / "2b", "data2D.csv")
    assert _read(tmp_path / "2s", "data2D.csv") == want
    assert all(not r.startswith("NaN") for r in want.splitlines()[2:])
