"""GPU: per-image frame pointers (jh_predictor_forward_images / JarvisPredictor*.forward_images).  The feature moves
WHERE bytes are read from and changes no arithmetic, so every comparison is torch.equal against the contiguous entry
point on the same images.  All 3D cases run at the cfg2 geometry (4 cameras, 512 x 640), whose inputs give valid == 1.

The images of a call are SCATTERED (scatter below): one uint8 pool, the images in reversed order at unequal gaps, the
gaps filled with 0xFF (fp32: NaN) -- a fetch that falls back to base + n * stride, or strays outside an image, changes
the result --, one image of every byte form at an ODD address (NV12 / semi-planar: the two-byte chroma read), every
fp32 image 4- but not 16-byte aligned.  A second variant uses separately allocated tensors."""
import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases
from tests.gpu_util import cuda
from tests.test_hip_predictor import make_cfg
from tests.test_hip_yuv_ingest import to_bgr_u8

pytestmark = pytest.mark.gpu

H, W = 512, 640
FORMS = ("fp32", "bgr", "i420", "nv12", "nv12_pitched_709", "yv12_full", "mono", "rggb")


def how(name):
    """The keyword arguments that tell forward_batch / forward_images what the frames of form `name` are."""
    if name in ("i420", "nv12"):
        return dict(frame_format=name)
    layout = {"nv12_pitched_709": YuvSurface(H, W, "nv12", matrix="bt709", y_pitch=768, c_pitch=768, luma_rows=544),
              "yv12_full": YuvSurface(H, W, "yv12", range="full"),
              "mono": SensorSurface(H, W, "mono"),
              "rggb": SensorSurface(H, W, "rggb", pitch=768, offset=4096, image_stride=4096 + H * 768 + 333)}.get(name)
    return dict(frame_layout=layout) if layout is not None else {}


def frames_of(name, imgs):
    """(C,3,H,W) fp32 RGB -> the (C, ...) CPU tensor of the same frame set in source form `name`."""
    if name == "fp32":
        return imgs.contiguous()
    bgr = to_bgr_u8(imgs)
    if name == "bgr":
        return torch.from_numpy(bgr)
    if name in ("i420", "nv12"):
        return torch.from_numpy(S.bgr_to_yuv420(bgr, name))
    s = how(name)["frame_layout"]
    if isinstance(s, SensorSurface):
        return torch.from_numpy(S.pack_sensor_surface(S.mosaic(bgr, s.pattern), s, 0xA5))
    return torch.from_numpy(S.pack_yuv_surface(*S.bgr_to_yuv(bgr, s.matrix, s.range), s, 0xA5))


def offsets(n, nbytes, f32, variant=0):
    """Byte offsets of n images in the pool (index = position in the call) and the pool size: the LAST image of the
    call first, the gap in front of the k-th image placed 64 (k + 1) + 128 variant bytes and a little more -- fp32: up
    to the next offset that is 4 or 12 mod 16; bytes: the second image placed odd, the others even."""
    offs, cur = {}, 0
    for k, i in enumerate(reversed(range(n))):
        cur += 64 * (k + 1) + 128 * variant
        if f32:
            cur = (cur + 15) // 16 * 16 + (4 if k % 2 == 0 else 12)
        else:
            cur += (cur % 2) ^ int(k == 1)
        offs[i] = cur
        cur += nbytes
    return offs, cur + 64


def scatter(images, variant=0):
    """CPU tensors (one image each, one shape and dtype) -> device views of ONE 0xFF-filled uint8 pool, in the order
    given, placed as the module docstring says.  `variant` changes every gap."""
    nbytes = images[0].numel() * images[0].element_size()
    f32 = images[0].dtype == torch.float32
    offs, size = offsets(len(images), nbytes, f32, variant)
    pool = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    assert pool.data_ptr() % 16 == 0
    views = []
    for i, img in enumerate(images):
        v = pool[offs[i]:offs[i] + nbytes]
        v.copy_(cuda(img).reshape(-1).view(torch.uint8))
        v = v.view(img.dtype).view(img.shape)
        assert v.data_ptr() == pool.data_ptr() + offs[i] and v.is_contiguous()
        views.append(v)
    if f32:
        assert all(v.data_ptr() % 4 == 0 and v.data_ptr() % 16 != 0 for v in views)
        assert bool(torch.isnan(pool[:4].view(torch.float32)).all())
    else:
        assert sum(v.data_ptr() % 2 for v in views) == 1
    assert [v.data_ptr() for v in views] == sorted((v.data_ptr() for v in views), reverse=True)
    assert len({b - a for a, b in zip(sorted(offs.values()), sorted(offs.values())[1:])}) == len(images) - 1
    return views


def separate(images):
    """The second variant: every image an allocation of its own."""
    return [cuda(img.clone()) for img in images]


@pytest.fixture(scope="module")
def rig():
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    assert (c["H"], c["W"]) == (H, W)
    calib = (inp["cam"], inp["intr"], inp["dist"])
    # two DIFFERENT frame sets; every source form of each, computed once and never changed
    sets = [inp["imgs"], torch.roll(inp["imgs"], (24, -40), dims=(2, 3)).contiguous()]
    frames = {name: [frames_of(name, s) for s in sets] for name in FORMS}
    rig = dict(c=c, inp=inp, dev=[cuda(t) for t in calib], frames=frames, C=c["C"])
    # one pair of predictors for the fused-stem cases: `ref` eager at both time batches, `pred` as it comes (time batch
    # 1 replays its graph, time batch 2 is eager)
    rig["ref"], rig["pred"] = eager(eager(predictor(rig), 1), 2), predictor(rig)
    return rig


def predictor(rig, size=None, seeds=None):
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    c, inp = dict(rig["c"]), rig["inp"]
    if size is None:
        return JarvisPredictor3D(make_cfg(c, c["center_size"]), inp["sd_center"], inp["sd_hybrid"])
    c["size"] = size
    return JarvisPredictor3D(make_cfg(c, c["center_size"]), S.efficienttrack_weights(size, 1, seeds[0]),
                             S.hybridnet_weights(size, c["J"], seeds[1]))


def eager(pred, T):
    """The reference of every case: `pred`'s native predictor for time batch T with graph replay off."""
    n = pred.native(H, W, time_batch=T)
    n.graph_replay = False
    assert not n.graph_replay
    return pred


def clone(res):
    return [t.clone() for t in res]


def same(got, want, what):
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b), what


def every_form_equals_contiguous(rig, ref, pred, names):
    dev, C = rig["dev"], rig["C"]
    assert pred.native(H, W).graph_replay                       # (time_batch 1 replays; time_batch 2 is eager)
    for name in names:
        a, b = rig["frames"][name]
        kw = how(name)
        for k, x in enumerate((a, b)):
            want = clone(ref.forward_batch(cuda(x.unsqueeze(0)), *dev, **kw))
            assert int(want[2][0]) == 1, (name, k)
            for variant, views in (("pool", scatter(list(x), k)), ("separate", separate(list(x)))):
                same(pred.forward_images(views, *dev, **kw), want, (name, "T=1", k, variant))
        want2 = clone(ref.forward_batch(cuda(torch.stack([a, b])), *dev, **kw))
        assert int(want2[2].sum()) == 2 and not torch.equal(want2[0][0], want2[0][1]), name
        views = scatter(list(a) + list(b))
        same(pred.forward_images([views[:C], views[C:]], *dev, **kw), want2, (name, "T=2"))
        views = separate(list(a) + list(b))
        same(pred.forward_images([views[:C], views[C:]], *dev, **kw), want2, (name, "T=2", "separate"))


@pytest.mark.parametrize("name", FORMS)
def test_every_form_equals_its_contiguous_path(rig, name):
    every_form_equals_contiguous(rig, rig["ref"], rig["pred"], [name])


@pytest.mark.parametrize("name", ["bgr", "nv12"])
def test_stand_alone_kernels(rig, name, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    monkeypatch.setenv("JH_STEM_FUSE", "0")                     # read when a launch plan is built
    pred = predictor(rig)
    every_form_equals_contiguous(rig, eager(eager(predictor(rig), 1), 2), pred, [name])
    views = scatter(list(rig["frames"][name][0]))
    described = N.frame_images(views, rig["C"], **how(name))
    names = {r[0] for r in N.profile(lambda: pred.native(H, W).forward_images(described))}
    assert {"preprocess_resize", "preprocess_crop"} <= names, "JH_STEM_FUSE=0 had no effect"


@pytest.mark.parametrize("name", ["bgr", "nv12_pitched_709"])
def test_table_is_consulted_per_image(rig, name):
    ref, pred = rig["ref"], rig["pred"]
    dev, x, kw = rig["dev"], rig["frames"][name][0], how(name)
    plain = clone(ref.forward_batch(cuda(x.unsqueeze(0)), *dev, **kw))
    swapped = clone(ref.forward_batch(cuda(x[[1, 0, 2, 3]].unsqueeze(0)), *dev, **kw))
    torch.cuda.synchronize()
    assert not torch.equal(plain[0], swapped[0])
    v = scatter(list(x))
    for _ in range(2):                                          # the second pair replays
        same(pred.forward_images([v[1], v[0], v[2], v[3]], *dev, **kw), swapped, "exchanged")
        same(pred.forward_images(v, *dev, **kw), plain, "in order")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", ["bgr", "nv12"])
def test_graph_replay_follows_the_pointers(rig, name):
    """ONE replaying predictor: three scatterings of frame set A and two of frame set B, interleaved with contiguous
    calls of the same format, unmasked and with camera 1 masked.  A stale pointer or a stale recording would give
    another call's result."""
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c, inp, dev, C = rig["c"], rig["inp"], rig["dev"], rig["C"]
    kw = dict(num_cameras=C, num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"], roi_cube_size=c["roi"],
              grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN, std=S.STD, time_batch=1)
    g, e = (NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw) for _ in range(2))
    e.graph_replay = False
    assert g.graph_replay and not e.graph_replay
    for p in (g, e):
        p.set_calibration(*dev)
    fkw = {k: v for k, v in how(name).items() if k == "frame_format"}
    mask = [[cam != 1 for cam in range(C)]]
    A, B = rig["frames"][name]
    contig = {"A": cuda(A.unsqueeze(0)), "B": cuda(B.unsqueeze(0))}
    want = {(s, m is not None): clone(e.forward(contig[s], camera_mask=m, **fkw)) for s in "AB" for m in (None, mask)}
    torch.cuda.synchronize()
    assert not torch.equal(want["A", False][0], want["B", False][0])
    assert not torch.equal(want["A", False][0], want["A", True][0])
    pools = {("A", 0): scatter(list(A), 0), ("A", 1): scatter(list(A), 1), ("A", 2): separate(list(A)),
             ("B", 0): scatter(list(B), 2), ("B", 1): separate(list(B))}
    steps = [("img", "A", 0, None), ("contig", "A", None, None), ("img", "B", 0, None), ("contig", "A", None, mask),
             ("img", "A", 1, mask), ("contig", "B", None, None), ("img", "B", 1, None), ("img", "A", 2, None),
             ("contig", "B", None, mask), ("img", "B", 0, mask), ("img", "A", 0, None)]
    for i, (kind, s, v, m) in enumerate(steps):
        if kind == "img":
            views = pools[s, v]
            got = g.forward_images(N.frame_images(views, C, **fkw), camera_mask=m)
        else:
            got = g.forward(contig[s], camera_mask=m, **fkw)
        same(got, want[s, m is not None], (i, kind, s, v, m is not None))
        assert int(got[2][0]) == 1
    g.close()
    e.close()


def test_masks_and_views2d(rig):
    """return_2d on a masked and an unmasked call of a replaying predictor; the masked camera's slot points at another
    camera's image."""
    ref, pred = rig["ref"], rig["pred"]
    dev, C, x = rig["dev"], rig["C"], rig["frames"]["bgr"][0]
    assert pred.native(H, W).graph_replay
    v = scatter(list(x))
    mask = [[cam != 1 for cam in range(C)]]
    for m, views in ((mask, [v[0], v[0], v[2], v[3]]), (None, v), (mask, [v[0], v[3], v[2], v[3]])):
        got = pred.forward_images(views, *dev, camera_mask=m, return_2d=True)
        want = ref.forward_batch(cuda(x.unsqueeze(0)), *dev, camera_mask=m, return_2d=True)
        torch.cuda.synchronize()
        assert len(got) == len(want) == 4 and int(want[2][0]) == 1
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(_bits(a), _bits(b)), m
        assert len(want[3]._fields) == 5
        for f in want[3]._fields:                               # NaNs compared bitwise
            assert torch.equal(_bits(getattr(got[3], f)), _bits(getattr(want[3], f))), (m, f)
        assert int(want[3].used.sum()) == (C - 1 if m else C)


def test_medium_models_co32_stem(rig):
    """CenterDetect / KeypointDetect `medium` at the same geometry: the 32-channel stem."""
    c3 = cases.PREDICTOR_CASES["cfg3_medium"]
    seeds = (c3["cseed"], c3["hseed"])
    ref, pred = eager(eager(predictor(rig, "medium", seeds), 1), 2), predictor(rig, "medium", seeds)
    dev, C = rig["dev"], rig["C"]
    a, b = rig["frames"]["bgr"]
    want = clone(ref.forward_batch(cuda(a.unsqueeze(0)), *dev))
    same(pred.forward_images(scatter(list(a)), *dev), want, "medium T=1")
    want2 = clone(ref.forward_batch(cuda(torch.stack([a, b])), *dev))
    views = scatter(list(a) + list(b), 1)
    same(pred.forward_images([views[:C], views[C:]], *dev), want2, "medium T=2")
    assert not torch.equal(want2[0][0], want2[0][1])


def test_predictor2d():
    from jarvis_hybridnet_amd.prediction.jarvis2D import JarvisPredictor2D
    c = cases.PREDICTOR2D_CASES["cam0_j12"]
    ins = [cases.predictor2d_inputs(t) for t in ("cam0_j12", "cam2_j12")]
    cfg = make_cfg(dict(J=c["J"], bbox=c["bbox"], C=1, roi=32, spacing=2), c["center_size"])
    pred = JarvisPredictor2D(cfg, ins[0]["sd_center"], ins[0]["sd_kp"])
    imgs = torch.cat([ins[0]["img"], ins[1]["img"], torch.roll(ins[0]["img"], (24, -40), dims=(2, 3))])
    bgr = to_bgr_u8(imgs)                                                      # (3, H, W, 3)
    assert bgr.shape[1:3] == (H, W)
    s = SensorSurface(H, W, "grbg", pitch=W + 64, offset=33)
    raw = torch.from_numpy(S.pack_sensor_surface(S.mosaic(bgr, "grbg"), s, 0xA5))
    for x, kw in ((torch.from_numpy(bgr), {}), (raw, dict(frame_layout=s))):
        want = clone(pred.forward_batch(cuda(x), **kw))
        torch.cuda.synchronize()
        assert int(want[2][:2].sum()) == 2
        same(pred.forward_images(scatter(list(x)), **kw), want, sorted(kw))
        same(pred.forward_images(separate(list(x))[::-1], **kw), [t.flip(0) for t in want], (sorted(kw), "reversed"))


def test_error_codes_through_the_library(rig):
    from jarvis_hybridnet_amd import _native as N
    pred, ref = rig["pred"], rig["ref"]
    dev, C = rig["dev"], rig["C"]
    nat = pred.native(H, W)
    nat.set_calibration(*dev)
    out = (torch.empty((1, rig["c"]["J"], 3), device="cuda"), torch.empty((1, rig["c"]["J"]), device="cuda"),
           torch.empty((1,), device="cuda", dtype=torch.int32))
    u8, f32 = rig["frames"]["bgr"][0], rig["frames"]["fp32"][0]
    want = {"bgr": clone(ref.forward_batch(cuda(u8.unsqueeze(0)), *dev)),
            "fp32": clone(ref.forward_batch(cuda(f32.unsqueeze(0)), *dev))}
    vu8, vf32 = scatter(list(u8)), scatter(list(f32))

    def call(ptrs, fmt, yuv=None, sensor=None, n=None):
        table = (N.c_void_p * len(ptrs))(*ptrs)
        return N.lib().jh_predictor_forward_images(nat.handle, table, len(ptrs) if n is None else n, fmt, yuv, sensor,
                                                   None, *(N.ptr(t) for t in out), N.stream())

    pu8, pf32 = [t.data_ptr() for t in vu8], [t.data_ptr() for t in vf32]
    surf = YuvSurface(H, W, "nv12").struct()
    bad = [("null entry", lambda: call(pu8[:2] + [None] + pu8[3:], 1), "null image pointer"),
           ("misaligned fp32", lambda: call([pf32[0] + 2] + pf32[1:], 0), "4-byte aligned"),
           ("surface without a description", lambda: call(pu8, N.FRAME_SURFACE), "jh_yuv_surface"),
           ("a description the format does not take", lambda: call(pu8, 1, yuv=surf), "jh_yuv_surface"),
           ("count", lambda: call(pu8, 1, n=C - 1), "n_images")]
    for what, f, msg in bad:
        assert f() != 0, what
        assert msg in N.lib().jh_last_error().decode(), (what, N.lib().jh_last_error())
        for name, views in (("bgr", vu8), ("fp32", vf32)):
            same(pred.forward_images(views, *dev), want[name], ("after", what, name))
    assert int(want["bgr"][2][0]) == 1 and int(want["fp32"][2][0]) == 1
