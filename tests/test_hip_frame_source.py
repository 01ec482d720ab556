"""GPU: every frame source on ONE graph-replaying predictor.  The two described kinds (YuvSurface, SensorSurface) share
the re-record logic of the fixed formats' graph slots: a slot keeps the source it was recorded with, and a call with
another description of the same kind records again.  Alternating all of them, unmasked and masked, every call equals
the uint8 BGR path on the bytes its own description converts to -- a stale recording would read another layout, matrix
or Bayer pattern."""
import pytest
import torch

from jarvis_hybridnet_amd import SensorSurface, YuvSurface
from jarvis_hybridnet_amd import synthetic as S
from tests import cases
from tests.gpu_util import cuda
from tests.test_hip_yuv_ingest import to_bgr_u8, yuv_and_reference
from tests.test_hip_yuv_surface import surface_frames

pytestmark = pytest.mark.gpu

SEQUENCE = ("bgr", "A", "rggb", "B", "rggb", "bggr", "A", "nv12", "bgr")


def test_sources_alternate_under_replay():
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    H, W, C = c["H"], c["W"], c["C"]
    assert (H, W) == (512, 640)
    kw = dict(num_cameras=C, num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN, std=S.STD, time_batch=1)
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]
    bgr = to_bgr_u8(inp["imgs"])
    A = YuvSurface(H, W, "nv12", matrix="bt709", y_pitch=768, c_pitch=768)
    B = YuvSurface(H, W, "yv12", range="full")
    raw = S.mosaic(bgr, "rggb")                              # the SAME bytes are read as rggb and as bggr
    raw_t = torch.from_numpy(raw.reshape(raw.shape[0], -1))
    # name -> (frames, how forward() is told what they are, the BGR bytes they convert to)
    src = {"bgr": (torch.from_numpy(bgr), {}, torch.from_numpy(bgr))}
    for name, s in (("A", A), ("B", B)):
        x, ref = surface_frames(bgr, s)
        src[name] = (x, dict(frame_layout=s), ref)
    for p in ("rggb", "bggr"):
        src[p] = (raw_t, dict(frame_layout=SensorSurface(H, W, p)), torch.from_numpy(S.sensor_to_bgr(raw, p)))
    x, ref = yuv_and_reference(bgr, "nv12")
    src["nv12"] = (x, dict(frame_format="nv12"), ref)
    src = {k: (cuda(x).unsqueeze(0), how, cuda(ref).unsqueeze(0)) for k, (x, how, ref) in src.items()}

    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert g.graph_replay
    g.set_calibration(*dev)
    eager = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    eager.graph_replay = False
    assert not eager.graph_replay
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
        assert not torch.equal(first["A"][0], first["B"][0])
        assert not torch.equal(first["rggb"][0], first["bggr"][0])
    g.close()
    eager.close()


def test_forward_forms_combine_under_replay():
    """All 16 combinations of (masked, per-image, centred, spread) on ONE graph-replaying predictor, each visited twice
    and never twice in a row, the input alternating between two frame sets from call to call: every call equals the
    eager predictor's call of the same form on the same input.  The alternation tests above vary one flag at a time; two
    forms that shared a graph slot would show only here, as a recording replayed for the other form."""
    import itertools

    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    H, W, C = c["H"], c["W"], c["C"]
    kw = dict(num_cameras=C, num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN, std=S.STD, time_batch=1)
    dev = [cuda(inp[k]) for k in ("cam", "intr", "dist")]
    x = torch.from_numpy(to_bgr_u8(inp["imgs"]))
    y = torch.where(x < 128, x + 6, x - 6)                       # every pixel value moves by 6, none wraps
    contig = {"X": cuda(x).unsqueeze(0), "Y": cuda(y).unsqueeze(0)}
    views = {k: [cuda(img).clone() for img in v] for k, v in (("X", x), ("Y", y))}   # one allocation per image
    mask = [[cam != 1 for cam in range(C)]]

    g = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    eager = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    eager.graph_replay = False
    assert g.graph_replay and not eager.graph_replay
    for p in (g, eager):
        p.set_calibration(*dev)
    eager.forward(contig["X"])
    # centres that are NOT the detected ones: three, two and two voxels (2 mm each) off
    centres = eager.debug(contig["X"].device)["center3d"] + torch.tensor([6., -4., 4.], device="cuda")

    def run(p, name, form):
        masked, per_image, centred, spread = form
        how = dict(camera_mask=mask if masked else None, centers=centres if centred else None, return_spread=spread)
        out = p.forward_images(N.frame_images(views[name], C), **how) if per_image else p.forward(contig[name], **how)
        assert len(out) == (4 if spread else 3)
        return [t.clone() for t in out[:3]] + [t.clone() for t in (out[3] if spread else ())]

    forms = list(itertools.product((False, True), repeat=4))
    want = {(name, f): run(eager, name, f) for name in "XY" for f in forms}
    torch.cuda.synchronize()

    def differ(a, b):
        return any(not torch.equal(s, t) for s, t in zip(a, b))
    plain = (False, False, False, False)
    assert differ(want["X", plain], want["Y", plain])
    assert differ(want["X", plain], want["X", (True, False, False, False)])      # masked
    assert differ(want["X", plain], want["X", (False, False, True, False)])      # centred

    # second pass: another order (7 i + 3 is odd where i is even: every form meets the other input there)
    order = forms + [forms[(7 * i + 3) % 16] for i in range(16)]
    assert all(a != b for a, b in zip(order, order[1:])) and all(order.count(f) == 2 for f in forms)
    for step, f in enumerate(order):
        name = "XY"[step % 2]
        got = run(g, name, f)
        torch.cuda.synchronize()
        assert len(got) == len(want[name, f]) == (6 if f[3] else 3)
        for a, b in zip(got, want[name, f]):
            assert torch.equal(a, b), (step, name, f)
        assert int(got[2][0]) == 1, (step, name, f)
    g.close()
    eager.close()
