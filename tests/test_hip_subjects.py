"""GPU: several subjects per frame set -- the peak kernel and the association kernel against the numpy reference of their
definitions (tests/subjects_ref.py), jh_predictor_detect_subjects against the two operators and against itself over the
frame forms, and forward_subjects against the centred forward_batch.  On cfg2 (tests/cases.py: 4 cameras 640 x 512,
center_size 256: heat maps 128 x 128, sx2 = 5, sy2 = 4 full-frame pixels per heat-map pixel).

Bounds.  Peaks: exact (bits of (x, y, value) and the counts).  Association: views and members exact; every non-empty
centre bit-equal to jh_reconstruct_point (pinned by tests/test_hip_geometry_ops.py) on the members' pixels and
value / 255 -- the weight the triangulation gives a detection, formed here by the same IEEE division --; error within
1e-3 px of the float64 reference (fp32 projections of coordinates below 1024 px round at 6e-5 px per operation).  The
scenes' peaks are
projections rounded to the grid, at most sqrt(2.5^2 + 2^2) = 3.2 px <= sx2 / sqrt(2) off; max_error_px is 3 sx2 / sqrt(2).
The reference asserts, before anything is compared, that no choice of a round, no support decision and no nearest peak
lies within 1e-2 px of a tie.  Everything here calls a symbol the feature adds."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import subjects_ref as R
from tests import test_hip_centers as HC
from tests.gpu_util import cuda, report

pytestmark = pytest.mark.gpu

INF = float("inf")
SX2, SY2 = 5.0, 4.0
TOL = 3 * SX2 / math.sqrt(2)
same = HC.same


def params(K=1, P=1, r=4, min_views=2, min_peak=50.0, max_error_px=24.0):
    from jarvis_hybridnet_amd import _native as N
    return N.SubjectsParamsStruct(K, P, r, min_views, min_peak, max_error_px)


def center_peaks(heat, P, r, min_peak):
    """jh_op_center_peaks on heat (N,Hh,Wh,Cp) device -> peaks (N,P,3), count (N,) on the host."""
    from jarvis_hybridnet_amd import _native as N
    n, hh, wh, cp = heat.shape
    peaks = torch.empty((n, P, 3), device="cuda")
    count = torch.empty((n,), device="cuda", dtype=torch.int32)
    N.check(N.lib().jh_op_center_peaks(N.ptr(heat), n, hh, wh, cp, ctypes.byref(params(1, P, r, 2, min_peak)),
                                       N.ptr(peaks), N.ptr(count), N.stream()))
    return peaks.cpu(), count.cpu()


def associate(peaks, calib, per_frame, mask, p):
    """jh_op_associate_subjects on peaks (T,C,P,3) device -> Subjects-like tuple of device tensors."""
    from jarvis_hybridnet_amd import _native as N
    T, C = peaks.shape[:2]
    K = p.max_subjects
    out = (torch.empty((T, K, 3), device="cuda"), torch.empty((T, K), device="cuda", dtype=torch.int32),
           torch.empty((T, K, C), device="cuda", dtype=torch.int32), torch.empty((T, K), device="cuda"))
    N.check(N.lib().jh_op_associate_subjects(N.ptr(peaks), T, C, *(N.ptr(t) for t in calib), int(per_frame),
                                             N.ptr(mask), SX2, SY2, ctypes.byref(p), *(N.ptr(t) for t in out),
                                             N.stream()))
    return out


def reconstruct(px, py, w, calib):
    """jh_reconstruct_point on n observations (pixels, weights) under calib = three (n,..) device tensors -> (3,) host."""
    from jarvis_hybridnet_amd import _native as N
    n = len(px)
    pts = cuda(torch.stack([px, py]).float())
    wt = cuda(w.float())
    out = torch.empty((3,), device="cuda")
    nb = N.lib().jh_reconstruct_workspace_bytes(n)
    ws = N.workspace(nb, out.device)
    N.check(N.lib().jh_reconstruct_point(N.ptr(pts), N.ptr(wt), n, *(N.ptr(t) for t in calib), N.ptr(out), N.ptr(ws),
                                         nb, N.stream()))
    torch.cuda.synchronize()
    return out.cpu()


# ---- 1: the peak kernel -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def peak_maps(hh, wh):
    """Channel-0 maps (N,hh,wh) float32 on the host: small integers (plateaus and ties everywhere), peaks on the four
    borders and corners, a constant map, NaN and -inf pixels among integers, and plain random floats."""
    g = np.random.RandomState(1000 * hh + wh)
    ints = g.randint(0, 4, (hh, wh)).astype(np.float32)
    border = np.zeros((hh, wh), np.float32)
    for y, x, v in ((0, 0, 9), (0, wh - 1, 8), (hh - 1, 0, 7), (hh - 1, wh - 1, 6), (0, wh // 2, 5), (hh // 2, 0, 5),
                    (hh - 1, wh // 2 + 1, 4), (hh // 2 + 1, wh - 1, 3), (hh // 2, wh // 2, 2)):
        border[y, x] = v
    const = np.full((hh, wh), 3.0, np.float32)
    holes = g.randint(-2, 3, (hh, wh)).astype(np.float32)
    holes[g.rand(hh, wh) < 0.1] = np.nan
    holes[g.rand(hh, wh) < 0.1] = -np.inf
    holes[holes == 0] *= np.where(g.rand(hh, wh) < 0.5, -1.0, 1.0)[holes == 0]     # (both signs of zero)
    rand = (g.randn(hh, wh) * 30).astype(np.float32)
    return np.stack([ints, border, const, holes, rand])


# 24 and 40: one LDS allocation below 64 KB; 20 x 36: not square (x = p % hh, y = p / wh as the arg-max has it);
# 160: the largest map that fits the LDS (above 64 KB); 224: the global-memory form
@pytest.mark.parametrize("hh,wh,r,P", [(24, 24, 1, 1), (24, 24, 3, 4), (40, 40, 1, 4), (40, 40, 3, 1), (20, 36, 3, 4),
                                       (160, 160, 3, 4), (224, 224, 1, 4), (224, 224, 3, 1)])
def test_peaks_equal_the_reference(hh, wh, r, P):
    maps = peak_maps(hh, wh)
    heat = torch.from_numpy(maps)[..., None].repeat(1, 1, 1, 8).contiguous()
    heat[..., 1:] = heat[..., :1].nan_to_num(0.0, 0.0, 0.0) + 100.0       # (a stride error reads a larger value)
    for min_peak in (-INF, 0.5):
        want_p, want_n = R.peaks_ref(maps, P, r, min_peak)
        got_p, got_n = center_peaks(cuda(heat), P, r, min_peak)
        assert got_n.tolist() == want_n.tolist(), (min_peak, got_n.tolist(), want_n.tolist())
        assert np.array_equal(got_p.numpy().view(np.int32), want_p.view(np.int32)), min_peak
    assert want_n[2] == 1 and want_n[0] >= min(P, 2)       # (the constant map has one peak; the integer map many)


# ---- the cfg2 predictor and frames, shared with tests/test_hip_centers.py
def frames_f32(T):
    return cuda(HC.setup()[4][:T])


@functools.lru_cache(maxsize=None)
def detected(T, u8=False):
    """det and the results of a detected forward_batch of the first T frame sets."""
    c, inp, pred, calib, frames = HC.setup()
    x = cuda(HC.to_u8(frames[:T])) if u8 else frames_f32(T)
    res = pred.forward_batch(x, *calib)
    det = pred.native(c["H"], c["W"], time_batch=T).debug("cuda")["det"]
    torch.cuda.synchronize()
    return x, tuple(t.clone() for t in res), det.clone()


def detect(x, T, **kw):
    c, inp, pred, calib, _ = HC.setup()
    kw.setdefault("return_peaks", True)
    out = pred.detect_subjects(x, *kw.pop("calib", calib), kw.pop("K", 2), **kw)
    torch.cuda.synchronize()
    return out


def same_subjects(a, b):
    return all(same(x, y) for x, y in zip(a, b))


# ---- 2: slot 0 is the arg-max -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True])
def test_slot0_is_the_argmax(u8):
    x, _, det = detected(4, u8)
    _, peaks = detect(x, 4, K=1, max_peaks=1, min_peak=-INF)
    assert peaks.shape == (4, 4, 1, 3)
    assert same(peaks[:, :, 0], det)


# ---- 3: the association kernel ----------------------------------------------------------------------------------------
PTS = [(60.0, -40.0, 20.0), (-120.0, 90.0, -30.0), (40.0, 150.0, 60.0)]          # >= 150 mm apart
VALS = (200.0, 150.0, 120.0)


@functools.lru_cache(maxsize=None)
def scenes():
    """Two frame sets with a calibration each (sets A and D of tests/test_hip_calibration_frames.py: D has k1, k2
    halved), P = 4 slots.  Row 0: two subjects, the second hidden from camera 2, and in camera 1 a distractor with the
    highest value.  Row 1: three subjects, the third hidden from camera 0, camera 3 masked and full of NaN, a
    distractor in camera 2."""
    c, inp, _, _, _ = HC.setup()
    sets = HC.derived_sets(inp["cam"], inp["intr"], inp["dist"])
    row0 = R.scene_peaks(sets["A"], PTS[:2], VALS, SX2, SY2, 4, hidden={(2, 1)}, extra=[(1, 100, 20, 250.0)])
    row1 = R.scene_peaks(sets["D"], PTS, VALS, SX2, SY2, 4, hidden={(0, 2)}, extra=[(2, 15, 110, 250.0)])
    row1[3] = np.nan
    peaks = np.stack([row0, row1])
    mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0]], np.uint8)
    calib = tuple(torch.stack([sets["A"][i], sets["D"][i]]) for i in range(3))
    return peaks, mask, calib


def check_against_reference(peaks, mask, calib, per_frame, K, min_views, rows):
    """The operator on `rows` of the scenes against the reference and jh_reconstruct_point."""
    T = len(rows)
    p = params(K, 4, 4, min_views, 50.0, TOL)
    dev_calib = tuple(cuda(t[rows] if per_frame else t[rows[0]]) for t in calib)
    ctr, views, mem, err = (t.cpu() for t in associate(cuda(torch.from_numpy(peaks[rows])), dev_calib, per_frame,
                                                       cuda(torch.from_numpy(mask[rows])), p))
    worst = 0.0
    for i, t in enumerate(rows):
        cal = tuple(a[t] for a in calib)
        w_ctr, w_views, w_mem, w_err = R.associate_ref(peaks[t], *(a.numpy() for a in cal), mask[t], SX2, SY2, K, TOL,
                                                      min_views, margin=1e-2)
        assert views[i].tolist() == w_views.tolist() and mem[i].tolist() == w_mem.tolist(), (t, views[i], mem[i])
        for k in range(K):
            if w_views[k] == 0:
                assert torch.isnan(ctr[i, k]).all() and torch.isnan(err[i, k]) and mem[i, k].tolist() == [-1] * 4
                continue
            cams = [c for c in range(4) if w_mem[k][c] >= 0]
            pk = torch.from_numpy(np.stack([peaks[t, c, w_mem[k][c]] for c in cams]))
            want = reconstruct(pk[:, 0] * SX2, pk[:, 1] * SY2, pk[:, 2] / 255.0, tuple(cuda(a[cams]) for a in cal))
            assert same(ctr[i, k], want), (t, k, ctr[i, k], want)
            assert np.abs(want.numpy() - w_ctr[k]).max() < 1e-2           # (the float64 SVD agrees with the eigen-solve)
            worst = max(worst, abs(float(err[i, k]) - w_err[k]))
    assert worst < 1e-3, worst
    return ctr, views, mem, err, worst


def test_association_equals_the_reference():
    peaks, mask, calib = scenes()
    ctr, views, mem, err, worst = check_against_reference(peaks, mask, calib, True, 4, 2, [0, 1])
    report("subjects_association", error_vs_ref_px=worst)
    # row 0: the subject four cameras see comes first, then the one three see; K is larger than the scene
    assert views[0].tolist() == [4, 3, 0, 0]
    assert mem[0].tolist() == [[0, 1, 0, 0], [1, 2, -1, 1], [-1] * 4, [-1] * 4]       # (camera 1: slot 0 is the distractor)
    # row 1 under its own calibration: camera 3 masked; subjects 0 and 1 in three cameras, subject 2 in two
    assert views[1].tolist() == [3, 3, 2, 0] and mem[1, :, 3].tolist() == [-1] * 4
    for t, n in ((0, 2), (1, 3)):
        for k in range(n):
            assert (ctr[t, k] - torch.tensor(PTS[k])).abs().max() < 8      # (grid rounding: a few millimetres)
    # three views required: the pair-only subject of row 1 is not reported
    _, views3, _, _, _ = check_against_reference(peaks, mask, calib, True, 4, 3, [0, 1])
    assert views3.tolist() == [[4, 3, 0, 0], [3, 3, 0, 0]]
    # the shared-calibration form, one row, fewer subjects asked for than there are
    _, views1, _, _, _ = check_against_reference(peaks, mask, calib, False, 1, 2, [0])
    assert views1.tolist() == [[4]]
    # row t under per-frame-set calibration equals the row alone under its calibration shared, bit for bit
    both = associate(cuda(torch.from_numpy(peaks)), tuple(cuda(t) for t in calib), True, cuda(torch.from_numpy(mask)),
                     params(4, 4, 4, 2, 50.0, TOL))
    for t in (0, 1):
        alone = associate(cuda(torch.from_numpy(peaks[t:t + 1])), tuple(cuda(a[t]) for a in calib), False,
                          cuda(torch.from_numpy(mask[t:t + 1])), params(4, 4, 4, 2, 50.0, TOL))
        assert all(same(a[t:t + 1], b) for a, b in zip(both, alone)), t


# ---- 4: the predictor call --------------------------------------------------------------------------------------------
KW = dict(K=2, max_peaks=3, nms_radius=4, min_peak=-INF, max_error_px=40.0)


@functools.lru_cache(maxsize=None)
def detected_subjects(T=4):
    return detect(frames_f32(T), T, **KW)


def test_detect_subjects_equals_the_operators():
    c, inp, pred, calib, frames = HC.setup()
    subj, peaks = detected_subjects()
    want = associate(peaks, calib, False, None, params(2, 3, 4, 2, -INF, 40.0))
    torch.cuda.synchronize()
    assert same_subjects(subj, want)
    assert int(subj.views[:, 0].min()) >= 2           # (the comparison is not of empty results)
    # an all-ones mask is no mask
    assert same_subjects(detect(frames_f32(4), 4, camera_mask=torch.ones(4, 4, dtype=torch.bool), **KW)[0], subj)
    # per-image pointers
    x = frames_f32(4)
    imgs = [[x[t, cam].clone() for cam in range(4)] for t in range(4)]
    got = detect(imgs, 4, images=True, **KW)
    assert same_subjects(got[0], subj) and same(got[1], peaks)


def test_detect_subjects_masked_slot_and_yuv():
    from jarvis_hybridnet_amd import synthetic as S
    from tests.test_yuv_ingest_cpu import yuv420_to_bgr
    c, inp, pred, calib, frames = HC.setup()
    u8 = HC.to_u8(frames[:4])
    mask = torch.ones(4, 4, dtype=torch.uint8)
    mask[1, 2] = mask[3, 0] = 0
    base = detect(cuda(u8), 4, camera_mask=mask, **KW)
    assert base[0].members[1, :, 2].tolist() == [-1, -1] and base[0].members[3, :, 0].tolist() == [-1, -1]
    junk = u8.clone()
    junk[1, 2] = junk[3, 0] = 0xFF
    got = detect(cuda(junk), 4, camera_mask=mask, **KW)
    assert same_subjects(got[0], base[0])               # (the masked slot's bytes reach no result)
    # NV12 frames against the uint8 call on the bytes the contract converts them to
    yuv = S.bgr_to_yuv420(u8.reshape(16, c["H"], c["W"], 3).numpy(), "nv12")
    bgr = torch.from_numpy(yuv420_to_bgr(yuv, "nv12")).reshape(4, 4, c["H"], c["W"], 3)
    a = detect(cuda(torch.from_numpy(yuv).reshape(4, 4, c["H"] * 3 // 2, c["W"])), 4, frame_format="nv12", **KW)
    b = detect(cuda(bgr), 4, **KW)
    assert same_subjects(a[0], b[0]) and same(a[1], b[1])


def test_detect_subjects_per_frame_calibration():
    c, inp, pred, calib, frames = HC.setup()
    sets = HC.derived_sets(inp["cam"], inp["intr"], inp["dist"])
    order = ("A", "B", "D", "B")
    per = tuple(cuda(torch.stack([sets[k][i] for k in order])) for i in range(3))
    x = frames_f32(4)
    got, peaks = detect(x, 4, calib=per, **KW)
    assert same(peaks, detected_subjects()[1])          # (the heat maps do not depend on the calibration)
    for k in set(order):
        shared = detect(x, 4, calib=tuple(cuda(t) for t in sets[k]), **KW)[0]
        for t in (t for t in range(4) if order[t] == k):
            assert all(same(a[t], b[t]) for a, b in zip(got, shared)), (k, t)
    detect(x, 4, **KW)                                  # (back to the shared calibration of the other tests)


def test_forwards_around_the_call_keep_their_bits():
    c, inp, pred, calib, frames = HC.setup()
    for T in (1, 4):
        pr = pred.native(c["H"], c["W"], time_batch=T)
        assert pr.graph_replay == (T == 1)
        x, before, det = detected(T)
        bytes_before = pr.device_bytes
        detect(x, T, **KW)
        after = pred.forward_batch(x, *calib)
        dbg = pr.debug("cuda")
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(after, before)) and same(dbg["det"], det)
        from jarvis_hybridnet_amd import _native as N
        assert N.lib().jh_predictor_device_bytes(pr.handle) == bytes_before


# ---- 5: end to end ----------------------------------------------------------------------------------------------------
def test_forward_subjects_rows_are_centred_forwards():
    c, inp, pred, calib, frames = HC.setup()
    x = frames_f32(8)
    kw = dict(max_peaks=2, min_peak=-INF, max_error_px=INF)
    pts, conf, valid, subj = pred.forward_subjects(x, *calib, 3, **kw)
    torch.cuda.synchronize()
    assert pts.shape == (8, 3, c["J"], 3) and conf.shape == (8, 3, c["J"]) and valid.shape == (8, 3)
    assert same_subjects(subj, pred.detect_subjects(x, *calib, 3, **kw))
    rows = 0
    for k in range(3):
        want = pred.forward_batch(x, *calib, centers=subj.centers[:, k])
        torch.cuda.synchronize()
        assert same(valid[:, k], want[2])
        for t in range(8):
            if int(subj.views[t, k]) == 0:             # an empty subject: NaN centre, an invalid row
                assert torch.isnan(subj.centers[t, k]).all() and int(valid[t, k]) == 0
                continue
            assert int(valid[t, k]) == 1
            assert same(pts[t, k], want[0][t]) and same(conf[t, k], want[1][t]), (t, k)
            rows += k == 0
    # two peaks per camera cannot give a third subject; at most 2 of the 8 frame sets may lack a first one
    assert int(subj.views[:, 2].max()) == 0 and int(valid[:, 2].max()) == 0
    assert rows >= 6, rows


# ---- 6: misuse --------------------------------------------------------------------------------------------------------
def test_misuse_raises_and_enqueues_nothing():
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, frames = HC.setup()
    x, before, det = detected(4)
    pr = pred.native(c["H"], c["W"], time_batch=4)
    fr = pr._describe(x)
    good = N.subjects_params(2)
    for field, value in (("max_subjects", 9), ("max_peaks", 0), ("nms_radius", 17), ("min_views", 1),
                         ("min_peak", float("nan")), ("max_error_px", -1.0)):
        bad = N.SubjectsParamsStruct.from_buffer_copy(good)
        setattr(bad, field, value)
        with pytest.raises(RuntimeError, match="jh_subjects_params"):
            pr.detect_subjects(fr, bad)
    with pytest.raises(ValueError):
        pred.detect_subjects(x, *calib, 0)
    no_center = HC.native(4, center=False)
    with pytest.raises(RuntimeError, match="without CenterDetect weights"):
        no_center.detect_subjects(no_center._describe(x), good)
    no_center.close()
    shard = HC.native(4, cam_lo=0, cam_n=2)
    with pytest.raises(RuntimeError, match="all cameras local"):
        shard.detect_subjects(shard._describe(x[:, :2].contiguous()), good)
    shard.close()
    after = pred.forward_batch(x, *calib)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(after, before))
