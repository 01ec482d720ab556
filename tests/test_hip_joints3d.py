"""GPU: per-joint robust triangulation -- the refinement kernel against its float32 emulation, the consensus kernel
against the numpy reference of its definition (tests/joints3d_ref.py), jh_predictor_triangulate_joints against the two
operators, against heat maps whose answer is known, and against itself over the call forms.  The predictor tests run on
cfg2 (tests/cases.py: 4 cameras 640 x 512, crops of 256: heat maps 128 x 128 with 23 joints in 24 channels).

Bounds.  Offsets and observations: exact (bits).  Consensus: views and members exact; every non-empty point bit-equal to
jh_reconstruct_point (pinned by tests/test_hip_geometry_ops.py) on the members' pixels and weights; error within 1e-3 px
of the float64 reference (fp32 projections of coordinates below 1024 px round at 6e-5 px per operation, the bound
tests/test_hip_subjects.py derives); the float64 SVD and the fp64 eigen-solve agree within 1e-2 mm.  The reference
asserts, before anything is compared and over every candidate pair, that no support distance lies within 1e-2 px of
max_error_px and that no choice rests on a cost difference below 1e-2 px; the scenes' seeds are fixed and were chosen on
the CPU so that this holds on every case (nothing is skipped at run time).  Everything here calls a symbol the feature
adds."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import joints3d_ref as JR
from tests import test_hip_centers as HC
from tests.gpu_util import cuda, report

pytestmark = pytest.mark.gpu

INF = float("inf")
MAX_ERR = 6.0
# For the cfg2 predictor's own heat maps: its weights are random, so its cameras' keypoints need not agree within any
# bound; without the bounds every camera with a positive maximum in front of which the pair's point lies is a member.
WIDE = dict(max_error_px=INF, min_conf=0.0)
same = HC.same


def jparams(min_views=2, refine_radius=1, min_conf=0.1, max_error_px=MAX_ERR):
    from jarvis_hybridnet_amd import _native as N
    return N.joints3d_params(min_views, refine_radius, min_conf, max_error_px)


def reconstruct(obs, calib):
    """jh_reconstruct_point on the observations obs (n,3) = (u, v, w) under calib = three (n,..) host arrays -> (3,)."""
    from tests.test_hip_subjects import reconstruct as rec
    o = torch.from_numpy(np.ascontiguousarray(obs))
    return rec(o[:, 0], o[:, 1], o[:, 2], tuple(cuda(torch.from_numpy(np.ascontiguousarray(a)).float()) for a in calib))


# ---- 1: the refinement kernel -----------------------------------------------------------------------------------------
def refine(heat, idx, r):
    """jh_op_joint_peaks_refine on heat (N,hh,wh,jp), idx (N,J) host arrays -> offsets (N,J,2) host."""
    from jarvis_hybridnet_amd import _native as N
    n, hh, wh, jp = heat.shape
    j = idx.shape[1]
    out = torch.full((n, j, 2), 7.0, device="cuda")
    heat_dev, idx_dev = cuda(torch.from_numpy(heat)), cuda(torch.from_numpy(idx))     # (alive across the call)
    N.check(N.lib().jh_op_joint_peaks_refine(N.ptr(heat_dev), n, hh, wh, jp, N.ptr(idx_dev), j, r, N.ptr(out),
                                             N.stream()))
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def refine_maps(hh, wh, jp, j):
    """Four images (4,hh,wh,jp) and their arg-max indices (4,j).  0: noise with one peak per channel, the peaks walking
    over the four corners, the four borders and the interior, with a sloped neighbourhood; 1: the same peaks among NaN
    and negative pixels; 2: constant non-positive maps (offset 0), even channels -1, odd channels 0; 3: image 0 again
    with indices outside the map in channels 0 and 1 (nothing is read, offset 0).  The padding channels j .. jp-1 hold
    1e4: a stride error reads a larger value."""
    g = np.random.RandomState(100 * hh + wh + jp)
    spots = [(0, 0), (0, wh - 1), (hh - 1, 0), (hh - 1, wh - 1), (0, wh // 2), (hh // 2, 0), (hh - 1, wh // 2 - 1),
             (hh // 2 + 1, wh - 1), (hh // 2, wh // 2), (1, 1), (hh - 2, wh - 2), (2, wh - 3)]
    heat = np.empty((4, hh, wh, jp), np.float32)
    heat[0] = g.uniform(0.0, 1.0, (hh, wh, jp))
    heat[1] = g.uniform(-2.0, 1.0, (hh, wh, jp))
    heat[1][g.rand(hh, wh, jp) < 0.2] = np.nan
    for k in range(j):
        y, x = spots[k % len(spots)]
        for n in (0, 1):
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    yy, xx = y + dy, x + dx
                    if (dy or dx) and 0 <= yy < hh and 0 <= xx < wh and g.rand() < 0.7:
                        heat[n, yy, xx, k] = g.uniform(2.0, 9.0) * (k + 1)
            heat[n, y, x, k] = 10.0 * (k + 1)
    heat[2, :, :, 0::2] = -1.0
    heat[2, :, :, 1::2] = 0.0
    heat[3] = heat[0]
    heat[..., j:] = 1e4
    with np.errstate(invalid="ignore"):
        idx = np.where(np.isnan(heat), -np.inf, heat).reshape(4, hh * wh, jp)[:, :, :j].argmax(1).astype(np.int32)
    idx[3, 0], idx[3, 1] = -1, hh * wh
    return heat, idx


@pytest.mark.parametrize("hh,wh", [(8, 8), (24, 24), (20, 36)])
@pytest.mark.parametrize("jp,j", [(8, 5), (24, 23)])
def test_refinement_equals_the_float32_emulation(hh, wh, jp, j):
    heat, idx = refine_maps(hh, wh, jp, j)
    assert idx[2].tolist() == [0] * j and (idx[0] == idx[1]).all()
    for r in (1, 2, 3):
        want = JR.refine_ref(heat, idx, r)
        got = refine(heat, idx, r)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (r, np.abs(got - want).max())
        assert (want[2] == 0).all() and (want[3, :2] == 0).all()
        assert np.abs(want[:2]).max() > 0.2 and np.abs(want).max() <= r          # (the comparison is not of zeros)
    assert (refine(heat, idx, 0) == 0).all()


# ---- 2: the consensus kernel ------------------------------------------------------------------------------------------
def triangulate(obs, calib, per_frame, p):
    """jh_op_triangulate_joints on obs (T,C,J,3) and calib = three host arrays -> four host arrays."""
    from jarvis_hybridnet_amd import _native as N
    T, C, J = obs.shape[:3]
    dev = tuple(cuda(torch.from_numpy(np.ascontiguousarray(a)).float()) for a in calib)
    out = (torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda", dtype=torch.int32),
           torch.empty((T, J, C), device="cuda", dtype=torch.uint8), torch.empty((T, J), device="cuda"))
    obs_dev = cuda(torch.from_numpy(np.ascontiguousarray(obs)))                        # (alive across the call)
    N.check(N.lib().jh_op_triangulate_joints(N.ptr(obs_dev), T, C, J, *(N.ptr(t) for t in dev),
                                             int(per_frame), ctypes.byref(p), *(N.ptr(t) for t in out), N.stream()))
    return tuple(t.cpu().numpy() for t in out)


def check_consensus(obs, calibs, per_frame, got, kw, margin):
    """The operator's four outputs against the reference and jh_reconstruct_point, joint by joint -> the worst error
    difference in px and the number of non-empty joints."""
    pts, views, mem, err = got
    T, C, J = obs.shape[:3]
    worst, full = 0.0, 0
    for t in range(T):
        f32 = [a.astype(np.float32) for a in calibs[t]]
        for j in range(J):
            w_pt, w_views, w_mem, w_err = JR.joint_ref(obs[t, :, j], *f32, margin=margin, **kw)
            assert views[t, j] == w_views and mem[t, j].tolist() == w_mem.tolist(), (t, j, views[t, j], mem[t, j], w_mem)
            if w_views == 0:
                assert np.isnan(pts[t, j]).all() and np.isnan(err[t, j]) and not mem[t, j].any(), (t, j)
                continue
            cams = np.flatnonzero(w_mem)
            want = reconstruct(obs[t, cams, j], [a[cams] for a in f32])
            assert same(torch.from_numpy(pts[t, j]), want), (t, j, pts[t, j], want)
            assert np.abs(pts[t, j] - w_pt).max() < 1e-2, (t, j)      # (the float64 SVD agrees with the eigen-solve)
            worst = max(worst, abs(float(err[t, j]) - w_err))
            full += 1
    assert worst < 1e-3, worst
    return worst, full


# (C, J, per frame set, the camera whose matrix is negated, seed): C = 2 .. 64; J = 1, 5, 23 -- 3, 15 and 69 waves in
# workgroups of four, so the last workgroup has idle waves
CONSENSUS_CASES = [(2, 1, False, None, 2001), (3, 5, True, None, 3005), (4, 23, False, None, 4023), (4, 5, True, 1, 4005),
                   (12, 5, True, 7, 12007), (12, 23, False, 3, 12128), (64, 1, False, 5, 64001)]


@pytest.mark.parametrize("C,J,per_frame,flip,seed", CONSENSUS_CASES)
def test_consensus_equals_the_reference(C, J, per_frame, flip, seed):
    T = 3
    calibs = JR.case_calibs(C, T, per_frame, flip)
    obs, truth, kind, out = JR.scenes(C, T, J, seed, calibs)
    calib = tuple(np.stack([c[i] for c in calibs]) if per_frame else calibs[0][i] for i in range(3))
    got = triangulate(obs, calib, per_frame, jparams())
    worst, full = check_consensus(obs, calibs, per_frame, got, dict(max_error_px=MAX_ERR), JR.MARGIN)
    report("joints3d_consensus", cameras=C, joints=J, error_vs_ref_px=worst)
    pts, views, mem, err = got
    for t in range(T):
        for j in range(J):
            back = [] if flip is None or (per_frame and t % 3 != 2) else [flip]
            left = sorted(set(out[t][j]) | set(back))
            if kind[t][j] == "too_few" or C - len(left) < 2:
                assert views[t, j] == 0, (t, j, kind[t][j])
                continue
            # the cameras that disagree, are below min_conf, unused or behind the point are left out; the others agree
            assert mem[t, j].tolist() == [0 if c in left else 1 for c in range(C)], (t, j, kind[t][j], mem[t, j])
            assert np.abs(pts[t, j] - truth[t, j]).max() < 4.0 and err[t, j] < 2.0, (t, j)
    assert full >= 1
    # two calls give the same bits
    again = triangulate(obs, calib, per_frame, jparams())
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))
    # min_views above what agrees: the joint is empty
    strict = triangulate(obs, calib, per_frame, jparams(min_views=C + 1))
    assert not strict[1].any() and not strict[2].any() and np.isnan(strict[0]).all() and np.isnan(strict[3]).all()
    # without the bounds: all usable cameras in front of which the point lies, and jh_reconstruct_point over them
    if C > 12:                       # (the reference of 2016 pairs takes seconds: the first frame set, not shared per frame)
        T, obs, calibs = 1, obs[:1], calibs[:1]
    wide = triangulate(obs, calib, per_frame, jparams(max_error_px=INF, min_conf=0.0))
    check_consensus(obs, calibs, per_frame, wide, dict(max_error_px=INF, min_conf=0.0), None)
    for t in range(T):
        back = None if flip is None or (per_frame and t % 3 != 2) else flip
        for j in range(J):
            ok = JR.usable(obs[t, :, j], 0.0)
            if back is not None:
                ok[back] = False
            assert wide[2][t, j].tolist() == (ok.astype(int).tolist() if ok.sum() >= 2 else [0] * C), (t, j)


# ---- 3: the predictor -------------------------------------------------------------------------------------------------
def as_host(tri):
    return type(tri)(*(t.cpu() for t in tri))


def same_tri(a, b, rows=slice(None)):
    return all(same(x[rows], y[rows]) for x, y in zip(a, b))


def test_predictor_r0_observations_are_the_2d_views():
    c, inp, pred, calib, frames = HC.setup()
    x = cuda(frames[:2])
    plain = pred.forward_batch(x, *calib, return_2d=True)
    plain_views = [t.clone() for t in plain[3]]
    plain = [t.clone() for t in plain[:3]]
    p = jparams(refine_radius=0, **WIDE)
    pts, conf, valid, views, tri = pred.forward_batch(x, *calib, return_2d=True, return_triangulated=p)
    torch.cuda.synchronize()
    # the forward keeps its bits, and the tuple stands behind Views2D
    assert all(same(a, b) for a, b in zip(plain, (pts, conf, valid))) and valid.tolist() == [1, 1]
    # ... Views2D too, all five tensors -- also when asked again BEHIND the triangulation, whose scan went through the
    # workspace the 2D views share
    assert len(views) == 5 and all(same(a, b) for a, b in zip(plain_views, views))
    behind = pred.native(c["H"], c["W"], time_batch=2).views2d(pts)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(plain_views, behind))
    assert type(tri).__name__ == "Triangulated3D" and tri.observations.shape == (2, c["C"], c["J"], 3)
    assert tri.members.dtype == torch.uint8 and tri.views.dtype == torch.int32
    assert same(tri.observations[..., :2], views.points2D.float()) and same(tri.observations[..., 2], views.confidences2D)
    # ... and the result is the operator's on those observations
    got = triangulate(tri.observations.cpu().numpy(), tuple(t.cpu().numpy() for t in calib), False, p)
    for a, b in zip(as_host(tri)[:4], got):
        assert same(a, torch.from_numpy(b))
    assert int(tri.views.min()) >= 0 and int(tri.views.max()) >= 2         # (the comparison is not of empty results)
    # True means the library's defaults
    a = pred.forward_batch(x, *calib, return_triangulated=True)[3]
    b = pred.forward_batch(x, *calib, return_triangulated=jparams(2, 1, 0.1, 8.0))[3]
    torch.cuda.synchronize()
    assert same_tri(a, b)


HEAT_SEED = 5000
FALSE_PEAK = (0, 2, 3)                   # (frame set, camera, joint) that gets a higher peak somewhere else


def heat_scene(chm, centres, calib, J, Jp, Hh, seed=HEAT_SEED):
    """Heat maps (T,C,Hh,Hh,Jp) float32 whose answer is known: joint j of frame set t is a 3D point within +-60 mm of
    centres[t]; every camera's map holds a Gaussian blob (tests/joints3d_ref.py: blob) at its projection (float64), in
    the heat-map coordinates of the crop around chm[t][c].  FALSE_PEAK's map has a higher value far from its blob.  The
    padding channel holds 1e4.  -> heat, the points (T,J,3)."""
    g = np.random.RandomState(seed)
    T, C = chm.shape[:2]
    heat = np.zeros((T, C, Hh, Hh, Jp), np.float32)
    truth = np.asarray(centres, np.float64)[:, None, :] + g.uniform(-60.0, 60.0, (T, J, 3))
    for t in range(T):
        for j in range(J):
            uv, _ = JR.R.project64(truth[t, j], *calib)
            for cam in range(C):
                hx, hy = (uv[cam] - chm[t, cam] + Hh) / 2.0
                assert 4 < hx < Hh - 4 and 4 < hy < Hh - 4
                heat[t, cam, :, :, j] = JR.blob(Hh, Hh, hx, hy)
    t, cam, j = FALSE_PEAK
    heat[t, cam, 10, 100, j] = 250.0
    heat[..., J:] = 1e4
    return heat, truth


def observations_of(heat, chm, J, Hh, r):
    """The observations (T,C,J,3) the definition gives for heat maps under the crop centres chm, all cameras used."""
    T, C = heat.shape[:2]
    maps = heat.reshape(T * C, Hh, Hh, -1)
    flat = maps.reshape(T * C, Hh * Hh, -1)[:, :, :J]
    idx = flat.argmax(1).astype(np.int32)
    p2d = np.stack([(idx % Hh) * 2, (idx // Hh) * 2], -1) + chm.reshape(T * C, 1, 2) - Hh
    conf = np.minimum(flat.max(1), np.float32(255)) / np.float32(255)
    return JR.observations_ref(p2d, conf, JR.refine_ref(maps, idx, r)).reshape(T, C, J, 3)


@functools.lru_cache(maxsize=None)
def centred():
    """forward_batch of frame sets 0 and 1 from the centres K1 and K2 of tests/test_hip_centers.py, whose crop centres
    are that file's table: the heat-map scene is known without a GPU."""
    c, inp, pred, calib, frames = HC.setup()
    table, _ = HC.centres()
    centres = torch.stack([table["K1"][0], table["K2"][0]])
    chm = np.array([HC.TABLE["K1"][1], HC.TABLE["K2"][1]])
    res = [t.clone() for t in pred.forward_batch(cuda(frames[:2]), *calib, centers=centres)]
    pr = pred.native(c["H"], c["W"], time_batch=2)
    assert pr.debug("cuda")["center_hm"].cpu().tolist() == chm.tolist() and res[2].tolist() == [1, 1]
    calib64 = tuple(inp[k].double().numpy() for k in HC.KEYS)
    heat, truth = heat_scene(chm, centres.numpy(), calib64, c["J"], pr.Jp, pr.Hh)
    return pr, centres, chm, calib64, heat, truth, res


def test_predictor_known_heat_maps():
    c, inp, pred, calib, frames = HC.setup()
    pr, centres, chm, calib64, heat, truth, _ = centred()
    dev = cuda(torch.from_numpy(heat))
    dist = {}
    for r in (0, 1):
        tri = as_host(pr.triangulate_joints(heat=dev, params=jparams(refine_radius=r)))
        obs = tri.observations.numpy()
        want = observations_of(heat, chm, c["J"], pr.Hh, r)
        assert np.array_equal(obs.view(np.int32), want.view(np.int32)), r
        ref = JR.triangulate_ref(obs, *calib64, False, max_error_px=MAX_ERR)
        assert tri.views.tolist() == ref[1].tolist() and tri.members.tolist() == ref[2].tolist()
        t, cam, j = FALSE_PEAK
        assert tri.members[t, j].tolist() == [0 if k == cam else 1 for k in range(c["C"])] and int(tri.views[t, j]) == 3
        assert int(tri.views.sum()) == 2 * c["J"] * c["C"] - 1
        d_got = np.linalg.norm(tri.points.numpy() - truth, axis=-1)
        d_ref = np.linalg.norm(ref[0] - truth, axis=-1)
        assert (d_got <= d_ref + 1e-3).all(), (r, (d_got - d_ref).max())
        assert np.abs(tri.error.numpy() - ref[3]).max() < 1e-3
        dist[r] = d_got
    # the refined peak is nearer the truth than the grid's: the +-1 px of the grid is a millimetre at this range
    report("joints3d_known_heat", mean_mm_r0=dist[0].mean(), max_mm_r0=dist[0].max(), mean_mm_r1=dist[1].mean(),
           max_mm_r1=dist[1].max())
    assert dist[1].mean() < dist[0].mean() and dist[1].max() < dist[0].max(), (dist[0].mean(), dist[1].mean())
    assert (dist[1] < dist[0]).mean() > 0.9


def test_masked_camera_and_invalid_row():
    c, inp, pred, calib, frames = HC.setup()
    pr, centres, chm, calib64, heat, truth, _ = centred()
    mask = torch.tensor([[1, 1, 0, 1], [1, 1, 1, 1]], dtype=torch.uint8)
    x = cuda(frames[:2])
    bad = centres.clone()
    bad[1] = float("nan")
    pred.forward_batch(x, *calib, centers=bad, camera_mask=mask)          # row 1 is not valid
    clean = as_host(pr.triangulate_joints(heat=cuda(torch.from_numpy(heat)), camera_mask=mask, params=jparams()))
    junk = heat.copy()
    junk[0, 2] = np.nan
    got = as_host(pr.triangulate_joints(heat=cuda(torch.from_numpy(junk)), camera_mask=mask, params=jparams()))
    assert same_tri(got, clean)                                           # (the masked camera's heat reaches nothing)
    assert not got.members[0, :, 2].any() and got.views[0].tolist() == [3] * c["J"]
    assert torch.isnan(got.observations[0, 2, :, :2]).all() and (got.observations[0, 2, :, 2] == 0).all()
    assert torch.isnan(got.points[1]).all() and torch.isnan(got.error[1]).all()
    assert not got.views[1].any() and not got.members[1].any()
    assert torch.isnan(got.observations[1, :, :, :2]).all() and (got.observations[1, :, :, 2] == 0).all()
    # unmasked and valid again, the same predictor gives the unmasked result
    pred.forward_batch(x, *calib, centers=centres)
    full = as_host(pr.triangulate_joints(heat=cuda(torch.from_numpy(heat)), params=jparams()))
    assert full.views[1].tolist() == [4] * c["J"] and not same(full.points[0], got.points[0])


def test_per_frame_set_calibration_and_centred_call():
    c, inp, pred, calib, frames = HC.setup()
    sets = {k: tuple(cuda(t) for t in v) for k, v in HC.derived_sets(*(inp[k] for k in HC.KEYS)).items()}
    order = "ABD"
    per = tuple(torch.stack([sets[k][i] for k in order]) for i in range(3))
    x = cuda(frames[:3])
    p = jparams(**WIDE)
    got = as_host(pred.forward_batch(x, *per, return_triangulated=p)[3])
    assert int(got.views.min()) >= 2
    for t, k in enumerate(order):
        shared = as_host(pred.forward_batch(x, *sets[k], return_triangulated=p)[3])
        assert same_tri(got, shared, slice(t, t + 1)), k
    # row 2 under D is not row 2 under A: the calibration is really read per row
    assert not same(got.points[2], as_host(pred.forward_batch(x, *calib, return_triangulated=p)[3]).points[2])
    # a centred call equals the detected one given its centre
    det = pred.forward_batch(x, *calib, return_2d=True, return_triangulated=p)
    centre = pred.native(c["H"], c["W"], time_batch=3).debug("cuda")["center3d"].clone()
    det = [t.clone() for t in det[:3]] + [det[3], as_host(det[4])]
    cen = pred.forward_batch(x, *calib, return_2d=True, return_triangulated=p, centers=centre)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(det[:3], cen[:3])) and same_tri(as_host(cen[4]), det[4])
    assert all(same(a, b) for a, b in zip(det[3], cen[3]))


def test_graph_replay_single_forms_and_untouched_state():
    from jarvis_hybridnet_amd import _native as N
    c, inp, pred, calib, frames = HC.setup()
    x = cuda(frames[:1])
    g, e = HC.native(1), HC.native(1)
    e.graph_replay = False
    assert g.graph_replay and not e.graph_replay
    bytes_before = N.lib().jh_predictor_device_bytes(g.handle)
    outs = []
    for pr in (g, e):
        first = [t.clone() for t in pr.forward(x)]
        tri = as_host(pr.triangulate_joints(params=WIDE))
        again = [t.clone() for t in pr.forward(x)]                  # (a replay behind the plain launches)
        tri2 = as_host(pr.triangulate_joints(params=WIDE))
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(first, again)) and same_tri(tri, tri2)
        outs.append((first, tri))
    assert all(same(a, b) for a, b in zip(outs[0][0], outs[1][0])) and same_tri(outs[0][1], outs[1][1])
    assert N.lib().jh_predictor_device_bytes(g.handle) == bytes_before
    assert int(outs[0][1].views.max()) >= 2
    # the single-frame form: the tuple comes last, and None with the others
    pts, conf, views, tri = pred(x[0], *calib, return_2d=True, return_triangulated=WIDE)
    assert same(pts, outs[0][0][0]) and same_tri(as_host(tri), outs[0][1])
    nothing = pred(x[0], *calib, return_triangulated=True, centers=torch.full((3,), float("nan")))
    assert nothing == (None, None, None)
    # misuse: parameters out of range raise before anything is enqueued
    bad = N.joints3d_params()
    bad.refine_radius = 4
    with pytest.raises(ValueError, match="refine_radius"):
        g.triangulate_joints(params=bad)
    with pytest.raises(ValueError):
        pred.forward_batch(x, *calib, return_triangulated="yes")
    g.close()
    e.close()


def test_driver_writes_triangulated_csv(tmp_path):
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames, triangulated_row
    c, inp, pred, calib, frames = HC.setup()
    cfg = HC.make_cfg(c)
    cfg.KEYPOINT_NAMES = ["joint%d" % j for j in range(c["J"])]
    sets = [frames[t].numpy() for t in range(3)]
    masks = [None, [1, 1, 0, 1], [0, 0, 0, 1]]                   # the last frame set is not valid
    plain = str(tmp_path / "plain")
    out = str(tmp_path / "tri")
    assert predict3D_frames(pred, iter(sets), *calib, cfg, plain, time_batch=2, camera_mask=iter(masks)) == 3
    assert predict3D_frames(pred, iter(sets), *calib, cfg, out, time_batch=2, camera_mask=iter(masks),
                            output_triangulated=dict(refine_radius=2, **WIDE)) == 3
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    assert read(out, "data3D.csv") == read(plain, "data3D.csv")
    assert not os.path.exists(os.path.join(plain, "triangulated3D.csv"))
    rows = list(csv.reader(read(out, "triangulated3D.csv").decode().splitlines()))
    assert len(rows) == 5 and rows[1] == ["x", "y", "z", "views", "error"] * c["J"]
    assert rows[0][:6] == ["joint0"] * 5 + ["joint1"]
    # the rows are the direct call's values
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]], dtype=torch.uint8)
    x = cuda(torch.stack([frames[0], frames[1], frames[2], frames[2]]))
    for t0 in (0, 2):
        res = pred.forward_batch(x[t0:t0 + 2], *calib, camera_mask=mask[t0:t0 + 2],
                                 return_triangulated=dict(refine_radius=2, **WIDE))
        torch.cuda.synchronize()
        tri = as_host(res[3])
        for t in range(2 if t0 == 0 else 1):
            ok = int(res[2][t]) != 0
            want = triangulated_row(tri.points[t] if ok else None, tri.views[t], tri.error[t], c["J"])
            assert rows[2 + t0 + t] == [str(v) for v in want], (t0, t)
    assert rows[4] == ["NaN"] * (5 * c["J"]) and "NaN" not in rows[2][:3]
