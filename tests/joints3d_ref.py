"""numpy reference of the per-joint robust triangulation (include/jarvis_hip.h: jh_joints3d_params,
jh_op_joint_peaks_refine, jh_op_triangulate_joints), written from the definition and not from the kernels: the
sub-pixel offset emulated in np.float32 operation by operation in the walk order, the consensus built on the float64
reference of the subject association (tests/subjects_ref.py: one slot per camera, one round).  Shared by
tests/test_joints3d_cpu.py (self-tests on scenes whose answer is known) and tests/test_hip_joints3d.py (the kernels
against it)."""
import numpy as np

from tests import subjects_ref as R

F = np.float32
MARGIN = 1e-2           # px: no support distance this near max_error_px, no choice resting on a smaller cost difference


# ---- sub-pixel offset --------------------------------------------------------------------------------------------------
def offset_ref(img, mx, my, r):
    """img (hh,wh) float32, the peak's column mx and row my, radius r -> (ox, oy) float32: the centroid of max(h, 0)
    over the window clipped at the edge, walked y ascending then x ascending, one fp32 rounding per operation."""
    hh, wh = img.shape
    s0, sx, sy = F(0), F(0), F(0)
    for y in range(max(0, my - r), min(hh - 1, my + r) + 1):
        for x in range(max(0, mx - r), min(wh - 1, mx + r) + 1):
            h = F(img[y, x])
            wgt = h if h > 0 else F(0)                    # fmaxf(h, 0): NaN and negative pixels count as 0
            s0 = F(s0 + wgt)
            sx = F(sx + F(wgt * F(x - mx)))
            sy = F(sy + F(wgt * F(y - my)))
    if not s0 > 0:
        return F(0), F(0)
    with np.errstate(all="ignore"):
        return F(sx / s0), F(sy / s0)


def refine_ref(heat, idx, r):
    """heat (N,hh,wh,Jp) float32, idx (N,J) flat indices y*wh + x -> offsets (N,J,2) float32 (jh_op_joint_peaks_refine:
    mx = m % wh, my = m // wh; an index outside the map has offset 0)."""
    heat = np.asarray(heat, F)
    N, hh, wh, _ = heat.shape
    J = idx.shape[1]
    out = np.zeros((N, J, 2), F)
    for n in range(N):
        for j in range(J):
            m = int(idx[n, j])
            if r > 0 and 0 <= m < hh * wh:
                out[n, j] = offset_ref(heat[n, :, :, j], m % wh, m // wh, r)
    return out


def observations_ref(points2d, conf2d, offsets):
    """points2d (...,2) integers, conf2d (...), offsets (...,2) float32 -> obs (...,3) float32 = (u, v, w):
    u = (float)x2d + 2 * ox, the product exact, the sum rounded once."""
    p = np.asarray(points2d).astype(F)
    o = np.asarray(offsets, F)
    return np.concatenate([(p + F(2) * o).astype(F), np.asarray(conf2d, F)[..., None]], -1)


def blob(hh, wh, cx, cy, sigma=0.6, amp=200.0):
    """A Gaussian blob sampled on the hh x wh grid, centred at the sub-pixel position (cx, cy) -> float32.  sigma 0.6:
    narrower than the smallest window, whose centroid then lies within 0.05 pixel of the centre (measured on the CPU
    for radius 1, 2 and 3; at sigma 1.5 the 3 x 3 window cuts the blob and its centroid is biased by up to 0.36)."""
    y, x = np.mgrid[0:hh, 0:wh].astype(np.float64)
    return (amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma ** 2))).astype(F)


# ---- consensus ---------------------------------------------------------------------------------------------------------
def usable(obs, min_conf):
    """obs (C,3) -> (C,) bool: w > 0, w >= min_conf and a finite pixel (an unused camera's row is (NaN, NaN, 0))."""
    obs = np.asarray(obs, F)
    with np.errstate(invalid="ignore"):
        return (obs[:, 2] > 0) & (obs[:, 2] >= F(min_conf)) & np.isfinite(obs[:, 0]) & np.isfinite(obs[:, 1])


def joint_ref(obs, cam, intr, dist, min_views=2, min_conf=0.1, max_error_px=8.0, margin=MARGIN):
    """One joint of one frame set: obs (C,3) float32 = (u, v, w), calibration (C,..) -> point (3,) float64, views int,
    members (C,) uint8, error float64, as jh_op_triangulate_joints defines them: the association of
    subjects_ref.associate_ref with one slot per camera (pixels as given: sx2 = sy2 = 1; weight w: the slot's value is
    255 w) and one round.  margin: its assertions -- over EVERY candidate pair, not only the winner -- that no support
    distance lies within `margin` of max_error_px and no choice rests on a smaller cost difference."""
    obs = np.asarray(obs, F)
    C = obs.shape[0]
    ok = usable(obs, min_conf)
    peaks = np.empty((C, 1, 3), F)
    peaks[:] = np.array(R.EMPTY, F)
    assert (obs[ok, :2] >= 0).all(), "the association's slots are non-negative pixels"
    peaks[ok, 0, :2] = obs[ok, :2]
    peaks[ok, 0, 2] = (obs[ok, 2].astype(np.float64) * 255.0).astype(F)
    ctr, views, mem, err = R.associate_ref(peaks, cam, intr, dist, ok.astype(np.uint8), 1.0, 1.0, 1, max_error_px,
                                           min_views, margin=margin)
    return ctr[0], int(views[0]), (mem[0] >= 0).astype(np.uint8), float(err[0])


def triangulate_ref(obs, cam, intr, dist, per_frame, **kw):
    """obs (T,C,J,3); calibration (C,..) or, per_frame, (T,C,..) -> points (T,J,3), views (T,J), members (T,J,C), error
    (T,J) by joint_ref."""
    obs = np.asarray(obs, F)
    T, C, J = obs.shape[:3]
    pts, views = np.full((T, J, 3), np.nan), np.zeros((T, J), np.int32)
    mem, err = np.zeros((T, J, C), np.uint8), np.full((T, J), np.nan)
    for t in range(T):
        cal = [np.asarray(a[t] if per_frame else a, np.float64) for a in (cam, intr, dist)]
        for j in range(J):
            pts[t, j], views[t, j], mem[t, j], err[t, j] = joint_ref(obs[t, :, j], *cal, **kw)
    return pts, views, mem, err


# ---- scenes ------------------------------------------------------------------------------------------------------------
W, H, FOCAL = 640, 512, 900.0
OUTLIER = (40.0, -30.0)
KINDS = ("clean", "outlier", "two_outliers", "low_conf", "unused", "too_few")


def rig(C):
    """The fixture rig: C cameras on a ring, 640 x 512, f = 900 -> (cam, intr, dist) float64 numpy."""
    from jarvis_hybridnet_amd import synthetic as S
    return tuple(t.double().numpy() for t in S.ring_calibration(C, W, H, FOCAL))


def flipped(calib, c):
    """The calibration with camera c's matrix negated: the same pixels, every point behind the camera."""
    cam = calib[0].copy()
    cam[c] = -cam[c]
    return (cam,) + tuple(calib[1:])


def joint_scene(calib, g, kind="clean", noise=1.0):
    """One joint seen by the cameras of `calib`: a 3D point within +-120 mm of the origin projected in float64, every
    pixel moved by up to +-noise px (1: the heat map's 2-pixel grid), weights in [0.3, 1] -> obs (C,3) float32, the point, and
    the cameras that must not be members.  kind: "clean"; "outlier" / "two_outliers": one / two cameras moved by (40,
    -30) px; "low_conf": one camera far off with w = 0.05; "unused": one camera's row is (NaN, NaN, 0); "too_few": all
    cameras but one have w = 0."""
    C = calib[0].shape[0]
    X = g.uniform(-120.0, 120.0, 3)
    uv, _ = R.project64(X, *calib)
    obs = np.concatenate([uv + g.uniform(-noise, noise, (C, 2)), g.uniform(0.3, 1.0, (C, 1))], 1).astype(F)
    out = []
    if kind in ("outlier", "two_outliers"):
        out = sorted(g.choice(C, 1 if kind == "outlier" else 2, replace=False).tolist())
        obs[out, 0] += F(OUTLIER[0])
        obs[out, 1] += F(OUTLIER[1])
    elif kind == "low_conf":
        out = [int(g.randint(C))]
        obs[out[0]] = (obs[out[0], 0] + F(25), obs[out[0], 1] + F(25), F(0.05))
    elif kind == "unused":
        out = [int(g.randint(C))]
        obs[out[0]] = (np.nan, np.nan, 0.0)
    elif kind == "too_few":
        keep = int(g.randint(C))
        out = [c for c in range(C) if c != keep]
        obs[out, 2] = F(0)
    else:
        assert kind == "clean", kind
    return obs, X, out


def kinds_for(C):
    """The kinds a rig of C cameras carries: an outlier needs three cameras that agree, two need more.  A ring of 32
    cameras and more has none: its 2016 pairs x 64 support distances, those of the pairs with an outlier spread over
    tens of pixels, put one within 1e-2 px of max_error_px in nearly every scene, which the reference refuses."""
    if C < 4 or C >= 32:
        return ("clean", "low_conf", "unused", "too_few")
    return KINDS if C >= 12 else tuple(k for k in KINDS if k != "two_outliers")


def noise_for(C):
    """The pixel noise of a rig's scenes: 1 px, the grid's; 0.05 px for a ring of 32 cameras and more, whose neighbours
    stand 6 degrees apart -- a pixel of noise moves their two-view point by centimetres and its projections in the
    other cameras across max_error_px."""
    return 0.05 if C >= 32 else 1.0


def scenes(C, T, J, seed, calibs):
    """obs (T,C,J,3) float32 for T frame sets of J joints, the kinds of kinds_for(C) in turn; calibs: the T
    calibrations -> obs, the points (T,J,3), kinds (T,J) and the excluded cameras (T,J) lists."""
    g = np.random.RandomState(seed)
    kinds = kinds_for(C)
    obs, pts = np.empty((T, C, J, 3), F), np.empty((T, J, 3))
    kind, out = [[None] * J for _ in range(T)], [[None] * J for _ in range(T)]
    for t in range(T):
        for j in range(J):
            kind[t][j] = kinds[(t * J + j) % len(kinds)]
            obs[t, :, j], pts[t, j], out[t][j] = joint_scene(calibs[t], g, kind[t][j], noise_for(C))
    return obs, pts, kind, out


def case_calibs(C, T, per_frame, flip):
    """The T calibrations of a test case on the rig of C cameras.  Shared: the rig T times, camera `flip` (or None)
    negated.  Per frame set: the rig; the rig with k1, k2 halved; the rig with camera `flip` negated; ... in turn."""
    base = rig(C)
    if not per_frame:
        return [base if flip is None else flipped(base, flip)] * T
    halved = (base[0], base[1], base[2].copy())
    halved[2][:, 0, 0:2] *= 0.5
    three = [base, halved, base if flip is None else flipped(base, flip)]
    return [three[t % 3] for t in range(T)]
