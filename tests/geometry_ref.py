"""References of the three operators at the numerical base of the geometry code -- jh_reconstruct_point (the weighted
DLT: dlt_rows, dlt_term, dlt_solve of csrc/dlt.h), jh_reproject_point (project_one) and jh_softargmax (the V2V tail,
csrc/softargmax.hip) -- in numpy on the CPU, with the case tables tests/test_geometry_ref_cpu.py and
tests/test_hip_geometry_ops.py share.

Each operator has a DEFINITION in float64 and the forward-error bounds below.  The triangulation and the projection also
have an op-by-op float32 EMULATION: one rounding per operation, exactly as csrc/dlt.h spells them, so the kernel can be
held to bits, not to a tolerance that would hide a changed rounding order.

The definition (float64 on the float32 inputs)
  project_def      synthetic.project: q = [x y z 1] M, r = q_a / q_2, uu = r - c_a, dd = 1 + (k1 + k2 r2) r2,
                   U = uu dd + c_a.
  reconstruct_def  oracle.reconstruct_point: the detection undistorted in one step, the rows u P2 - P0 and v P2 - P1
                   weighted by maxval, vh[-1] of the SVD of the UNSCALED A (scaling the columns changes the minimiser),
                   dehomogenised.
  tail_def         oracle.softargmax_tail: softplus (x above 20 passes through), soft-argmax in voxels and mm,
                   min(max h, 255) / 255 and softplus(softplus(x)).

The emulation (float32, u = 2^-24 throughout)
  fma32            a correctly rounded fp32 FMA: the product of two floats is exact in float64 (48 bits), TwoSum gives
                   the exact error of adding the addend, the float64 sum is moved to the odd neighbour when it is
                   inexact (round to odd) and then rounded to float32.  53 >= 2 * 24 + 2, so the double rounding is
                   innocuous: the result is the float32 nearest the exact a b + c.
  project_emu      project_one: fmul, three fmaf, then one rounding per operation.
  dlt_rows_emu     dlt_rows (with the operator's sx2 = sy2 = wdiv = 1, which are exact).
  reconstruct_emu  A^T A in float64 with the terms summed in camera order (dlt_term: both products are exact, so a
                   contracted and a plain evaluation agree), symmetrised, the eigenvector of the smallest eigenvalue by
                   numpy.linalg.eigh, dehomogenised, rounded once to float32.
  smallest_eigvec4 a Python port of the device's cyclic Jacobi, to pin its stop rule and its choice of eigenvalue.

Distance of the emulation to the definition, max over 24 seeds per class, mm (tests/test_geometry_ref_cpu.py prints
them; all points uniform(+-spread) about the origin, detections = the float64 projection + Gaussian pixel noise,
weights wlo + (1 - wlo) rand):

  class          rig / subset                                                     max |emu - def|, mm
  c4             C=4, 640x512, f=900, noise 2 px                                  2.9e-5
  c12            C=12, 1280x1024, f=1800                                          2.2e-5
  c64            C=64 (the ABI's maximum)                                         6.6e-6
  pair30         cameras 0,1 of 12                                                1.2e-4
  pair11         cameras 0,1 of 32                                                2.1e-4
  pair150        cameras 0,5 of 12                                                1.4e-4
  far            C=3, 1920x1200, f=3000, radius 5000, spread 300, noise 1         1.3e-4
  exact          c4 with noise 0 (lambda_0 ~ 0)                                   3.4e-5
  weights        C=6, wlo = 1e-3                                                  3.5e-5
  dist           C=5, f=1200, radius 1200, k1=-0.25, k2=0.08                      5.0e-5
  noisy          c12, noise 20 px                                                 7.7e-5
  pair180 *      cameras 0,6 of 12, rays nearly collinear                         5.8e-3
  triple_narrow * cameras 0,1,2 of 32 (22.5 degrees end to end)                   9.8e-5

  * ill-conditioned IN THE DEFINITION: the float32 rows alone can move the point past 1e-3 mm (pair180 reaches 19 mm
  over 300 seeds, where the two rays all but coincide; triple_narrow, the narrowest three-camera baseline, stays at
  1.5e-4 mm with this spread and noise and is listed with it all the same).  These two are the cases where choosing the
  smaller of two close eigenvalues matters; they are held kernel-versus-emulation only, and their distance to the
  definition is recorded, not asserted.  Every other class is held to 1e-3 mm, the project's bar for a
  triangulated point (tests/test_hip_stages.py::test_geometry).

The Jacobi port against eigh (solver_agreement_bound).  Both are backward stable: each returns the eigenvector of a
matrix within p(n) u64 |A| of A^T A, p(4) about 8, u64 = 2^-53, so by Davis-Kahan the two unit vectors lie within
theta = 16 u64 lambda_3 / (lambda_1 - lambda_0) of each other, and the dehomogenised points within
theta sqrt(1 + |X|^2) (1 + |X_k|) per coordinate (d(x_k / x_3) <= theta (1 + |X_k|) / |x_3|, |x_3| = 1 / sqrt(1 + |X|^2)).
That is asserted for every class; a wrong choice of eigenvalue or a stop rule that ends a sweep early misses it by many
orders of magnitude (measured: the two solvers are within 0.1 of it).  The points rounded to float32 are then EQUAL
unless a coordinate of eigh's float64 point lies within that bound of the midpoint of two neighbouring floats, where
the last bits of either solver -- or of another LAPACK build -- decide the rounding; that is the assertion, together
with one float32 ulp at most, the bar the kernel is held to against the emulation.  For the well-conditioned classes the
bound is about a hundredth of a float32 ulp and every rounded point of the 24 seeds is equal; for pair11 and pair180
it reaches 2 ulp, the float64 points differ by up to 0.04 ulp, and one coordinate of 72 rounds to the neighbouring float
(pair180, seed 1 -- the kernel's Jacobi rounds it the same way).

Forward-error bounds (evaluated in float64 from the REFERENCE's quantities, never from the kernel's output)

  Projection, coordinate a of one camera (project_bound).  q = [x y z 1] M, S = [|x| |y| |z| 1] |M|.  The four-term
  dot product (one product rounding, three FMAs) has |dq_a| <= 4u S_a to first order.  r = q_a / q_2:
  |dr| <= (|dq_a| + |r| |dq_2|) / |q_2| + u |r| <= 4u (S_a + |r| S_2) / |q_2| + u |r|.  uu = r - c_a adds u |uu|.
  dd is built from uu / f in eight roundings, each with a condition of at most about one at the distortions used here,
  so |d dd| <= 8u |dd|; the product uu dd and the last add contribute u |uu dd| (absorbed in the 8u term) and u |U|:
      B = |dd| (4u (S_a + |r| S_2) / |q_2| + u (|r| + |uu|)) + 8u |uu dd| + u |U|.
  The dependence of dd on the error of uu is second order here (|k1 + 2 k2 r2| * 2 |a| |da| * |uu| stays below 1e-5 px
  at the rigs of the table).  B is 1e-4 .. 2e-3 px; the emulation stays below about 0.3 B (printed by the CPU test).

  Soft-argmax index (softargmax_bounds).  rows = 256 / (Jp / 4); a lane sums 8 voxels (ppb = rows * 8 per block), a
  block adds its `rows` lane sums sequentially, the blocks are added exactly.  All terms are positive, so a block sum
  has relative error <= (8 + rows) u; the device softplus is within 4 ulp (expf <= 1, log1pf <= 2, compounded -- the
  figure of tests/test_hip_spread.py) on numerator and denominator; one rounding for the product h * index, three for
  the two conversions to float and the division:
      |idx - idx64| <= (2 (8 + rows) + 13) u idx64      voxels
  and in mm: that times 2 spacing, plus 3u (roi / 2 + |centre| + |mm|) for the last three roundings that are not exact
  (idx * spacing; the subtraction of roi / 2; the addition of the centre.  The doubling is exact).
  conf            relative <= 6u  (4 ulp softplus, fmin exact, one division, one to spare).
  heatmap_final   relative <= 10u (4 ulp inner, propagated with a factor x sigmoid(x) / softplus(x) <= 1, 4 ulp outer,
                  and the roundings).
  softargmax_model is a numpy model of the kernel's summation tree (lane sums of 8 strided voxels, `rows` sequential
  adds, float64 across blocks); at the shapes below it sits 10-50 x under the bound, and one dropped voxel per block
  moves the index of a 'rand' input more than 500 x over it.
"""
import functools
import math

import numpy as np
import torch

from jarvis_hybridnet_amd import synthetic as S

U = 2.0 ** -24
f32 = np.float32


# ---- a correctly rounded fp32 FMA -------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise on float32 arrays (see the module docstring)."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)             # exact: 24 + 24 bits
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                               # TwoSum: p + c == s + e exactly
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))     # the inexact sum lies between s and this neighbour
    return np.where((e != 0) & even, odd, s).astype(np.float32)


# ---- the projection ---------------------------------------------------------------------------------------------------
def _calib_np(cam, intr, dist, dtype):
    return tuple(np.asarray(t.numpy() if hasattr(t, "numpy") else t).astype(dtype) for t in (cam, intr, dist))


def project_def(points, cam, intr, dist):
    """float64 definition: points (P,3) -> (C,P,2)."""
    return S.project(np.asarray(points, dtype=np.float64), *(torch.as_tensor(np.asarray(t)) for t in (cam, intr, dist)))


def project_emu(points, cam, intr, dist):
    """project_one of csrc/dlt.h, one float32 rounding per operation: points (P,3) float32 -> (C,P,2) float32."""
    cam, intr, dist = _calib_np(cam, intr, dist, np.float32)
    pts = np.asarray(points, dtype=np.float32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty((cam.shape[0], pts.shape[0], 2), np.float32)
    one = np.ones_like(x)
    for c in range(cam.shape[0]):
        M, K, D = cam[c], intr[c], dist[c].reshape(-1)
        p = []
        for col in range(3):
            a = x * M[0, col]
            a = fma32(y, M[1, col], a)
            a = fma32(z, M[2, col], a)
            a = fma32(one, M[3, col], a)
            p.append(a)
        cx, cy, fx, fy = K[2, 0], K[2, 1], K[0, 0], K[1, 1]
        uu = p[0] / p[2] - cx
        vv = p[1] / p[2] - cy
        a1, a2 = uu / fx, vv / fy
        r2 = a1 * a1 + a2 * a2
        dd = f32(1) + (D[0] + D[1] * r2) * r2
        out[c, :, 0] = uu * dd + cx
        out[c, :, 1] = vv * dd + cy
    return out


def project_bound(points, cam, intr, dist):
    """B of the module docstring, (C,P,2) float64 pixels, and the depths q_2 (C,P)."""
    cam, intr, dist = _calib_np(cam, intr, dist, np.float64)
    pts = np.asarray(points, dtype=np.float32).astype(np.float64)
    ph = np.concatenate([pts, np.ones((pts.shape[0], 1))], 1)
    B = np.empty((cam.shape[0], pts.shape[0], 2))
    depth = np.empty((cam.shape[0], pts.shape[0]))
    for c in range(cam.shape[0]):
        q, Sq = ph @ cam[c], np.abs(ph) @ np.abs(cam[c])
        ctr, foc = (intr[c, 2, 0], intr[c, 2, 1]), (intr[c, 0, 0], intr[c, 1, 1])
        r = [q[:, a] / q[:, 2] for a in range(2)]
        uu = [r[a] - ctr[a] for a in range(2)]
        r2 = (uu[0] / foc[0]) ** 2 + (uu[1] / foc[1]) ** 2
        dd = 1 + (dist[c, 0, 0] + dist[c, 0, 1] * r2) * r2
        for a in range(2):
            Ua = uu[a] * dd + ctr[a]
            B[c, :, a] = (np.abs(dd) * (4 * U * (Sq[:, a] + np.abs(r[a]) * Sq[:, 2]) / np.abs(q[:, 2])
                                        + U * (np.abs(r[a]) + np.abs(uu[a])))
                          + 8 * U * np.abs(uu[a] * dd) + U * np.abs(Ua))
        depth[c] = q[:, 2]
    return B, depth


# ---- the triangulation ------------------------------------------------------------------------------------------------
def reconstruct_def(points2d, maxvals, cam, intr, dist):
    """float64 definition: points2d (2,C) pixels, maxvals (C,), calibration of the C cameras -> (3,) float64 mm."""
    cam, intr, dist = _calib_np(cam, intr, dist, np.float64)
    pts = np.asarray(points2d, dtype=np.float32).astype(np.float64)
    w = np.asarray(maxvals, dtype=np.float32).astype(np.float64).reshape(-1)
    P = cam.transpose(0, 2, 1)                                   # (C,3,4)
    u = pts[0] - intr[:, 2, 0]
    v = pts[1] - intr[:, 2, 1]
    r2 = (u / intr[:, 0, 0]) ** 2 + (v / intr[:, 1, 1]) ** 2
    dd = 1 + (dist[:, 0, 0] + dist[:, 0, 1] * r2) * r2
    u = u / dd + intr[:, 2, 0]
    v = v / dd + intr[:, 2, 1]
    A = np.stack([u[:, None] * P[:, 2] - P[:, 0], v[:, None] * P[:, 2] - P[:, 1]], 1) * w[:, None, None]
    X = np.linalg.svd(A.reshape(-1, 4))[2][-1]
    return X[:3] / X[3]


def dlt_rows_emu(points2d, maxvals, cam, intr, dist):
    """dlt_rows of csrc/dlt.h for every camera, one float32 rounding per operation -> r0, r1 (C,4) float32."""
    cam, intr, dist = _calib_np(cam, intr, dist, np.float32)
    pts = np.asarray(points2d, dtype=np.float32)
    one = f32(1)
    cx, cy, fx, fy = intr[:, 2, 0], intr[:, 2, 1], intr[:, 0, 0], intr[:, 1, 1]
    k1, k2 = dist[:, 0, 0], dist[:, 0, 1]
    wgt = np.asarray(maxvals, dtype=np.float32).reshape(-1) / one
    u = pts[0] * one - cx
    v = pts[1] * one - cy
    a1, a2 = u / fx, v / fy
    r2 = a1 * a1 + a2 * a2
    dd = one + (k1 + k2 * r2) * r2
    u = u / dd + cx
    v = v / dd + cy
    r0 = (u[:, None] * cam[:, :, 2] - cam[:, :, 0]) * wgt[:, None]
    r1 = (v[:, None] * cam[:, :, 2] - cam[:, :, 1]) * wgt[:, None]
    assert r0.dtype == np.float32 and r1.dtype == np.float32
    return r0, r1


def ata_emu(r0, r1):
    """A^T A (4,4) float64, the terms of dlt_term summed in camera order, then symmetrised as dlt_solve does."""
    r0, r1 = r0.astype(np.float64), r1.astype(np.float64)
    ata = np.zeros((4, 4))
    for c in range(r0.shape[0]):
        ata = ata + (np.outer(r0[c], r0[c]) + np.outer(r1[c], r1[c]))
    return 0.5 * (ata + ata.T)


def point_of(x):
    """dlt_solve's tail: dehomogenise in float64, round once to float32."""
    return (x[:3] / x[3]).astype(np.float32)


def reconstruct_emu(points2d, maxvals, cam, intr, dist, full=False):
    """The emulation of jh_reconstruct_point -> (3,) float32 (full: also the symmetrised A^T A and its eigenvalues)."""
    a = ata_emu(*dlt_rows_emu(points2d, maxvals, cam, intr, dist))
    lam, vec = np.linalg.eigh(a)
    p = point_of(vec[:, 0])
    return (p, a, lam) if full else p


def smallest_eigvec4(a):
    """Python port of smallest_eigvec4 (csrc/dlt.h): cyclic Jacobi in float64 -> (eigenvector (4,), sweeps)."""
    a = [[float(a[i][j]) for j in range(4)] for i in range(4)]
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    sweeps = 0
    for sweep in range(30):
        off = 0.0
        for p in range(4):
            for q in range(p + 1, 4):
                off += a[p][q] * a[p][q]
        diag = 0.0
        for p in range(4):
            diag += a[p][p] * a[p][p]
        if off <= 1e-30 * diag:
            break
        sweeps += 1
        for p in range(4):
            for q in range(p + 1, 4):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(tt * tt + 1.0)
                sn = tt * c
                for k in range(4):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - sn * akq
                    a[k][q] = sn * akp + c * akq
                for k in range(4):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - sn * aqk
                    a[q][k] = sn * apk + c * aqk
                for k in range(4):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - sn * vkq
                    v[k][q] = sn * vkp + c * vkq
    m = 0
    for i in range(1, 4):
        if a[i][i] < a[m][m]:
            m = i
    return np.array([v[k][m] for k in range(4)]), sweeps


def solver_agreement_bound(lam, vec):
    """How far the float64 points of two backward-stable eigen-solvers may lie apart, per coordinate, mm (module
    docstring): lam the ascending eigenvalues, vec the unit eigenvector of lam[0]."""
    X = vec[:3] / vec[3]
    theta = 16 * 2.0 ** -53 * lam[3] / (lam[1] - lam[0])
    return theta * np.sqrt(1.0 + (X ** 2).sum()) * (1.0 + np.abs(X))


# ---- the triangulation and projection cases ---------------------------------------------------------------------------
# class -> C of the ring, (W, H), focal, radius, k1, k2, the cameras used (None: all), spread mm, noise px, wlo
def _rig(C, size=(1280, 1024), focal=1800.0, radius=1500.0, k1=-0.05, k2=0.01, subset=None, spread=100.0, noise=2.0,
         wlo=0.3):
    return dict(C=C, size=size, focal=focal, radius=radius, k1=k1, k2=k2, subset=subset, spread=spread, noise=noise,
                wlo=wlo)


TRI_CLASSES = {
    "c4": _rig(4, (640, 512), 900.0),
    "c12": _rig(12),
    "c64": _rig(64),
    "pair30": _rig(12, subset=(0, 1)),
    "pair11": _rig(32, subset=(0, 1)),
    "pair150": _rig(12, subset=(0, 5)),
    "far": _rig(3, (1920, 1200), 3000.0, radius=5000.0, spread=300.0, noise=1.0),
    "exact": _rig(4, (640, 512), 900.0, noise=0.0),
    "weights": _rig(6, wlo=1e-3),
    "dist": _rig(5, focal=1200.0, radius=1200.0, k1=-0.25, k2=0.08),
    "noisy": _rig(12, noise=20.0),
    "pair180": _rig(12, subset=(0, 6)),
    "triple_narrow": _rig(32, subset=(0, 1, 2)),
}
ILL_CONDITIONED = ("pair180", "triple_narrow")       # in the definition itself: kernel-versus-emulation only
TRI_BAR_MM = 1e-3
PROJECT_RIGS = ("c4", "c12", "far", "dist")
PROJECT_SHAPES = [(1, 1), (4, 16), (4, 17), (12, 130), (64, 3)]      # (C, P): P * C = 1, 64, 68, 1560, 192 threads
MIN_DEPTH_MM = 100.0


@functools.lru_cache(maxsize=None)
def _ring(C, size, focal, radius, k1, k2):
    return S.ring_calibration(C, size[0], size[1], focal, radius, k1, k2)


def rig_calibration(name, C=None):
    """(cam, intr, dist) float32 tensors of class `name`'s ring (all of its cameras), or of the same optics with C."""
    r = TRI_CLASSES[name]
    return _ring(C or r["C"], r["size"], r["focal"], r["radius"], r["k1"], r["k2"])


def tri_case(name, seed):
    """One triangulation case -> dict(calib = the used cameras' (cam, intr, dist) float32 tensors, pts2d (2,C) float32,
    maxvals (C,) float32, p3d (3,) the true point)."""
    r = TRI_CLASSES[name]
    rng = np.random.RandomState(1000 * (1 + list(TRI_CLASSES).index(name)) + seed)
    calib = rig_calibration(name)
    if r["subset"] is not None:
        calib = tuple(t[list(r["subset"])].contiguous() for t in calib)
    n = calib[0].shape[0]
    p3d = rng.uniform(-r["spread"], r["spread"], 3)
    uv = S.project(p3d[None], *calib)[:, 0] + rng.randn(n, 2) * r["noise"]
    w = r["wlo"] + (1.0 - r["wlo"]) * rng.rand(n)
    return dict(calib=calib, pts2d=np.ascontiguousarray(uv.T).astype(np.float32), maxvals=w.astype(np.float32), p3d=p3d)


def project_case(rig, C, P):
    """One projection case -> (calib, points (P,3) float32): `rig`'s optics on a ring of C cameras, points uniform in
    +-0.4 radius (some project outside the frame), every one at least MIN_DEPTH_MM in front of every camera."""
    r = TRI_CLASSES[rig]
    calib = rig_calibration(rig, C)
    rng = np.random.RandomState(7000 + 100 * PROJECT_RIGS.index(rig) + C + P)
    pts = np.empty((0, 3), np.float32)
    while pts.shape[0] < P:
        cand = rng.uniform(-0.4 * r["radius"], 0.4 * r["radius"], (P, 3)).astype(np.float32)
        depth = project_bound(cand, *calib)[1]
        pts = np.concatenate([pts, cand[(depth >= MIN_DEPTH_MM).all(0)]])[:P]
    return calib, pts


# ---- the soft-argmax tail ---------------------------------------------------------------------------------------------
SOFT_SHAPES = [(2, 1, 6), (1, 23, 9), (2, 30, 16), (1, 100, 5)]     # (T, J, Gh), see tests/test_hip_geometry_ops.py
SOFT_KINDS = ("rand", "peaked", "corner", "range")
SPACING = 2.0


def padded_joints(J):
    return (J + 7) // 8 * 8


def block_geometry(J):
    """(Jp, rows, ppb) of softargmax_partial_kernel for J joints."""
    Jp = padded_joints(J)
    rows = 256 // (Jp // 4)
    return Jp, rows, rows * 8


def soft_input(kind, T, J, Gh, seed):
    """x (T,J,Gh,Gh,Gh) float32 tensor.  'rand' / 'peaked': make_input of tests/test_hip_spread.py.  'corner':
    background -30 and one voxel of +10 per joint at a flat index cycling through the first and last voxel of the cube,
    of a block and of a lane's stride.  'range': the softplus branch (> 20) and the confidence clamp (255)."""
    from tests.test_hip_spread import make_input
    if kind in ("rand", "peaked"):
        return make_input(kind, T, J, Gh, seed)
    P = Gh ** 3
    _, rows, ppb = block_geometry(J)
    if kind == "corner":
        x = torch.full((T, J, P), -30.0)
        spots = [0, P - 1, ppb - 1, ppb, rows - 1, rows]
        for t in range(T):
            for j in range(J):
                x[t, j, min(spots[(j + t) % len(spots)], P - 1)] = 10.0
        return x.view(T, J, Gh, Gh, Gh).contiguous()
    assert kind == "range"
    x = make_input("rand", T, J, Gh, seed).view(T, J, P)
    g = torch.Generator().manual_seed(seed + 1)
    above = float(np.nextafter(f32(20), f32(np.inf)))
    for t in range(T):
        plant = {0: [20.0, above, 21.0, -30.0], 1: [21.0], 2: [255.0], 3: [300.0]}
        if J == 1:
            plant[0] = plant[0] + [300.0]
        for j, vals in plant.items():
            if j < J:
                where = torch.randperm(P, generator=g)[:len(vals)].tolist()
                for p, val in zip(where, vals):
                    x[t, j, p] = val
    return x.view(T, J, Gh, Gh, Gh).contiguous()


def soft_centres(T, seed):
    """(T,3) int32 centres, randint(-600, 600), different for every t."""
    from tests.test_hip_spread import centres_int
    return centres_int(T, seed)


def _softplus64(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def tail_def(x, c3, spacing, roi):
    """float64 definition -> dict(idx (T,J,3) voxels, points (T,J,3) mm, conf (T,J), final (T,J,Gh,Gh,Gh))."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    T, J, Gh = xd.shape[:3]
    h = _softplus64(xd)
    ax = np.arange(Gh, dtype=np.float64)
    grids = np.meshgrid(ax, ax, ax, indexing="ij")
    norm = h.sum(axis=(2, 3, 4))
    idx = np.stack([(h * g).sum(axis=(2, 3, 4)) / norm for g in grids], -1)
    points = idx * spacing * 2 - roi / 2.0 + np.asarray(c3, dtype=np.float64)[:, None, :]
    conf = np.minimum(h.reshape(T, J, -1).max(-1), 255.0) / 255.0
    return dict(idx=idx, points=points, conf=conf, final=_softplus64(h))


def softargmax_bounds(ref, c3, J, spacing, roi):
    """(index bound in voxels, points bound in mm), both (T,J,3), from the float64 reference `ref` = tail_def(...)."""
    rows = block_geometry(J)[1]
    bidx = (2 * (8 + rows) + 13) * U * ref["idx"]
    centre = np.abs(np.asarray(c3, dtype=np.float64))[:, None, :]
    return bidx, bidx * 2 * spacing + 3 * U * (roi / 2.0 + centre + np.abs(ref["points"]))


CONF_REL, FINAL_REL = 6 * U, 10 * U


def softargmax_model(x, c3, spacing, roi, drop_last=False):
    """numpy float32 model of softargmax_partial_kernel + softargmax_final_kernel's summation tree -> (idx, points),
    (T,J,3) float32.  drop_last: leave out the last voxel of every block (the `p < p1 - 1` mistake)."""
    xn = np.asarray(x, dtype=np.float32)
    T, J, Gh = xn.shape[:3]
    P = Gh ** 3
    _, rows, ppb = block_geometry(J)
    with np.errstate(over="ignore"):
        h = np.where(xn > 20, xn, np.log1p(np.exp(np.minimum(xn, f32(20))))).astype(np.float32).reshape(T, J, P)
    if drop_last:
        h = h.copy()
        h[:, :, [min(P, b + ppb) - 1 for b in range(0, P, ppb)]] = 0
    p = np.arange(P)
    coords = [(p // (Gh * Gh)).astype(np.float32), ((p // Gh) % Gh).astype(np.float32), (p % Gh).astype(np.float32)]
    nb = (P + ppb - 1) // ppb

    def tree(vals):                                              # (T,J,P) float32 terms -> (T,J) float64
        pad = np.zeros((T, J, nb * ppb), np.float32)
        pad[:, :, :P] = vals
        pad = pad.reshape(T, J, nb, 8, rows)                     # voxel p0 + k * rows + row
        lane = np.zeros((T, J, nb, rows), np.float32)
        for k in range(8):
            lane = lane + pad[:, :, :, k, :]
        acc = np.zeros((T, J, nb), np.float32)
        for r in range(rows):
            acc = acc + lane[:, :, :, r]
        assert acc.dtype == np.float32
        return acc.astype(np.float64).sum(-1)

    norm = tree(h).astype(np.float32)
    idx = np.stack([tree(h * c).astype(np.float32) / norm for c in coords], -1)
    centre = np.asarray(c3).astype(np.float32)[:, None, :]
    points = ((idx * f32(spacing)) * f32(2) - f32(roi) / f32(2)) + centre
    assert idx.dtype == np.float32 and points.dtype == np.float32
    return idx, points
