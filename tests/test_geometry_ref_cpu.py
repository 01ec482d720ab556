"""CPU: the references of tests/geometry_ref.py against each other and against exact arithmetic, so that what the GPU
tests of tests/test_hip_geometry_ops.py hold the kernels to is itself pinned:

  fma32                  against fractions.Fraction arithmetic, cancelling triples included;
  project_emu            within the bound B of the float64 projection, every camera and point of the projection cases;
  reconstruct_emu        within 1e-3 mm of the float64 definition for every well-conditioned class (the worst distance of
                         every class is printed: the table of the geometry_ref docstring);
  smallest_eigvec4       the port of the device's Jacobi gives the float32 point of numpy.linalg.eigh on the A^T A of
                         every class (up to rounding ties, see geometry_ref): its stop rule is relative to the LARGEST
                         diagonal entry (~1e13) while the wanted eigenvalue lies between 1e0 and 1e8;
  softargmax_model       the kernel's summation tree within the index bound at every shape and input kind -- and a model
                         that drops one voxel per block outside it.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import geometry_ref as R

SEEDS = 24


def round_fraction_f32(q):
    """The float32 nearest the Fraction q (ties to even), normal range only."""
    if q == 0:
        return np.float32(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 24
    while q / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while q / Fraction(2) ** e < 2 ** 23:
        e -= 1
    s = q / Fraction(2) ** e
    m = s.numerator // s.denominator
    rem = s - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    assert -126 <= e + 23 <= 126
    return np.float32(sign * float(m) * 2.0 ** e)       # m <= 2^24 and 2^e are exact, so is the product


def test_fma32_against_exact_arithmetic():
    rng = np.random.RandomState(5)
    n = 10000
    a = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(np.float32)
    # a third cancels to the last bits (c = -fl(a b), moved by 0..2 ulp), a third has a product of c's magnitude
    k = n // 3
    ab = (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    c[:k] = -ab[:k]
    for _ in range(2):
        step = rng.randint(0, 2, k).astype(bool)
        toward = np.where(rng.rand(k) < 0.5, -np.inf, np.inf).astype(np.float32)
        c[:k] = np.where(step, np.nextafter(c[:k], toward), c[:k])
    c[k:2 * k] = ab[k:2 * k] * rng.uniform(-4, 4, k).astype(np.float32)
    got = R.fma32(a, b, c)
    assert got.dtype == np.float32
    wrong = two_roundings = 0
    for i in range(n):
        want = round_fraction_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        wrong += int(got[i] != want)
        two_roundings += int(np.float32(ab[i] + c[i]) != want)
    print("fma32: %d of %d differ from the exact result; mul + add would differ on %d" % (wrong, n, two_roundings))
    assert wrong == 0
    assert two_roundings > n // 20          # the triples can tell an FMA from a multiply and an add


@pytest.mark.parametrize("rig", R.PROJECT_RIGS)
def test_projection_emulation_within_bound(rig):
    worst, outside, total = 0.0, 0, 0
    for C, P in R.PROJECT_SHAPES:
        calib, pts = R.project_case(rig, C, P)
        ref = R.project_def(pts, *calib)
        B, depth = R.project_bound(pts, *calib)
        emu = R.project_emu(pts, *calib)
        assert emu.shape == (C, P, 2) and emu.dtype == np.float32
        assert depth.min() >= R.MIN_DEPTH_MM
        ratio = np.abs(emu.astype(np.float64) - ref) / B
        worst = max(worst, float(ratio.max()))
        W, H = R.TRI_CLASSES[rig]["size"]
        outside += int(((ref[..., 0] < 0) | (ref[..., 0] > W) | (ref[..., 1] < 0) | (ref[..., 1] > H)).sum())
        total += C * P
        print("project %s C=%d P=%d: worst |emu - def| / B = %.3f, B in [%.3g, %.3g] px"
              % (rig, C, P, ratio.max(), B.min(), B.max()))
        assert ratio.max() <= 1.0
    assert 0 < outside < total                  # some projections outside the frame, some inside


@pytest.mark.parametrize("name", list(R.TRI_CLASSES))
def test_triangulation_emulation_against_definition(name):
    worst = ratio = solver = 0.0
    sweeps_max = flips = 0
    for seed in range(SEEDS):
        c = R.tri_case(name, seed)
        want = R.reconstruct_def(c["pts2d"], c["maxvals"], *c["calib"])
        emu, a, lam = R.reconstruct_emu(c["pts2d"], c["maxvals"], *c["calib"], full=True)
        worst = max(worst, float(np.abs(emu.astype(np.float64) - want).max()))
        ratio = max(ratio, float(max(lam[0], 0.0) / lam[1]))
        # the port of the device's Jacobi picks the same eigenvector (see solver_agreement_bound)
        x, sweeps = R.smallest_eigvec4(a)
        sweeps_max = max(sweeps_max, sweeps)
        got, vec = R.point_of(x), np.linalg.eigh(a)[1][:, 0]
        apart = np.abs(x[:3] / x[3] - vec[:3] / vec[3]) / R.solver_agreement_bound(lam, vec)
        solver = max(solver, float(apart.max()))
        assert apart.max() <= 1.0, (name, seed, apart)
        # the rounded points are equal, except where eigh's float64 coordinate lies within that bound of the midpoint of
        # two floats (then the last bits of either solver decide the rounding), and never more than one ulp apart
        X = vec[:3] / vec[3]
        mids = [(emu.astype(np.float64) + np.nextafter(emu, np.float32(s * np.inf)).astype(np.float64)) / 2
                for s in (-1, 1)]
        tie = np.minimum(np.abs(X - mids[0]), np.abs(X - mids[1])) <= R.solver_agreement_bound(lam, vec)
        flips += int((got != emu).sum())
        assert ((got == emu) | tie).all(), (name, seed, got, emu)
        assert (np.abs(got - emu) <= np.spacing(np.abs(emu))).all(), (name, seed, got, emu)
        if name == "exact":                     # ... and it is the subject's point: the detections carry no noise
            assert np.abs(want - c["p3d"]).max() < 0.05
    print("triangulation %-14s max |emulation - definition| = %.2g mm over %d seeds (lambda_0 / lambda_1 up to %.3g, "
          "Jacobi sweeps <= %d, Jacobi - eigh <= %.3g of its bound, %d float32 coordinates differ)"
          % (name, worst, SEEDS, ratio, sweeps_max, solver, flips))
    assert sweeps_max < 30                      # the stop rule ended the iteration, not the sweep limit
    if name not in R.ILL_CONDITIONED:
        assert worst < R.TRI_BAR_MM


def test_zero_weight_rows_leave_the_sum_alone():
    """A camera of weight 0 contributes rows of +-0 and s + 0.0 == s: the emulation on all cameras has the bits of the
    emulation on the others (what the masked forms of the kernels rely on)."""
    c = R.tri_case("weights", 0)
    w = c["maxvals"].copy()
    w[[2, 4]] = 0
    keep = [0, 1, 3, 5]
    full = R.reconstruct_emu(c["pts2d"], w, *c["calib"])
    part = R.reconstruct_emu(c["pts2d"][:, keep], w[keep], *(t[keep] for t in c["calib"]))
    assert np.array_equal(full, part)


@pytest.mark.parametrize("kind", R.SOFT_KINDS)
@pytest.mark.parametrize("T,J,Gh", R.SOFT_SHAPES)
def test_softargmax_summation_tree_within_bound(T, J, Gh, kind):
    x = R.soft_input(kind, T, J, Gh, 11 + Gh)
    c3 = R.soft_centres(T, Gh).numpy()
    roi = 2 * Gh * R.SPACING
    ref = R.tail_def(x.numpy(), c3, R.SPACING, roi)
    bidx, bmm = R.softargmax_bounds(ref, c3, J, R.SPACING, roi)
    idx, points = R.softargmax_model(x.numpy(), c3, R.SPACING, roi)
    ri = float((np.abs(idx.astype(np.float64) - ref["idx"]) / bidx).max())
    rp = float((np.abs(points.astype(np.float64) - ref["points"]) / bmm).max())
    print("soft-argmax model %s %s: index error / bound = %.3f, mm error / bound = %.3f" % ((T, J, Gh), kind, ri, rp))
    assert ri <= 1.0 and rp <= 1.0
    if kind == "rand":
        # the bound can tell: without the last voxel of every block the index leaves it
        idx_d, _ = R.softargmax_model(x.numpy(), c3, R.SPACING, roi, drop_last=True)
        moved = np.abs(idx_d.astype(np.float64) - ref["idx"]) / bidx
        print("    one voxel per block dropped: index error / bound = %.3g" % moved.max())
        assert moved.max() > 1.0
    if kind == "range":
        # the planted values are where the issue's exact confidences come from
        mx = x.numpy().reshape(T, J, -1).max(-1)
        assert (mx[:, 0] == (300.0 if J == 1 else 21.0)).all()
        if J > 3:
            assert (mx[:, 1] == 21.0).all() and (mx[:, 2] == 255.0).all() and (mx[:, 3] == 300.0).all()
