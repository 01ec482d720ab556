"""GPU: the three operators at the numerical base of the geometry code at op level -- jh_reconstruct_point (dlt_rows,
dlt_term, dlt_solve of csrc/dlt.h through triangulate_body), jh_reproject_point (project_one) and jh_softargmax (the V2V
tail, csrc/softargmax.hip) -- against the references of tests/geometry_ref.py, whose docstring derives every bound used
here and whose own consistency tests/test_geometry_ref_cpu.py checks without a GPU.

  jh_reconstruct_point  every class of the table x 3 seeds within ONE float32 ulp per coordinate of the op-by-op
                        emulation (the fraction that is bit-equal is reported), the well-conditioned classes also within
                        1e-3 mm of the float64 definition; zero weights give the bits of the call without those cameras;
                        0 and 65 cameras are refused.
  jh_reproject_point    (C, P) = (1,1), (4,16), (4,17), (12,130), (64,3) -- P * C is one thread, exactly one 64-thread
                        block, one over, several ragged blocks -- on four rigs, points outside the frame included:
                        BIT-EQUAL to the emulation, within the bound B of float64, in the ABI's (C, P, 2) layout;
                        ReprojectionTool's (C,2,P) / (C,2) against per-point calls.
  jh_softargmax         shapes (T, J, Gh) = (2,1,6): Jp 8, 128 rows, P smaller than one block; (1,23,9): q = 6, 4 idle
                        lanes, ragged last block; (2,30,16): q = 8, P an exact number of blocks; (1,100,5): Jp 104,
                        q = 26, 9 rows, 22 idle lanes, 72 voxels per block, ragged.  Inputs 'rand', 'peaked', 'corner'
                        (all mass in the first / last voxel of the cube, of a block, of a lane's stride) and 'range' (the
                        softplus branch above 20, the confidence clamp at 255).  points within the mm bound, conf within
                        6u (and exact where the clamp or an exact quotient decides it), heatmap_final for all T within
                        10u elementwise, the same bits without heatmap_final, row t of the batch = the T = 1 call.
"""
import numpy as np
import pytest
import torch

from tests import geometry_ref as R
from tests.gpu_util import cuda, report

pytestmark = pytest.mark.gpu

SEEDS = 3


def native():
    from jarvis_hybridnet_amd import _native as N
    return N


def dev_calib(calib):
    return tuple(cuda(t.float()) for t in calib)


# ---- jh_reconstruct_point ---------------------------------------------------------------------------------------------
def reconstruct(pts2d, maxvals, calib):
    """jh_reconstruct_point on pts2d (2,C) and maxvals (C,) float32 arrays under calib (host tensors) -> (3,) float32."""
    N = native()
    n = pts2d.shape[1]
    pts, wt = cuda(torch.from_numpy(np.ascontiguousarray(pts2d))), cuda(torch.from_numpy(np.ascontiguousarray(maxvals)))
    out = torch.empty((3,), device="cuda")
    nb = N.lib().jh_reconstruct_workspace_bytes(n)
    ws = N.workspace(nb, out.device)
    N.check(N.lib().jh_reconstruct_point(N.ptr(pts), N.ptr(wt), n, *(N.ptr(t) for t in dev_calib(calib)), N.ptr(out),
                                         N.ptr(ws), nb, N.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(R.TRI_CLASSES))
def test_reconstruct_point_against_emulation(name):
    equal = total = 0
    worst_ulp = worst_def = 0.0
    for seed in range(SEEDS):
        c = R.tri_case(name, seed)
        got = reconstruct(c["pts2d"], c["maxvals"], c["calib"])
        emu = R.reconstruct_emu(c["pts2d"], c["maxvals"], *c["calib"])
        want = R.reconstruct_def(c["pts2d"], c["maxvals"], *c["calib"])
        ulps = np.abs(got.astype(np.float64) - emu.astype(np.float64)) / np.spacing(np.abs(emu)).astype(np.float64)
        dist = float(np.abs(got.astype(np.float64) - want).max())
        print("reconstruct %s seed %d: kernel %s emulation %s (%.3g ulp apart), %.3g mm from the definition"
              % (name, seed, got, emu, ulps.max(), dist))
        equal += int((got == emu).sum())
        total += 3
        worst_ulp, worst_def = max(worst_ulp, float(ulps.max())), max(worst_def, dist)
    report("geom_reconstruct", cls=name, seeds=SEEDS, bit_equal_fraction=equal / total, max_ulp=worst_ulp,
           max_mm_to_definition=worst_def)
    assert worst_ulp <= 1.0
    if name not in R.ILL_CONDITIONED:
        assert worst_def < R.TRI_BAR_MM


def test_reconstruct_point_zero_weights_drop_the_camera():
    """Rows of weight 0 are +-0 and s + 0.0 == s: the bits of the call on the four remaining cameras with their
    calibration rows (the property the masked forms rely on)."""
    c = R.tri_case("weights", 0)
    w = c["maxvals"].copy()
    w[[2, 4]] = 0
    keep = [0, 1, 3, 5]
    full = reconstruct(c["pts2d"], w, c["calib"])
    part = reconstruct(np.ascontiguousarray(c["pts2d"][:, keep]), w[keep], tuple(t[keep].contiguous() for t in c["calib"]))
    emu = R.reconstruct_emu(c["pts2d"], w, *c["calib"])
    assert np.array_equal(full.view(np.int32), part.view(np.int32)), (full, part)
    assert (np.abs(full - emu) <= np.spacing(np.abs(emu))).all(), (full, emu)


@pytest.mark.parametrize("cams", [0, 65])
def test_reconstruct_point_refuses_camera_counts(cams):
    N = native()
    n = 65
    calib = dev_calib(R.rig_calibration("c12", n))
    pts, wt, out = torch.zeros((2, n), device="cuda"), torch.ones((n,), device="cuda"), torch.zeros((3,), device="cuda")
    nb = N.lib().jh_reconstruct_workspace_bytes(64)
    ws = N.workspace(nb, out.device)
    rc = N.lib().jh_reconstruct_point(N.ptr(pts), N.ptr(wt), cams, *(N.ptr(t) for t in calib), N.ptr(out), N.ptr(ws),
                                      nb, N.stream())
    torch.cuda.synchronize()
    assert rc != 0 and len(N.lib().jh_last_error()) > 0
    assert out.cpu().tolist() == [0.0, 0.0, 0.0]                 # nothing was enqueued


def test_reconstruct_point_of_the_tool_is_the_abi_call():
    from jarvis_hybridnet_amd.utils.reprojection import ReprojectionTool
    c = R.tri_case("c12", 0)
    tool = ReprojectionTool()
    tool.cameraMatrices, tool.intrinsicMatrices, tool.distortionCoefficients = dev_calib(c["calib"])
    rec = tool.reconstructPoint(cuda(torch.from_numpy(c["pts2d"])), cuda(torch.from_numpy(c["maxvals"]).reshape(-1, 1, 1)))
    torch.cuda.synchronize()
    assert rec.shape == (3,)
    assert np.array_equal(rec.cpu().numpy().view(np.int32), reconstruct(c["pts2d"], c["maxvals"], c["calib"]).view(np.int32))


# ---- jh_reproject_point -----------------------------------------------------------------------------------------------
def reproject(pts, calib):
    """jh_reproject_point on pts (P,3) float32 under calib (device tensors) -> (C,P,2) float32 on the host."""
    N = native()
    C, P = calib[0].shape[0], pts.shape[0]
    uv = torch.full((C, P, 2), float("nan"), device="cuda")
    N.check(N.lib().jh_reproject_point(N.ptr(cuda(torch.from_numpy(pts))), P, C, *(N.ptr(t) for t in calib), N.ptr(uv),
                                       N.stream()))
    torch.cuda.synchronize()
    return uv.cpu().numpy()


@pytest.mark.parametrize("C,P", R.PROJECT_SHAPES)
@pytest.mark.parametrize("rig", R.PROJECT_RIGS)
def test_reproject_point_against_emulation(rig, C, P):
    calib, pts = R.project_case(rig, C, P)
    got = reproject(pts, dev_calib(calib))
    emu = R.project_emu(pts, *calib)
    ref = R.project_def(pts, *calib)
    B, depth = R.project_bound(pts, *calib)
    assert depth.min() >= R.MIN_DEPTH_MM
    ratio = float((np.abs(got.astype(np.float64) - ref) / B).max())
    differ = int((got.view(np.int32) != emu.view(np.int32)).sum())
    W, H = R.TRI_CLASSES[rig]["size"]
    outside = int(((ref[..., 0] < 0) | (ref[..., 0] > W) | (ref[..., 1] < 0) | (ref[..., 1] > H)).sum())
    report("geom_project", rig=rig, C=C, P=P, err_over_B=ratio, not_bit_equal=differ, outside_frame=outside)
    print("reproject %s C=%d P=%d: %d of %d elements differ from the emulation, worst error / B = %.3f, %d outside"
          % (rig, C, P, differ, got.size, ratio, outside))
    # (C, P, 2): camera-major, the pixel pair innermost -- the emulation is laid out by definition, not by the kernel
    assert got.shape == emu.shape == (C, P, 2)
    assert differ == 0
    assert ratio <= 1.0


def test_reproject_point_layouts_of_the_tool():
    """ReprojectionTool.reprojectPoint: (C,2,P) for P > 1, (C,2) for P = 1, each point what a call on it alone gives."""
    from jarvis_hybridnet_amd.utils.reprojection import ReprojectionTool
    calib, pts = R.project_case("c4", 4, 17)
    dev = dev_calib(calib)
    tool = ReprojectionTool()
    tool.cameraMatrices, tool.intrinsicMatrices, tool.distortionCoefficients = dev
    abi = reproject(pts, dev)                                    # (C,P,2)
    many = tool.reprojectPoint(cuda(torch.from_numpy(pts)))
    torch.cuda.synchronize()
    assert many.shape == (4, 2, 17)
    assert np.array_equal(many.cpu().numpy().view(np.int32), abi.transpose(0, 2, 1).view(np.int32))
    for p in range(17):
        one = tool.reprojectPoint(cuda(torch.from_numpy(pts[p:p + 1])))
        torch.cuda.synchronize()
        assert one.shape == (4, 2)
        assert np.array_equal(one.cpu().numpy().view(np.int32), np.ascontiguousarray(abi[:, p, :]).view(np.int32)), p


# ---- jh_softargmax ----------------------------------------------------------------------------------------------------
def tail(x, c3, spacing, roi, final=True):
    """jh_softargmax on device tensors x (T,J,Gh,Gh,Gh), c3 (T,3) int32 -> host arrays points, conf, final (or None)."""
    N = native()
    T, J, Gh = x.shape[:3]
    pts = torch.full((T, J, 3), float("nan"), device="cuda")
    conf = torch.full((T, J), float("nan"), device="cuda")
    fin = torch.full((T, J, Gh, Gh, Gh), float("nan"), device="cuda") if final else None
    nb = N.lib().jh_softargmax_workspace_bytes(T, J, Gh)
    ws = N.workspace(nb, "cuda")
    N.check(N.lib().jh_softargmax(N.ptr(x), T, J, Gh, float(spacing), float(roi), N.ptr(c3), N.ptr(fin), N.ptr(pts),
                                  N.ptr(conf), N.ptr(ws), nb, N.stream()))
    torch.cuda.synchronize()
    return pts.cpu().numpy(), conf.cpu().numpy(), (fin.cpu().numpy() if final else None)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("kind", R.SOFT_KINDS)
@pytest.mark.parametrize("T,J,Gh", R.SOFT_SHAPES)
def test_softargmax_tail_against_float64(T, J, Gh, kind):
    x = R.soft_input(kind, T, J, Gh, 11 + Gh)
    c3 = R.soft_centres(T, Gh)
    assert T == 1 or not torch.equal(c3[0], c3[1])
    roi = 2 * Gh * R.SPACING
    xn, cn = x.numpy(), c3.numpy()
    ref = R.tail_def(xn, cn, R.SPACING, roi)
    _, bmm = R.softargmax_bounds(ref, cn, J, R.SPACING, roi)
    xd, cd = cuda(x), cuda(c3)
    pts, conf, fin = tail(xd, cd, R.SPACING, roi)
    rp = float((np.abs(pts.astype(np.float64) - ref["points"]) / bmm).max())
    rc = float((np.abs(conf.astype(np.float64) - ref["conf"]) / ref["conf"]).max() / R.U)
    rf = float((np.abs(fin.astype(np.float64) - ref["final"]) / ref["final"]).max() / R.U)
    report("softargmax_tail", shape=str((T, J, Gh)), kind=kind, points_err_over_bound=rp, conf_rel_ulp=rc,
           final_rel_ulp=rf, bound_mm_min=float(bmm.min()), bound_mm_max=float(bmm.max()))
    print("soft-argmax %s %s: points error / bound = %.3f (bound %.3g .. %.3g mm), conf %.3g u (bar 6), "
          "heatmap_final %.3g u (bar 10)" % ((T, J, Gh), kind, rp, bmm.min(), bmm.max(), rc, rf))
    assert rp <= 1.0
    assert rc * R.U <= R.CONF_REL
    assert fin.shape == (T, J, Gh, Gh, Gh) and rf * R.U <= R.FINAL_REL
    mx = xn.reshape(T, J, -1).max(-1)
    assert (conf[mx >= 255.0] == np.float32(1.0)).all()
    assert (conf[mx == 21.0] == np.float32(21) / np.float32(255)).all()
    if kind == "range":
        assert (mx >= 255.0).any() and ((mx == 21.0).any() or J == 1)
    # without heatmap_final: the same bits
    pts0, conf0, _ = tail(xd, cd, R.SPACING, roi, final=False)
    assert np.array_equal(bits(pts0), bits(pts)) and np.array_equal(bits(conf0), bits(conf))
    # row t of the batch: the T = 1 call on that row with its centre
    for t in range(T if T > 1 else 0):
        p1, c1, f1 = tail(xd[t:t + 1].contiguous(), cd[t:t + 1].contiguous(), R.SPACING, roi)
        assert np.array_equal(bits(p1[0]), bits(pts[t])) and np.array_equal(bits(c1[0]), bits(conf[t])), t
        assert np.array_equal(bits(f1[0]), bits(fin[t])), t
