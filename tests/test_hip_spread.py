"""GPU: per-joint 3D spread -- covariance, peak and mass of the V2V heat map (jh_softargmax_spread,
jh_predictor_set_spread / _get_spread; include/jarvis_hip.h).

The definition is the contract (the reference computes the mean and throws the rest away), so the op is held to a numpy
float64 evaluation of it, and the predictor to the op run on the predictor's own V2V output (jh_predictor_debug_v2v):

  cov   per element within 16 * 2^-24 * trace(cov_ref).  Device softplus (expf <= 1 ulp, log1pf <= 2 ulp, compounded)
        is within 4 fp32 ulp of the float64 weight; a relative weight error e moves cov_ab by at most 2 e trace; with the
        output rounding that is <= 9 * 2^-24 * trace, and 16 leaves under 2x margin.  The ten sums are fp64 and exact
        across workgroups, so nothing else contributes.
  peak  EQUAL to np.argmax(x) (first among equal maxima) mapped by the points' expression in float32.
  mass  within 2^-22 relative of the float64 sum: float32 of the op's own exact fp64 S_0 (4-ulp weights average far
        below that).  It is NOT the bits of the float the points are divided by: that one comes from fp32 block sums and
        is 1.6 x 2^-22 off the float64 sum at (2,1,6), where one block adds 128 rows in fp32 (measured).

Shapes (T, J, Gh) for the places the kernel can go wrong: (2,1,6): Jp = 8, q = 2, P = 216 smaller than one block;
(1,23,9): q = 6 leaves 4 idle lanes, P = 729 a ragged last block; (2,30,16): q = 8; (1,23,24): the cfg2 geometry.
The predictor tests run on cfg2 through tests/test_hip_centers.py's shared predictor and frame sets.
forward_uint8: the uint8 and the fp32 entry points differ by the frame conversion's 1 ulp per sample (the existing parity,
tests/test_hip_predictor.py, holds them to 1e-3 mm, not to bits), so the uint8 call is held to what can be exact: its
own bits with the spread off, and the op on its own V2V output.
Every test calls a symbol or passes a keyword that does not exist without the feature."""
import csv
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests.gpu_util import cuda, report

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 6), (1, 23, 9), (2, 30, 16), (1, 23, 24)]
SPACING = 2.0
MIRROR = [0, 1, 2, 1, 3, 4, 2, 4, 5]                   # xx xy xz yy yz zz -> the symmetric 3 x 3


def TC():
    from tests import test_hip_centers
    return test_hip_centers


def make_input(kind, T, J, Gh, seed):
    """x (T,J,Gh,Gh,Gh) float32 on the CPU.  'rand': rand * 3, the convention of tests/test_hip_stages.py, with the
    maximum of every map planted TWICE (the lower flat index must win) and map (0, 0) shifted below zero (the arg-max
    key of negative floats).  'peaked': background -30 plus 40 exp(-q / 2), q an anisotropic Gaussian form correlated
    in (i, j), random centre >= 2 voxels inside the cube, sigma in [0.7, 2.2] voxels: swapped axes, a wrong
    off-diagonal sign and wrong units all show."""
    g = torch.Generator().manual_seed(seed)
    if kind == "rand":
        x = torch.rand(T, J, Gh, Gh, Gh, generator=g) * 3
        flat = x.view(T, J, -1)
        for t in range(T):
            for j in range(J):
                a, b = torch.randperm(Gh ** 3, generator=g)[:2].tolist()
                flat[t, j, a] = flat[t, j, b] = 3.5
        x[0, 0] -= 10.0
        return x.contiguous()
    ax = torch.arange(Gh, dtype=torch.float64)
    I, Jx, K = torch.meshgrid(ax, ax, ax, indexing="ij")
    x = torch.empty(T, J, Gh, Gh, Gh, dtype=torch.float64)
    for t in range(T):
        for j in range(J):
            r = torch.rand(7, generator=g, dtype=torch.float64)
            c = 2.0 + r[:3] * (Gh - 1 - 4.0)
            s = 0.7 + r[3:6] * 1.5
            rho = (r[6] - 0.5) * 1.2
            di, dj, dk = (I - c[0]) / s[0], (Jx - c[1]) / s[1], (K - c[2]) / s[2]
            q = (di * di - 2 * rho * di * dj + dj * dj) / (1 - rho * rho) + dk * dk
            x[t, j] = -30.0 + 40.0 * torch.exp(-q / 2)
    return x.float().contiguous()


def reference(x, c3, spacing, roi):
    """numpy float64 of the definition -> cov (T,J,3,3) mm^2, peak (T,J,3) float32 mm, mass (T,J) float64."""
    xn = x.numpy()
    T, J, Gh = xn.shape[:3]
    xd = xn.astype(np.float64)
    h = np.where(xd > 20, xd, np.log1p(np.exp(np.minimum(xd, 20.0))))
    ax = np.arange(Gh, dtype=np.float64)
    grids = np.meshgrid(ax, ax, ax, indexing="ij")
    S0 = h.sum(axis=(2, 3, 4))
    m = [(h * g).sum(axis=(2, 3, 4)) / S0 for g in grids]
    # S_ab / S_0 - m_a m_b, evaluated about the mean: the same number without the reference's own cancellation error
    # (1e-16 * 400 voxel^2 would be the whole bar for a joint as sharp as one voxel)
    d = [g - ma[:, :, None, None, None] for g, ma in zip(grids, m)]
    cov = np.empty((T, J, 3, 3))
    for a in range(3):
        for b in range(3):
            cov[..., a, b] = (h * d[a] * d[b]).sum(axis=(2, 3, 4)) / S0 * (2 * spacing) ** 2
    p = np.argmax(xn.reshape(T, J, -1), axis=2)
    vox = np.stack([p // (Gh * Gh), (p // Gh) % Gh, p % Gh], axis=-1).astype(np.float32)
    f = np.float32
    peak = ((vox * f(spacing)) * f(2) - f(roi) / f(2)) + c3.numpy().astype(np.float32)[:, None, :]
    return cov, peak.astype(np.float32), S0


def op(x, c3, spacing, roi, spread=True):
    """jh_softargmax_spread (or jh_softargmax) on device tensors -> dict of device tensors."""
    from jarvis_hybridnet_amd import _native as N
    T, J, Gh = x.shape[:3]
    L = N.lib()
    out = dict(points=torch.empty((T, J, 3), device="cuda"), conf=torch.empty((T, J), device="cuda"))
    if not spread:
        ws = N.workspace(L.jh_softargmax_workspace_bytes(T, J, Gh), "cuda")
        N.check(L.jh_softargmax(x.data_ptr(), T, J, Gh, float(spacing), float(roi), c3.data_ptr(), None,
                                out["points"].data_ptr(), out["conf"].data_ptr(), ws.data_ptr(), ws.numel(),
                                N.stream()))
        return out
    out.update(cov6=torch.empty((T, J, 6), device="cuda"), peak=torch.empty((T, J, 3), device="cuda"),
               mass=torch.empty((T, J), device="cuda"))
    ws = N.workspace(L.jh_softargmax_spread_workspace_bytes(T, J, Gh), "cuda")
    N.check(L.jh_softargmax_spread(x.data_ptr(), T, J, Gh, float(spacing), float(roi), c3.data_ptr(), None,
                                   out["points"].data_ptr(), out["conf"].data_ptr(), out["cov6"].data_ptr(),
                                   out["peak"].data_ptr(), out["mass"].data_ptr(), ws.data_ptr(), ws.numel(),
                                   N.stream()))
    out["cov"] = out["cov6"][..., MIRROR].reshape(T, J, 3, 3)
    return out


def centres_int(T, seed):
    return torch.randint(-600, 600, (T, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


# ---- 1, 2: the op ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rand", "peaked"])
@pytest.mark.parametrize("T,J,Gh", SHAPES)
def test_op_against_float64(T, J, Gh, kind):
    x = make_input(kind, T, J, Gh, 7 + Gh)
    c3 = centres_int(T, Gh)
    roi = 2 * Gh * SPACING
    cov_ref, peak_ref, mass_ref = reference(x, c3, SPACING, roi)
    got = op(cuda(x), cuda(c3), SPACING, roi)
    torch.cuda.synchronize()
    cov = got["cov"].cpu().double().numpy()
    trace = np.trace(cov_ref, axis1=2, axis2=3)
    ratio = float((np.abs(cov - cov_ref) / (2.0 ** -24 * trace[..., None, None])).max())
    mass_rel = float((np.abs(got["mass"].cpu().double().numpy() - mass_ref) / mass_ref).max())
    report("spread_op_vs_float64", shape=str((T, J, Gh)), kind=kind, cov_err_over_ulp_trace=ratio,
           mass_rel_over_2_pow_minus_22=mass_rel * 2.0 ** 22)
    print("spread op %s %s: max |cov - ref| = %.3g x 2^-24 trace (bar 16), mass rel %.3g x 2^-22 (bar 1)"
          % ((T, J, Gh), kind, ratio, mass_rel * 2.0 ** 22))
    assert np.array_equal(got["peak"].cpu().numpy(), peak_ref)
    assert mass_rel <= 2.0 ** -22
    assert ratio <= 16.0
    # the six values are mirrored into a symmetric matrix whose diagonal is a variance
    assert torch.equal(got["cov"], got["cov"].transpose(2, 3)) and bool((got["cov"].diagonal(dim1=2, dim2=3) > 0).all())


@pytest.mark.parametrize("T,J,Gh", SHAPES)
def test_op_leaves_the_mean_alone(T, J, Gh):
    x, c3 = cuda(make_input("rand", T, J, Gh, 3 + Gh)), cuda(centres_int(T, Gh))
    roi = 2 * Gh * SPACING
    plain = op(x, c3, SPACING, roi, spread=False)
    a = {k: v.clone() for k, v in op(x, c3, SPACING, roi).items()}
    b = op(x, c3, SPACING, roi)
    torch.cuda.synchronize()
    assert torch.equal(a["points"], plain["points"]) and torch.equal(a["conf"], plain["conf"])
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- the predictor (cfg2) ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def native(T, graph=None, precision=None):
    """A cfg2 native predictor of its own (not the shared JarvisPredictor3D's), kept for the module."""
    pr = TC().native(T, **({} if precision is None else {"precision": precision}))
    if graph is not None:
        pr.graph_replay = graph
    return pr


def frames(T):
    return cuda(TC().setup()[4][:T])


def call(pr, x, **kw):
    """One forward -> dict of clones; with return_spread the Spread3D's three tensors too."""
    res = pr.forward(x, **kw)
    out = dict(points=res[0], conf=res[1], valid=res[2])
    if kw.get("return_spread"):
        out.update(res[3]._asdict())
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def op_on_own_v2v(pr):
    """jh_softargmax_spread on the V2V output and the integer centres the predictor's last call used."""
    c = TC().setup()[0]
    v2v = pr.debug_v2v("cuda")
    c3i = pr.debug("cuda")["center3d_int"][:pr.T3].contiguous()
    return op(v2v, c3i, float(c["spacing"]), float(c["roi"]))


def assert_spread(got, want, what=""):
    same = TC().same
    for k in ("cov", "peak", "mass"):
        assert same(got[k], want[k]), (k, what)


@pytest.mark.parametrize("T,graph", [(1, True), (3, None)])
def test_predictor_equals_the_op_on_its_own_v2v(T, graph):
    same = TC().same
    pr = native(T, graph)
    assert pr.graph_replay == bool(graph)
    x = frames(T)
    off = call(pr, x)
    on = call(pr, x, return_spread=True)
    assert off["valid"].tolist() == [1] * T
    for k in ("points", "conf", "valid"):
        assert same(on[k], off[k]), k
    want = op_on_own_v2v(pr)
    torch.cuda.synchronize()
    assert_spread(on, want)
    assert same(want["points"], on["points"]) and same(want["conf"], on["conf"])
    assert on["cov"].shape == (T, 23, 3, 3) and bool(torch.isfinite(on["cov"]).all())
    # how far mode and mean are apart, against the spread: for the record
    d = (on["peak"] - on["points"]).norm(dim=-1)
    report("spread_cfg2", T=T, trace_mm2_max=float(on["cov"].diagonal(dim1=2, dim2=3).sum(-1).max()),
           peak_minus_point_mm_max=float(d.max()))


def test_reproducibility_graph_batch_rows_and_alternation():
    same = TC().same
    g, e, b3 = native(1, True), native(1, False), native(3)
    x3 = frames(3)
    batch = call(b3, x3, return_spread=True)
    for t in range(3):
        x = x3[t:t + 1].contiguous()
        rg, re = call(g, x, return_spread=True), call(e, x, return_spread=True)
        assert_spread(rg, re, "graph replay vs eager, frame set %d" % t)
        for k in ("cov", "peak", "mass", "points", "conf"):
            assert same(batch[k][t], rg[k][0]), (k, t)
    # alternation on the graph-replaying predictor: both recordings live side by side (graph slots of their own),
    # every call gives its own result again -- compared, as tests/test_hip_centers.py compares its alternation
    x = x3[:1].contiguous()
    first_on, first_off = call(g, x, return_spread=True), call(g, x)
    for _ in range(2):
        on, off = call(g, x, return_spread=True), call(g, x)
        assert_spread(on, first_on)
        for k in ("points", "conf", "valid"):
            assert same(on[k], first_off[k]) and same(off[k], first_off[k]), k
    # ... and the getter still holds the last spread-on call after a spread-off one
    kept = g.spread()
    torch.cuda.synchronize()
    assert same(kept.cov, first_on["cov"]) and same(kept.peak, first_on["peak"]) and same(kept.mass, first_on["mass"])


def test_composition():
    tc = TC()
    same = tc.same
    c, inp, pred, calib, fr = tc.setup()
    x = frames(3)
    base = pred.forward_batch(x, *calib, return_spread=True)
    pr = pred.native(c["H"], c["W"], time_batch=3)
    centres = pr.debug("cuda")["center3d"].clone()
    torch.cuda.synchronize()
    assert len(base) == 4 and base[2].tolist() == [1, 1, 1]
    base = [base[0].clone(), base[1].clone(), base[2].clone(), type(base[3])(*(t.clone() for t in base[3]))]

    def check(res, what):
        for a, b in zip(res[:3], base[:3]):
            assert same(a, b), what
        for a, b in zip(res[-1], base[3]):
            assert same(a, b), what
    check(pred.forward_batch(x, *calib, return_spread=True, centers=centres), "centers")
    check(pred.forward_batch(x, *calib, return_spread=True, camera_mask=torch.ones(3, c["C"], dtype=torch.uint8)),
          "camera_mask")
    both = pred.forward_batch(x, *calib, return_2d=True, return_spread=True)
    views = pred.forward_batch(x, *calib, return_2d=True)[3]
    torch.cuda.synchronize()
    assert len(both) == 5
    check(both, "return_2d")
    for a, b in zip(both[3], views):
        assert same(a, b)
    # uint8 frames (see the module docstring): the call's own bits with the spread off, the op on its own V2V output
    x8 = cuda(tc.to_u8(fr[:1]))[0]
    p8, c8, s8 = pred.forward_uint8(x8, *calib, return_spread=True)
    want = op_on_own_v2v(pred.native(c["H"], c["W"]))
    p0, c0 = pred.forward_uint8(x8, *calib)
    torch.cuda.synchronize()
    assert same(p8, p0) and same(c8, c0)
    assert_spread(s8._asdict(), want, "forward_uint8")


def test_invalid_frame_set():
    tc = TC()
    same = tc.same
    c, inp, pred, calib, fr = tc.setup()
    x = frames(3)
    pr = pred.native(c["H"], c["W"], time_batch=3)
    pred.forward_batch(x, *calib)
    K = pr.debug("cuda")["center3d"].clone()
    good = [t.clone() for t in pred.forward_batch(x, *calib, return_spread=True, centers=K)[3]]
    K[1, 0] = float("nan")
    _, _, valid, spread = pred.forward_batch(x, *calib, return_spread=True, centers=K)
    torch.cuda.synchronize()
    assert valid.tolist() == [1, 0, 1]
    for got, want in zip(spread, good):
        assert bool(torch.isnan(got[1]).all())
        assert same(got[0], want[0]) and same(got[2], want[2])
    assert pred(x[0], *calib, centers=[float("nan"), 0.0, 0.0], return_spread=True) == (None, None, None)
    assert pred(x[0], *calib, centers=[float("nan"), 0.0, 0.0], return_2d=True, return_spread=True) == (None,) * 4
    res = pred(x[0], *calib, return_spread=True)
    assert len(res) == 3 and res[2].cov.shape == (1, c["J"], 3, 3)


def test_a_predictor_that_never_asks():
    from jarvis_hybridnet_amd import _native as N
    pr = TC().native(1)
    size = lambda: int(N.lib().jh_predictor_device_bytes(pr.handle))           # noqa: E731
    before = size()
    pr.forward(frames(1))
    torch.cuda.synchronize()
    assert size() == before == pr.device_bytes
    pr.set_spread(True)
    T, J, Jp = 1, pr.J, pr.Jp
    assert size() - before == (T * Jp * 10 * 3 + T * Jp) * 8 + T * J * 10 * 4 and pr.device_bytes == size()
    grown = size()
    pr.set_spread(False)
    pr.set_spread(True)
    pr.forward(frames(1), return_spread=True)
    torch.cuda.synchronize()
    assert size() == grown


def test_driver(tmp_path):
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames, spread_row
    tc = TC()
    c, inp, pred, calib, fr = tc.setup()
    cfg = tc.make_cfg(c)
    J = c["J"]
    _, det = tc.detected(3)
    K = [det["center3d"][t].cpu() for t in range(3)]
    sets = [fr[t].numpy() for t in range(3)]

    def run(name, **kw):
        out = str(tmp_path / name)
        assert predict3D_frames(pred, iter(sets), *calib, cfg, out, centers=iter([K[0], None, K[2]]), **kw) == 3
        return out
    plain, spread = run("plain"), run("spread", output_spread=True)
    assert not os.path.exists(os.path.join(plain, "spread3D.csv"))
    assert open(os.path.join(plain, "data3D.csv"), "rb").read() == open(os.path.join(spread, "data3D.csv"), "rb").read()
    rows = open(os.path.join(spread, "spread3D.csv"), newline="").read().splitlines()
    assert len(rows) == 3
    for t in range(3):
        if t == 1:
            want = spread_row(None, None, J)
        else:
            p, cf, s = pred(cuda(fr[t]), *calib, centers=K[t], return_spread=True)
            torch.cuda.synchronize()
            want = spread_row(s.cov[0], s.peak[0], J)
        text = io.StringIO()
        csv.writer(text, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL, lineterminator="").writerow(want)
        assert rows[t] == text.getvalue(), t
        assert len(next(csv.reader([rows[t]]))) == 9 * J
    assert next(csv.reader([rows[1]])) == ["NaN"] * (9 * J)


def test_bf16x3_predictor():
    pr = native(1, None, "bf16x3")
    assert pr.precision == "bf16x3"
    on = call(pr, frames(1), return_spread=True)
    want = op_on_own_v2v(pr)
    torch.cuda.synchronize()
    assert on["valid"].tolist() == [1]
    assert_spread(on, want, "bf16x3")
