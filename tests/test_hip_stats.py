"""GPU: the InstanceNorm statistics every convolution, depthwise and stem launch emits -- per (image, channel) the sum s1 and
the sum of squares s2 of the raw y it stored -- read back through the test-only entries (jh_op_operand::out_sums_host,
jh_op_depthwise_ex, jh_op_stem) and held against the float64 sums of the y the SAME launch returned.

Rows, inputs, references and the depths d1, d2 with their derivations from the code: tests/stat_cases.py;
tests/test_stat_cases_cpu.py shows without a GPU that the float32 reference is within 1e-5 of float64, that the outputs
are off-centre (|mean| of 2 .. 4 sigma: every pixel carries about 1 / P of its channel's sums), that d 2^-24 P <= 1 / 8
(one dropped or double-counted pixel is at least eight bounds away) and that each row takes the form it names.

Bars.  y: 2e-5 of the maximum for the float32 kernels, 5e-5 in the bf16x3 modes (tests/operand_cases.py), for the stem
too (its first direct test).  Statistics: |s1 - sum v| <= d1 2^-24 sum |v|, |s2 - sum v^2| <= d2 2^-24 sum v^2 per (image,
channel).  Behind an InstanceNorm built from the emitted sums: 2e-4 (BAR_NORM_Y).  Pooled sums of the POOL depthwise
form: 1e-4 (BAR_NORM_POOL).

Measured on an MI355X (the report() lines conv_stats, depthwise_stats, stem_stats, stats_chain and stats_near_constant of
parity.jsonl): see DESIGN.md, section 3.2."""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

from tests import operand_cases as OC
from tests import stat_cases as SC
from tests.gpu_util import cuda, rel_err, report

pytestmark = pytest.mark.gpu

KNOBS = ("JH_WINO", "JH_WINO_PW", "JH_DECONV4_WINDOW")


class Out:
    def __init__(self, y, sums, pool=None):
        self.y, self.sums, self.pool = y, sums, pool


@contextlib.contextmanager
def row_settings(cs):
    """The knobs and the precision mode of a row, for the duration of its launch (both are read when a layer is made)."""
    from jarvis_hybridnet_amd import _native as N
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(dict(cs.env))
    prev = N.set_precision(SC.PRECISIONS[cs.prec])
    try:
        yield
    finally:
        N.set_precision(prev)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_conv(cs, case, x=None):
    """One jh_op_conv_operand launch of the row with want_stats and out_sums_host -> Out (CPU tensors)."""
    from jarvis_hybridnet_amd import _native as N
    import ctypes
    r = cs.row
    x = case.x if x is None else x
    n = x.shape[0]
    sums = torch.full((n, r.cout, 2), float("nan"), dtype=torch.float64)
    opd = N.OpOperand(latency_class=cs.lat, want_stats=1, out_sums_host=sums.data_ptr())
    keep = []
    if cs.gate:
        pool, inv_hw, params = case.recipe
        assert pool.shape[0] == n
        keep = [OC.sums(x), pool.contiguous()] + [p.contiguous() for p in params]
        opd.in_sums_host, opd.in_act = keep[0].data_ptr(), OC.SILU
        opd.se_c, opd.se_s, opd.se_inv_hw = params[0].shape[1], params[0].shape[0], inv_hw
        opd.se_pool_host = keep[1].data_ptr()
        opd.se_wr_host, opd.se_br_host, opd.se_we_host, opd.se_be_host = (p.data_ptr() for p in keep[2:])
    d = x.shape[2] if r.nd == 3 else 1
    xc = cuda(x)
    y = torch.full((n, r.cout) + SC.out_shape(r), float("nan"), device="cuda")
    wh, bh = case.w.contiguous(), (case.b.contiguous() if case.b is not None else None)
    with row_settings(cs):
        N.check(N.lib().jh_op_conv_operand(r.nd, r.kind, r.k, r.stride, SC.pad_of(r), r.cin, r.cout, wh.data_ptr(),
                                           bh.data_ptr() if bh is not None else None, xc.data_ptr(), n, d, x.shape[-2],
                                           x.shape[-1], None, ctypes.byref(opd), y.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    return Out(y.cpu(), sums)


def run_dw(row, case, x=None):
    from jarvis_hybridnet_amd import _native as N
    k, c, h, w, want_pool = row
    x = case.x if x is None else x
    n = x.shape[0]
    xc = cuda(x)
    y = torch.full((n, c, h, w), float("nan"), device="cuda")
    sums = torch.full((n, c, 2), float("nan"), dtype=torch.float64)
    pool = torch.full((n, c), float("nan"), dtype=torch.float64)
    N.check(N.lib().jh_op_depthwise_ex(k, c, case.w.contiguous().data_ptr(), xc.data_ptr(), n, h, w, want_pool,
                                       y.data_ptr(), sums.data_ptr(), pool.data_ptr() if want_pool else None,
                                       N.stream()))
    torch.cuda.synchronize()
    return Out(y.cpu(), sums, pool if want_pool else None)


def run_stem(row, case, x=None):
    from jarvis_hybridnet_amd import _native as N
    cout, h, w = row
    x = case.x if x is None else x
    n = x.shape[0]
    xc = cuda(x)
    y = torch.full((n, cout, h // 2, w // 2), float("nan"), device="cuda")
    sums = torch.full((n, cout, 2), float("nan"), dtype=torch.float64)
    N.check(N.lib().jh_op_stem(cout, case.w.contiguous().data_ptr(), xc.data_ptr(), n, h, w, y.data_ptr(),
                               sums.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    return Out(y.cpu(), sums)


_RUNS = {}


def once(key, run):
    """A row on the GPU, once: y and the statistics come from ONE launch, as a consumer gets them."""
    if key not in _RUNS:
        _RUNS[key] = run()
    return _RUNS[key]


def conv_run(cs):
    return once(("conv", cs.id), lambda: run_conv(cs, SC.conv_case(cs)))


def dw_run(row):
    return once(("dw", row), lambda: run_dw(row, SC.dw_case(row)))


def stem_run(row):
    return once(("stem", row), lambda: run_stem(row, SC.stem_case(row)))


def check_row(kind, name, out, ref, bar, d1, d2, **more):
    e = rel_err(out.y, ref)
    nan = bool(torch.isnan(out.y).any())
    e1, b1, e2, b2, worst = SC.stat_errors(out.y, out.sums, d1, d2)
    report(kind, row=name, s1_err=e1, s1_bound=b1, s2_err=e2, s2_bound=b2, rel=e, over_bound=worst, **more)
    print("%s %s rel=%.3g s1 %.3g / %.3g s2 %.3g / %.3g worst error / bound %.3g"
          % (kind, name, e, e1, b1, e2, b2, worst))
    assert not nan, "an output element nobody stored"
    assert e < bar, (name, e)
    assert e1 <= b1 and e2 <= b2 and worst <= 1.0, (name, e1, b1, e2, b2, worst)


# ---- (a) per row
@pytest.mark.parametrize("cid", [c.id for c in SC.CONV_STATS])
def test_conv_statistics(cid):
    """y against float64, no element left unwritten, and the emitted sums against the float64 sums of that y within the
    depth of the row's code path (tests/stat_cases.py)."""
    cs = SC.CONV_BY_ID[cid]
    out = conv_run(cs)
    d1, d2 = SC.conv_depth(cs, out.y)
    check_row("conv_stats", cid, out, SC.conv_case(cs).ref, OC.BAR_BF16X3 if cs.prec else OC.BAR_FP32, d1, d2,
              path=cs.path, mr=cs.mr)


@pytest.mark.parametrize("row", SC.DW_ROWS, ids=SC.dw_id)
def test_depthwise_statistics(row):
    """... and, in the POOL form, the pooled sums against float64 silu(instance_norm(y)).sum() of the returned y: `tot`,
    the statistics they are normalised with, is the emitted partial."""
    out = dw_run(row)
    e_pool = 0.0
    if row[4]:
        e_pool = rel_err(out.pool, F.silu(F.instance_norm(out.y.double(), eps=1e-5)).sum((2, 3)))
    check_row("depthwise_stats", SC.dw_id(row), out, SC.dw_case(row).ref, OC.BAR_FP32, *SC.dw_depth(row[2], row[3]),
              tile=SC.dw_tile(row[2], row[3]), pool_rel=e_pool)
    assert (out.pool is not None) == bool(row[4])
    assert e_pool < OC.BAR_NORM_POOL, (row, e_pool)


@pytest.mark.parametrize("row", SC.STEM_ROWS, ids=SC.stem_id)
def test_stem_statistics(row):
    """stem_conv_kernel<0, 0, 16 | 32> against F.conv2d(x, w, None, 2, 1) in float64 (the reference of
    tests/stat_cases.py: make_stem) and its statistics: fp64 from the first addition on."""
    case, out = SC.stem_case(row), stem_run(row)
    assert rel_err(case.ref, F.conv2d(case.x.double(), case.w.double(), None, 2, 1)) == 0.0
    check_row("stem_stats", SC.stem_id(row), out, case.ref, OC.BAR_FP32, *SC.STEM_DEPTH)


# ---- (b) as a consumer gets it
def norm_with_emitted(out):
    """jh_op_norm_apply (the `materialise` form) on the kernel's own y with the sums the kernel emitted."""
    from jarvis_hybridnet_amd import _native as N
    y = out.y
    n, c = y.shape[:2]
    d = y.shape[2] if y.dim() == 5 else 1
    yc = cuda(y)
    res = torch.full(y.shape, float("nan"), device="cuda")
    sums = out.sums.contiguous()
    N.check(N.lib().jh_op_norm_apply(yc.data_ptr(), n, c, d, y.shape[-2], y.shape[-1], sums.data_ptr(), OC.NONE, None,
                                     None, None, 1, 0, 0, res.data_ptr(), None, N.stream()))
    torch.cuda.synchronize()
    return res.cpu()


def check_chain(name, out, const=None):
    got = norm_with_emitted(out)
    e = rel_err(got, F.instance_norm(out.y.double(), eps=1e-5))
    report("stats_chain", row=name, rel=e, bar=OC.BAR_NORM_Y)
    print("stats_chain %s rel=%.3g" % (name, e))
    assert torch.isfinite(got).all()
    assert e < OC.BAR_NORM_Y, (name, e)
    if const is not None:
        # the constant channel of image 0: the variance the sums give is noise far below eps (clamped where negative),
        # rstd = 1 / sqrt(eps), and the normalised channel stays at 0 within the bar
        P = SC.pixels(out.y.shape[2:])
        var = SC.near_variance(out.sums[0, const], P).item()
        v = out.y[0, const].double()
        assert (v.max() - v.min()).item() == 0.0
        assert abs(var) < 1e-7, var
        assert got[0, const].abs().max().item() < OC.BAR_NORM_Y * F.instance_norm(out.y.double(), eps=1e-5).abs().max()


@pytest.mark.parametrize("cid", [c.id for c in SC.CONV_STATS])
def test_conv_chain(cid):
    cs = SC.CONV_BY_ID[cid]
    check_chain(cid, conv_run(cs), SC.CO_CONST if cs.const else None)


@pytest.mark.parametrize("row", SC.DW_ROWS, ids=SC.dw_id)
def test_depthwise_chain(row):
    check_chain("dw_" + SC.dw_id(row), dw_run(row), OC.CONST_CHANNEL if row == SC.DW_CONST else None)


@pytest.mark.parametrize("row", SC.STEM_ROWS, ids=SC.stem_id)
def test_stem_chain(row):
    check_chain("stem_" + SC.stem_id(row), stem_run(row), SC.CO_CONST if row == SC.STEM_CONST else None)


# ---- (c) image count: one row per code path
TWICE_CONV = ["k3_8x16", "deconv4_88_23", "pwd_16_8", "wino_6_23", "wino_pw_18"]
TWICE_DW = [SC.DW_ROWS[2], SC.DW_ROWS[5]]        # four ragged 16-tiles; the POOL form on the 20-tile
TWICE_STEM = [SC.STEM_ROWS[3]]


def check_twice(one, two, n):
    assert torch.equal(two.y[:n], one.y)
    assert torch.equal(two.sums[:n], one.sums)
    assert one.pool is None or torch.equal(two.pool[:n], one.pool)
    assert not torch.equal(two.y[n:], one.y)                 # (the other images are other images)


def test_twice_covers_every_code_path():
    assert [SC.CONV_BY_ID[c].path for c in TWICE_CONV] == ["epilogue2d", "epilogue2d", "pw_direct", "wino", "wino_pw"]
    assert len(TWICE_CONV) + len(TWICE_DW) + len(TWICE_STEM) == 8


@pytest.mark.parametrize("cid", TWICE_CONV)
def test_conv_image_count_does_not_change_the_bits(cid):
    """No sum's grouping depends on the batch: the same n images first in a launch of 2 n give the same y and the same
    statistics, bit for bit."""
    cs = SC.CONV_BY_ID[cid]
    case, one = SC.conv_case(cs), conv_run(cs)
    n = cs.row.n
    other = SC.make_conv(cs, SC.conv_seed(cs) + 424243)
    check_twice(one, run_conv(cs, case, x=torch.cat([case.x, other.x])), n)


@pytest.mark.parametrize("row", TWICE_DW, ids=SC.dw_id)
def test_depthwise_image_count_does_not_change_the_bits(row):
    case, one = SC.dw_case(row), dw_run(row)
    other = SC.make_dw(row, 424243 + row[1])
    check_twice(one, run_dw(row, case, x=torch.cat([case.x, other.x])), SC.DW_N)


@pytest.mark.parametrize("row", TWICE_STEM, ids=SC.stem_id)
def test_stem_image_count_does_not_change_the_bits(row):
    case, one = SC.stem_case(row), stem_run(row)
    other = SC.make_stem(row, 424243 + row[0])
    check_twice(one, run_stem(row, case, x=torch.cat([case.x, other.x])), SC.STEM_N)


# ---- (d) persistent against one-role Winograd
@pytest.mark.parametrize("cid", ["wino_pw_16", "wino_pw_18"])
def test_winograd_forms_emit_the_same_sums(cid):
    """JH_WINO_PW on and off: the persistent kernel's tile lists and the one-role kernel's grid cut the volume into the
    same tiles, so y and the float32 partials, hence the sums, are the same bits."""
    pw, one_role = conv_run(SC.CONV_BY_ID[cid]), conv_run(SC.CONV_BY_ID[cid + "_one_role"])
    assert torch.equal(pw.y, one_role.y)
    assert torch.equal(pw.sums, one_role.sums)


# ---- (e) nearly constant channels
@pytest.mark.parametrize("path", sorted(SC.NEAR))
def test_nearly_constant_channels(path):
    """What the fp64 partials of the 2D producers exist for (csrc/jh_common.h, above exact_add_rounded): a channel whose
    sigma is a small fraction of its mean -- here |mean| / sigma of about 300 -- still gets its variance.  The variance
    a consumer derives, s2 / P - (s1 / P)^2, is held against the float64 variance of the returned y, per (image,
    channel), with mean, A = sum |v|, Q = sum v^2 and R = max |v - mean| of that channel:

        |var' - var| <= 2^-31 Q / P + 2 |mean| 2^-31 A / P + 4 (a + b) 2^-24 R^2 + e1^2 + 2^-48 Q / P,
        e1 = 2^-31 A / P + 2 a 2^-24 R.

    Terms one and two: exact_add_rounded keeps 2^-31 relative per partial, so at most 2^-31 Q on s2 and 2^-31 A on s1;
    the square of s1 / P turns the latter into 2 |mean| times it.  Term three, the pivoted float32 sums: a lane with
    pivot m computes D1 ~ sum d and D2 ~ sum d^2, d = v - m, with errors eps1, eps2, and hands on cnt m + D1 and
    cnt m^2 + 2 m D1 + D2 in fp64.  In var' the shared error cancels down to the spread:
    (2 m eps1 + eps2) - 2 mean eps1 = 2 (m - mean) eps1 + eps2, and with the pivot one of the channel's values,
    |m - mean| <= R and |d| <= 2 R, so |eps1| <= a u cnt 2 R and |eps2| <= b u cnt 4 R^2: summed over the lanes and divided
    by P, 4 (a + b) u R^2.  a, b: the float32 roundings on sum |d| and sum d^2 of the path (tests/stat_cases.py: NEAR; the
    stem has none).  Term four is the second-order term of the square, term five the fp64 roundings of the un-shift
    and of the lane, wave and LDS sums (fewer than 2^5 of 2^-53 each).  Everything else -- limb atomics, the reader --
    is exact.

    tests/test_stat_cases_cpu.py shows on these very inputs that float32 partials, at their best, miss this bar by
    more than 8 x.  The 3D kernels hand on float32 partials by design (their channels are never nearly constant: every
    V2V layer sees the heat maps' voxel grid) and are not part of this test."""
    key, a, b = SC.NEAR[path]
    case = SC.near_case(path)
    if path in ("epilogue2d", "pw_direct"):
        cs = SC.CONV_BY_ID[key]._replace(const=False)
        out = run_conv(cs, case)
        assert cs.path == path
    elif path == "depthwise":
        out = run_dw(key, case)
    else:
        out = run_stem(key, case)
    e = rel_err(out.y, case.ref)
    assert not torch.isnan(out.y).any() and e < OC.BAR_FP32, (path, e)
    P = SC.pixels(out.y.shape[2:])
    var = out.y.double().flatten(2).var(2, unbiased=False)
    err = (SC.near_variance(out.sums, P) - var).abs()
    bar = SC.near_bar(out.y, a, b)
    ratio = SC.offcentre_ratio(out.y.double())
    worst = (err / bar).max().item()
    report("stats_near_constant", path=path, ratio=ratio.median().item(), var_rel_err=(err / var).max().item(),
           var_rel_bar=(bar / var).max().item(), over_bar=worst, rel=e)
    print("stats_near_constant %s |mean| / sigma %.0f var err / var %.3g bar / var %.3g err / bar %.3g"
          % (path, ratio.median(), (err / var).max(), (bar / var).max(), worst))
    assert worst <= 1.0, (path, worst)
