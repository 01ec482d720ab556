"""CPU: the rows, inputs, references and bounds of tests/test_hip_stats.py, checked without a GPU.

For every row: the float32 evaluation of the reference stays within 1e-5 of float64 (half the bar the kernels are held to
and less); at least 90 % of the output (image, channel) are off-centre, |mean| of 2 .. 4 of their own sigma (the range is
printed); d 2^-24 P <= 1 / 8, so that one dropped or double-counted pixel -- about 1 / P of its channel's sums -- is at
least eight bounds away; and the row takes the form its comment says, wherever jh_conv_form can tell.  The bar of the
nearly-constant test separates fp64 partials from float32 partials on the very inputs the GPU test uses."""
import ctypes

import pytest
import torch

from tests import operand_cases as OC
from tests import stat_cases as SC
from tests.gpu_util import rel_err


def check_conditioning(name, ref, y32, d1, d2, const=None):
    P = SC.pixels(ref.shape[2:])
    assert ref.dtype == torch.float64 and P <= 4096
    e = rel_err(y32, ref)
    ratio = SC.offcentre_ratio(ref)
    keep = torch.ones_like(ratio, dtype=torch.bool)
    if const is not None:
        v = ref[0, const]
        assert (v.max() - v.min()).item() == 0.0 and v.flatten()[0].item() != 0.0, "the constant channel of image 0"
        keep[0, const] = False
    ok = ((ratio >= 2.0) & (ratio <= 4.0))[keep].double().mean().item()
    worst1, worst2 = float(torch.as_tensor(d1).max()), float(torch.as_tensor(d2).max())
    print("stat_case %s fp32 %.3g ratio %.2f .. %.2f (%.0f %% in 2 .. 4) d %.0f / %.0f P %d d u P %.3g / %.3g"
          % (name, e, ratio[keep].min(), ratio[keep].max(), 100 * ok, worst1, worst2, P, worst1 * SC.U * P,
             worst2 * SC.U * P))
    assert e < 1e-5, (name, e)
    assert ok >= 0.9, (name, ok)
    assert worst1 >= 1 and worst2 >= 1
    assert worst1 * SC.U * P <= 0.125 and worst2 * SC.U * P <= 0.125, (name, worst1, worst2, P)


@pytest.mark.parametrize("cid", [c.id for c in SC.CONV_STATS])
def test_conv_row(cid):
    cs = SC.CONV_BY_ID[cid]
    case = SC.conv_case(cs)
    r = cs.row
    assert case.ref.shape == (r.n, r.cout) + SC.out_shape(r)
    assert (case.b is not None) == r.bias
    d1, d2 = SC.conv_depth(cs, case.ref)
    check_conditioning(cid, case.ref, SC.conv_fp32(cs, case), d1, d2, SC.CO_CONST if cs.const else None)


@pytest.mark.parametrize("row", SC.DW_ROWS, ids=SC.dw_id)
def test_depthwise_row(row):
    case = SC.dw_case(row)
    d1, d2 = SC.dw_depth(row[2], row[3])
    check_conditioning(SC.dw_id(row), case.ref, SC._dw(case.x, case.w), d1, d2,
                       OC.CONST_CHANNEL if row == SC.DW_CONST else None)
    assert SC.dw_tile(row[2], row[3]) == (20 if row in (SC.DW_ROWS[3], SC.DW_ROWS[5], SC.DW_ROWS[6]) else 16)
    if row[4]:
        assert row[2] <= 20 and row[3] <= 20          # depthwise_can_pool


@pytest.mark.parametrize("row", SC.STEM_ROWS, ids=SC.stem_id)
def test_stem_row(row):
    case = SC.stem_case(row)
    check_conditioning(SC.stem_id(row), case.ref, SC._stem(case.x, case.w), *SC.STEM_DEPTH,
                       const=SC.CO_CONST if row == SC.STEM_CONST else None)


def test_one_constant_channel_per_2d_path():
    paths = sorted(c.path for c in SC.CONV_STATS if c.const)
    assert paths == ["epilogue2d", "pw_direct"]


KNOBS = ("JH_WINO", "JH_WINO_PW", "JH_DECONV4_WINDOW")


@pytest.mark.parametrize("cid", [c.id for c in SC.CONV_STATS])
def test_row_takes_its_form(cid, monkeypatch):
    """jh_conv_form tells the layer's form (the weight layout and the Winograd / bf16x3 kernels); the tile inside `mfma`
    and the one-role / persistent Winograd choice are launch-time decisions the row's comment derives from the shape."""
    from jarvis_hybridnet_amd import _native as N
    cs = SC.CONV_BY_ID[cid]
    r = cs.row
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cs.env:
        monkeypatch.setenv(k, v)
    name = ctypes.create_string_buffer(32)
    N.check(N.lib().jh_conv_form(r.nd, r.kind, r.k, r.stride, SC.pad_of(r), r.cin, r.cout, int(r.bias), 1,
                                 2 if cs.gate else 0, cs.prec, 0, name, len(name)))
    assert name.value.decode() == cs.form, (cid, name.value.decode())
    if cs.path == "pw_direct":
        # conv_pw_direct_eligible (csrc/conv_pw_direct.hip): at most 48 input channels, 1 or 4 column blocks, enough pixels
        P, nb = SC.pixels(r.shape), (r.cout + 15) // 16
        assert r.k == 1 and r.cin <= 48 and nb in (1, 4) and P % 16 == 0 and P >= (1024 if nb == 1 else 4096)


@pytest.mark.parametrize("path", sorted(SC.NEAR))
def test_near_constant_bar_separates_the_designs(path):
    """The bar of test_nearly_constant_channels on the float64 reference of the same inputs: sums whose partials are
    exact (what fp64 partials rounded to 2^-31 are, to the bar's first term) pass it trivially; sums whose partials are
    rounded to float32 -- the best a float32 partial can be: the exact sum of its pixels, rounded once -- miss it by at
    least 8 x in the worst (image, channel)."""
    key, a, b = SC.NEAR[path]
    case = SC.near_case(path)
    ref = case.ref
    P = SC.pixels(ref.shape[2:])
    ratio = SC.offcentre_ratio(ref)
    var = ref.flatten(2).var(2, unbiased=False)
    bar = SC.near_bar(ref, a, b)
    parts = SC.near_partials(path, ref)
    assert sum(p.shape[2] for p in parts) == P
    s1 = sum(p.sum(2).float().double() for p in parts)
    s2 = sum((p * p).sum(2).float().double() for p in parts)
    miss = ((SC.near_variance(torch.stack([s1, s2], -1), P) - var).abs() / bar).max().item()
    print("near_constant %s ratio %.0f .. %.0f (median %.0f) partials %d bar / var %.3g float32 partials miss by %.1f x"
          % (path, ratio.min(), ratio.max(), ratio.median(), len(parts), (bar / var).max(), miss))
    assert 0.8 * SC.NEAR_RATIO <= ratio.median() <= 1.25 * SC.NEAR_RATIO
    assert miss >= 8.0, (path, miss)
    # and the float32 evaluation of the reference is as good as on the other rows
    f32 = {"depthwise": SC._dw, "stem": SC._stem}.get(path) or (lambda x, w: SC._conv(OC.BY_ID[key], x, w, None))
    assert rel_err(f32(case.x, case.w), ref) < 1e-5
