"""CPU: the inputs and the float64 reference of tests/test_hip_node_outputs.py, checked without a GPU.

On one case per distinct (channels, level, variant) the reference expression evaluated in torch float32 agrees with its
float64 form within 1e-5 of the output's maximum -- half the 2e-5 bar the kernels are held to, so the bar is attainable
and the reference alone stays inside it -- and the generated tensors are what tests/node_cases.py promises: off-centre
inputs, one constant channel, a bias of 2 .. 4 output sigmas.  The statistics bound can see one pixel on every case."""
import pytest
import torch

from tests import node_cases as NC
from tests import operand_cases as OC
from tests.gpu_util import rel_err

CASES = NC.cases()


def _distinct():
    seen, out = set(), []
    for k in CASES:
        c, cout, h, w, modes = k.node[:5]
        key = (c, cout, h, w, modes, k.node[5])
        if key not in seen:
            seen.add(key)
            out.append(k)
    return out


@pytest.mark.parametrize("case", _distinct(), ids=lambda k: k.id)
def test_reference_conditioning(case):
    nd = NC.case_tensors(case)
    c, cout, h, w, modes, act, n = case.node
    assert n >= 2 and nd.ref.dtype == torch.float64 and nd.ref.shape == (n, cout, h, w)
    for i, (x, m) in enumerate(zip(nd.xs, modes)):
        assert x.shape == (n, c) + NC.input_shape(m, h, w) and x.dtype == torch.float32
        xd = x.double()
        mean, sigma = xd.mean((2, 3)), xd.var((2, 3), unbiased=False).sqrt()
        keep = torch.ones_like(mean, dtype=torch.bool)
        if i == 0:
            assert torch.equal(x[0, OC.CONST_CHANNEL], torch.full_like(x[0, OC.CONST_CHANNEL], OC.CONST_VALUE))
            keep[0, OC.CONST_CHANNEL] = False
        if x[0, 0].numel() > 1:
            ratio = (mean.abs() / sigma)[keep]
            assert ratio.min() >= 2.0 and ratio.max() <= 4.0
    # the bias: 2 .. 4 sigmas of the output without it, so every pixel carries about 1 / (H W) of its channel's sum
    y0 = nd.ref - nd.bias.double()[None, :, None, None]
    ratio = nd.bias.double().abs() / y0.var((0, 2, 3), unbiased=False).sqrt()
    assert ratio.min() >= 2.0 and ratio.max() <= 4.0
    e = rel_err(NC.node_fp32(case.node, nd), nd.ref)
    print("node fp32 vs fp64: %s rel=%.3g" % (case.id, e))
    assert e < 1e-5, (case.id, e)


@pytest.mark.parametrize("case", _distinct(), ids=lambda k: k.id)
def test_reference_catches_the_mistakes(case):
    """What the inputs are for.  Statistics taken from another image, or divided by another pixel count (a pooled tensor
    carries its producer's H W, four times its own), move y by more than 1e-2 of its maximum -- 500 bars; and in at
    least 99 % of the (image, channel, pixel) the value is larger than its channel's statistics bound, so losing or
    doubling that one pixel shows in the emitted sum."""
    nd = NC.case_tensors(case)
    modes, act = case.node[4], case.node[5]
    last = len(modes) - 1

    def with_last(v):
        vs = [OC.inorm(x, torch.float64) for x in nd.xs[:last]] + [v]
        return NC.node_expr(vs, modes, act, nd.wts, nd.dw, nd.pw, nd.bias, torch.float64)

    xd = nd.xs[last].double()
    px = xd[0, 0].numel()
    s1, s2 = xd.sum((2, 3), keepdim=True), (xd * xd).sum((2, 3), keepdim=True)

    def norm(s1, s2, count):
        mean = s1 / count
        return (xd - mean) / ((s2 / count - mean * mean).clamp_min(0.0) + 1e-5).sqrt()

    assert rel_err(with_last(norm(s1, s2, px)), nd.ref) < 1e-9
    assert rel_err(with_last(norm(s1.roll(1, 0), s2.roll(1, 0), px)), nd.ref) > 1e-2
    assert rel_err(with_last(norm(s1, s2, px * 4)), nd.ref) > 1e-2
    share = nd.ref.abs() / nd.ref.abs().sum((2, 3), keepdim=True)
    assert (share > NC.stat_depth(case.want)[0] * 2.0 ** -24).double().mean() > 0.99


def test_statistics_bound_sees_one_pixel():
    """d 2^-24 H W <= 1 / 8 on every case: with every pixel carrying about 1 / (H W) of its channel's sum, a dropped or
    double-counted pixel is at least eight bounds away."""
    for k in CASES:
        h, w = k.node[2], k.node[3]
        for d in NC.stat_depth(k.want):
            assert d >= 5 and d * 2.0 ** -24 * h * w <= 0.125, (k.id, d)
    for c, cls, levels in NC.CHAINS:
        for k in NC.chain_nodes(CASES, c, cls, levels):
            assert NC.stat_depth(k.want) == NC.stat_depth(NC.by_key(CASES, k.node[:6], k.cls, k.want_pool).want)
