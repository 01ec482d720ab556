"""CPU: the inputs and the float64 reference of tests/test_hip_operand.py, checked without a GPU.

For every row the reference expression evaluated in torch float32 agrees with its float64 form within 1e-5 of the
output's magnitude -- half the 2e-5 bar the kernels are held to, so the reference alone stays inside it -- and the
generated inputs really are what the rows promise: |mean| >= 2 sigma (and <= 4 sigma) in every (image, channel), the
constant channel where a row says so."""
import pytest
import torch

from tests import operand_cases as OC
from tests.gpu_util import rel_err


def _check_input(x, const):
    dims = tuple(range(2, x.dim()))
    xd = x.double()
    mean, sigma = xd.mean(dims), xd.var(dims, unbiased=False).sqrt()
    keep = torch.ones_like(mean, dtype=torch.bool)
    if const:
        assert torch.equal(x[0, OC.CONST_CHANNEL], torch.full_like(x[0, OC.CONST_CHANNEL], OC.CONST_VALUE))
        keep[0, OC.CONST_CHANNEL] = False
    ratio = (mean.abs() / sigma)[keep]
    assert ratio.min() >= 2.0 and ratio.max() <= 4.0
    assert sigma[keep].min() >= 0.499 and sigma[keep].max() <= 2.001
    s = OC.sums(x)
    assert s.shape == x.shape[:2] + (2,) and s.dtype == torch.float64
    assert torch.allclose(s[..., 0] / x[0, 0].numel(), mean, rtol=1e-12, atol=0)


@pytest.mark.parametrize("rid", [r.id for r in OC.CONV_ROWS])
def test_conv_row_reference(rid):
    r = OC.BY_ID[rid]
    assert r.n >= 2
    x, w, b = OC.row_tensors(r)
    _check_input(x, r.const)
    for act in r.acts:
        gate64 = gate32 = None
        if r.se:
            pool, inv_hw, params, gate64 = OC.row_gate(r, x, act)
            gate32 = OC.se_gate_ref(pool, inv_hw, *params, dtype=torch.float32)
            assert rel_err(gate32, gate64) < 1e-5
        ref = OC.conv_ref(r, x, w, b, act, gate64)
        e = rel_err(OC.conv_ref(r, x, w, b, act, gate32, dtype=torch.float32), ref)
        assert e < 1e-5, (rid, act, e)


@pytest.mark.parametrize("rid", [r.id for r in OC.CONV_ROWS])
def test_conv_row_catches_the_mistakes(rid):
    """What the inputs are for: the two ways an operand transform goes wrong cost whole units on every row, four orders
    above the bar -- zero padding that is normalised with the image (rows with a neighbourhood), and statistics taken
    from another image."""
    import torch.nn.functional as F
    r = OC.BY_ID[rid]
    x, w, b = OC.row_tensors(r)
    act = r.acts[-1]
    ref = OC.conv_ref(r, x, w, b, act)
    dims = tuple(range(2, x.dim()))
    xd, wd, bd = x.double(), w.double(), (b.double() if b is not None else None)
    mean = xd.mean(dims, keepdim=True)
    rstd = 1.0 / (xd.var(dims, unbiased=False, keepdim=True) + 1e-5).sqrt()

    def conv(v, pad):
        if r.kind == 1:
            return F.conv_transpose2d(v, wd, bd, 2, 1)
        if r.kind == 2:
            return F.conv_transpose3d(v, wd, bd, 2, 0)
        return (F.conv2d if r.nd == 2 else F.conv3d)(v, wd, bd, r.stride, pad)

    swapped = OC.ACTS[act]((xd - mean.roll(1, 0)) * rstd.roll(1, 0))
    assert rel_err(conv(swapped, r.k // 2), ref) > 0.1
    if r.kind == 0 and r.k > 1:
        p = r.k // 2
        padded = OC.ACTS[act]((F.pad(xd, (p, p) * r.nd) - mean) * rstd)     # padding pixels become -mean * rstd
        assert rel_err(conv(padded, 0), ref) > 0.1


@pytest.mark.parametrize("C,S", OC.SE_GATE)
def test_se_gate_reference(C, S):
    """The float32 figure the kernel's bar is derived from: the kernel's own expression without fused multiply-adds
    against float64, on the test's inputs."""
    pool, inv_hw, params = OC.se_gate_case(C, S)
    ref = OC.se_gate_ref(pool, inv_hw, *params)
    e = rel_err(OC.se_gate_fp32_sequential(pool, inv_hw, *params), ref)
    print("se_gate fp32 sequential vs fp64: C=%d S=%d rel=%.3g" % (C, S, e))
    # (a quarter of slack for another host's vector exp: the written figure, not this run, sets the kernel's bar)
    assert 0 < e <= 1.25 * OC.SE_GATE_FP32_REF[(C, S)]
    assert ref.min() > 0.02 and ref.max() < 0.98 and ref.std() > 0.05      # gates that differ, none saturated


@pytest.mark.parametrize("C", OC.NORM_CHANNELS)
@pytest.mark.parametrize("shape", OC.NORM_SHAPES)
def test_norm_apply_reference(C, shape):
    x, r1, r2 = OC.norm_tensors(C, shape)
    _check_input(x, True)
    _check_input(r1, False)
    for form in OC.NORM_FORMS:
        y64, p64 = OC.norm_ref(form, x, r1, r2)
        y32, p32 = OC.norm_ref(form, x, r1, r2, dtype=torch.float32)
        # half of each bar of the GPU test (a normalised tensor carries the float32 error of its statistics:
        # the file bar "after an InstanceNorm"); pooled sums only where the form delivers them
        assert rel_err(y32, y64) < OC.BAR_NORM_Y / 2, form.id
        assert not form.pool or rel_err(p32, p64) < OC.BAR_NORM_POOL / 2, form.id
