"""GPU: every kernel's operand transform -- InstanceNorm + activation + squeeze-excite gate applied while the input is
staged -- at op level, against the same operation in float64.

The statistics are supplied from the host in float64 (jh_op_conv_operand, jh_op_norm_apply, jh_op_se_gate), so only the
consumer is under test.  Inputs (tests/operand_cases.py): n >= 2, every (image, channel) with its own sigma and a mean
of +-(2 .. 4) sigma, so that zero padding that is normalised instead of staying zero, K-padding channels that do not
stay zero and statistics indexed by the wrong image all cost whole units; one row per kernel family carries a constant
channel (variance 0: the clamp and rstd = 1 / sqrt(eps)).

Bars: the file-level bars of raw convolution outputs, rel_err < 2e-5 for float32 kernels and < 5e-5 in the bf16x3 modes
(tests/test_hip_ops.py, tests/test_hip_bf16x3.py).  The reference expression in torch float32 stays within 1e-5 of
float64 on these inputs (tests/test_operand_cases_cpu.py)."""
import ctypes

import pytest
import torch

from tests import operand_cases as OC
from tests.gpu_util import cuda, rel_err, report

pytestmark = pytest.mark.gpu

WINDOW_SWITCH = "JH_DECONV4_WINDOW"


def _conv(r, x, w, b, act, *, gate=None, recipe=None, lat=0, want_stats=0):
    """jh_op_conv_operand on a row: InstanceNorm(float64 sums of x) + act on load, gate as a device tensor (n, cin) or as
    the recipe (pool, inv_hw, (wr, br, we, be)); returns the raw output on the CPU."""
    from jarvis_hybridnet_amd import _native as N
    s = OC.sums(x)
    opd = N.OpOperand(in_sums_host=s.data_ptr(), in_act=act, latency_class=lat, want_stats=want_stats)
    keep = [s]
    if recipe is not None:
        pool, inv_hw, params = recipe
        keep += [pool.contiguous()] + [p.contiguous() for p in params]
        opd.se_c, opd.se_s, opd.se_inv_hw = params[0].shape[1], params[0].shape[0], inv_hw
        opd.se_pool_host = keep[1].data_ptr()
        opd.se_wr_host, opd.se_br_host, opd.se_we_host, opd.se_be_host = (p.data_ptr() for p in keep[2:])
    d = x.shape[2] if r.nd == 3 else 1
    h, wd = x.shape[-2:]
    if r.kind == 0:
        oshape = tuple((e + 2 * (r.k // 2) - r.k) // r.stride + 1 for e in x.shape[2:])
    else:
        oshape = tuple(2 * e for e in x.shape[2:])
    xc = cuda(x)
    y = torch.full((r.n, r.cout) + oshape, float("nan"), device="cuda")
    wh, bh = w.contiguous(), (b.contiguous() if b is not None else None)
    N.check(N.lib().jh_op_conv_operand(r.nd, r.kind, r.k, r.stride, r.k // 2 if r.kind == 0 else (1 if r.kind == 1 else 0),
                                       r.cin, r.cout, wh.data_ptr(), bh.data_ptr() if bh is not None else None,
                                       xc.data_ptr(), r.n, d, h, wd, N.ptr(gate), ctypes.byref(opd), y.data_ptr(),
                                       N.stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _se_gate(pool, inv_hw, params):
    """se_gate_kernel through jh_op_se_gate -> (n, C) on the device."""
    from jarvis_hybridnet_amd import _native as N
    n, (S, C) = pool.shape[0], params[0].shape
    host = [pool.contiguous()] + [p.contiguous() for p in params]
    gate = torch.full((n, C), float("nan"), device="cuda")
    N.check(N.lib().jh_op_se_gate(host[0].data_ptr(), n, C, S, inv_hw, *(p.data_ptr() for p in host[1:]),
                                  gate.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    return gate


def _window_launches():
    from jarvis_hybridnet_amd import _native as N
    return N.lib().jh_deconv4_window_launches()


@pytest.mark.parametrize("rid", [r.id for r in OC.CONV2D + OC.PW_DIRECT if not r.se])
def test_conv2d_norm_on_load(rid):
    """conv_mfma.h (every tile form, both latency classes where they differ) and conv_pw_direct.hip without a gate."""
    r = OC.BY_ID[rid]
    x, w, b = OC.row_tensors(r)
    for act in r.acts:
        ref = OC.conv_ref(r, x, w, b, act)
        for lat in r.lat:
            e = rel_err(_conv(r, x, w, b, act, lat=lat, want_stats=1), ref)
            report("operand_conv", row=rid, family=r.family, in_act=act, latency_class=lat, rel=e, bar=OC.BAR_FP32)
            assert e < OC.BAR_FP32, (rid, act, lat, e)


@pytest.mark.parametrize("rid", [r.id for r in OC.PROJECT + OC.PW_DIRECT if r.se])
def test_conv2d_silu_gate_on_load(rid):
    """The project convolutions: SiLU + squeeze-excite gate, the gate as a tensor (from se_gate_kernel) and as the recipe
    the kernel's prologue evaluates -- the same bits either way."""
    r = OC.BY_ID[rid]
    x, w, b = OC.row_tensors(r)
    pool, inv_hw, params, gate64 = OC.row_gate(r, x, OC.SILU)
    ref = OC.conv_ref(r, x, w, b, OC.SILU, gate64)
    y_t = _conv(r, x, w, b, OC.SILU, gate=_se_gate(pool, inv_hw, params), want_stats=1)
    y_r = _conv(r, x, w, b, OC.SILU, recipe=(pool, inv_hw, params), want_stats=1)
    e_t, e_r = rel_err(y_t, ref), rel_err(y_r, ref)
    report("operand_conv_gate", row=rid, family=r.family, rel_tensor=e_t, rel_recipe=e_r, bar=OC.BAR_FP32)
    assert e_t < OC.BAR_FP32 and e_r < OC.BAR_FP32, (rid, e_t, e_r)
    assert torch.equal(y_t, y_r), "gate tensor and gate recipe disagree"


@pytest.mark.parametrize("rid", [r.id for r in OC.DECONV4])
def test_deconv4_norm_on_load(rid, monkeypatch):
    """ConvTranspose2d k4 s2 p1: Deconv4Stage::commit_mode in the window form (no statistics), the four-parity form
    (statistics, or JH_DECONV4_WINDOW=0) and the general four-phase path (88 channels with statistics)."""
    r = OC.BY_ID[rid]
    monkeypatch.delenv(WINDOW_SWITCH, raising=False)
    x, w, b = OC.row_tensors(r)
    ref = OC.conv_ref(r, x, w, b, OC.NONE)
    for want_stats, switch, window in ((0, None, 1), (1, None, 0), (0, "0", 0)):
        if switch is not None:
            monkeypatch.setenv(WINDOW_SWITCH, switch)
        before = _window_launches()
        y = _conv(r, x, w, b, OC.NONE, want_stats=want_stats)
        ran = _window_launches() - before
        e = rel_err(y, ref)
        report("operand_deconv4", row=rid, family=r.family, want_stats=want_stats, window_switch=switch or "",
               window_launches=ran, rel=e, bar=OC.BAR_FP32)
        assert not torch.isnan(y).any()
        assert e < OC.BAR_FP32, (rid, want_stats, switch, e)
        assert ran == window, "which form ran"


@pytest.mark.parametrize("rid", [r.id for r in OC.DECONV_C1])
def test_deconv_c1_norm_on_load(rid):
    r = OC.BY_ID[rid]
    x, w, b = OC.row_tensors(r)
    ref = OC.conv_ref(r, x, w, b, OC.NONE)
    before = _window_launches()
    y = _conv(r, x, w, b, OC.NONE)
    e = rel_err(y, ref)
    report("operand_deconv_c1", row=rid, family=r.family, rel=e, bar=OC.BAR_FP32)
    assert _window_launches() == before, "one output channel takes the vector-ALU kernel"
    assert e < OC.BAR_FP32, (rid, e)


@pytest.mark.parametrize("rid", [r.id for r in OC.WINO])
def test_conv3d_winograd_relu_on_load(rid, monkeypatch):
    """The one-role Winograd kernel (the `okmask` path) and, JH_WINO=0, the direct 3 x 3 x 3 kernel of conv_mfma.h."""
    r = OC.BY_ID[rid]
    monkeypatch.delenv("JH_WINO", raising=False)
    x, w, b = OC.row_tensors(r)
    ref = OC.conv_ref(r, x, w, b, OC.RELU)
    y_w = _conv(r, x, w, b, OC.RELU, want_stats=1)
    e_w = rel_err(y_w, ref)
    report("operand_conv3d", row=rid, family=r.family, rel=e_w, bar=OC.BAR_FP32)
    assert e_w < OC.BAR_FP32, (rid, e_w)
    if rid == "wino_46":
        monkeypatch.setenv("JH_WINO", "0")
        y_d = _conv(r, x, w, b, OC.RELU, want_stats=1)
        e_d = rel_err(y_d, ref)
        report("operand_conv3d", row=rid + "_direct", family="conv3d_direct", rel=e_d, bar=OC.BAR_FP32)
        assert e_d < OC.BAR_FP32, (rid, e_d)
        assert not torch.equal(y_w, y_d), "JH_WINO had no effect"


@pytest.mark.parametrize("rid", [r.id for r in OC.WINO_PW])
def test_conv3d_winograd_persistent_relu_on_load(rid, monkeypatch):
    """The persistent kernel's loader-wave commit against float64, and bit for bit against the one-role kernel."""
    r = OC.BY_ID[rid]
    monkeypatch.delenv("JH_WINO", raising=False)
    monkeypatch.delenv("JH_WINO_PW", raising=False)
    x, w, b = OC.row_tensors(r)
    ref = OC.conv_ref(r, x, w, b, OC.RELU)
    y = _conv(r, x, w, b, OC.RELU, want_stats=1)
    monkeypatch.setenv("JH_WINO_PW", "0")
    y0 = _conv(r, x, w, b, OC.RELU, want_stats=1)
    e, e0 = rel_err(y, ref), rel_err(y0, ref)
    report("operand_conv3d", row=rid, family=r.family, rel=e, rel_one_role=e0, bar=OC.BAR_FP32)
    assert e < OC.BAR_FP32 and e0 < OC.BAR_FP32, (rid, e, e0)
    assert torch.equal(y, y0)


@pytest.mark.parametrize("rid", [r.id for r in OC.DECONV3D])
def test_deconv3d_relu_on_load(rid):
    r = OC.BY_ID[rid]
    x, w, b = OC.row_tensors(r)
    ref = OC.conv_ref(r, x, w, b, OC.RELU)
    e = rel_err(_conv(r, x, w, b, OC.RELU, want_stats=1), ref)
    report("operand_conv3d", row=rid, family=r.family, rel=e, bar=OC.BAR_FP32)
    assert e < OC.BAR_FP32, (rid, e)


@pytest.fixture()
def precision():
    from jarvis_hybridnet_amd import _native as N
    prev = N.set_precision("f32")
    yield N
    N.set_precision(prev)


# row, precision mode, in_act, want_stats: conv3d_bf16x3.hip, deconv4_bf16x3.hip (no statistics), conv_bf16x3.h
BF16X3 = [("wino_46", "bf16x3", OC.RELU, 1), ("deconv4_64_23", "bf16x3", OC.NONE, 0), ("k3_8x16", "bf16x3_wide", OC.SILU, 1)]


@pytest.mark.parametrize("rid,mode,act,want_stats", BF16X3)
def test_bf16x3_norm_on_load(rid, mode, act, want_stats, precision, monkeypatch):
    r = OC.BY_ID[rid]
    monkeypatch.delenv("JH_WINO", raising=False)
    monkeypatch.delenv(WINDOW_SWITCH, raising=False)
    x, w, b = OC.row_tensors(r)
    ref = OC.conv_ref(r, x, w, b, act)
    y32 = _conv(r, x, w, b, act, want_stats=want_stats)
    precision.set_precision(mode)
    y = _conv(r, x, w, b, act, want_stats=want_stats)
    e, e32 = rel_err(y, ref), rel_err(y32, ref)
    report("operand_bf16x3", row=rid, family=mode, in_act=act, rel=e, rel_fp32_kernel=e32, bar=OC.BAR_BF16X3)
    assert not torch.equal(y, y32), "the precision mode had no effect"
    assert e < OC.BAR_BF16X3, (rid, mode, e)


@pytest.mark.parametrize("C,S", OC.SE_GATE)
def test_se_gate(C, S):
    """se_gate_kernel alone against float64.  The bar is not a round number: the kernel's expression without fused
    multiply-adds, in torch float32 on the CPU, is 7.5e-8 / 8.9e-8 / 1.45e-7 of float64 on these inputs
    (tests/operand_cases.py: SE_GATE_FP32_REF, asserted by tests/test_operand_cases_cpu.py); the kernel gets four times
    that, because its fmaf order differs: 3.0e-7 / 3.6e-7 / 5.8e-7."""
    pool, inv_hw, params = OC.se_gate_case(C, S)
    ref = OC.se_gate_ref(pool, inv_hw, *params)
    e = rel_err(_se_gate(pool, inv_hw, params), ref)
    report("operand_se_gate", c=C, s=S, rel=e, fp32_reference=OC.SE_GATE_FP32_REF[(C, S)], bar=OC.SE_GATE_BAR[(C, S)])
    assert e < OC.SE_GATE_BAR[(C, S)], (C, S, e)


@pytest.mark.parametrize("C", OC.NORM_CHANNELS)
@pytest.mark.parametrize("shape", OC.NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_norm_apply(C, shape):
    """norm_apply_kernel in the forms the plans build, with small blocks and with 64 KB blocks."""
    from jarvis_hybridnet_amd import _native as N
    x, r1, r2 = OC.norm_tensors(C, shape)
    sx, s1 = OC.sums(x), OC.sums(r1)
    xc, r1c, r2c = cuda(x), cuda(r1), cuda(r2)
    d = shape[0] if len(shape) == 3 else 1
    for form in OC.NORM_FORMS:
        ref_y, ref_pool = OC.norm_ref(form, x, r1, r2)
        for kb in (0, 64):
            y = torch.full(x.shape, float("nan"), device="cuda")
            pool = torch.full((OC.NORM_N, C), float("nan"), dtype=torch.float64)
            N.check(N.lib().jh_op_norm_apply(xc.data_ptr(), OC.NORM_N, C, d, shape[-2], shape[-1], sx.data_ptr(), form.act,
                                             r1c.data_ptr() if form.r1 else None, s1.data_ptr() if form.r1n else None,
                                             r2c.data_ptr() if form.r2 else None, int(form.y), int(form.pool), kb,
                                             y.data_ptr(), pool.data_ptr(), N.stream()))
            torch.cuda.synchronize()
            e_y = rel_err(y, ref_y) if form.y else 0.0
            e_p = rel_err(pool, ref_pool) if form.pool else 0.0
            report("operand_norm_apply", form=form.id, c=C, shape=list(shape), min_block_kb=kb, rel_y=e_y, rel_pool=e_p,
                   bar_y=OC.BAR_NORM_Y, bar_pool=OC.BAR_NORM_POOL)
            assert e_y < OC.BAR_NORM_Y and e_p < OC.BAR_NORM_POOL, (form.id, C, shape, kb, e_y, e_p)
