"""Rows, inputs and float64 references of the operand-transform tests (tests/test_hip_operand.py on the GPU,
tests/test_operand_cases_cpu.py for the reference itself).

A consumer kernel applies InstanceNorm + activation + squeeze-excite gate to its input while it stages it, from the
producer's (sum, sum of squares).  Here the statistics come from the host in float64, so only the consumer is under
test, and the inputs are made so that a mistake cannot hide: every (image, channel) has its own sigma in [0.5, 2] and a
mean of +-(2.05 .. 3.95) sigma -- a padding pixel that is normalised instead of staying zero is off by 2 .. 4 units, and
statistics read from the wrong image are off by as much.  |mean| / sigma stays below 4 because the kernels take the
variance as E[x^2] * inv - mean^2 with a float `inv`."""
from collections import namedtuple

import torch
import torch.nn.functional as F

NONE, RELU, SILU = 0, 1, 2
ACTS = {NONE: lambda v: v, RELU: F.relu, SILU: F.silu}
CONST_CHANNEL, CONST_VALUE = 1, 3.0      # the constant channel (of image 0) of the rows that promise one

Row = namedtuple("Row", "id family nd kind k stride cin cout shape n acts lat bias const se")


def row(id, family, k, stride, cin, cout, shape, acts=(NONE, SILU), lat=(0,), bias=False, const=False, se=None, n=2,
        kind=0):
    return Row(id, family, len(shape), kind, k, stride, cin, cout, tuple(shape), n, tuple(acts), tuple(lat), bias, const,
               se)


# ---- conv_mfma.h, 2D: the smallest shape that meets each dispatch rule of launch_conv (csrc/conv_host.hip)
CONV2D = [
    # "if (d.k == 1 && d.stride == 1) return conv_launch_2d_k1(a, nr, small, ...)", small = (Wout <= 8): 8 x 16 tiles
    row("k1_8x16", "conv_mfma", 1, 1, 56, 56, (16, 16)),
    # ... the same rule with Wout <= 8: 8 x 8 tiles (H * W = 16 < 96 keeps it off the flat form)
    row("k1_8x8", "conv_mfma", 1, 1, 56, 56, (4, 4)),
    # "d.k == 1 && ... && (a.Wout % 16 != 0 || a.Hout % 8 != 0) && a.Hout * a.Wout >= 96": one row of H * W pixels, 1 x 128
    row("k1_flat_480", "conv_mfma", 1, 1, 480, 80, (20, 20)),
    row("k1_flat_16", "conv_mfma", 1, 1, 16, 8, (10, 13)),         # (130 pixels: no multiple of 16, not conv_pw_direct's)
    # "big = a.Wout >= 64 && a.Hout >= 64 && w.cin_p <= 32 && ... (d.k == 1 || d.k == 3)": 16 x 16 tiles; two column
    # blocks ("if (nb != 1 && nb != 4) return false") keep the layer off conv_pw_direct whatever the knobs say
    row("k1_big", "conv_mfma", 1, 1, 32, 24, (64, 64)),
    # "if (d.k == 3 && d.stride <= 2) return conv_launch_2d_k3(...)": 8 x 16 tiles
    row("k3_8x16", "conv_mfma", 3, 1, 16, 16, (32, 48), const=True),
    row("k3_big", "conv_mfma", 3, 1, 16, 16, (64, 64)),            # the `big` rule with k == 3
    # "d.k == 3 && d.stride == 1 && ... a.Wout > 16 && a.Wout <= 20 && a.Hout <= 22 && !d.latency_class": one whole-image
    # tile of 23 x 20 pixel slots; latency_class 1: the 8 x 16 tiles
    row("k3_w20", "conv_mfma", 3, 1, 24, 40, (22, 17), lat=(0, 1)),
    # "d.k == 3 && d.stride == 2 && a.Wout > 16 && a.Wout <= 20 && a.Hout <= 22" (under !d.latency_class): the 23 x 20 tile
    row("k3s2_w20", "conv_mfma", 3, 2, 8, 48, (40, 40), lat=(0, 1)),
    # "if (d.k == 5 && d.stride <= 2) return conv_launch_2d_k5(...)": 8 x 16 tiles
    row("k5s2_8x16", "conv_mfma", 5, 2, 16, 96, (32, 32)),
    # "d.k == 5 && d.stride <= 2 && a.Wout > 32 && a.Wout <= 40" (under !d.latency_class): 8 x 40 tiles
    row("k5_w40", "conv_mfma", 5, 1, 16, 32, (36, 38), lat=(0, 1)),
    row("k5s2_w40", "conv_mfma", 5, 2, 8, 16, (70, 66), lat=(0, 1)),
    # final_conv1 of the head (EffTrackPlan::build, want_res1): k3 s1, 23 of 32 output columns real
    row("final_conv1", "conv_mfma", 3, 1, 64, 23, (24, 24), acts=(NONE,)),
]

# ---- the project convolutions of the MBConv blocks: SiLU + squeeze-excite gate on load, se = (C, S)
PROJECT = [
    row("project_240", "project", 1, 1, 240, 40, (12, 12), acts=(SILU,), se=(240, 10), const=True),   # flat (144 pixels)
    row("project_720", "project", 1, 1, 720, 120, (8, 8), acts=(SILU,), se=(720, 30)),   # widest of the large model; 8 x 8
    row("project_480", "project", 1, 1, 480, 80, (20, 20), acts=(SILU,), se=(480, 20)),  # flat
]

# ---- conv_pw_direct.hip: "a.cin_p > 48 ... return false", "nb != 1 && nb != 4", "min_px = nb == 1 ? 1024 : 4096"
PW_DIRECT = [
    row("pwd_16_8", "conv_pw_direct", 1, 1, 16, 8, (32, 32), acts=(SILU,), se=(16, 4), const=True),
    row("pwd_48_16", "conv_pw_direct", 1, 1, 48, 16, (32, 32), acts=(SILU,), se=(48, 12)),
    row("pwd_24_56", "conv_pw_direct", 1, 1, 24, 56, (64, 64), acts=(NONE,), bias=True),
    row("pwd_40_56", "conv_pw_direct", 1, 1, 40, 56, (64, 64), acts=(NONE,), bias=True),
]

# ---- ConvTranspose2d k4 s2 p1 (csrc/deconv4.hip; kind 1).  Without statistics: the window form
# ("window = d.nd == 2 && d.ostride > 1 && d.plain_out && wmode != 0 && deconv4_window_eligible(...)"); with statistics
# the four-parity kernel ("deconv4_eligible: cout_p16 <= 32 && cin_p % 16 == 0") or, 88 channels, the general
# four-phase path of conv_mfma.h
DECONV4 = [
    row("deconv4_64_23", "deconv4", 4, 2, 64, 23, (24, 24), acts=(NONE,), kind=1, const=True),
    row("deconv4_32_8", "deconv4", 4, 2, 32, 8, (20, 12), acts=(NONE,), kind=1),
    row("deconv4_16_23", "deconv4", 4, 2, 16, 23, (8, 16), acts=(NONE,), kind=1),
    row("deconv4_88_23", "deconv4", 4, 2, 88, 23, (12, 12), acts=(NONE,), kind=1),
]
# ---- one output channel: csrc/deconv_c1.hip ("if (J == 1)" of EffTrackPlan::build)
DECONV_C1 = [
    row("deconv_c1_64", "deconv_c1", 4, 2, 64, 1, (24, 24), acts=(NONE,), kind=1, const=True),
    row("deconv_c1_88", "deconv_c1", 4, 2, 88, 1, (9, 21), acts=(NONE,), kind=1),
]

# ---- 3D, ReLU on load (V2VPlan::res_block).  "wino = d.nd == 3 && d.k == 3 && d.stride == 1 && ..." (Plan::add_conv)
WINO = [        # too few tiles for the persistent form: the one-role kernel (csrc/conv3d_wino.hip)
    row("wino_46", "conv3d_wino", 3, 1, 46, 46, (8, 12, 20), acts=(RELU,), bias=True, const=True),
    row("wino_6_23", "conv3d_wino", 3, 1, 6, 23, (5, 9, 11), acts=(RELU,), bias=True),
]
WINO_PW = [     # at least two tiles per CU: the persistent form (csrc/conv3d_wino_pw.hip); 6 x 18 x 18: remainder strips
    row("wino_pw_16", "conv3d_wino_pw", 3, 1, 24, 24, (8, 16, 16), acts=(RELU,), bias=True, n=64, const=True),
    row("wino_pw_18", "conv3d_wino_pw", 3, 1, 24, 24, (6, 18, 18), acts=(RELU,), bias=True, n=40),
]
DECONV3D = [    # ConvTranspose3d k2 s2 (kind 2): eight one-tap phases of conv_mfma.h
    row("deconv3d_92", "deconv3d", 2, 2, 92, 46, (4, 4, 4), acts=(RELU,), bias=True, kind=2, const=True),
]

CONV_ROWS = CONV2D + PROJECT + PW_DIRECT + DECONV4 + DECONV_C1 + WINO + WINO_PW + DECONV3D
BY_ID = {r.id: r for r in CONV_ROWS}
assert len(BY_ID) == len(CONV_ROWS)

# bars of raw convolution outputs, as tests/test_hip_ops.py and tests/test_hip_bf16x3.py hold them
BAR_FP32, BAR_BF16X3 = 2e-5, 5e-5


def _seed(r):
    return 1000 * r.k + 10 * r.cin + r.cout + sum(r.shape)


def operand_input(seed, shape, const=False, sign=None):
    """(n, c, *spatial) float32: each (image, channel) has EXACTLY (in float64, before the rounding to float32) the drawn
    sigma and mean; `const`: channel CONST_CHANNEL of image 0 is the constant CONST_VALUE (variance 0: the clamp of a
    negative variance and rstd = 1 / sqrt(eps)); `sign` (+1 / -1): every mean with that sign instead of a drawn one
    (the draws, hence every other number, stay what they are without it)."""
    g = torch.Generator().manual_seed(seed)
    n, c = shape[:2]
    dims = tuple(range(2, len(shape)))
    z = torch.randn(shape, generator=g, dtype=torch.float64)
    z = z - z.mean(dims, keepdim=True)
    z = z / z.pow(2).mean(dims, keepdim=True).sqrt()
    sigma = 0.5 + 1.5 * torch.rand(n, c, generator=g, dtype=torch.float64)
    ratio = 2.05 + 1.9 * torch.rand(n, c, generator=g, dtype=torch.float64)
    drawn = (torch.rand(n, c, generator=g) < 0.5).double() * 2 - 1
    sign = drawn if sign is None else torch.full_like(drawn, float(sign))
    ex = (...,) + (None,) * len(dims)
    x = (z * sigma[ex] + (sign * ratio * sigma)[ex]).float()
    if const:
        x[0, CONST_CHANNEL] = CONST_VALUE
    return x


def sums(x):
    """(n, c, 2) float64: sum and sum of squares per image and channel of the float32 tensor."""
    xd = x.double()
    dims = tuple(range(2, x.dim()))
    return torch.stack([xd.sum(dims), (xd * xd).sum(dims)], -1).contiguous()


def row_tensors(r):
    """x, weights, bias of a row (float32; weights in torch layout, asymmetric: tap and phase swaps show)."""
    g = torch.Generator().manual_seed(_seed(r) + 1)
    x = operand_input(_seed(r), (r.n, r.cin) + r.shape, r.const)
    if r.kind == 0:
        w = torch.randn((r.cout, r.cin) + (r.k,) * r.nd, generator=g) / (r.cin * r.k ** r.nd) ** 0.5
    elif r.kind == 1:
        w = torch.randn(r.cin, r.cout, 4, 4, generator=g) / (r.cin * 4) ** 0.5
    else:
        w = torch.randn(r.cin, r.cout, 2, 2, 2, generator=g) / r.cin ** 0.5
    b = torch.randn(r.cout, generator=g) * 0.3 if r.bias else None
    return x, w, b


def se_params(seed, C, S):
    """The two fully connected layers of a squeeze-excite block (efficientnet.py:107-112), float32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S, C, generator=g) / C ** 0.5, torch.randn(S, generator=g) * 0.1,
            torch.randn(C, S, generator=g) / S ** 0.5, torch.randn(C, generator=g) * 0.5)


def inv_f32(count):
    """1 / count as the float the plans hand to the kernels."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(count), dtype=torch.float32))


def se_gate_ref(pool, inv_hw, wr, br, we, be, dtype=torch.float64):
    """sigmoid(We silu(Wr (pool * inv_hw) + br) + be), pool (n, C) float64."""
    mean = (pool * inv_hw).to(dtype)
    hid = F.silu(mean @ wr.to(dtype).t() + br.to(dtype))
    return torch.sigmoid(hid @ we.to(dtype).t() + be.to(dtype))


def se_gate_fp32_sequential(pool, inv_hw, wr, br, we, be):
    """The expression of se_gate_kernel in float32 WITHOUT fused multiply-adds, in the kernel's order: every product and
    every sum rounded on its own (the kernel accumulates with fmaf: one rounding per term)."""
    mean = (pool * inv_hw).float()
    acc = br.clone().expand(pool.shape[0], -1).contiguous()
    for c in range(wr.shape[1]):
        acc = acc + wr[:, c] * mean[:, c:c + 1]
    hid = acc / (1.0 + torch.exp(-acc))
    acc = be.clone().expand(pool.shape[0], -1).contiguous()
    for j in range(we.shape[1]):
        acc = acc + we[:, j] * hid[:, j:j + 1]
    return 1.0 / (1.0 + torch.exp(-acc))


def inorm(x, dtype):
    """InstanceNorm(eps 1e-5).  float64: torch's own.  float32: the expression the kernels evaluate -- mean and rstd
    from the float64 sums, rounded to float32, then (x - mean) * rstd in float32 (the operation under test takes the
    statistics as an input; torch's float32 instance_norm computes them in float32, which on these offset inputs costs
    1e-5 of a normalised value and more of a pooled sum)."""
    if dtype == torch.float64:
        return F.instance_norm(x.double(), eps=1e-5)
    dims = tuple(range(2, x.dim()))
    xd = x.double()
    mean = xd.mean(dims, keepdim=True)
    rstd = 1.0 / ((xd * xd).mean(dims, keepdim=True) - mean * mean).clamp_min(0.0).add(1e-5).sqrt()
    return (x.to(dtype) - mean.to(dtype)) * rstd.to(dtype)


def transformed(x, act, gate, dtype):
    """InstanceNorm(eps 1e-5) -> activation -> * gate: what the consumer's MFMAs must see."""
    v = ACTS[act](inorm(x, dtype))
    if gate is not None:
        v = v * gate.to(dtype)[(...,) + (None,) * (x.dim() - 2)]
    return v


def pooled(x, act):
    """(n, c) float64 pooled sums of the activated tensor: what a squeeze-excite block's pooling pass leaves."""
    return transformed(x, act, None, torch.float64).sum(tuple(range(2, x.dim())))


def conv_ref(r, x, w, b, act, gate=None, dtype=torch.float64):
    v = transformed(x, act, gate, dtype)
    w, b = w.to(dtype), (b.to(dtype) if b is not None else None)
    if r.kind == 1:
        return F.conv_transpose2d(v, w, b, 2, 1)
    if r.kind == 2:
        return F.conv_transpose3d(v, w, b, 2, 0)
    return (F.conv2d if r.nd == 2 else F.conv3d)(v, w, b, r.stride, r.k // 2)


def row_gate(r, x, act, dtype=torch.float64):
    """The recipe of a row with a squeeze-excite gate -> (pool, inv_hw, (wr, br, we, be), gate in `dtype`)."""
    C, S = r.se
    pool = pooled(x, act).contiguous()
    inv_hw = inv_f32(x[0, 0].numel())
    params = se_params(_seed(r) + 2, C, S)
    return pool, inv_hw, params, se_gate_ref(pool, inv_hw, *params, dtype=dtype)


# ---- se_gate_kernel alone: (C, S) with n = 3
SE_GATE = [(16, 4), (240, 10), (720, 30)]
SE_GATE_N, SE_GATE_HW = 3, 144
# |float32 sequential expression - float64| / max |float64| of each case, measured on the CPU (7.48e-8, 8.82e-8,
# 1.42e-7, rounded up here; tests/test_operand_cases_cpu.py asserts that they are not exceeded).  The kernel's bar is
# four times its case's figure, because its fmaf order differs: 3.0e-7, 3.6e-7, 5.8e-7.
SE_GATE_FP32_REF = {(16, 4): 7.5e-8, (240, 10): 8.9e-8, (720, 30): 1.45e-7}
SE_GATE_BAR = {k: 4 * v for k, v in SE_GATE_FP32_REF.items()}


def se_gate_case(C, S):
    g = torch.Generator().manual_seed(31 * C + S)
    pool = ((torch.randn(SE_GATE_N, C, generator=g, dtype=torch.float64) * 0.3 + 0.2) * SE_GATE_HW).contiguous()
    return pool, inv_f32(SE_GATE_HW), se_params(C + S, C, S)


# ---- norm_apply: the forms the plans build (act, r1, r1 normalised on load, r2, writes y, pooled sums)
NormForm = namedtuple("NormForm", "id act r1 r1n r2 y pool")
NORM_FORMS = [
    NormForm("materialise", NONE, False, False, False, True, False),       # EffTrackPlan::materialise
    NormForm("se_pool", SILU, False, False, False, False, True),           # mbconv: pooled sums only
    NormForm("mbconv_skip", NONE, True, False, False, True, False),        # mbconv: + skip connection
    NormForm("v2v_r1n", RELU, True, True, False, True, False),             # V2VPlan::res_block, r1 raw
    NormForm("v2v_r1n_r2", RELU, True, True, True, True, False),           # ... + the encoder / decoder skip sum
]
NORM_CHANNELS = [16, 46, 92, 240, 528, 720]          # Cp 16, 48, 96, 240, 528, 720: 256 / 512 / 1024 threads, idle lanes
NORM_SHAPES = [(8, 8), (20, 20), (25, 40), (6, 18, 18)]   # P = 64, 400, 1000, 1944: unrolled loop, tail, partial block
NORM_N = 2
BAR_NORM_Y, BAR_NORM_POOL = 2e-4, 1e-4


def norm_tensors(C, shape):
    seed = 7 * C + sum(shape)
    x = operand_input(seed, (NORM_N, C) + tuple(shape), const=True)
    r1 = operand_input(seed + 1, (NORM_N, C) + tuple(shape))
    g = torch.Generator().manual_seed(seed + 2)
    r2 = torch.randn((NORM_N, C) + tuple(shape), generator=g)
    return x, r1, r2


def norm_ref(form, x, r1, r2, dtype=torch.float64):
    """act(IN(x) + r1') + r2, r1' = relu(IN(r1)) in the r1n forms -> (y, pooled sums of y)."""
    v = inorm(x, dtype)
    if form.r1:
        v = v + (F.relu(inorm(r1, dtype)) if form.r1n else r1.to(dtype))
    v = ACTS[form.act](v)
    if form.r2:
        v = v + r2.to(dtype)
    return v, v.sum(tuple(range(2, x.dim())))
