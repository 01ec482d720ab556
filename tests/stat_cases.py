"""Rows, inputs, float64 references and rounding depths of the emitted-statistics tests (tests/test_hip_stats.py on the
GPU; tests/test_stat_cases_cpu.py for the rows, the inputs and the bounds themselves).

Every convolution, depthwise and stem launch hands its consumer the raw y plus, per (image, channel), the sum s1 and the
sum of squares s2 of the y it stored.  Here those sums are read back (jh_op_operand::out_sums_host, jh_op_depthwise_ex,
jh_op_stem) and held against the float64 sums of the y the SAME launch returned -- a y error and a statistics error stay
separate findings:
    |s1 - sum v| <= d1 2^-24 sum |v|,      |s2 - sum v^2| <= d2 2^-24 sum v^2        per (image, channel).

Rows.  The convolution rows are tests/operand_cases.py's, by id: the smallest shapes that meet each dispatch rule; three
3D rows (strided, k2 s2, pointwise) are added here.  The row says which statistics code path it runs and with how many
16-pixel blocks per wave (MR), read from the dispatch (csrc/conv_host.hip, csrc/conv_tu_*.hip, csrc/deconv4.hip,
csrc/conv_bf16x3*.hip, csrc/conv3d_bf16x3.hip); where the tile of a 3D layer depends on a count of tiles, the row carries
the larger MR of the two candidates (the depth grows with MR).

Inputs.  Every output (image, channel) is off-centre, |mean| of 2 .. 4 of its own sigma, so that each pixel carries about
1 / P of its channel's sums and the pivot, un-shift and limb code works on numbers whose mean matters:
  layers the plans run with a bias: the input is centred per (image, channel), and the bias is +-(2.05 .. 3.95) of the
    float64 sigma of the output without it (tests/node_cases.py: make_node);
  bias-free layers, depthwise and stem: the input means are one-signed (onesigned_input: operand_input(sign=+1), every
    image with image 0's sigma and mean per channel), and one constant per output channel, found on the CPU in float64,
    is added to all of that channel's weights -- the output then gains c * (box sum of the input), which is far from
    zero -- so that the worst image of the channel lands closest to a drawn ratio in 2.5 .. 3.5;
  one row per 2D code path carries a constant channel in image 0: output channel CO_CONST reads input channel
    CONST_CHANNEL alone, through its centre tap, and that input channel of image 0 is constant.
An operand transform on load is part of a row only where the row's form needs it (the gate recipe of project_240).

Depths d1, d2: float32 roundings an addend passes on its way into one partial, weighted by how much larger than the addend
the rounded number can be.  u = 2^-24.  Everything behind a partial is exact or fp64: exact_add / exact_add_rounded
(csrc/jh_common.h) put it on fixed grids -- the rounded form keeps 2^-31 relative (2^-36 absolute below 2^-5) --, the
limb atomics are exact, the reader adds three limbs in fp64.  "+ 1" below is that tail, a 2^-7 of it in fact.

  conv_epilogue<MR, NR, TY, TX, NW, FULL> (csrc/conv_mfma.h), the model being the MR = 1 derivation of
  tests/test_hip_node_outputs.py (10 / 58).  A lane holds n = 4 MR values of one channel.  It subtracts the pivot m (slot
  0 of its first block), d_r = fl(v_r - m): one rounding relative to |d_r|.  The d_r of the lane are added in packed
  float32: MR - 1 roundings along a slot pair (the first addition, to zero, is exact), one for t1a + t1b, one for the two
  halves: with the subtraction MR + 2 roundings on sum |d_r|.  The squares go through fma(d, d, t): the product carries
  the two relative roundings of d_r, the chain MR roundings, the two closing additions two: MR + 4 on sum d_r^2.  The
  un-shift sum v = cnt m + sum d, sum v^2 = cnt m^2 + 2 m sum d + sum d^2 is fp64, as are the lanes' (sum_xor16 / 32) and
  the NW waves' sums: NW does not enter.
    pivot inside the image (it is one of the lane's values; true whenever a lane's blocks are 16 slots apart in a tile
    whose width divides 16 or is a multiple of it -- slot 0 then has the lane's smallest row and its own column -- i.e.
    every tile but 23 x 20 and 8 x 40): |d_r| <= |v_r| + |v_0|, sum |d_r| <= (n - 1) sum |v| of the lane,
      d1 = (MR + 2)(n - 1) + 1
      squares: 2 |m| (MR + 2) u sum |d_r| with |v_0| sum (|v_r| + |v_0|) <= 1.5 (n - 1) sum v^2, and
               (MR + 4) u sum d_r^2 with sum d_r^2 <= 2 (n - 1) sum v^2:
      d2 = (n - 1)(3 (MR + 2) + 2 (MR + 4)) + 1 = (n - 1)(5 MR + 14) + 1            MR = 1: 10 / 58, 2: 29 / 169, 4: 91 / 511
    pivot possibly outside the image (23 x 20 and 8 x 40 tiles: 16 slots further is another column): m is then a sum
    over the zero-filled halo, NOT one of the channel's values; it is BOUNDED HERE BY THE CHANNEL'S max |v| = M, which
    is an assumption about the data (a halo sum has fewer terms than an inside one), not a property of the code.  With
    k1 = P M / sum |v| and k2 = P M^2 / sum v^2 of the (image, channel), sum |d_r| <= sum |v| + P M over the channel:
      d1 = (MR + 2)(1 + k1) + 1
      d2 = 2 (MR + 2)(sqrt(k2) + k2) + 2 (MR + 4)(1 + k2) + 1          (M sum |v| <= sqrt(k2) sum v^2: Cauchy-Schwarz)
    These depend on the returned y; on these inputs k1 is about 2, k2 about 4.
  In the phase paths (four-parity deconv4.hip, the four- and eight-phase transposed paths) every phase's workgroups add
  partials of this kind into one row: the bound is per addend, so it is the same.

  conv_pw_direct.hip: a lane holds one pixel of rbw = max(8, min(32, P / 256)) row blocks per channel; the pivot is the
  value of pixel 0 of the wave's first row block (ds_bpermute) -- known, so the bound uses it instead of a worst case:
  with D1 = sum |v - m| and D2 = sum (v - m)^2 over the wave's rbw 16 pixels, the subtraction, rbw - 1 additions and the
  four DPP steps of row_sum are rbw + 4 roundings on D1; the squares 2 + rbw + 4 on D2:
      |s1 - sum v| <= u ((rbw + 4) sum_waves D1 + sum |v|),
      |s2 - sum v^2| <= u (2 (rbw + 4) sum_waves |m| D1 + (rbw + 6) sum_waves D2 + sum v^2).
  d1, d2 are these over u sum |v|, u sum v^2.

  conv3d_wino.hip, conv3d_wino_pw.hip: plain float32, the partials too (by design; stat_add(float) is exact).  Every
  float32 addition on the longest path into one partial counts once: 16 sequential `s1 += v` of a lane (2 x 2 outputs of
  4 tiles), two sum_xor steps, four additions over the waves: 22; the squares are rounded before they are added: 23.

  depthwise_lds_kernel (csrc/elementwise.hip): a thread holds nv = 4 outputs of one channel (16-tile: one strip) or 8
  (20-tile: two strips), the pivot is its first in-image output (one of its values).  d = fl(v - m), nv - 1 additions:
  nv roundings on sum |d| <= (nv - 1) sum |v|; squares 2 + nv on sum d^2 <= 2 (nv - 1) sum v^2, cross term
  3 nv (nv - 1).  Behind that fp64 through LDS, then exact_add_rounded:
      d1 = nv (nv - 1) + 1,   d2 = (nv - 1)(5 nv + 4) + 1              16-tile: 13 / 73, 20-tile: 57 / 309
  The POOL form's `tot` is the same number as the one emitted partial.

  stem_conv_kernel (csrc/stem.hip): `in_img ? acc : 0` converted to fp64 (stat_acc), 16 x 16 fp64 partials,
  exact_add_rounded: no float32 rounding at all.  d1 = d2 = 1 (the tail).

The table is plain Python; what needs torch imports it where it is used."""
from collections import namedtuple
from functools import lru_cache

from tests import operand_cases as OC

U = 2.0 ** -24
PRECISIONS = ("f32", "bf16x3", "bf16x3_wide")
CO_CONST, W_CONST = 2, 0.7               # the output channel that reads the constant input channel alone, its weight

# row: an operand_cases.Row (shape, layer); path: the statistics code path; mr / pivot_in: see the docstring; lat:
# ConvDesc::latency_class; prec: index into PRECISIONS; env: knobs set for the launch; form: what jh_conv_form answers
ConvStat = namedtuple("ConvStat", "id row path mr pivot_in lat prec env form const gate")


def _cs(id, base, path, mr, pivot_in=True, lat=0, prec=0, env=(), form="mfma", const=False, gate=False, row=None):
    return ConvStat(id, row or OC.BY_ID[base], path, mr, pivot_in, lat, prec, tuple(env), form, const, gate)


# 3D forms of conv_epilogue that tests/operand_cases.py has no row for (V2VPlan: the strided front convolution, the k2 s2
# pooling convolution, a pointwise convolution); with a bias, as the V2V layers run
ROWS_3D = {
    "c3d_k3s2": OC.row("c3d_k3s2", "conv3d", 3, 2, 23, 46, (10, 12, 14), acts=(OC.NONE,), bias=True),
    "c3d_k2s2": OC.row("c3d_k2s2", "conv3d", 2, 2, 46, 92, (8, 8, 8), acts=(OC.NONE,), bias=True),
    "c3d_k1": OC.row("c3d_k1", "conv3d", 1, 1, 46, 23, (6, 10, 12), acts=(OC.NONE,), bias=True),
}

CONV_STATS = [
    # ---- conv_epilogue, 2D tiles of conv_mfma.h: 8 x 16 (MR 2), 8 x 8 (1), 1 x 128 (2), 16 x 16 (4), 23 x 20 (7), 8 x 40 (5)
    _cs("k1_8x16", "k1_8x16", "epilogue2d", 2, const=True),
    _cs("k1_8x8", "k1_8x8", "epilogue2d", 1),
    _cs("k1_flat_16", "k1_flat_16", "epilogue2d", 2),
    _cs("k1_big", "k1_big", "epilogue2d", 4),
    _cs("k3_8x16", "k3_8x16", "epilogue2d", 2),
    _cs("k3_big", "k3_big", "epilogue2d", 4),
    _cs("k3_w20", "k3_w20", "epilogue2d", 7, pivot_in=False),
    _cs("k3_w20_lat1", "k3_w20", "epilogue2d", 2, lat=1),
    _cs("k3s2_w20", "k3s2_w20", "epilogue2d", 7, pivot_in=False),
    _cs("k3s2_w20_lat1", "k3s2_w20", "epilogue2d", 2, lat=1),
    _cs("k5_w40", "k5_w40", "epilogue2d", 5, pivot_in=False),
    _cs("k5_w40_lat1", "k5_w40", "epilogue2d", 2, lat=1),
    _cs("k5s2_w40", "k5s2_w40", "epilogue2d", 5, pivot_in=False),
    _cs("k5s2_w40_lat1", "k5s2_w40", "epilogue2d", 2, lat=1),
    _cs("k5s2_8x16", "k5s2_8x16", "epilogue2d", 2),
    _cs("final_conv1", "final_conv1", "epilogue2d", 2),
    _cs("project_240", "project_240", "epilogue2d", 2, gate=True),
    # ---- conv_pw_direct.hip
    _cs("pwd_16_8", "pwd_16_8", "pw_direct", 0, const=True),
    _cs("pwd_48_16", "pwd_48_16", "pw_direct", 0),
    _cs("pwd_24_56", "pwd_24_56", "pw_direct", 0),
    # ---- transposed, with statistics: the four-parity kernel (8 x 16 tiles of input pixels, MR 2), 88 channels the
    # four-phase path (k2 phases on 8 x 16 tiles)
    _cs("deconv4_64_23", "deconv4_64_23", "epilogue2d", 2, form="mfma_paired"),
    _cs("deconv4_32_8", "deconv4_32_8", "epilogue2d", 2, form="mfma_paired"),
    _cs("deconv4_88_23", "deconv4_88_23", "epilogue2d", 2),
    # ---- 3D
    _cs("wino_46", "wino_46", "wino", 0, form="wino"),
    _cs("wino_6_23", "wino_6_23", "wino", 0, form="wino"),
    _cs("wino_46_direct", "wino_46", "epilogue3d", 2, env=(("JH_WINO", "0"),)),      # 1 x 4 x 16 or 2 x 4 x 16 tiles
    _cs("wino_pw_16", "wino_pw_16", "wino_pw", 0, form="wino"),
    _cs("wino_pw_18", "wino_pw_18", "wino_pw", 0, form="wino"),
    _cs("wino_pw_16_one_role", "wino_pw_16", "wino", 0, env=(("JH_WINO_PW", "0"),), form="wino"),
    _cs("wino_pw_18_one_role", "wino_pw_18", "wino", 0, env=(("JH_WINO_PW", "0"),), form="wino"),
    _cs("deconv3d_92", "deconv3d_92", "epilogue3d", 2),                              # eight k1 phases
    _cs("c3d_k3s2", None, "epilogue3d", 1, form="mfma_tappair", row=ROWS_3D["c3d_k3s2"]),   # 1 x 4 x 16
    _cs("c3d_k2s2", None, "epilogue3d", 1, row=ROWS_3D["c3d_k2s2"]),                 # 1 x 4 x 16
    _cs("c3d_k1", None, "epilogue3d", 2, row=ROWS_3D["c3d_k1"]),
    # ---- precision modes: conv3d_bf16x3.hip (4 x 4 x 16 tiles, MR 4), conv_bf16x3.h 2D (1 x 16 x 16, MR 4) and 3D
    # (2 x 4 x 16, MR 2)
    _cs("wino_46_bf16x3", "wino_46", "epilogue3d", 4, prec=1, form="wino_bf16x3"),
    _cs("k3_8x16_bf16x3_wide", "k3_8x16", "epilogue2d", 4, prec=2, form="conv_bf16x3"),
    _cs("c3d_k3s2_bf16x3_wide", None, "epilogue3d", 2, prec=2, form="conv_bf16x3", row=ROWS_3D["c3d_k3s2"]),
]
CONV_BY_ID = {c.id: c for c in CONV_STATS}
assert len(CONV_BY_ID) == len(CONV_STATS)

# depthwise (k, c, H, W, pool), n = 3; 88 channels leave a last chunk of two quads
DW_N = 3
DW_ROWS = [(3, 88, 8, 8, 0), (5, 240, 12, 14, 0), (5, 96, 24, 20, 0), (3, 88, 18, 20, 0), (5, 240, 16, 16, 1),
           (3, 96, 17, 19, 1), (5, 88, 20, 18, 1)]
DW_CONST = DW_ROWS[0]
# stem (cout, H, W), n = 2; 40 x 56: 20 x 28 outputs, ragged tiles in both directions
STEM_N = 2
STEM_ROWS = [(16, 64, 64), (32, 64, 64), (16, 40, 56), (32, 40, 56)]
STEM_CONST = STEM_ROWS[0]


def dw_id(r):
    return "k%d_c%d_%dx%d%s" % (r[0], r[1], r[2], r[3], "_pool" if r[4] else "")


def stem_id(r):
    return "c%d_%dx%d" % r


def pad_of(r):
    return r.k // 2 if r.kind == 0 and r.k != 2 else (1 if r.kind == 1 else 0)


def out_shape(r):
    if r.kind == 0:
        return tuple((e + 2 * pad_of(r) - r.k) // r.stride + 1 for e in r.shape)
    return tuple(2 * e for e in r.shape)


def pixels(shape):
    p = 1
    for e in shape:
        p *= e
    return p


# ---- depths
def dw_tile(h, w):
    return 20 if 16 < max(h, w) <= 20 else 16          # launch_depthwise (csrc/elementwise.hip)


def dw_depth(h, w):
    nv = 4 if dw_tile(h, w) == 16 else 8
    return nv * (nv - 1) + 1, (nv - 1) * (5 * nv + 4) + 1


STEM_DEPTH = (1, 1)
WINO_DEPTH = (22, 23)


def epilogue_depth(mr):
    n = 4 * mr
    return (mr + 2) * (n - 1) + 1, (n - 1) * (5 * mr + 14) + 1


def pw_rbw(P):
    return max(8, min(32, (P // 16) // 16))            # launch_conv_pw_direct


def sums64(y):
    """(sum, sum |v|, sum v^2, max |v|) per (image, channel) of y, float64."""
    v = y.double().flatten(2)
    return v.sum(2), v.abs().sum(2), (v * v).sum(2), v.abs().amax(2)


def conv_depth(cs, y):
    """(d1, d2) per (image, channel), float64 tensors (n, c), of the row's code path on the tensor y it returned."""
    import torch
    s, a, q, m = sums64(y)
    one = torch.ones_like(a)
    if cs.path in ("wino", "wino_pw"):
        return WINO_DEPTH[0] * one, WINO_DEPTH[1] * one
    if cs.path == "pw_direct":
        v = y.double().flatten(2)
        P = v.shape[2]
        rbw = pw_rbw(P)
        b1, b2 = torch.zeros_like(a), torch.zeros_like(a)
        for p0 in range(0, P, 16 * rbw):
            piv = v[:, :, p0:p0 + 1]
            d = (v[:, :, p0:p0 + 16 * rbw] - piv).abs()
            b1 += (rbw + 4) * d.sum(2)
            b2 += 2 * (rbw + 4) * piv[:, :, 0].abs() * d.sum(2) + (rbw + 6) * (d * d).sum(2)
        return b1 / a + 1, b2 / q + 1
    if cs.pivot_in:
        d1, d2 = epilogue_depth(cs.mr)
        return d1 * one, d2 * one
    P = pixels(y.shape[2:])
    k1, k2 = P * m / a, P * m * m / q
    mr = cs.mr
    return (mr + 2) * (1 + k1) + 1, 2 * (mr + 2) * (k2.sqrt() + k2) + 2 * (mr + 4) * (1 + k2) + 1


def stat_errors(y, sums, d1, d2):
    """|s1 - sum v| / sum |v| and |s2 - sum v^2| / sum v^2 against the float64 sums of y, at the (image, channel) where
    the error comes closest to (or exceeds most) its bound d u: (s1_err, s1_bound, s2_err, s2_bound, worst error over
    bound of both).  d1, d2: numbers or (n, c) tensors."""
    import torch
    s, a, q, _ = sums64(y)
    out, worst = [], 0.0
    for got, want, scale, d in ((sums[..., 0], s, a, d1), (sums[..., 1], q, q, d2)):
        e = (got - want).abs() / scale
        b = torch.as_tensor(d, dtype=torch.float64).expand_as(e) * U
        over = torch.where(torch.isfinite(e), e / b, torch.full_like(e, float("inf"))).flatten()
        at = over.argmax()
        out += [e.flatten()[at].item(), b.flatten()[at].item()]
        worst = max(worst, over[at].item())
    return tuple(out) + (worst,)


# ---- tensors and references (torch)
Case = namedtuple("Case", "x w b ref recipe")      # float32 input, weights, bias (or None); float64 y; gate recipe or None


def centred_input(seed, shape):
    """(n, c, *spatial) float32 with mean 0 per (image, channel) and a sigma in [0.5, 2] per CHANNEL (the same in every
    image, so that the sigma of a channel of the output is the same in every image, up to the noise's own)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    dims = tuple(range(2, len(shape)))
    z = torch.randn(shape, generator=g, dtype=torch.float64)
    z = z - z.mean(dims, keepdim=True)
    z = z / z.pow(2).mean(dims, keepdim=True).sqrt()
    sigma = 0.5 + 1.5 * torch.rand(shape[1], generator=g, dtype=torch.float64)
    return (z * sigma[(None, slice(None)) + (None,) * len(dims)]).float()


def onesigned_input(seed, shape, const=False):
    """operand_input with every mean positive, and every image given the sigma and the mean image 0 drew for the
    channel: one constant per output channel then puts that channel off-centre in EVERY image (the weights are shared by
    the images; with a sigma and a mean per image no constant fits them all).  The images still differ in every pixel."""
    x = OC.operand_input(seed, shape, sign=1).double()
    dims = tuple(range(2, len(shape)))
    mean, sigma = x.mean(dims, keepdim=True), x.var(dims, unbiased=False, keepdim=True).sqrt()
    x = ((x - mean) / sigma * sigma[:1] + mean[:1]).float()
    if const:
        x[0, OC.CONST_CHANNEL] = OC.CONST_VALUE
    return x


def offcentre_constants(y0, S, g, skip=None):
    """y0, S (n, c, *spatial) float64, S the response to all-ones weights (one channel, or one per channel) -> c (c,)
    float64 such that y0 + c S has, in its worst image, |mean| / sigma closest to a drawn ratio in 2.5 .. 3.5."""
    import torch
    n, co = y0.shape[:2]
    a, b = y0.flatten(2), S.flatten(2).expand(n, co, -1)
    m0, mS = a.mean(2), b.mean(2)
    a0, b0 = a - m0[..., None], b - mS[..., None]
    v0, vS, cov = (a0 * a0).mean(2), (b0 * b0).mean(2), (a0 * b0).mean(2)
    want = 2.5 + torch.rand(co, generator=g, dtype=torch.float64)
    sign = (torch.rand(co, generator=g) < 0.5).double() * 2 - 1
    scale = (v0.mean(0).sqrt() / mS.abs().mean(0))                              # c of about one sigma of mean shift
    t = torch.logspace(-2, 3, 800, dtype=torch.float64)

    def best(sg):
        c = sg[None] * scale[None] * t[:, None]                                 # (grid, co)
        mean = m0[None] + c[:, None] * mS[None]                                 # (grid, n, co)
        var = v0[None] + 2 * c[:, None] * cov[None] + c[:, None] ** 2 * vS[None]
        miss = (mean.abs() / var.sqrt() - want[None, None]).abs().amax(1)       # worst image
        at = miss.argmin(0, keepdim=True)
        return c.gather(0, at)[0], miss.gather(0, at)[0]

    (c_a, miss_a), (c_b, miss_b) = best(sign), best(-sign)                      # the drawn sign, unless it cannot get there
    pick = torch.where(miss_a <= miss_b + 0.25, c_a, c_b)
    if skip is not None:
        pick[skip] = 0.0
    return pick


def _conv(r, v, w, b):
    import torch.nn.functional as F
    if r.kind == 1:
        return F.conv_transpose2d(v, w, b, 2, 1)
    if r.kind == 2:
        return F.conv_transpose3d(v, w, b, 2, 0)
    return (F.conv2d if r.nd == 2 else F.conv3d)(v, w, b, r.stride, pad_of(r))


def _operand(cs, x, recipe, dtype):
    """What the convolution's MFMAs see: x as it is, or (project_240) SiLU(InstanceNorm(x)) * gate."""
    if not cs.gate:
        return x.to(dtype)
    pool, inv_hw, params = recipe
    return OC.transformed(x, OC.SILU, OC.se_gate_ref(pool, inv_hw, *params, dtype=dtype), dtype)


def make_conv(cs, seed, n=None):
    import torch
    r = cs.row
    n = r.n if n is None else n
    g = torch.Generator().manual_seed(seed + 1)
    shape = (n, r.cin) + r.shape
    x = centred_input(seed, shape) if r.bias else onesigned_input(seed, shape, const=cs.const)
    taps = r.k ** r.nd if r.kind == 0 else (4 if r.kind == 1 else 1)
    if r.kind == 0:
        w = torch.randn((r.cout, r.cin) + (r.k,) * r.nd, generator=g, dtype=torch.float64) / (r.cin * taps) ** 0.5
    else:
        w = torch.randn((r.cin, r.cout) + ((4, 4) if r.kind == 1 else (2, 2, 2)), generator=g,
                        dtype=torch.float64) / (r.cin * taps) ** 0.5
    recipe = None
    if cs.gate:
        pool, inv_hw, params, _ = OC.row_gate(r, x, OC.SILU)
        recipe = (pool, inv_hw, params)
    v = _operand(cs, x, recipe, torch.float64)
    if cs.const:
        assert r.kind == 0 and not r.bias
        w[CO_CONST] = 0.0
        w[(CO_CONST, OC.CONST_CHANNEL) + (r.k // 2,) * r.nd] = W_CONST
    y0 = _conv(r, v, w, None)
    sp = tuple(range(2, y0.dim()))
    if r.bias:
        sigma = y0.var(sp, unbiased=False).mean(0).sqrt()
        ratio = 2.05 + 1.9 * torch.rand(r.cout, generator=g, dtype=torch.float64)
        sign = (torch.rand(r.cout, generator=g) < 0.5).double() * 2 - 1
        b = (sign * ratio * sigma - y0.mean((0,) + sp)).float()
        w = w.float()
    else:
        ones = torch.ones_like(w[:1]) if r.kind == 0 else torch.ones_like(w[:, :1])
        c = offcentre_constants(y0, _conv(r, v, ones, None), g, skip=CO_CONST if cs.const else None)
        w = (w + (c[(slice(None),) + (None,) * (w.dim() - 1)] if r.kind == 0
                  else c[(None, slice(None)) + (None,) * (w.dim() - 2)])).float()
        b = None
    ref = _conv(r, v, w.double(), b.double() if b is not None else None)
    return Case(x, w, b, ref, recipe)


def conv_fp32(cs, case):
    import torch
    return _conv(cs.row, _operand(cs, case.x, case.recipe, torch.float32), case.w, case.b)


def conv_seed(cs):
    return OC._seed(cs.row) + 7001


@lru_cache(maxsize=None)
def conv_case(cs):
    """The tensors and the float64 reference of a row: computed once, shared by the tests, never written to."""
    return make_conv(cs, conv_seed(cs))


def _dw(v, w):
    import torch.nn.functional as F
    return F.conv2d(v, w, None, 1, w.shape[-1] // 2, 1, w.shape[0])


def make_dw(row, seed, n=DW_N):
    import torch
    k, c, h, wd, _ = row
    const = row == DW_CONST
    g = torch.Generator().manual_seed(seed + 1)
    x = onesigned_input(seed, (n, c, h, wd), const=const)
    w = torch.randn(c, 1, k, k, generator=g, dtype=torch.float64) / k
    if const:
        w[OC.CONST_CHANNEL] = 0.0
        w[OC.CONST_CHANNEL, 0, k // 2, k // 2] = W_CONST
    v = x.double()
    cc = offcentre_constants(_dw(v, w), _dw(v, torch.ones_like(w)), g, skip=OC.CONST_CHANNEL if const else None)
    w = (w + cc[:, None, None, None]).float()
    return Case(x, w, None, _dw(v, w.double()), None)


@lru_cache(maxsize=None)
def dw_case(row):
    return make_dw(row, 811 * row[0] + 13 * row[1] + 5 * row[2] + row[3] + row[4])


def _stem(v, w):
    import torch.nn.functional as F
    return F.conv2d(v, w, None, 2, 1)


def make_stem(row, seed, n=STEM_N):
    import torch
    cout, h, wd = row
    const = row == STEM_CONST
    g = torch.Generator().manual_seed(seed + 1)
    x = onesigned_input(seed, (n, 3, h, wd), const=const)
    w = torch.randn(cout, 3, 3, 3, generator=g, dtype=torch.float64) / 27 ** 0.5
    if const:
        w[CO_CONST] = 0.0
        w[CO_CONST, OC.CONST_CHANNEL, 1, 1] = W_CONST       # the centre tap reads input pixel (2 oy, 2 ox)
    v = x.double()
    cc = offcentre_constants(_stem(v, w), _stem(v, torch.ones_like(w[:1])), g, skip=CO_CONST if const else None)
    w = (w + cc[:, None, None, None]).float()
    return Case(x, w, None, _stem(v, w.double()), None)


@lru_cache(maxsize=None)
def stem_case(row):
    return make_stem(row, 523 * row[0] + 7 * row[1] + row[2])


def offcentre_ratio(ref):
    """|mean| / sigma per (image, channel) of a float64 tensor."""
    v = ref.flatten(2)
    return v.mean(2).abs() / v.var(2, unbiased=False).sqrt()


# ---- nearly constant channels, the 2D code paths: |mean| / sigma of the output about NEAR_RATIO.  One row per path:
# (path, partial: how the pixels of an image are cut into the partials that reach exact_add_rounded, a, b: float32
# roundings on sum |d| and on sum d^2 of the pivoted sums, see the docstring)
NEAR_RATIO = 300.0
NEAR = {
    "epilogue2d": ("k1_8x16", 4, 6),          # conv_epilogue, MR 2: a = MR + 2, b = MR + 4; one partial per 8 x 16 tile
    "pw_direct": ("pwd_16_8", 12, 14),        # rbw = 8: a = rbw + 4, b = rbw + 6; one partial per wave of 128 pixels
    "depthwise": (DW_ROWS[0], 4, 6),          # 16-tile: a = nv, b = nv + 2; one partial per tile
    "stem": (STEM_ROWS[0], 0, 0),             # fp64 from the first addition on; one partial per 16 x 16 tile
}


def near_partials(path, y):
    """The pixels of y (n, c, h, w) grouped as the path's workgroups (conv_pw_direct: waves) group them -> list of
    (n, c, pixels) views, one per emitted partial."""
    if path == "pw_direct":
        v = y.flatten(2)
        step = 16 * pw_rbw(v.shape[2])
        return [v[:, :, p:p + step] for p in range(0, v.shape[2], step)]
    th, tw = (8, 16) if path == "epilogue2d" else (16, 16)
    h, w = y.shape[2:]
    return [y[:, :, i:i + th, j:j + tw].flatten(2) for i in range(0, h, th) for j in range(0, w, tw)]


def near_bar(y, a, b):
    """Per (image, channel): the bar on |s2 / P - (s1 / P)^2 - var(y)| for the sums a 2D producer emits (derivation:
    tests/test_hip_stats.py, test_nearly_constant_channels)."""
    v = y.double().flatten(2)
    P = v.shape[2]
    mean, A, Q = v.mean(2), v.abs().sum(2), (v * v).sum(2)
    R = (v - mean[..., None]).abs().amax(2)
    lim = 2.0 ** -31
    e1 = lim * A / P + 2 * a * U * R                       # bound on the error of s1 / P
    return lim * Q / P + 2 * mean.abs() * lim * A / P + 4 * (a + b) * U * R * R + e1 * e1 + 2.0 ** -48 * Q / P


def near_variance(sums, P):
    return sums[..., 1] / P - (sums[..., 0] / P) ** 2


@lru_cache(maxsize=None)
def near_case(path):
    """Tensors of the path's row with a nearly constant output: the input is mu_c (1 + noise), the weights are positive
    (convolutions, k = 1) or their centre tap dominates (depthwise, stem: the zero padding then moves a border pixel by
    1e-4 of its value, below the noise), and the noise is scaled, in float64 on the CPU, so that the median
    |mean| / sigma of the output channels is NEAR_RATIO."""
    import torch
    key = NEAR[path][0]
    g = torch.Generator().manual_seed(9001 + len(path))
    if path in ("epilogue2d", "pw_direct"):
        r = OC.BY_ID[key]
        assert r.k == 1 and r.kind == 0
        shape, n = (r.n, r.cin) + r.shape, r.n
        w = (torch.randn(r.cout, r.cin, 1, 1, generator=g).abs() / r.cin ** 0.5 + 0.01)
        f = lambda v: _conv(r, v, w.double(), None)
    elif path == "depthwise":
        k, c, h, wd, _ = key
        shape, n = (DW_N, c, h, wd), DW_N
        w = torch.randn(c, 1, k, k, generator=g) * 1e-4
        w[:, 0, k // 2, k // 2] = 0.5 + torch.rand(c, generator=g)
        f = lambda v: _dw(v, w.double())
    else:
        cout, h, wd = key
        shape, n = (STEM_N, 3, h, wd), STEM_N
        w = torch.randn(cout, 3, 3, 3, generator=g) * 1e-4
        w[:, :, 1, 1] = 0.2 + torch.rand(cout, 3, generator=g)
        f = lambda v: _stem(v, w.double())
    mu = 1.0 + 2.0 * torch.rand(shape[:2], generator=g, dtype=torch.float64)
    mu = mu[(...,) + (None,) * (len(shape) - 2)].expand(shape)
    z = torch.randn(shape, generator=g, dtype=torch.float64)
    base, noise = f(mu.contiguous()), f((mu * z).contiguous())
    s = (base.flatten(2).mean(2).abs() / noise.flatten(2).std(2)).median().item() / NEAR_RATIO
    x = (mu * (1 + s * z)).float()
    return Case(x, w, None, f(x.double()), None)
