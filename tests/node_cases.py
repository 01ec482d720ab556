"""Cases, inputs and float64 references of the fused BiFPN node's output tests (tests/test_hip_node_outputs.py on the
GPU; tests/test_node_form_cpu.py and tests/test_node_cases_cpu.py for the table and the reference themselves).

The cases are the nodes the network plans run, not invented shapes: every row of MODEL_ROWS and every row of
BOUNDARY_ROWS that carries a time-batch class (tests/test_node_form_cpu.py), with the image count replaced by 3 -- or by
2 where three images would change the choice: the producer / consumer pairs need strips * segs * n % 4 == 0.  The
segmentation of a time-batch class does not look at the image count, so the case runs the kernel form, the rows per
segment and the pooled output of its row; tests/test_node_form_cpu.py asks jh_node_form that this is so.

The table is plain Python; what needs torch imports it where it is used.

Inputs follow tests/operand_cases.py: every (image, channel) of every input has its own sigma in [0.5, 2] and a mean of
+-(2.05 .. 3.95) sigma, channel CONST_CHANNEL of image 0 of the first input is constant, and the pointwise bias is
+-(2 .. 4) times the per-channel sigma of the output without it -- each output pixel then carries about 1 / (H W) of its
channel's sum, which is what lets the statistics check see a single pixel."""
from collections import namedtuple
from functools import lru_cache

BY_SIZE, BELOW8, ATLEAST8 = 0, 1, 2
SAME, UP2, UP4, POOL2 = 0, 1, 2, 3
FORMS = ("tile", "rows_wave", "rows_pairs", "rows_wg")

# node: (C, Cout, H, W, modes, act, n) as jh_node_form takes it; want: the table row's choice (name, seg_rows, strips,
# segs, grid.x, grid.y, block.x, lds, pool) -- the grid is the row's, at ITS image count
NodeCase = namedtuple("NodeCase", "id node cls want_pool want")


def case_images(want):
    """Images of a case: 3, or 2 where three would take a node of the pair form out of it."""
    name, _, strips, segs = want[:4]
    return 2 if name == "rows_pairs" and strips * segs * 3 % 4 else 3


def case_id(node, cls, want_pool):
    c, cout, h, w, modes, act, n = node
    return "%dx%d_%dx%d_m%s_a%d_n%d_%s%s" % (c, cout, h, w, "".join(str(m) for m in modes), act, n,
                                            ("size", "below8", "atleast8")[cls], "_pool" if want_pool else "")


def runnable(node):
    """Up-sampled inputs of whole pixels.  (One BOUNDARY_ROWS row pins the choice of a 63-row node with a x2 input; no
    such tensor exists -- a 31-row input has no source for output row 62 -- and the operator entry refuses it.)"""
    h, w, modes = node[2], node[3], node[4]
    step = 4 if UP4 in modes else (2 if UP2 in modes else 1)
    return h % step == 0 and w % step == 0


def make_cases(rows):
    """rows of (node, class, want_pool, choice) -> the distinct cases of the rows in a time-batch class."""
    out, seen = [], set()
    for node, cls, want_pool, want in rows:
        if cls == BY_SIZE or not runnable(node):
            continue
        node = tuple(node[:6]) + (case_images(want),)
        key = (node, cls, want_pool)
        if key in seen:
            continue
        seen.add(key)
        out.append(NodeCase(case_id(node, cls, want_pool), node, cls, want_pool, tuple(want)))
    return out


def cases():
    from tests.test_node_form_cpu import BOUNDARY_ROWS, MODEL_ROWS
    return make_cases(MODEL_ROWS + BOUNDARY_ROWS)


def input_shape(mode, h, w):
    return {SAME: (h, w), UP2: (h // 2, w // 2), UP4: (h // 4, w // 4), POOL2: (h * 2, w * 2)}[mode]


# ---- statistics: fp32 additions on the longest path into one partial (derivations: tests/test_hip_node_outputs.py)
TILE_D1, TILE_D2 = 10, 58


def stat_depth(want):
    """(d of the sum, d of the sum of squares) of the form a choice names."""
    name, seg_rows = want[0], want[1]
    return (TILE_D1, TILE_D2) if name == "tile" else (seg_rows + 4, seg_rows + 4)


# ---- tensors and references (torch)
Node = namedtuple("Node", "xs wts dw pw bias ref")       # float32 inputs and parameters, float64 reference of y


def _seed(node, cls, want_pool):
    c, cout, h, w, modes, act, n = node
    return 100003 * c + 1009 * h + 53 * w + 7 * sum((i + 1) * (m + 1) for i, m in enumerate(modes)) + 3 * cls + want_pool


def resampled(v, mode):
    import torch.nn.functional as F
    if mode == UP2:
        return F.interpolate(v, scale_factor=2, mode="nearest")
    if mode == UP4:
        return F.interpolate(v, scale_factor=4, mode="nearest")
    if mode == POOL2:
        return F.max_pool2d(v, 2, 2)
    return v


def node_expr(vs, modes, act, wts, dw, pw, bias, dtype):
    """The expression of test_bifpn_node (tests/test_hip_ops.py) behind the InstanceNorm: vs are the NORMALISED inputs at
    their own resolution -> pointwise(depthwise3x3(act(sum_k w_k resample_k(v_k)))) + bias in `dtype`."""
    import torch.nn.functional as F
    fused = 0
    for v, m, wk in zip(vs, modes, wts.to(dtype)):
        fused = fused + wk * resampled(v.to(dtype), m)
    if act == 2:
        fused = F.silu(fused)
    elif act == 1:
        fused = F.relu(fused)
    C = dw.shape[0]
    y = F.conv2d(F.conv2d(fused, dw.to(dtype), None, 1, 1, 1, C), pw.to(dtype)[:, :, None, None])
    return y if bias is None else y + bias.to(dtype)[None, :, None, None]


def make_node(node, seed, given=None):
    """The tensors of a node.  given: {input index: (x float32, v float64)} -- an input that exists already (a
    producer's pooled output) with the normalised values the float64 reference takes for it; every other input is drawn
    (tests/operand_cases.py: operand_input).  The bias is +-(2.05 .. 3.95) x the sigma of the output without it."""
    import torch
    from tests import operand_cases as OC
    c, cout, h, w, modes, act, n = node
    given = given or {}
    g = torch.Generator().manual_seed(seed)
    xs, vs = [], []
    for i, m in enumerate(modes):
        if i in given:
            x, v = given[i]
        else:
            x = OC.operand_input(seed + 17 * (i + 1), (n, c) + input_shape(m, h, w), const=(i == 0))
            v = OC.inorm(x, torch.float64)
        xs.append(x)
        vs.append(v)
    wts = torch.rand(len(modes), generator=g) + 0.2
    wts = wts / (wts.sum() + 1e-4)
    dw = torch.randn(c, 1, 3, 3, generator=g) / 3
    pw = torch.randn(cout, c, generator=g) / c ** 0.5
    y0 = node_expr(vs, modes, act, wts, dw, pw, None, torch.float64)
    sigma = y0.var((0, 2, 3), unbiased=False).sqrt()
    ratio = 2.05 + 1.9 * torch.rand(cout, generator=g, dtype=torch.float64)
    sign = (torch.rand(cout, generator=g) < 0.5).double() * 2 - 1
    bias = (sign * ratio * sigma).float()
    return Node(xs, wts, dw, pw, bias, y0 + bias.double()[None, :, None, None])


def node_fp32(node, nd):
    """The reference expression in float32: InstanceNorm from the float64 sums as the kernels take it (OC.inorm)."""
    import torch
    from tests import operand_cases as OC
    modes, act = node[4], node[5]
    return node_expr([OC.inorm(x, torch.float32) for x in nd.xs], modes, act, nd.wts, nd.dw, nd.pw, nd.bias,
                     torch.float32)


@lru_cache(maxsize=None)
def case_tensors(case):
    """The tensors and the float64 reference of a table case: computed once, shared by the tests, never written to."""
    return make_node(case.node, _seed(case.node, case.cls, case.want_pool))


def by_key(all_cases, node6, cls, want_pool):
    """The table case of a node (C, Cout, H, W, modes, act) in a class: the tests that pick cases pick them from the
    table, so that they too run what a plan runs."""
    hit = [k for k in all_cases if k.node[:6] == tuple(node6) and k.cls == cls and k.want_pool == want_pool]
    assert len(hit) == 1, (node6, cls, want_pool, len(hit))
    return hit[0]


# ---- chains, as EffTrackPlan::node wires them: the producer runs with want_pool, the consumer's third same-level input
# is the producer's pooled output with the producer's emitted sums and the producer's pixel count.  (C, class, levels)
CHAINS = [
    (56, ATLEAST8, (64, 32)),
    (88, ATLEAST8, (80, 40, 20)),        # pairs, then the workgroup form on the ragged levels
    (88, BELOW8, (64, 32, 16)),
    (160, ATLEAST8, (64, 32, 16)),
]


def chain_nodes(all_cases, c, cls, levels):
    """The table cases of a chain: the top-down node of the first level, then bottom-up nodes with three same-level
    inputs.  One image count for the chain: the smallest of its cases (2 where the first node is of the pair form)."""
    ks = [by_key(all_cases, (c, c, levels[0], levels[0], (SAME, UP2), 2), cls, 1)]
    ks += [by_key(all_cases, (c, c, s, s, (SAME, SAME, SAME), 2), cls, 1) for s in levels[1:]]
    n = min(k.node[6] for k in ks)
    return [k._replace(node=k.node[:6] + (n,)) for k in ks]
