"""GPU: everything a fused BiFPN node hands to its consumers -- y, the 2x2-max-pooled y and the InstanceNorm statistics --
in the kernel forms, segmentations and time-batch classes the network plans run (jh_op_bifpn_node_ex).

The cases are tests/node_cases.py's: every row of MODEL_ROWS / BOUNDARY_ROWS in a time-batch class with 3 (or 2) images;
tests/test_node_form_cpu.py proves that each runs its row's form, rows per segment and pooled output.  Inputs are
off-centre (tests/operand_cases.py), the reference is the expression of test_bifpn_node (tests/test_hip_ops.py) in torch
float64, and tests/test_node_cases_cpu.py shows that float32 evaluates it within 1e-5.

Bars.  y: 2e-5 of the maximum, the bar tests/test_hip_ops.py holds this node to.  Pooled output: bit-equal (max is
exact).  Behind an InstanceNorm (the chains): 2e-4, the file bar of tests/test_hip_ops.py times ten.

Statistics.  The node emits per (image, channel) the sum s1 and the sum of squares s2 of the y it stored; they are held
against the float64 sums of that same y:
    |s1 - sum v| <= d 2^-24 sum |v|,   |s2 - sum v^2| <= d 2^-24 sum v^2,
d the number of float32 roundings an addend can pass on its way into one partial.  Behind the partial everything is
exact: exact_add (csrc/jh_common.h) splits it on fixed grids into limbs whose fp64 atomics are exact, and the reader's two
fp64 additions cost 2^-52, far below one of the d roundings.  d per form, from the code:

  rows_wave, rows_pairs, rows_wg (csrc/bifpn_rows{,_ps,_wg}.hip): a lane adds the value of its pixel column row after
    row -- `s1 += v`, `s2 = fma(v, v, s2)`, one rounding per row, the product inside the fma unrounded -- over the rows
    of its segment, then row_sum() adds the 16 pixel lanes in four DPP steps:  d = seg_rows + 4  (the first addition, to
    zero, is exact; that spare rounding covers the reader).  seg_rows is the choice's (jh_node_form), at most 64.

  tile (csrc/bifpn_node.hip -> conv_epilogue<1, 4, 8, 16, 8> of csrc/conv_mfma.h): a lane holds four pixels of one row and
    one channel.  It subtracts a pivot m -- its first value: a lane's pixels are consecutive in a row, so when any of
    them lies inside the image the first does -- d_r = fl(v_r - m) (one rounding, relative to |v_r - m|), adds the four
    d_r in two float32 steps and the four fma(d_r, d_r, .) in three, and un-shifts in fp64:
    sum v = cnt m + sum d, sum v^2 = cnt m^2 + 2 m sum d + sum d^2.  Everything after that is fp64 (the waves' partials,
    then one limb rounded to 2^-31 relative).  With |v_r - v_0| <= |v_r| + |v_0|:
      sum:      3 roundings on sum |d_r| <= sum_{r>0} |v_r| + 3 |v_0| <= 3 sum |v|        -> 9, and 1 for the fp64 tail: 10
      squares:  2 |m| x 3 roundings on sum |d_r|: |v_0| (|v_r| + |v_0|) summed <= 4.5 sum v^2 -> 27;
                5 roundings (2 from d_r^2, 3 adds) on sum d_r^2 <= 6 sum v^2                 -> 30, and 1: 58
    These are worst cases (a lane whose first value dwarfs the others); on these inputs, whose values sit within a few
    sigma of the bias, the measured error is far smaller.

d 2^-24 H W <= 1 / 8 on every case (tests/test_node_cases_cpu.py), and the bias makes every pixel about 1 / (H W) of its
channel's sum: one dropped or double-counted pixel is eight bounds away.

Measured on an MI355X (the report() lines node_outputs and node_chain of parity.jsonl): see DESIGN.md, section 3.2."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import node_cases as NC
from tests.gpu_util import cuda, rel_err, report

pytestmark = pytest.mark.gpu

CASES = NC.cases()
BAR_Y, BAR_CHAIN = 2e-5, 2e-4
U = 2.0 ** -24


class Out:
    def __init__(self, y, y_pool, written, sums):
        self.y, self.y_pool, self.written, self.sums = y, y_pool, written, sums


def run_node(node, cls, want_pool, nd, xs=None, sums=None, counts=None):
    """One jh_op_bifpn_node_ex call -> Out (CPU tensors).  xs: other inputs than nd.xs (same parameters); sums / counts:
    per input the (n, c, 2) float64 statistics and the pixel count that replace the input's own, or None."""
    from jarvis_hybridnet_amd import _native as N
    c, cout, h, w, modes, act, n = node
    xs = nd.xs if xs is None else xs
    assert all(x.shape[0] == n for x in xs)
    dev = [cuda(x) for x in xs] + [None] * (3 - len(xs))
    y = torch.empty((n, cout, h, w), device="cuda")
    # (the entry fills its own buffers with NaN; these are only copied into -- NaN here too, so that a copy that did not
    #  happen cannot pass either)
    y.fill_(float("nan"))
    y_pool = torch.full((n, cout, h // 2, w // 2), float("nan"), device="cuda")
    out_sums = torch.full((n, cout, 2), float("nan"), dtype=torch.float64)
    written = ctypes.c_int32(-1)
    ex = N.OpNodeEx()
    ex.batch_class, ex.want_pool = cls, want_pool
    keep = []
    for i in range(len(modes)):
        if sums is not None and sums[i] is not None:
            t = sums[i].double().contiguous()
            assert t.shape == (n, c, 2)
            keep.append(t)
            ex.in_sums_host[i] = t.data_ptr()
            ex.in_count[i] = int(counts[i])
    ex.y_pool_dev = y_pool.data_ptr()
    ex.pool_written_host = ctypes.pointer(written)
    ex.out_sums_host = out_sums.data_ptr()
    m3 = (ctypes.c_int * 3)(*(list(modes) + [0] * (3 - len(modes))))
    w3 = (ctypes.c_float * 3)(*([float(v) for v in nd.wts] + [0.0] * (3 - len(modes))))
    N.check(N.lib().jh_op_bifpn_node_ex(len(modes), m3, w3, act, n, c, cout, h, w, N.ptr(dev[0]), N.ptr(dev[1]),
                                        N.ptr(dev[2]), nd.dw.contiguous().data_ptr(), nd.pw.contiguous().data_ptr(),
                                        nd.bias.contiguous().data_ptr(), y.data_ptr(), ctypes.byref(ex), N.stream()))
    torch.cuda.synchronize()
    assert written.value in (0, 1)
    return Out(y.cpu(), y_pool.cpu() if written.value else None, written.value, out_sums)


_RUNS = {}


def case_run(case):
    """The case on the GPU, once: y, the pooled output and the statistics come from ONE launch, as a consumer gets them."""
    if case not in _RUNS:
        _RUNS[case] = run_node(case.node, case.cls, case.want_pool, NC.case_tensors(case))
    return _RUNS[case]


def stat_errors(out, want):
    """Per (image, channel): |s1 - sum v| / sum |v| and |s2 - sum v^2| / sum v^2 of the kernel's own y, with their bounds."""
    v = out.y.double()
    a1, r1, r2 = v.abs().sum((2, 3)), v.sum((2, 3)), (v * v).sum((2, 3))
    d1, d2 = NC.stat_depth(want)
    e1 = ((out.sums[..., 0] - r1).abs() / a1).max().item()
    e2 = ((out.sums[..., 1] - r2).abs() / r2).max().item()
    return e1, d1 * U, e2, d2 * U


@pytest.mark.parametrize("case", CASES, ids=lambda k: k.id)
def test_y_pool_and_statistics(case):
    """y against float64; the pooled output against max_pool2d of the y the kernel returned, written exactly where the
    choice says so; the emitted statistics against the float64 sums of that y (the bounds: this file's docstring)."""
    nd, out = NC.case_tensors(case), case_run(case)
    e = rel_err(out.y, nd.ref)
    e1, b1, e2, b2 = stat_errors(out, case.want)
    pool_equal = out.written and torch.equal(out.y_pool, F.max_pool2d(out.y, 2, 2))
    report("node_outputs", case=case.id, form=case.want[0], seg_rows=case.want[1], rel=e, pool=out.written,
           pool_equal=int(bool(pool_equal)), s1_err=e1, s1_bound=b1, s2_err=e2, s2_bound=b2)
    print("node_outputs %s %s rel=%.3g s1 %.3g / %.3g s2 %.3g / %.3g" % (case.id, case.want[0], e, e1, b1, e2, b2))
    assert e < BAR_Y
    assert out.written == case.want[8]
    if out.written:
        assert pool_equal
    assert e1 <= b1 and e2 <= b2


def chain_id(ch):
    return "%d_%s_%s" % (ch[0], ("size", "below8", "atleast8")[ch[1]], "_".join(str(s) for s in ch[2]))


@pytest.mark.parametrize("chain", NC.CHAINS, ids=chain_id)
def test_chain_as_the_plans_wire_it(chain):
    """The producer runs with want_pool; the consumer's third same-level input is the producer's pooled output with the
    producer's EMITTED sums and the producer's pixel count (EffTrackPlan::node: pooled->st, pooled->inv) -- a tensor of
    H W / 4 pixels normalised with statistics over H W.  Reference: the whole chain in float64,
    max_pool2d(instance_norm(y_producer))."""
    c, cls, levels = chain
    ks = NC.chain_nodes(CASES, c, cls, levels)
    seed = 7919 * c + 31 * cls + levels[0]
    nd = NC.make_node(ks[0].node, seed)
    out = run_node(ks[0].node, cls, 1, nd)
    assert out.written == 1 and rel_err(out.y, nd.ref) < BAR_Y
    for i, k in enumerate(ks[1:]):
        hp, wp = ks[i].node[2], ks[i].node[3]
        v2 = F.max_pool2d(F.instance_norm(nd.ref, eps=1e-5), 2, 2)
        nd = NC.make_node(k.node, seed + 1 + i, given={2: (out.y_pool, v2)})
        out = run_node(k.node, cls, 1, nd, sums=[None, None, out.sums], counts=[0, 0, hp * wp])
        e = rel_err(out.y, nd.ref)
        e1, b1, e2, b2 = stat_errors(out, k.want)
        report("node_chain", chain=chain_id(chain), level=k.node[2], form=k.want[0], rel=e, s1_err=e1, s1_bound=b1,
               s2_err=e2, s2_bound=b2)
        print("node_chain %s level %d %s rel=%.3g" % (chain_id(chain), k.node[2], k.want[0], e))
        assert e < BAR_CHAIN
        assert out.written == k.want[8]
        assert not out.written or torch.equal(out.y_pool, F.max_pool2d(out.y, 2, 2))
        assert e1 <= b1 and e2 <= b2


# one case per (form, channel count) in a time-batch class, with the pooled output where the form writes it
TWICE = [
    ((56, 56, 32, 32, (0, 1), 2), NC.BELOW8, 0),            # tile
    ((88, 88, 16, 16, (0, 0, 3), 2), NC.ATLEAST8, 0),       # tile, more than 64 channels
    ((56, 56, 64, 64, (0, 1), 2), NC.ATLEAST8, 1),          # rows_wave
    ((88, 88, 64, 64, (0, 1), 2), NC.ATLEAST8, 1),          # rows_pairs
    ((88, 88, 32, 32, (0, 0, 0), 2), NC.BELOW8, 1),         # rows_wg, many short segments
    ((88, 88, 40, 40, (0, 0, 0), 2), NC.ATLEAST8, 1),       # rows_wg on a ragged level
    ((160, 160, 32, 32, (0, 0, 0), 2), NC.ATLEAST8, 1),     # rows_wg
]


def test_twice_covers_every_form_and_width():
    ks = [NC.by_key(CASES, *t) for t in TWICE]
    assert {(k.want[0], k.node[0]) for k in ks} == {("tile", 56), ("tile", 88), ("rows_wave", 56), ("rows_pairs", 88),
                                                    ("rows_wg", 88), ("rows_wg", 160)}
    assert {(k.want[0], k.node[0]) for k in CASES} - {(k.want[0], k.node[0]) for k in ks} == set()


@pytest.mark.parametrize("key", TWICE, ids=lambda t: NC.case_id(t[0] + (0,), t[1], t[2]))
def test_image_count_does_not_change_the_bits(key):
    """choose_node's invariant (csrc/node_layer.hip: the segmentation of a time-batch class does not look at the image
    count): the same n images first in a launch of 2 n give the same y, pooled output and statistics, bit for bit."""
    case = NC.by_key(CASES, *key)
    nd, one = NC.case_tensors(case), case_run(case)
    n = case.node[6]
    other = NC.make_node(case.node, 424243 + case.node[0] + case.node[2])
    xs = [torch.cat([a, b]) for a, b in zip(nd.xs, other.xs)]
    two = run_node(case.node[:6] + (2 * n,), case.cls, case.want_pool, nd, xs=xs)
    assert two.written == one.written == case.want[8]
    assert torch.equal(two.y[:n], one.y)
    assert not one.written or torch.equal(two.y_pool[:n], one.y_pool)
    assert torch.equal(two.sums[:n], one.sums)
    assert not torch.equal(two.y[n:], one.y)                 # (the other images are other images)
