"""GPU: the window form of ConvTranspose2d(k4, s2, p1) (csrc/deconv4.hip, deconv4_window_kernel).

Layers without fused statistics and gate -- the keypoint head -- run as ONE 2 x 2 convolution over
windows (outputs 2y - 1 and 2y read the same inputs {y - 1, y}) with 4 cout_p columns instead of four
parities padded to 16 columns each.  JH_DECONV4_WINDOW=0, read where the weights are packed, selects
the four-parity forms (the fused kernel, or the general four-phase path).  Per output value the order
of accumulation is the same in both, so the two must agree bit for bit; which form ran is told by the
library's count of window-form launches, never by the outputs.

Bar against torch on the CPU: that of tests/test_hip_ops.py (fp32 kernels with another summation
order: max abs error <= 2e-5 x the output's max magnitude).
"""
import pytest
import torch
import torch.nn.functional as F

from tests import cases
from tests.gpu_util import cuda, rel_err, report

pytestmark = pytest.mark.gpu

SWITCH = "JH_DECONV4_WINDOW"


def _launches():
    from jarvis_hybridnet_amd import _native as N
    return N.lib().jh_deconv4_window_launches()


def _deconv(x, w, b):
    """jh_op_conv kind 1; returns (y on the CPU, window launches).  For a ConvTranspose2d without statistics jh_op_conv
    fills the channel-last tensor the kernel stores into with NaN before the launch, so an output element that no
    workgroup writes reaches `y` as NaN (`y` itself is pre-filled too: nothing of it may be left)."""
    from jarvis_hybridnet_amd import _native as N
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    xc = cuda(x)
    y = torch.full((n, cout, 2 * h, 2 * wd), float("nan"), device="cuda")
    wh, bh = w.contiguous(), (b.contiguous() if b is not None else None)
    before = _launches()
    N.check(N.lib().jh_op_conv(2, 1, 4, 2, 1, cin, cout, wh.data_ptr(), bh.data_ptr() if bh is not None else None,
                               xc.data_ptr(), n, 1, h, wd, None, -1, y.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    return y.cpu(), _launches() - before


# cin, J, H, W, n, bias, takes the window form
SHAPES = [
    (64, 23, 8, 16, 2, False, True),      # exactly one interior tile plus edge windows
    (64, 23, 9, 17, 2, False, True),      # ragged interior tiles in both directions
    (64, 23, 5, 3, 1, True, True),        # image smaller than a tile
    (64, 23, 1, 1, 1, False, True),       # the corner window alone
    (64, 23, 64, 64, 12, False, True),    # more workgroups than CUs, two resident per CU; two edge workgroups
    (16, 8, 20, 12, 2, True, True),       # 32 columns, 16-channel passes
    (32, 17, 12, 12, 2, False, True),
    (64, 24, 8, 24, 2, False, True),      # no pad column
    (64, 30, 8, 16, 2, False, False),     # 128 columns: 8 blocks in either form, stays with the four parities
    (160, 23, 16, 16, 1, False, True),    # the large model
    (88, 23, 12, 12, 2, False, True),     # the half pair: the last channel pass holds three real 8-channel steps
    (88, 23, 9, 17, 1, True, True),
    (88, 23, 9, 8, 1, False, True),       # ... on an image 8 wide, where the general path takes its 8 x 8 tiles
    (64, 40, 12, 12, 2, False, False),    # 160 columns: the general four-phase path
]


@pytest.mark.parametrize("cin,J,H,W,n,bias,window", SHAPES)
def test_window_form_equals_four_parity_form(cin, J, H, W, n, bias, window, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    g = torch.Generator().manual_seed(8 + cin + H)
    x = torch.randn(n, cin, H, W, generator=g)
    w = torch.randn(cin, J, 4, 4, generator=g) / (cin * 4) ** 0.5     # asymmetric: catches tap / phase swaps
    b = torch.randn(J, generator=g) * 0.3 if bias else None
    ref = F.conv_transpose2d(x, w, b, 2, 1)
    y_w, ran_w = _deconv(x, w, b)
    monkeypatch.setenv(SWITCH, "0")
    y_p, ran_p = _deconv(x, w, b)
    e_w, e_p = rel_err(y_w, ref), rel_err(y_p, ref)
    report("deconv4_window", cin=cin, cout=J, h=H, w=W, rel_window=e_w, rel_parity=e_p, window_launches=ran_w)
    # every element is stored: the kernel's output tensor was all NaN before the launch (see _deconv)
    assert not torch.isnan(y_w).any() and not torch.isnan(y_p).any()
    assert e_w < 2e-5 and e_p < 2e-5
    assert ran_w == (1 if window else 0), "which form the default takes"
    assert ran_p == 0, SWITCH + "=0 must select the four-parity forms"
    assert torch.equal(y_w, y_p)


@pytest.mark.parametrize("tag", ["small_j23_b2", "medium_j23"])
def test_head_with_instance_norm_on_load(tag, monkeypatch):
    """The head's ConvTranspose2d inside EfficientTrack: its input's InstanceNorm + activation is applied while the
    patch is staged (64 channels, and the medium model's 88 = 5.5 pairs).  Both forms, bit for bit; accuracy against
    the oracle is tests/test_hip_stages.py::test_efficienttrack's."""
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd.efficienttrack.model import EfficientTrackBackbone
    monkeypatch.delenv(SWITCH, raising=False)
    size, J, N, hw, wseed, xseed = {**cases.EFFTRACK_CASES, **cases.EFFTRACK_GPU_CASES}[tag]
    sd = S.efficienttrack_weights(size, J, wseed)
    x = cuda(cases.efftrack_input(N, hw, xseed))

    def run():
        net = EfficientTrackBackbone(None, size, J)
        net.load_state_dict(sd, strict=True)
        before = _launches()
        res1, res2 = net(x)
        torch.cuda.synchronize()
        return res1.clone(), res2.clone(), _launches() - before

    r1_w, r2_w, ran_w = run()
    monkeypatch.setenv(SWITCH, "0")
    r1_p, r2_p, ran_p = run()
    assert ran_w >= 1 and ran_p == 0
    assert torch.equal(r1_w, r1_p) and torch.equal(r2_w, r2_p)
