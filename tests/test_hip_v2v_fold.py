"""GPU: the V2V output fold (csrc/conv3d_out_fold.hip) against the three launches it replaces, bit for bit.

A plan built under JH_V2V_FOLD=0 ends in norm_apply (skip_res1), norm_apply (decoder_res1), conv3d_k1s1 (output layer);
a plan built under the default ends in one launch that applies both closing passes on load.  Both plans live in this
process, take the same seeded weights and the same inputs, and must give `torch.equal` outputs: the fold derives mean /
rstd with norm_apply's expressions, evaluates its terms in its order and keeps the MFMA sequence of the general
kernel, so there is no tolerance to set.  Which form a plan took is read from the launch names of a profiled forward.
"""
import ctypes

import pytest
import torch

from tests import cases
from tests.gpu_util import cuda

pytestmark = pytest.mark.gpu


def _plan(sd, J, T, G, fold, monkeypatch):
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd.hybridnet.v2vnet import _Plan
    if fold:
        monkeypatch.delenv("JH_V2V_FOLD", raising=False)
    else:
        monkeypatch.setenv("JH_V2V_FOLD", "0")
    return _Plan(N.Params(sd), J, T, G)


def _run(plan, x, J):
    """(output, launch names) of one profiled forward."""
    from jarvis_hybridnet_amd import _native as N
    g = x.shape[2] // 2
    out = torch.empty((x.shape[0], J, g, g, g), device="cuda")
    recs = N.profile(lambda: N.check(N.lib().jh_v2v_forward(plan.handle, N.ptr(x), N.ptr(out), N.stream())))
    torch.cuda.synchronize()
    return out, [r[0] for r in recs]


def _says_fold(J, T, G):
    from jarvis_hybridnet_amd import _native as N
    f = ctypes.c_int(-1)
    N.check(N.lib().jh_v2v_fold(J, T, G, ctypes.byref(f)))
    return bool(f.value)


def _volumes(J, T, G, seed, zero_slot=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(T, J, G, G, G, generator=g)
    x = (x * x * x).contiguous()          # the 0..1 range V2V sees, a different volume per frame set
    if zero_slot is not None:
        x[zero_slot] = 0.0
    return x


def _tail(names):
    """Launch names behind the last Winograd launch."""
    last = max(i for i, n in enumerate(names) if "wino" in n)
    return names[last + 1:]


# (J, G, T, zero slot, folds): flagship channels at P = 512; Gh = 12 (P = 1728, no power of two: the `/ (double)P`
# derivation); the 64-channel operand with 32 output columns; few channels with pad channels in both operands; Gh = 10
# (P = 1000, no whole number of 16-voxel row blocks: the plan keeps the three launches); the larger time batch; and a zero
# volume in slot 1, whose r_skip / r_dec channels are constant over the frame set (variance clamp and eps path)
SHAPES = [
    (23, 16, 3, None, True),
    (23, 24, 3, None, True),
    (30, 16, 3, None, True),
    (5, 16, 3, None, True),
    (23, 20, 3, None, False),
    (23, 16, 9, None, True),
    (23, 16, 3, 1, True),
    # ... and the kernel's other instantiations (8-channel steps 1, 3, 4, 5, 7 beside the 2, 6 and 8 above; 5 is the
    # one whose prefetching form was withdrawn, see csrc/conv3d_out_fold.hip)
    (3, 16, 3, None, True),
    (10, 16, 3, None, True),
    (14, 16, 3, None, True),
    (18, 16, 3, None, True),
    (26, 16, 3, None, True),
]


@pytest.mark.parametrize("J,G,T,zero_slot,folds", SHAPES)
def test_fold_equals_three_launches(J, G, T, zero_slot, folds, monkeypatch):
    from jarvis_hybridnet_amd import synthetic as S
    sd = S.v2v_weights(J, 7)
    x = cuda(_volumes(J, T, G, 100 + J + G + T, zero_slot))
    off = _plan(sd, J, T, G, False, monkeypatch)
    assert not _says_fold(J, T, G)                    # the knob as it stands: off
    on = _plan(sd, J, T, G, True, monkeypatch)
    assert _says_fold(J, T, G) == folds
    y_off, n_off = _run(off, x, J)
    y_on, n_on = _run(on, x, J)
    y_off2, _ = _run(off, x, J)                       # both plans stay usable side by side
    fold_name = "conv3d_k1s1fold_%dx%d@%d" % (2 * J, J, G // 2)
    plain_name = "conv3d_k1s1_%dx%d@%d" % (2 * J, J, G // 2)
    assert fold_name not in n_off and _tail(n_off) == ["norm_apply", plain_name]
    if folds:
        assert len(n_on) == len(n_off) - 2
        assert _tail(n_on) == [fold_name]
        assert n_on.count("norm_apply") == n_off.count("norm_apply") - 2
    else:
        assert n_on == n_off
    assert bool(torch.isfinite(y_off).all())
    if zero_slot is None:
        assert float((y_off[0] - y_off[1]).abs().max()) > 0      # the frame sets differ: a wrong statistics row shows
    assert torch.equal(y_on, y_off)
    assert torch.equal(y_off2, y_off)
    on.close()
    off.close()


def test_predictor_with_fold_equals_without(monkeypatch):
    """NativePredictor on the cfg2 geometry, time batch 2 with two different frame sets: fold on against fold off --
    points, confidences, validity, and the final heat map of the 3D stage on seeded crops."""
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd import synthetic as S
    from jarvis_hybridnet_amd._predictor import NativePredictor
    c = cases.PREDICTOR_CASES["cfg2"]
    inp = cases.predictor_inputs("cfg2")
    hyb = cases.hybrid_inputs("cfg2")
    calib = (inp["cam"], inp["intr"], inp["dist"])
    T = 2
    kw = dict(num_cameras=c["C"], num_joints=c["J"], center_size=c["center_size"], bbox=c["bbox"],
              roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"],
              mean=S.MEAN, std=S.STD, time_batch=T)
    monkeypatch.setenv("JH_V2V_FOLD", "0")
    p_off = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    monkeypatch.delenv("JH_V2V_FOLD")
    p_on = NativePredictor(inp["sd_center"], inp["sd_hybrid"], **kw)
    assert p_on.launches == p_off.launches - 2
    dev = [cuda(t) for t in calib]
    frames = cuda(torch.stack([inp["imgs"], S.blob_frames(calib, c["W"], c["H"], c["J"], 61)[0]]))
    g = torch.Generator().manual_seed(5)
    crops = cuda(torch.randn(T, c["C"], 3, c["bbox"], c["bbox"], generator=g))
    chm = cuda(hyb["center_hm"].int().expand(T, -1, -1).contiguous())
    c3 = cuda(hyb["center3d"].int().expand(T, -1).contiguous())
    res = {}
    for tag, p in (("off", p_off), ("on", p_on)):
        p.set_calibration(*dev)
        names = []
        out = []

        def go():
            out.extend(t.clone() for t in p.forward(frames))
        names = [r[0] for r in N.profile(go)]
        fin, _, pts, conf = p.hybridnet_forward(crops, chm, c3, want_padded=False)
        torch.cuda.synchronize()
        res[tag] = out + [fin, pts, conf]
        Gh = int(c["roi"] / c["spacing"]) // 2
        fold_name = "conv3d_k1s1fold_%dx%d@%d" % (2 * c["J"], c["J"], Gh)
        assert (fold_name in names) == (tag == "on")
    for a, b in zip(res["on"], res["off"]):
        # (bit patterns: rows of a frame set that is not valid are NaN in both)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    fin = res["off"][3]
    assert bool(torch.isfinite(fin).all()) and float((fin[0] - fin[1]).abs().max()) > 0
    p_on.close()
    p_off.close()
