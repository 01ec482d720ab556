"""CPU: per-joint camera masks (jh_predictor_set_joint_mask) -- the normalisation of the joint_mask argument and its
errors, the reference's effective-set rule (tests/joint_mask_ref.py) on hand-made rows, the new symbols in the header,
the ctypes table and the built library with their GPU-free refusals, the CSV helpers, and the refusals of the driver
and of the camera-sharded path.  No kernel runs here; tests/test_hip_joint_mask.py holds the GPU side.  Every test
uses a name this feature adds."""
import csv
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import joint_mask_ref as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("jh_predictor_set_joint_mask", "jh_predictor_get_joint_mask", "jh_predictor_stage_3d_joint_masked",
       "jh_reproject_joint_masked_workspace_bytes", "jh_reproject_forward_joint_masked")


def test_joint_mask_argument():
    from jarvis_hybridnet_amd import _native as N
    T, J, C = 2, 3, 4
    assert N.joint_mask(None, T, J, C) is None
    for value in ("consensus", True):
        mode, p = N.joint_mask(value, T, J, C)
        assert mode == N.JOINT_MASK_CONSENSUS and isinstance(p, N.Joints3dParamsStruct)
        assert (p.min_views, p.refine_radius) == (2, 1) and p.min_conf == np.float32(0.1) and p.max_error_px == 8.0
    mode, p = N.joint_mask(dict(max_error_px=5.0, refine_radius=2), T, J, C)
    assert mode == N.JOINT_MASK_CONSENSUS and p.max_error_px == 5.0 and p.refine_radius == 2
    made = N.joints3d_params(3, 0, 0.2, 4.0)
    assert N.joint_mask(made, T, J, C) == (N.JOINT_MASK_CONSENSUS, made)
    # a mask: bool or integer, tensor, array or sequence; nonzero = on; (J,C) at T = 1
    m = torch.zeros((T, J, C), dtype=torch.int64)
    m[0, 1, 2], m[1, 2, 3] = 7, -1
    mode, got = N.joint_mask(m, T, J, C)
    assert mode == N.JOINT_MASK_GIVEN and got.dtype == torch.uint8 and got.is_contiguous()
    assert got.tolist() == (m != 0).int().tolist()
    assert N.joint_mask(m.bool().numpy(), T, J, C)[1].tolist() == got.tolist()
    assert N.joint_mask(m.tolist(), T, J, C)[1].tolist() == got.tolist()
    assert tuple(N.joint_mask(m[0], 1, J, C)[1].shape) == (1, J, C)
    # what a Triangulated3D's members are
    members = torch.ones((T, J, C), dtype=torch.uint8)
    assert N.joint_mask(members, T, J, C)[1].tolist() == members.tolist()
    for bad in (False, "yes", "", m.float(), m[0], m[:, :, :3], torch.zeros((T, C, J)), [[1, 0], [1]], 5):
        with pytest.raises(ValueError):
            N.joint_mask(bad, T, J, C)
    with pytest.raises(ValueError, match="refine_radius"):
        N.joint_mask(dict(refine_radius=4), T, J, C)
    with pytest.raises(TypeError):
        N.joint_mask(dict(radius=1), T, J, C)


def test_effective_set_rule_on_hand_made_rows():
    # one frame set, four joints, three cameras: full, single camera, empty (falls back), two cameras
    jm = [[[1, 1, 1], [0, 1, 0], [0, 0, 0], [1, 0, 2]]]
    e, n = R.effective_sets(jm)
    assert e.dtype == np.uint8 and n.dtype == np.int32
    assert e.tolist() == [[[1, 1, 1], [0, 1, 0], [1, 1, 1], [1, 0, 1]]] and n.tolist() == [[3, 1, 3, 2]]
    # under a camera mask: jm & m; the single-camera joint loses its camera and falls back to the mask's cameras
    e, n = R.effective_sets(jm, [[1, 0, 1]])
    assert e.tolist() == [[[1, 0, 1], [1, 0, 1], [1, 0, 1], [1, 0, 1]]] and n.tolist() == [[2, 2, 2, 2]]
    # ... which is the rule on jm & m without a camera mask wherever a camera is left, and differs in the fallback
    both = (np.asarray(jm) != 0) & np.array([1, 0, 1], bool)
    e2, n2 = R.effective_sets(both)
    assert e2[0, [0, 3]].tolist() == e[0, [0, 3]].tolist() and e2[0, 1].tolist() == [1, 1, 1]
    # no camera at all: empty sets, count 0; rows are independent
    e, n = R.effective_sets(jm + jm, [[0, 0, 0], [1, 1, 1]])
    assert not e[0].any() and n[0].tolist() == [0] * 4 and n[1].tolist() == [3, 1, 3, 2]
    # all ones is the camera mask, all zeros too
    ones, zeros = np.ones((2, 4, 3), np.uint8), np.zeros((2, 4, 3), np.uint8)
    m = [[1, 1, 0], [0, 1, 0]]
    for x in (ones, zeros):
        e, n = R.effective_sets(x, m)
        assert (e == np.asarray(m, np.uint8)[:, None, :]).all() and n.tolist() == [[2] * 4, [1] * 4]


def test_gather_reference_selects_and_divides():
    # two cameras, two joints, hs = 2, G = 1: the one voxel taps pixel 3 of camera 0 and pixel 0 of camera 1
    hm = torch.tensor([[[[0., 0.], [0., 6.]], [[0., 0.], [0., float("nan")]]],
                       [[[2., 0.], [0., 0.]], [[5., 0.], [0., 0.]]]])
    idx = torch.tensor([3, 0]).reshape(2, 1, 1, 1)
    vol = R.gather_ref(hm, idx, [[1, 1], [0, 1]])
    assert vol.reshape(2).tolist() == [4.0, 5.0]                 # (6 + 2) / 2; the NaN is selected out: 5 / 1
    assert R.gather_ref(hm, idx, [[0, 0], [0, 0]]).reshape(2).tolist() == [0.0, 0.0]


def test_symbols_in_header_ctypes_table_and_library():
    from jarvis_hybridnet_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jarvis_hip.h")).read(), flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in N.symbols() and hasattr(lib, name)
    for k, v in (("OFF", 0), ("GIVEN", 1), ("CONSENSUS", 2)):
        assert re.search(r"#define JH_JOINT_MASK_%s %d\b" % (k, v), text) and getattr(N, "JOINT_MASK_" + k) == v
    assert lib.jh_abi_version() == 4
    # refusals that need no GPU: nothing is enqueued
    assert lib.jh_predictor_set_joint_mask(None, 1, None, None, None) != 0 and b"null predictor" in lib.jh_last_error()
    assert lib.jh_predictor_get_joint_mask(None, None, None, None) != 0 and b"null predictor" in lib.jh_last_error()
    assert lib.jh_predictor_stage_3d_joint_masked(None, None, 0, None, None, None, None, None, None) != 0
    assert lib.jh_reproject_forward_joint_masked(*([None, 2, 3, 16] + [None] * 5 + [8, 4.0] + [None] * 4 + [0, None])) != 0
    assert b"workspace" in lib.jh_last_error()
    plain = lib.jh_reproject_workspace_bytes(4, 23, 130, 48)
    assert plain < lib.jh_reproject_joint_masked_workspace_bytes(4, 23, 130, 48) <= plain + 1024


def test_csv_helpers():
    from jarvis_hybridnet_amd.joint_mask import JointMask, create_header_joint_cameras, joint_cameras_row
    assert JointMask._fields == ("cameras", "count")
    assert create_header_joint_cameras(["nose", "tail"]) == [["nose", "nose", "tail", "tail"],
                                                             ["count", "cameras", "count", "cameras"]]
    cams = [[1, 1, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]]
    assert joint_cameras_row(cams, [3, 0, 1]) == [3, 11, 0, 0, 1, 4]
    assert joint_cameras_row(torch.tensor(cams).tolist(), torch.tensor([3, 0, 1]).tolist(), True) == [3, 11, 0, 0, 1, 4]
    assert joint_cameras_row(cams, [3, 0, 1], valid=False) == ["NaN"] * 6


class _Stub:
    """forward_batch with the JointMask last: joint j of frame set t (the frames' value) counts cameras 0 .. (t+j) % C."""

    def __init__(self, C, J):
        self.C, self.J, self.calls = C, J, []

    def forward_batch(self, x, *calib, **kw):
        from jarvis_hybridnet_amd.joint_mask import JointMask
        self.calls.append(kw.get("joint_mask"))
        T = x.shape[0]
        k = x.reshape(T, -1)[:, 0].float()
        pts = k[:, None, None].expand(T, self.J, 3).contiguous()
        conf = torch.ones((T, self.J), device=x.device)
        valid = (k != 3).int()
        res = (pts, conf, valid)
        if kw.get("joint_mask") is not None:
            count = (k.long()[:, None] + torch.arange(self.J, device=x.device)[None]) % self.C + 1
            cams = (torch.arange(self.C, device=x.device)[None, None] < count[..., None]).to(torch.uint8)
            res += (JointMask(cams, count.int()),)
        return res


def test_driver_file_and_refusals(tmp_path):
    from jarvis_hybridnet_amd import _native as N
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    C, J, n = 3, 2, 5
    cfg = NS(KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C), KEYPOINT_NAMES=["nose", "tail"])
    frames = [np.full((C, 4, 4, 3), k, np.uint8) for k in range(n)]
    plain, masked = tmp_path / "plain", tmp_path / "masked"
    stub = _Stub(C, J)
    assert predict3D_frames(stub, frames, None, None, None, cfg, str(plain), time_batch=2) == n
    assert stub.calls == [None] * 3 and not (plain / "joint_cameras.csv").exists()
    stub = _Stub(C, J)
    assert predict3D_frames(stub, frames, None, None, None, cfg, str(masked), time_batch=2,
                            joint_mask=dict(max_error_px=5.0)) == n
    assert len(stub.calls) == 3 and all(isinstance(p, N.Joints3dParamsStruct) and p.max_error_px == 5.0
                                        for p in stub.calls)
    assert (plain / "data3D.csv").read_bytes() == (masked / "data3D.csv").read_bytes()     # (the stub's points)
    rows = list(csv.reader((masked / "joint_cameras.csv").read_text().splitlines()))
    assert rows[0] == ["nose", "nose", "tail", "tail"] and rows[1] == ["count", "cameras"] * J and len(rows) == 2 + n
    for k in range(n):
        want = ["NaN"] * (2 * J) if k == 3 else [str(v) for j in range(J)
                                                 for v in ((k + j) % C + 1, 2 ** ((k + j) % C + 1) - 1)]
        assert rows[2 + k] == want, k
    # 'consensus' / True are the defaults; no header without KEYPOINT_NAMES
    cfg.KEYPOINT_NAMES = []
    stub = _Stub(C, J)
    predict3D_frames(stub, frames[:2], None, None, None, cfg, str(tmp_path / "c"), joint_mask="consensus")
    assert stub.calls[0].max_error_px == 8.0 and len((tmp_path / "c" / "joint_cameras.csv").read_text().splitlines()) == 2
    d = str(tmp_path / "bad")
    for bad in (torch.ones((1, J, C), dtype=torch.uint8), np.ones((J, C), np.uint8), [[1] * C] * J, "members", False):
        with pytest.raises(ValueError):
            predict3D_frames(_Stub(C, J), frames[:2], None, None, None, cfg, d, joint_mask=bad)
    with pytest.raises(ValueError, match="joint_mask"):
        predict3D_frames(_Stub(C, J), frames[:2], None, None, None, cfg, d, joint_mask="consensus", max_subjects=2)


def test_sharded_path_refuses_joint_masks():
    from jarvis_hybridnet_amd.distributed import ShardedPredictor
    with pytest.raises(ValueError, match="joint_mask"):
        ShardedPredictor.submit(object(), None, joint_mask="consensus")
    shell = NS()                                     # (step hands its arguments to submit)
    shell.submit = lambda *a: ShardedPredictor.submit(shell, *a)
    with pytest.raises(ValueError, match="joint_mask"):
        ShardedPredictor.step(shell, None, joint_mask=torch.ones((1, 2, 4)))
