"""CPU: the per-camera 2D views of the 3D predictor (jh_predictor_views2d) -- the C ABI additions, the GPU-free
workspace query, the CSV helpers of predict3D_frames(output_2d=True) and the refusal of the camera-sharded path.
No kernel runs here; tests/test_hip_views2d.py holds the GPU side."""
import csv
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N
from tests.test_native_abi import header_symbols

NEW = ("jh_predictor_views2d", "jh_joint_argmax_all_workspace_bytes", "jh_op_joint_argmax_all")


def test_new_symbols_in_header_and_ctypes_table():
    for name in NEW:
        assert name in header_symbols(), name
        assert name in N.symbols(), name
        assert hasattr(N.lib(), name), name
    assert N.lib().jh_abi_version() == 4


def test_workspace_bytes_without_a_gpu():
    lib = N.lib()
    n = lib.jh_joint_argmax_all_workspace_bytes(4, 128, 128, 24)
    # at least one (max, index) pair per image and channel, far less than the heat maps themselves
    assert 4 * 24 * 8 <= n < 4 * 128 * 128 * 24 * 4 // 16
    assert lib.jh_joint_argmax_all_workspace_bytes(5, 8, 8, 8) > 0
    assert lib.jh_joint_argmax_all_workspace_bytes(2, 160, 160, 32) > 0
    # more images never need less
    assert lib.jh_joint_argmax_all_workspace_bytes(384, 128, 128, 24) >= n
    # shapes the scan does not take: channel counts that are no multiple of 8
    assert lib.jh_joint_argmax_all_workspace_bytes(4, 128, 128, 23) == 0
    assert lib.jh_joint_argmax_all_workspace_bytes(0, 128, 128, 24) == 0


def _csv_text(rows):
    import io
    buf = io.StringIO()
    w = csv.writer(buf, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)
    for r in rows:
        w.writerow(r)
    return buf.getvalue()


def test_views2d_row_is_the_predict2d_row():
    from jarvis_hybridnet_amd.prediction import predict2D, predict3D
    J = 5
    g = torch.Generator().manual_seed(3)
    pts = torch.randint(0, 640, (J, 2), generator=g, dtype=torch.int32)
    conf = torch.rand(J, generator=g)
    row = predict3D.views2d_row(pts, conf, torch.tensor(1, dtype=torch.uint8), J)
    want = predict2D.frame_row(pts.long(), conf, J)
    assert len(row) == 3 * J
    assert _csv_text([row]) == _csv_text([want])
    assert row[0] == int(pts[0, 0]) and row[1] == int(pts[0, 1]) and row[2] == conf.numpy()[0]
    # not used: whatever the tensors hold (-1 / 0 from the kernel), the row is NaN
    for used in (0, torch.tensor(0, dtype=torch.uint8)):
        assert predict3D.views2d_row(torch.full((J, 2), -1), torch.zeros(J), used, J) == ["NaN"] * (3 * J)


def test_reprojection_error_row_width_and_nan_placement():
    from jarvis_hybridnet_amd.prediction import predict3D
    C, J = 4, 3
    err = torch.arange(C * J, dtype=torch.float32).reshape(C, J) / 7
    err[2] = float("nan")
    row = predict3D.reprojection_error_row(err)
    assert len(row) == C * J
    for c in range(C):
        for j in range(J):
            v = row[c * J + j]                        # camera-major
            if c == 2:
                assert v == "NaN"
            else:
                assert isinstance(v, np.float32) and v == err[c, j].item()
    # the text round-trips to the same float32
    back = _csv_text([row]).strip().split(",")
    assert [b for b in back[2 * J:3 * J]] == ["NaN"] * J
    assert all(np.float32(b) == np.float32(err.reshape(-1)[i].item()) for i, b in enumerate(back)
               if not math.isnan(err.reshape(-1)[i].item()))
    # header rows: camera names once per joint, joint names once per camera
    cfg = NS(KEYPOINT_NAMES=["a", "b", "c"])
    rows = []
    predict3D.create_header_reprojection_error(NS(writerow=rows.append), cfg, ["L", "R"])
    assert rows == [["L", "L", "L", "R", "R", "R"], ["a", "b", "c", "a", "b", "c"]]


class _Stub:
    """A predictor with the batch interface: frame set k has 3D point k everywhere; camera c sees joint j at
    (10 c + j, k), the reprojection error is c + j / 8 + k."""

    def __init__(self, C, J):
        self.C, self.J, self.k, self.calls = C, J, 0, []

    def forward_batch(self, x, cam, intr, dist, camera_mask=None, return_2d=False):
        from jarvis_hybridnet_amd._predictor import Views2D
        self.calls.append(return_2d)
        T, C, J = x.shape[0], self.C, self.J
        k = torch.arange(self.k, self.k + T, dtype=torch.float32)
        self.k += T
        mask = torch.ones(T, C, dtype=torch.uint8) if camera_mask is None else camera_mask
        valid = (mask.sum(1) >= 2).to(torch.int32)
        used = mask * valid[:, None].to(torch.uint8)
        pts = k[:, None, None].expand(T, J, 3).contiguous()
        res = (pts, torch.full((T, J), 0.5), valid)
        if not return_2d:
            return res
        p2d = torch.zeros(T, C, J, 2, dtype=torch.int32)
        p2d[..., 0] = (10 * torch.arange(C)[None, :, None] + torch.arange(J)[None, None, :]).int()
        p2d[..., 1] = k[:, None, None].int()
        err = torch.arange(C)[None, :, None] + torch.arange(J)[None, None, :] / 8 + k[:, None, None]
        p2d[used == 0] = -1
        err[used == 0] = float("nan")
        return res + (Views2D(p2d, torch.full((T, C, J), 0.25) * used[..., None], torch.zeros(T, C, J, 2), err, used),)


def test_driver_writes_per_camera_csvs_with_a_stub_predictor(tmp_path):
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    C, J, n = 3, 2, 5
    cfg = NS(KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C), KEYPOINT_NAMES=["nose", "tail"])
    frames = [np.zeros((C, 4, 4, 3), np.uint8) for _ in range(n)]
    masks = [None, [1, 0, 1], None, [0, 0, 1], None]             # frame set 1: camera 1 dropped; 3: invalid
    plain, with2d = tmp_path / "plain", tmp_path / "with2d"
    stub = _Stub(C, J)
    assert predict3D_frames(stub, frames, None, None, None, cfg, str(plain), time_batch=2, camera_mask=iter(masks)) == n
    assert stub.calls == [False] * 3
    stub = _Stub(C, J)
    assert predict3D_frames(stub, frames, None, None, None, cfg, str(with2d), time_batch=2, camera_mask=iter(masks),
                            output_2d=True, camera_names=["L", "M", "R"]) == n
    assert stub.calls == [True] * 3
    assert (plain / "data3D.csv").read_bytes() == (with2d / "data3D.csv").read_bytes()
    assert sorted(p.name for p in plain.iterdir()) == ["data3D.csv"]
    assert sorted(p.name for p in with2d.iterdir()) == ["data2D_L.csv", "data2D_M.csv", "data2D_R.csv", "data3D.csv",
                                                        "reprojection_error.csv"]
    for c, name in enumerate("LMR"):
        rows = (with2d / ("data2D_%s.csv" % name)).read_text().splitlines()
        assert rows[:2] == ["nose,nose,nose,tail,tail,tail", "x,y,confidence,x,y,confidence"]
        assert len(rows) == 2 + n
        for k, r in enumerate(rows[2:]):
            gone = k == 3 or (k == 1 and c == 1)
            assert r == (",".join(["NaN"] * 3 * J) if gone else "%d,%d,0.25,%d,%d,0.25" % (10 * c, k, 10 * c + 1, k))
    rows = (with2d / "reprojection_error.csv").read_text().splitlines()
    assert rows[:2] == ["L,L,M,M,R,R", "nose,tail,nose,tail,nose,tail"] and len(rows) == 2 + n
    for k, r in enumerate(rows[2:]):
        cells = r.split(",")
        assert len(cells) == C * J
        for c in range(C):
            for j in range(J):
                gone = k == 3 or (k == 1 and c == 1)
                assert cells[c * J + j] == ("NaN" if gone else str(np.float32(c + j / 8 + k)))
    # default names, no header without KEYPOINT_NAMES; bad names are refused
    cfg.KEYPOINT_NAMES = []
    d = tmp_path / "default"
    predict3D_frames(_Stub(C, J), frames[:2], None, None, None, cfg, str(d), output_2d=True)
    assert len((d / "data2D_Camera_2.csv").read_text().splitlines()) == 2
    assert len((d / "reprojection_error.csv").read_text().splitlines()) == 2
    with pytest.raises(ValueError):
        predict3D_frames(_Stub(C, J), frames[:2], None, None, None, cfg, str(d), output_2d=True, camera_names=["a", "b"])


def test_sharded_path_refuses_2d_views():
    from jarvis_hybridnet_amd.distributed import ShardedPredictor

    class Stages:                                   # never reached: the refusal comes first
        def __getattr__(self, name):
            raise AssertionError("stage call %s before the argument check" % name)

    sh = ShardedPredictor(Stages(), num_cameras=4, num_joints=3, time_batch=2, heat_shape=(8, 8, 8), rank=0, world=1,
                          device="cpu")
    x = torch.zeros(2, 4, 3, 16, 16)
    with pytest.raises(ValueError, match="2D views"):
        sh.submit(x, return_2d=True)
    with pytest.raises(ValueError, match="2D views"):
        sh.step(x, return_2d=True)


def test_views2d_arguments_are_checked_before_any_native_call():
    """NativePredictor.views2d refuses tensors whose bytes would be misread (this process has no GPU: CPU tensors)."""
    from jarvis_hybridnet_amd._predictor import NativePredictor, Views2D
    assert Views2D._fields == ("points2D", "confidences2D", "reprojections", "errors", "used")
    pr = NativePredictor.__new__(NativePredictor)
    pr.T = pr.T3 = 2
    pr.C, pr.J, pr.Jp, pr.Hh, pr.handle = 4, 3, 8, 8, None
    with pytest.raises(ValueError):
        pr.views2d(torch.zeros(2, 3, 3))
