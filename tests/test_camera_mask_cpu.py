"""CPU: the host side of per-frame camera masks -- argument validation, the masks' way through the ingest
pipelines with a fake `submit`, the driver's mask iterator, and the camera-sharded path's refusal.  No compute
call."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N
from jarvis_hybridnet_amd.prediction import _ingest


def test_mask_argument_validation():
    assert N.camera_mask(None, (4,)) is None
    for good in ([1, 0, 1, 1], [True, False, True, True], torch.tensor([2, 0, 5, 1]),
                 torch.tensor([True, False, True, True]), np.array([1, 0, 1, 1]), (1, 0, 1, 1)):
        m = N.camera_mask(good, (4,))
        assert m.dtype == torch.uint8 and m.tolist() == [1, 0, 1, 1] and m.is_contiguous()
    assert N.camera_mask(torch.ones(3, 4, dtype=torch.int64), (3, 4)).shape == (3, 4)
    for bad in ([1, 0, 1], torch.ones(4, 1), torch.ones(2, 4, dtype=torch.bool)):
        with pytest.raises(ValueError):
            N.camera_mask(bad, (4,))
    for bad in (torch.ones(4), [1.0, 0.0, 1.0, 1.0], np.ones(4, np.float32), torch.ones(4, dtype=torch.float16)):
        with pytest.raises(ValueError):
            N.camera_mask(bad, (4,))
    with pytest.raises(ValueError):
        N.camera_mask([[1, 0], [1]], (2, 2))


def test_predictor_arguments_are_checked_before_any_native_call():
    """forward / forward_uint8 / forward_yuv / forward_batch raise ValueError on a bad mask without touching the
    GPU (this process has none)."""
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    pred = JarvisPredictor3D.__new__(JarvisPredictor3D)
    torch.nn.Module.__init__(pred)
    pred.num_cameras = 4
    x = torch.zeros(4, 3, 8, 8)
    for call in (lambda m: pred.forward(x, None, None, None, camera_mask=m),
                 lambda m: pred.forward_uint8(x.to(torch.uint8), None, None, None, camera_mask=m),
                 lambda m: pred.forward_yuv(torch.zeros(4, 12, 8, dtype=torch.uint8), "i420", None, None, None,
                                            camera_mask=m),
                 lambda m: pred.forward_batch(x[None], None, None, None, camera_mask=[m] if m is not None else m)):
        for bad in ([1, 1, 1], torch.ones(4), [[1, 1, 1, 1]]):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        pred.forward_batch(torch.zeros(2, 4, 3, 8, 8), None, None, None, camera_mask=torch.ones(3, 4, dtype=torch.bool))


def test_batch_mask():
    assert _ingest.batch_mask([None, None], 4) is None
    m = _ingest.batch_mask([torch.tensor([1, 0, 1], dtype=torch.uint8), None], 4)
    assert m.dtype == torch.uint8 and m.tolist() == [[1, 0, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    m = _ingest.batch_mask([None, torch.tensor([0, 0, 1], dtype=torch.uint8)], 3)
    assert m.tolist() == [[1, 1, 1], [0, 0, 1], [0, 0, 1]]


@pytest.mark.parametrize("T", [1, 2, 3])
def test_frame_pipeline_carries_masks_with_their_batch(T):
    C, seen, rows = 3, [], []

    def submit(x, slot, mask=None):
        seen.append((x[:, :, 0, 0, 0].clone(), None if mask is None else mask.clone()))
        return (x[:, :, 0, 0, 0].float().sum(1, keepdim=True), x[:, 0, 0, 0, :1].float(),
                torch.ones(x.shape[0], dtype=torch.int32)), None

    pipe = _ingest.FramePipeline((C, 2, 2, 3), torch.uint8, T, 1, submit, lambda outs, real: rows.append(real), None)
    masks = [[1, 1, 0], None, [0, 1, 1], [1, 0, 1], None]
    for k, m in enumerate(masks):
        frames = np.full((C, 2, 2, 3), k, np.uint8)
        if m is None:
            pipe.push(frames)
        else:
            pipe.push(frames, torch.tensor(m, dtype=torch.uint8))
    assert pipe.finish() == len(masks) and sum(rows) == len(masks)
    pipe.close()
    k = 0
    for x, mask in seen:
        real = min(T, len(masks) - k)
        want = masks[k:k + real]
        assert x[:real, 0].tolist() == list(range(k, k + real))            # the mask rows sit beside THEIR frames
        if all(w is None for w in want):
            assert mask is None                                             # submit(x, slot) exactly as before
        else:
            want = [[1] * C if w is None else w for w in want]
            assert mask.shape == (T, C) and mask.tolist() == want + [want[-1]] * (T - real)
        k += real
    # a run without masks never passes the argument
    seen.clear()
    pipe = _ingest.FramePipeline((C, 2, 2, 3), torch.uint8, T, 1, lambda x, slot: submit(x, slot), lambda o, r: None, None)
    pipe.push(np.zeros((C, 2, 2, 3), np.uint8))
    assert pipe.finish() == 1 and seen[0][1] is None
    pipe.close()


class _Stub:
    """A predictor with the batch interface that records the masks it is given."""

    def __init__(self, J=2):
        self.J, self.masks = J, []

    def forward_batch(self, x, cam, intr, dist, camera_mask=None):
        self.masks.append(None if camera_mask is None else camera_mask.clone())
        T = x.shape[0]
        valid = torch.ones(T, dtype=torch.int32)
        if camera_mask is not None:
            valid = (camera_mask.sum(1) >= 2).to(torch.int32)
        return torch.zeros(T, self.J, 3), torch.zeros(T, self.J), valid


def _cfg(C=3, J=2):
    return NS(KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C), KEYPOINT_NAMES=[])


def _run(tmp_path, n, **kw):
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames
    stub = _Stub()
    frames = [np.zeros((3, 4, 4, 3), np.uint8) for _ in range(n)]
    got = predict3D_frames(stub, frames, None, None, None, _cfg(), str(tmp_path), **kw)
    return stub, got, (tmp_path / "data3D.csv").read_text().splitlines()


def test_driver_mask_for_the_whole_run(tmp_path):
    stub, n, rows = _run(tmp_path, 5, time_batch=2, camera_mask=[1, 0, 1])
    assert n == 5 and len(rows) == 5 and all("NaN" not in r for r in rows)
    assert all(m.tolist() == [[1, 0, 1]] * 2 for m in stub.masks) and len(stub.masks) == 3
    stub, n, rows = _run(tmp_path, 2, camera_mask=torch.tensor([True, True, True]))
    assert [m.tolist() for m in stub.masks] == [[[1, 1, 1]]] * 2


def test_driver_mask_iterator_in_step_with_frame_sets(tmp_path):
    per = [None, [1, 1, 1], [0, 0, 1], [0, 1, 0], None]
    stub, n, rows = _run(tmp_path, 5, camera_mask=iter(per))
    assert n == 5
    assert [("NaN" in r) for r in rows] == [False, False, True, True, False]
    assert stub.masks[0] is None and stub.masks[4] is None and stub.masks[2].tolist() == [[0, 0, 1]]
    # a list of per-frame-set masks is taken as such, not as one mask
    stub, n, rows = _run(tmp_path, 2, camera_mask=[[1, 1, 0], [0, 1, 1]])
    assert [m.tolist() for m in stub.masks] == [[[1, 1, 0]], [[0, 1, 1]]]


def test_driver_mask_errors(tmp_path):
    with pytest.raises(ValueError):
        _run(tmp_path, 3, camera_mask=iter([[1, 1, 1]] * 2))               # too few masks
    with pytest.raises(ValueError):
        _run(tmp_path, 3, camera_mask=iter([[1, 1, 1]] * 4))               # too many
    with pytest.raises(ValueError):
        _run(tmp_path, 3, camera_mask=[1, 1])                               # wrong length
    with pytest.raises(ValueError):
        _run(tmp_path, 3, camera_mask=torch.ones(3))                        # floating dtype
    with pytest.raises(ValueError):
        _run(tmp_path, 3, camera_mask=iter([[1.0, 1.0, 1.0]] * 3))


def test_sharded_path_refuses_masks():
    from jarvis_hybridnet_amd.distributed import ShardedPredictor
    sp = ShardedPredictor.__new__(ShardedPredictor)
    for call in (sp.submit, sp.step):
        with pytest.raises(ValueError, match="camera_mask"):
            call(torch.zeros(1, 1, 3, 4, 4), None, torch.ones(1, 4, dtype=torch.bool))


@pytest.mark.parametrize("T,streams", [(1, 1), (2, 1), (3, 2)])
def test_device_pipeline_carries_masks_with_their_batch(T, streams):
    """DevicePipeline (frame sets already resident: here plain tensors) with a fake submit."""
    C, seen, rows = 3, [], []

    def submit(x, slot, mask=None):
        seen.append((x[:, 0, 0].clone(), None if mask is None else mask.clone()))
        return (torch.zeros(T, 1, 3), torch.zeros(T, 1), torch.ones(T, dtype=torch.int32)), None

    pipe = _ingest.DevicePipeline(T, submit, lambda outs, real: rows.append(real), streams)
    masks = [None, [1, 1, 0], [0, 1, 1], None, None, [1, 0, 1], None]
    for k, m in enumerate(masks):
        frames = torch.full((C, 2), k, dtype=torch.uint8)
        if m is None:
            pipe.push(frames)
        else:
            pipe.push(frames, torch.tensor(m, dtype=torch.uint8))
    assert pipe.finish() == len(masks) and sum(rows) == len(masks)
    k = 0
    for x, mask in seen:
        real = min(T, len(masks) - k)
        want = masks[k:k + real]
        assert x[:real].tolist() == list(range(k, k + real))
        if all(w is None for w in want):
            assert mask is None
        else:
            want = [[1] * C if w is None else w for w in want]
            assert mask.tolist() == want + [want[-1]] * (T - real)
        k += real
    assert k == len(masks)


def test_single_mask_or_one_per_frame_set():
    from jarvis_hybridnet_amd.prediction.predict3D import _is_single_mask
    for one in ([1, 0, 1], (True, False), torch.tensor([1, 0]), np.array([1, 0]), [np.int64(1), 0], [1.0, 0.0], []):
        assert _is_single_mask(one)
    for many in ([[1, 0], [0, 1]], [None, [1, 0]], torch.ones(2, 3), np.ones((2, 3)), iter([[1, 0]]),
                 [torch.tensor([1, 0])], (m for m in [[1]])):
        assert not _is_single_mask(many)
