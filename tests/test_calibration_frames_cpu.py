"""CPU: per-frame-set calibration -- the C ABI addition, the shape checker `_native.calibration` and the batched
validation-analysis loop `analyze_frames(time_batch=T)` with a stub predictor.  No kernel runs here;
tests/test_hip_calibration_frames.py holds the GPU side.
Except for the symbol test's last line, every test here fails on a build without the feature: the symbol, the checker
and the `time_batch` argument do not exist there."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N
from tests import cases
from tests.test_native_abi import ROOT, header_symbols

NEW = ("jh_predictor_set_calibration_frames",)
FILES = ("frame_names.csv", "points_HybridNet.csv", "points_GroundTruth.csv")


def test_new_symbols_in_header_and_ctypes_table():
    for name in NEW:
        assert name in header_symbols(), name
        assert name in N.symbols(), name
        assert hasattr(N.lib(), name), name
    # matching arity: the parameters of the header's prototype against the ctypes argument list, and against the
    # shared form's, whose signature it repeats
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jarvis_hip.h")).read(), flags=re.S)
    for name in NEW + ("jh_predictor_set_calibration",):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        res, args = N._SIGS[name]
        assert len([p for p in params.split(",") if p.strip()]) == len(args) == 5, name
        assert res is N.c_int
    assert N.lib().jh_abi_version() == 4


def _calib(C, T=None, dtype=torch.float32):
    lead = (C,) if T is None else (T, C)
    return (torch.zeros(lead + (4, 3), dtype=dtype), torch.zeros(lead + (3, 3), dtype=dtype),
            torch.zeros(lead + (1, 5), dtype=dtype))


def test_calibration_accepts_the_two_forms():
    T, C = 3, 4
    shared, frames = _calib(C), _calib(C, T)
    got = N.calibration(shared, T, C)
    assert got[0] == "shared" and all(a is b for a, b in zip(got[1:], shared))      # the tensors as given
    got = N.calibration(list(frames), T, C)
    assert got[0] == "frames" and all(a is b for a, b in zip(got[1:], frames))
    assert N.calibration(_calib(C, T, torch.float64), T, C)[0] == "frames"          # any floating dtype
    assert N.calibration(_calib(C, dtype=torch.float16), T, C)[0] == "shared"
    # T == C and T == 1 are not ambiguous: the number of dimensions tells the forms apart
    assert N.calibration(_calib(4), 4, 4)[0] == "shared"
    assert N.calibration(_calib(4, 4), 4, 4)[0] == "frames"
    assert N.calibration(_calib(C, 1), 1, C)[0] == "frames"
    assert N.calibration(_calib(C), 1, C)[0] == "shared"


def test_calibration_rejects():
    T, C = 3, 4
    shared, frames = _calib(C), _calib(C, T)
    with pytest.raises(ValueError, match="either all per camera"):                  # mixed forms
        N.calibration((frames[0], shared[1], shared[2]), T, C)
    with pytest.raises(ValueError, match="either all per camera"):
        N.calibration((shared[0], shared[1], frames[2]), T, C)
    with pytest.raises(ValueError, match="cameraMatrices must have shape"):         # a wrong T
        N.calibration(_calib(C, T + 1), T, C)
    with pytest.raises(ValueError, match="must have shape"):                        # a wrong C, either form
        N.calibration(_calib(C + 1, T), T, C)
    with pytest.raises(ValueError, match="must have shape"):
        N.calibration(_calib(C + 1), T, C)
    with pytest.raises(ValueError, match="distortionCoefficients must have shape"):   # (C,5) is not (C,1,5)
        N.calibration((shared[0], shared[1], torch.zeros(C, 5)), T, C)
    with pytest.raises(ValueError, match="floating-point"):                         # a non-floating dtype
        N.calibration((frames[0], frames[1].to(torch.int32), frames[2]), T, C)
    with pytest.raises(ValueError, match="three tensors"):                          # fewer than three tensors
        N.calibration(frames[:2], T, C)
    with pytest.raises(ValueError, match="three tensors"):
        N.calibration((frames[0], frames[1], None), T, C)
    with pytest.raises(ValueError, match="three tensors"):
        N.calibration(frames[0], T, C)


# ---- analyze_frames(time_batch=T) with a stub predictor

class StubPredictor:
    """Stands where JarvisPredictor3D stands in analyze_frames: records what it is given and returns scripted points
    and valid flags, keyed by the frame set's first pixel (so a row's result does not depend on where it runs)."""

    def __init__(self, samples, preds):
        self.by_pixel = {float(s[0][0, 0, 0, 0]): p for s, p in zip(samples, preds)}
        assert len(self.by_pixel) == len(samples)
        self.single, self.batches = [], []

    def _of(self, imgs):                         # imgs (C,3,H,W) float32: channel 0 of pixel (0,0) of camera 0
        return self.by_pixel[float(imgs[0, 0, 0, 0].double())]

    def __call__(self, imgs, cam, intr, dist):
        self.single.append((imgs, cam, intr, dist))
        return self._of(imgs), None

    def forward_batch(self, imgs, cam, intr, dist):
        self.batches.append((imgs, cam, intr, dist))
        pts = [self._of(x) for x in imgs]
        J = next(p for p in self.by_pixel.values() if p is not None).shape[1]
        points = torch.stack([torch.full((J, 3), float("nan")) if p is None else p[0] for p in pts])
        return points, None, torch.tensor([0 if p is None else 1 for p in pts], dtype=torch.int32)


def _tools(C):
    """Two calibration sets that differ in every tensor."""
    def tool(k):
        return NS(cameraMatrices=torch.full((C, 4, 3), float(k)), intrinsicMatrices=torch.full((C, 3, 3), 10.0 + k),
                  distortionCoefficients=torch.full((C, 1, 5), 20.0 + k))
    return {"calibA": tool(1), "calibB": tool(2)}


def _samples(n, reject_last=True):
    """n stub samples, dataset names A, B interleaved, frame set 2 `not detected` and, with reject_last, frame set n-1
    too (a rejected sample that is repeated as padding)."""
    J = 23
    samples, preds = cases.analysis_samples(J, n=max(n, 5))
    samples, preds = samples[:n], preds[:n]
    # float32-exact first pixels tell the frame sets apart after the loop's .float()
    for i, s in enumerate(samples):
        s[0][0, 0, 0, 0] = float(i + 1)
        s[-2] = "calibA" if i % 2 == 0 else "calibB"
    if reject_last:
        preds[-1] = None
    return J, samples, preds


def _run(tmp_path, name, n, reject_last=True, **kw):
    from torch.utils.data import DataLoader
    from jarvis_hybridnet_amd.analysis.analyze import analyze_frames
    J, samples, preds = _samples(n, reject_last)
    stub = StubPredictor(samples, preds)
    out = tmp_path / name
    seen, done = analyze_frames(stub, DataLoader(samples, batch_size=1, shuffle=False), _tools(2), str(out), J, **kw)
    assert seen == n and done == sum(p is not None for p in preds)
    return stub, samples, preds, [open(out / f, "rb").read() for f in FILES]


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("n", [5, 6, 8, 12])          # multiples of T and not: 6 = 2 * 3, 8 = 2 * 4, 12 all; 5 none
def test_analyze_frames_time_batch_files_equal_time_batch_1(tmp_path, monkeypatch, T, n):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)    # no GPU here
    ref_stub, _, _, ref = _run(tmp_path, "t1", n)
    assert len(ref_stub.single) == n and not ref_stub.batches                # time_batch 1: today's path
    stub, samples, preds, got = _run(tmp_path, "t%d" % T, n, time_batch=T)
    assert not stub.single and len(stub.batches) == -(-n // T)
    assert got == ref
    names = got[0].decode().split()
    assert names == [s[-1] for s, p in zip(samples, preds) if p is not None]   # sample order, rejected ones left out


def test_stub_sees_stacked_calibrations_in_sample_order(tmp_path, monkeypatch):
    """T = 4 over 6 samples: one full group and a tail of two, padded with two repeats of sample 5 -- which the
    predictor rejects, so a padded row that reached a file would show as a wrong count and a NaN row."""
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    T, n, C = 4, 6, 2
    stub, samples, preds, got = _run(tmp_path, "t4", n, time_batch=T)
    tools = _tools(C)
    order = [0, 1, 2, 3], [4, 5, 5, 5]
    assert len(stub.batches) == 2
    for (imgs, cam, intr, dist), idx in zip(stub.batches, order):
        assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (T, C, 3, 8, 10) and imgs.is_contiguous()
        assert tuple(cam.shape) == (T, C, 4, 3) and tuple(intr.shape) == (T, C, 3, 3) and tuple(dist.shape) == (T, C, 1, 5)
        assert N.calibration((cam, intr, dist), T, C)[0] == "frames"
        for row, i in enumerate(idx):
            tool = tools[samples[i][-2]]
            assert torch.equal(cam[row], tool.cameraMatrices) and torch.equal(intr[row], tool.intrinsicMatrices)
            assert torch.equal(dist[row], tool.distortionCoefficients)
            # converted per sample exactly as time_batch 1 converts it (analyze.py:66)
            want = torch.from_numpy(samples[i][0]).float().permute(0, 3, 1, 2)
            assert torch.equal(imgs[row], want)
    # rows: samples 0, 1, 3, 4 (2 and 5 rejected); nothing of the padding
    net = np.loadtxt(tmp_path / "t4" / "points_HybridNet.csv", delimiter=",")
    assert net.shape == (4, 23 * 3) and not np.isnan(net).any()
    for row, i in enumerate((0, 1, 3, 4)):
        assert np.array_equal(net[row].astype(np.float32), preds[i][0].numpy().reshape(-1))
    assert got[0].decode().split() == ["Frame_%03d.jpg" % i for i in (0, 1, 3, 4)]


def test_padded_valid_rows_are_dropped(tmp_path, monkeypatch):
    """A VALID last sample repeated as padding: its row appears once."""
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    stub, samples, preds, got = _run(tmp_path, "t4", 2, reject_last=False, time_batch=4)
    assert [int(x) for x in stub.batches[0][0][:, 0, 0, 0, 0]] == [1, 2, 2, 2]
    assert got[0].decode().split() == ["Frame_000.jpg", "Frame_001.jpg"]
    _, _, _, ref = _run(tmp_path, "t1", 2, reject_last=False)
    assert got == ref


def test_analyze_validation_data_passes_time_batch_through(tmp_path, monkeypatch):
    from jarvis_hybridnet_amd.analysis import analyze as A
    seen = {}

    def fake_frames(predictor, loader, tools, out, J, bar, n, **kw):
        seen.update(kw, batch_size=loader.batch_size, n=n)
        return n, n
    monkeypatch.setattr(A, "analyze_frames", fake_frames)
    monkeypatch.setattr(A, "JarvisPredictor3D", lambda *a, **k: None)
    cfg = NS(PARENT_DIR=str(tmp_path), KEYPOINTDETECT=NS(NUM_JOINTS=23))
    A.analyze_validation_data("p", cfg=cfg, dataset=[0, 1, 2], output_root=str(tmp_path / "o"), reproTools={},
                              time_batch=8)
    assert seen == dict(time_batch=8, batch_size=1, n=3)              # the loader still delivers single samples
    A.analyze_validation_data("p", cfg=cfg, dataset=[0], output_root=str(tmp_path / "o1"), reproTools={})
    assert seen["time_batch"] == 1
