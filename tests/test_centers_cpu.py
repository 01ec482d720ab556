"""CPU: caller-supplied 3D centres (jh_predictor_set_centers) -- the symbol in the header and the ctypes table, the
argument check `_native.centers`, and the predict3D driver's `centers=` with a stub predictor (the pattern of
tests/test_io_formats.py: plain host buffers, no streams).  Every test uses the new symbol or argument."""
import csv
import math
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_symbol_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+jh_predictor_set_centers\s*\(([^)]*)\)\s*;", text)
    assert m, "include/jarvis_hip.h does not declare jh_predictor_set_centers"
    params = [p for p in m.group(1).split(",") if p.strip()]
    res, args = N._SIGS["jh_predictor_set_centers"]
    assert res is N.c_int and len(args) == len(params) == 3
    assert "jh_predictor_set_centers" in N.symbols()
    lib = N.lib()
    assert hasattr(lib, "jh_predictor_set_centers")
    assert lib.jh_abi_version() == N.ABI_VERSION == 4
    # validation needs no GPU: a null predictor is refused with a message
    assert lib.jh_predictor_set_centers(None, None, None) != 0
    assert b"null predictor" in lib.jh_last_error()


def test_centers_argument_accepts():
    assert N.centers(None, 1) is None and N.centers(None, 4) is None
    t = N.centers(torch.arange(12).reshape(4, 3), 4)                     # an integer tensor
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (4, 3) and not t.is_cuda
    assert t.tolist() == torch.arange(12.0).reshape(4, 3).tolist()
    a = N.centers(np.array([[1.5, -2.0, 3.25]], dtype=np.float64), 1)    # a float64 array
    assert a.dtype == torch.float32 and a.tolist() == [[1.5, -2.0, 3.25]]
    s = N.centers([[1, 2, 3], [4, 5, 6.5]], 2)                           # a sequence
    assert s.dtype == torch.float32 and s.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.5]]
    one = N.centers(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float16), 1)      # (3,) when T == 1
    assert one.dtype == torch.float32 and tuple(one.shape) == (1, 3)
    assert tuple(N.centers((7, 8, 9), 1).shape) == (1, 3)
    nc = N.centers(torch.arange(24.0).reshape(4, 6)[:, ::2], 4)          # a strided view is made contiguous
    assert nc.is_contiguous() and nc[1].tolist() == [6.0, 8.0, 10.0]
    # values are not looked at: a row that is not finite is an invalid row of the result, not an error
    nan = N.centers(torch.tensor([[float("nan"), 0.0, float("inf")]]), 1)
    assert math.isnan(nan[0, 0]) and math.isinf(nan[0, 2])
    f = torch.zeros(2, 3)
    assert N.centers(f, 2).data_ptr() == f.data_ptr()                    # (what is already right is not copied)


@pytest.mark.parametrize("value,T", [
    (torch.zeros(3), 2),                    # (3,) only for T == 1
    (torch.zeros(2, 3), 3),                 # wrong T
    (torch.zeros(3, 2), 3),                 # transposed
    (torch.zeros(1, 1, 3), 1),
    (torch.zeros(4), 1),
    (torch.zeros(0, 3), 1),
    (torch.zeros(2, 3, dtype=torch.bool), 2),
    (torch.zeros(2, 3, dtype=torch.complex64), 2),
    ([[1, 2, 3], [4, 5]], 2),               # ragged
    ("abc", 1),
    (5.0, 1),
])
def test_centers_argument_rejects(value, T):
    with pytest.raises(ValueError):
        N.centers(value, T)


def test_centers_error_names_both_shapes():
    with pytest.raises(ValueError) as e:
        N.centers(torch.zeros(2, 3), 5)
    assert "(5, 3)" in str(e.value) and "(2, 3)" in str(e.value)
    with pytest.raises(ValueError) as e:
        N.centers(torch.zeros(4), 1)
    assert "(1, 3) or (3,)" in str(e.value) and "(4,)" in str(e.value)


J, C = 3, 2
CFG = NS(KEYPOINT_NAMES=["a", "b", "c"], KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C))


class Stub:
    """points = frame id + joint index; a frame set is valid iff its centre is finite; every call is recorded."""

    def __init__(self):
        self.calls = []

    def forward_batch(self, x, *calib, **kw):
        self.calls.append(kw)
        T = x.shape[0]
        ids = x.reshape(T, -1)[:, 0].float()
        pts = ids[:, None, None] + torch.arange(J).float()[None, :, None] + torch.zeros(1, 1, 3)
        valid = torch.ones(T, dtype=torch.int32)
        if "centers" in kw:
            assert tuple(kw["centers"].shape) == (T, 3) and kw["centers"].dtype == torch.float32
            valid = torch.isfinite(kw["centers"]).all(1).int()
        return pts, torch.full((T, J), 0.5), valid


def frame_sets(n):
    return [np.full((C, 4, 6, 3), i, dtype=np.uint8) for i in range(n)]


def rows(path):
    return list(csv.reader(open(os.path.join(path, "data3D.csv"))))[2:]


def test_driver_centres_in_frame_order_with_padding(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    cs = [torch.tensor([10.0 * i, 1.0, -2.0]) for i in range(5)]
    given = [cs[0], cs[1].tolist(), None, cs[3].numpy(), torch.tensor([float("inf"), 0.0, 0.0])]
    pred = Stub()
    out = str(tmp_path / "iter")
    assert P.predict3D_frames(pred, iter(frame_sets(5)), None, None, None, CFG, out, time_batch=2,
                              centers=iter(given)) == 5
    got = [kw["centers"] for kw in pred.calls]
    assert len(got) == 3 and all("camera_mask" not in kw for kw in pred.calls)
    assert torch.equal(got[0], torch.stack([cs[0], cs[1]]))
    assert torch.isnan(got[1][0]).all() and torch.equal(got[1][1], cs[3])            # None: a NaN centre
    assert math.isinf(got[2][0, 0]) and torch.equal(got[2][1].isinf(), got[2][0].isinf())   # padding: the last centre
    r = rows(out)
    assert [x[0] for x in r] == ["0.0", "1.0", "NaN", "3.0", "NaN"] and r[2] == ["NaN"] * (4 * J)
    # one (3,) centre for the whole run, with a per-frame mask beside it
    pred = Stub()
    out = str(tmp_path / "single")
    masks = [[1, 1], None, [1, 0]]
    assert P.predict3D_frames(pred, iter(frame_sets(3)), None, None, None, CFG, out, time_batch=2,
                              centers=(1.0, 2.0, 3.0), camera_mask=iter(masks)) == 3
    assert [kw["centers"].tolist() for kw in pred.calls] == [[[1.0, 2.0, 3.0]] * 2] * 2
    assert [kw["camera_mask"].tolist() for kw in pred.calls] == [[[1, 1], [1, 1]], [[1, 0], [1, 0]]]
    assert [x[0] for x in rows(out)] == ["0.0", "1.0", "2.0"]
    # a run without centres calls the predictor as it always did
    pred = Stub()
    assert P.predict3D_frames(pred, iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "none"),
                              time_batch=2) == 3
    assert pred.calls == [{}, {}]
    release_ingest_buffers(pred)


def test_driver_centres_iterable_length_and_shape(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    c = torch.zeros(3)
    with pytest.raises(ValueError, match="fewer centres"):
        P.predict3D_frames(Stub(), iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "short"), time_batch=2,
                           centers=iter([c, c]))
    with pytest.raises(ValueError, match="more centres"):
        P.predict3D_frames(Stub(), iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "long"), time_batch=2,
                           centers=iter([c, c, c, c]))
    with pytest.raises(ValueError):                     # one centre for the run, wrong shape
        P.predict3D_frames(Stub(), iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "shape1"), time_batch=2,
                           centers=torch.zeros(4))
    with pytest.raises(ValueError):                     # a wrong shape inside the iterable
        P.predict3D_frames(Stub(), iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "shape2"), time_batch=2,
                           centers=iter([c, torch.zeros(2), c]))
