"""CPU: centre keyframes (jh_predictor_set_center_keyframes) -- the library's key rows against the numpy reference
(tests/center_keys_ref.py) for every small batch, the reference fill's properties, the three entries in the header and
the ctypes table, the Python argument checks and the predict3D driver's `center_every=` with a stub predictor.  Every
test uses a new symbol or argument."""
import csv
import ctypes
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from jarvis_hybridnet_amd import _native as N
from tests import center_keys_ref as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = {"jh_center_keyframe_rows": 5, "jh_predictor_set_center_keyframes": 5, "jh_predictor_get_center_keyframes": 4}


def lib_rows(T, every, n_rows):
    buf = (ctypes.c_int32 * T)()
    n = N.lib().jh_center_keyframe_rows(T, every, n_rows, buf, T)
    assert n >= 1, N.lib().jh_last_error()
    return list(buf[:n])


# ---- key rows ------------------------------------------------------------------------------------------------------
def test_key_rows_equal_the_reference_and_have_their_properties():
    for T in range(1, 34):
        for every in range(1, T + 2):
            for n_rows in range(1, T + 1):
                keys = lib_rows(T, every, n_rows)
                assert keys == R.key_rows(T, every, n_rows), (T, every, n_rows)
                assert keys[0] == 0 and keys[-1] == n_rows - 1
                assert all(0 < b - a <= every for a, b in zip(keys, keys[1:]))
                assert N.center_keyframe_rows(T, every, n_rows) == keys
                # the count alone, without a buffer
                assert N.lib().jh_center_keyframe_rows(T, every, n_rows, None, 0) == len(keys)
            assert len(lib_rows(T, every, T)) == R.key_slots(T, every), (T, every)
    assert lib_rows(8, 3, 8) == [0, 3, 6, 7] and lib_rows(8, 4, 6) == [0, 4, 5] and lib_rows(1, 5, 1) == [0]
    assert lib_rows(32, 4, 32) == [0, 4, 8, 12, 16, 20, 24, 28, 31]


@pytest.mark.parametrize("T,every,n_rows,cap,what", [
    (0, 1, 1, 8, "time_batch"), (-3, 1, 1, 8, "time_batch"), (8, 0, 8, 8, "every"), (8, -1, 8, 8, "every"),
    (8, 2, 0, 8, "n_rows"), (8, 2, 9, 8, "n_rows"), (8, 2, -1, 8, "n_rows"), (8, 2, 8, 4, "smaller"),
])
def test_key_rows_bad_arguments(T, every, n_rows, cap, what):
    buf = (ctypes.c_int32 * 8)(*([77] * 8))
    assert N.lib().jh_center_keyframe_rows(T, every, n_rows, buf, cap) == -1
    assert what.encode() in N.lib().jh_last_error()
    assert list(buf) == [77] * 8                                # nothing written
    if what != "smaller":
        with pytest.raises(ValueError, match=what):
            N.center_keyframe_rows(T, every, n_rows)


def test_a_large_every_does_not_overflow():
    assert lib_rows(8, 2 ** 31 - 1, 8) == [0, 7]
    assert lib_rows(33, 2 ** 30, 2) == [0, 1]


# ---- the reference fill --------------------------------------------------------------------------------------------
def rand_centres(keys, seed):
    rng = np.random.default_rng(seed)
    return {k: (rng.standard_normal(3) * 300).astype(np.float32) for k in keys}


def test_fill_key_rows_keep_their_bits_and_sources():
    keys = R.key_rows(8, 3)
    c = rand_centres(keys, 0)
    centers, source = R.fill(8, 3, 8, c, {k: True for k in keys})
    assert centers.dtype == np.float32 and source.dtype == np.int32
    for k in keys:
        assert centers[k].tobytes() == c[k].tobytes()
    assert source.tolist() == [0, 1, 1, 0, 1, 1, 0, 0]
    # the interpolation, spelled out once more in float32: row 1 between 0 and 3, row 5 between 3 and 6
    for t, ta, tb in ((1, 0, 3), (2, 0, 3), (4, 3, 6), (5, 3, 6)):
        w = np.float32(np.float32(t - ta) / np.float32(tb - ta))
        want = c[ta] + (c[tb] - c[ta]) * w
        assert centers[t].tobytes() == want.astype(np.float32).tobytes(), t
        assert np.all(np.minimum(c[ta], c[tb]) - 1e-3 <= centers[t]) and np.all(centers[t] <= np.maximum(c[ta], c[tb]) + 1e-3)


def test_fill_equal_neighbours_give_that_centre_exactly():
    keys = R.key_rows(9, 4)
    one = np.array([123.456, -7.875, 0.1], np.float32)
    centers, source = R.fill(9, 4, 9, {k: one for k in keys}, {k: True for k in keys})
    assert all(centers[t].tobytes() == one.tobytes() for t in range(9))
    assert source.tolist() == [0, 1, 1, 1, 0, 1, 1, 1, 0]


def test_fill_invalid_keys_hold_or_give_none_and_are_never_filled_in():
    keys = R.key_rows(8, 3)                                     # 0 3 6 7
    c = rand_centres(keys, 1)
    valid = {0: True, 3: False, 6: True, 7: True}
    centers, source = R.fill(8, 3, 8, c, valid)
    assert source.tolist() == [0, 2, 2, -1, 2, 2, 0, 0]
    assert centers[1].tobytes() == centers[2].tobytes() == c[0].tobytes()
    assert centers[4].tobytes() == centers[5].tobytes() == c[6].tobytes()
    assert np.isnan(centers[3]).all()                           # the invalid key is not given a neighbour's centre
    valid[6] = False
    centers, source = R.fill(8, 3, 8, c, valid)
    assert source.tolist() == [0, 2, 2, -1, -1, -1, -1, 0]
    assert np.isnan(centers[3:7]).all() and centers[7].tobytes() == c[7].tobytes()


def test_fill_padding_rows_hold_the_last_real_row():
    keys = R.key_rows(8, 4, 6)
    assert keys == [0, 4, 5]
    c = rand_centres(keys, 2)
    centers, source = R.fill(8, 4, 6, c, {k: True for k in keys})
    assert source.tolist() == [0, 1, 1, 1, 0, 0, 2, 2]
    assert centers[6].tobytes() == centers[7].tobytes() == c[5].tobytes()
    centers, source = R.fill(8, 4, 6, c, {0: True, 4: True, 5: False})
    assert source.tolist() == [0, 1, 1, 1, 0, -1, -1, -1] and np.isnan(centers[5:]).all()


# ---- host side -----------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "jarvis_hip.h")).read()
    assert re.search(r"#define\s+JH_ABI_VERSION\s+4\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = N.lib()
    assert lib.jh_abi_version() == N.ABI_VERSION == 4
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/jarvis_hip.h does not declare " + name
        res, args = N._SIGS[name]
        assert res is N.c_int and len(args) == n_args == len([p for p in m.group(1).split(",") if p.strip()]), name
        assert name in N.symbols() and hasattr(lib, name)
    # validation needs no GPU: a null predictor is refused with a message, by both
    assert lib.jh_predictor_set_center_keyframes(None, None, 2, 1, None) != 0
    assert b"null predictor" in lib.jh_last_error()
    assert lib.jh_predictor_get_center_keyframes(None, None, None, None) != 0
    assert b"null predictor" in lib.jh_last_error()


def test_center_every_argument():
    assert N.center_every(None, 8) is None
    assert N.center_every(3, 8) == (3, 8) and N.center_every((4, 6), 8) == (4, 6) and N.center_every([1, 1], 1) == (1, 1)
    assert N.center_every(100, 8) == (100, 8)                   # beyond the batch: first and last row
    for bad in (0, -1, True, 2.0, "3", (3,), (3, 0), (3, 9), (0, 4), (3, 4, 5), (3, None)):
        with pytest.raises(ValueError):
            N.center_every(bad, 8)


def test_predictor_refuses_centres_with_keyframes_before_anything_is_touched():
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    stub = NS(num_cameras=2)
    x = torch.zeros(4, 2, 3, 8, 8)
    for call, arg in ((JarvisPredictor3D.forward_batch, x), (JarvisPredictor3D.forward_images, [[x[0, 0]] * 2] * 4)):
        with pytest.raises(ValueError, match="center_every"):
            call(stub, arg, None, None, None, centers=torch.zeros(4, 3), center_every=2)


J, C = 3, 2
CFG = NS(KEYPOINT_NAMES=["a", "b", "c"], KEYPOINTDETECT=NS(NUM_JOINTS=J), HYBRIDNET=NS(NUM_CAMERAS=C))


class Stub:
    """points = frame id + joint index; every call is recorded; a keyframe call returns its CenterKeyframes last."""

    def __init__(self):
        self.calls = []

    def forward_batch(self, x, *calib, **kw):
        self.calls.append(kw)
        T = x.shape[0]
        ids = x.reshape(T, -1)[:, 0].float()
        pts = ids[:, None, None] + torch.arange(J).float()[None, :, None] + torch.zeros(1, 1, 3)
        res = (pts, torch.full((T, J), 0.5), torch.ones(T, dtype=torch.int32))
        return res + (("keyframes",),) if "center_every" in kw else res


def frame_sets(n):
    return [np.full((C, 4, 6, 3), i, dtype=np.uint8) for i in range(n)]


def test_driver_passes_the_real_rows_of_every_group(tmp_path):
    from jarvis_hybridnet_amd.prediction import predict3D as P
    from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers
    pred = Stub()
    out = str(tmp_path / "keys")
    assert P.predict3D_frames(pred, iter(frame_sets(7)), None, None, None, CFG, out, time_batch=3, center_every=2) == 7
    assert [kw["center_every"] for kw in pred.calls] == [(2, 3), (2, 3), (2, 1)]     # the short last group: 1 real row
    rows = list(csv.reader(open(os.path.join(out, "data3D.csv"))))[2:]
    assert [r[0] for r in rows] == ["%d.0" % i for i in range(7)]
    # device-resident-style pipeline aside, a run without the option calls the predictor as it always did
    pred = Stub()
    assert P.predict3D_frames(pred, iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "none"), time_batch=2) == 3
    assert pred.calls == [{}, {}]
    for bad in (dict(center_every=0), dict(center_every=(2, 2)), dict(center_every=2, centers=(0.0, 0.0, 0.0)),
                dict(center_every=2, max_subjects=2)):
        with pytest.raises(ValueError):
            P.predict3D_frames(Stub(), iter(frame_sets(3)), None, None, None, CFG, str(tmp_path / "bad"), time_batch=2,
                               **bad)
    release_ingest_buffers(pred)
