"""CPU: subject identity across frame sets (jh_op_track_subjects) -- the numpy reference of the definition
(tests/tracks_ref.py) on hand-made cases whose answers are written out here, the scenes the GPU test uses (each run
through the reference's 1e-3 mm margin assertion, each keeping one id per animal), the parameter check at its bounds, the
exported names, the new symbols in the header, the ctypes table and the built library, and the driver's refusals.  Every
test uses a name this feature adds."""
import os
import re

import numpy as np
import pytest

from tests import tracks_ref as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("jh_track_params_check", "jh_op_track_reset", "jh_op_track_subjects")
INF = float("inf")


def run(name):
    centers, p = R.hand_cases()[name]
    state = R.new_state()
    return R.track_ref(centers, None, None, None, p, state), state


def xs(out):
    """The x coordinates of centers_out, None for NaN."""
    return [[None if np.isnan(v) else float(v) for v in row[:, 0]] for row in out["centers"]]


# ---- the reference on hand-made cases, checked by eye
def test_ref_swap_of_two_rows():
    out, state = run("swap")
    assert out["slots"].tolist() == [[0, 1], [1, 0], [0, 1]]          # frame set 1: slot 0 holds row 1
    assert out["ids"].tolist() == [[0, 1]] * 3 and out["missed"].tolist() == [[0, 0]] * 3
    assert xs(out) == [[0, 100], [5, 106], [10, 110]] and out["dropped"].tolist() == [0, 0, 0]
    assert state["next_id"] == 2 and state["vel"][:2, 0].tolist() == [5.0, 4.0]


def test_ref_nan_row():
    out, state = run("nan_row")
    assert out["slots"].tolist() == [[0, 1], [0, -1], [0, 1]]
    assert out["ids"].tolist() == [[0, 1]] * 3 and out["missed"].tolist() == [[0, 0], [0, 1], [0, 0]]
    assert xs(out) == [[0, 100], [5, None], [10, 110]]
    assert state["vel"][1, 0] == 5.0                                   # (110 - 100) / 2 elapsed frame sets


def test_ref_gap_of_max_missed_keeps_the_id_one_more_ends_it():
    out, state = run("gap_keeps")
    assert out["ids"][:, 0].tolist() == [0] * 5 and out["missed"][:, 0].tolist() == [0, 0, 1, 2, 0]
    assert out["slots"][:, 0].tolist() == [0, 0, -1, -1, 0] and state["next_id"] == 1
    assert state["vel"][0, 0] == 10.0 and state["pos"][0, 0] == 40.0   # (40 - 10) / 3
    out, state = run("gap_ends")
    assert out["ids"][:, 0].tolist() == [0, 0, 0, 0, -1, 1] and out["missed"][:, 0].tolist() == [0, 0, 1, 2, -1, 0]
    assert state["next_id"] == 2 and out["dropped"].sum() == 0


def test_ref_dropped_and_freed_and_reused():
    out, state = run("dropped")
    assert out["dropped"].tolist() == [0, 1] and out["ids"][:, 0].tolist() == [0, 0]
    assert out["slots"][:, 0].tolist() == [0, -1] and out["missed"][:, 0].tolist() == [0, 1] and state["next_id"] == 1
    out, state = run("freed_and_reused")
    assert out["dropped"].tolist() == [0, 0] and out["ids"][:, 0].tolist() == [0, 1]
    assert out["slots"][:, 0].tolist() == [0, 0] and out["missed"][:, 0].tolist() == [0, 0] and state["next_id"] == 2
    assert state["pos"][0, 0] == 100.0 and state["vel"][0, 0] == 0.0


def test_ref_tie_goes_to_the_lowest_detection():
    out, _ = run("tie")
    assert out["slots"].tolist() == [[0, -1], [0, 1]] and out["ids"].tolist() == [[0, -1], [0, 1]]
    # ... and the margin assertion sees that tie
    centers, p = R.hand_cases()["tie"]
    with pytest.raises(AssertionError):
        R.track_ref(centers, None, None, None, p, R.new_state(), margin=R.MARGIN)


def test_ref_coast_and_predict():
    want = {(0, 0): None, (0, 1): None, (1, 0): 10.0, (1, 1): 20.0}     # (coast, predict) -> x of the empty frame set
    for (coast, predict), x in want.items():
        out, state = run("coast%d_predict%d" % (coast, predict))
        assert xs(out) == [[0.0], [10.0], [x]], (coast, predict)
        assert out["ids"][:, 0].tolist() == [0, 0, 0] and out["missed"][:, 0].tolist() == [0, 0, 1]
        assert state["vel"][0, 0] == (10.0 if predict else 0.0)


def test_ref_rows_move_with_their_detection():
    sc, K, mm = R.scene_by_name("three_in_four")
    out = R.track_ref(sc["centers"], sc["views"], sc["members"], sc["error"], R.params(K, R.GATE, mm), R.new_state())
    for t in range(32):
        for k in range(K):
            i = out["slots"][t, k]
            if i < 0:
                assert out["views"][t, k] == 0 and (out["members"][t, k] == -1).all() and np.isnan(out["error"][t, k])
                assert np.isnan(out["centers"][t, k]).all()
            else:
                assert out["views"][t, k] == sc["views"][t, i] and (out["members"][t, k] == sc["members"][t, i]).all()
                assert out["error"][t, k] == sc["error"][t, i] and (out["centers"][t, k] == sc["centers"][t, i]).all()


# ---- the scenes of the GPU test
@pytest.mark.parametrize("name", [s[0] for s in R.SCENES])
def test_scenes_clear_the_margin_and_keep_their_ids(name):
    sc, K, mm = R.scene_by_name(name)
    assert np.abs(np.nan_to_num(sc["centers"])).max() <= 205.0
    # every animal moves 8 - 12 mm per frame set (0.5 mm noise on either end: 4 sigma of the difference is 2.9 mm)
    for s in range(sc["truth"].max() + 1):
        where = {t: sc["centers"][t, list(sc["truth"][t]).index(s)] for t in range(32) if s in sc["truth"][t]}
        steps = [np.linalg.norm(where[t + 1] - where[t]) for t in where if t + 1 in where]
        assert len(steps) >= 20 and 8.0 - 2.9 <= min(steps) and max(steps) <= 12.0 + 2.9, (name, s, min(steps), max(steps))
    assert sc["truth"].max() + 1 <= K
    for predict in (1, 0):
        out = R.track_ref(sc["centers"], sc["views"], sc["members"], sc["error"],
                          R.params(K, R.GATE, mm, predict), R.new_state(), margin=R.MARGIN)
        ids = R.ids_of_subjects(out, sc["truth"])
        gap7 = name == "three_in_four_gap7"
        for s, got in ids.items():
            # one id per animal; the animal that is away for 7 frame sets against max_missed = 4 rightly gets a new one
            assert len(got) == (2 if gap7 and s == 2 else 1), (name, predict, ids)
        assert len(set.union(*ids.values())) == sum(len(v) for v in ids.values())    # (no id serves two animals)
        assert out["dropped"].sum() == 0
    # the rows really are permuted: the scene is no identity mapping
    if K > 1:
        assert len({tuple(r) for r in sc["truth"].tolist()}) > 1
    # every case the GPU test makes of this scene (prefixes, both camera counts, predict / coast off, the NULL form with
    # max_missed 0, the open gate) clears the margin too
    cases = R.scene_cases(name)
    assert len(cases) == 12
    for what, inputs, p in cases:
        R.track_ref(*inputs, p, R.new_state(), margin=R.MARGIN)


def test_crossing_swaps_without_prediction_only():
    cr = R.crossing()
    a = R.track_ref(cr["centers"], None, None, None, R.params(2, R.GATE, 0, 1), R.new_state(), margin=R.MARGIN)
    b = R.track_ref(cr["centers"], None, None, None, R.params(2, R.GATE, 0, 0), R.new_state(), margin=R.MARGIN)
    assert R.ids_of_subjects(a, cr["truth"]) == {0: {0}, 1: {1}}
    assert R.ids_of_subjects(b, cr["truth"]) == {0: {0, 1}, 1: {0, 1}}
    assert a["slots"].tolist() == [[0, 1]] * 12 and b["slots"].tolist() == [[0, 1]] * 6 + [[1, 0]] * 6


def test_ref_state_carries_over():
    sc, K, mm = R.scene_by_name("three_in_eight_gap3")
    p = R.params(K, R.GATE, mm, 1, 1)
    whole_state = R.new_state()
    whole = R.track_ref(sc["centers"], sc["views"], sc["members"], sc["error"], p, whole_state)
    state = R.new_state()
    parts = [R.track_ref(*(sc[n][t:t + 8] for n in ("centers", "views", "members", "error")), p, state)
             for t in range(0, 32, 8)]
    for n in ("centers", "views", "members", "error", "ids", "slots", "missed", "dropped"):
        assert np.array_equal(np.concatenate([q[n] for q in parts]), whole[n], equal_nan=True), n
    assert R.same_state(state, whole_state)


# ---- the Python surface that needs no device
def test_track_params_bounds():
    from jarvis_hybridnet_amd import _native as N
    p = N.track_params(2, 30.0)
    assert (p.max_subjects, p.max_missed, p.predict, p.coast, p.max_jump_mm) == (2, 0, 1, 0, 30.0)
    assert N.track_params(1, INF).max_jump_mm == INF and N.track_params(8, 1e-30, 2 ** 31 - 1, False, True).coast == 1
    bad = [dict(max_subjects=0, max_jump_mm=1.0), dict(max_subjects=9, max_jump_mm=1.0),
           dict(max_subjects=2, max_jump_mm=0.0), dict(max_subjects=2, max_jump_mm=-1.0),
           dict(max_subjects=2, max_jump_mm=float("nan")), dict(max_subjects=2, max_jump_mm="far"),
           dict(max_subjects=2, max_jump_mm=1.0, max_missed=-1), dict(max_subjects=2, max_jump_mm=1.0, max_missed=1.5),
           dict(max_subjects=2, max_jump_mm=1.0, predict=2), dict(max_subjects=2, max_jump_mm=1.0, coast="yes"),
           dict(max_subjects=True, max_jump_mm=1.0), dict(max_subjects=2 ** 40, max_jump_mm=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            N.track_params(**kw)
    with pytest.raises(TypeError):
        N.track_params(2)                                   # max_jump_mm has no default
    # the library's own check, on a struct made by hand
    lib = N.lib()
    for field, value in (("max_subjects", 9), ("max_missed", -1), ("predict", 2), ("coast", -1), ("max_jump_mm", 0.0)):
        q = N.TrackParamsStruct.from_buffer_copy(p)
        setattr(q, field, value)
        assert lib.jh_track_params_check(q) != 0 and b"jh_track_params" in lib.jh_last_error(), field
    assert lib.jh_track_params_check(p) == 0 and lib.jh_track_params_check(None) != 0


def test_tracks_exported_without_loading_the_library():
    import subprocess
    import sys
    code = ("import sys; import jarvis_hybridnet_amd as p; "
            "assert p.Tracks._fields == ('ids', 'slots', 'missed', 'dropped'); "
            "from jarvis_hybridnet_amd.tracks import SubjectTracker; assert SubjectTracker is p.SubjectTracker; "
            "from jarvis_hybridnet_amd import _native as N; assert N._lib is None")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    import inspect
    from jarvis_hybridnet_amd import SubjectTracker
    from jarvis_hybridnet_amd._predictor import MultiStreamPredictor
    from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D
    sig = inspect.signature(SubjectTracker.__init__).parameters
    assert list(sig)[1:] == ["max_subjects", "max_jump_mm", "max_missed", "predict", "coast", "device"]
    assert sig["max_jump_mm"].default is inspect.Parameter.empty
    assert (sig["max_missed"].default, sig["predict"].default, sig["coast"].default) == (0, True, False)
    assert all(callable(getattr(SubjectTracker, n)) for n in ("update", "reset", "state"))
    for fn in (JarvisPredictor3D.detect_subjects, JarvisPredictor3D.forward_subjects,
               MultiStreamPredictor.forward_subjects):
        assert inspect.signature(fn).parameters["tracker"].default is None


def test_symbols_in_header_ctypes_table_and_library():
    import ctypes
    from jarvis_hybridnet_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jarvis_hip.h")).read(), flags=re.S)
    assert re.search(r"typedef struct jh_track_params \{\s*int32_t max_subjects;\s*int32_t max_missed;\s*int32_t predict;"
                     r"\s*int32_t coast;\s*float\s+max_jump_mm;\s*\} jh_track_params;", text)
    assert re.search(r"typedef struct jh_track_state \{\s*float pos\[8\]\[3\], vel\[8\]\[3\];\s*int32_t missed\[8\];"
                     r"\s*int32_t id\[8\];\s*int32_t next_id, reserved\[3\];\s*\} jh_track_state;", text)
    assert ctypes.sizeof(N.TrackStateStruct) == 272 and N.TrackStateStruct.missed.offset == 192
    assert N.TrackStateStruct.next_id.offset == 256
    lib = N.lib()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/jarvis_hip.h does not declare %s" % name
        res, args = N._SIGS[name]
        assert res is N.c_int and len(args) == len([p for p in m.group(1).split(",") if p.strip()]), name
        assert name in N.symbols() and hasattr(lib, name)
    assert lib.jh_abi_version() == 4
    # validation needs no GPU: nothing is enqueued for null pointers or parameters out of range
    p = N.track_params(2, 30.0)
    assert lib.jh_op_track_reset(None, None) != 0 and b"null state" in lib.jh_last_error()
    assert lib.jh_op_track_subjects(None, None, None, None, 1, 4, p, *([None] * 10)) != 0
    assert b"null pointer" in lib.jh_last_error()
    p.max_subjects = 9
    assert lib.jh_op_track_subjects(None, None, None, None, 1, 4, p, *([None] * 10)) != 0
    assert b"max_subjects" in lib.jh_last_error()


def test_driver_refusals(tmp_path):
    from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames, subjects_row
    import torch
    c = torch.zeros(2, 4, 3)
    args = (None, [], c, c, c, None, str(tmp_path / "out"))
    for kw in (dict(centers=[0.0, 0.0, 0.0]), dict(output_2d=True), dict(output_spread=True),
               dict(output_triangulated=True)):
        with pytest.raises(ValueError, match="max_subjects does not combine"):
            predict3D_frames(*args, max_subjects=2, **kw)
    for kw in (dict(subject_params=dict(min_views=2)), dict(track=dict(max_jump_mm=30.0))):
        with pytest.raises(ValueError, match="need max_subjects"):
            predict3D_frames(*args, **kw)
    for kw in (dict(max_subjects=9), dict(max_subjects=2, subject_params=dict(min_views=1)),
               dict(max_subjects=2, subject_params=[1]), dict(max_subjects=2, track="yes"),
               dict(max_subjects=2, track=dict(max_missed=1)), dict(max_subjects=2, track=dict(max_jump_mm=-1.0))):
        with pytest.raises(ValueError):
            predict3D_frames(*args, **kw)
    assert not os.path.exists(str(tmp_path / "out"))            # (refused before anything is written)
    # a row of subjects3D.csv: ints as ints, 'NaN' for an empty slot
    row = subjects_row(torch.tensor([[1.5, 2.0, -3.0], [float("nan")] * 3]), torch.tensor([3, 0]),
                       torch.tensor([0.25, float("nan")]), torch.tensor([4, -1]), torch.tensor([0, -1]), 1)
    assert row == [4, 1.5, 2.0, -3.0, 3, 0.25, 0, -1, "NaN", "NaN", "NaN", 0, "NaN", -1, 1]
    assert subjects_row(torch.zeros(1, 3), torch.tensor([2]), torch.tensor([1.0])) == [-1, 0.0, 0.0, 0.0, 2, 1.0, -1, 0]
