"""GPU: subject identity across frame sets -- jh_op_track_subjects against the numpy reference of its definition
(tests/tracks_ref.py, written from the header text), the state carried from call to call, one tracker updated from two
streams, forward_subjects(..., tracker=) against the call without a tracker, and the driver's per-subject files.

Bounds: everything is exact.  ids, slots, missed, dropped, views, members and the whole jh_track_state are compared as
integers; centers_out, error_out and the state's floats bit for bit (NaN as NaN).  That is a fair demand because the
reference asserts, before anything is compared, that no decision of a scene lies within 1e-3 mm of going the other way
in float64 (tests/tracks_ref.py: coordinates within +-1000 mm round at 6e-5 mm in fp32), and because the definition
fixes one fp32 rounding per operation.  The predictor tests run on cfg2 (tests/test_hip_centers.py: 4 cameras 640 x 512).
Every test calls a symbol this feature adds."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import test_hip_centers as HC
from tests import tracks_ref as R
from tests.gpu_util import cuda

pytestmark = pytest.mark.gpu

INF = float("inf")
same = HC.same
NAMES = ("centers", "views", "members", "error", "ids", "slots", "missed", "dropped")


def struct(p):
    from jarvis_hybridnet_amd import _native as N
    return N.TrackParamsStruct(p["max_subjects"], p["max_missed"], p["predict"], p["coast"], float(p["max_jump_mm"]))


def fresh_state():
    from jarvis_hybridnet_amd import _native as N
    state = torch.empty((272,), dtype=torch.uint8, device="cuda")
    state.fill_(0xA5)                                          # (reset writes every word)
    N.check(N.lib().jh_op_track_reset(N.ptr(state), N.stream()))
    return state


def host_state(state):
    from jarvis_hybridnet_amd import _native as N
    s = N.TrackStateStruct.from_buffer_copy(state.cpu().numpy().tobytes())
    return dict(pos=np.array(s.pos, np.float32).reshape(8, 3), vel=np.array(s.vel, np.float32).reshape(8, 3),
                missed=np.array(s.missed, np.int32), id=np.array(s.id, np.int32), next_id=int(s.next_id),
                reserved=list(s.reserved))


def op(inputs, p, state):
    """jh_op_track_subjects on numpy inputs (centers, views, members, error; the last three None together) -> dict of
    host arrays; `state` (device) is updated."""
    from jarvis_hybridnet_amd import _native as N
    centers, views, members, error = inputs
    T, K = centers.shape[:2]
    dev = [None if a is None else cuda(torch.from_numpy(np.ascontiguousarray(a))) for a in inputs]
    cams = 1 if members is None else members.shape[2]
    out = [torch.empty_like(dev[0])] + [None if t is None else torch.empty_like(t) for t in dev[1:]]
    trk = [torch.empty((T, K), device="cuda", dtype=torch.int32) for _ in range(3)]
    trk.append(torch.empty((T,), device="cuda", dtype=torch.int32))
    N.check(N.lib().jh_op_track_subjects(*(N.ptr(t) for t in dev), T, cams, ctypes.byref(struct(p)), N.ptr(state),
                                         *(N.ptr(t) for t in out), *(N.ptr(t) for t in trk), N.stream()))
    torch.cuda.synchronize()
    return {n: (None if t is None else t.cpu().numpy()) for n, t in zip(NAMES, out + trk)}


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_equal(got, want, what):
    for n in NAMES:
        if want[n] is None:
            assert got[n] is None, (what, n)
            continue
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
        if n in ("centers", "error"):
            # bit-equal, NaN compared as NaN (the payload of an empty row's NaN is not part of the definition)
            nan = np.isnan(want[n])
            assert np.array_equal(np.isnan(got[n]), nan), (what, n)
            assert np.array_equal(bits(np.where(nan, 0, got[n]).astype(np.float32)),
                                  bits(np.where(nan, 0, want[n]).astype(np.float32))), (what, n)
        else:
            assert np.array_equal(got[n], want[n]), (what, n, got[n].tolist(), want[n].tolist())


def check(inputs, p, what, margin=None):
    """The operator on a fresh state against the reference: outputs and state."""
    state = fresh_state()
    got = op(inputs, p, state)
    ref_state = R.new_state()
    want = R.track_ref(*inputs, p, ref_state, margin=margin)
    assert_equal(got, want, what)
    hs = host_state(state)
    assert R.same_state(hs, ref_state, p["max_subjects"]), (what, hs, ref_state)
    # slots >= K are never touched: they are as reset left them
    K = p["max_subjects"]
    assert (hs["missed"][K:] == -1).all() and (hs["id"][K:] == -1).all() and not hs["pos"][K:].any()
    assert hs["reserved"] == [0, 0, 0]
    return got


@functools.lru_cache(maxsize=None)
def scene(name, cams):
    return R.scene_by_name(name, cams)


cut = R.cut


# ---- 1: the operator against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in R.SCENES])          # K = 1, 2, 3, 4, 8
def test_scenes_equal_the_reference(name):
    """t = 1, 2, 7, 32; cams = 2, 12; predict and coast on and off; the NULL form; the open gate (R.scene_cases)."""
    for what, inputs, p in R.scene_cases(name):
        got = check(inputs, p, what, margin=R.MARGIN)
        # every detection found a slot (the scenes have no more animals than slots)
        assert (got["slots"] >= 0).sum() == np.isfinite(inputs[0]).all(-1).sum() and got["dropped"].sum() == 0


def test_hand_made_cases_equal_the_reference():
    for name, (centers, p) in R.hand_cases().items():
        got = check((centers, None, None, None), p, name)
        T, K = centers.shape[:2]
        g = np.random.RandomState(5)
        rows = (g.randint(0, 5, (T, K)).astype(np.int32), g.randint(-1, 8, (T, K, 2)).astype(np.int32),
                g.rand(T, K).astype(np.float32))
        again = check((centers,) + rows, p, name + " with rows")
        assert np.array_equal(again["slots"], got["slots"]) and np.array_equal(again["ids"], got["ids"])
        if name == "dropped":
            assert got["dropped"].tolist() == [0, 1]


def test_empty_frames_first_frame_and_open_gate():
    # all rows NaN: nothing is born, nothing dropped
    got = check((np.full((2, 3, 3), np.nan, np.float32), None, None, None), R.params(3, R.GATE), "all NaN")
    assert (got["ids"] == -1).all() and got["dropped"].tolist() == [0, 0]
    # K detections on a first frame set: K births in row order
    g = np.random.RandomState(11)
    first = (g.uniform(-200, 200, (1, 8, 3)).astype(np.float32), g.randint(2, 5, (1, 8)).astype(np.int32),
             g.randint(-1, 8, (1, 8, 12)).astype(np.int32), g.rand(1, 8).astype(np.float32))
    got = check(first, R.params(8, R.GATE), "first frame")
    assert got["ids"].tolist() == [list(range(8))] and got["slots"].tolist() == [list(range(8))]
    # an infinite value is not present; a huge finite one is
    odd = np.zeros((1, 2, 3), np.float32)
    odd[0, 0, 1], odd[0, 1, 2] = np.inf, 3e38
    assert check((odd, None, None, None), R.params(2, R.GATE), "inf")["slots"].tolist() == [[1, -1]]
    cr = R.crossing()
    for predict in (0, 1):
        check((cr["centers"], None, None, None), R.params(2, R.GATE, 0, predict), ("crossing", predict), margin=R.MARGIN)


# ---- 2: the state carries over ---------------------------------------------------------------------------------------
def test_state_carries_from_call_to_call():
    sc, K, mm = scene("three_in_eight_gap3", 12)
    p = R.params(K, R.GATE, mm, 1, 1)
    runs = {}
    for step in (32, 8, 1):
        state = fresh_state()
        parts = [op(tuple(a[t:t + step] for a in cut(sc, 32)), p, state) for t in range(0, 32, step)]
        runs[step] = ({n: np.concatenate([q[n] for q in parts]) for n in NAMES}, state.cpu().numpy().tobytes())
    for step in (8, 1):
        assert runs[step][1] == runs[32][1], step                      # (the 272 bytes of the state)
        for n in NAMES:
            assert np.array_equal(bits(runs[step][0][n]), bits(runs[32][0][n])), (step, n)
    ref_state = R.new_state()
    assert_equal(runs[1][0], R.track_ref(*cut(sc, 32), p, ref_state, margin=R.MARGIN), "32 calls of 1")


def test_operator_inside_a_stream_capture():
    """The call allocates nothing and does not synchronise: captured once, its graph replayed twice is two calls -- the
    state carries from replay to replay."""
    from jarvis_hybridnet_amd import _native as N
    sc, K, mm = scene("three_in_four", 2)
    p = R.params(K, R.GATE, mm, 1, 1)
    first, second = (tuple(a[t:t + 16] for a in cut(sc, 32)) for t in (0, 16))
    eager_state = fresh_state()
    want = [op(first, p, eager_state), op(second, p, eager_state)]
    state = fresh_state()
    dev = [cuda(torch.from_numpy(np.ascontiguousarray(a))) for a in first]
    out = [torch.empty_like(t) for t in dev]
    trk = [torch.empty((16, K), device="cuda", dtype=torch.int32) for _ in range(3)]
    trk.append(torch.empty((16,), device="cuda", dtype=torch.int32))
    ps = struct(p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.check(N.lib().jh_op_track_subjects(*(N.ptr(t) for t in dev), 16, 2, ctypes.byref(ps), N.ptr(state),
                                             *(N.ptr(t) for t in out), *(N.ptr(t) for t in trk), N.stream()))
    for inputs, w in zip((first, second), want):
        for t, a in zip(dev, inputs):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        graph.replay()
        torch.cuda.synchronize()
        assert_equal({n: t.cpu().numpy() for n, t in zip(NAMES, out + trk)}, w, "replay")
    assert state.cpu().numpy().tobytes() == eager_state.cpu().numpy().tobytes()


# ---- 3: one tracker, two streams --------------------------------------------------------------------------------------
def tracker_run(sc, K, mm, streams):
    from jarvis_hybridnet_amd import Subjects, SubjectTracker
    tr = SubjectTracker(K, R.GATE, max_missed=mm, predict=True, coast=True)
    halves = [Subjects(*(cuda(torch.from_numpy(a[t:t + 16])) for a in cut(sc, 32))) for t in (0, 16)]
    torch.cuda.synchronize()
    outs = []
    for half, s in zip(halves, streams):
        if s is None:
            outs.append(tr.update(half))
            continue
        with torch.cuda.stream(s):
            outs.append(tr.update(half))
    torch.cuda.synchronize()
    return outs, tr.state()


def test_updates_on_two_streams_are_ordered():
    from jarvis_hybridnet_amd import Subjects, Tracks
    sc, K, mm = scene("eight", 12)
    one, state_one = tracker_run(sc, K, mm, (None, None))
    two, state_two = tracker_run(sc, K, mm, (torch.cuda.Stream(), torch.cuda.Stream()))
    for (sa, ta), (sb, tb) in zip(one, two):
        assert isinstance(sa, Subjects) and isinstance(ta, Tracks)
        assert all(same(a, b) for a, b in zip(tuple(sa) + tuple(ta), tuple(sb) + tuple(tb)))
    assert R.same_state(state_one, state_two)
    # ... and they are the reference's
    ref_state = R.new_state()
    want = R.track_ref(*cut(sc, 32), R.params(K, R.GATE, mm, 1, 1), ref_state, margin=R.MARGIN)
    got = {n: np.concatenate([(tuple(h[0]) + tuple(h[1]))[i].cpu().numpy() for h in two]) for i, n in enumerate(NAMES)}
    assert_equal(got, want, "tracker")
    assert R.same_state(state_two, ref_state)


def test_tracker_misuse():
    from jarvis_hybridnet_amd import SubjectTracker
    c, inp, pred, calib, frames = HC.setup()
    tr = SubjectTracker(2, 30.0)
    with pytest.raises(ValueError):
        tr.update((torch.zeros(4, 3, 3, device="cuda"), None, None, None))          # K = 3 rows for 2 slots
    with pytest.raises(ValueError):
        tr.update((torch.zeros(4, 2, 3, device="cuda"), torch.zeros(4, 2, device="cuda", dtype=torch.int32), None, None))
    with pytest.raises(ValueError):
        tr.update((torch.zeros(4, 2, 3), None, None, None))                          # a host tensor
    with pytest.raises(ValueError, match="slots"):
        pred.detect_subjects(cuda(frames[:4]), *calib, 3, tracker=tr)
    assert tr.state()["next_id"] == 0 and (tr.state()["missed"] == -1).all()           # (nothing was enqueued)
    tr.update((torch.zeros(1, 2, 3, device="cuda"), None, None, None))
    assert tr.state()["next_id"] == 2
    tr.reset()
    assert tr.state()["next_id"] == 0


# ---- 4: the predictor --------------------------------------------------------------------------------------------------
KW = dict(max_peaks=2, min_peak=-INF, max_error_px=INF)


@functools.lru_cache(maxsize=None)
def untracked(T):
    c, inp, pred, calib, frames = HC.setup()
    out = pred.forward_subjects(cuda(frames[:T]), *calib, 3, **KW)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("gate", [INF, 1.0])
def test_forward_subjects_rows_follow_their_slots(gate):
    """gate 1 mm, max_missed 0: the two alternating frame sets' subjects do not match each other, so every frame set ends
    the tracks of the one before (step 6) and bears its own into the slots just freed (step 7)."""
    from jarvis_hybridnet_amd import Subjects, SubjectTracker, Tracks
    c, inp, pred, calib, frames = HC.setup()
    T, K = 8, 3
    x = cuda(frames[:T])
    pts, conf, valid, subj = untracked(T)
    tr = SubjectTracker(K, gate, max_missed=1 if gate == INF else 0, coast=False)
    out = pred.forward_subjects(x, *calib, K, tracker=tr, **KW)
    torch.cuda.synchronize()
    assert len(out) == 5 and isinstance(out[3], Subjects) and isinstance(out[4], Tracks)
    tpts, tconf, tvalid, tsubj, tracks = out
    # detect_subjects alone gives the same Subjects and Tracks from the same start
    tr.reset()
    d_subj, d_peaks, d_tracks = pred.detect_subjects(x, *calib, K, tracker=tr, return_peaks=True, **KW)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(tuple(d_subj) + tuple(d_tracks), tuple(tsubj) + tuple(tracks)))
    assert d_peaks.shape == (T, 4, 2, 3)
    slots = tracks.slots.cpu()
    held = 0
    for t in range(T):
        for k in range(K):
            i = int(slots[t, k])
            if i < 0:
                assert int(tvalid[t, k]) == 0 and torch.isnan(tsubj.centers[t, k]).all()
                assert int(tsubj.views[t, k]) == 0 and (tsubj.members[t, k] == -1).all() and torch.isnan(tsubj.error[t, k])
                continue
            held += 1
            assert all(same(a[t, k], b[t, i]) for a, b in zip(tsubj, subj)), (t, k, i)
            assert same(tvalid[t, k], valid[t, i])
            if int(valid[t, i]):
                assert same(tpts[t, k], pts[t, i]) and same(tconf[t, k], conf[t, i]), (t, k, i)
    # every non-empty subject is held by a slot (3 slots, at most 2 subjects per frame set)
    assert held == int((subj.views > 0).sum()) and held >= 12 and int(tracks.dropped.sum()) == 0
    ids = tracks.ids.cpu()
    if gate == INF:
        assert int(ids.max()) == int((subj.views[0] > 0).sum()) - 1            # (nobody is born after frame set 0)
    else:
        assert int(ids.max()) > 2


def test_forwards_around_a_tracked_call_keep_their_bits():
    from jarvis_hybridnet_amd import SubjectTracker
    c, inp, pred, calib, frames = HC.setup()
    for T in (1, 4):                                           # graph replay on (T = 1) and off
        pr = pred.native(c["H"], c["W"], time_batch=T)
        assert pr.graph_replay == (T == 1)
        x = cuda(frames[:T])
        before = tuple(t.clone() for t in pred.forward_batch(x, *calib))
        tr = SubjectTracker(2, INF)
        pred.forward_subjects(x, *calib, 2, tracker=tr, **KW)
        after = pred.forward_batch(x, *calib)
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(after, before)), T


# ---- 5: the driver -----------------------------------------------------------------------------------------------------
def test_driver_writes_one_file_per_subject(tmp_path):
    from jarvis_hybridnet_amd import SubjectTracker
    from jarvis_hybridnet_amd.prediction import predict3D as D
    c, inp, pred, calib, frames = HC.setup()
    cfg = HC.make_cfg(c)
    cfg.KEYPOINT_NAMES = ["joint%d" % j for j in range(c["J"])]
    n, K, J = 6, 2, c["J"]
    sets = [frames[t].numpy() for t in range(n)]
    track = dict(max_jump_mm=1.0, max_missed=0, coast=False)
    files = ["data3D_subject0.csv", "data3D_subject1.csv", "subjects3D.csv"]

    def run(name, **kw):
        out = str(tmp_path / name)
        assert D.predict3D_frames(pred, iter(sets), *calib, cfg, out, max_subjects=K, subject_params=KW, **kw) == n
        assert sorted(os.listdir(out)) == files
        return [open(os.path.join(out, f), "rb").read() for f in files]

    a = run("batched", track=track, time_batch=4, streams=2)
    b = run("single", track=track, time_batch=1, streams=1)
    assert a == b                                              # (the tracker saw the frame sets in order)
    # the rows are those of forward_subjects + SubjectTracker run by hand
    tr = SubjectTracker(K, **track)
    pts, conf, valid, subj, tracks = (pred.forward_subjects(cuda(frames[:n]), *calib, K, tracker=tr, **KW))
    torch.cuda.synchronize()
    got = [list(csv.reader(text.decode().splitlines())) for text in a]
    text = lambda row: [str(v) for v in row]                   # noqa: E731 -- what csv.writer writes
    for k in range(K):
        assert got[k][0] == [name for name in cfg.KEYPOINT_NAMES for _ in range(4)] and len(got[k]) == 2 + n
        for t in range(n):
            ok = int(valid[t, k]) != 0
            assert got[k][2 + t] == text(D.frame_row(pts[t, k].cpu() if ok else None, conf[t, k].cpu() if ok else None,
                                                     J)), (k, t)
    assert got[2][1] == list(D.SUBJECT_COLUMNS) * K + ["dropped"] and len(got[2]) == 2 + n
    for t in range(n):
        assert got[2][2 + t] == text(D.subjects_row(subj.centers[t], subj.views[t].cpu(), subj.error[t],
                                                    tracks.ids[t].cpu(), tracks.missed[t].cpu(),
                                                    tracks.dropped[t].cpu()))
    assert int(tracks.ids.max()) >= K                          # (1 mm gate: tracks ended and were born)
    assert any(row[0] != "NaN" for row in got[0][2:]) and int(valid.sum()) >= n
    # without a tracker: detection order, no identity
    plain = run("plain", time_batch=4, streams=2)
    rows = list(csv.reader(plain[2].decode().splitlines()))[2:]
    assert all(r[0] == "-1" and r[6] == "-1" and r[-1] == "0" for r in rows)
    # a SubjectTracker handed in serves as the dict does
    assert run("object", track=SubjectTracker(K, **track), time_batch=4, streams=2) == a
