"""numpy reference of the subject tracker, written from the text of include/jarvis_hip.h (jh_op_track_subjects, steps
1 .. 8), not from the kernel: float32 operation by operation with np.float32 scalars (one IEEE rounding each, which is
what the definition asks of the kernel), every decision evaluated a second time in float64.

margin (millimetres): a condition on the INPUTS, not a tolerance on the kernel.  With it the reference asserts that no
decision is within `margin` of going the other way in float64: at every greedy step the best distance against the
second best of the pairs still open, and every distance of a live slot and a present detection against its gate.
Coordinates stay within +-1000 mm, whose fp32 ulp is 6e-5 mm, and a distance carries a few of those, hence 1e-3 mm: a
scene that meets it has one answer whatever the rounding of a correct implementation.  A scene that trips it is
replaced by another seed.  margin=None: the hand-made cases, whose ties are exact and decided by the lowest (k, i)."""
import numpy as np

F = np.float32
MARGIN = 1e-3
NAN = F(np.nan)


def params(max_subjects, max_jump_mm, max_missed=0, predict=1, coast=0):
    return dict(max_subjects=int(max_subjects), max_missed=int(max_missed), predict=int(predict), coast=int(coast),
                max_jump_mm=F(max_jump_mm))


def new_state():
    """jh_op_track_reset: all slots free, next_id 0, floats 0."""
    return dict(pos=np.zeros((8, 3), F), vel=np.zeros((8, 3), F), missed=np.full(8, -1, np.int32),
                id=np.full(8, -1, np.int32), next_id=0)


def copy_state(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def same_state(a, b, K=8):
    """Bit-equal on the slots below K (the others are never touched) and on next_id."""
    return (all(np.array_equal(np.asarray(a[n][:K]).view(np.int32), np.asarray(b[n][:K]).view(np.int32))
                for n in ("pos", "vel", "missed", "id")) and int(a["next_id"]) == int(b["next_id"]))


def _dist32(p, c):
    dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    return np.sqrt(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))


def track_ref(centers, views, members, error, p, state, margin=None):
    """centers (T,K,3) float32, views (T,K) / members (T,K,C) int32 / error (T,K) float32 or None together; p from
    params(); state from new_state(), updated in place -> dict of centers, views, members, error (None where not
    given), ids, slots, missed (T,K) and dropped (T)."""
    centers = np.asarray(centers, F)
    T, K = centers.shape[:2]
    assert K == p["max_subjects"] and centers.shape[2] == 3
    predict, coast, max_missed, jump = p["predict"], p["coast"], p["max_missed"], F(p["max_jump_mm"])
    pos, vel, missed, ident = state["pos"], state["vel"], state["missed"], state["id"]
    out = dict(centers=np.full((T, K, 3), np.nan, F), ids=np.full((T, K), -1, np.int32),
               slots=np.full((T, K), -1, np.int32), missed=np.full((T, K), -1, np.int32),
               dropped=np.zeros(T, np.int32), views=None, members=None, error=None)
    if views is not None:
        out.update(views=np.zeros((T, K), np.int32), members=np.full(np.shape(members), -1, np.int32),
                   error=np.full((T, K), np.nan, F))
    with np.errstate(all="ignore"):
        for t in range(T):
            c = centers[t]
            # 1, 2
            live = [k for k in range(K) if missed[k] >= 0]
            present = [i for i in range(K) if np.isfinite(c[i]).all()]
            pred, pred64 = {}, {}
            for k in live:
                m1 = F(missed[k] + 1)
                pred[k] = np.array([F(pos[k][a] + F(vel[k][a] * m1)) for a in range(3)], F) if predict else pos[k].copy()
                pred64[k] = (pos[k].astype(np.float64) + vel[k].astype(np.float64) * float(m1)) if predict \
                    else pos[k].astype(np.float64)
            # 3
            d32, d64 = {}, {}
            for k in live:
                m1 = F(missed[k] + 1)
                gate = F(jump * m1)
                for i in present:
                    d = _dist32(pred[k], c[i])
                    e = float(np.sqrt(((pred64[k] - c[i].astype(np.float64)) ** 2).sum()))
                    if margin is not None and np.isfinite(gate):
                        assert abs(e - float(jump) * float(m1)) >= margin, ("gate", t, k, i, e)
                    if d <= gate:                                   # (a NaN d compares false)
                        d32[(k, i)], d64[(k, i)] = d, e
            # 4
            det_of, slot_of = {}, {}
            while True:
                open_ = [ki for ki in d32 if ki[0] not in det_of and ki[1] not in slot_of]
                if not open_:
                    break
                best = min(open_, key=lambda ki: (d32[ki], ki[0], ki[1]))
                if margin is not None and len(open_) > 1:
                    second = min(d64[ki] for ki in open_ if ki != best)
                    assert second - d64[best] >= margin, ("choice", t, best, d64[best], second)
                det_of[best[0]], slot_of[best[1]] = best[1], best[0]
            # 5, 6
            for k in range(K):
                if k in det_of:
                    ci, m1 = c[det_of[k]], F(missed[k] + 1)
                    vel[k] = [F(F(ci[a] - pos[k][a]) / m1) for a in range(3)] if predict else [0, 0, 0]
                    pos[k] = ci
                    missed[k] = 0
                elif missed[k] >= 0:
                    missed[k] += 1
                    if missed[k] > max_missed:
                        missed[k], ident[k] = -1, -1
                        pos[k], vel[k] = 0, 0
            # 7
            for i in present:
                if i in slot_of:
                    continue
                free = [k for k in range(K) if missed[k] < 0]
                if not free:
                    out["dropped"][t] += 1
                    continue
                k = free[0]
                ident[k], state["next_id"] = state["next_id"], state["next_id"] + 1
                pos[k], vel[k], missed[k] = c[i], 0, 0
                det_of[k] = i
            # 8
            for k in range(K):
                i = det_of.get(k, -1)
                out["slots"][t, k], out["ids"][t, k], out["missed"][t, k] = i, ident[k], missed[k]
                if i >= 0:
                    out["centers"][t, k] = c[i]
                    if views is not None:
                        out["views"][t, k], out["members"][t, k], out["error"][t, k] = views[t][i], members[t][i], error[t][i]
                elif missed[k] >= 0 and coast:
                    fm = F(missed[k])
                    out["centers"][t, k] = [F(pos[k][a] + F(vel[k][a] * fm)) for a in range(3)] if predict else pos[k]
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------
def scene(S, K, T, seed, gaps=(), cams=4, speed=(8.0, 12.0), noise=0.5):
    """S subjects on straight lines through a +-200 mm arena at 8 - 12 mm per frame set with 0.5 mm noise, the detections
    of every frame set in K rows permuted by the seeded generator (rows without a subject: an empty Subjects row).
    gaps: (subject, first frame set, length) -- the subject is not detected there.
    -> dict centers (T,K,3), views (T,K), members (T,K,cams), error (T,K), truth (T,K) the subject in each row or -1."""
    g, g2 = np.random.RandomState(seed), np.random.RandomState(seed + 7919)   # (the centres do not depend on cams)
    direction = g.randn(S, 3)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    step = direction * g.uniform(speed[0], speed[1], (S, 1))
    half = np.abs(step) * (T - 1) / 2.0
    mid = g.uniform(-1.0, 1.0, (S, 3)) * (200.0 - half)            # (the whole segment stays inside the arena)
    centers = np.full((T, K, 3), np.nan, F)
    views, members = np.zeros((T, K), np.int32), np.full((T, K, cams), -1, np.int32)
    error, truth = np.full((T, K), np.nan, F), np.full((T, K), -1, np.int32)
    for t in range(T):
        rows = g.permutation(K)
        for s in range(S):
            where = mid[s] + step[s] * (t - (T - 1) / 2.0) + g.randn(3) * noise
            if any(s == gs and g0 <= t < g0 + n for gs, g0, n in gaps):
                continue
            r = rows[s]
            centers[t, r], truth[t, r] = where.astype(F), s
            views[t, r] = g2.randint(2, cams + 1)
            members[t, r] = g2.randint(-1, 8, cams)
            error[t, r] = F(g2.uniform(0.0, 5.0))
    return dict(centers=centers, views=views, members=members, error=error, truth=truth)


def crossing(T=12, seed=3, dy=8.7):
    """Two subjects head on along x at 10 mm per frame set, dy apart in y, rows fixed: matched against the last position
    each track is nearer to the OTHER subject's next detection when they pass (dy < 10 mm); matched against the
    prediction it is not."""
    g = np.random.RandomState(seed)
    centers = np.full((T, 2, 3), np.nan, F)
    for t in range(T):
        x = 10.0 * (t - (T - 1) / 2.0)
        centers[t, 0] = (np.array([x, 0.0, 0.0]) + g.randn(3) * 0.05).astype(F)
        centers[t, 1] = (np.array([-x, dy, 0.0]) + g.randn(3) * 0.05).astype(F)
    truth = np.tile(np.array([0, 1], np.int32), (T, 1))
    return dict(centers=centers, views=None, members=None, error=None, truth=truth)


def _frames(K, *frames):
    """(T,K,3) centres from per-frame-set lists of x coordinates (None: an empty row); y = z = 0."""
    out = np.full((len(frames), K, 3), np.nan, F)
    for t, xs in enumerate(frames):
        for i, x in enumerate(xs):
            if x is not None:
                out[t, i] = (x, 0.0, 0.0)
    return out


def hand_cases():
    """The hand-made cases: {name: (centers (T,K,3), params)}; what each must give is written out, number by number, in
    tests/test_tracks_cpu.py.  All on the x axis, gate 30 mm."""
    c = {}
    # two animals 100 mm apart whose rows swap in frame set 1 and swap back in 2
    c["swap"] = (_frames(2, [0, 100], [106, 5], [10, 110]), params(2, 30.0))
    # the second animal's row is NaN in frame set 1: its track waits (max_missed 1) and takes it back in 2
    c["nan_row"] = (_frames(2, [0, 100], [5, None], [10, 110]), params(2, 30.0, max_missed=1))
    # a gap of max_missed = 2 frame sets keeps the id (gate 30 * 3 = 90 >= 30) ...
    c["gap_keeps"] = (_frames(1, [0], [10], [None], [None], [40]), params(1, 30.0, max_missed=2))
    # ... a gap of max_missed + 1 ends the track in the third empty frame set: the animal comes back as id 1
    c["gap_ends"] = (_frames(1, [0], [10], [None], [None], [None], [50]), params(1, 30.0, max_missed=2))
    # a jump beyond the gate while the one slot is still alive (max_missed 1): the detection is dropped
    c["dropped"] = (_frames(1, [0], [100]), params(1, 30.0, max_missed=1))
    # the same jump with max_missed 0: the slot is freed in step 6 and taken again in step 7 of the same frame set
    c["freed_and_reused"] = (_frames(1, [0], [100]), params(1, 30.0, max_missed=0))
    # an exact tie: both detections 5 mm from the one track -- the lowest i wins, the other is born into slot 1
    c["tie"] = (_frames(2, [0, None], [5, -5]), params(2, 30.0))
    # coast and predict, all four: a track at x = 0, 10 and then an empty frame set
    for predict in (0, 1):
        for coast in (0, 1):
            c["coast%d_predict%d" % (coast, predict)] = (_frames(1, [0], [10], [None]),
                                                         params(1, 30.0, max_missed=2, predict=predict, coast=coast))
    return c


# (name, S, K, T, seed, gaps, max_missed): the scenes of the CPU and the GPU test; gate 30 mm.  The seeds are those
# whose every decision clears MARGIN (tests/test_tracks_cpu.py asserts it for each).
SCENES = (("one", 1, 1, 32, 0, (), 0),
          ("two", 2, 2, 32, 0, (), 0),
          ("two_in_three", 2, 3, 32, 0, (), 0),
          ("three_in_four", 3, 4, 32, 0, (), 0),
          ("three_in_eight_gap3", 3, 8, 32, 0, ((1, 10, 3),), 4),
          ("eight", 8, 8, 32, 0, (), 0),
          ("three_in_four_gap7", 3, 4, 32, 0, ((2, 12, 7),), 4))
GATE = 30.0


def scene_by_name(name, cams=4):
    _, S, K, T, seed, gaps, max_missed = next(s for s in SCENES if s[0] == name)
    return scene(S, K, T, seed, gaps, cams), K, max_missed


def cut(sc, t, nul=False):
    """The first t frame sets of a scene as (centers, views, members, error); nul: the last three None."""
    return tuple(None if nul and n != "centers" else sc[n][:t] for n in ("centers", "views", "members", "error"))


def scene_cases(name):
    """Every (what, inputs, params) the GPU test runs on scene `name`: t = 1, 2, 7, 32 and cams = 2, 12 with predict and
    coast on; predict and coast off; the NULL views / members / error form with max_missed 0 (a scene with a gap then
    ends a track and bears another); max_jump_mm = +inf.  tests/test_tracks_cpu.py runs each through the margin
    assertion."""
    out = []
    for cams in (2, 12):
        sc, K, mm = scene_by_name(name, cams)
        for t in (1, 2, 7, 32):
            out.append(((name, cams, t), cut(sc, t), params(K, GATE, mm, 1, 1)))
        out.append(((name, cams, "predict 0"), cut(sc, 32), params(K, GATE, mm, 0, 0)))
    sc, K, mm = scene_by_name(name, 2)
    out.append(((name, "null form"), cut(sc, 32, nul=True), params(K, GATE, 0, 1, 1)))
    out.append(((name, "open gate"), cut(sc, 32), params(K, np.inf, mm, 1, 0)))
    return out


def ids_of_subjects(out, truth):
    """{subject: the set of ids it carried}, through slots: row (t, k) holds detection slots[t, k] of frame set t."""
    seen = {}
    T, K = out["slots"].shape
    for t in range(T):
        for k in range(K):
            i = out["slots"][t, k]
            if i >= 0:
                seen.setdefault(int(truth[t, i]), set()).add(int(out["ids"][t, k]))
    return seen
