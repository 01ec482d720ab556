"""numpy reference of the two definitions behind detect_subjects (include/jarvis_hip.h: jh_op_center_peaks,
jh_op_associate_subjects), written from the definitions and not from the kernels: brute-force windows for the peaks,
float64 SVD for the triangulations.  Shared by tests/test_subjects_cpu.py (hand-made cases) and
tests/test_hip_subjects.py (the kernels against it)."""
import itertools

import numpy as np

EMPTY = (-1.0, -1.0, -np.inf)


def peaks_ref(heat, max_peaks, nms_radius, min_peak):
    """heat (N,Hh,Wh) float32 -> peaks (N,P,3) float32 = (x, y, value), count (N,) int32.
    p is a peak iff v(p) > min_peak and no q != p within |dx|, |dy| <= r (clipped at the edge) has v(q) > v(p) or
    (v(q) == v(p) and q < p); NaN compares false both ways.  Ordered by (value descending, index ascending);
    x = p % Hh, y = p // Wh (the arg-max kernel's expression)."""
    heat = np.asarray(heat, dtype=np.float32)
    N, Hh, Wh = heat.shape
    r = int(nms_radius)
    peaks = np.empty((N, max_peaks, 3), np.float32)
    peaks[:] = np.array(EMPTY, np.float32)
    count = np.zeros((N,), np.int32)
    with np.errstate(invalid="ignore"):
        for n in range(N):
            v = heat[n]
            ok = v > np.float32(min_peak)
            pad = np.full((Hh + 2 * r, Wh + 2 * r), np.nan, np.float32)      # (outside the map: never suppresses)
            pad[r:r + Hh, r:r + Wh] = v
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if dy == 0 and dx == 0:
                        continue
                    q = pad[r + dy:r + dy + Hh, r + dx:r + dx + Wh]
                    earlier = dy < 0 or (dy == 0 and dx < 0)                 # q's flat index is below p's
                    ok &= ~((q > v) | ((q == v) & earlier))
            idx = np.flatnonzero(ok.ravel())
            vals = v.ravel()[idx]
            order = np.lexsort((idx, -vals.astype(np.float64)))              # value descending, then index ascending
            idx = idx[order][:max_peaks]
            count[n] = len(idx)
            for k, m in enumerate(idx):
                peaks[n, k] = (m % Hh, m // Wh, v.ravel()[m])
    return peaks, count


def project64(X, cam, intr, dist):
    """reprojectPoint of one 3D point in float64 -> uv (C,2), depth (C,)."""
    q = np.concatenate([np.asarray(X, np.float64), [1.0]]) @ cam          # (C,3)
    with np.errstate(all="ignore"):
        u = q[:, 0] / q[:, 2] - intr[:, 2, 0]
        v = q[:, 1] / q[:, 2] - intr[:, 2, 1]
        r2 = (u / intr[:, 0, 0]) ** 2 + (v / intr[:, 1, 1]) ** 2
        d = 1 + (dist[:, 0, 0] + dist[:, 0, 1] * r2) * r2
        return np.stack([u * d + intr[:, 2, 0], v * d + intr[:, 2, 1]], 1), q[:, 2]


def dlt64(obs, cam, intr, dist):
    """reconstructPoint over the observations obs = [(camera, u, v, weight)] in float64 -> (3,)."""
    rows = []
    for c, u, v, w in obs:
        P = cam[c].T                                                       # (3,4)
        uu, vv = u - intr[c, 2, 0], v - intr[c, 2, 1]
        r2 = (uu / intr[c, 0, 0]) ** 2 + (vv / intr[c, 1, 1]) ** 2
        dd = 1 + (dist[c, 0, 0] + dist[c, 0, 1] * r2) * r2
        uu, vv = uu / dd + intr[c, 2, 0], vv / dd + intr[c, 2, 1]
        rows += [(uu * P[2] - P[0]) * w, (vv * P[2] - P[1]) * w]
    with np.errstate(all="ignore"):
        X = np.linalg.svd(np.asarray(rows))[2][-1]
        return X[:3] / X[3]


def scene_peaks(calib, points, values, sx2, sy2, max_peaks, hidden=(), extra=()):
    """Synthetic peaks of one frame set: the 3D `points` (S,3) projected with oracle.reproject_point under calib = (cam,
    intr, dist) torch tensors and rounded to the heat-map grid (so at most (sx2/2, sy2/2) from the projection), subject
    s with value values[s] in every camera except the (camera, subject) pairs of `hidden`; extra: (camera, x, y,
    value) peaks that belong to nothing.  -> (C,P,3) float32, every camera's slots by value descending, empty slots
    (-1, -1, -inf)."""
    import torch
    from oracle import hybridnet_oracle as O
    C = calib[0].shape[0]
    per_cam = [[] for _ in range(C)]
    for s, X in enumerate(points):
        uv = O.reproject_point(torch.tensor(X, dtype=torch.float32)[None], *calib).numpy()
        for c in range(C):
            if (c, s) not in hidden:
                per_cam[c].append((float(np.round(uv[c, 0] / sx2)), float(np.round(uv[c, 1] / sy2)), float(values[s])))
    for c, x, y, v in extra:
        per_cam[c].append((float(x), float(y), float(v)))
    out = np.empty((C, max_peaks, 3), np.float32)
    out[:] = np.array(EMPTY, np.float32)
    for c in range(C):
        rows = sorted(per_cam[c], key=lambda p: -p[2])
        assert len(rows) <= max_peaks
        for k, p in enumerate(rows):
            out[c, k] = p
    return out


def associate_ref(peaks, cam, intr, dist, mask, sx2, sy2, max_subjects, max_error_px, min_views, margin=None):
    """One frame set: peaks (C,P,3), calibration (C,..) float, mask (C,) or None -> centers (K,3), views (K,), members
    (K,C), error (K,) as jh_op_associate_subjects defines them, in float64.
    margin (px): assert that nothing rests on a float tie -- in every round the chosen candidate has strictly more
    views than every candidate with another member set or beats it in cost by more than `margin`; no support distance
    lies within `margin` of max_error_px; the nearest peak of a camera is nearer than its runner-up by more than
    `margin`."""
    cam, intr, dist = (np.asarray(a, np.float64) for a in (cam, intr, dist))
    peaks = np.asarray(peaks, np.float32)
    C, P = peaks.shape[:2]
    K = max_subjects
    live = np.ones(C, bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid="ignore"):
        state = live[:, None] & (peaks[..., 0] >= 0) & (peaks[..., 1] >= 0)      # unused and usable
    px = peaks[..., 0].astype(np.float64) * sx2
    py = peaks[..., 1].astype(np.float64) * sy2
    wt = peaks[..., 2].astype(np.float64) / 255.0
    centers = np.full((K, 3), np.nan)
    views = np.zeros(K, np.int32)
    members = np.full((K, C), -1, np.int32)
    error = np.full(K, np.nan)

    def support(X):
        uv, depth = project64(X, cam, intr, dist)
        mem, ds = [-1] * C, []
        for c in range(C):
            slots = np.flatnonzero(state[c])
            if len(slots) == 0:
                continue
            d = np.hypot(uv[c, 0] - px[c, slots], uv[c, 1] - py[c, slots])
            if np.all(np.isnan(d)):
                continue
            o = np.argsort(np.where(np.isnan(d), np.inf, d), kind="stable")
            best = d[o[0]]
            if margin is not None:
                assert not abs(best - max_error_px) <= margin, "a support distance on the bound"
                if len(o) > 1 and np.isfinite(d[o[1]]) and best <= max_error_px + margin:
                    assert d[o[1]] - best > margin, "two peaks of a camera equally near"
            if depth[c] > 0 and best <= max_error_px:
                mem[c] = int(slots[o[0]])
                ds.append(best)
        return mem, ds

    for k in range(K):
        cands = []
        for a, b in itertools.combinations(range(C), 2):
            for i, j in itertools.product(np.flatnonzero(state[a]), np.flatnonzero(state[b])):
                X = dlt64([(a, px[a, i], py[a, i], wt[a, i]), (b, px[b, j], py[b, j], wt[b, j])], cam, intr, dist)
                if not np.all(np.isfinite(X)):
                    continue
                mem, ds = support(X)
                cands.append((-len(ds), float(np.sum(ds)), (a, int(i), b, int(j)), tuple(mem)))
        if not cands:
            break
        cands.sort(key=lambda t: t[:3])
        nv, cost, _, mem = cands[0]
        if margin is not None:
            for nv2, cost2, _, mem2 in cands[1:]:
                if mem2 != mem and -nv >= min_views:
                    assert nv2 > nv or cost2 - cost > margin, "the choice rests on a float tie"
        if -nv < min_views:
            break
        obs = [(c, px[c, s], py[c, s], wt[c, s]) for c, s in enumerate(mem) if s >= 0]
        ctr = dlt64(obs, cam, intr, dist)
        uv, _ = project64(ctr, cam, intr, dist)
        centers[k], views[k], members[k] = ctr, -nv, mem
        error[k] = np.mean([np.hypot(uv[c, 0] - u, uv[c, 1] - v) for c, u, v, _ in obs])
        for c, s in enumerate(mem):
            if s >= 0:
                state[c, s] = False
    return centers, views, members, error
