"""What subject tracking costs (jh_op_track_subjects: one 64-lane wave walks the frame sets of a call in order), on one
GPU at BASELINE configs[2] (12 cameras 1280 x 1024), small models.  HIP events, median of the passes:
  a  the operator alone at (t, K) = (1, 2), (32, 2), (32, 8), cams 12: subjects 100 mm apart moving 10 mm per frame set,
     rows rotated per frame set, gate 30 mm -- every step matches: SubjectTracker.update per call as the host enqueues
     it (reset + update, less reset), and the kernel alone from the library's per-launch profile (jh_profile_*);
  b  forward_subjects at t = 32, K = 2 on fp32 frames resident in HBM, without and with a tracker;
  c  the shipped driver from host memory (uint8 BGR numpy frame sets) at time_batch 32 with streams 1 and 3:
     max_subjects=2 with a tracker, max_subjects=2 without, and the single-subject driver, in the same run (wall clock
     around the whole call: the driver ends in a host synchronisation).
python tools/tracks_probe.py [--passes 7] [--calls 50] [--driver-batches 4] [--out profiles/r10_tracks_probe.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from jarvis_hybridnet_amd import Subjects, SubjectTracker  # noqa: E402
from jarvis_hybridnet_amd import _native as N  # noqa: E402
from jarvis_hybridnet_amd import synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402
from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames  # noqa: E402

INF = float("inf")


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return dict(ms=median(v), ms_min=min(v), ms_max=max(v))


def event_ms(fn, calls, passes):
    """HIP-event time of `calls` calls of fn(), per call."""
    ms = []
    for _ in range(passes):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / calls)
    return spread(ms)


def moving_subjects(t, K, cams):
    """K subjects 100 mm apart moving 10 mm per frame set along x, their rows rotated by one per frame set."""
    centers = np.zeros((t, K, 3), np.float32)
    for f in range(t):
        for s in range(K):
            centers[f, (s + f) % K] = (10.0 * f, 100.0 * s, 0.0)
    return Subjects(torch.from_numpy(centers).cuda(), torch.full((t, K), cams, dtype=torch.int32, device="cuda"),
                    torch.zeros((t, K, cams), dtype=torch.int32, device="cuda"), torch.ones((t, K), device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed pass of part a")
    ap.add_argument("--driver-batches", type=int, default=4, help="time batches of a timed driver run")
    ap.add_argument("--out", default=os.path.join("profiles", "r10_tracks_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tracks_probe: no GPU; a timing needs one")
    c, T = bench.CONFIGS["cfg3"], 32
    H, W, C, J = c["H"], c["W"], c["C"], c["J"]
    out = dict(config="cfg3", cameras=C, height=H, width=W, models="small", passes=a.passes, operator={})
    # a: the operator
    for t, K in ((1, 2), (32, 2), (32, 8)):
        subj = moving_subjects(t, K, C)
        tr = SubjectTracker(K, 30.0, max_missed=2)

        def step():
            tr.reset()
            tr.update(subj)
        for _ in range(5):
            step()
        reset = event_ms(tr.reset, a.calls, a.passes)
        both = event_ms(step, a.calls, a.passes)
        _, tracks = tr.update(subj)
        kernel = []                                             # (the library's per-launch profile: the kernel alone)
        for _ in range(a.passes):
            tr.reset()
            kernel += [r[1] for r in N.profile(lambda: tr.update(subj)) if r[0] == "track_subjects"]
        assert len(kernel) == a.passes
        out["operator"]["t%d_K%d" % (t, K)] = dict(reset_and_update=both, reset=reset, kernel=spread(kernel),
                                                    update_ms=both["ms"] - reset["ms"],
                                                    matched=int((tracks.slots >= 0).sum()))
    # b: forward_subjects
    cfg = NS(PARENT_DIR="/nonexistent", PROJECT_NAME="probe", DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
             CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center"]),
             KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=J, BOUNDING_BOX_SIZE=c["bbox"]),
             HYBRIDNET=NS(NUM_CAMERAS=C, ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(J)]
    calib = S.ring_calibration(C, W, H, c["focal"])
    dev = [t.cuda() for t in calib]
    pred = JarvisPredictor3D(cfg, S.efficienttrack_weights("small", 1, c["seeds"][0]),
                             S.hybridnet_weights("small", J, c["seeds"][1]))
    base = torch.stack([S.blob_frames(calib, W, H, J, c["seeds"][2] + i)[0] for i in range(4)])
    x = base[torch.arange(T) % 4].cuda()
    kw = dict(max_peaks=2, min_peak=-INF, max_error_px=INF)
    tr = SubjectTracker(2, INF, max_missed=2)
    for _ in range(3):
        pred.forward_subjects(x, *dev, 2, **kw)
        pred.forward_subjects(x, *dev, 2, tracker=tr, **kw)
    plain = event_ms(lambda: pred.forward_subjects(x, *dev, 2, **kw), 3, a.passes)
    tracked = event_ms(lambda: pred.forward_subjects(x, *dev, 2, tracker=tr, **kw), 3, a.passes)
    single = event_ms(lambda: pred.forward_batch(x, *dev), 3, a.passes)
    res = pred.forward_subjects(x, *dev, 2, tracker=tr, **kw)
    out["forward_subjects_t32_K2"] = dict(without_tracker=plain, with_tracker=tracked, forward_batch=single,
                                          valid_rows=int(res[2].sum()))
    del x
    # c: the driver
    bgr = (base.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).numpy()      # (4,C,H,W,3)
    out["driver_t32"] = {}
    modes = {"single_subject": {}, "subjects2": dict(max_subjects=2, subject_params=kw),
             "subjects2_tracked": dict(max_subjects=2, subject_params=kw, track=dict(max_jump_mm=INF, max_missed=2))}
    with tempfile.TemporaryDirectory() as tmp:
        for streams in (1, 3):
            row = {}
            for name, mkw in modes.items():
                def gen(n):
                    return (bgr[i % 4] for i in range(n))
                dkw = dict(time_batch=T, streams=streams, **mkw)
                predict3D_frames(pred, gen(T * streams), *dev, cfg, tmp, **dkw)          # buffers, plans
                n, rates = T * a.driver_batches, []
                for _ in range(a.passes):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert predict3D_frames(pred, gen(n), *dev, cfg, tmp, **dkw) == n
                    rates.append(n / (time.perf_counter() - t0))
                row[name] = dict(sets_per_s=median(rates), sets_per_s_min=min(rates), sets_per_s_max=max(rates))
            row["tracked_vs_untracked"] = row["subjects2_tracked"]["sets_per_s"] / row["subjects2"]["sets_per_s"]
            row["subjects2_vs_single"] = row["subjects2"]["sets_per_s"] / row["single_subject"]["sets_per_s"]
            out["driver_t32"]["streams_%d" % streams] = row
            release_ingest_buffers(pred)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
