"""What centre keyframes buy (jh_predictor_set_center_keyframes: CenterDetect on every k-th frame set of a time batch
and on the last one, the rows in between on an interpolated centre), on one GPU at BASELINE configs[2] (12 cameras
1280 x 1024, 23 keypoints, bbox 256, 64^3 grid), small models, fp32 frames resident in HBM as bench.py feeds them.
  1  3 streams x 32 frame sets (MultiStreamPredictor, the throughput form bench.py measures), in ONE run and interleaved
     -- every pass times every mode once, in turn --: detected, center_every = 1, 2, 4, 8, and centred (the detected
     run's own centres, so stage 2 and 3 do the same work).  `frame_sets_per_s` is the multi-view frames/s of bench.py.
     One untimed step in front of every timed window switches the predictors to the mode (another every builds another
     key plan, which synchronises the device) and warms it, so no timed window builds anything.
  2  One predictor, one time batch, per-launch HIP events (_native.profile): stage 1 of the full plan (everything up to
     the centre arg-max) against stage 1 of the key plan (up to the detection scatter) for each every, and the three new
     kernels' own times.
python tools/center_keyframes_probe.py [--passes 7] [--steps 4] [--out profiles/r15_center_keyframes_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import torch  # noqa: E402

import bench  # noqa: E402
from jarvis_hybridnet_amd import _native as N  # noqa: E402
from jarvis_hybridnet_amd import synthetic as S  # noqa: E402
from jarvis_hybridnet_amd._predictor import MultiStreamPredictor, NativePredictor  # noqa: E402

NEW_KERNELS = ("center_key_table", "center_key_scatter", "center_key_fill")


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    """The HIP-event time of fn() in milliseconds; fn enqueues on the current stream or makes it wait for what it
    enqueued elsewhere."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stage1(profile, last):
    """Milliseconds of the launches of a profiled forward up to and including the one named `last`."""
    names = [r[0] for r in profile]
    end = names.index(last) + 1
    return sum(r[1] for r in profile[:end]), end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4, help="steps (one batch per stream) per timed pass")
    ap.add_argument("--out", default=os.path.join("profiles", "r15_center_keyframes_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("center_keyframes_probe: no GPU; a timing needs one")
    c, T, K = bench.CONFIGS["cfg3"], a.time_batch, a.streams
    H, W, C, J = c["H"], c["W"], c["C"], c["J"]
    calib = S.ring_calibration(C, W, H, c["focal"])
    calib_dev = [t.cuda() for t in calib]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", J, c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, J, c["seeds"][2] + i)[0] for i in range(4)]).cuda()
    x = base[torch.arange(T, device="cuda") % 4].contiguous()                     # (T,C,3,H,W) fp32

    def make():
        return NativePredictor(sd_c, sd_h, num_cameras=C, num_joints=J, center_size=c["center"], bbox=c["bbox"],
                               roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN,
                               std=S.STD, time_batch=T)
    out = dict(config="cfg3", cameras=C, height=H, width=W, models="small", frames="fp32 RGB, resident",
               passes=a.passes)

    # ---- 1: K streams x T frame sets, every mode once per pass
    plain = MultiStreamPredictor(make, streams=K)
    plain.set_calibration(*calib_dev)
    outs = [(torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda"),
             torch.empty((T,), device="cuda", dtype=torch.int32)) for _ in range(K)]
    plain.forward(x, outs[0])
    plain.synchronize()
    kT = plain.preds[0].debug("cuda")["center3d"].clone()
    torch.cuda.synchronize()
    valid, want = int(outs[0][2].sum()), outs[0][0].clone()
    modes = [("detected", plain, {}), ("centred", plain, dict(centers=kT))]
    modes += [("every_%d" % k, plain, dict(center_every=k)) for k in a.every]

    def steps(msp, kw, n):
        for _ in range(n):
            for i in range(K):
                msp.forward(x, outs[i], **kw)
        cur = torch.cuda.current_stream()
        for s in msp.streams:
            cur.wait_stream(s)
    times = {name: [] for name, _, _ in modes}
    for name, msp, kw in modes:
        steps(msp, kw, a.warmup)
    for _ in range(a.passes):
        for name, msp, kw in modes:
            steps(msp, kw, 1)                                      # (the switch to this mode, outside the window)
            times[name].append(event_ms(lambda: steps(msp, kw, a.steps)))
    sets = a.steps * K * T
    rows = {}
    for name, msp, kw in modes:
        ms = median(times[name])
        rows[name] = dict(ms=ms, ms_min=min(times[name]), ms_max=max(times[name]), frame_sets_per_s=sets / (ms * 1e-3),
                          frames_per_s=sets * C / (ms * 1e-3))
        steps(msp, kw, 1)
        torch.cuda.synchronize()
        rows[name]["equals_detected_bits"] = bool(torch.equal(outs[K - 1][0], want))
        if "center_every" in kw:
            rows[name]["key_rows"] = len(N.center_keyframe_rows(T, kw["center_every"]))
        rows[name]["vs_detected"] = rows[name]["frame_sets_per_s"] / rows["detected"]["frame_sets_per_s"]
    out["streams_x_time_batch"] = dict(streams=K, time_batch=T, steps_per_pass=a.steps, valid_frame_sets=valid, **rows)
    del modes, plain

    # ---- 2: one predictor, per-launch events: stage 1 of the full plan and of the key plans, the new kernels
    pr = make()
    pr.set_calibration(*calib_dev)
    res = pr.forward(x)
    torch.cuda.synchronize()

    def profiled(**kw):
        pr.forward(x, res[:3], **kw)                               # (warm: the plan of this every is built here)
        runs = [N.profile(lambda: pr.forward(x, res[:3], **kw)) for _ in range(a.passes)]
        torch.cuda.synchronize()
        return runs
    runs = profiled()
    full = median([stage1(r, "center_argmax")[0] for r in runs])
    prof = dict(full_plan=dict(stage1_ms=full, launches=stage1(runs[0], "center_argmax")[1],
                               forward_ms=median([sum(q[1] for q in r) for r in runs])))
    for k in a.every:
        runs = profiled(center_every=k)
        row = dict(key_rows=len(N.center_keyframe_rows(T, k)),
                   stage1_ms=median([stage1(r, "center_key_scatter")[0] for r in runs]),
                   launches=stage1(runs[0], "center_key_scatter")[1],
                   forward_ms=median([sum(q[1] for q in r) for r in runs]))
        for name in NEW_KERNELS:
            row[name + "_us"] = 1e3 * median([sum(q[1] for q in r if q[0] == name) for r in runs])
        row["stage1_vs_full"] = row["stage1_ms"] / full
        prof["every_%d" % k] = row
    out["stage_1_profiled"] = dict(time_batch=T, note="per-launch HIP events on one stream: no overlap between launches",
                                   **prof)

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
