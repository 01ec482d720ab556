"""What the per-joint robust triangulation costs (jh_predictor_triangulate_joints: the all-joint arg-max scan, the
observations with their sub-pixel refinement, the consensus), on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024,
23 keypoints, bbox 256, 64^3 grid), small models, fp32 frames resident in HBM as bench.py feeds them.  In one process,
timed with HIP events after a warm-up, median of the passes:
  1  the kernels alone, from the library's per-launch profile of one call behind a 32-frame forward: the scan
     ("joint_argmax_all", shared with the 2D views), "joint_observations" at refine_radius 0 .. 3 and "joints3d",
     milliseconds; the members the consensus finds are reported beside them (the models' weights are random: their
     cameras need not agree, and the work of the consensus does not depend on whether they do);
  2  the whole call against views2d, behind the same forward: milliseconds per call of 32 frame sets;
  3  the forward with and without return_triangulated: time_batch 1 under graph replay (milliseconds per frame set) and
     3 streams x 32 frame sets (MultiStreamPredictor, the throughput form bench.py measures: frame sets per second);
     "off" is measured before and after "on" -- the two differ by the run's own repeat-to-repeat scatter.
python tools/triangulate_probe.py [--passes 7] [--calls 50] [--steps 4] [--out profiles/r09_triangulate_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import torch  # noqa: E402

import bench  # noqa: E402
from centers_probe import timed  # noqa: E402
from jarvis_hybridnet_amd import _native as N  # noqa: E402
from jarvis_hybridnet_amd import synthetic as S  # noqa: E402
from jarvis_hybridnet_amd._predictor import MultiStreamPredictor, NativePredictor  # noqa: E402

KERNELS = ("joint_argmax_all", "joint_observations", "joints3d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="time_batch 1: forwards per timed pass")
    ap.add_argument("--steps", type=int, default=4, help="3 x 32: steps (one batch per stream) per timed pass")
    ap.add_argument("--out", default=os.path.join("profiles", "r09_triangulate_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("triangulate_probe: no GPU; a timing needs one")
    c, T, K = bench.CONFIGS["cfg3"], a.time_batch, a.streams
    H, W, C, J = c["H"], c["W"], c["C"], c["J"]
    calib = S.ring_calibration(C, W, H, c["focal"])
    calib_dev = [t.cuda() for t in calib]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", J, c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, J, c["seeds"][2] + i)[0] for i in range(4)]).cuda()
    x = base[torch.arange(T, device="cuda") % 4].contiguous()                     # (T,C,3,H,W) fp32

    def make(frames):
        return NativePredictor(sd_c, sd_h, num_cameras=C, num_joints=J, center_size=c["center"], bbox=c["bbox"],
                               roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN,
                               std=S.STD, time_batch=frames)
    out = dict(config="cfg3", cameras=C, height=H, width=W, joints=J, models="small", frames="fp32 RGB, resident",
               passes=a.passes)

    msp = MultiStreamPredictor(lambda: make(T), streams=K)
    msp.set_calibration(*calib_dev)
    outs = [(torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda"),
             torch.empty((T,), device="cuda", dtype=torch.int32)) for _ in range(K)]
    msp.forward(x, outs[0])
    msp.synchronize()
    want = outs[0][0].clone()
    p32 = msp.preds[0]
    p32.forward(x, outs[0])
    torch.cuda.synchronize()

    # ---- 1: the kernels alone
    rows = {}
    for r in (0, 1, 2, 3):
        for name, kw in (("default_bounds", {}), ("no_bounds", dict(max_error_px=float("inf"), min_conf=0.0))):
            p = N.joints3d_params(refine_radius=r, **kw)
            ms = {k: [] for k in KERNELS}
            for _ in range(a.passes + 2):
                prof = N.profile(lambda: p32.triangulate_joints(params=p))
                for k in KERNELS:
                    ms[k].append(sum(rec[1] for rec in prof if rec[0] == k))
            tri = p32.triangulate_joints(params=p)
            torch.cuda.synchronize()
            row = {k: sorted(v[2:])[len(v[2:]) // 2] for k, v in ms.items()}
            row["sum_ms"] = sum(row[k] for k in KERNELS)
            row["joints_found"] = int((tri.views > 0).sum())
            row["mean_views"] = float(tri.views.float().mean())
            rows["radius_%d_%s" % (r, name)] = row
    out["kernels_alone"] = dict(time_batch=T, joints=T * J, **rows)

    # ---- 2: the whole call against views2d
    p = N.joints3d_params()

    def tri_calls(n=20):
        for _ in range(n):
            p32.triangulate_joints(params=p)

    def v2d_calls(n=20):
        for _ in range(n):
            p32.views2d(outs[0][0])
    rows = {}
    for name, fn in (("triangulate_joints", tri_calls), ("views2d", v2d_calls)):
        fn(3)
        r = timed(fn, a.passes)
        rows[name] = {k + "_per_call": v / 20 for k, v in r.items()}
    out["whole_call"] = dict(time_batch=T, **rows)

    # ---- 3a: the forward, K streams x T frame sets
    rows = {}
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        def steps(n=a.steps):
            for _ in range(n):
                for i in range(K):
                    msp.forward(x, outs[i], return_triangulated=on)
            cur = torch.cuda.current_stream()
            for s in msp.streams:
                cur.wait_stream(s)
        steps(a.warmup)
        r = timed(steps, a.passes)
        sets = a.steps * K * T
        rows[name] = dict(r, frame_sets_per_s=sets / (r["ms"] * 1e-3), ms_per_batch=r["ms"] / (a.steps * K))
        torch.cuda.synchronize()
        rows[name]["equals_off_bits"] = bool(torch.equal(outs[0][0], want))
    rows["on_vs_off"] = rows["on"]["frame_sets_per_s"] / rows["off"]["frame_sets_per_s"]
    rows["off_again_vs_off"] = rows["off_again"]["frame_sets_per_s"] / rows["off"]["frame_sets_per_s"]
    rows["on_minus_off_ms_per_batch"] = rows["on"]["ms_per_batch"] - rows["off"]["ms_per_batch"]
    out["streams_x_time_batch"] = dict(streams=K, time_batch=T, steps_per_pass=a.steps, **rows)

    # ---- 3b: time_batch 1, graph replay
    p1 = make(1)
    p1.set_calibration(*calib_dev)
    assert p1.graph_replay
    x1 = x[:1].contiguous()
    res = p1.forward(x1)
    torch.cuda.synchronize()
    assert int(res[2][0]) == 1, "the probe's frame set must be a valid detection"
    want1 = res[0].clone()
    rows = {}
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        def calls(n=a.calls):
            for _ in range(n):
                p1.forward(x1, res)
                if on:
                    p1.triangulate_joints(params=p)
        calls(10)
        r = timed(calls, a.passes)
        rows[name] = {k + "_per_frame_set": v / a.calls for k, v in r.items()}
        torch.cuda.synchronize()
        rows[name]["equals_off_bits"] = bool(torch.equal(res[0], want1))
    rows["on_minus_off_ms"] = rows["on"]["ms_per_frame_set"] - rows["off"]["ms_per_frame_set"]
    rows["off_again_minus_off_ms"] = rows["off_again"]["ms_per_frame_set"] - rows["off"]["ms_per_frame_set"]
    out["time_batch_1_graph"] = dict(calls_per_pass=a.calls, **rows)

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
