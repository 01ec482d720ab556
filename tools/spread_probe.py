"""What the per-joint 3D spread costs (jh_predictor_set_spread: covariance, peak and mass of the V2V heat map from the
soft-argmax tail's own pass), on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024, 23 keypoints, bbox 256, 64^3
grid), small models, fp32 frames resident in HBM as bench.py feeds them.  Spread off against spread on in the same
process, timed with HIP events after a warm-up, median of the passes:
  1  time_batch 1 with graph replay: milliseconds per frame set (the spread's copy-out included when it is on);
  2  3 streams x 32 frame sets (MultiStreamPredictor, the throughput form bench.py measures): `frame_sets_per_s`;
  3  the tail alone, from the library's per-launch profile of one 32-frame forward: the plain tail ("softargmax") and
     the spread form ("softargmax_spread"), milliseconds.  `fused_extra_ms` is what the fused form adds.  A second
     kernel for the spread would do all of that work too -- the same double accumulations, block reduction and atomics
     -- after reading the volume and evaluating softplus a second time, and pay a launch: `fused_extra_ms` is a lower
     bound of what a two-pass form would add, which is why none is built or timed.
python tools/spread_probe.py [--passes 7] [--calls 50] [--steps 4] [--out profiles/r07_spread_probe.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="time_batch 1: forwards per timed pass")
    ap.add_argument("--steps", type=int, default=4, help="3 x 32: steps (one batch per stream) per timed pass")
    ap.add_argument("--out", default=os.path.join("profiles", "r07_spread_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spread_probe: no GPU; a timing needs one")
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
    out = dict(config="cfg3", cameras=C, height=H, width=W, models="small", frames="fp32 RGB, resident",
               passes=a.passes)

    # ---- 1: time_batch 1, graph replay
    p1 = make(1)
    p1.set_calibration(*calib_dev)
    assert p1.graph_replay
    x1 = x[:1].contiguous()
    res = p1.forward(x1)
    torch.cuda.synchronize()
    assert int(res[2][0]) == 1, "the probe's frame set must be a valid detection"
    want = res[0].clone()
    rows = {}
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        def calls(n=a.calls):
            for _ in range(n):
                p1.forward(x1, res, return_spread=on)
        calls(10)
        r = timed(calls, a.passes)
        rows[name] = {k + "_per_frame_set": v / a.calls for k, v in r.items()}
        torch.cuda.synchronize()
        rows[name]["equals_off_bits"] = bool(torch.equal(res[0], want))
    rows["on_minus_off_ms"] = rows["on"]["ms_per_frame_set"] - rows["off"]["ms_per_frame_set"]
    out["time_batch_1_graph"] = dict(calls_per_pass=a.calls, **rows)

    # ---- 2: K streams x T frame sets
    msp = MultiStreamPredictor(lambda: make(T), streams=K)
    msp.set_calibration(*calib_dev)
    outs = [(torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda"),
             torch.empty((T,), device="cuda", dtype=torch.int32)) for _ in range(K)]
    msp.forward(x, outs[0])
    msp.synchronize()
    want = outs[0][0].clone()
    rows = {}
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        def steps(n=a.steps):
            for _ in range(n):
                for i in range(K):
                    msp.forward(x, outs[i], return_spread=on)
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
    rows["on_minus_off_ms_per_batch"] = rows["on"]["ms_per_batch"] - rows["off"]["ms_per_batch"]
    out["streams_x_time_batch"] = dict(streams=K, time_batch=T, steps_per_pass=a.steps, **rows)

    # ---- 3: the tail alone (the library's per-launch HIP-event profile of one T-frame forward)
    p32 = msp.preds[0]
    rows = {}
    for name, on in (("softargmax", False), ("softargmax_spread", True)):
        ms = []
        for _ in range(a.passes + 2):
            prof = N.profile(lambda: p32.forward(x, outs[0], return_spread=on))
            ms.append(sum(r[1] for r in prof if r[0] == name))
        ms = sorted(ms[2:])
        rows[name] = dict(ms=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1])
    rows["fused_extra_ms"] = rows["softargmax_spread"]["ms"] - rows["softargmax"]["ms"]
    out["tail_alone"] = dict(time_batch=T, **rows)

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
