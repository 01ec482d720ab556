"""What the per-joint camera masks cost (jh_predictor_set_joint_mask: the joint-masked voxel-row gather in place of the
cube gather, the consensus between stage 2 and stage 3, plain launches in place of the graph replay), on one GPU at
BASELINE configs[2] (12 cameras 1280 x 1024, 23 keypoints, bbox 256, 64^3 grid), small models, fp32 frames resident in
HBM as bench.py feeds them.  In one process, after a warm-up, the variants alternating inside every pass, medians:
  1  the gather per 32 frame sets, from the library's per-launch profile of a forward: the plain cube gather, the
     camera-masked one with all ones, the joint-masked one (its set kernel included) with all ones and with the members
     of the consensus (whose three kernels are reported beside it, with the share of partial and empty rows: the models'
     weights are random, so their cameras need not agree);
  2  3 streams x 32 frame sets (MultiStreamPredictor, the throughput form bench.py measures), plain against
     joint_mask='consensus', HIP events: frame sets per second; "off" is measured before and after "on";
  3  one frame set: the plain forward under graph replay against the joint-masked call, which runs plain launches --
     what leaving the graph costs --, with all ones and with the consensus: milliseconds per frame set.
python tools/joint_mask_probe.py [--passes 7] [--calls 50] [--steps 4] [--out profiles/r11_joint_mask_probe.json]"""
import argparse
import json
import os
import sys
from statistics import median

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import torch  # noqa: E402

import bench  # noqa: E402
from centers_probe import timed  # noqa: E402
from jarvis_hybridnet_amd import _native as N  # noqa: E402
from jarvis_hybridnet_amd import synthetic as S  # noqa: E402
from jarvis_hybridnet_amd._predictor import MultiStreamPredictor, NativePredictor  # noqa: E402

GATHERS = ("reproject_gather", "reproject_gather_masked", "reproject_gather_joint_masked")
CONSENSUS = ("joint_argmax_all", "joint_observations", "joints3d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="one frame set: forwards per timed pass")
    ap.add_argument("--steps", type=int, default=4, help="3 x 32: steps (one batch per stream) per timed pass")
    ap.add_argument("--out", default=os.path.join("profiles", "r11_joint_mask_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("joint_mask_probe: no GPU; a timing needs one")
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

    # ---- 1: the gather alone
    ones_c = torch.ones((T, C), dtype=torch.uint8, device="cuda")
    ones_j = torch.ones((T, J, C), dtype=torch.uint8, device="cuda")
    variants = (("plain_cube", {}), ("camera_masked_all_ones", dict(camera_mask=ones_c)),
                ("joint_masked_all_ones", dict(joint_mask=ones_j)), ("joint_masked_consensus", dict(joint_mask="consensus")))
    ms = {name: {k: [] for k in GATHERS + CONSENSUS} for name, _ in variants}
    bits, used = {}, None
    for i in range(a.passes + 2):
        for name, kw in variants:
            prof = N.profile(lambda: p32.forward(x, outs[0], **kw))
            for k in GATHERS + CONSENSUS:
                ms[name][k].append(sum(rec[1] for rec in prof if rec[0] == k))
            torch.cuda.synchronize()
            bits[name] = bool(torch.equal(outs[0][0], want))
    used = p32.joint_mask()
    torch.cuda.synchronize()
    rows = {}
    for name, _ in variants:
        row = {k + "_ms": median(v[2:]) for k, v in ms[name].items() if max(v) > 0}
        row["points_equal_plain_bits"] = bits[name]
        rows[name] = row
    n = used.count.float()
    rows["joint_masked_consensus"].update(partial_rows=float(((n > 0) & (n < C)).float().mean()),
                                          mean_cameras=float(n.mean()))
    out["gather_alone"] = dict(time_batch=T, **rows)
    p32.forward(x, outs[0])                                                      # (the joint mask is off again)

    # ---- 2: K streams x T frame sets
    rows = {}
    for name, jm in (("off", None), ("on", "consensus"), ("off_again", None)):
        def steps(n=a.steps):
            for _ in range(n):
                for i in range(K):
                    msp.forward(x, outs[i], joint_mask=jm)
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

    # ---- 3: one frame set, graph replay against the eager joint-masked call
    p1 = make(1)
    p1.set_calibration(*calib_dev)
    assert p1.graph_replay
    x1 = x[:1].contiguous()
    res = p1.forward(x1)
    torch.cuda.synchronize()
    assert int(res[2][0]) == 1, "the probe's frame set must be a valid detection"
    want1 = res[0].clone()
    one_j = ones_j[:1].contiguous()
    forms = (("graph_plain", None), ("eager_joint_masked_all_ones", one_j), ("eager_joint_masked_consensus", "consensus"),
             ("graph_plain_again", None))
    times = {name: [] for name, _ in forms}
    for name, jm in forms:                                                       # (warm-up, and the first-call allocations)
        for _ in range(10):
            p1.forward(x1, res, joint_mask=jm)
    for _ in range(a.passes):
        for name, jm in forms:
            def calls(n=a.calls):
                for _ in range(n):
                    p1.forward(x1, res, joint_mask=jm)
            calls(3)
            times[name].append(timed(calls, 1)["ms"] / a.calls)
    torch.cuda.synchronize()
    rows = {name: dict(ms_per_frame_set=median(v), ms_min=min(v), ms_max=max(v)) for name, v in times.items()}
    rows["plain_bits_kept"] = bool(torch.equal(res[0], want1))
    for name in ("eager_joint_masked_all_ones", "eager_joint_masked_consensus", "graph_plain_again"):
        rows[name + "_minus_graph_ms"] = rows[name]["ms_per_frame_set"] - rows["graph_plain"]["ms_per_frame_set"]
    out["one_frame_set"] = dict(calls_per_pass=a.calls, **rows)

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
