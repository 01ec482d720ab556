"""What per-frame-set calibration costs and what it buys, on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024,
23 keypoints, bbox 256), small models, everything resident in HBM.
  1  forward_batch at T = 32 (uint8 BGR frames): one calibration shared by the batch (the path of every earlier
     commit, measured in this same run) against one calibration per frame set (two sets, alternating rows).  Wall time
     of the whole batch (median of the passes, one synchronisation per pass), without and with return_2d, and from the
     jh_profile_* records the lines of the three launches that read calibration: `triangulate`, `reproject_gather`
     (the coarse projection table + the gather) and `views2d_final`.
  2  The frame-set rate of analysis.analyze_frames at time_batch 1, 8 and 32 over synthetic samples of two calibration
     sets (dataset names alternate).  The samples are float32 (1,C,H,W,3) tensors already on the device, so the figure
     is the loop's conversion + predictor + read-back, not the host's DataLoader or the PCIe copy of a float64 frame.
python tools/calibration_frames_probe.py [--time-batch 32] [--passes 7] [--samples 64]
                                         [--out profiles/calibration_frames_probe.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import torch  # noqa: E402

import bench  # noqa: E402
from jarvis_hybridnet_amd import _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.analysis.analyze import analyze_frames  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402

LINES = ("triangulate", "reproject_gather", "views2d_final")


def median(v):
    return sorted(v)[len(v) // 2]


def translated(cam, d=(30.0, -20.0, 10.0)):
    """The calibration in a world frame translated by d (mm): the same projections, another centre."""
    out = cam.clone()
    out[:, 3] = cam[:, 3] - torch.einsum("k,ckj->cj", torch.tensor(d), cam[:, 0:3])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=os.path.join("profiles", "calibration_frames_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calibration_frames_probe: no GPU; a timing needs one")
    c, T = bench.CONFIGS["cfg3"], a.time_batch
    H, W, C, J = c["H"], c["W"], c["C"], c["J"]
    cfg = NS(PARENT_DIR="/nonexistent", PROJECT_NAME="probe", DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
             CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center"]),
             KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=J, BOUNDING_BOX_SIZE=c["bbox"]),
             HYBRIDNET=NS(NUM_CAMERAS=C, ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))
    calib = S.ring_calibration(C, W, H, c["focal"])
    set_a = [t.cuda() for t in calib]
    set_b = [translated(calib[0]).cuda(), set_a[1].clone(), set_a[2].clone()]
    per_frame = [torch.stack([(set_a, set_b)[t % 2][k] for t in range(T)]) for k in range(3)]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", J, c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, J, c["seeds"][2] + i)[0] for i in range(4)])      # (4,C,3,H,W)
    bgr = (base.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8)
    x = bgr[torch.arange(T) % 4].cuda()
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    out = dict(config="cfg3", time_batch=T, cameras=C, height=H, width=W, models="small", passes=a.passes)

    # ---- 1: forward_batch, shared against per-frame calibration
    rows = {}
    for name, cal in (("shared", set_a), ("per_frame", per_frame)):
        row = {}
        for key, kw in (("wall_ms", {}), ("wall_2d_ms", dict(return_2d=True))):
            def run():
                return pred.forward_batch(x, *cal, **kw)
            for _ in range(a.warmup):
                run()
            wall = []
            for _ in range(a.passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            row[key] = median(wall)
            row[key + "_min"], row[key + "_max"] = min(wall), max(wall)
            row["valid_frames"] = int(res[2].sum())
        recs = [N.profile(lambda: pred.forward_batch(x, *cal, return_2d=True)) for _ in range(a.passes)]
        row["batch_kernel_ms"] = median([sum(r[1] for r in rec) for rec in recs])
        for line in LINES:
            row[line + "_ms"] = median([sum(r[1] for r in rec if r[0] == line) for rec in recs])
        row["frames_per_s"] = T * C / (row["wall_ms"] * 1e-3)
        rows[name] = row
    for k in ("wall_ms", "wall_2d_ms", "batch_kernel_ms") + tuple(n + "_ms" for n in LINES):
        rows["per_frame"][k.replace("_ms", "_vs_shared")] = rows["per_frame"][k] / rows["shared"][k]
    out["forward_batch"] = rows

    # ---- 2: analyze_frames at time_batch 1, 8, 32 (samples resident on the device)
    imgs = [base[i].permute(0, 2, 3, 1).contiguous().cuda().unsqueeze(0) for i in range(4)]          # (1,C,H,W,3) fp32
    kp = torch.zeros((1, J, 3), dtype=torch.float64)
    samples = [[imgs[i % 4], kp, None, None, None, None, None, None, [("rigA", "rigB")[i % 2]], ["Frame_%04d.jpg" % i]]
               for i in range(a.samples)]
    tools = {name: NS(cameraMatrices=s[0], intrinsicMatrices=s[1], distortionCoefficients=s[2])
             for name, s in (("rigA", set_a), ("rigB", set_b))}
    rates = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tb in (1, 8, 32):
            analyze_frames(pred, samples[:max(tb, 4)], tools, os.path.join(tmp, "warm%d" % tb), J, time_batch=tb)
            wall = []
            for p in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seen, done = analyze_frames(pred, samples, tools, os.path.join(tmp, "t%d_%d" % (tb, p)), J,
                                            time_batch=tb)
                wall.append(time.perf_counter() - t0)
            rates[str(tb)] = dict(frame_sets=seen, predicted=done, seconds=median(wall),
                                  frame_sets_per_s=seen / median(wall))
    for tb in ("8", "32"):
        rates[tb]["vs_time_batch_1"] = rates[tb]["frame_sets_per_s"] / rates["1"]["frame_sets_per_s"]
    out["analyze_frames"] = dict(samples=a.samples, calibration_sets=2, resident="device, float32", rates=rates)

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
