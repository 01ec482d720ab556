"""What raw sensor frames (SensorSurface: Mono8 / Bayer, demosaiced in the stems) cost and save against the other
uint8 inputs, on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024, 23 keypoints, bbox 256), small models.
Inputs, all of the same seeded frame sets:
  bgr    uint8 BGR (3 bytes per pixel);
  nv12   tight NV12, frame_format='nv12' (1.5);
  mono   SensorSurface(H, W, 'mono'), the green channel (1);
  rggb   SensorSurface(H, W, 'rggb'), the mosaic of the frames (1).
Per input, in one run: the forward on one time batch resident in HBM -- frame sets/s by wall clock (median of the
passes) and the kernel time of the two fused stems (jh_profile_* records; the crop stem is where the 3 x 3
neighbourhoods of a dense window overlap) -- and the shipped driver, predict3D_frames from host memory (numpy frame
sets, three streams), in frame sets/s.
python tools/sensor_surface_probe.py [--time-batch 32] [--passes 7] [--out profiles/sensor_surface_probe.json]"""
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
from jarvis_hybridnet_amd import SensorSurface, _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402
from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--driver-batches", type=int, default=12, help="time batches of the timed driver run")
    ap.add_argument("--out", default=os.path.join("profiles", "sensor_surface_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sensor_surface_probe: no GPU; a timing needs one")
    c, T = bench.CONFIGS["cfg3"], a.time_batch
    H, W = c["H"], c["W"]
    cfg = NS(PARENT_DIR="/nonexistent", PROJECT_NAME="probe", DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
             CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center"]),
             KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
             HYBRIDNET=NS(NUM_CAMERAS=c["C"], ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))
    cfg.KEYPOINT_NAMES = ["k%d" % i for i in range(c["J"])]
    calib = S.ring_calibration(c["C"], W, H, c["focal"])
    dev = [t.cuda() for t in calib]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", c["J"], c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, c["J"], c["seeds"][2] + i)[0] for i in range(4)])
    bgr = (base.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).numpy()      # (4,C,H,W,3)
    mono, rggb = SensorSurface(H, W, "mono"), SensorSurface(H, W, "rggb")
    host = {
        "bgr": (bgr, {}),
        "nv12": (S.bgr_to_yuv420(bgr, "nv12"), dict(frame_format="nv12")),
        "mono": (S.pack_sensor_surface(S.mosaic(bgr, "mono"), mono), dict(frame_layout=mono)),
        "rggb": (S.pack_sensor_surface(S.mosaic(bgr, "rggb"), rggb), dict(frame_layout=rggb)),
    }
    pick = torch.arange(T) % 4
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    out = dict(config="cfg3", time_batch=T, cameras=c["C"], height=H, width=W, models="small", passes=a.passes,
               streams=a.streams, inputs={})
    for name, (frames, kw) in host.items():
        x = torch.from_numpy(frames)[pick].cuda()

        def run():
            return pred.forward_batch(x, *dev, **kw)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        valid = int(run()[2].sum())
        walls = []
        for _ in range(a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        recs = [N.profile(run) for _ in range(a.passes)]
        stems = np.array([[r[1] for r in rec if r[0].startswith("stem_conv")] for rec in recs])
        assert stems.shape[1] == 2, "expected the resize stem and the crop stem"
        out["inputs"][name] = dict(
            bytes_per_frame_set=int(frames[0].nbytes), valid_frames=valid, forward_sets_per_s=T / median(walls),
            resize_stem_ms=median(list(stems[:, 0])), crop_stem_ms=median(list(stems[:, 1])),
            batch_kernel_ms=median([sum(r[1] for r in rec) for rec in recs]))
        del x
    # the shipped driver from host memory: numpy frame sets staged through pinned buffers, `streams` predictors
    with tempfile.TemporaryDirectory() as tmp:
        for name, (frames, kw) in host.items():
            def gen(n):
                return (frames[i % 4] for i in range(n))
            dkw = dict(time_batch=T, streams=a.streams, **kw)
            predict3D_frames(pred, gen(T * a.streams), *dev, cfg, tmp, **dkw)          # buffers, plans, graphs
            torch.cuda.synchronize()
            n = T * a.driver_batches
            t0 = time.perf_counter()
            done = predict3D_frames(pred, gen(n), *dev, cfg, tmp, **dkw)
            dt = time.perf_counter() - t0
            assert done == n
            out["inputs"][name]["driver_sets_per_s"] = n / dt
            out["inputs"][name]["driver_gb_per_s"] = n * frames[0].nbytes / dt / 1e9
            release_ingest_buffers(pred)
    ref = out["inputs"]["bgr"]
    for v in out["inputs"].values():
        for k in ("forward_sets_per_s", "driver_sets_per_s", "crop_stem_ms", "resize_stem_ms"):
            v[k + "_vs_bgr"] = v[k] / ref[k]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
