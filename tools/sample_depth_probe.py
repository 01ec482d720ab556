"""What samples wider than a byte cost against their 8-bit forms, on one GPU at BASELINE configs[2] (12 cameras
1280 x 1024, 23 keypoints, bbox 256), small models.  Inputs, all of the same seeded frame sets, in one run:
  mono8      SensorSurface(H, W, 'mono')                                   1    byte per pixel
  mono12     SensorSurface(H, W, 'mono', bits=12)             16-bit words 2
  mono12p    SensorSurface(H, W, 'mono', bits=12, container='packed')      1.5
  rggb8      SensorSurface(H, W, 'rggb')                                   1
  rggb12p    SensorSurface(H, W, 'rggb', bits=12, container='packed')      1.5
  nv12       tight NV12, frame_format='nv12'                               1.5
  p010       YuvSurface(H, W, 'nv12', bits=10, msb=True)                   3
The wide samples carry random low bits under the bytes of the 8-bit form, so every pair computes the same result.
Per input: the forward on one time batch resident in HBM -- frame sets/s by wall clock (median of the passes) and the
kernel time of the two fused stems (jh_profile_* records) -- and the shipped driver, predict3D_frames from host memory
(numpy frame sets, three streams of one time batch each), in frame sets/s.
python tools/sample_depth_probe.py [--time-batch 32] [--passes 7] [--out profiles/r12_sample_depth_probe.json]"""
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
from jarvis_hybridnet_amd import SensorSurface, YuvSurface, _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402
from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames  # noqa: E402

# the 8-bit form each input is measured against
PAIRS = {"mono12": "mono8", "mono12p": "mono8", "rggb12p": "rggb8", "p010": "nv12"}


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--driver-batches", type=int, default=12, help="time batches of the timed driver run")
    ap.add_argument("--out", default=os.path.join("profiles", "r12_sample_depth_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_depth_probe: no GPU; a timing needs one")
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
    g = np.random.default_rng(12)
    green, rggb = S.mosaic(bgr, "mono"), S.mosaic(bgr, "rggb")
    yuv = S.bgr_to_yuv(bgr)
    L = dict(mono8=SensorSurface(H, W, "mono"), mono12=SensorSurface(H, W, "mono", bits=12),
             mono12p=SensorSurface(H, W, "mono", bits=12, container="packed"), rggb8=SensorSurface(H, W, "rggb"),
             rggb12p=SensorSurface(H, W, "rggb", bits=12, container="packed"),
             p010=YuvSurface(H, W, "nv12", bits=10, msb=True))
    host = {
        "mono8": (S.pack_sensor_surface(green, L["mono8"]), dict(frame_layout=L["mono8"])),
        "mono12": (S.pack_sensor_surface(S.widen(green, 4, g), L["mono12"]), dict(frame_layout=L["mono12"])),
        "mono12p": (S.pack_sensor_surface(S.widen(green, 4, g), L["mono12p"]), dict(frame_layout=L["mono12p"])),
        "rggb8": (S.pack_sensor_surface(rggb, L["rggb8"]), dict(frame_layout=L["rggb8"])),
        "rggb12p": (S.pack_sensor_surface(S.widen(rggb, 4, g), L["rggb12p"]), dict(frame_layout=L["rggb12p"])),
        "nv12": (S.pack_yuv420(*yuv, "nv12"), dict(frame_format="nv12")),
        "p010": (S.pack_yuv_surface(*(S.widen(p, 8, g) for p in yuv), L["p010"]), dict(frame_layout=L["p010"])),
    }
    pick = torch.arange(T) % 4
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    out = dict(config="cfg3", time_batch=T, cameras=c["C"], height=H, width=W, models="small", passes=a.passes,
               streams=a.streams, inputs={})
    points = {}
    for name, (frames, kw) in host.items():
        x = torch.from_numpy(frames)[pick].cuda()

        def run():
            return pred.forward_batch(x, *dev, **kw)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        res = run()
        points[name], valid = res[0].clone(), int(res[2].sum())
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
    for wide, narrow in PAIRS.items():                 # a timing of a wrong result is no timing
        assert torch.equal(points[wide], points[narrow]), (wide, narrow)
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
    for wide, narrow in PAIRS.items():
        v, ref = out["inputs"][wide], out["inputs"][narrow]
        for k in ("forward_sets_per_s", "driver_sets_per_s", "crop_stem_ms", "resize_stem_ms"):
            v[k + "_vs_" + narrow] = v[k] / ref[k]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
