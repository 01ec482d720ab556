"""What reading every image through its own pointer costs, on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024,
23 keypoints, bbox 256), small models, one time batch resident in HBM.  Per format ('bgr', 'nv12'):
  contiguous  (a) forward_batch on one (T,C,...) tensor;
  images      (b) forward_images on the same images scattered over T * C separate allocations;
  gather      (c) what a caller had to do before forward_images: copy the scattered images into one tensor
                  (T * C device-to-device copies), then (a).
Per variant: wall time of the enqueued call(s) to completion (median of the passes, one synchronisation per pass) and,
from the jh_profile_* records, the kernel time of the two fused stems -- the resize stem of CenterDetect and the crop
stem of KeypointDetect, in launch order -- and of the whole batch.  The gather's copies are no kernels of the library:
they show in the wall time only.
python tools/frame_images_probe.py [--time-batch 32] [--passes 7] [--out profiles/frame_images_probe.json]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from jarvis_hybridnet_amd import _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "frame_images_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_images_probe: no GPU; a timing needs one")
    c, T = bench.CONFIGS["cfg3"], a.time_batch
    H, W, C = c["H"], c["W"], c["C"]
    cfg = NS(PARENT_DIR="/nonexistent", PROJECT_NAME="probe", DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
             CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center"]),
             KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
             HYBRIDNET=NS(NUM_CAMERAS=C, ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))
    calib = S.ring_calibration(C, W, H, c["focal"])
    dev = [t.cuda() for t in calib]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", c["J"], c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, c["J"], c["seeds"][2] + i)[0] for i in range(4)])
    bgr = (base.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).numpy()
    pick = torch.arange(T) % 4
    frames = {"bgr": (torch.from_numpy(bgr)[pick].cuda(), {}),
              "nv12": (torch.from_numpy(S.bgr_to_yuv420(bgr, "nv12"))[pick].cuda(), dict(frame_format="nv12"))}
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    out = dict(config="cfg3", time_batch=T, cameras=C, height=H, width=W, models="small", passes=a.passes, formats={})
    for fmt, (x, kw) in frames.items():
        # the same images, every one an allocation of its own, handed out in an order unrelated to (t, c)
        order = np.random.RandomState(0).permutation(T * C)
        scattered = [None] * (T * C)
        for i in order:
            scattered[i] = x[i // C, i % C].clone()
        images = [scattered[t * C:(t + 1) * C] for t in range(T)]
        staging = torch.empty_like(x)

        def contiguous():
            return pred.forward_batch(x, *dev, **kw)

        def per_image():
            return pred.forward_images(images, *dev, **kw)

        def gather():
            for t in range(T):
                for cam in range(C):
                    staging[t, cam].copy_(images[t][cam], non_blocking=True)
            return pred.forward_batch(staging, *dev, **kw)

        ref = [t.clone() for t in contiguous()]
        rows = {}
        for name, run in (("contiguous", contiguous), ("images", per_image), ("gather", gather)):
            for _ in range(a.warmup):
                run()
            res = run()
            torch.cuda.synchronize()
            assert all(torch.equal(p, q) for p, q in zip(res, ref)), (fmt, name)
            wall = []
            for _ in range(a.passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            recs = [N.profile(run) for _ in range(a.passes)]
            stems = np.array([[r[1] for r in rec if r[0].startswith("stem_conv")] for rec in recs])
            assert stems.shape[1] == 2, "expected the resize stem and the crop stem"
            rows[name] = dict(wall_ms=median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                              resize_stem_ms=median(list(stems[:, 0])), crop_stem_ms=median(list(stems[:, 1])),
                              batch_kernel_ms=median([sum(r[1] for r in rec) for rec in recs]),
                              valid_frames=int(res[2].sum()))
        for name, v in rows.items():
            for k in ("wall_ms", "resize_stem_ms", "crop_stem_ms", "batch_kernel_ms"):
                v[k.replace("_ms", "_vs_contiguous")] = v[k] / rows["contiguous"][k]
        rows["bytes_per_image"] = int(x[0, 0].numel())
        rows["copies_per_gather"] = T * C
        out["formats"][fmt] = rows
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
