"""What reading frames through a YuvSurface description costs against the fixed NV12 format, on one GPU at BASELINE
configs[2] (12 cameras 1280 x 1024, 23 keypoints, bbox 256), small models, one time batch resident in HBM.  Variants:
  nv12            frame_format='nv12' (the reference: the kernel of the fixed format);
  surface_tight   the same bytes through YuvSurface(H, W, 'nv12');
  surface_pitched pitch 1536, BT.709 (the same planes in a pitched layout; other constants).
Per variant: the kernel time (jh_profile_* records, median of the passes) of the two fused stems -- the resize stem
of CenterDetect and the crop stem of KeypointDetect, in launch order -- and of the whole batch.
python tools/yuv_surface_probe.py [--time-batch 32] [--passes 7] [--out profiles/yuv_surface_probe.json]"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from jarvis_hybridnet_amd import YuvSurface, _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "yuv_surface_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("yuv_surface_probe: no GPU; a timing needs one")
    c, T = bench.CONFIGS["cfg3"], a.time_batch
    H, W = c["H"], c["W"]
    cfg = NS(PARENT_DIR="/nonexistent", PROJECT_NAME="probe", DATASET=NS(DATASET_ROOT_DIR="x", MEAN=S.MEAN, STD=S.STD),
             CENTERDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=1, IMAGE_SIZE=c["center"]),
             KEYPOINTDETECT=NS(MODEL_SIZE="small", NUM_JOINTS=c["J"], BOUNDING_BOX_SIZE=c["bbox"]),
             HYBRIDNET=NS(NUM_CAMERAS=c["C"], ROI_CUBE_SIZE=c["roi"], GRID_SPACING=c["spacing"]))
    calib = S.ring_calibration(c["C"], W, H, c["focal"])
    dev = [t.cuda() for t in calib]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", c["J"], c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, c["J"], c["seeds"][2] + i)[0] for i in range(4)])
    bgr = (base.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).numpy()
    planes = S.bgr_to_yuv(bgr, "bt601", "limited")
    pick = torch.arange(T) % 4
    tight = YuvSurface(H, W, "nv12")
    pitched = YuvSurface(H, W, "nv12", matrix="bt709", y_pitch=1536, c_pitch=1536)
    nv12 = torch.from_numpy(S.pack_yuv420(*planes, "nv12"))[pick].cuda()                     # (T,C,3H/2,W)
    variants = {
        "nv12": (nv12, dict(frame_format="nv12")),
        "surface_tight": (nv12.reshape(T, c["C"], -1), dict(frame_layout=tight)),
        "surface_pitched": (torch.from_numpy(S.pack_yuv_surface(*S.bgr_to_yuv(bgr, "bt709", "limited"), pitched))[pick].cuda(),
                            dict(frame_layout=pitched)),
    }
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    out = dict(config="cfg3", time_batch=T, cameras=c["C"], height=H, width=W, models="small", passes=a.passes,
               variants={})
    for name, (x, kw) in variants.items():
        def run():
            return pred.forward_batch(x, *dev, **kw)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        valid = int(run()[2].sum())
        recs = [N.profile(run) for _ in range(a.passes)]
        stems = np.array([[r[1] for r in rec if r[0].startswith("stem_conv")] for rec in recs])
        assert stems.shape[1] == 2, "expected the resize stem and the crop stem"
        out["variants"][name] = dict(
            bytes_per_image=int(x.shape[-1] if x.dim() == 3 else x.shape[-2] * x.shape[-1]), valid_frames=valid,
            resize_stem_ms=median(list(stems[:, 0])), crop_stem_ms=median(list(stems[:, 1])),
            batch_kernel_ms=median([sum(r[1] for r in rec) for rec in recs]), launches=len(recs[0]))
    ref = out["variants"]["nv12"]
    for name, v in out["variants"].items():
        for k in ("resize_stem_ms", "crop_stem_ms", "batch_kernel_ms"):
            v[k.replace("_ms", "_vs_nv12")] = v[k] / ref[k]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
