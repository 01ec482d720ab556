"""What per-camera tone tables (jh_predictor_set_tone) cost against the same call without them, on one GPU at BASELINE
configs[2] (12 cameras 1280 x 1024, 23 keypoints, bbox 256), small models, frames resident in HBM.  Forms, all of the
same seeded frame sets:
  bgr        uint8 BGR                                               3    bytes per pixel
  nv12       tight NV12, frame_format='nv12'                         1.5
  rggb       SensorSurface(H, W, 'rggb')                             1
  mono12p    SensorSurface(H, W, 'mono', bits=12, container='packed')  1.5
The tables are ToneTables.from_curve with a different black level, white-balance gain and gamma per camera.  Per form,
tables off and on ALTERNATING within this one process (off, on, off, on ...: drift hits both alike):
  streams_sets_per_s   `streams` predictors x one time batch each in flight (MultiStreamPredictor), wall clock;
  replay_ms            one frame set (T = 1) under graph replay, wall clock per call;
  resize_stem_ms / crop_stem_ms   the two fused stems' own kernel times at the time batch (jh_profile_* records).
Medians of the passes; `spread` is (max - min) / median of the passes of a figure.
python tools/tone_probe.py [--time-batch 32] [--passes 5] [--out profiles/r14_tone_probe.json]"""
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
from jarvis_hybridnet_amd import SensorSurface, ToneTables, _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def stat(v):
    m = median(v)
    return dict(median=m, spread=(max(v) - min(v)) / m if m else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--batches", type=int, default=6, help="time batches per timed multi-stream pass")
    ap.add_argument("--replays", type=int, default=30, help="T = 1 calls per timed replay pass")
    ap.add_argument("--out", default=os.path.join("profiles", "r14_tone_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tone_probe: no GPU; a timing needs one")
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
    bgr = (base.permute(0, 1, 3, 4, 2)[..., [2, 1, 0]] * 255).round().to(torch.uint8).numpy()      # (4,C,H,W,3)
    g = np.random.default_rng(14)
    L = dict(rggb=SensorSurface(H, W, "rggb"), mono12p=SensorSurface(H, W, "mono", bits=12, container="packed"))
    host = {
        "bgr": (bgr, {}),
        "nv12": (S.pack_yuv420(*S.bgr_to_yuv(bgr), "nv12"), dict(frame_format="nv12")),
        "rggb": (S.pack_sensor_surface(S.mosaic(bgr, "rggb"), L["rggb"]), dict(frame_layout=L["rggb"])),
        "mono12p": (S.pack_sensor_surface(S.widen(S.mosaic(bgr, "mono"), 4, g), L["mono12p"]),
                    dict(frame_layout=L["mono12p"])),
    }
    cam = np.arange(C)
    tone = ToneTables.from_curve(C, black=2.0 + cam % 5, white=250.0 - cam % 3,
                                 gain=np.stack([1.0 + 0.01 * (cam % 7), np.ones(C), 1.0 - 0.01 * (cam % 5)], 1),
                                 gamma=1.0 + 0.02 * (cam % 6))
    pick = torch.arange(T) % 4
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    out = dict(config="cfg3", time_batch=T, cameras=C, height=H, width=W, models="small", passes=a.passes,
               streams=a.streams, batches=a.batches, replays=a.replays, forms={})
    for name, (frames, kw) in host.items():
        x = torch.from_numpy(frames)[pick].cuda()
        x1 = x[:1].contiguous()
        msp = pred.native_streams(H, W, T, a.streams)
        msp.set_calibration(*dev)
        nat, nat1 = pred.native(H, W, time_batch=T), pred.native(H, W, time_batch=1)
        assert nat1.graph_replay

        def streams_pass():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.batches):
                msp.forward(x, **kw)
            msp.synchronize()
            return T * a.batches / (time.perf_counter() - t0)

        def replay_pass():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                pred.forward_batch(x1, *dev, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.replays * 1e3

        def stems_pass():
            rec = N.profile(lambda: pred.forward_batch(x, *dev, **kw))
            stems = [r[1] for r in rec if r[0].startswith("stem_conv")]
            assert len(stems) == 2, "expected the resize stem and the crop stem"
            return stems

        figs = {s: dict(streams_sets_per_s=[], replay_ms=[], resize_stem_ms=[], crop_stem_ms=[]) for s in ("off", "on")}
        points = {}
        for p in range(a.warmup + a.passes):
            for state in ("off", "on"):
                pred.set_tone(tone if state == "on" else None)
                res = pred.forward_batch(x, *dev, **kw)                  # (plans and buffers of this state)
                points[state], valid = res[0].clone(), int(res[2].sum())
                assert valid == T, "a timing of invalid frame sets is no timing"
                pred.forward_batch(x1, *dev, **kw)                       # (this state's recording: the later calls replay)
                records = nat1.graph_records
                vals = dict(streams_sets_per_s=streams_pass(), replay_ms=replay_pass())
                assert nat1.graph_records == records, "the timed T = 1 calls were not replays"
                vals["resize_stem_ms"], vals["crop_stem_ms"] = stems_pass()
                if p >= a.warmup:
                    for k, v in vals.items():
                        figs[state][k].append(v)
        assert not torch.equal(points["off"], points["on"]), "the tables changed nothing"
        form = dict(bytes_per_frame_set=int(frames[0].nbytes))
        for state in ("off", "on"):
            form[state] = {k: stat(v) for k, v in figs[state].items()}
        form["on_vs_off"] = {k: form["on"][k]["median"] / form["off"][k]["median"] for k in figs["off"]}
        out["forms"][name] = form
        del x, x1
        assert nat is pred.native(H, W, time_batch=T)
    pred.set_tone(None)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
