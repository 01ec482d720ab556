"""What the pixel-surface form costs, on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024, 23 keypoints, bbox 256),
small models.  Resident frames, `--streams` MultiStreamPredictor streams of one time batch each, the variants
ALTERNATING inside each of `--passes` passes; medians over the passes:
  bgr            the uint8 BGR form                                           3 bytes per pixel
  rgb24          PixelSurface.packed('rgb') over the SAME bytes: any gap to bgr is the form's overhead
  bgra_word      PixelSurface.packed('bgra'), frames at a 4-aligned base
  bgra_bytes     the same description and bytes at base + 1
  yuyv_word / yuyv_bytes   PixelSurface.yuv_packed('yuyv') likewise               2
  yuv422p        PixelSurface.from_pix_fmt('yuv422p')                          2
  planar_rgb     PixelSurface.planar()                                         3
(`*_word` / `*_bytes` are the two ALIGNMENTS of one buffer.  The recorded run was made with a fetch that took one 4-byte
load per pixel from a base that is a multiple of 4 and three byte loads otherwise, so the two alignments were the two
variants, with no switch in the library; the word load did not pay -- DESIGN.md 3.15e -- and was deleted, so on the tree
as it stands both alignments run the byte loads and the pair shows that the alignment of a base does not matter.)
spread: the 10th to 90th percentile of the *_bytes variant's passes, relative to its median; word_gain:
median(*_word) / median(*_bytes) - 1.
Then the shipped driver, predict3D_frames from host memory (numpy frame sets, `--streams` streams of one time batch
each), for bgr, rgb24, bgra, yuyv and nv12 in one run, in frame sets/s.
python tools/pixel_surface_probe.py [--time-batch 32] [--passes 7] [--out profiles/r13_pixel_surface_probe.json]"""
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
from jarvis_hybridnet_amd import PixelSurface, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd.prediction._ingest import release_ingest_buffers  # noqa: E402
from jarvis_hybridnet_amd.prediction.jarvis3D import JarvisPredictor3D  # noqa: E402
from jarvis_hybridnet_amd.prediction.predict3D import predict3D_frames  # noqa: E402


def yuv_planes(bgr, s):
    """uint8 BGR -> the (Y, U, V) planes of the description `s`: BT.601 limited in float32, chroma taken at every
    (2^ys, 2^xs)-th pixel (timing data: the content only has to give valid frames)."""
    x = np.asarray(bgr, np.float32)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)  # noqa: E731
    y = q(16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b)
    u = q(128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b)[..., ::1 << s.ys[1], ::1 << s.xs[1]]
    v = q(128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b)[..., ::1 << s.ys[1], ::1 << s.xs[1]]
    return y, np.ascontiguousarray(u), np.ascontiguousarray(v)


def at_base(host, pick, shift):
    """The picked frame sets on the device, the first byte `shift` bytes behind a 256-byte aligned address."""
    x = torch.from_numpy(host)[pick]
    pool = torch.empty((x.numel() + 16,), dtype=torch.uint8, device="cuda")
    assert pool.data_ptr() % 256 == 0
    v = pool[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 4 == shift % 4 and v.is_contiguous()
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="time batches per stream in one timed pass of a variant")
    ap.add_argument("--driver-batches", type=int, default=12, help="time batches of the timed driver run")
    ap.add_argument("--out", default=os.path.join("profiles", "r13_pixel_surface_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pixel_surface_probe: no GPU; a timing needs one")
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
    del base
    P = PixelSurface
    L = dict(rgb24=P.packed(H, W, "rgb"), bgra=P.packed(H, W, "bgra"), yuyv=P.yuv_packed(H, W, "yuyv"),
             yuv422p=P.from_pix_fmt(H, W, "yuv422p"), planar_rgb=P.planar(H, W))
    flat = bgr.reshape(4, c["C"], -1)
    host = {"bgr": (bgr, {}),
            "rgb24": (flat, dict(frame_layout=L["rgb24"])),            # the same bytes, read with red and blue exchanged
            "bgra": (S.pack_pixel_surface(bgr, L["bgra"], 0xFF), dict(frame_layout=L["bgra"])),
            "yuyv": (S.pack_pixel_surface(yuv_planes(bgr, L["yuyv"]), L["yuyv"]), dict(frame_layout=L["yuyv"])),
            "yuv422p": (S.pack_pixel_surface(yuv_planes(bgr, L["yuv422p"]), L["yuv422p"]),
                        dict(frame_layout=L["yuv422p"])),
            "planar_rgb": (S.pack_pixel_surface(bgr, L["planar_rgb"]), dict(frame_layout=L["planar_rgb"])),
            "nv12": (S.bgr_to_yuv420(bgr, "nv12"), dict(frame_format="nv12"))}
    pick = torch.arange(T) % 4
    pred = JarvisPredictor3D(cfg, sd_c, sd_h)
    msp = pred.native_streams(H, W, T, a.streams)
    msp.set_calibration(*dev)
    out = dict(config="cfg3", time_batch=T, cameras=c["C"], height=H, width=W, models="small", passes=a.passes,
               streams=a.streams, rounds=a.rounds, resident={}, driver={})
    # variant -> (device frames, how forward() is told what they are)
    variants = {"bgr": (at_base(host["bgr"][0], pick, 0), {}),
                "rgb24": (at_base(host["rgb24"][0], pick, 0), host["rgb24"][1]),
                "bgra_word": (at_base(host["bgra"][0], pick, 0), host["bgra"][1]),
                "bgra_bytes": (at_base(host["bgra"][0], pick, 1), host["bgra"][1]),
                "yuyv_word": (at_base(host["yuyv"][0], pick, 0), host["yuyv"][1]),
                "yuyv_bytes": (at_base(host["yuyv"][0], pick, 1), host["yuyv"][1]),
                "yuv422p": (at_base(host["yuv422p"][0], pick, 0), host["yuv422p"][1]),
                "planar_rgb": (at_base(host["planar_rgb"][0], pick, 0), host["planar_rgb"][1])}
    n_calls = a.streams * a.rounds

    def run(name):
        x, kw = variants[name]
        res = None
        for _ in range(n_calls):
            res = msp.forward(x, **kw)
        return res
    points = {}
    for name in variants:
        for _ in range(a.warmup):
            run(name)
        torch.cuda.synchronize()
        res = run(name)
        torch.cuda.synchronize()
        points[name], valid = res[0].clone(), int(res[2].sum())
        out["resident"][name] = dict(bytes_per_frame_set=int(variants[name][0][0].numel()), valid_frames=valid)
    # a timing of a wrong result is no timing: the two alignments of one buffer compute the same, and planar RGB holds
    # the pixels of the BGR frames
    assert torch.equal(points["bgra_word"], points["bgra_bytes"]) and torch.equal(points["bgra_word"], points["bgr"])
    assert torch.equal(points["yuyv_word"], points["yuyv_bytes"]) and torch.equal(points["planar_rgb"], points["bgr"])
    walls = {name: [] for name in variants}
    for _ in range(a.passes):
        for name in variants:                              # the variants alternate inside a pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name)
            torch.cuda.synchronize()
            walls[name].append(time.perf_counter() - t0)
    for name, w in walls.items():
        rate = np.array([n_calls * T / t for t in w])
        out["resident"][name].update(sets_per_s=float(np.median(rate)), passes_sets_per_s=[float(r) for r in rate],
                                     p10=float(np.percentile(rate, 10)), p90=float(np.percentile(rate, 90)))
    r = out["resident"]
    r["rgb24"]["vs_bgr"] = r["rgb24"]["sets_per_s"] / r["bgr"]["sets_per_s"]
    out["word_load"] = {}
    for k in ("bgra", "yuyv"):
        b, w = r[k + "_bytes"], r[k + "_word"]
        out["word_load"][k] = dict(word_gain=w["sets_per_s"] / b["sets_per_s"] - 1.0,
                                   spread=(b["p90"] - b["p10"]) / b["sets_per_s"])
    out["word_load"]["keep"] = any(v["word_gain"] > v["spread"] for v in out["word_load"].values())
    del variants, points
    torch.cuda.empty_cache()
    # the shipped driver from host memory: numpy frame sets staged through pinned buffers, `streams` predictors
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("bgr", "rgb24", "bgra", "yuyv", "nv12"):
            frames, kw = host[name]

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
            out["driver"][name] = dict(bytes_per_frame_set=int(frames[0].nbytes), sets_per_s=n / dt,
                                       gb_per_s=n * frames[0].nbytes / dt / 1e9)
            release_ingest_buffers(pred)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
