"""What detect_subjects costs (jh_predictor_detect_subjects: the top local maxima of every camera's centre heat map,
grouped across cameras), on one GPU at BASELINE configs[2] (12 cameras 1280 x 1024, centre heat maps 128 x 128), small
models, fp32 frames resident in HBM as bench.py feeds them.  Median of the passes:
  a  the peak kernel against the arg-max kernel it stands in for: kernel time from the library's per-launch profile
     (jh_profile_*), at time_batch 32 (384 maps) with the library's default parameters and max_peaks 4;
  b  the association kernel at max_peaks 1, 2 and 4 (max_subjects 2), same profile, min_peak -inf so that every slot is
     filled and max_error_px +inf so that every camera supports: the most work the shape allows;
  c  detect_subjects as a whole against a stage-1 call (resize / stem, CenterDetect, arg-max) on the same frames, HIP
     events, at time_batch 1 and 32.
python tools/subjects_probe.py [--passes 7] [--calls 20] [--out profiles/r08_subjects_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import torch  # noqa: E402

import bench  # noqa: E402
from jarvis_hybridnet_amd import _native as N  # noqa: E402
from jarvis_hybridnet_amd import synthetic as S  # noqa: E402
from jarvis_hybridnet_amd._predictor import NativePredictor  # noqa: E402

INF = float("inf")


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return dict(ms=median(v), ms_min=min(v), ms_max=max(v))


def kernel_ms(fn, name, passes):
    """Per-launch profile time of the kernel `name` inside fn(), once per pass."""
    ms = []
    for _ in range(passes):
        rec = [r for r in N.profile(fn) if r[0] == name]
        assert len(rec) == 1, (name, len(rec))
        ms.append(rec[0][1])
    return spread(ms)


def event_ms(fn, calls, passes):
    """HIP-event time of `calls` calls of fn(), per call."""
    ms = []
    for _ in range(passes):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / calls)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed pass of part c")
    ap.add_argument("--out", default=os.path.join("profiles", "r08_subjects_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("subjects_probe: no GPU; a timing needs one")
    c = bench.CONFIGS["cfg3"]
    H, W, C, J = c["H"], c["W"], c["C"], c["J"]
    calib = S.ring_calibration(C, W, H, c["focal"])
    calib_dev = [t.cuda() for t in calib]
    sd_c = S.efficienttrack_weights("small", 1, c["seeds"][0])
    sd_h = S.hybridnet_weights("small", J, c["seeds"][1])
    base = torch.stack([S.blob_frames(calib, W, H, J, c["seeds"][2] + i)[0] for i in range(4)]).cuda()

    def make(T):
        pr = NativePredictor(sd_c, sd_h, num_cameras=C, num_joints=J, center_size=c["center"], bbox=c["bbox"],
                             roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=H, img_w=W, mean=S.MEAN,
                             std=S.STD, time_batch=T)
        pr.set_calibration(*calib_dev)
        return pr
    out = dict(config="cfg3", cameras=C, height=H, width=W, heat_map=c["center"] // 2, models="small",
               frames="fp32 RGB, resident", passes=a.passes)
    for T in (32, 1):
        pr = make(T)
        x = base[torch.arange(T, device="cuda") % 4].contiguous()
        fr = pr._describe(x)
        det = torch.empty((T, C, 3), device="cuda")
        default = N.subjects_params(2, max_peaks=4)
        full = {P: N.subjects_params(2, max_peaks=P, min_peak=-INF, max_error_px=INF) for P in (1, 2, 4)}
        subj = pr.detect_subjects(fr, default)          # (the first call allocates)
        pr.stage_center(x, det)
        torch.cuda.synchronize()
        row = dict(valid_first_subjects=int((subj.views[:, 0] > 0).sum()))
        if T == 32:
            row["center_argmax_kernel"] = kernel_ms(lambda: pr.stage_center(x, det), "center_argmax", a.passes)
            row["center_peaks_kernel"] = kernel_ms(lambda: pr.detect_subjects(fr, default), "center_peaks", a.passes)
            row["associate_kernel_default"] = kernel_ms(lambda: pr.detect_subjects(fr, default), "associate_subjects",
                                                        a.passes)
            for P, p in full.items():
                row["associate_kernel_full_P%d" % P] = kernel_ms(lambda p=p: pr.detect_subjects(fr, p),
                                                                "associate_subjects", a.passes)
        for _ in range(3):
            pr.stage_center(x, det)
            pr.detect_subjects(fr, default)
        row["stage_center_call"] = event_ms(lambda: pr.stage_center(x, det), a.calls, a.passes)
        row["detect_subjects_call"] = event_ms(lambda: pr.detect_subjects(fr, default), a.calls, a.passes)
        row["detect_subjects_call_full_P4"] = event_ms(lambda: pr.detect_subjects(fr, full[4]), a.calls, a.passes)
        row["detect_vs_stage_center"] = row["detect_subjects_call"]["ms"] / row["stage_center_call"]["ms"]
        out["time_batch_%d" % T] = row
        pr.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
