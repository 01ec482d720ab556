"""The keypoint head's boxes on a benchmark workload: one time batch through the whole-path forward, the
boxes stage 2 wrote read back, and per image the part of the heat map inside its box and the workgroups of the window
head that compute something -- interior tiles laid from the box's first window plus edge workgroups, of the
tiles + edge of the launch grid.  The fraction to hold the head's measured time against.

    python tools/head_roi_probe.py [--config cfg3] [--model-size small] [-T 32] [--out profiles/head_roi_tiles_cfg3.tsv]
"""
import argparse
import ctypes
import os
import sys
sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from jarvis_hybridnet_amd import _native as N, synthetic as S  # noqa: E402
from jarvis_hybridnet_amd._predictor import NativePredictor  # noqa: E402
from tests import head_roi_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg3")
ap.add_argument("--model-size", default=None)
ap.add_argument("-T", type=int, default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
c = bench.CONFIGS[a.config]
a.model_size = a.model_size or c.get("size", "small")
T = a.T or c["time_batch"]
calib = S.ring_calibration(c["C"], c["W"], c["H"], c["focal"])
sd_c = S.efficienttrack_weights(a.model_size, 1, c["seeds"][0])
sd_h = S.hybridnet_weights(a.model_size, c["J"], c["seeds"][1])
pr = NativePredictor(sd_c, sd_h, num_cameras=c["C"], num_joints=c["J"], center_size=c["center"], bbox=c["bbox"],
                     roi_cube_size=c["roi"], grid_spacing=c["spacing"], img_h=c["H"], img_w=c["W"], mean=S.MEAN,
                     std=S.STD, time_batch=T, center_model=a.model_size, kp_model=a.model_size)
pr.set_calibration(*[t.cuda() for t in calib])
nd = min(T, 8)                                       # (the frame sets of bench.py and tools/launch_table.py)
base = torch.stack([S.blob_frames(calib, c["W"], c["H"], c["J"], c["seeds"][2] + i)[0] for i in range(nd)]).cuda()
fr = base[torch.arange(T, device="cuda") % nd].contiguous()
_, _, valid = pr.forward(fr)
box = torch.zeros((T, c["C"], 4), dtype=torch.int32, device="cuda")
boxed = ctypes.c_int32(-1)
N.check(N.lib().jh_predictor_debug_head_boxes(pr.handle, box.data_ptr(), ctypes.byref(boxed), N.stream()))
torch.cuda.synchronize()
box, valid = box.cpu().numpy(), valid.cpu().numpy()
Hh = c["bbox"] // 2
H = W = Hh // 2                                      # the head's input
tiles_all, edge_all = R.all_workgroups(H, W)
lines = []
area, wgs, tiles = [], [], []
for t in range(T):
    for cam in range(c["C"]):
        b = box[t, cam]
        nt, ne = R.workgroups(b, H, W) if boxed.value else (tiles_all, edge_all)
        area.append((b[2] - b[0] + 1) * (b[3] - b[1] + 1) / float(Hh * Hh))
        tiles.append(nt / float(tiles_all))
        wgs.append((nt + ne) / float(tiles_all + edge_all))
        lines.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (t, cam, valid[t], b[0], b[1], b[2], b[3], nt, ne))
head = ["# %s %s T=%d: head took its box: %d; heat map %d^2, %d tiles + %d edge workgroups per image"
        % (a.config, a.model_size, T, boxed.value, Hh, tiles_all, edge_all),
        "# box area / heat map: mean %.3f max %.3f; interior tiles that run: mean %.3f max %.3f; workgroups that run "
        "(tiles + edge): mean %.3f max %.3f" % (np.mean(area), np.max(area), np.mean(tiles), np.max(tiles), np.mean(wgs),
                                                np.max(wgs)),
        "t\tcam\tvalid\tx0\ty0\tx1\ty1\ttiles\tedge_wgs"]
text = "\n".join(head + lines)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
print("\n".join(head))
