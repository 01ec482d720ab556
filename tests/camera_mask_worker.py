"""Child process of tests/test_hip_camera_mask.py::test_masked_row_gather_in_a_child_process.  Environment knobs of
the native library are read once per process, so the voxel-row form of the masked gather at a geometry that takes the
cube form by default (JH_REPRO_CUBE=0) needs a fresh process.  Runs the masked predictor against the |S|-camera
predictor, NaN in the masked slots and all ones against no mask; prints one JSON line."""
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.test_hip_camera_mask import keep, predictor  # noqa: E402


def main(tag, mask):
    assert os.environ.get("JH_REPRO_CUBE") == "0"
    pred, c, inp = predictor(tag)
    S_idx = keep(mask)
    sub, _, _ = predictor(tag, cams=len(S_idx))
    calib = tuple(inp[k].cuda() for k in ("cam", "intr", "dist"))
    calib_s = tuple(inp[k][S_idx].contiguous().cuda() for k in ("cam", "intr", "dist"))
    imgs = inp["imgs"]
    got = pred(imgs.cuda(), *calib, camera_mask=mask)
    want = sub(imgs[S_idx].contiguous().cuda(), *calib_s)
    dirty = imgs.clone()
    dirty[[i for i, m in enumerate(mask) if not m]] = float("nan")
    nan = pred(dirty.cuda(), *calib, camera_mask=mask)
    ones = pred(imgs.cuda(), *calib, camera_mask=[1] * len(mask))
    none = pred(imgs.cuda(), *calib)
    torch.cuda.synchronize()
    eq = lambda a, b: bool(a[0] is not None and b[0] is not None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))  # noqa: E731
    print(json.dumps(dict(tag=tag, cameras=len(S_idx), subset_equal=eq(got, want), garbage_equal=eq(got, nan),
                          ones_equal=eq(ones, none),
                          points_mm=float((got[0] - want[0]).abs().max()) if got[0] is not None else None)))


if __name__ == "__main__":
    main(sys.argv[1], [int(ch) for ch in sys.argv[2]])
