"""Validation-set analysis: the second caller of the hot path (mirrors
jarvis/analysis/analyze.py:22-96).

`analyze_frames` is the reference's loop over validation frame sets -- predict every
frame set, keep the ones the network detected, write `frame_names.csv`,
`points_HybridNet.csv` and `points_GroundTruth.csv` with the same numpy.savetxt calls
(hence byte-identical files for identical predictions).  Project management and the
Dataset3D loader are outside the hot path: `analyze_validation_data`
keeps the reference's signature but takes the configuration and the dataset from the
caller instead of constructing them from a project name.
"""
import os
import time

import numpy as np
from numpy import savetxt

from ..prediction.jarvis3D import JarvisPredictor3D
from ..utils.reprojection import load_reprojection_tools


def analyze_frames(predictor, samples, reproTools, output_dir, num_joints, progress_bar=None,
                   num_frame_sets=None, frame_layout=None, time_batch=1):
    """samples: iterable of batch-1 collated Dataset3D analysis samples
    `[imgs (1,C,H,W,3), keypoints3D (1,J,3), ..., dataset_name [str], file_name [str]]`
    (dataset3D.py:248-258 behind a DataLoader(batch_size=1), analyze.py:46-51).
    frame_layout: a YuvSurface -- imgs is (1,C,image_stride) uint8, one described YUV 4:2:0 surface per camera
    (JarvisPredictor3D.forward_surface); a SensorSurface likewise (one raw sensor image per camera).
    time_batch: T > 1 runs T consecutive samples through ONE predictor call (JarvisPredictor3D.forward_batch with
    per-frame-set calibration: every sample keeps the ReprojectionTool of its own dataset_name, so a group may mix
    calibration sets).  Each sample is converted exactly as with time_batch 1, then the T frame sets and their T
    calibrations are stacked; the valid rows are appended in sample order.  A last group of fewer than T samples is
    padded with repeats of its last sample and the padded rows are dropped.  The files are those of time_batch 1
    whenever a frame set's result does not depend on the time batch it runs in: bit for bit for T < 8 (DESIGN.md
    section 1: time batches below 8 share one arithmetic); T >= 8 is the other class.  1: one call per sample, as the
    reference.
    Returns (number of frame sets seen, number predicted)."""
    from .. import _native as N
    N.check_layout(frame_layout)
    if int(time_batch) != 1:
        return _analyze_frames_batched(predictor, samples, reproTools, output_dir, num_joints, progress_bar,
                                       num_frame_sets, frame_layout, int(time_batch))
    pointsNet, pointsGT, filenames = [], [], []
    seen = 0
    for item, sample in enumerate(samples):
        seen += 1
        if progress_bar is not None and num_frame_sets:
            progress_bar.progress(float(item + 1) / num_frame_sets)
        keypoints3D = sample[1][0].numpy()
        imgs_orig = sample[0][0]
        dataset_name = sample[-2][0]
        reproTool = reproTools[dataset_name]
        file_name = sample[-1][0]
        calib = (reproTool.cameraMatrices.cuda(), reproTool.intrinsicMatrices.cuda(),
                 reproTool.distortionCoefficients.cuda())
        if frame_layout is not None:
            points3D_net, _ = predictor.forward_surface(imgs_orig.cuda(), frame_layout, *calib)
        else:
            imgs = imgs_orig.cuda().float().permute(0, 3, 1, 2)          # analyze.py:66
            points3D_net, _ = predictor(imgs.contiguous(), *calib)
        if points3D_net is not None:
            pointsNet.append(points3D_net[0].cpu().detach().numpy())
            pointsGT.append(keypoints3D)
            filenames.append(file_name)
    os.makedirs(output_dir, exist_ok=True)
    savetxt(os.path.join(output_dir, "frame_names.csv"), np.array(filenames), delimiter=",", fmt="%s")
    savetxt(os.path.join(output_dir, "points_HybridNet.csv"),
            np.array(pointsNet).reshape((-1, num_joints * 3)), delimiter=",")
    savetxt(os.path.join(output_dir, "points_GroundTruth.csv"),
            np.array(pointsGT).reshape((-1, num_joints * 3)), delimiter=",")
    return seen, len(pointsNet)


def _analyze_frames_batched(predictor, samples, reproTools, output_dir, num_joints, progress_bar, num_frame_sets,
                            frame_layout, T):
    """analyze_frames for time_batch = T > 1 (see there): groups of T samples, one forward_batch per group."""
    import torch
    if T < 1:
        raise ValueError("time_batch must be a positive integer, got %d" % T)
    pointsNet, pointsGT, filenames = [], [], []
    group = []                      # (frames, (cam, intr, dist), keypoints3D, file_name) of the samples not yet run
    seen = 0

    def run_group():
        n = len(group)
        rows = group + [group[-1]] * (T - n)                          # (padding: repeats of the last sample)
        imgs = torch.stack([r[0] for r in rows])
        calib = tuple(torch.stack([r[1][k] for r in rows]) for k in range(3))
        kw = {} if frame_layout is None else {"frame_layout": frame_layout}
        points, _, valid = predictor.forward_batch(imgs, *calib, **kw)
        points, valid = points.cpu().detach().numpy(), valid.cpu()
        for i in range(n):                                            # (padded rows never reach a file)
            if int(valid[i]) != 0:
                pointsNet.append(points[i])
                pointsGT.append(rows[i][2])
                filenames.append(rows[i][3])
        del group[:]

    for item, sample in enumerate(samples):
        seen += 1
        if progress_bar is not None and num_frame_sets:
            progress_bar.progress(float(item + 1) / num_frame_sets)
        keypoints3D = sample[1][0].numpy()
        imgs_orig = sample[0][0]
        reproTool = reproTools[sample[-2][0]]
        file_name = sample[-1][0]
        calib = (reproTool.cameraMatrices.cuda(), reproTool.intrinsicMatrices.cuda(),
                 reproTool.distortionCoefficients.cuda())
        if frame_layout is not None:
            imgs = imgs_orig.cuda()
        else:
            imgs = imgs_orig.cuda().float().permute(0, 3, 1, 2).contiguous()     # analyze.py:66, as time_batch 1
        group.append((imgs, calib, keypoints3D, file_name))
        if len(group) == T:
            run_group()
    if group:
        run_group()
    os.makedirs(output_dir, exist_ok=True)
    savetxt(os.path.join(output_dir, "frame_names.csv"), np.array(filenames), delimiter=",", fmt="%s")
    savetxt(os.path.join(output_dir, "points_HybridNet.csv"),
            np.array(pointsNet).reshape((-1, num_joints * 3)), delimiter=",")
    savetxt(os.path.join(output_dir, "points_GroundTruth.csv"),
            np.array(pointsGT).reshape((-1, num_joints * 3)), delimiter=",")
    return seen, len(pointsNet)


def analyze_validation_data(project_name=None, weights_center="latest", weights_hybridnet="latest",
                            cameras_to_use=None, progress_bar=None, *, cfg=None, dataset=None,
                            output_root=None, reproTools=None, time_batch=1):
    """analyze.py:22-96 with the project manager and Dataset3D supplied by the caller:
    cfg = the project's configuration, dataset = a Dataset3D(cfg, set='val',
    analysisMode=True)-shaped sequence.  time_batch: frame sets per predictor call (analyze_frames; the loader
    still delivers one sample at a time).  Returns the output directory."""
    if cfg is None or dataset is None:
        raise NotImplementedError(
            "project management and Dataset3D are outside this package (SURVEY section 2): pass "
            "cfg= and dataset= (project %r)" % (project_name,))
    from torch.utils.data import DataLoader
    root = output_root if output_root is not None else os.path.join(
        cfg.PARENT_DIR, getattr(cfg, "PROJECTS_ROOT_PATH", "projects"), str(project_name), "analysis")
    output_dir = os.path.join(root, "Validation_Predictions_" + time.strftime("%Y%m%d-%H%M%S"))
    os.makedirs(output_dir)
    predictor = JarvisPredictor3D(cfg, weights_center, weights_hybridnet)
    if reproTools is None:
        reproTools = load_reprojection_tools(cfg, cameras_to_use=cameras_to_use)
    loader = DataLoader(dataset, batch_size=1, shuffle=False,
                        num_workers=getattr(cfg, "DATALOADER_NUM_WORKERS", 0), pin_memory=True)
    seen, done = analyze_frames(predictor, loader, reproTools, output_dir,
                                cfg.KEYPOINTDETECT.NUM_JOINTS, progress_bar, len(dataset), time_batch=time_batch)
    if done != seen:
        print("Network could not detect instance in %d frameSets. Those were not included in the "
              "output files!" % (seen - done))
    return output_dir
