// Per-joint robust triangulation (include/jarvis_hip.h: jh_joints3d_params, jh_op_joint_peaks_refine,
// jh_op_triangulate_joints, jh_predictor_triangulate_joints): every joint's 3D point from the cameras' own 2D
// keypoints -- the arg-max of the heat map, optionally refined to sub-pixel position by the centroid of a small
// window --, with the cameras that disagree left out by a consensus over two-view triangulations.  Kernels and
// launchers: joints3d.hip; the only reader of the parameters' ranges: joints3d_check.
#pragma once
#include "jh_common.h"

namespace jh {

constexpr int kMaxRefineRadius = 3;

struct Joints3dParams {
  int min_views, refine_radius;
  float min_conf, max_error_px;
};

// the ranges of include/jarvis_hip.h; 0, or 1 with the error set (host arithmetic only)
int joints3d_check(const Joints3dParams& p);

// heat [N][Hh][Wh][Jp], idx [N][J] flat arg-max indices (y * Wh + x) -> offsets [N][J][2] = (ox, oy) in heat-map pixels
int launch_joint_peaks_refine(const float* heat, const int* idx, float* offsets, int N, int Hh, int Wh, int J, int Jp,
                              int radius, hipStream_t s);
// The partials of launch_joint_argmax_all (csrc/views2d.h) over the T * C heat maps heat [T*C][Hh][Hh][Jp] + crop
// centres [T][C][2], validity [T] and mask [T][C] (or nullptr) -> obs [T][C][J][3] = (u, v, w): the full-frame pixel of
// views2d's points2D plus twice the sub-pixel offset, and views2d's conf2D; (NaN, NaN, 0) for a camera that is not
// used.  radius 0: the heat map is not read.
int launch_joint_observations(const float* pmax, const int* pidx, const float* heat, const int* center_hm,
                              const int* valid, const unsigned char* mask, float* obs, int T, int C, int J, int Jp,
                              int Hh, int hw, int radius, hipStream_t s);
// obs [T][C][J][3] -> points [T][J][3], views [T][J], members [T][J][C] bytes, error [T][J]
int launch_joints3d(const float* obs, const Calib& cal, float* points, int* views, unsigned char* members,
                    float* error, int T, int C, int J, int min_views, float min_conf, float max_error_px,
                    hipStream_t s);

}  // namespace jh
