// The voxel gather of the 3D stage: every camera's 2D heat maps sampled into the cube around the centre (kernels:
// reproject.hip).
#pragma once
#include "jh_common.h"

namespace jh {

// Calib (jh_common.h): the calibration, shared by all frames or one per frame.
// Per-frame camera masks -- `mask`, here and below: [T][C] bytes on the device, nonzero = the camera
// takes part in frame t; nullptr = all cameras.  The masked forms of the kernels that sum over cameras are kernels of
// their own (repro_gather_masked_kernel, repro_cube_masked_kernel; centers.hip: triangulate_masked_kernel) that share
// their bodies with the plain kernels through a template parameter: the plain kernels keep their names, signatures and
// code.
// launch_reproject under a mask: frame t sums its unmasked cameras in camera order and divides by their number (IEEE
// division; a frame without any camera gets an all-zero volume); at most 64 cameras then.
int launch_reproject(const Calib& cal, const int* center3d, const int* center_hm, const float* heat, float2* coarse,
                     float* vol, int* idx_out, int T, int C, int G, float spacing, int hs, int Jp, int heat_pad,
                     int div255, const unsigned char* mask, hipStream_t s, const HeatLayout* layout = nullptr,
                     bool coarse_ready = false);
// The first half of launch_reproject on its own: the coarse (u, v) field of T frames x C cameras, [T][C][(G/2)^3].  It
// depends on the calibration and the centres alone, so a caller may launch it as soon as those are known and hand the
// field to launch_reproject / launch_reproject_joint_masked with coarse_ready = true (the same launch, the same bits).
int launch_repro_coarse(const Calib& cal, const int* center3d, const int* center_hm, float2* coarse, int T, int C, int G,
                        float spacing, int hs, hipStream_t s);
// The box of stored heat-map pixels the gather can read, per image: image n = t * cam_n + l is camera
// cam0 + l of frame t, box[n] = (x0, y0, x1, y1) inclusive.  From the min / max of (u, v) over the camera's coarse
// field: the x2 trilinear upsampling with edge clamp forms convex combinations only, so every fine (u, v) lies in the
// coarse hull up to the rounding of the interpolation, for which the box takes the one pixel of margin of the cube
// gather's own boxes:  [trunc(min / 2) - 1 + heat_pad - 1, trunc(max / 2) - 1 + heat_pad + 1], clipped to the map.
// A frame that is not valid (valid[t] == 0; valid may be nullptr) and a camera the mask leaves out get the full map.
int launch_repro_box(const float2* coarse, const int* valid, const unsigned char* mask, int4* box, int T, int C,
                     int cam0, int cam_n, int G, int hs, int heat_pad, hipStream_t s);
// Per-joint camera masks -- joint_mask: [T][J][C] bytes on the device, nonzero = camera c counts for
// joint j of frame t.  With a(t,c) the camera mask (1 without one), the effective set of joint j is
// e(t,j,c) = a(t,c) && joint_mask[t][j][c]; an empty set falls back to a(t,.), and so do the padding channels.  One
// launch turns (mask, joint_mask) into the workspace `js` -- sets [T][C] 64-bit channel sets, ncam [T][Jp] counts; eff
// [T][J][C] bytes and cnt [T][J] optional copies for a caller to read -- and the voxel-row gather (a kernel of its own
// on the shared body; there is no joint-masked cube form) sums every channel over its own cameras in camera order and
// divides by its own count (IEEE division; no camera at all: 0).  At most 64 cameras and 64 channels.
// (JointSets: jh_common.h)
int launch_reproject_joint_masked(const Calib& cal, const int* center3d, const int* center_hm, const float* heat,
                                  float2* coarse, float* vol, int* idx_out, int T, int C, int G, float spacing, int hs,
                                  int J, int Jp, int heat_pad, int div255, const unsigned char* mask,
                                  const unsigned char* joint_mask, const JointSets& js, hipStream_t s,
                                  const HeatLayout* layout = nullptr, bool coarse_ready = false);

}  // namespace jh
