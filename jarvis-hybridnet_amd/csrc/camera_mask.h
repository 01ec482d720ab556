// Per-frame camera masks: launchers of the masked forms of the three kernels that sum over
// cameras.  mask: [T][C] bytes on the device, nonzero = the camera takes part in frame t.  The masked forms are
// kernels of their own (triangulate_masked_kernel, repro_gather_masked_kernel, repro_cube_masked_kernel) that
// share their bodies with the plain kernels through a template parameter: the plain kernels keep their names,
// signatures and code.
// calib_fs, here as in the plain launchers (nets.h): the calibration's frame stride in cameras.
#pragma once
#include "jh_common.h"

namespace jh {

// As launch_triangulate; a masked camera adds an exact 0.0 to A^T A (selected, never multiplied: its detection
// may be NaN) and is not counted.  n_active[t]: unmasked cameras of frame t, n_detect[t]: those of them with
// maxval > 50 (valid[t] = n_detect[t] >= 2).  Crop centres are written for every camera.
int launch_triangulate_masked(const float* det, const float* cam, const float* intr, const float* dist, int calib_fs,
                              float* center3d_f, int* center3d_i, int* center_hm, int* valid, int T, int C,
                              float sx2, float sy2, float wdiv, int hw, int W, int H,
                              const unsigned char* mask, int* n_active, int* n_detect, hipStream_t s);

// As launch_reproject; frame t sums its unmasked cameras in camera order and divides by their number
// (IEEE division; a frame without any camera gets an all-zero volume).
int launch_reproject_masked(const float* cam, const float* intr, const float* dist, int calib_fs, const int* center3d,
                            const int* center_hm, const float* heat, float2* coarse, float* vol, int* idx_out,
                            int T, int C, int G, float spacing, int hs, int Jp, int heat_pad, int div255,
                            const unsigned char* mask, hipStream_t s, const HeatLayout* layout = nullptr);

}  // namespace jh
