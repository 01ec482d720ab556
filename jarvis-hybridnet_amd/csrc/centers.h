// From a centre heat map to the 3D centre and the crop centres of every camera (kernels: centers.hip).
// `mask`, here and elsewhere: the per-frame camera mask, [T][C] bytes on the device, nonzero = the camera takes part in
// frame t; nullptr = all cameras.
#pragma once
#include "jh_common.h"

namespace jh {

// heat [N][Hh][Wh][Cp], channel 0 -> det [N][3] = (x, y, maxval); the lowest index wins among equal maxima
int launch_center_argmax(const float* heat, float* det, int N, int Hh, int Wh, int Cp,
                         hipStream_t s);
int launch_center2d(const float* det, int* center_hm, int* valid, int T, float sx, float sy, int hw,
                    int W, int H, hipStream_t s);
// Under a mask (n_active and n_detect are then required) a masked camera adds an exact 0.0 to A^T A (selected, never
// multiplied: its detection may be NaN) and is not counted.  n_active[t]: unmasked cameras of frame t, n_detect[t]:
// those of them with maxval > 50 (valid[t] = n_detect[t] >= 2).  Crop centres are written for every camera.
// The masked form is a kernel of its own (triangulate_masked_kernel) that shares its body with the plain kernel
// through a template parameter: the plain kernel keeps its name, signature and code.
int launch_triangulate(const float* det, const Calib& cal, float* center3d_f, int* center3d_i, int* center_hm,
                       int* valid, int T, int C, float sx2, float sy2, float wdiv, int hw, int W, int H,
                       const unsigned char* mask, int* n_active, int* n_detect, hipStream_t s);
// Caller-supplied 3D centres (T,3) in place of the triangulation: the buffers launch_triangulate writes, det excepted
// (centers.hip: centers_kernel).
int launch_centers(const float* centers, const Calib& cal, float* center3d_f, int* center3d_i, int* center_hm,
                   int* valid, int T, int C, int hw, int W, int H, const unsigned char* mask, int* n_active,
                   int* n_detect, hipStream_t s);
int launch_project_points(const float* pts, const float* cam, const float* intr, const float* dist,
                          float* uv, int P, int C, hipStream_t s);

}  // namespace jh
