// Arg-max of the keypoint heat maps (csrc/views2d.hip): the 2D predictor's one-joint-per-block form, and for the
// per-camera 2D views of the 3D predictor (jh_predictor_views2d) the all-joint argmax in one pass over
// [N][Hh*Wh][Jp] channel-last heat maps and the kernels that merge its slices.
#pragma once
#include "jh_common.h"
#include "argmax.h"

namespace jh {

// heat [T][Hh][Wh][Jp] -> points [T][J][2] = (m % Hh, m / Wh) * 2 + center_hm - hw, conf [T][J] = min(max, 255) / 255
int launch_joint_argmax(const float* heat, const int* center_hm, int* points, float* conf, int T,
                        int J, int Jp, int Hh, int Wh, int hw, hipStream_t s);

// How the scan cuts a shape: threads per block, pixels per slice, slices per image.
struct ScanShape { int threads = 0, ppb = 0, slices = 0; };
ScanShape joint_argmax_all_shape(int N, int Hh, int Wh, int Jp);
// elements of each of the two partial arrays (max: float, index: int) the scan writes: [N][slices][Jp]
size_t joint_argmax_all_partials(int N, int Hh, int Wh, int Jp);
int launch_joint_argmax_all(const float* heat, float* pmax, int* pidx, int N, int Hh, int Wh, int J, int Jp,
                            hipStream_t s);
// partials -> idx / maxv [N][J] (the scan's own result, for the unit test)
int launch_joint_argmax_all_combine(const float* pmax, const int* pidx, int* idx, float* maxv, int N, int Hh,
                                    int Wh, int J, int Jp, hipStream_t s);
// partials + crop centres, validity, mask and 3D points of T frames -> the five outputs of jh_predictor_views2d
int launch_views2d_final(const float* pmax, const int* pidx, const int* center_hm, const int* valid,
                         const unsigned char* mask, const float* pts3d, const Calib& cal, int* points2d,
                         float* conf2d, float* reproj, float* err, unsigned char* used, int T, int C, int J, int Jp,
                         int Hh, int Wh, int hw, hipStream_t s);

// Device side of the scan, for the kernels that read its partials (views2d.hip: the 2D views; joints3d.hip: the
// observations of the joint triangulation): the merge of the slices, in the order of argmax_take (argmax.h).
// (max, index) of channel j of image n over its slices (the partials of launch_joint_argmax_all)
__device__ __forceinline__ void argmax_combine(const float* __restrict__ pmax, const int* __restrict__ pidx,
                                               int n, int slices, int Jp, int j, float* best, int* bi) {
  float b = -INFINITY;
  int i = 0x7fffffff;
  for (int k = 0; k < slices; ++k) {
    const size_t o = ((size_t)n * slices + k) * Jp + j;
    argmax_take(pmax[o], pidx[o], b, i);
  }
  *best = b;
  *bi = i;
}

}  // namespace jh
