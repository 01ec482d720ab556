// The soft-argmax tail of the V2V network, with and without the per-joint spread (kernels: softargmax.hip).
#pragma once
#include "jh_common.h"

namespace jh {

// The spread form of the soft-argmax tail (softargmax.hip): workspace and outputs of T frame sets.
// sums: softargmax_spread_sums(T, Jp) doubles with T * Jp 64-bit keys right behind them (`key`), one allocation;
// valid: [T] validity flags (rows of a frame set that is not valid are NaN) or nullptr = all valid;
// cov [T][J][6] (xx, xy, xz, yy, yz, zz; mm^2), peak [T][J][3] (mm), mass [T][J].
struct SoftargmaxSpread {
  double* sums = nullptr;
  unsigned long long* key = nullptr;
  const int* valid = nullptr;
  float *cov = nullptr, *peak = nullptr, *mass = nullptr;
};
size_t softargmax_spread_sums(int T, int Jp);
int launch_softargmax(const float* x, const int* center3d, double* partial, int* pmax,
                      float* points, float* conf, float* heatmap_final, int T, int J, int Jp,
                      int Gh, float spacing, float roi, hipStream_t s, const SoftargmaxSpread* spread = nullptr);

}  // namespace jh
