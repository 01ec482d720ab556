// Centre keyframes (jh_predictor_set_center_keyframes, include/jarvis_hip.h): CenterDetect on the key rows of a time
// batch, the rows in between take a centre interpolated between their two key rows (kernels: center_keys.hip).
//
// THE definition of the key rows, for the C ABI, the launch code and the kernels alike: of a batch of T rows whose
// first n_rows are real, with every = k >= 1, key slot i holds row center_key_row(i, k, n_rows) = min(i * k,
// n_rows - 1).  Slots 0 .. center_key_count(k, n_rows) - 1 are the distinct key rows {0, k, 2k, ... < n_rows} and
// n_rows - 1, ascending; the slots behind them -- a predictor has center_key_slots(T, k) of them, the count at
// n_rows = T -- repeat the last key: work is wasted, nothing is read out of range, and no launch size depends on n_rows.
#pragma once
#include "jh_common.h"

namespace jh {

__host__ __device__ inline int center_key_row(int slot, int every, int n_rows) {
  const long long r = (long long)slot * every;
  return r < n_rows - 1 ? (int)r : n_rows - 1;
}
// ceil((n_rows - 1) / every) + 1: the distinct key rows (1 for a single row)
__host__ __device__ inline int center_key_count(int every, int n_rows) {
  return (int)(((long long)n_rows - 1 + every - 1) / every) + 1;
}
inline int center_key_slots(int T, int every) { return center_key_count(every, T); }
// row t < n_rows is a key row
__host__ __device__ inline bool center_key_is(int t, int every, int n_rows) {
  return t % every == 0 || t == n_rows - 1;
}
// ... and the slot that holds it
__host__ __device__ inline int center_key_slot_of(int t, int every, int n_rows) {
  return t % every == 0 ? t / every : center_key_count(every, n_rows) - 1;
}

// The distinct key rows of (T, every, n_rows), ascending, into rows[0 .. cap) (rows may be nullptr: the count alone).
// Host arithmetic only.  *count: how many there are.  Non-zero with the error set for T < 1, every < 1, n_rows outside
// 1 .. T, or a cap below the count.
int center_key_rows(int T, int every, int n_rows, int* rows, int cap, int* count);

// table[i * C + c], i < K, c < C: the pointer of image (center_key_row(i), c) of a call -- base + (row * C + c) *
// image_bytes of contiguous frames, or src_table[row * C + c] of a per-image call (src_table != nullptr).
int launch_center_key_table(const void** table, int K, int C, int every, int n_rows, const void* base,
                            long long image_bytes, const void* const* src_table, hipStream_t s);
// det_keys [K][C][3], the detections of the key slots -> det_all [T][C][3]: row center_key_row(i) takes slot i, every
// other row is zero-filled (no detection: the triangulation finds it invalid).
int launch_center_key_scatter(const float* det_keys, float* det_all, int T, int C, int every, int n_rows, hipStream_t s);
// The fill.  center3d_f [T][3] / valid [T]: what the triangulation wrote (the key rows are read) -> centers [T][3],
// source [T] (0 detected, 1 interpolated, 2 held, -1 none); include/jarvis_hip.h has the arithmetic.
int launch_center_key_fill(const float* center3d_f, const int* valid, float* centers, int* source, int T, int every,
                           int n_rows, hipStream_t s);

}  // namespace jh
