// Centre keyframes: the key rows of a time batch (host), the pointer table of their images, the scatter of their
// detections into the batch's detection buffer, and the fill of the rows in between (center_keys.h).
#include "center_keys.h"

namespace jh {

int center_key_rows(int T, int every, int n_rows, int* rows, int cap, int* count) {
  JH_REQUIRE(T >= 1, "centre keyframes: time_batch must be at least 1");
  JH_REQUIRE(every >= 1, "centre keyframes: every must be at least 1");
  JH_REQUIRE(n_rows >= 1 && n_rows <= T, "centre keyframes: n_rows must be 1 .. time_batch");
  const int n = center_key_count(every, n_rows);
  JH_REQUIRE(!rows || cap >= n, "centre keyframes: the rows buffer is smaller than the number of key rows");
  if (rows)
    for (int i = 0; i < n; ++i) rows[i] = center_key_row(i, every, n_rows);
  *count = n;
  return 0;
}

namespace {

__global__ void center_key_table_kernel(const void** __restrict__ table, int K, int C, int every, int n_rows,
                                        const void* base, long long image_bytes,
                                        const void* const* __restrict__ src_table) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= K * C) return;
  const size_t src = (size_t)center_key_row(n / C, every, n_rows) * C + n % C;
  table[n] = src_table ? src_table[src] : static_cast<const char*>(base) + (long long)src * image_bytes;
}

__global__ void center_key_scatter_kernel(const float* __restrict__ det_keys, float* __restrict__ det_all, int T, int C,
                                          int every, int n_rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * C * 3) return;
  const int t = i / (C * 3), rest = i % (C * 3);
  float v = 0.f;
  if (t < n_rows && center_key_is(t, every, n_rows))
    v = det_keys[(size_t)center_key_slot_of(t, every, n_rows) * C * 3 + rest];
  det_all[i] = v;
}

// One thread per row.  A row >= n_rows is row n_rows - 1 held.  fp32 with one rounding per operation, as written.
__global__ void center_key_fill_kernel(const float* __restrict__ c3f, const int* __restrict__ valid,
                                       float* __restrict__ centers, int* __restrict__ source, int T, int every,
                                       int n_rows) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float qnan = __int_as_float(0x7fc00000);
  const int r = t < n_rows ? t : n_rows - 1;
  float c[3] = {qnan, qnan, qnan};
  int src = -1;
  if (center_key_is(r, every, n_rows)) {
    if (valid[r] != 0) {
      for (int k = 0; k < 3; ++k) c[k] = c3f[r * 3 + k];
      src = r == t ? 0 : 2;
    }
  } else {
    const int ta = r / every * every;
    const int tb = center_key_row(ta / every + 1, every, n_rows);
    const bool va = valid[ta] != 0, vb = valid[tb] != 0;
    if (va && vb) {
      const float w = __fdiv_rn((float)(r - ta), (float)(tb - ta));
      for (int k = 0; k < 3; ++k) {
        const float a = c3f[ta * 3 + k], b = c3f[tb * 3 + k];
        c[k] = __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), w));
      }
      src = 1;
    } else if (va || vb) {
      const int h = va ? ta : tb;
      for (int k = 0; k < 3; ++k) c[k] = c3f[h * 3 + k];
      src = 2;
    }
  }
  for (int k = 0; k < 3; ++k) centers[t * 3 + k] = c[k];
  source[t] = src;
}

}  // namespace

int launch_center_key_table(const void** table, int K, int C, int every, int n_rows, const void* base,
                            long long image_bytes, const void* const* src_table, hipStream_t s) {
  JH_REQUIRE(table && K >= 1 && C >= 1 && every >= 1 && n_rows >= 1, "centre keyframes: key table");
  JH_REQUIRE(src_table || (base && image_bytes > 0), "centre keyframes: contiguous frames come with their image bytes");
  hipLaunchKernelGGL(center_key_table_kernel, dim3((K * C + 255) / 256), dim3(256), 0, s, table, K, C, every, n_rows,
                     base, image_bytes, src_table);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_center_key_scatter(const float* det_keys, float* det_all, int T, int C, int every, int n_rows,
                              hipStream_t s) {
  JH_REQUIRE(det_keys && det_all && every >= 1 && n_rows >= 1 && n_rows <= T, "centre keyframes: detection scatter");
  hipLaunchKernelGGL(center_key_scatter_kernel, dim3((T * C * 3 + 255) / 256), dim3(256), 0, s, det_keys, det_all, T, C,
                     every, n_rows);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_center_key_fill(const float* center3d_f, const int* valid, float* centers, int* source, int T, int every,
                           int n_rows, hipStream_t s) {
  JH_REQUIRE(center3d_f && valid && centers && source && every >= 1 && n_rows >= 1 && n_rows <= T,
             "centre keyframes: fill");
  hipLaunchKernelGGL(center_key_fill_kernel, dim3((T + 63) / 64), dim3(64), 0, s, center3d_f, valid, centers, source, T,
                     every, n_rows);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
