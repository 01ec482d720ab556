// Device functions of the weighted DLT triangulation and of the projection, shared by centers.hip (triangulation,
// caller-supplied centres), views2d.hip (2D views), subjects.hip (subject association) and joints3d.hip (per-joint
// robust triangulation): ONE definition, so that a point triangulated from a subset of the observations has the bits
// of the triangulation run on that subset, whichever kernel does it.
#pragma once
#include "jh_common.h"

namespace jh {

// ---------------------------------------------------------------- triangulation
// Smallest-eigenvalue eigenvector of a symmetric 4x4 matrix by cyclic Jacobi in
// fp64.  A^T A of the weighted DLT system shares its right singular vectors with
// A (reprojection.py:85-89 takes V[:, -1] of the SVD); fp64 keeps the squared
// condition number harmless.
__device__ inline void smallest_eigvec4(double a[4][4], double out[4]) {
  double v[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) off += a[p][q] * a[p][q];
    double diag = 0.0;
    for (int p = 0; p < 4; ++p) diag += a[p][p] * a[p][p];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - sn * akq;
          a[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - sn * aqk;
          a[q][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - sn * vkq;
          v[k][q] = sn * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  for (int i = 1; i < 4; ++i)
    if (a[i][i] < a[m][m]) m = i;
  for (int k = 0; k < 4; ++k) out[k] = v[k][m];
}

// depth: the homogeneous depth p[2] of the projection, where the caller needs to know the point lies in front of the camera
__device__ __forceinline__ void project_one(const float* M, const float* K, const float* D,
                                            float x, float y, float z, float* u, float* v, float* depth = nullptr) {
  float p[3];
#pragma unroll
  for (int col = 0; col < 3; ++col) {
    float a = __fmul_rn(x, M[0 * 3 + col]);
    a = __fmaf_rn(y, M[1 * 3 + col], a);
    a = __fmaf_rn(z, M[2 * 3 + col], a);
    a = __fmaf_rn(1.f, M[3 * 3 + col], a);
    p[col] = a;
  }
  if (depth) *depth = p[2];
  const float cx = K[6], cy = K[7], fx = K[0], fy = K[4];
  float uu = __fsub_rn(__fdiv_rn(p[0], p[2]), cx);
  float vv = __fsub_rn(__fdiv_rn(p[1], p[2]), cy);
  const float a1 = __fdiv_rn(uu, fx), a2 = __fdiv_rn(vv, fy);
  const float r2 = __fadd_rn(__fmul_rn(a1, a1), __fmul_rn(a2, a2));
  const float dd = __fadd_rn(1.f, __fmul_rn(__fadd_rn(D[0], __fmul_rn(D[1], r2)), r2));
  *u = __fadd_rn(__fmul_rn(uu, dd), cx);
  *v = __fadd_rn(__fmul_rn(vv, dd), cy);
}

// The weighted DLT of ReprojectionTool.reconstructPoint (reprojection.py:69-90) in three pieces, shared by the
// triangulation (triangulate_body), the cross-camera association (associate_subjects_kernel) and the per-joint
// triangulation (joints3d_kernel), so that a centre triangulated from a subset of the observations has the bits of the
// triangulation run on that subset:
//   dlt_rows   one observation d = (x, y, maxval) of the camera with calibration row (M, K, k1, k2) -> its two fp32
//              rows of A: the detection undistorted (single-step inverse, reprojection.py:71-78), u*P2 - P0 and
//              v*P2 - P1 with P = cameraMatrix^T, weighted by maxval / wdiv
//   dlt_term   element (i, j) of that observation's term of A^T A in fp64
//   dlt_solve  A^T A (16 doubles, the terms summed in camera order) -> the point: symmetrised, smallest eigenvector,
//              dehomogenised, rounded once to fp32
__device__ __forceinline__ void dlt_rows(const float* __restrict__ d, const float* __restrict__ M,
                                         const float* __restrict__ K, float k1, float k2, float sx2, float sy2,
                                         float wdiv, float* r0, float* r1) {
  const float cx = K[6], cy = K[7], fx = K[0], fy = K[4];
  const float wgt = __fdiv_rn(d[2], wdiv);
  float u = __fsub_rn(__fmul_rn(d[0], sx2), cx);
  float v = __fsub_rn(__fmul_rn(d[1], sy2), cy);
  const float a1 = __fdiv_rn(u, fx), a2 = __fdiv_rn(v, fy);
  const float r2 = __fadd_rn(__fmul_rn(a1, a1), __fmul_rn(a2, a2));
  const float dd = __fadd_rn(1.f, __fmul_rn(__fadd_rn(k1, __fmul_rn(k2, r2)), r2));
  u = __fadd_rn(__fdiv_rn(u, dd), cx);
  v = __fadd_rn(__fdiv_rn(v, dd), cy);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r0[k] = __fmul_rn(__fsub_rn(__fmul_rn(u, M[k * 3 + 2]), M[k * 3 + 0]), wgt);
    r1[k] = __fmul_rn(__fsub_rn(__fmul_rn(v, M[k * 3 + 2]), M[k * 3 + 1]), wgt);
  }
}

__device__ __forceinline__ double dlt_term(const float* r0, const float* r1, int i, int j) {
  return (double)r0[i] * (double)r0[j] + (double)r1[i] * (double)r1[j];
}

__device__ __forceinline__ void dlt_solve(const double* ata, float* point) {
  double a[4][4], x[4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) a[i][j] = 0.5 * (ata[i * 4 + j] + ata[j * 4 + i]);
  smallest_eigvec4(a, x);
  for (int k = 0; k < 3; ++k) point[k] = (float)(x[k] / x[3]);
}

// The pieces the two consensus kernels share (associate_subjects_kernel, joints3d_kernel): a hypothesis from two
// observations, the point of its members, and the distance that decides support and is reported as the error.
// A row below is the float[8] of one observation: r0[4], then r1[4] of dlt_rows.

// |(u, v) - (x, y)| in pixels, one fp32 rounding per operation (also the reprojection error of the 2D views)
__device__ __forceinline__ float pixel_distance(float u, float v, float x, float y) {
  const float dx = __fsub_rn(u, x), dy = __fsub_rn(v, y);
  return __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}

// the two-view DLT point of the rows ra, rb (summed in this order: the first camera, then the second)
__device__ __forceinline__ void dlt_pair_point(const float* ra, const float* rb, float* X) {
  double ata[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      s += dlt_term(ra, ra + 4, i, j);
      s += dlt_term(rb, rb + 4, i, j);
      ata[i * 4 + j] = s;
    }
  dlt_solve(ata, X);
}

// The DLT point of the members among the cameras 0 .. C-1: A^T A summed in camera order, then dlt_solve.
// row_of(c): the row of camera c's observation, or < 0 when the camera is not a member.  A non-member's term is
// evaluated on the row `fallback` (any row that has been written) and SELECTED as an exact 0.0, like a masked camera's
// in triangulate_body: s + 0.0 == s, so the point has the bits of the triangulation of the members alone.
template <class RowOf>
__device__ __forceinline__ void dlt_members_point(const float (*rows)[8], int C, int fallback, RowOf row_of,
                                                  float* point) {
  double ata[16];
  for (int e = 0; e < 16; ++e) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
      const int r = row_of(c);
      const int sl = r >= 0 ? r : fallback;
      const double term = dlt_term(rows[sl], rows[sl] + 4, e >> 2, e & 3);
      s += r >= 0 ? term : 0.0;
    }
    ata[e] = s;
  }
  dlt_solve(ata, point);
}

}  // namespace jh
