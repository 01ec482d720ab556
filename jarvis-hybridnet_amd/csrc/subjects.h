// Several subjects in one frame set (include/jarvis_hip.h: jh_subjects_params, jh_op_center_peaks,
// jh_op_associate_subjects, jh_predictor_detect_subjects): the top-P local maxima of every camera's centre heat map in
// place of its one arg-max, and their grouping across cameras by reprojection consistency in place of the one
// triangulation.  Kernels and launchers: subjects.hip; the only reader of the parameters' ranges: subjects_check.
#pragma once
#include "jh_common.h"

namespace jh {

constexpr int kMaxPeaks = 8, kMaxSubjects = 8, kMaxNmsRadius = 16;

struct SubjectsParams {
  int max_subjects, max_peaks, nms_radius, min_views;
  float min_peak, max_error_px;
};

// the ranges of include/jarvis_hip.h; 0, or 1 with the error set (host arithmetic only)
int subjects_check(const SubjectsParams& p);

// Workspace of the peak kernel for N maps of Hh x Wh: 0 where a map fits the LDS (the kernel then touches no global
// scratch), otherwise the bytes of the global path (row maxima and the peak mask of every image).
size_t center_peaks_workspace(int N, int Hh, int Wh);
// heat [N][Hh][Wh][Cp], channel 0 -> peaks [N][max_peaks][3] = (x, y, value), count [N]
int launch_center_peaks(const float* heat, float* peaks, int* count, int N, int Hh, int Wh, int Cp, int max_peaks,
                        int nms_radius, float min_peak, void* workspace, hipStream_t s);
// peaks [T][C][P][3] -> centers [T][K][3], views [T][K], members [T][K][C], error [T][K]; mask [T][C] or nullptr;
// The work of a frame set grows with C^2 * P^2 per round (K rounds).
int launch_associate_subjects(const float* peaks, const Calib& cal, const unsigned char* mask, float* centers,
                              int* views, int* members, float* error, int T, int C, int P, int K, int min_views,
                              float max_error_px, float sx2, float sy2, float wdiv, hipStream_t s);

}  // namespace jh
