// Subject identity across frame sets (include/jarvis_hip.h: jh_track_params, jh_track_state, jh_op_track_reset,
// jh_op_track_subjects): the detections of consecutive frame sets matched greedily, nearest first, against up to eight
// tracks that live in caller-owned device memory, so that slot k of frame set t and of t+1 is the same animal.
// Kernels and launchers: tracks.hip; the only reader of the parameters' ranges: tracks_check.
#pragma once
#include "jh_common.h"

namespace jh {

constexpr int kMaxTracks = 8;

struct TrackParams {
  int max_subjects, max_missed, predict, coast;
  float max_jump_mm;
};

// jh_track_state of include/jarvis_hip.h, field for field (api_features.hip asserts the size)
struct TrackState {
  float pos[kMaxTracks][3], vel[kMaxTracks][3];
  int missed[kMaxTracks], id[kMaxTracks];
  int next_id, reserved[3];
};

// the ranges of include/jarvis_hip.h; 0, or 1 with the error set (host arithmetic only)
int tracks_check(const TrackParams& p);

// every slot free, next_id 0, every float 0
int launch_track_reset(TrackState* state, hipStream_t s);
// centers [T][K][3], views [T][K], members [T][K][C], error [T][K] (the last three nullptr together, their outputs
// too) + state -> the same rows in slot order, ids / slots / missed [T][K], dropped [T], and the state after frame set
// T - 1.  One launch of one wave; nothing is allocated.
int launch_track_subjects(const float* centers, const int* views, const int* members, const float* error, int T, int C,
                          const TrackParams& p, TrackState* state, float* centers_out, int* views_out,
                          int* members_out, float* error_out, int* ids, int* slots, int* missed, int* dropped,
                          hipStream_t s);

}  // namespace jh
