// Subject identity across frame sets (csrc/tracks.h; the definition: include/jarvis_hip.h, jh_track_params).
//   track_subjects_kernel   one 64-lane wave per call: the frame sets are walked in order, the 8 x 8 (slot, detection)
//       pairs of a frame set are the 64 lanes, and every greedy step is one wave minimum over a 64-bit key
//   track_reset_kernel      the empty state
// The arithmetic is spelled with the _rn intrinsics, one IEEE rounding per operation of the definition, so that a
// float32 emulation of the header text gives the same bits.
#include "jh_common.h"
#include "argmax.h"
#include "tracks.h"

namespace jh {

__device__ __forceinline__ bool track_finite(float v) { return fabsf(v) < INFINITY; }   // (NaN compares false)

// lane = k * 8 + i: slot k, detection i.  The track of slot k lives in the registers of the slot's eight lanes, which
// all do the same arithmetic on it; detection i of the frame set lives in the registers of the eight lanes with that i
// (lanes 0 .. 7, slot 0, are where a shuffle fetches detection i from).  Lanes with k >= K or i >= K are never
// eligible and touch no memory.
//
// Per frame set: the key of a pair is  bits(d) << 6 | lane  when the pair is eligible (d >= 0: its bit pattern orders
// as it does) and all ones otherwise; the wave minimum (wave_min_u64, argmax.h: xor shuffles) is the
// smallest d, then the lowest k, then the lowest i -- a total order, no LDS atomics, so the result does not depend on
// timing.  The winner's row and column take the all-ones key and the step repeats, at most K times.  Births are
// resolved from two ballots (free slots, unmatched present detections) by every lane alike.
//
// The rows that only move (views, members, error) are copied by all 64 lanes after the walk, from the slots[] the
// walk wrote: the barrier between the two parts makes those writes visible to the whole (one-wave) workgroup.
__global__ __launch_bounds__(64) void track_subjects_kernel(
    const float* __restrict__ centers, const int* __restrict__ views, const int* __restrict__ members,
    const float* __restrict__ error, int T, int C, int K, int max_missed, int predict, int coast, float max_jump,
    TrackState* state, float* __restrict__ centers_out, int* __restrict__ views_out, int* __restrict__ members_out,
    float* __restrict__ error_out, int* __restrict__ ids, int* slots, int* __restrict__ missed_out,
    int* __restrict__ dropped) {
  const int lane = threadIdx.x, k = lane >> 3, i = lane & 7;
  const bool slot_ok = k < K, det_ok = i < K;
  const unsigned long long kNone = ~0ull;
  const float nan = __int_as_float(0x7fc00000);

  float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  int miss = -1, id = -1;
  if (slot_ok) {
    px = state->pos[k][0]; py = state->pos[k][1]; pz = state->pos[k][2];
    vx = state->vel[k][0]; vy = state->vel[k][1]; vz = state->vel[k][2];
    miss = state->missed[k];
    id = state->id[k];
  }
  int next_id = state->next_id;

  // detection i of the frame set at hand; the next one's is loaded a frame set ahead of its use
  float cx = nan, cy = nan, cz = nan;
  if (det_ok) {
    const float* c = centers + (size_t)i * 3;
    cx = c[0]; cy = c[1]; cz = c[2];
  }
  for (int t = 0; t < T; ++t) {
    float nx = nan, ny = nan, nz = nan;
    if (det_ok && t + 1 < T) {
      const float* c = centers + ((size_t)(t + 1) * K + i) * 3;
      nx = c[0]; ny = c[1]; nz = c[2];
    }
    // 1 - 3: prediction, presence, distance and gate
    const bool present = det_ok && track_finite(cx) && track_finite(cy) && track_finite(cz);
    const bool live = slot_ok && miss >= 0;
    const float m1 = (float)(miss + 1);
    float qx = px, qy = py, qz = pz;
    if (predict) {
      qx = __fadd_rn(px, __fmul_rn(vx, m1));
      qy = __fadd_rn(py, __fmul_rn(vy, m1));
      qz = __fadd_rn(pz, __fmul_rn(vz, m1));
    }
    const float dx = __fsub_rn(qx, cx), dy = __fsub_rn(qy, cy), dz = __fsub_rn(qz, cz);
    const float d = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    const bool eligible = live && present && d <= __fmul_rn(max_jump, m1);       // (a NaN d compares false)
    unsigned long long key = eligible ? ((unsigned long long)__float_as_uint(d) << 6) | (unsigned)lane : kNone;

    // 4: greedy match.  det: the detection slot k holds; slot: the slot detection i went to
    int det = -1, slot = -1;
    for (int r = 0; r < K; ++r) {
      const unsigned long long best = wave_min_u64(key);
      if (best == kNone) break;                  // (wave-uniform)
      const int wk = (int)(best & 63) >> 3, wi = (int)(best & 7);
      if (k == wk) { det = wi; key = kNone; }
      if (i == wi) { slot = wk; key = kNone; }
    }

    // 5, 6: the slot's track
    const int src = det < 0 ? 0 : det;
    const float mx = __shfl(cx, src), my = __shfl(cy, src), mz = __shfl(cz, src);
    if (det >= 0) {
      vx = predict ? __fdiv_rn(__fsub_rn(mx, px), m1) : 0.f;
      vy = predict ? __fdiv_rn(__fsub_rn(my, py), m1) : 0.f;
      vz = predict ? __fdiv_rn(__fsub_rn(mz, pz), m1) : 0.f;
      px = mx; py = my; pz = mz;
      miss = 0;
    } else if (live) {
      miss += 1;
      if (miss > max_missed) {
        miss = -1; id = -1;
        px = py = pz = vx = vy = vz = 0.f;
      }
    }

    // 7: births, in ascending detection, each into the lowest free slot (bit k * 8 of `fr`: slot k is free)
    unsigned long long fr = __ballot(slot_ok && i == 0 && miss < 0);
    const unsigned long long fresh = __ballot(k == 0 && present && slot < 0);
    int drop = 0, born = -1;
    for (int j = 0; j < K; ++j) {
      if (!((fresh >> j) & 1)) continue;
      if (fr) {
        const int s = (__ffsll((unsigned long long)fr) - 1) >> 3;
        fr &= fr - 1;
        if (s == k) { born = j; id = next_id; }
        ++next_id;
      } else {
        ++drop;
      }
    }
    const int bsrc = born < 0 ? 0 : born;
    const float bx = __shfl(cx, bsrc), by = __shfl(cy, bsrc), bz = __shfl(cz, bsrc);
    if (born >= 0) {
      px = bx; py = by; pz = bz;
      vx = vy = vz = 0.f;
      miss = 0;
      det = born;
    }

    // 8: row (t, k)
    if (slot_ok && i == 0) {
      const size_t row = (size_t)t * K + k;
      slots[row] = det;
      ids[row] = id;
      missed_out[row] = miss;
      float ox = nan, oy = nan, oz = nan;
      if (det >= 0) {
        ox = px; oy = py; oz = pz;               // (the detection's centre, bit for bit)
      } else if (miss >= 0 && coast) {
        const float fm = (float)miss;
        ox = predict ? __fadd_rn(px, __fmul_rn(vx, fm)) : px;
        oy = predict ? __fadd_rn(py, __fmul_rn(vy, fm)) : py;
        oz = predict ? __fadd_rn(pz, __fmul_rn(vz, fm)) : pz;
      }
      centers_out[row * 3 + 0] = ox;
      centers_out[row * 3 + 1] = oy;
      centers_out[row * 3 + 2] = oz;
    }
    if (lane == 0) dropped[t] = drop;
    cx = nx; cy = ny; cz = nz;
  }

  if (slot_ok && i == 0) {
    state->pos[k][0] = px; state->pos[k][1] = py; state->pos[k][2] = pz;
    state->vel[k][0] = vx; state->vel[k][1] = vy; state->vel[k][2] = vz;
    state->missed[k] = miss;
    state->id[k] = id;
  }
  if (lane == 0) state->next_id = next_id;
  if (views == nullptr) return;                  // (uniform: the three optional inputs come together)

  __syncthreads();
  const long long rows = (long long)T * K;
  for (long long r = lane; r < rows; r += 64) {
    const int s = slots[r];
    const long long from = r - r % K + s;
    views_out[r] = s >= 0 ? views[from] : 0;
    error_out[r] = s >= 0 ? error[from] : nan;
  }
  for (long long e = lane; e < rows * C; e += 64) {
    const long long r = e / C;
    const int s = slots[r];
    members_out[e] = s >= 0 ? members[(r - r % K + s) * C + e % C] : -1;
  }
}

__global__ __launch_bounds__(64) void track_reset_kernel(TrackState* state) {
  const int lane = threadIdx.x;
  if (lane < kMaxTracks) {
    for (int a = 0; a < 3; ++a) {
      state->pos[lane][a] = 0.f;
      state->vel[lane][a] = 0.f;
    }
    state->missed[lane] = -1;
    state->id[lane] = -1;
  }
  if (lane == 0) {
    state->next_id = 0;
    for (int a = 0; a < 3; ++a) state->reserved[a] = 0;
  }
}

// ------------------------------------------------------------------- host side
int tracks_check(const TrackParams& p) {
  JH_REQUIRE(p.max_subjects >= 1 && p.max_subjects <= kMaxTracks, "jh_track_params: max_subjects must be 1 .. 8");
  JH_REQUIRE(p.max_missed >= 0, "jh_track_params: max_missed must be >= 0");
  JH_REQUIRE(p.predict == 0 || p.predict == 1, "jh_track_params: predict must be 0 or 1");
  JH_REQUIRE(p.coast == 0 || p.coast == 1, "jh_track_params: coast must be 0 or 1");
  JH_REQUIRE(p.max_jump_mm > 0.f, "jh_track_params: max_jump_mm must be > 0 (+inf allowed, NaN refused)");
  return 0;
}

int launch_track_reset(TrackState* state, hipStream_t s) {
  JH_REQUIRE(state, "track reset: null state");
  hipLaunchKernelGGL(track_reset_kernel, dim3(1), dim3(kWave), 0, s, state);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_track_subjects(const float* centers, const int* views, const int* members, const float* error, int T, int C,
                          const TrackParams& p, TrackState* state, float* centers_out, int* views_out,
                          int* members_out, float* error_out, int* ids, int* slots, int* missed, int* dropped,
                          hipStream_t s) {
  if (tracks_check(p)) return 1;
  JH_REQUIRE(centers && state && centers_out && ids && slots && missed && dropped, "subject tracking: null pointer");
  const bool rows = views != nullptr;
  JH_REQUIRE((members != nullptr) == rows && (error != nullptr) == rows,
             "subject tracking: views, members and error are given together or not at all");
  JH_REQUIRE((views_out != nullptr) == rows && (members_out != nullptr) == rows && (error_out != nullptr) == rows,
             "subject tracking: views, members and error have their outputs exactly when they are given");
  JH_REQUIRE(T >= 1 && C >= 1, "subject tracking: at least one frame set and one camera");
  JH_REQUIRE((long long)T * p.max_subjects * C < (1ll << 31), "subject tracking: too many rows");
  hipLaunchKernelGGL(track_subjects_kernel, dim3(1), dim3(kWave), 0, s, centers, views, members, error, T, C,
                     p.max_subjects, p.max_missed, p.predict, p.coast, p.max_jump_mm, state, centers_out, views_out,
                     members_out, error_out, ids, slots, missed, dropped);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace jh
