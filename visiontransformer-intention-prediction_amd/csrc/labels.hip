// Heuristic intention labels of heuristic_labeling.py:10-124 as driven by
// preprocess_intent_labels.py:41-57, for every annotation row of one or more logs in one launch.
//
// The reference filters and sorts the whole table once per row; here the rows arrive sorted by
// (track, timestamp_ns) with the track offsets, so a row's "future track" (:37) is the rows after
// it in its track and the row it is compared with is min(horizon, rows left) further on. One
// thread per row: it reads its own row, that one later row, and finds its track by bisecting the
// offsets. Everything is f64 in the reference's order of operations, compiled with floating-point
// contraction off so that no fused multiply-add moves a value across a threshold.
//
// Only the map-free branch is implemented: what the reference computes when av2 cannot be imported
// (AV2_MAP_AVAILABLE false, static_map None) -- no intersection context (:61-77, :83-84) and the
// lateral-displacement fallback (:118-122) instead of the lane polygons (:93-117).
#include "ivit_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LT = 256;
constexpr int OTHER = 7, KEEP_LANE = 0, TURN_LEFT = 1, TURN_RIGHT = 2, LEFT_CHANGE_LANE = 3, RIGHT_CHANGE_LANE = 4,
              STOPPING_STOPPED = 5, PARKED = 6;  // constants.py INTENTIONS_MAP

// z angle of scipy's Rotation.from_quat(q).as_euler('xyz') (extrinsic) away from gimbal lock, on the
// normalised quaternion; false for a zero norm (from_quat raises ValueError, :47-52).
IVIT_DEV bool quat_yaw(const double* __restrict__ q, double& yaw) {
  double x = q[0], y = q[1], z = q[2], w = q[3];
  const double n = sqrt(x * x + y * y + z * z + w * w);
  if (!(n > 0.0)) {
    yaw = 0.0;
    return false;
  }
  x /= n; y /= n; z /= n; w /= n;
  yaw = atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z));
  return true;
}

__global__ __launch_bounds__(LT) void intent_labels_kernel(const long* __restrict__ ts, const double* __restrict__ xy,
                                                           const double* __restrict__ quat,
                                                           const unsigned char* __restrict__ is_vehicle,
                                                           const long* __restrict__ track_off, long n, long n_tracks,
                                                           ivit_label_params p, int* __restrict__ intent,
                                                           double* __restrict__ yaw_out) {
  const long i = (long)blockIdx.x * LT + threadIdx.x;
  if (i >= n) return;
  double yaw0;
  const bool ok0 = quat_yaw(quat + 4 * i, yaw0);
  yaw_out[i] = yaw0;
  if (!is_vehicle[i]) {  // preprocess_intent_labels.py:42-49
    intent[i] = -1;
    return;
  }
  // the track that owns row i: the last t with track_off[t] <= i
  long lo = 0, hi = n_tracks;
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (track_off[mid] <= i) lo = mid; else hi = mid;
  }
  long end = track_off[lo + 1];
  if (end > n) end = n;              // never read past the table, whatever the offsets say
  const long left = end - 1 - i;     // rows after this one in its track
  const long used = left < (long)p.horizon_steps ? left : (long)p.horizon_steps;
  int label = OTHER;
  if (used >= (long)p.min_future_points && used > 0) {  // :37-38
    const long e = i + used;
    const double dx = xy[2 * e] - xy[2 * i], dy = xy[2 * e + 1] - xy[2 * i + 1];
    const double dist = sqrt(dx * dx + dy * dy);                      // :42-43
    const double elapsed = (double)(ts[e] - ts[i]) * 1e-9 + 1e-9;     // :44
    const double speed = dist / elapsed;                              // :45
    double yaw1;
    if (ok0 && quat_yaw(quat + 4 * e, yaw1)) {                        // :47-52
      const double dd = yaw1 - yaw0;
      const double dh = atan2(sin(dd), cos(dd));
      const double adh = fabs(dh);
      if (speed < p.stopped_speed) {                                  // :54-55
        label = dist < p.parked_max_disp ? PARKED : STOPPING_STOPPED;
      } else if (speed >= p.moving_speed) {
        if (dh > p.turn_heading) label = TURN_LEFT;                   // :80
        else if (dh < -p.turn_heading) label = TURN_RIGHT;            // :81
        else if (p.keep_heading < adh && adh < p.turn_heading)        // :87-88
          label = dh > 0.0 ? LEFT_CHANGE_LANE : RIGHT_CHANGE_LANE;
        else if (adh <= p.keep_heading) {                             // :90, :118-122
          const double hx = cos(yaw0), hy = sin(yaw0);
          const double along = dx * hx + dy * hy;
          const double lx = dx - along * hx, ly = dy - along * hy;
          if (sqrt(lx * lx + ly * ly) < p.keep_lane_max_lat) label = KEEP_LANE;
        }
      }
    }
  }
  intent[i] = label;
}

}  // namespace

extern "C" int ivit_intent_labels(const long* ts, const double* xy, const double* quat,
                                  const unsigned char* is_vehicle, const long* track_off, long n, long n_tracks,
                                  const ivit_label_params* params, int* intent, double* yaw, void* stream) {
  IVIT_CHECK_ARG(n >= 0 && n_tracks >= 0, "ivit_intent_labels: negative row or track count");
  if (n == 0) return 0;
  IVIT_CHECK_ARG(params != nullptr, "ivit_intent_labels: params is null");
  IVIT_CHECK_ARG(n_tracks >= 1 && n_tracks <= n, "ivit_intent_labels: %ld rows need 1..%ld tracks (got %ld)", n, n,
                 n_tracks);
  IVIT_CHECK_ARG(params->horizon_steps >= 0 && params->min_future_points >= 0,
                 "ivit_intent_labels: negative horizon_steps or min_future_points");
  IVIT_CHECK_ARG(n < 2147483647L * LT, "ivit_intent_labels: grid too large");
  hipLaunchKernelGGL(intent_labels_kernel, dim3(ivit_cdiv(n, LT)), dim3(LT), 0, ivit_stream(stream), ts, xy, quat,
                     is_vehicle, track_off, n, n_tracks, *params, intent, yaw);
  IVIT_LAUNCH_CHECK();
  return 0;
}
