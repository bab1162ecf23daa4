// covariance.hpp -- the host-only pieces of the covariance path: the argument checks of xrhip_ba_covariance and the
// permutation that turns the pose part of a 15 x 15 state block into nav_msgs/Odometry's order.  No device types: the stand-alone
// check tests/host_check/cov_host.cpp runs them under the sanitizers.
#pragma once
#include <cstdint>

#include "../../../include/xrslam_hip.h"

namespace xrh {

constexpr int COV_MAX_FREE_DOFS = 15 * 64;   // order of the largest reduced system xrhip_ba_covariance factors
constexpr int COV_MAX_SELECTED = 1024;

// -> nullptr when the request is acceptable for a problem of n_frames frames with the given fix bits (*na: its free frame dofs), else
// what is wrong with it
inline const char *covariance_check_request(const xrhip_cov_request *req, int n_frames, const uint8_t *frame_fix, int *na) {
    if (!req || !req->status) return "null request or status";
    if (req->n_sel < 0 || req->n_sel > COV_MAX_SELECTED) return "n_sel outside 0..1024";
    if (req->n_sel > 0 && (!req->sel_frames || !req->out_blocks)) return "sel_frames / out_blocks missing";
    if (n_frames <= 0 || !frame_fix) return "frames missing";
    for (int k = 0; k < req->n_sel; ++k)
        if (req->sel_frames[k] < 0 || req->sel_frames[k] >= n_frames) return "sel_frames index out of range";
    int n = 0;
    for (int f = 0; f < n_frames; ++f) n += ((frame_fix[f] & XRHIP_FIX_POSE) ? 0 : 6) + ((frame_fix[f] & XRHIP_FIX_MOTION) ? 0 : 9);
    if (na) *na = n;
    if (n > COV_MAX_FREE_DOFS) return "more free frame dofs than the limit of 960 (15 x 64)";
    return nullptr;
}

// pose_ros [6][6] = the pose part of state [15][15] (dq dp ...) in the order x y z, rotation about x y z: p = 3 4 5 0 1 2
inline void covariance_pose_ros(const double *state225, double *pose_ros36) {
    static const int p[6] = {3, 4, 5, 0, 1, 2};
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) pose_ros36[6 * i + j] = state225[15 * p[i] + p[j]];
}

}   // namespace xrh
