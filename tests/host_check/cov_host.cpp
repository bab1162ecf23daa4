// Stand-alone check of the host-only pieces of the covariance path (xrslam_amd/csrc/host/covariance.hpp): the argument checks of
// xrhip_ba_covariance and the pose_ros permutation.  Built with -fsanitize=address,undefined by tests/test_cov_cpu.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../xrslam_amd/csrc/host/covariance.hpp"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                               \
        }                                                          \
    } while (0)

int main() {
    // the permutation: x y z, rotation about x y z out of dq dp dv dbg dba
    std::vector<double> state(225), ros(36);
    for (int i = 0; i < 15; ++i)
        for (int j = 0; j < 15; ++j) state[15 * i + j] = 100.0 * i + j;
    xrh::covariance_pose_ros(state.data(), ros.data());
    const int p[6] = {3, 4, 5, 0, 1, 2};
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) CHECK(ros[6 * i + j] == 100.0 * p[i] + p[j]);
    CHECK(ros[0] == state[15 * 3 + 3] && ros[6 * 3 + 3] == state[0] && ros[5] == state[15 * 3 + 2]);

    // the argument checks
    std::vector<uint8_t> fix(66, 0);
    fix[0] = XRHIP_FIX_POSE | XRHIP_FIX_MOTION;
    fix[1] = XRHIP_FIX_MOTION;
    std::vector<int> sel = {0, 5, 5};
    std::vector<double> blocks(3 * 225);
    int status = -9, na = -1;
    xrhip_cov_request rq = {3, sel.data(), blocks.data(), nullptr, &status, nullptr};
    CHECK(xrh::covariance_check_request(&rq, 6, fix.data(), &na) == nullptr && na == 0 + 6 + 4 * 15);
    CHECK(xrh::covariance_check_request(nullptr, 6, fix.data(), &na) != nullptr);
    xrhip_cov_request bad = rq;
    bad.status = nullptr;
    CHECK(xrh::covariance_check_request(&bad, 6, fix.data(), &na) != nullptr);
    bad = rq;
    bad.out_blocks = nullptr;
    CHECK(xrh::covariance_check_request(&bad, 6, fix.data(), &na) != nullptr);
    bad = rq;
    bad.n_sel = -1;
    CHECK(xrh::covariance_check_request(&bad, 6, fix.data(), &na) != nullptr);
    bad.n_sel = xrh::COV_MAX_SELECTED + 1;
    CHECK(xrh::covariance_check_request(&bad, 6, fix.data(), &na) != nullptr);
    sel[1] = 6;
    CHECK(std::strstr(xrh::covariance_check_request(&rq, 6, fix.data(), &na), "out of range") != nullptr);
    sel[1] = -1;
    CHECK(xrh::covariance_check_request(&rq, 6, fix.data(), &na) != nullptr);
    sel[1] = 5;
    CHECK(xrh::covariance_check_request(&rq, 0, fix.data(), &na) != nullptr);
    // the cap: 64 free frames fit, 65 do not (the message names the limit)
    std::vector<uint8_t> free_fix(66, 0);
    CHECK(xrh::covariance_check_request(&rq, 64, free_fix.data(), &na) == nullptr && na == 960);
    const char *why = xrh::covariance_check_request(&rq, 65, free_fix.data(), &na);
    CHECK(why && std::strstr(why, "960") && na == 975);
    xrhip_cov_request none = {0, nullptr, nullptr, nullptr, &status, nullptr};
    CHECK(xrh::covariance_check_request(&none, 6, fix.data(), nullptr) == nullptr);
    if (!fails) std::printf("cov_host OK\n");
    return fails ? 1 : 0;
}
