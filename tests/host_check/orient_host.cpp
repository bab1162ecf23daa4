// The host side of the frame orientation, stand-alone (its own main, no GPU code, never loaded into Python; built with
// -fsanitize=address,undefined by tests/test_orient_host.py): xrslam_amd/csrc/host/pixel_format.hpp's orientation_from_exif,
// orient_plane and orient_intrinsics -- what XRSLAMAmdOrientationFromExif, the host turn of a build without the device kernel and
// XRSLAMAmdOrientIntrinsics compute.  Prints one line per result for the test to hold against tests/orient_model.py:
//   E exif o
//   P o sw sh byte...                       a small plane turned (exactly sized heap blocks: a wrong index is the sanitizer's)
//   I case o fx fy cx cy R0 .. R8           (%.17g)
#include <cstdio>
#include <memory>

#include "../../xrslam_amd/csrc/host/pixel_format.hpp"

int main() {
    for (int e = -1; e <= 10; ++e) std::printf("E %d %d\n", e, xrh::orientation_from_exif(e));
    const int sizes[3][2] = {{5, 3}, {4, 4}, {1, 7}};
    for (const auto &sz : sizes) {
        const int sw = sz[0], sh = sz[1];
        std::unique_ptr<uint8_t[]> src(new uint8_t[sw * sh]), dst(new uint8_t[sw * sh]), back(new uint8_t[sw * sh]);
        for (int i = 0; i < sw * sh; ++i) src[i] = (uint8_t)(17 * i + 3);
        for (int o = 0; o < 8; ++o) {
            xrh::orient_plane(dst.get(), src.get(), sw, sh, o);
            std::printf("P %d %d %d", o, sw, sh);
            for (int i = 0; i < sw * sh; ++i) std::printf(" %d", dst[i]);
            std::printf("\n");
            const int inv = (o & 4) ? o : (4 - o) & 3;
            xrh::orient_plane(back.get(), dst.get(), (o & 1) ? sh : sw, (o & 1) ? sw : sh, inv);
            for (int i = 0; i < sw * sh; ++i)
                if (back[i] != src[i]) {
                    std::printf("orient_plane: orientation %d is not undone by %d\n", o, inv);
                    return 1;
                }
        }
    }
    // case 0: the whole frame (geo null); 1: a crop of a larger frame, scaled; 2: an anisotropic crop with an odd origin
    const double K[4] = {458.654, 457.296, 367.215, 248.375};
    const xrhip_frame_geometry geos[2] = {{1920, 1080, 114, 0, 1692, 1080}, {1300, 1000, 3, 5, 1111, 977}};
    for (int c = 0; c < 3; ++c)
        for (int o = 0; o < 8; ++o) {
            double out[4], R[9];
            xrh::orient_intrinsics(K, c ? &geos[c - 1] : nullptr, o, 752, 480, out, R);
            std::printf("I %d %d %.17g %.17g %.17g %.17g", c, o, out[0], out[1], out[2], out[3]);
            for (int i = 0; i < 9; ++i) std::printf(" %.17g", R[i]);
            std::printf("\n");
        }
    std::printf("ok\n");
    return 0;
}
