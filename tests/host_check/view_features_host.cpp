// view_features_host.cpp -- XRSLAM_RESULT_FEATURES read the way a C++ host reads it (XRSLAMFeatures holds a std::vector, so ctypes
// cannot), next to the C getter XRSLAMAmdGetFeatures.  Drives the staged stream of player_loop_host.cpp and prints, after every image,
//   frame <timestamp> <key points of the C getter> <of which tracked> <XRSLAMFeatures::pos.size()>
//   R <x> <y>              one line per entry of XRSLAMFeatures::pos
//   G <x> <y> <track id>   one line per TRACKED entry of the C getter
// tests/test_view_stream_gpu.py requires the R and G coordinates to be the same text.
#include <cstdio>
#include <vector>

#include "../../include/XRSLAM.h"

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s slam.yaml device.yaml frames.bin\n", argv[0]);
        return 2;
    }
    // frames.bin: int32 n_frames, w, h, n_imu; double cam_t[n_frames]; double imu[n_imu][7]; uint8 frames[n_frames][h][w]
    FILE *f = std::fopen(argv[3], "rb");
    if (!f) return 2;
    int hdr[4];
    if (std::fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int n_frames = hdr[0], w = hdr[1], h = hdr[2], n_imu = hdr[3];
    std::vector<double> cam_t(n_frames), imu((size_t)7 * n_imu);
    std::vector<unsigned char> frames((size_t)n_frames * w * h);
    if (std::fread(cam_t.data(), sizeof(double), n_frames, f) != (size_t)n_frames) return 2;
    if (std::fread(imu.data(), sizeof(double), imu.size(), f) != imu.size()) return 2;
    if (std::fread(frames.data(), 1, frames.size(), f) != frames.size()) return 2;
    std::fclose(f);
    void *config = nullptr;
    if (XRSLAMCreate(argv[1], argv[2], "", "view_features_host", &config) != 1) {
        std::fprintf(stderr, "create failed: %s\n", XRSLAMAmdLastError());
        return 1;
    }
    XRSLAMFeatures before;
    before.pos.push_back({1.0, 2.0});
    XRSLAMGetResult(XRSLAM_RESULT_FEATURES, &before);
    std::printf("before %zu %d\n", before.pos.size(), XRSLAMAmdGetFeatures(nullptr, 0, nullptr));
    int k = 0;
    std::vector<XRSLAMAmdFeature> all;
    for (int i = 0; i < n_frames; ++i) {
        while (k < n_imu && imu[7 * (size_t)k] <= cam_t[i] + 1e-9) {
            const double *r = &imu[7 * (size_t)k];
            XRSLAMGyroscope gyro = {{r[1], r[2], r[3]}, r[0]};
            XRSLAMPushSensorData(XRSLAM_SENSOR_GYROSCOPE, &gyro);
            XRSLAMAcceleration acc = {{r[4], r[5], r[6]}, r[0]};
            XRSLAMPushSensorData(XRSLAM_SENSOR_ACCELERATION, &acc);
            ++k;
        }
        XRSLAMImage image;
        image.camera_id = 0;
        image.timeStamp = cam_t[i];
        image.ext = nullptr;
        image.data = &frames[(size_t)i * w * h];
        image.channel = 1;
        image.stride = w;
        XRSLAMPushSensorData(XRSLAM_SENSOR_CAMERA, &image);
        XRSLAMRunOneFrame();
        XRSLAMFeatures res;
        XRSLAMGetResult(XRSLAM_RESULT_FEATURES, &res);
        double t = 0.0;
        const int n = XRSLAMAmdGetFeatures(nullptr, 0, &t);
        all.resize((size_t)n);
        if (n > 0 && XRSLAMAmdGetFeatures(all.data(), n, &t) != n) return 3;
        int tracked = 0;
        for (const XRSLAMAmdFeature &g : all) tracked += g.track_id >= 0;
        std::printf("frame %.9f %d %d %zu\n", t, n, tracked, res.pos.size());
        for (const auto &p : res.pos) std::printf("R %.17g %.17g\n", p.x, p.y);
        for (const XRSLAMAmdFeature &g : all)
            if (g.track_id >= 0) std::printf("G %.17g %.17g %lld\n", g.x, g.y, g.track_id);
    }
    const char *err = XRSLAMAmdLastError();
    if (err && *err) {
        std::fprintf(stderr, "error: %s\n", err);
        return 1;
    }
    XRSLAMDestroy();
    return 0;
}
