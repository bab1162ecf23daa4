// xrslam_player.cpp -- headless EuRoC player over XRSLAM.h.
//
// The GUI-free equivalent of the loop in xrslam-pc/player/src/main.cpp:116-169: reads an ASL/EuRoC directory,
// feeds gyroscope / accelerometer / camera events in the order of the reference's asynchronous reader, undistorts
// every image like EurocDatasetReader::read_image, writes the body poses in TUM format and, when the ground truth
// is present, reports the ATE.  It links against libxrslam_hip.so only through XRSLAM.h.
//
//   xrslam-player --slam configs/euroc_slam.yaml --device configs/euroc_sensor.yaml --euroc <dir>/mav0
//                 [--out traj.tum] [--bootstrap-frames N] [--max-frames N] [--no-undistort | --host-undistort] [--pipelined]
//                 [--push-color] [--push-format gray16|rgb|rgba|bayer_rggb8|bayer_bggr16|gray10_mipi|gray12_mipi|gray10p|gray12p|
//                  bayer_rggb10_mipi|bayer_bggr12p] [--push-scaled] [--cov-out FILE]
//                 [--push-oriented rot90|rot180|rot270|flip|flip-rot90|flip-rot180|flip-rot270|0..7]
//
// (--push-color: a colour PNG is pushed as BGR / BGRA with channel 3 / 4 and reduced to gray by the library instead of by the reader.)
// (--push-scaled: a PNG larger than cam0.resolution is pushed at its own size, the whole frame as the crop, and cropped / area-scaled
// down by the library -- through any --push-color / --push-format setting; without the flag a size mismatch is an error.)
// (--push-oriented O: every PNG is turned by the inverse of orientation O in the reader -- the frame a sensor mounted that way would
// deliver -- and XRSLAMAmdSetFrameOrientation(O) has the library turn it back in the frame's upload: the run sees the original images.
// Works through --push-color / --push-format / --push-scaled; the reader's own rectification (--host-undistort) takes upright frames.)
// (--push-format: a 16-bit PNG is handed to the library as GRAY16 instead of being stripped to its high byte by the reader; a colour
// PNG as RGB8 / RGBA8 -- XRSLAMAmdPushImageFormat.  bayer_rggb8 / bayer_bggr16: the gray PNG becomes a raw mosaic whose every site
// holds the gray value -- bytes, or 16-bit samples with the value in the high byte -- and is pushed as BAYER_RGGB8 / BAYER_BGGR16.
// gray10_mipi .. bayer_bggr12p: the gray PNG -- a 16-bit one keeps its top 10 / 12 bits, an 8-bit one is shifted up -- is re-packed into
// the CSI-2 RAW10 / RAW12 or PFNC lsb-packed rows a sensor would send and pushed as that format, after any --push-oriented turn.)
// (--pipelined: XRSLAMAmdSetThreading(1), the reference's XRSLAM_ENABLE_THREADING build with deterministic hand-offs.)
// The reference player's own command line (main.cpp:57-79) is accepted as well, so its invocations carry over:
//
//   xrslam-player -sc configs/euroc_slam.yaml -dc configs/euroc_sensor.yaml [-lc license] [--tum traj.tum]
//                 [--csv traj.csv] [-p] euroc://<dir>/mav0 | tum://<dir>/mav0
//
// (-p / --play and the license are accepted and ignored: there is no viewer to start.)  `tum://` is the reference's
// TUM-VI reader (IO/tum_dataset_reader.cpp): same ASL directory layout, images undistorted with the equidistant
// (fisheye) model of xrslam::extra::ImageUndistorter instead of cv::undistort.
//
// By default the library initialises itself (SfM + IMU alignment, like the reference).  With --bootstrap-frames N
// the first N camera frames are instead seeded from state_groundtruth_estimate0 through XRSLAMAmdSetInitialState
// (N >= 36 covers the first window), which takes the initialiser out of an accuracy / throughput comparison.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "XRSLAM.h"
#include "euroc_io.hpp"
#include "../host/config.hpp"
#include "../host/pixel_format.hpp"

using namespace xrplayer;

// --push-oriented: a name or 0..7 -> the orientation o = quarter turns clockwise + 4 * mirrored first, -1 if it is neither
static int parse_orientation(const std::string &s) {
    static const char *names[8] = {"none", "rot90", "rot180", "rot270", "flip", "flip-rot90", "flip-rot180", "flip-rot270"};
    for (int o = 0; o < 8; ++o)
        if (s == names[o]) return o;
    if (s == "transverse") return 5;
    if (s == "flipv") return 6;
    if (s == "transpose") return 7;
    return s.size() == 1 && s[0] >= '0' && s[0] <= '7' ? s[0] - '0' : -1;
}
// The image whose turn by orientation o is `img`: its turn by the inverse orientation (a mirrored orientation undoes itself, a plain
// turn is undone by the opposite turn), pixel by pixel whatever a pixel's bytes are
static void turn_back(GrayImage &img, int o) {
    const int inv = (o & 4) ? o : (4 - o) & 3;
    if (inv == 0) return;
    const int W = (inv & 1) ? img.h : img.w, H = (inv & 1) ? img.w : img.h, c = img.channels;
    std::vector<uint8_t> out(img.px.size());
    for (int j = 0; j < img.h; ++j)
        for (int i = 0; i < img.w; ++i) {
            long long X, Y;
            xrh::orient_point(inv, img.w, img.h, i, j, X, Y);
            std::memcpy(&out[((size_t)Y * W + (size_t)X) * c], &img.px[((size_t)j * img.w + i) * c], (size_t)c);
        }
    img.px.swap(out);
    img.w = W;
    img.h = H;
}

// --push-format <packed>: the frame's samples (16-bit PNG: little-endian pairs, else bytes; the top pf.bits bits are kept) packed into
// dense rows of pf's packing (include/XRSLAM.h has the layouts), the frame a sensor would send.  -> the row's bytes
static int pack_image(GrayImage &img, const xrh::PixelFormat &pf) {
    const int row = (int)pf.row_bytes(img.w), low = pf.bits - 8, c = img.channels;
    std::vector<uint8_t> out((size_t)row * img.h, 0);
    for (int y = 0; y < img.h; ++y) {
        uint8_t *B = &out[(size_t)y * row];
        for (int x = 0; x < img.w; ++x) {
            const uint8_t *p = &img.px[((size_t)y * img.w + x) * c];
            const uint32_t v16 = c == 2 ? (uint32_t)p[0] | (uint32_t)p[1] << 8 : (uint32_t)p[0] << 8, v = v16 >> (16 - pf.bits);
            if (pf.packing == xrh::PixelFormat::PACK_MIPI) {
                const int g = x / pf.group_px(), i = x % pf.group_px();
                B[g * pf.group_bytes() + i] = (uint8_t)(v >> low);
                B[g * pf.group_bytes() + pf.group_px()] |= (uint8_t)((v & ((1u << low) - 1u)) << (low * i));
            } else {
                const size_t bit = (size_t)x * pf.bits;
                const uint32_t s = v << (bit & 7);
                B[bit >> 3] |= (uint8_t)s;
                B[(bit >> 3) + 1] |= (uint8_t)(s >> 8);
            }
        }
    }
    img.px.swap(out);
    img.channels = 0;   // (no whole bytes per pixel)
    return row;
}

static const TruthRow *nearest_truth(const std::vector<TruthRow> &gt, double t, double tol) {
    if (gt.empty()) return nullptr;
    size_t lo = 0, hi = gt.size();
    while (lo + 1 < hi) {
        const size_t mid = (lo + hi) / 2;
        if (gt[mid].t <= t) lo = mid;
        else hi = mid;
    }
    const TruthRow *best = &gt[lo];
    if (lo + 1 < gt.size() && std::fabs(gt[lo + 1].t - t) < std::fabs(best->t - t)) best = &gt[lo + 1];
    return std::fabs(best->t - t) <= tol ? best : nullptr;
}

int main(int argc, char **argv) {
    std::map<std::string, std::string> opt;
    bool undistort = true, host_undistort = false, pipelined = false, push_color = false, push_scaled = false;
    int png_keep = PNG_GRAY;   // --push-format
    int push_bayer = -1;       // --push-format bayer_*: the XRSLAMAmdPixelFormat the gray frames are pushed as
    int push_packed = -1;      // --push-format gray10_mipi ...: the packed XRSLAMAmdPixelFormat the gray frames are re-packed to
    int push_oriented = 0;     // --push-oriented: the orientation the frames are pushed in
    // the reference's option names (main.cpp:57-71) map onto ours
    const std::map<std::string, std::string> alias = {{"-sc", "slam"}, {"--slamconfig", "slam"}, {"-dc", "device"},
                                                      {"--deviceconfig", "device"}, {"-lc", "license"}, {"--license", "license"},
                                                      {"--tum", "out"}};
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--no-undistort") undistort = false;
        else if (a == "--host-undistort") host_undistort = true;   // the reference's arrangement: the reader rectifies on the host
        else if (a == "--pipelined") pipelined = true;
        else if (a == "--push-color") push_color = true;   // colour PNGs are pushed as BGR / BGRA (channel 3 / 4): the library reduces them
        else if (a == "--push-scaled") push_scaled = true;   // PNGs larger than cam0.resolution are scaled down by the library
        else if (a == "--push-oriented" && i + 1 < argc) {
            push_oriented = parse_orientation(argv[++i]);
            if (push_oriented < 0) {
                std::fprintf(stderr, "--push-oriented: rot90, rot180, rot270, flip, flip-rot90, flip-rot180, flip-rot270 or 0..7\n");
                return 2;
            }
        }
        else if (a == "--push-format" && i + 1 < argc) {
            const std::string f = argv[++i];
            if (f == "gray16") png_keep = PNG_KEEP_GRAY16;
            else if (f == "rgb") png_keep = PNG_KEEP_RGB;
            else if (f == "rgba") png_keep = PNG_KEEP_RGBA;
            else if (f == "bayer_rggb8") push_bayer = XRSLAM_AMD_PIXEL_BAYER_RGGB8;
            else if (f == "bayer_bggr16") push_bayer = XRSLAM_AMD_PIXEL_BAYER_BGGR16;
            else if (f == "gray10_mipi") push_packed = XRSLAM_AMD_PIXEL_GRAY10_MIPI;
            else if (f == "gray12_mipi") push_packed = XRSLAM_AMD_PIXEL_GRAY12_MIPI;
            else if (f == "gray10p") push_packed = XRSLAM_AMD_PIXEL_GRAY10P;
            else if (f == "gray12p") push_packed = XRSLAM_AMD_PIXEL_GRAY12P;
            else if (f == "bayer_rggb10_mipi") push_packed = XRSLAM_AMD_PIXEL_BAYER_RGGB10_MIPI;
            else if (f == "bayer_bggr12p") push_packed = XRSLAM_AMD_PIXEL_BAYER_BGGR12P;
            else {
                std::fprintf(stderr, "--push-format: gray16, rgb, rgba, bayer_rggb8, bayer_bggr16, gray10_mipi, gray12_mipi, gray10p, gray12p, "
                                     "bayer_rggb10_mipi or bayer_bggr12p\n");
                return 2;
            }
            if (push_packed >= 0) png_keep = PNG_KEEP_GRAY16;   // (a 16-bit PNG keeps its low byte for the packer)
        }
        else if (a == "-p" || a == "--play") continue;
        else if (alias.count(a) && i + 1 < argc) opt[alias.at(a)] = argv[++i];
        else if (a.rfind("--", 0) == 0 && i + 1 < argc) opt[a.substr(2)] = argv[++i];
        else if (a[0] != '-' && !opt.count("input")) opt["input"] = a;
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    std::string model = "cv_undistort";   // EurocDatasetReader::read_image: cv::undistort, radial-tangential
    if (opt.count("input")) {
        const auto [scheme, path] = split_dataset_url(opt["input"]);
        if (scheme.empty()) {
            std::fprintf(stderr, "Cannot open \"%s\"\n", opt["input"].c_str());   // main.cpp:99-103
            return 1;
        }
        opt["euroc"] = path;
        if (scheme == "tum") model = "equidistant";
    }
    if (!opt.count("slam") || !opt.count("device") || !opt.count("euroc")) {
        std::fprintf(stderr, "usage: xrslam-player --slam cfg.yaml --device sensor.yaml --euroc <dir>/mav0 [--out traj.tum] "
                             "[--csv traj.csv] [--bootstrap-frames N] [--max-frames N] [--no-undistort | --host-undistort] [--pipelined] [--push-color] [--push-format gray16|rgb|rgba|bayer_rggb8|bayer_bggr16|gray10_mipi|gray12_mipi|gray10p|gray12p|bayer_rggb10_mipi|bayer_bggr12p] [--push-scaled] [--push-oriented rot90|rot180|rot270|flip|...|0..7] [--mask mask.pgm|mask.png]\n"
                             "       [--cov-out FILE] [--view-out DIR [--view-every N] [--view-mode reference|age] [--view-trail K]]\n"
                             "   or: xrslam-player -sc cfg.yaml -dc sensor.yaml [--tum traj.tum] [--csv traj.csv] [-p] "
                             "euroc://<dir>/mav0 | tum://<dir>/mav0\n");
        return 2;
    }
    const std::string root = opt["euroc"];
    const size_t bootstrap = opt.count("bootstrap-frames") ? (size_t)std::atol(opt["bootstrap-frames"].c_str()) : 0;
    const size_t max_frames = opt.count("max-frames") ? (size_t)std::atol(opt["max-frames"].c_str()) : (size_t)-1;

    // the same configuration surface the library parses (camera offset, intrinsics and distortion for the reader)
    xrh::Config cfg;
    try {
        cfg = xrh::load_config(opt["slam"], opt["device"]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "configuration: %s\n", e.what());
        return 1;
    }
    // --mask FILE: an 8-bit PGM (P5) or gray PNG at the working resolution, nonzero = usable: the static mask, set before the first frame
    GrayImage mask;
    if (opt.count("mask")) {
        try {
            mask = load_mask(read_file(opt["mask"]), (int)cfg.cam_resolution[0], (int)cfg.cam_resolution[1]);
        } catch (const std::exception &e) {
            std::fprintf(stderr, "--mask %s: %s\n", opt["mask"].c_str(), e.what());
            return 1;
        }
    }
    const std::vector<CameraRow> cam = load_camera_csv(root + "/cam0/data.csv");
    const std::vector<ImuRow> imu = load_imu_csv(root + "/imu0/data.csv");
    const std::vector<TruthRow> gt = load_groundtruth_csv(root + "/state_groundtruth_estimate0/data.csv");
    if (cam.empty() || imu.empty()) {
        std::fprintf(stderr, "no camera or IMU data under %s\n", root.c_str());
        return 1;
    }
    const std::vector<Event> events = merge_events(cam, imu, cfg.cam_time_offset);

    void *handle = nullptr;
    if (XRSLAMCreate(opt["slam"].c_str(), opt["device"].c_str(), "", "xrslam-player", &handle) != 1) {
        std::fprintf(stderr, "XRSLAMCreate failed: %s\n", XRSLAMAmdLastError());
        return 1;
    }
    // Frames are rectified on the GPU by default (one upload of the frame as recorded, no host pass over the pixels);
    // --host-undistort keeps the reference's arrangement, where the reader thread runs cv::undistort.  Same pixels
    // either way: the library builds the same 1/32-pixel map (host/undistort_map.hpp).
    const bool device_undistort = undistort && cfg.cam_distortion_flag && !host_undistort;
    if (device_undistort) XRSLAMAmdSetDeviceUndistort(model.c_str());
    if (pipelined) XRSLAMAmdSetThreading(1);
    if (push_oriented != 0 && XRSLAMAmdSetFrameOrientation(push_oriented) != 1) {
        std::fprintf(stderr, "--push-oriented: %s\n", XRSLAMAmdLastError());
        XRSLAMDestroy();
        return 1;
    }
    // the frame as it is pushed: height x width of the working image for odd quarter turns
    const int frame_w = (int)cfg.cam_resolution[(push_oriented & 1) ? 1 : 0], frame_h = (int)cfg.cam_resolution[(push_oriented & 1) ? 0 : 1];
    if (!mask.px.empty() && XRSLAMAmdSetMask(mask.px.data(), mask.w, 0) != 1) {
        std::fprintf(stderr, "--mask %s: %s\n", opt["mask"].c_str(), XRSLAMAmdLastError());
        XRSLAMDestroy();
        return 1;
    }
    size_t seeded = 0;
    for (size_t i = 0; i < cam.size() && i < bootstrap; ++i) {
        const double t = cam[i].t + cfg.cam_time_offset;
        if (const TruthRow *g = nearest_truth(gt, t, 2.6e-3)) {
            const double q[4] = {g->q[1], g->q[2], g->q[3], g->q[0]};   // ASL stores w first
            XRSLAMAmdSetInitialState(t, q, g->p, g->v, g->bg, g->ba);
            ++seeded;
        }
    }
    FILE *out = opt.count("out") ? std::fopen(opt["out"].c_str(), "w") : nullptr;
    FILE *csv = opt.count("csv") ? std::fopen(opt["csv"].c_str(), "w") : nullptr;
    // --cov-out FILE: one line per answered frame -- timestamp of the covariance, the 21 upper-triangle entries of pose_ros, status
    FILE *cov = opt.count("cov-out") ? std::fopen(opt["cov-out"].c_str(), "w") : nullptr;
    if (cov) XRSLAMAmdSetCovariance(1);
    if ((opt.count("out") && !out) || (opt.count("csv") && !csv) || (opt.count("cov-out") && !cov)) {
        std::fprintf(stderr, "Cannot open file\n");   // trajectory_writer.h:37,62
        return 1;
    }
    // --view-out DIR: the tracker's view of every N-th tracked frame (XRSLAMAmdRenderTrackingView: the reference player's
    // feature_tracker_painter window, main.cpp:110-113) as DIR/<timestamp in ns>.ppm -- binary P6, RGB
    const bool view_on = opt.count("view-out") != 0;
    const long view_every = opt.count("view-every") ? std::max(1L, std::atol(opt["view-every"].c_str())) : 1;
    XRSLAMAmdViewOptions view_opt = {0, 0, 0};
    if (opt.count("view-mode")) {
        if (opt["view-mode"] == "age") view_opt.color_mode = 1, view_opt.draw_new = 1;
        else if (opt["view-mode"] != "reference") {
            std::fprintf(stderr, "--view-mode is reference or age\n");
            return 2;
        }
    }
    if (opt.count("view-trail")) view_opt.trail = (int)std::max(0L, std::min(8L, std::atol(opt["view-trail"].c_str())));
    if (view_on && view_opt.trail > 0) XRSLAMAmdSetFeatureHistory(view_opt.trail);
    long view_seen = 0, view_written = 0;
    double view_last_t = -1.0;
    std::vector<uint8_t> view_px;
    auto write_view = [&]() -> bool {   // false: the run ends with the error
        double t = 0.0;
        if (!view_on || XRSLAMAmdGetFeatures(nullptr, 0, &t) <= 0 || t == view_last_t) return true;
        view_last_t = t;
        if (view_seen++ % view_every != 0) return true;
        const int w = (int)cfg.cam_resolution[0], h = (int)cfg.cam_resolution[1];
        view_px.resize((size_t)w * h * 3);
        if (XRSLAMAmdRenderTrackingView(view_px.data(), w * 3, 3, 0, &view_opt) != 1) return false;
        for (size_t i = 0; i < view_px.size(); i += 3) std::swap(view_px[i], view_px[i + 2]);   // BGR -> RGB
        char name[64];
        std::snprintf(name, sizeof(name), "/%lld.ppm", (long long)std::llround(t * 1e9));
        FILE *fp = std::fopen((opt["view-out"] + name).c_str(), "wb");
        if (!fp) {
            std::fprintf(stderr, "Cannot open file\n");
            return false;
        }
        std::fprintf(fp, "P6\n%d %d\n255\n", w, h);
        const bool ok = std::fwrite(view_px.data(), 1, view_px.size(), fp) == view_px.size();
        std::fclose(fp);
        if (ok) ++view_written;
        return ok;
    };
    bool view_failed = false;
    const double K4[4] = {cfg.K.fx, cfg.K.fy, cfg.K.cx, cfg.K.cy};
    std::unique_ptr<Undistorter> und;
    std::vector<uint8_t> rectified;
    std::vector<xrh::V3> est, ref;
    bool has_gyro = false, has_acc = false;
    size_t frames = 0, tracked = 0;
    // a frame is processed when the next IMU sample arrives (detail.cpp:134), so the loop is timed as a whole;
    // PNG decoding and undistortion run in the reference's reader thread and are timed separately here
    double io_seconds = 0.0;
    const auto loop_begin = std::chrono::steady_clock::now();
    for (const Event &ev : events) {
        if (ev.type == EV_GYROSCOPE) {
            has_gyro = true;
            XRSLAMGyroscope g{{imu[ev.index].w[0], imu[ev.index].w[1], imu[ev.index].w[2]}, ev.t};
            XRSLAMPushSensorData(XRSLAM_SENSOR_GYROSCOPE, &g);
        } else if (ev.type == EV_ACCELEROMETER) {
            has_acc = true;
            XRSLAMAcceleration a{{imu[ev.index].a[0], imu[ev.index].a[1], imu[ev.index].a[2]}, ev.t};
            XRSLAMPushSensorData(XRSLAM_SENSOR_ACCELERATION, &a);
        } else {
            if (frames >= max_frames) break;
            const auto io0 = std::chrono::steady_clock::now();
            GrayImage img;
            try {
                img = decode_png(read_file(root + "/cam0/data/" + cam[ev.index].filename), png_keep != PNG_GRAY ? png_keep : (int)push_color);
            } catch (const std::exception &e) {
                std::fprintf(stderr, "%s: %s\n", cam[ev.index].filename.c_str(), e.what());
                break;
            }
            if (push_bayer >= 0 && img.channels == 1 && img.pixel_format < 0) {   // the mosaic: every site gets the gray value
                if (push_bayer >= XRSLAM_AMD_PIXEL_BAYER_RGGB16) {
                    std::vector<uint8_t> m(img.px.size() * 2, 0);
                    for (size_t i = 0; i < img.px.size(); ++i) m[2 * i + 1] = img.px[i];
                    img.px.swap(m);
                    img.channels = 2;
                }
                img.pixel_format = push_bayer;
            }
            // the library copies cam0.resolution rows x columns out of the buffer it is handed
            // (XRSLAMManager.cpp:113-131 does the same with the configured size): a frame of any other size is an error
            if (push_oriented != 0) {
                if (undistort && cfg.cam_distortion_flag && !device_undistort) {
                    std::fprintf(stderr, "%s: --push-oriented with --host-undistort: the reader rectifies upright frames only\n",
                                 cam[ev.index].filename.c_str());
                    break;
                }
                turn_back(img, push_oriented);
            }
            int stride = img.w * img.channels;
            if (push_packed >= 0 && img.channels <= 2 && (img.pixel_format < 0 || img.pixel_format == XRSLAM_AMD_PIXEL_GRAY16)) {
                xrh::PixelFormat pf;
                xrh::describe_pixel_format(push_packed, 0, 0, pf);
                stride = pack_image(img, pf);
                img.pixel_format = push_packed;
            }
            const bool oversized = push_scaled && img.w >= frame_w && img.h >= frame_h && (img.w != frame_w || img.h != frame_h);
            if (oversized) {   // --push-scaled: the frame goes in at its own size, the whole of it as the crop
                if (undistort && cfg.cam_distortion_flag && !device_undistort) {
                    std::fprintf(stderr, "%s: --push-scaled with --host-undistort: the reader rectifies working-size frames only\n",
                                 cam[ev.index].filename.c_str());
                    break;
                }
                io_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - io0).count();
                const XRSLAMAmdFrameFormat ff{img.pixel_format >= 0 ? img.pixel_format
                                              : img.channels == 3 ? (int)XRSLAM_AMD_PIXEL_BGR8
                                              : img.channels == 4 ? (int)XRSLAM_AMD_PIXEL_BGRA8 : (int)XRSLAM_AMD_PIXEL_GRAY8, 0, 0};
                const XRSLAMAmdFrameGeometry geo{img.w, img.h, 0, 0, img.w, img.h};
                XRSLAMAmdPushImageScaled(img.px.data(), stride, &ff, &geo, 0, ev.t);
            } else if (img.w != frame_w || img.h != frame_h) {
                std::fprintf(stderr, "%s: image is %dx%d, the device configuration says %dx%d\n", cam[ev.index].filename.c_str(), img.w,
                             img.h, frame_w, frame_h);
                break;
            }
            const bool rectify_here = !oversized && undistort && cfg.cam_distortion_flag && !device_undistort;
            const bool mosaic = img.pixel_format >= XRSLAM_AMD_PIXEL_BAYER_RGGB8;   // (or packed: reduce_frame's either way)
            if ((img.channels != 1 || mosaic) && rectify_here) {   // the host remap takes gray: reduced first, rectified second, as in the library
                std::vector<uint8_t> g((size_t)img.w * img.h);
                xrh::PixelFormat pf;
                if (mosaic && !xrh::describe_pixel_format(img.pixel_format, 0, 0, pf))
                    xrh::reduce_frame(g.data(), img.px.data(), stride, img.w, img.h, pf);
                for (size_t i = 0; i < g.size() && !mosaic; ++i) {
                    const uint8_t *c = &img.px[i * img.channels];
                    if (img.pixel_format == XRSLAM_AMD_PIXEL_GRAY16) g[i] = c[1];   // 16 significant bits: the high byte
                    else if (img.pixel_format >= 0) g[i] = (uint8_t)((c[0] * 4899 + c[1] * 9617 + c[2] * 1868 + 8192) >> 14);   // RGB(A)
                    else g[i] = (uint8_t)((c[0] * 1868 + c[1] * 9617 + c[2] * 4899 + 8192) >> 14);
                }
                img.px.swap(g);
                img.channels = 1;
                img.pixel_format = -1;
            }
            const uint8_t *pixels = img.px.data();
            if (rectify_here) {
                if (!und) {
                    if (model == "cv_undistort") und.reset(new Undistorter(img.w, img.h, K4, cfg.cam_distortion));
                    else und.reset(new Undistorter(img.w, img.h, K4, std::vector<double>(cfg.cam_distortion, cfg.cam_distortion + 4), model));
                }
                rectified.resize((size_t)img.w * img.h);
                und->apply(img.px.data(), img.w, rectified.data(), img.w);
                pixels = rectified.data();
            }
            if (!oversized) io_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - io0).count();
            if (oversized) {
                // (pushed above)
            } else if (img.pixel_format >= 0) {
                const XRSLAMAmdFrameFormat ff{img.pixel_format, 0, 0};
                XRSLAMAmdPushImageFormat(pixels, stride, &ff, 0, ev.t);
            } else {
                XRSLAMImage xi;
                std::memset(&xi, 0, sizeof(xi));
                xi.camera_id = 0;
                xi.timeStamp = ev.t;
                xi.data = const_cast<uint8_t *>(pixels);
                xi.channel = img.channels;
                xi.stride = img.w * img.channels;
                XRSLAMPushSensorData(XRSLAM_SENSOR_CAMERA, &xi);
            }
            if (has_gyro && has_acc) {
                XRSLAMRunOneFrame();
                if (!write_view()) {   // (the frame tracked since the last image: its plane lives until the next one is tracked)
                    view_failed = true;
                    break;
                }
                XRSLAMState state;
                XRSLAMGetResult(XRSLAM_RESULT_STATE, &state);
                if (state == XRSLAM_STATE_TRACKING_SUCCESS) {
                    XRSLAMPose pose;
                    XRSLAMGetResult(XRSLAM_RESULT_BODY_POSE, &pose);
                    // before the first tracked frame the library reports an all-zero quaternion (detail.cpp:165-168);
                    // such a pose carries no estimate and is kept out of the trajectory
                    const bool valid = pose.quaternion[0] != 0 || pose.quaternion[1] != 0 || pose.quaternion[2] != 0 || pose.quaternion[3] != 0;
                    if (pose.timestamp > 0 && valid) {
                        ++tracked;
                        if (out) write_tum_pose(out, pose.timestamp, pose.translation, pose.quaternion);
                        if (csv) write_csv_pose(csv, pose.timestamp, pose.translation, pose.quaternion);
                        if (cov) {
                            XRSLAMAmdCovariance cv;
                            XRSLAMAmdGetCovariance(&cv);
                            std::fprintf(cov, "%.9f", cv.timestamp);
                            for (int i = 0; i < 6; ++i)
                                for (int j = i; j < 6; ++j) std::fprintf(cov, " %.17g", cv.pose_ros[i][j]);
                            std::fprintf(cov, " %d\n", cv.status);
                        }
                        if (const TruthRow *g = nearest_truth(gt, pose.timestamp, 2.6e-3)) {
                            est.push_back({pose.translation[0], pose.translation[1], pose.translation[2]});
                            ref.push_back({g->p[0], g->p[1], g->p[2]});
                        }
                    }
                }
            }
            ++frames;
        }
    }
    XRSLAMAmdFlush();   // pipelined mode: the backend of the last frame belongs to the run
    const double busy = std::chrono::duration<double>(std::chrono::steady_clock::now() - loop_begin).count() - io_seconds;
    if (out) std::fclose(out);
    if (csv) std::fclose(csv);
    if (cov) std::fclose(cov);
    if (!view_failed && !write_view()) view_failed = true;
    const char *err = XRSLAMAmdLastError();
    if (view_failed && !(err && *err)) err = "the tracking view could not be written";
    XRSLAMAmdInitReport rep;
    std::memset(&rep, 0, sizeof(rep));
    XRSLAMAmdGetInitReport(&rep);
    std::printf("{\"frames\": %zu, \"tracked\": %zu, \"bootstrap_states\": %zu, \"init_attempts\": %ld, \"init_scale\": %.6f, "
                "\"ms_per_frame\": %.4f, \"io_ms_per_frame\": %.4f, \"ate_rmse_m\": %.6f, \"views\": %ld, \"error\": \"%s\"}\n",
                frames, tracked, seeded, rep.attempts, rep.successes ? rep.scale : 0.0, frames ? 1e3 * busy / frames : 0.0,
                frames ? 1e3 * io_seconds / frames : 0.0, est.size() >= 3 ? ate_rmse(est, ref) : -1.0, view_written, err ? err : "");
    XRSLAMDestroy();
    return (err && *err) ? 1 : 0;
}
