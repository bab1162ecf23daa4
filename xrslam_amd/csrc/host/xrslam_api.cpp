// xrslam_api.cpp -- the outer C ABI (include/XRSLAM.h) on top of the host pipeline.
// Mirrors XRSLAMManager (reference xrslam-interface/src/XRSLAMManager.cpp:85-242) and
// XRSLAMInternal.cpp:4-90: deep-copied images, synchronous calls.  The six reference symbols keep the reference's
// process-global instance (XRSLAMManager.cpp:6-9); every entry point is a thin wrapper over the same functions on an
// `Instance`, and the additive XRSLAMAmdInstance* symbols expose those directly, so that one process can run several
// independent sequences on one GPU (the reference's globals force one instance per process; here all
// state -- id counters, CLAHE / Harris scratch, solver configuration, RD-VIO bin confidences -- lives in the instance).
// An instance may be driven by one thread at a time; different instances may be driven by different threads.
#include "../../../include/XRSLAM.h"

#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

#include "pipeline.hpp"

namespace {

struct Manager {
    std::unique_ptr<xrh::System> sys;
    xrh::Config config;
    std::shared_ptr<xrh::HipImage> cur_image;
    std::mutex input_mutex;
    std::string last_error;
    int device = -1;   // HIP device the instance was created on (the current device is a per-thread setting)
    bool bound_by_replay = false;   // inside XRSLAMAmdInstanceReplay: the device is current for the whole loop
    // XRSLAMAmdSetNextFrameMask: waits for the next pushed camera frame (a host mask: our copy, packed; an HBM mask: the caller's)
    bool next_mask_set = false, next_mask_on_device = false;
    std::vector<uint8_t> next_mask_host;
    const void *next_mask_dev = nullptr;
    int next_mask_stride = 0;
    // XRSLAMAmdSetFrameOrientation: how the camera is mounted; every pushed frame takes the value in force when it is pushed
    std::atomic<int> orientation{0};
};

Manager &mgr() {
    static Manager m;
    return m;
}

// The thread that drives an instance need not be the one that created it: make the instance's device current.
void bind_device(const Manager &m) {
    if (m.bound_by_replay) return;   // XRSLAMAmdInstanceReplay made the device current once for all the pushes of its loop
    if (m.device >= 0) xrhip_bind_device(m.device);
}

template <class F> void guarded(Manager &m, F &&f) {
    try {
        f();
    } catch (const std::exception &e) {
        m.last_error = e.what();
        std::fprintf(stderr, "[xrslam_hip] %s\n", e.what());
        // whoever threw may have left work between a begin and its end, on the device and in the host's bookkeeping, and -- in
        // pipelined mode -- a backend job running: System::recover_after_error joins it, unwinds both sides and, if the sliding-window
        // tracker was interrupted, falls back to the initialiser like the reference's tracking-failure branch
        if (m.sys) m.sys->recover_after_error();
    }
}

void fill_pose(const xrh::PoseState &latest, const xrh::Quat &q_ext, const xrh::V3 &p_ext, double t, XRSLAMPose *pose) {
    xrh::Quat q = latest.q * q_ext;
    xrh::V3 p = latest.p + latest.q * p_ext;
    pose->timestamp = t;
    pose->quaternion[0] = q.x;
    pose->quaternion[1] = q.y;
    pose->quaternion[2] = q.z;
    pose->quaternion[3] = q.w;
    pose->translation[0] = p.x;
    pose->translation[1] = p.y;
    pose->translation[2] = p.z;
}


int impl_create(Manager &m, const char *slam_config_path, const char *device_config_path, void **config) {
    int ok = 0;
    if (xrhip_get_device(&m.device) != 0) m.device = -1;
    m.last_error.clear();   // XRSLAMAmdLastError speaks about the instance being created, not about an earlier one
    m.orientation.store(0);   // (likewise the frame orientation: a new instance starts with upright frames)
    guarded(m, [&] {
        {   // a second Create without Destroy: drop the previous instance first, in XRSLAMDestroy's order -- the pending
            // image returns its device buffer to the Pipeline that owns it, which must still be alive at that point
            std::lock_guard<std::mutex> lk(m.input_mutex);
            m.cur_image.reset();
            m.sys.reset();
        }
        m.config = xrh::load_config(slam_config_path, device_config_path);
        m.sys = std::make_unique<xrh::System>(m.config);
        if (config) *config = static_cast<void *>(&m.config);
        ok = 1;
    });
    return ok;
}

// A camera frame becomes the image XRSLAMRunOneFrame tracks next.  A frame that is refused does not arrive: the error is reported and
// the pending image is dropped, so that XRSLAMRunOneFrame does not track the previous image a second time.
// (refused: what the entry point itself found wrong with its arguments, in place of the frame)
void push_frame(Manager &m, const xrh::FrameInput &in, double t, const char *refused = nullptr) {
    if (!m.sys) return;
    bind_device(m);
    guarded(m, [&] {
        try {
            std::lock_guard<std::mutex> lk(m.input_mutex);
            // the mask waiting for this frame goes with it, whatever becomes of the frame
            xrh::FrameInput fin = in;
            fin.orientation = m.orientation.load();
            if (m.next_mask_set) {
                fin.mask = m.next_mask_on_device ? static_cast<const uint8_t *>(m.next_mask_dev) : m.next_mask_host.data();
                fin.mask_stride = m.next_mask_stride;
                fin.mask_on_device = m.next_mask_on_device;
                m.next_mask_set = false;
            }
            if (refused) throw std::runtime_error(refused);
            m.cur_image = m.sys->P.make_image(fin, t);
        } catch (...) {
            std::lock_guard<std::mutex> lk(m.input_mutex);
            m.cur_image.reset();
            throw;
        }
    });
}
xrhip_frame_geometry to_inner(const XRSLAMAmdFrameGeometry &g) {
    return xrhip_frame_geometry{g.src_width, g.src_height, g.crop_x, g.crop_y, g.crop_width, g.crop_height};
}
// pixels of `channels` (fmt null) or of *fmt; geo set: larger than the working resolution
xrh::FrameInput frame_input(const void *pixels, int stride, int on_device, int channels, const XRSLAMAmdFrameFormat *fmt,
                            const xrhip_frame_geometry *geo = nullptr) {
    xrh::FrameInput in;
    in.pixels = static_cast<const uint8_t *>(pixels);
    in.stride = stride;
    in.on_device = on_device != 0;
    in.channels = channels;
    in.by_format = fmt != nullptr;
    if (fmt) {
        in.format = fmt->format;
        in.bits = fmt->bits;
        in.limited_range = fmt->limited_range;
    }
    in.geo = geo;
    return in;
}

void impl_push(Manager &m, XRSLAMSensorType type, void *data) {
    if (!m.sys || !data) return;
    if (type == XRSLAM_SENSOR_CAMERA) {   // channel 3 / 4 (BGR / BGRA): the frame's upload reduces it to gray
        auto *im = static_cast<XRSLAMImage *>(data);
        if (im->camera_id == 0) push_frame(m, frame_input(im->data, im->stride, 0, im->channel, nullptr), im->timeStamp);
        return;
    }
    bind_device(m);
    guarded(m, [&] {
        switch (type) {
        case XRSLAM_SENSOR_ACCELERATION: {
            auto *a = static_cast<XRSLAMAcceleration *>(data);
            m.sys->track_accelerometer(a->timestamp, a->data[0], a->data[1], a->data[2], false);
            break;
        }
        case XRSLAM_SENSOR_GYROSCOPE: {
            auto *g = static_cast<XRSLAMGyroscope *>(data);
            m.sys->track_gyroscope(g->timestamp, g->data[0], g->data[1], g->data[2], false);
            break;
        }
        default:
            break;
        }
    });
}

void impl_run(Manager &m) {
    if (!m.sys) return;
    bind_device(m);
    guarded(m, [&] {
        std::lock_guard<std::mutex> lk(m.input_mutex);
        if (m.cur_image) m.sys->track_camera(m.cur_image);
    });
}

void impl_get_result(Manager &m, XRSLAMResultType type, void *out) {
    if (!m.sys || !out) return;
    guarded(m, [&] {
        switch (type) {
        case XRSLAM_RESULT_BODY_POSE:
            fill_pose(m.sys->latest_pose, m.config.q_bi, m.config.p_bi, m.sys->latest_timestamp, static_cast<XRSLAMPose *>(out));
            break;
        case XRSLAM_RESULT_CAMERA_POSE:
            fill_pose(m.sys->latest_pose, m.config.q_bc, m.config.p_bc, m.sys->latest_timestamp, static_cast<XRSLAMPose *>(out));
            break;
        case XRSLAM_RESULT_STATE: {
            auto st = m.sys->get_system_state();
            *static_cast<XRSLAMState *>(out) = st == xrh::SYS_INITIALIZING ? XRSLAM_STATE_INITIALIZING
                                               : st == xrh::SYS_TRACKING   ? XRSLAM_STATE_TRACKING_SUCCESS
                                                                           : XRSLAM_STATE_TRACKING_FAIL;
            break;
        }
        case XRSLAM_RESULT_LANDMARKS: {
            m.sys->sync();   // pipelined mode: the window map belongs to the backend thread while a frame is in flight
            auto *lm = static_cast<XRSLAMLandmarks *>(out);
            lm->num_landmarks = 0;
            lm->landmarks = nullptr;
            if (m.sys->swt) {
                xrh::Map *map = m.sys->swt->map.get();
                std::vector<XRSLAMLandmark> pts;
                for (size_t i = 0; i < map->track_num(); ++i) {
                    xrh::Track *t = map->get_track(i);
                    if (t->tag(xrh::TT_VALID)) {
                        xrh::V3 p = t->get_landmark_point();
                        pts.push_back({p.x, p.y, p.z});
                    }
                }
                lm->num_landmarks = (int)pts.size();
                lm->landmarks = new XRSLAMLandmark[pts.size() + 1];   // caller-owned, like the reference (:207)
                std::memcpy(lm->landmarks, pts.data(), sizeof(XRSLAMLandmark) * pts.size());
            }
            break;
        }
        case XRSLAM_RESULT_FEATURES: {   // the painter's set (core/feature_tracker.cpp:143): key points with a track, in key-point order
            auto *ft = static_cast<XRSLAMFeatures *>(out);
            ft->pos.clear();
            std::lock_guard<std::mutex> lk(m.sys->view_mutex);
            for (const auto &f : m.sys->view.features)
                if (f.track_id >= 0) ft->pos.push_back({f.x, f.y});
            break;
        }
        case XRSLAM_RESULT_BIAS: {
            auto *b = static_cast<XRSLAMIMUBias *>(out);
            m.sys->sync();
            if (m.sys->swt) {
                auto [t, pose, motion] = m.sys->swt->get_latest_state();
                (void)t;
                (void)pose;
                for (int i = 0; i < 3; ++i) {
                    b->acc_bias.data[i] = motion.ba[i];
                    b->gyr_bias.data[i] = motion.bg[i];
                }
            }
            break;
        }
        case XRSLAM_RESULT_VERSION: {
            auto *s = static_cast<XRSLAMStringOutput *>(out);
            static const char ver[] = "0.1.0";
            s->str_length = (int)std::strlen(ver);
            s->data = new char[s->str_length + 5];
            std::strcpy(s->data, ver);
            break;
        }
        case XRSLAM_INFO_INTRINSICS: {
            auto *k = static_cast<XRSLAMIntrinsics *>(out);
            k->fx = m.config.K.fx;
            k->fy = m.config.K.fy;
            k->cx = m.config.K.cx;
            k->cy = m.config.K.cy;
            break;
        }
        default:
            break;
        }
    });
}

void impl_destroy(Manager &m) {
    bind_device(m);
    guarded(m, [&] {
        m.cur_image.reset();
        m.sys.reset();
    });
}

void impl_set_initial_state(Manager &m, double t, const double q[4], const double p[3], const double v[3],
                            const double bg[3], const double ba[3]) {
    if (!m.sys) return;
    xrh::InitialState s;
    s.t = t;
    s.pose.q = xrh::Quat{q[0], q[1], q[2], q[3]}.normalized();
    s.pose.p = {p[0], p[1], p[2]};
    s.motion.v = {v[0], v[1], v[2]};
    s.motion.bg = {bg[0], bg[1], bg[2]};
    s.motion.ba = {ba[0], ba[1], ba[2]};
    m.sys->init.states.push_back(s);
}

void impl_push_image_device(Manager &m, const void *gray_dev, int stride, double timestamp, int channels = 1) {
    push_frame(m, frame_input(gray_dev, stride, 1, channels, nullptr), timestamp);
}

// A frame in one of the XRSLAMAmdPixelFormat layouts, from host memory or HBM.  A bad format drops the frame and sets the last error.
void impl_push_image_format(Manager &m, const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt, int on_device, double timestamp) {
    push_frame(m, frame_input(pixels, stride, on_device, 1, fmt), timestamp,
               fmt && pixels ? nullptr : "Image format is not supported: null pixels or format");
}

// A frame larger than the working resolution (XRSLAMAmdFrameGeometry), of any format (null: GRAY8).  A bad geometry or format drops
// the frame and sets the last error.
void impl_push_image_scaled(Manager &m, const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt, const XRSLAMAmdFrameGeometry *geo,
                            int on_device, double timestamp) {
    const xrhip_frame_geometry g = geo ? to_inner(*geo) : xrhip_frame_geometry{};
    push_frame(m, frame_input(pixels, stride, on_device, 1, fmt, &g), timestamp,
               geo && pixels ? nullptr : "Image geometry is not supported: null pixels or geometry");
}

// A value outside 0..7 is reported and the setting stays; nothing aborts and no frame is touched.
int impl_set_frame_orientation(Manager &m, int o) {
    if (!xrh::orientation_valid(o)) {
        m.last_error = "Frame orientation is not supported: " + std::to_string(o) + " is not 0..7 (quarter turns clockwise + 4 * mirrored)";
        std::fprintf(stderr, "[xrslam_hip] %s\n", m.last_error.c_str());
        return 0;
    }
    m.orientation.store(o);
    return 1;
}

void impl_get_camera_config(Manager &m, XRSLAMAmdCameraConfig *out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    if (!m.sys) return;
    const xrh::Config &c = m.config;
    out->time_offset = c.cam_time_offset;
    out->distortion_flag = (int)c.cam_distortion_flag;
    for (int i = 0; i < 4; ++i) out->distortion[i] = c.cam_distortion[i];
    out->intrinsics[0] = c.K.fx;
    out->intrinsics[1] = c.K.fy;
    out->intrinsics[2] = c.K.cx;
    out->intrinsics[3] = c.K.cy;
    out->resolution[0] = (int)c.cam_resolution[0];
    out->resolution[1] = (int)c.cam_resolution[1];
}

int impl_describe_config(Manager &m, char *buf, int cap) {
    if (!m.sys) return 0;
    const std::string text = xrh::describe_config(m.config);
    if (buf && cap > 0) {
        const size_t n = std::min(text.size(), (size_t)cap - 1);
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int)text.size();
}

void impl_set_device_undistort(Manager &m, const char *model) {
    if (!m.sys) return;
    bind_device(m);
    guarded(m, [&] { m.sys->P.set_device_undistort(model); });
}

void impl_flush(Manager &m) {
    if (!m.sys) return;
    bind_device(m);
    guarded(m, [&] { m.sys->sync(); });
}

// XRSLAMAmdSetMask / XRSLAMAmdSetNextFrameMask: 1, or 0 with the reason in last_error and the mask in force unchanged
int mask_refused(Manager &m, const std::string &why) {
    m.last_error = why;
    std::fprintf(stderr, "[xrslam_hip] %s\n", why.c_str());
    return 0;
}
int impl_set_mask(Manager &m, const void *mask, int stride, int on_device) {
    if (!m.sys) return mask_refused(m, "XRSLAMAmdSetMask: no instance");
    if (mask && stride < (int)m.config.cam_resolution[0]) return mask_refused(m, "XRSLAMAmdSetMask: stride < width of the working image");
    bind_device(m);
    int ok = 1;
    try {   // (not guarded(): a refused mask is an answer, not a failure of the frame in flight)
        std::lock_guard<std::mutex> lk(m.input_mutex);
        m.sys->P.set_static_mask(mask, stride, on_device != 0);
    } catch (const std::exception &e) {
        ok = mask_refused(m, std::string("XRSLAMAmdSetMask: ") + e.what());
    }
    return ok;
}
int impl_set_next_frame_mask(Manager &m, const void *mask, int stride, int on_device) {
    if (!m.sys) return mask_refused(m, "XRSLAMAmdSetNextFrameMask: no instance");
    const int w = (int)m.config.cam_resolution[0], h = (int)m.config.cam_resolution[1];
    if (mask && stride < w) return mask_refused(m, "XRSLAMAmdSetNextFrameMask: stride < width of the working image");
    if (mask && !xrhip_image_set_mask) return mask_refused(m, "XRSLAMAmdSetNextFrameMask: Mask is not supported: this library has no xrhip_image_set_mask");
    if (mask && m.sys->P.group) return mask_refused(m, "XRSLAMAmdSetNextFrameMask: the instance is a member of a group");
    std::lock_guard<std::mutex> lk(m.input_mutex);
    m.next_mask_set = mask != nullptr;
    if (!mask) return 1;
    m.next_mask_on_device = on_device != 0;
    if (on_device) {
        m.next_mask_dev = mask;
        m.next_mask_stride = stride;
    } else {   // copied now: the caller's buffer is free on return
        m.next_mask_host.resize((size_t)w * h);
        for (int y = 0; y < h; ++y) std::memcpy(&m.next_mask_host[(size_t)y * w], static_cast<const uint8_t *>(mask) + (size_t)y * stride, (size_t)w);
        m.next_mask_stride = w;
    }
    return 1;
}

void impl_set_threading(Manager &m, int mode) {
    if (!m.sys) return;
    bind_device(m);
    guarded(m, [&] { m.sys->set_threading(mode); });
}

void impl_get_times(Manager &m, XRSLAMAmdTimes *out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    if (!m.sys) return;
    impl_flush(m);
    const xrh::StageTimes &t = m.sys->P.times;
    out->frames = t.frames;
    out->solves = t.solves;
    out->solve_iterations = t.solve_iterations;
    out->marginalizations = t.marginalizations;
    out->keyframes = t.keyframes;
    out->ba_device_ms = t.ba_device_ms;
    out->wall_preprocess = t.w_preprocess;
    out->wall_track = t.w_track;
    out->wall_detect = t.w_detect;
    out->wall_preintegrate = t.w_preintegrate + t.w_preintegrate_ft;
    out->wall_solve = t.w_solve;
    out->wall_marginalize = t.w_marginalize;
    out->wall_frame = t.w_frame;
    for (int i = 0; i < 15; ++i) out->wall_scope[i] = t.scope[i];
    out->wall_scope[15] = t.w_join;
}

void impl_set_profiling(Manager &m, int enable) {
    if (m.sys) {
        impl_flush(m);   // pipelined mode: the backend thread may be inside xrhip_ba_solve, which reads the profiling switch
        bind_device(m);
        xrhip_klt_set_profiling(m.sys->P.klt, enable);
        xrhip_ba_set_profiling(m.sys->P.ba, enable);
        xrhip_ba_set_profiling(m.sys->P.ba_sub, enable);   // (localize_newframe's problem when it is solved together with refine_subwindow's)
    }
}

void impl_get_ba_stats(Manager &m, void *out, int reset) {
    if (!m.sys || !out) return;
    impl_flush(m);
    bind_device(m);
    guarded(m, [&] {
        xrhip_ba_stats *o = static_cast<xrhip_ba_stats *>(out), sub;
        xrh::hip_check(xrhip_ba_get_stats(m.sys->P.ba, o, reset), "xrhip_ba_get_stats");
        xrh::hip_check(xrhip_ba_get_stats(m.sys->P.ba_sub, &sub, reset), "xrhip_ba_get_stats");
        o->n_tiny += sub.n_tiny;   // the single-launch solves of the pair are booked on the context that began the first
        o->n_chain_timed += sub.n_chain_timed;
        o->ms_chain += sub.ms_chain;
        o->bytes_chain += sub.bytes_chain;
    });
}

void impl_set_covariance(Manager &m, int enable) {
    if (!m.sys) return;
    impl_flush(m);   // pipelined mode: the backend thread reads the switch
    m.sys->P.cov.enabled = enable != 0;
}

int impl_get_covariance(Manager &m, XRSLAMAmdCovariance *out) {
    if (!out) return 0;
    std::memset(out, 0, sizeof(*out));
    out->status = -1;
    if (!m.sys) return 0;
    impl_flush(m);
    const xrh::Pipeline::Covariance &cv = m.sys->P.cov;
    out->timestamp = cv.t;
    out->status = cv.status;
    out->rcond_estimate = cv.rcond;
    std::memcpy(out->state, cv.state, sizeof(cv.state));
    xrh::covariance_pose_ros(cv.state, &out->pose_ros[0][0]);
    if (cv.status == -1 && !cv.error.empty()) m.last_error = cv.error;
    return cv.status == 0 ? 1 : 0;
}

int impl_get_landmark_variances(Manager &m, double *var, long long *ids, int cap) {
    if (!m.sys) return 0;
    impl_flush(m);
    int n = 0;
    guarded(m, [&] {
        if (!m.sys->swt || m.sys->P.cov.status != 0) return;
        xrh::Map *map = m.sys->swt->map.get();
        std::vector<long long> valid;
        for (size_t i = 0; i < map->track_num(); ++i)
            if (map->get_track(i)->tag(xrh::TT_VALID)) valid.push_back((long long)map->get_track(i)->id);
        std::sort(valid.begin(), valid.end());
        for (const auto &[id, v] : m.sys->P.cov.landmark_var) {
            if (!std::binary_search(valid.begin(), valid.end(), id)) continue;
            if (n < cap) {
                if (var) var[n] = v;
                if (ids) ids[n] = id;
            }
            ++n;
        }
    });
    return n;
}

void impl_get_klt_stats(Manager &m, void *out, int reset) {
    if (!m.sys || !out) return;
    bind_device(m);
    guarded(m, [&] { xrh::hip_check(xrhip_klt_get_stats(m.sys->P.klt, static_cast<xrhip_klt_stats *>(out), reset), "xrhip_klt_get_stats"); });
}

static_assert(sizeof(XRSLAMAmdFeature) == sizeof(xrh::System::ViewFeature) && XRSLAM_AMD_VIEW_MAX_TRAIL == xrh::System::VIEW_MAX_TRAIL,
              "XRSLAMAmdFeature is the snapshot's record");

int impl_get_features(Manager &m, XRSLAMAmdFeature *out, int cap, double *timestamp) {
    if (!m.sys) return 0;
    std::lock_guard<std::mutex> lk(m.sys->view_mutex);
    const auto &v = m.sys->view;
    if (!v.valid) return 0;
    if (timestamp) *timestamp = v.t;
    const int n = (int)v.features.size();
    if (out && cap > 0) std::memcpy(out, v.features.data(), sizeof(XRSLAMAmdFeature) * (size_t)std::min(n, cap));
    return n;
}

void impl_set_feature_history(Manager &m, int frames) {
    if (m.sys) m.sys->view_history.store(std::max(0, std::min(frames, (int)XRSLAM_AMD_VIEW_MAX_TRAIL)), std::memory_order_relaxed);
}

// palette of the tracking view: the reference's yellow, the three ages, the new key points, the trails
const uint8_t kViewPalette[6][3] = {{0, 255, 255}, {0, 0, 255}, {0, 255, 255}, {0, 255, 0}, {255, 255, 0}, {255, 160, 0}};

// (a view that cannot be drawn is reported, not recovered from: nothing of the pipeline was touched)
int impl_render_view(Manager &m, void *out, int stride, int channels, int on_device, const XRSLAMAmdViewOptions *opt) {
    if (!m.sys) return 0;
    bind_device(m);
    try {
        if (!xrhip_image_render_view) throw std::runtime_error("this library has no view renderer");
        const XRSLAMAmdViewOptions o = opt ? *opt : XRSLAMAmdViewOptions{0, 0, 0};
        std::lock_guard<std::mutex> lk(m.sys->view_mutex);
        const auto &v = m.sys->view;
        if (!v.valid) throw std::runtime_error("no frame has been tracked yet");
        if (!v.image || !v.image->h) throw std::runtime_error("the newest frame's image has been released");
        std::vector<xrhip_view_marker> markers;
        std::vector<xrhip_view_segment> segs;
        markers.reserve(v.features.size());
        if (o.draw_new)
            for (const auto &f : v.features)
                if (f.track_id < 0) markers.push_back({(int32_t)f.x, (int32_t)f.y, 4u | (2u << 8)});
        for (const auto &f : v.features) {
            if (f.track_id < 0) continue;
            const uint32_t pal = o.color_mode == 1 ? (f.age < 4 ? 1u : f.age < 10 ? 2u : 3u) : 0u;
            markers.push_back({(int32_t)f.x, (int32_t)f.y, pal | (10u << 8)});
            int px = (int32_t)f.x, py = (int32_t)f.y;
            for (int j = 0; j < std::min(o.trail, f.n_trail); ++j) {
                const int qx = (int32_t)f.trail[j][0], qy = (int32_t)f.trail[j][1];
                segs.push_back({px, py, qx, qy, 5u});
                px = qx;
                py = qy;
            }
        }
        xrh::hip_check(xrhip_image_render_view(v.image->h, segs.data(), (int)segs.size(), markers.data(), (int)markers.size(),
                                               &kViewPalette[0][0], 6, out, stride, channels, on_device),
                       "xrhip_image_render_view");
        return 1;
    } catch (const std::exception &e) {
        m.last_error = std::string("XRSLAMAmdRenderTrackingView: ") + e.what();
        return 0;
    }
}

int impl_get_tracker_params(Manager &m, XRSLAMAmdTrackerParams *out) {
    if (!m.sys || !out) return 0;
    const xrh::Config &c = m.sys->P.config;   // (checked whole numbers: Pipeline::check_lk_params)
    out->lk_window_size = (int)c.feature_tracker_lk_window_size;
    out->lk_max_level = (int)c.feature_tracker_lk_max_level;
    out->lk_max_iterations = (int)c.feature_tracker_lk_max_iterations;
    out->lk_epsilon = c.feature_tracker_lk_epsilon;
    return 1;
}

void impl_get_init_report(Manager &m, XRSLAMAmdInitReport *out) {
    if (!m.sys || !out) return;
    const xrh::Initializer &in = m.sys->init;
    out->attempts = in.attempts;
    out->successes = in.successes;
    out->sfm_candidate = in.sfm_candidate;
    out->sfm_triangulated = (int)in.sfm_triangulated;
    out->scale = in.scale;
    for (int k = 0; k < 3; ++k) {
        out->gravity[k] = in.gravity[k];
        out->bg[k] = in.bg[k];
    }
}

}   // namespace

// An opaque handle for the instance-scoped entry points
struct XRSLAMAmdInstance {
    Manager m;
};
// ... and for a group of instances on one GPU whose per-frame launches are issued together (xrslam_hip.h: xrhip_group)
struct XRSLAMAmdGroup {
    xrhip_group *g = nullptr;
    int device = -1;
};

extern "C" {

// ---- the reference's six symbols: one process-global instance (XRSLAMManager.cpp:6-9)
int XRSLAMCreate(const char *slam_config_path, const char *device_config_path, const char *, const char *, void **config) {
    return impl_create(mgr(), slam_config_path, device_config_path, config);
}
void XRSLAMPushSensorData(XRSLAMSensorType type, void *data) { impl_push(mgr(), type, data); }
void XRSLAMRunOneFrame() { impl_run(mgr()); }
void XRSLAMSetViewer(void *) {}
void XRSLAMGetResult(XRSLAMResultType type, void *out) { impl_get_result(mgr(), type, out); }
void XRSLAMDestroy() { impl_destroy(mgr()); }

// ---- additive entry points on the process-global instance
void XRSLAMAmdSetInitialState(double t, const double q[4], const double p[3], const double v[3], const double bg[3],
                              const double ba[3]) {
    impl_set_initial_state(mgr(), t, q, p, v, bg, ba);
}
void XRSLAMAmdPushImageDevice(const void *gray_dev, int stride, double timestamp) {
    impl_push_image_device(mgr(), gray_dev, stride, timestamp);
}
void XRSLAMAmdPushImageDeviceColor(const void *pixels_dev, int stride, int channels, double timestamp) {
    impl_push_image_device(mgr(), pixels_dev, stride, timestamp, channels);
}
void XRSLAMAmdPushImageScaled(const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt, const XRSLAMAmdFrameGeometry *geo,
                              int on_device, double timestamp) {
    impl_push_image_scaled(mgr(), pixels, stride, fmt, geo, on_device, timestamp);
}
void XRSLAMAmdScaleIntrinsics(const double src[4], const XRSLAMAmdFrameGeometry *geo, int W, int H, double out[4]) {
    if (!src || !geo || !out || W < 1 || H < 1 || geo->crop_width < 1 || geo->crop_height < 1) return;
    xrh::scale_intrinsics(src, to_inner(*geo), W, H, out);
}
int XRSLAMAmdSetFrameOrientation(int orientation) { return impl_set_frame_orientation(mgr(), orientation); }
int XRSLAMAmdGetFrameOrientation(void) { return mgr().orientation.load(); }
int XRSLAMAmdOrientationFromExif(int exif) { return xrh::orientation_from_exif(exif); }
int XRSLAMAmdOrientIntrinsics(const double src[4], const XRSLAMAmdFrameGeometry *geo, int orientation, int W, int H, double out[4], double R[9]) {
    if (!src || !out || !R || W < 1 || H < 1 || !xrh::orientation_valid(orientation) || (geo && (geo->crop_width < 1 || geo->crop_height < 1))) return 0;
    const xrhip_frame_geometry g = geo ? to_inner(*geo) : xrhip_frame_geometry{};
    xrh::orient_intrinsics(src, geo ? &g : nullptr, orientation, W, H, out, R);
    return 1;
}
void XRSLAMAmdPushImageFormat(const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt, int on_device, double timestamp) {
    impl_push_image_format(mgr(), pixels, stride, fmt, on_device, timestamp);
}
void XRSLAMAmdGetCameraConfig(XRSLAMAmdCameraConfig *out) { impl_get_camera_config(mgr(), out); }
int XRSLAMAmdDescribeConfig(char *buf, int cap) { return impl_describe_config(mgr(), buf, cap); }
void XRSLAMAmdSetDeviceUndistort(const char *model) { impl_set_device_undistort(mgr(), model); }
void XRSLAMAmdGetTimes(XRSLAMAmdTimes *out) { impl_get_times(mgr(), out); }
void XRSLAMAmdSetProfiling(int enable) { impl_set_profiling(mgr(), enable); }
void XRSLAMAmdGetBaStats(void *out, int reset) { impl_get_ba_stats(mgr(), out, reset); }
void XRSLAMAmdGetKltStats(void *out, int reset) { impl_get_klt_stats(mgr(), out, reset); }
void XRSLAMAmdSetCovariance(int enable) { impl_set_covariance(mgr(), enable); }
int XRSLAMAmdGetCovariance(XRSLAMAmdCovariance *out) { return impl_get_covariance(mgr(), out); }
int XRSLAMAmdGetLandmarkVariances(double *var, long long *ids, int cap) { return impl_get_landmark_variances(mgr(), var, ids, cap); }
void XRSLAMAmdGetInitReport(XRSLAMAmdInitReport *out) { impl_get_init_report(mgr(), out); }
int XRSLAMAmdGetTrackerParams(XRSLAMAmdTrackerParams *out) { return impl_get_tracker_params(mgr(), out); }
const char *XRSLAMAmdLastError(void) { return mgr().last_error.c_str(); }
void XRSLAMAmdSetThreading(int mode) { impl_set_threading(mgr(), mode); }
int XRSLAMAmdSetMask(const void *mask, int stride, int on_device) { return impl_set_mask(mgr(), mask, stride, on_device); }
int XRSLAMAmdSetNextFrameMask(const void *mask, int stride, int on_device) { return impl_set_next_frame_mask(mgr(), mask, stride, on_device); }
void XRSLAMAmdFlush(void) { impl_flush(mgr()); }
int XRSLAMAmdGetFeatures(XRSLAMAmdFeature *out, int cap, double *timestamp) { return impl_get_features(mgr(), out, cap, timestamp); }
void XRSLAMAmdSetFeatureHistory(int frames) { impl_set_feature_history(mgr(), frames); }
int XRSLAMAmdRenderTrackingView(void *out, int stride, int channels, int on_device, const XRSLAMAmdViewOptions *opt) {
    return impl_render_view(mgr(), out, stride, channels, on_device, opt);
}

// ---- the same entry points on caller-owned instances (several sequences per process / per GPU)
int XRSLAMAmdInstanceCreate(const char *slam_config_path, const char *device_config_path, XRSLAMAmdInstance **out,
                            void **config) {
    if (!out) return 0;
    *out = nullptr;
    XRSLAMAmdInstance *inst = new (std::nothrow) XRSLAMAmdInstance();
    if (!inst) return 0;
    if (impl_create(inst->m, slam_config_path, device_config_path, config) != 1) {
        // the error text must outlive the failed instance: park it in the global one, where XRSLAMAmdLastError reads
        mgr().last_error = inst->m.last_error;
        delete inst;
        return 0;
    }
    *out = inst;
    return 1;
}
void XRSLAMAmdInstanceDestroy(XRSLAMAmdInstance *inst) {
    if (!inst) return;
    impl_destroy(inst->m);
    delete inst;
}
void XRSLAMAmdInstancePushSensorData(XRSLAMAmdInstance *inst, XRSLAMSensorType type, void *data) {
    if (inst) impl_push(inst->m, type, data);
}
void XRSLAMAmdInstanceRunOneFrame(XRSLAMAmdInstance *inst) {
    if (inst) impl_run(inst->m);
}
void XRSLAMAmdInstanceGetResult(XRSLAMAmdInstance *inst, XRSLAMResultType type, void *out) {
    if (inst) impl_get_result(inst->m, type, out);
}
void XRSLAMAmdInstanceSetInitialState(XRSLAMAmdInstance *inst, double t, const double q[4], const double p[3],
                                      const double v[3], const double bg[3], const double ba[3]) {
    if (inst) impl_set_initial_state(inst->m, t, q, p, v, bg, ba);
}
void XRSLAMAmdInstancePushImageDevice(XRSLAMAmdInstance *inst, const void *gray_dev, int stride, double timestamp) {
    if (inst) impl_push_image_device(inst->m, gray_dev, stride, timestamp);
}
void XRSLAMAmdInstancePushImageDeviceColor(XRSLAMAmdInstance *inst, const void *pixels_dev, int stride, int channels,
                                           double timestamp) {
    if (inst) impl_push_image_device(inst->m, pixels_dev, stride, timestamp, channels);
}
void XRSLAMAmdInstancePushImageScaled(XRSLAMAmdInstance *inst, const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt,
                                      const XRSLAMAmdFrameGeometry *geo, int on_device, double timestamp) {
    if (inst) impl_push_image_scaled(inst->m, pixels, stride, fmt, geo, on_device, timestamp);
}
void XRSLAMAmdInstancePushImageFormat(XRSLAMAmdInstance *inst, const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt,
                                      int on_device, double timestamp) {
    if (inst) impl_push_image_format(inst->m, pixels, stride, fmt, on_device, timestamp);
}
int XRSLAMAmdInstanceSetFrameOrientation(XRSLAMAmdInstance *inst, int orientation) {
    return inst ? impl_set_frame_orientation(inst->m, orientation) : 0;
}
int XRSLAMAmdInstanceGetFrameOrientation(XRSLAMAmdInstance *inst) { return inst ? inst->m.orientation.load() : 0; }
void XRSLAMAmdInstanceGetCameraConfig(XRSLAMAmdInstance *inst, XRSLAMAmdCameraConfig *out) {
    if (inst) impl_get_camera_config(inst->m, out);
}
int XRSLAMAmdInstanceDescribeConfig(XRSLAMAmdInstance *inst, char *buf, int cap) {
    return inst ? impl_describe_config(inst->m, buf, cap) : 0;
}
void XRSLAMAmdInstanceSetDeviceUndistort(XRSLAMAmdInstance *inst, const char *model) {
    if (inst) impl_set_device_undistort(inst->m, model);
}
void XRSLAMAmdInstanceGetTimes(XRSLAMAmdInstance *inst, XRSLAMAmdTimes *out) {
    if (inst) impl_get_times(inst->m, out);
}
void XRSLAMAmdInstanceSetProfiling(XRSLAMAmdInstance *inst, int enable) {
    if (inst) impl_set_profiling(inst->m, enable);
}
void XRSLAMAmdInstanceGetBaStats(XRSLAMAmdInstance *inst, void *out, int reset) {
    if (inst) impl_get_ba_stats(inst->m, out, reset);
}
void XRSLAMAmdInstanceGetKltStats(XRSLAMAmdInstance *inst, void *out, int reset) {
    if (inst) impl_get_klt_stats(inst->m, out, reset);
}
void XRSLAMAmdInstanceGetInitReport(XRSLAMAmdInstance *inst, XRSLAMAmdInitReport *out) {
    if (inst) impl_get_init_report(inst->m, out);
}
int XRSLAMAmdInstanceGetTrackerParams(XRSLAMAmdInstance *inst, XRSLAMAmdTrackerParams *out) {
    return inst ? impl_get_tracker_params(inst->m, out) : 0;
}
void XRSLAMAmdInstanceSetCovariance(XRSLAMAmdInstance *inst, int enable) {
    if (inst) impl_set_covariance(inst->m, enable);
}
int XRSLAMAmdInstanceGetCovariance(XRSLAMAmdInstance *inst, XRSLAMAmdCovariance *out) {
    if (inst) return impl_get_covariance(inst->m, out);
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->status = -1;
    }
    return 0;
}
int XRSLAMAmdInstanceGetLandmarkVariances(XRSLAMAmdInstance *inst, double *var, long long *ids, int cap) {
    return inst ? impl_get_landmark_variances(inst->m, var, ids, cap) : 0;
}
const char *XRSLAMAmdInstanceLastError(XRSLAMAmdInstance *inst) { return inst ? inst->m.last_error.c_str() : ""; }
void XRSLAMAmdInstanceSetThreading(XRSLAMAmdInstance *inst, int mode) {
    if (inst) impl_set_threading(inst->m, mode);
}
int XRSLAMAmdInstanceSetMask(XRSLAMAmdInstance *inst, const void *mask, int stride, int on_device) {
    return inst ? impl_set_mask(inst->m, mask, stride, on_device) : 0;
}
int XRSLAMAmdInstanceSetNextFrameMask(XRSLAMAmdInstance *inst, const void *mask, int stride, int on_device) {
    return inst ? impl_set_next_frame_mask(inst->m, mask, stride, on_device) : 0;
}
void XRSLAMAmdInstanceFlush(XRSLAMAmdInstance *inst) {
    if (inst) impl_flush(inst->m);
}

int XRSLAMAmdInstanceGetFeatures(XRSLAMAmdInstance *inst, XRSLAMAmdFeature *out, int cap, double *timestamp) {
    return inst ? impl_get_features(inst->m, out, cap, timestamp) : 0;
}
void XRSLAMAmdInstanceSetFeatureHistory(XRSLAMAmdInstance *inst, int frames) {
    if (inst) impl_set_feature_history(inst->m, frames);
}
int XRSLAMAmdInstanceRenderTrackingView(XRSLAMAmdInstance *inst, void *out, int stride, int channels, int on_device,
                                        const XRSLAMAmdViewOptions *opt) {
    return inst ? impl_render_view(inst->m, out, stride, channels, on_device, opt) : 0;
}

// ---- instance groups
int XRSLAMAmdGroupCreate(XRSLAMAmdGroup **out) {
    if (!out) return 0;
    *out = nullptr;
    XRSLAMAmdGroup *grp = new (std::nothrow) XRSLAMAmdGroup();
    if (!grp) return 0;
    if (xrhip_get_device(&grp->device) != 0) grp->device = -1;
    if (xrhip_group_create(&grp->g) != 0) {
        mgr().last_error = xrhip_last_error();
        delete grp;
        return 0;
    }
    *out = grp;
    return 1;
}
int XRSLAMAmdGroupDestroy(XRSLAMAmdGroup *grp) {
    if (!grp) return 1;
    if (grp->device >= 0) xrhip_bind_device(grp->device);
    if (xrhip_group_destroy(grp->g) != 0) {   // instances are still joined: the group stays
        mgr().last_error = xrhip_last_error();
        return 0;
    }
    delete grp;
    return 1;
}
int XRSLAMAmdInstanceJoinGroup(XRSLAMAmdInstance *inst, XRSLAMAmdGroup *grp) {
    if (!inst || !inst->m.sys) return 0;
    if (grp && inst->m.next_mask_set) return mask_refused(inst->m, "XRSLAMAmdInstanceJoinGroup: a mask is waiting for the next frame; a masked instance cannot join a group");
    int ok = 0;
    bind_device(inst->m);
    guarded(inst->m, [&] {
        inst->m.sys->resolve_device_work();
        inst->m.sys->P.join_group(grp ? grp->g : nullptr);
        ok = 1;
    });
    return ok;
}
void XRSLAMAmdGroupSetProfiling(XRSLAMAmdGroup *grp, int enable) {
    if (grp) xrhip_group_set_profiling(grp->g, enable);
}
void XRSLAMAmdGroupGetStats(XRSLAMAmdGroup *grp, void *out, int reset) {
    if (grp && out) xrhip_group_get_stats(grp->g, static_cast<xrhip_group_stats *>(out), reset);
}

// The player's loop (xrslam-pc/player/src/main.cpp:116-169) for n_steps camera frames of a pre-staged sequence, without a
// host-language round trip per sensor sample: at equal timestamps gyroscope, then accelerometer, then camera
// (IO/async_dataset_reader.cpp:41-48); RunOneFrame and the state / pose query after every image.
// (frame: what every frame is -- stride, format, geometry, host or HBM; its pixels are frames + k * frame_bytes)
static int replay(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames, const void *frames,
                  size_t frame_bytes, xrh::FrameInput frame, int *imu_cursor, int *frame_cursor, int n_steps, double *poses_out8) {
    if (!inst || !imu7 || !cam_t || !frames || !imu_cursor || !frame_cursor) return -1;
    Manager &m = inst->m;
    int n_poses = 0;
    // one hipSetDevice for the loop instead of one per pushed sample (~22 per frame); nothing in between runs foreign code on this thread
    bind_device(m);
    struct Bound {
        Manager &m;
        explicit Bound(Manager &mm) : m(mm) { m.bound_by_replay = true; }
        ~Bound() { m.bound_by_replay = false; }
    } bound(m);
    for (int s = 0; s < n_steps && *frame_cursor < n_frames; ++s) {
        const int fk = *frame_cursor;
        const double t = cam_t[fk], lim = t + 1e-9;
        int k = *imu_cursor;
        while (k < n_imu && imu7[7 * (size_t)k] <= lim) {
            const double *r = imu7 + 7 * (size_t)k;
            XRSLAMGyroscope g;
            g.data[0] = r[1]; g.data[1] = r[2]; g.data[2] = r[3]; g.timestamp = r[0];
            XRSLAMAcceleration a;
            a.data[0] = r[4]; a.data[1] = r[5]; a.data[2] = r[6]; a.timestamp = r[0];
            impl_push(m, XRSLAM_SENSOR_GYROSCOPE, &g);
            impl_push(m, XRSLAM_SENSOR_ACCELERATION, &a);
            ++k;
        }
        *imu_cursor = k;
        frame.pixels = static_cast<const uint8_t *>(frames) + (size_t)fk * frame_bytes;
        push_frame(m, frame, t);
        impl_run(m);
        XRSLAMState state = XRSLAM_STATE_INITIALIZING;
        impl_get_result(m, XRSLAM_RESULT_STATE, &state);
        if (state == XRSLAM_STATE_TRACKING_SUCCESS && poses_out8) {
            XRSLAMPose pose;
            impl_get_result(m, XRSLAM_RESULT_BODY_POSE, &pose);
            double *o = poses_out8 + 8 * (size_t)n_poses++;
            o[0] = pose.timestamp;
            for (int i = 0; i < 3; ++i) o[1 + i] = pose.translation[i];
            for (int i = 0; i < 4; ++i) o[4 + i] = pose.quaternion[i];
        }
        *frame_cursor = fk + 1;
    }
    return n_poses;
}

int XRSLAMAmdInstanceReplayColor(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                                 const void *frames, size_t frame_bytes, int stride, int channels, int on_device,
                                 int *imu_cursor, int *frame_cursor, int n_steps, double *poses_out8) {
    return replay(inst, imu7, n_imu, cam_t, n_frames, frames, frame_bytes, frame_input(nullptr, stride, on_device, channels, nullptr), imu_cursor,
                  frame_cursor, n_steps, poses_out8);
}

int XRSLAMAmdInstanceReplayFormat(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                                  const void *frames, size_t frame_bytes, int stride, const XRSLAMAmdFrameFormat *fmt, int on_device,
                                  int *imu_cursor, int *frame_cursor, int n_steps, double *poses_out8) {
    if (!fmt) return -1;
    return replay(inst, imu7, n_imu, cam_t, n_frames, frames, frame_bytes, frame_input(nullptr, stride, on_device, 1, fmt), imu_cursor,
                  frame_cursor, n_steps, poses_out8);
}

int XRSLAMAmdInstanceReplayScaled(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                                  const void *frames, size_t frame_bytes, int stride, const XRSLAMAmdFrameFormat *fmt,
                                  const XRSLAMAmdFrameGeometry *geo, int on_device, int *imu_cursor, int *frame_cursor, int n_steps,
                                  double *poses_out8) {
    if (!geo) return -1;
    const xrhip_frame_geometry g = to_inner(*geo);
    return replay(inst, imu7, n_imu, cam_t, n_frames, frames, frame_bytes, frame_input(nullptr, stride, on_device, 1, fmt, &g), imu_cursor,
                  frame_cursor, n_steps, poses_out8);
}

int XRSLAMAmdInstanceReplay(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                            const void *frames, size_t frame_bytes, int stride, int on_device, int *imu_cursor,
                            int *frame_cursor, int n_steps, double *poses_out8) {
    return XRSLAMAmdInstanceReplayColor(inst, imu7, n_imu, cam_t, n_frames, frames, frame_bytes, stride, 1, on_device, imu_cursor,
                                        frame_cursor, n_steps, poses_out8);
}

}   // extern "C"
