/*
 * XRSLAM.h -- outer C ABI of the MI355X-native XRSLAM hot path.
 *
 * Binary-compatible with the reference's public interface
 * (/root/reference/xrslam-interface/include/XRSLAM.h:19-229): same exported symbols,
 * enum values and POD layouts, so a host application built against the reference
 * (xrslam-pc/player/src/main.cpp:116-169, xrslam-ros/src/xrslam_node.cpp:44) links
 * against libxrslam_hip.so unchanged.  Implementation: xrslam_amd/csrc/host/xrslam_api.cpp.
 *
 * Differences, all additive:
 *   - the XRSLAMAmd* entry points at the bottom (optional externally supplied initial
 *     states, device-resident images, stage timers, initialiser report), and their
 *     XRSLAMAmdInstance* forms for several sequences per process;
 *   - XRSLAMFeatures is declared for C++ only, like the reference (it holds a std::vector).
 */
#ifndef XRSLAM_AMD_XRSLAM_H
#define XRSLAM_AMD_XRSLAM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
#include <vector>
extern "C" {
#endif

/* ---- sensor inputs ---- */
typedef enum XRSLAMSensorType {
    XRSLAM_SENSOR_CAMERA = 0,
    XRSLAM_SENSOR_DEPTH_CAMERA,
    XRSLAM_SENSOR_ACCELERATION,
    XRSLAM_SENSOR_GYROSCOPE,
    XRSLAM_SENSOR_GRAVITY,
    XRSLAM_SENSOR_ROTATION_VECTOR,
    XRSLAM_SENSOR_UNKNOWN
} XRSLAMSensorType;

typedef struct XRSLAMImageExtension {
    double exposure_time, default_focus_distance, focal_length, focus_distance;
} XRSLAMImageExtension;

typedef struct XRSLAMImage {
    unsigned char *data; /* 8-bit pixels */
    double timeStamp;    /* seconds */
    int stride;          /* bytes per row */
    int camera_id;       /* only 0 is consumed */
    int channel;         /* 1 (gray), 3 (BGR) or 4 (BGRA) */
    XRSLAMImageExtension *ext;
} XRSLAMImage;

typedef struct XRSLAMDepthImage {
    uint16_t *data, *confidence;
    double timeStamp;
} XRSLAMDepthImage;

typedef struct XRSLAMAcceleration {
    double data[3];
    double timestamp;
} XRSLAMAcceleration;
typedef struct XRSLAMGyroscope {
    double data[3];
    double timestamp;
} XRSLAMGyroscope;
typedef struct XRSLAMGravity {
    double data[3];
    double timestamp;
} XRSLAMGravity;
typedef struct XRSLAMRotationVector {
    double data[4];
    double timestamp;
} XRSLAMRotationVector;

/* ---- results ---- */
typedef enum XRSLAMResultType {
    XRSLAM_RESULT_BODY_POSE = 0,
    XRSLAM_RESULT_CAMERA_POSE,
    XRSLAM_RESULT_STATE,
    XRSLAM_RESULT_LANDMARKS,
    XRSLAM_RESULT_FEATURES,
    XRSLAM_RESULT_BIAS,
    XRSLAM_RESULT_DEBUG_LOGS,
    XRSLAM_RESULT_VERSION,
    XRSLAM_RESULT_UNKNOWN,
    XRSLAM_INFO_INTRINSICS
} XRSLAMResultType;

typedef struct XRSLAMPose {
    double quaternion[4];  /* x y z w */
    double translation[3];
    double timestamp;
} XRSLAMPose;

typedef struct XRSLAMIntrinsics {
    double fx, fy, cx, cy;
} XRSLAMIntrinsics;

typedef enum XRSLAMState {
    XRSLAM_STATE_INITIALIZING,
    XRSLAM_STATE_TRACKING_SUCCESS,
    XRSLAM_STATE_TRACKING_FAIL
} XRSLAMState;

typedef struct XRSLAMLandmark {
    double x, y, z;
} XRSLAMLandmark;
typedef struct XRSLAMLandmarks {
    XRSLAMLandmark *landmarks;
    int num_landmarks;
} XRSLAMLandmarks;

typedef struct XRSLAMFeature {
    double x, y;
} XRSLAMFeature;
#ifdef __cplusplus
typedef struct XRSLAMFeatures {
    struct Point {
        double x;
        double y;
    };
    std::vector<Point> pos;
} XRSLAMFeatures;
#endif

typedef struct XRSLAMBias {
    double data[3];
} XRSLAMBias;
typedef struct XRSLAMIMUBias {
    XRSLAMBias acc_bias;
    XRSLAMBias gyr_bias;
} XRSLAMIMUBias;

typedef struct XRSLAMStringOutput {
    int str_length;
    char *data;
} XRSLAMStringOutput;

/* ---- entry points (reference XRSLAM.h:201-229) ---- */
/* returns 1 on success, 0 otherwise; *config receives an opaque configuration handle owned by the library */
int XRSLAMCreate(const char *slam_config_path, const char *device_config_path, const char *license_path,
                 const char *product_name, void **config);
void XRSLAMPushSensorData(XRSLAMSensorType sensor_type, void *sensor_data);
void XRSLAMRunOneFrame();
void XRSLAMSetViewer(void *viewer); /* declared by the reference, defined nowhere there; a no-op here */
void XRSLAMGetResult(XRSLAMResultType result_type, void *result_data);
void XRSLAMDestroy();

/* ---- additive MI355X entry points ---- */
/* Optional: body pose/velocity/biases at image time t (q: x y z w).  While any such state is registered the
 * first window is seeded from them (poses of its 8 keyframes) instead of SfM + IMU alignment
 * (core/initializer.cpp:158-571); with none registered the library initialises itself like the reference. */
void XRSLAMAmdSetInitialState(double t, const double q[4], const double p[3], const double v[3],
                              const double bg[3], const double ba[3]);
/* like XRSLAM_SENSOR_CAMERA but `gray_dev` is an 8-bit single-channel image already resident in HBM */
void XRSLAMAmdPushImageDevice(const void *gray_dev, int stride, double timestamp);
/* Colour frames.  XRSLAM_SENSOR_CAMERA accepts channel 3 (BGR) and 4 (BGRA, byte 3 ignored) like the reference's PushImage
 * (cv::cvtColor); the frame is reduced to gray on the GPU as part of its upload, gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14.
 * This is the same for an interleaved 8-bit colour frame already resident in HBM (a decoder's or an ISP's output):
 * channels 3 or 4 (1: same as XRSLAMAmdPushImageDevice), stride in bytes >= width * channels, any base alignment.  With device
 * undistortion switched on the frame is reduced first and rectified second. */
void XRSLAMAmdPushImageDeviceColor(const void *pixels_dev, int stride, int channels, double timestamp);
/* Frames in the layouts cameras, decoders and ROS deliver, from host memory (on_device 0) or HBM, reduced to the 8-bit gray plane the
 * tracker works on as part of the frame's upload; all integer, per pixel:
 *   GRAY8           the byte                         BGR8 / BGRA8   as XRSLAM_SENSOR_CAMERA channel 3 / 4
 *   RGB8 / RGBA8    (R*4899 + G*9617 + B*1868 + 8192) >> 14, byte 3 ignored
 *   GRAY16          little endian, `bits` significant (8..16, 0 = 16): min(255, v >> (bits - 8)); 16: the high byte
 *   YUYV / UYVY     packed 4:2:2, the Y byte of each pixel's pair (byte 0 / byte 1)
 *   NV12 / I420     the luma plane: `stride` is that plane's, and only its `height` rows are read (push a decoder's surface as is)
 *   P010            the high byte of the luma plane's 16-bit samples; only `height` rows of that plane are read
 *   BAYER_*8 / *16  a raw colour-filter mosaic of 8-bit / little-endian 16-bit samples (`bits` as GRAY16).  The name is the frame's
 *                   top-left 2 x 2 tile read row by row (RGGB: (0,0) red, (1,0) green, (0,1) green, (1,1) blue -- the GenICam / V4L2 /
 *                   ROS bayer_* convention; OpenCV's COLOR_Bayer* names are shifted by one pixel against it).  Demosaiced bilinearly,
 *                   neighbours mirrored at the frame's (a scaled frame: the crop's) edges, and weighted like BGR8, in exact integer
 *                   arithmetic with one rounding (include/xrslam_hip.h has the formula); a constant mosaic gives that constant
 *   GRAY10_MIPI / GRAY12_MIPI / GRAY10P / GRAY12P and BAYER_<pattern>{10_MIPI, 12_MIPI, 10P, 12P}
 *                   bit-packed 10 / 12-bit samples as sensors send them: CSI-2 RAW10 / RAW12 (4 pixels in 5 bytes / 2 in 3, the low
 *                   bits in the group's last byte; V4L2 Y10P, Y12P, pRAA, pRCC ...) and the PFNC lsb-packed forms (Mono10p,
 *                   Mono12p, BayerRG10p ...: the row is one little-endian bit stream).  `stride` >= the packed row's bytes
 *                   (5 * ceil(w/4), 3 * ceil(w/2), ceil(10w/8), ceil(12w/8)); `bits` is not read.  The result is, bit for bit, that of
 *                   the same samples pushed as GRAY16 / BAYER_<pattern>16 with bits 10 / 12 (include/xrslam_hip.h has the byte
 *                   layouts).  Not supported: GigE Vision's legacy Mono10Packed / Mono12Packed, msb-packed or big-endian PFNC
 *                   forms, 14-bit packings
 * limited_range (video levels, luma 16..235; not for the RGB / BGR and Bayer formats): gray' = min(255, ((max(gray,16) - 16) * 255 + 109) / 219).
 * Any base alignment, any stride >= width * bytes per pixel (the packed forms: the row's bytes).  With device undistortion on: reduced first, rectified second.  A bad
 * format, bits, stride or flag drops the frame and sets XRSLAMAmdLastError; nothing aborts. */
typedef enum XRSLAMAmdPixelFormat {
    XRSLAM_AMD_PIXEL_GRAY8 = 0,
    XRSLAM_AMD_PIXEL_BGR8,
    XRSLAM_AMD_PIXEL_BGRA8,
    XRSLAM_AMD_PIXEL_RGB8,
    XRSLAM_AMD_PIXEL_RGBA8,
    XRSLAM_AMD_PIXEL_GRAY16,
    XRSLAM_AMD_PIXEL_YUYV,
    XRSLAM_AMD_PIXEL_UYVY,
    XRSLAM_AMD_PIXEL_NV12,
    XRSLAM_AMD_PIXEL_I420,
    XRSLAM_AMD_PIXEL_P010,
    /* (11..15 are not formats) */
    XRSLAM_AMD_PIXEL_BAYER_RGGB8 = 16,
    XRSLAM_AMD_PIXEL_BAYER_GRBG8 = 17,
    XRSLAM_AMD_PIXEL_BAYER_GBRG8 = 18,
    XRSLAM_AMD_PIXEL_BAYER_BGGR8 = 19,
    XRSLAM_AMD_PIXEL_BAYER_RGGB16 = 20,
    XRSLAM_AMD_PIXEL_BAYER_GRBG16 = 21,
    XRSLAM_AMD_PIXEL_BAYER_GBRG16 = 22,
    XRSLAM_AMD_PIXEL_BAYER_BGGR16 = 23,
    /* (24..31 are not formats) */
    XRSLAM_AMD_PIXEL_GRAY10_MIPI = 32,
    XRSLAM_AMD_PIXEL_GRAY12_MIPI = 33,
    XRSLAM_AMD_PIXEL_GRAY10P = 34,
    XRSLAM_AMD_PIXEL_GRAY12P = 35,
    /* (36..39 are not formats)  BAYER_<pattern><packing> = 40 + 4 * packing + pattern */
    XRSLAM_AMD_PIXEL_BAYER_RGGB10_MIPI = 40,
    XRSLAM_AMD_PIXEL_BAYER_GRBG10_MIPI = 41,
    XRSLAM_AMD_PIXEL_BAYER_GBRG10_MIPI = 42,
    XRSLAM_AMD_PIXEL_BAYER_BGGR10_MIPI = 43,
    XRSLAM_AMD_PIXEL_BAYER_RGGB12_MIPI = 44,
    XRSLAM_AMD_PIXEL_BAYER_GRBG12_MIPI = 45,
    XRSLAM_AMD_PIXEL_BAYER_GBRG12_MIPI = 46,
    XRSLAM_AMD_PIXEL_BAYER_BGGR12_MIPI = 47,
    XRSLAM_AMD_PIXEL_BAYER_RGGB10P = 48,
    XRSLAM_AMD_PIXEL_BAYER_GRBG10P = 49,
    XRSLAM_AMD_PIXEL_BAYER_GBRG10P = 50,
    XRSLAM_AMD_PIXEL_BAYER_BGGR10P = 51,
    XRSLAM_AMD_PIXEL_BAYER_RGGB12P = 52,
    XRSLAM_AMD_PIXEL_BAYER_GRBG12P = 53,
    XRSLAM_AMD_PIXEL_BAYER_GBRG12P = 54,
    XRSLAM_AMD_PIXEL_BAYER_BGGR12P = 55
} XRSLAMAmdPixelFormat;
typedef struct XRSLAMAmdFrameFormat {
    int format;          /* XRSLAMAmdPixelFormat */
    int bits;            /* GRAY16, BAYER_*16: significant bits, 8..16; 0 = 16.  Not read for the other formats (the packed ones carry theirs). */
    int limited_range;   /* 1: video levels, expanded to 0..255 */
} XRSLAMAmdFrameFormat;
void XRSLAMAmdPushImageFormat(const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt, int on_device, double timestamp);
/* Frames larger than cam0.resolution.  The tracker works at the configured resolution W x H; a camera or a video decoder delivers
 * 1280x720, 1920x1080, 3840x2160.  The crop rectangle of such a frame -- any XRSLAMAmdFrameFormat, host memory or HBM -- is cropped
 * and area-averaged down to W x H on the GPU as part of the frame's upload, all in integers: a working pixel is the exact mean of
 * the per-pixel gray values (format reduction first) over its footprint in the crop, rounded half up; the two axes scale
 * independently (include/xrslam_hip.h: xrhip_image_upload_scaled has the formula).  `pixels` is row 0 of the source frame, `stride`
 * its row pitch in bytes; only the crop's bytes are read, and of a host frame only the crop crosses the host link.
 * Required: the crop inside the source, W <= crop_width, H <= crop_height (no upscaling), crop_width * crop_height <= 2^24,
 * stride >= src_width * bytes per pixel.  A bad geometry drops the frame and sets XRSLAMAmdLastError; nothing aborts.
 * cam0.intrinsics / distortion / resolution describe the WORKING image, as always: with device undistortion on the frame is scaled
 * first and rectified second, and the library does not rewrite the configuration.  XRSLAMAmdScaleIntrinsics maps the source
 * camera's {fx, fy, cx, cy} through a geometry (pixel centres at integer coordinates): fx' = fx*W/cw, fy' = fy*H/ch,
 * cx' = (cx + 0.5 - crop_x)*W/cw - 0.5, cy' = (cy + 0.5 - crop_y)*H/ch - 0.5; distortion coefficients are unchanged. */
typedef struct XRSLAMAmdFrameGeometry {
    int src_width, src_height;                      /* the frame as it lies in memory */
    int crop_x, crop_y, crop_width, crop_height;    /* the rectangle that becomes the working image */
} XRSLAMAmdFrameGeometry;
void XRSLAMAmdPushImageScaled(const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt /* NULL = GRAY8 */,
                              const XRSLAMAmdFrameGeometry *geo, int on_device, double timestamp);
void XRSLAMAmdScaleIntrinsics(const double src[4], const XRSLAMAmdFrameGeometry *geo, int W, int H, double out[4]);
/* Frames from a sensor mounted a quarter turn against the device, hung upside down, read out with its mirror / flip register set, or
 * delivered by a decoder with an EXIF / display-matrix orientation: turned on the GPU as part of the frame's upload.  How the camera
 * is mounted is a property of the instance, so the orientation is a sticky setting (default 0) that every push and replay entry point
 * honours, XRSLAMPushSensorData(XRSLAM_SENSOR_CAMERA) included; it is bound to a frame when the frame is pushed (pipelined mode too).
 * An orientation is o = r + 4 f, 0 .. 7, applied to the gray crop c(i, j), 0 <= i < cw, 0 <= j < ch (after format reduction /
 * demosaicing and cropping, before scaling):
 *   f set: mirrored left to right first     c'(i, j) = c(cw-1-i, j)
 *   then r quarter turns CLOCKWISE          r = 1: u(X, Y) = c'(Y, ch-1-X);  r = 2: u(X, Y) = c'(cw-1-X, ch-1-Y);  r = 3: u(X, Y) = c'(cw-1-Y, X)
 * u (ch x cw for odd r) is then scaled to the working image W x H, and rectified if device undistortion is on.  An unscaled frame is
 * therefore H x W in memory for odd r (stride >= H * bytes per pixel); a scaled one needs W <= the turned crop's width and H <= its
 * height.  Masks and the tracking view describe the working image and are untouched.  SetFrameOrientation returns 1, or 0 with the
 * reason in XRSLAMAmdLastError for a value outside 0 .. 7 (the setting stays); a frame that does not fit the orientation is dropped
 * like any other bad frame, and nothing aborts.
 * cam0.* describe the WORKING image, as always, and the library does not rewrite the configuration.  Two helpers, pure host code:
 *   XRSLAMAmdOrientationFromExif  EXIF tag 274 -> o:  1->0, 6->1, 3->2, 8->3, 2->4, 7->5, 4->6, 5->7;  -1 for a value outside 1 .. 8.
 *   XRSLAMAmdOrientIntrinsics     maps the source camera's {fx, fy, cx, cy} through crop, orientation and scale (pixel centres at
 *     integer coordinates; geo NULL: the whole frame, W x H, or H x W for odd r).  A crop pixel (i, j) = (u - crop_x, v - crop_y)
 *     lands at (X, Y) in u:  i' = f ? cw-1-i : i;  r = 0: (i', j);  1: (ch-1-j, i');  2: (cw-1-i', ch-1-j);  3: (j, cw-1-i').
 *     That map is (X, Y)^T = P (i, j)^T + t with P a signed permutation; with (tw, th) = u's size, sx = W/tw, sy = H/th:
 *       (fx', fy') = (sx, sy) * |P| (fx, fy)      (fx and fy change places for odd r)
 *       (cx', cy') = (sx, sy) * (P (cx - crop_x, cy - crop_y)^T + t + 0.5) - 0.5
 *     R (row-major 3 x 3) = [P 0; 0 1] takes a ray of the source camera to the working camera's: a rotation about the optical axis, a
 *     reflection for f = 1; the caller composes it into cam0.extrinsic.  Returns 1, or 0 for a bad argument (nothing written).
 * Limit: distortion coefficients belong to the working image.  Radial terms survive a turn (they depend on the radius alone),
 * tangential ones (p1, p2) do not, and the library does not convert them. */
int XRSLAMAmdSetFrameOrientation(int orientation);
int XRSLAMAmdGetFrameOrientation(void);
int XRSLAMAmdOrientationFromExif(int exif);
int XRSLAMAmdOrientIntrinsics(const double src[4], const XRSLAMAmdFrameGeometry *geo /* NULL: whole frame */, int orientation, int W, int H,
                              double out[4], double R[9]);
/* What the reference's dataset readers ask the YamlConfig* for (xrslam-pc/player/src/IO/euroc_dataset_reader.cpp:4-7,16,62-66;
 * tum_dataset_reader.cpp:4-6,67-76): camera_time_offset(), camera_distortion_flag(), camera_distortion(),
 * camera_intrinsic(), camera_resolution().  The `config` out-parameter of XRSLAMCreate is an opaque handle here (the
 * reference hands out a C++ object whose virtuals the player calls -- not something a C ABI can promise), so a reader that
 * is built against this library takes those five values from this call instead (INTEGRATION.md section 1 shows the patch). */
typedef struct XRSLAMAmdCameraConfig {
    double time_offset;       /* cam0.time_offset */
    int distortion_flag;      /* cam0.camera_distortion_flag */
    double distortion[4];     /* cam0.distortion: k1 k2 p1 p2 (radtan) or k1..k4 (equidistant) */
    double intrinsics[4];     /* cam0.intrinsics: fx fy cx cy */
    int resolution[2];        /* cam0.resolution: width height */
} XRSLAMAmdCameraConfig;
void XRSLAMAmdGetCameraConfig(XRSLAMAmdCameraConfig *out);
/* Every value the two configuration files resolved to (the accessors of xrslam::Config, xrslam/include/xrslam/xrslam.h:36-116 /
 * yaml_config.cpp:152-362), one "key = value" line each (%.17g), keys as in the yaml files ("cam0.intrinsics", "sliding_window.size",
 * ...): lets a caller -- and tests/test_config.py -- check that two sets of files mean the same configuration.  Writes at most cap - 1
 * characters plus the terminator; returns the length the full text needs. */
int XRSLAMAmdDescribeConfig(char *buf, int cap);
/* Lucas-Kanade parameters of the tracker.  The reference hard-codes them in OpenCvImage::track_keypoints (winSize 21 x 21, maxLevel 3,
 * 30 iterations, epsilon 0.01: opencv_image.cpp:96-99), tuned for roughly VGA frames.  Four OPTIONAL keys of the slam yaml -- extensions,
 * the reference's files do not have them and load as before; an absent key means the reference's constant:
 *   feature_tracker.lk_window_size     odd, 5..21
 *   feature_tracker.lk_max_level       0..5; level lk_max_level of the working image (each level (n + 1) / 2) must be larger than the
 *                                      window in both dimensions
 *   feature_tracker.lk_max_iterations  1..100
 *   feature_tracker.lk_epsilon         0..10
 * A value outside these rules makes XRSLAMCreate / XRSLAMAmdInstanceCreate fail with the reason in XRSLAMAmdLastError.  Values other
 * than the reference's run the tracker's kernels with runtime parameters (xrslam_hip.h: xrhip_klt_set_lk_params) and such an instance
 * cannot join a group (XRSLAMAmdInstanceJoinGroup fails).  XRSLAMAmdDescribeConfig prints the four keys only for a file that has one
 * of them.  Returns 1 with the values in use, 0 when there is no instance. */
typedef struct XRSLAMAmdTrackerParams {
    int lk_window_size, lk_max_level, lk_max_iterations;
    double lk_epsilon;
} XRSLAMAmdTrackerParams;
int XRSLAMAmdGetTrackerParams(XRSLAMAmdTrackerParams *out);
/* Undistortion on the device.  The reference's readers rectify every frame on the host before pushing it
 * (cv::undistort, xrslam-pc/player/src/IO/euroc_dataset_reader.cpp:62-69; xrslam::extra::ImageUndistorter,
 * IO/tum_dataset_reader.cpp:67-76).  After this call the images handed to XRSLAM_SENSOR_CAMERA / XRSLAMAmdPushImageDevice
 * are taken as the camera recorded them and rectified on the GPU with cam0.intrinsics / cam0.distortion of the device
 * configuration -- bit-identical to the host path (the map is built once, on the host, in the reference's arithmetic).
 * model: "cv_undistort" (EuRoC reader), "radtan" or "equidistant" (ImageUndistorter); NULL or "" switches it off. */
void XRSLAMAmdSetDeviceUndistort(const char *model);
typedef struct XRSLAMAmdTimes {
    long frames, solves, solve_iterations, marginalizations, keyframes;
    double ba_device_ms; /* sum of xrhip_ba_summary.ms_solve (staging + kernels + result read-back of every solve) */
    /* host wall-clock seconds inside the inner C-ABI calls (preprocess, track, detect, preintegrate, solve,
     * marginalize) and in the whole per-frame work (FeatureTracker::work incl. the backend) */
    double wall_preprocess, wall_track, wall_detect, wall_preintegrate, wall_solve, wall_marginalize, wall_frame;
    /* host wall-clock seconds of whole pipeline stages (their device waits included): Frame::track_keypoints,
     * of which 5-pt RANSAC, 2-pt RANSAC; Frame::detect_keypoints; mirror_frame; localize_newframe; manage_keyframe;
     * track_landmark; refine_window; slide_window; refine_subwindow; initialiser (SfM + alignment attempts);
     * [12], [13] are COUNTS of the RD-VIO filter (parsac.parsac_flag): frames on which judge_track_status separated a
     * dynamic group, landmark observations it tagged as outliers; [14] COUNTS the constant copies the solver front end made for
     * prior factors whose reference frame / landmark was also a free parameter of the same solve; [15] pipelined mode
     * (XRSLAMAmdSetThreading): seconds the feature tracker waited for the previous frame's backend at the hand-off */
    double wall_scope[16];
} XRSLAMAmdTimes;
void XRSLAMAmdGetTimes(XRSLAMAmdTimes *out);
/* HIP-event profiling of the KLT kernels (off by default) and its accumulated counters; the struct is
 * xrhip_klt_stats from xrslam_hip.h (passed as void* to keep this header free of that include) */
void XRSLAMAmdSetProfiling(int enable);
void XRSLAMAmdGetKltStats(void *xrhip_klt_stats_out, int reset);
/* same for the BA context: xrhip_ba_stats from xrslam_hip.h (XRSLAMAmdSetProfiling switches both) */
void XRSLAMAmdGetBaStats(void *xrhip_ba_stats_out, int reset);
/* Covariance of the estimate (replaces: nothing the reference has; its users ask ceres::Covariance).  While enabled, every window
 * solve (a keyframe's refine_window) is followed by xrhip_ba_covariance (xrslam_hip.h) on the solved problem, for the newest keyframe
 * of the window; the answer stays, with its own timestamp, until the next window solve.  Off (the default) nothing is launched,
 * allocated or written that was not before.  The poses, landmarks and every other output are the same either way.
 *   state     15 x 15, error-state order dq dp dv dbg dba, in the body frame (the tangent space the solver works on)
 *   pose_ros  the pose part permuted for nav_msgs/Odometry: x y z, rotation about x y z, i.e. pose_ros[i][j] = state[p(i)][p(j)] with
 *             p = 3 4 5 0 1 2
 *   status    as xrhip_cov_request.status (0 ok, 1 not positive definite / rank deficient, 2 nothing free); -1 before the first window
 *             solve, and always with a library without xrhip_ba_covariance (XRSLAMAmdLastError says so)
 * XRSLAMAmdGetCovariance returns 1 when a covariance is available (status 0), else 0; `out` is filled either way.
 * XRSLAMAmdGetLandmarkVariances: the variance of the inverse depth of the landmarks that were free in that solve and are still valid
 * (the set XRSLAM_RESULT_LANDMARKS draws from), with their track ids; returns the count available and writes min(count, cap) entries
 * (either array may be NULL).  In pipelined mode both wait for the frame in flight, like XRSLAM_RESULT_LANDMARKS. */
typedef struct XRSLAMAmdCovariance {
    double timestamp;
    double state[15][15];
    double pose_ros[6][6];
    int status;
    double rcond_estimate;
} XRSLAMAmdCovariance;
void XRSLAMAmdSetCovariance(int enable);
int XRSLAMAmdGetCovariance(XRSLAMAmdCovariance *out);
int XRSLAMAmdGetLandmarkVariances(double *inv_depth_var, long long *track_ids, int cap);
/* What the initialiser (core/initializer.cpp) did so far: attempts that reached SfM, whether the last one
 * succeeded, which of the eight (R, T) hypotheses won its triangulation vote, and the IMU alignment it produced
 * (metric scale of the unit-baseline SfM map, gravity in the SfM frame, gyroscope bias). */
typedef struct XRSLAMAmdInitReport {
    long attempts, successes;
    int sfm_candidate, sfm_triangulated;
    double scale, gravity[3], bg[3];
} XRSLAMAmdInitReport;
void XRSLAMAmdGetInitReport(XRSLAMAmdInitReport *out);
/* last error raised inside the library ("" if none); the reference aborts/throws instead */
const char *XRSLAMAmdLastError(void);
/* Threading.  0 (default) = the reference's PC build: XRSLAMRunOneFrame / the IMU push that completes a frame run feature
 * tracker and sliding-window tracker inline, one after the other (utility/worker.h:37-45 without XRSLAM_ENABLE_THREADING).
 * 1 = its XRSLAM_ENABLE_THREADING build (utility/worker.h:16-60; feature tracker and frontend on threads of their own) with
 * deterministic hand-offs: the sliding-window tracker of frame t runs on a thread of the library beside the feature tracker of
 * frame t+1, which sees the state published for frame t-1 and propagates it by pre-integration exactly as
 * FeatureTracker::work does when the frontend lags (core/feature_tracker.cpp:44-66).  Same arithmetic, same kernels; poses
 * and landmark sets are those of a run whose backend is one frame late, reproducible bit for bit, and NOT those of mode 0.
 * With parsac.parsac_flag the frames stay inline (update_track_status reads the tracking map from inside the backend).
 * May be switched between frames.  XRSLAMAmdFlush waits for the frame in flight (also done by Destroy, by the LANDMARKS / BIAS
 * results and by the statistics getters). */
void XRSLAMAmdSetThreading(int mode);
void XRSLAMAmdFlush(void);
/* Masks: where in the frame the tracker must not look -- the vehicle's hood, a controller, a timestamp overlay, the black corners of
 * a rectified fisheye frame, what a segmentation network on the same GPU has just labelled (cv::goodFeaturesToTrack's mask, OpenVINS
 * use_mask, VINS fisheye_mask).  A mask is a W x H plane of bytes at the working resolution (cam0.resolution) and describes the
 * image the tracker works on, after format reduction, crop / scale and device undistortion: a byte != 0 may be used (1, 128 and 255
 * are the same), 0 is excluded.  Host memory or HBM (on_device), any base alignment, any stride >= W.
 *   XRSLAMAmdSetMask           the static mask: stays until cleared (mask == NULL)
 *   XRSLAMAmdSetNextFrameMask  the mask of the NEXT camera frame pushed through any of the push entry points; that frame consumes
 *                              it (a frame that is dropped, e.g. for a bad format, takes its mask with it); NULL withdraws it
 * The effective mask of a frame is static != 0 && per_frame != 0, a missing one counting as all ones; with neither, everything runs
 * exactly as it does without masks.  No new key point is detected on an excluded pixel -- and the corner threshold is taken over the
 * visible pixels only, so hiding the strongest corner lowers it -- and a tracked key point whose new position rounds to an excluded
 * pixel is dropped like one that failed the tracker's own gates (include/xrslam_hip.h, "Masks", has the rules).
 * A host mask is copied during the call.  A static HBM mask has been read on return; a per-frame HBM mask must stay valid until the
 * frame has been pushed.  Works in both threading modes: the mask is bound to the frame when it is pushed.
 * Returns 1 on success; 0 with the reason in XRSLAMAmdLastError for stride < W, no instance, or an instance that is a member of a
 * group -- the mask in force (or none) then stays as it was.  A masked instance cannot join a group (XRSLAMAmdInstanceJoinGroup fails).
 * Not here: masks at the source geometry of a scaled frame or in the distorted image, a configuration key, the CPU-reference pipeline. */
int XRSLAMAmdSetMask(const void *mask, int stride, int on_device);
int XRSLAMAmdSetNextFrameMask(const void *mask, int stride, int on_device);

/* ---- tracking view (additive) ----
 * XRSLAM_RESULT_FEATURES fills XRSLAMFeatures::pos with the pixel positions of the key points of the newest tracked frame that have a
 * track, in key-point order: the set the reference's feature_tracker_painter paints (core/feature_tracker.cpp:137-149).
 * XRSLAMAmdGetFeatures is its C-callable form with everything the tracker knows about the frame: ALL key points of the newest tracked
 * frame in key-point order (those just detected have track_id -1, age 0), `age` = the track's key-point count in the tracking map (what
 * Frame::track_keypoints sorts by), and -- with XRSLAMAmdSetFeatureHistory(frames), 0 (default) .. 8 = XRSLAM_AMD_VIEW_MAX_TRAIL -- `trail`:
 * the positions of the same track in the previous frames of the tracking map, newest first, up to the first frame without it.  Writes at
 * most `cap` entries (out may be NULL) and *timestamp (may be NULL); returns the count needed, 0 before the first tracked frame.  The
 * history setting takes effect with the next tracked frame. */
#define XRSLAM_AMD_VIEW_MAX_TRAIL 8
typedef struct XRSLAMAmdFeature {
    double x, y;
    long long track_id;
    int age;
    int n_trail;
    double trail[XRSLAM_AMD_VIEW_MAX_TRAIL][2];
} XRSLAMAmdFeature;
int XRSLAMAmdGetFeatures(XRSLAMAmdFeature *out, int cap, double *timestamp);
void XRSLAMAmdSetFeatureHistory(int frames);
/* The tracker's view of its newest frame, drawn on the GPU (xrslam_hip.h: xrhip_image_render_view) into interleaved 8-bit BGR
 * (channels 3) or BGRA (channels 4) rows of `stride` bytes: a host buffer, or one in HBM when on_device (complete after the next call that
 * waits for the instance, e.g. XRSLAMAmdGetKltStats; at once for a member of a group).
 *   opt NULL or all zero: the reference's view -- every key point with a track is a disc of r^2 = 10 in CV_RGB(255,255,0) = BGR (0,255,255),
 *     centred on its position truncated to int;
 *   color_mode 1: by age -- age < 4 BGR (0,0,255), 4 <= age < 10 (0,255,255), age >= 10 (0,255,0);
 *   draw_new: key points without a track as discs of r^2 = 2 in BGR (255,255,0), below the tracked ones;
 *   trail > 0: per tracked key point a polyline in BGR (255,160,0) from its position through its first min(trail, n_trail) trail positions
 *     (needs XRSLAMAmdSetFeatureHistory); all lines lie below all discs.
 * Deviation: the reference paints on the frame as pushed (in colour if it was); here the colour is gone after the upload and the canvas is
 * the gray plane the tracker works on (after colour reduction and device undistortion, before CLAHE), replicated to B = G = R.
 * Returns 1 on success; 0 with XRSLAMAmdLastError set when no frame has been tracked yet or the newest frame's plane is gone.  In
 * pipelined mode the call does not wait for the backend.  The frame's plane is valid until the next frame is tracked. */
typedef struct XRSLAMAmdViewOptions {
    int color_mode;
    int draw_new;
    int trail;
} XRSLAMAmdViewOptions;
int XRSLAMAmdRenderTrackingView(void *out, int stride, int channels, int on_device, const XRSLAMAmdViewOptions *opt);

/* ---- instance-scoped entry points (additive) ----
 * The six reference symbols above act on one process-global instance, like the reference's XRSLAMManager singleton
 * (xrslam-interface/src/XRSLAMManager.cpp:6-9).  The reference cannot do otherwise -- solver configuration, CLAHE /
 * GFTT objects, id counters and the RD-VIO bin confidences are function- or class-level statics there --
 * here all of that state lives in the instance, so one process can run several independent sequences on one GPU
 * (each instance owns its HIP streams; kernels of different instances overlap on the device).  Same semantics as the
 * global entry points, with the instance as first argument.  One thread at a time per instance; different instances
 * may be driven from different threads.  An instance belongs to the HIP device that was current when it was created. */
typedef struct XRSLAMAmdInstance XRSLAMAmdInstance;
int XRSLAMAmdInstanceCreate(const char *slam_config_path, const char *device_config_path, XRSLAMAmdInstance **out,
                            void **config);
void XRSLAMAmdInstanceDestroy(XRSLAMAmdInstance *inst);
void XRSLAMAmdInstancePushSensorData(XRSLAMAmdInstance *inst, XRSLAMSensorType sensor_type, void *sensor_data);
void XRSLAMAmdInstanceRunOneFrame(XRSLAMAmdInstance *inst);
void XRSLAMAmdInstanceGetResult(XRSLAMAmdInstance *inst, XRSLAMResultType result_type, void *result_data);
void XRSLAMAmdInstanceSetInitialState(XRSLAMAmdInstance *inst, double t, const double q[4], const double p[3],
                                      const double v[3], const double bg[3], const double ba[3]);
void XRSLAMAmdInstancePushImageDevice(XRSLAMAmdInstance *inst, const void *gray_dev, int stride, double timestamp);
void XRSLAMAmdInstancePushImageDeviceColor(XRSLAMAmdInstance *inst, const void *pixels_dev, int stride, int channels,
                                           double timestamp);
void XRSLAMAmdInstancePushImageFormat(XRSLAMAmdInstance *inst, const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt,
                                      int on_device, double timestamp);
void XRSLAMAmdInstancePushImageScaled(XRSLAMAmdInstance *inst, const void *pixels, int stride, const XRSLAMAmdFrameFormat *fmt,
                                      const XRSLAMAmdFrameGeometry *geo, int on_device, double timestamp);
int XRSLAMAmdInstanceSetFrameOrientation(XRSLAMAmdInstance *inst, int orientation);
int XRSLAMAmdInstanceGetFrameOrientation(XRSLAMAmdInstance *inst);
void XRSLAMAmdInstanceGetCameraConfig(XRSLAMAmdInstance *inst, XRSLAMAmdCameraConfig *out);
int XRSLAMAmdInstanceDescribeConfig(XRSLAMAmdInstance *inst, char *buf, int cap);
void XRSLAMAmdInstanceSetDeviceUndistort(XRSLAMAmdInstance *inst, const char *model);
void XRSLAMAmdInstanceGetTimes(XRSLAMAmdInstance *inst, XRSLAMAmdTimes *out);
void XRSLAMAmdInstanceSetProfiling(XRSLAMAmdInstance *inst, int enable);
void XRSLAMAmdInstanceGetBaStats(XRSLAMAmdInstance *inst, void *xrhip_ba_stats_out, int reset);
void XRSLAMAmdInstanceSetCovariance(XRSLAMAmdInstance *inst, int enable);
int XRSLAMAmdInstanceGetCovariance(XRSLAMAmdInstance *inst, XRSLAMAmdCovariance *out);
int XRSLAMAmdInstanceGetLandmarkVariances(XRSLAMAmdInstance *inst, double *inv_depth_var, long long *track_ids, int cap);
void XRSLAMAmdInstanceGetKltStats(XRSLAMAmdInstance *inst, void *xrhip_klt_stats_out, int reset);
int XRSLAMAmdInstanceGetTrackerParams(XRSLAMAmdInstance *inst, XRSLAMAmdTrackerParams *out);
void XRSLAMAmdInstanceGetInitReport(XRSLAMAmdInstance *inst, XRSLAMAmdInitReport *out);
const char *XRSLAMAmdInstanceLastError(XRSLAMAmdInstance *inst);
void XRSLAMAmdInstanceSetThreading(XRSLAMAmdInstance *inst, int mode);
int XRSLAMAmdInstanceSetMask(XRSLAMAmdInstance *inst, const void *mask, int stride, int on_device);
int XRSLAMAmdInstanceSetNextFrameMask(XRSLAMAmdInstance *inst, const void *mask, int stride, int on_device);
void XRSLAMAmdInstanceFlush(XRSLAMAmdInstance *inst);
int XRSLAMAmdInstanceGetFeatures(XRSLAMAmdInstance *inst, XRSLAMAmdFeature *out, int cap, double *timestamp);
void XRSLAMAmdInstanceSetFeatureHistory(XRSLAMAmdInstance *inst, int frames);
int XRSLAMAmdInstanceRenderTrackingView(XRSLAMAmdInstance *inst, void *out, int stride, int channels, int on_device,
                                        const XRSLAMAmdViewOptions *opt);
/* ---- instance groups (additive) ----
 * S independent sequences on one GPU leave it waiting on its own front end: every sequence issues ~26 small dependent launches per
 * frame.  Instances that have joined a group keep their state, ids and results to themselves but share launches: the library issues
 * ONE launch per kernel of the per-frame path (frame upload, CLAHE / pyramid, LK, Harris, pre-integration, the localisation and
 * sub-window solves) for all members that are waiting for it at that moment.  The trajectory of a member is the one it has alone,
 * bit for bit.  Usage: create the group on the device, create the instances, join each before its first frame, drive every instance
 * from a thread of its own (XRSLAMAmdInstanceReplay or the per-sample entry points); destroy the instances (or leave: group NULL)
 * before the group.  Returns 1 on success, 0 otherwise (XRSLAMAmdLastError / XRSLAMAmdInstanceLastError).
 * XRSLAMAmdGroupGetStats fills an xrhip_group_stats (xrslam_hip.h): batches and requests per kind -- requests / batches is the
 * number of sequences a launch served. */
typedef struct XRSLAMAmdGroup XRSLAMAmdGroup;
int XRSLAMAmdGroupCreate(XRSLAMAmdGroup **out);
int XRSLAMAmdGroupDestroy(XRSLAMAmdGroup *group);
int XRSLAMAmdInstanceJoinGroup(XRSLAMAmdInstance *inst, XRSLAMAmdGroup *group);
void XRSLAMAmdGroupSetProfiling(XRSLAMAmdGroup *group, int enable);
void XRSLAMAmdGroupGetStats(XRSLAMAmdGroup *group, void *xrhip_group_stats_out, int reset);
/* The player's loop (xrslam-pc/player/src/main.cpp:116-169) over a pre-staged sequence for the next `n_steps` camera frames:
 * IMU samples up to each frame's time (gyroscope before accelerometer, IO/async_dataset_reader.cpp:41-48), the frame,
 * XRSLAMRunOneFrame, state / body-pose query.  imu7: [n_imu][7] = t, gyroscope xyz, accelerometer xyz; cam_t: [n_frames];
 * frames: n_frames 8-bit images of frame_bytes each, host memory or (on_device != 0) HBM; the cursors are advanced.
 * poses_out8 (may be NULL): [n_steps][8] = t, translation xyz, quaternion xyzw of every frame answered in state
 * TRACKING_SUCCESS.  Returns the number of poses written, -1 on bad arguments.  Lets a harness drive several instances from
 * several threads without a host-language call per sensor sample. */
int XRSLAMAmdInstanceReplay(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                            const void *frames, size_t frame_bytes, int stride, int on_device, int *imu_cursor,
                            int *frame_cursor, int n_steps, double *poses_out8);
/* The same loop over colour frames: channels 1, 3 (BGR) or 4 (BGRA); frame_bytes and stride describe the colour frames. */
int XRSLAMAmdInstanceReplayColor(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                                 const void *frames, size_t frame_bytes, int stride, int channels, int on_device,
                                 int *imu_cursor, int *frame_cursor, int n_steps, double *poses_out8);
/* The same loop over frames of any XRSLAMAmdFrameFormat; frame_bytes and stride describe the frames as they lie in memory. */
int XRSLAMAmdInstanceReplayFormat(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                                  const void *frames, size_t frame_bytes, int stride, const XRSLAMAmdFrameFormat *fmt, int on_device,
                                  int *imu_cursor, int *frame_cursor, int n_steps, double *poses_out8);
/* The same loop over frames larger than cam0.resolution (XRSLAMAmdPushImageScaled): frame_bytes, stride and geo describe the
 * frames as they lie in memory; fmt NULL = GRAY8. */
int XRSLAMAmdInstanceReplayScaled(XRSLAMAmdInstance *inst, const double *imu7, int n_imu, const double *cam_t, int n_frames,
                                  const void *frames, size_t frame_bytes, int stride, const XRSLAMAmdFrameFormat *fmt,
                                  const XRSLAMAmdFrameGeometry *geo, int on_device, int *imu_cursor, int *frame_cursor, int n_steps,
                                  double *poses_out8);

#ifdef __cplusplus
}
#endif
#endif /* XRSLAM_AMD_XRSLAM_H */
