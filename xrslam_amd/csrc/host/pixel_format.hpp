// Camera pixel formats (include/xrslam_hip.h: XRHIP_PIXFMT_*): what a format means, in one place for the device upload's argument
// block (klt_api.hip), for the host reduction of a build without the device upload (Pipeline::make_image in the CPU reference build)
// and for the stand-alone host check (tests/host_check/pixfmt_host.cpp).  Plain C++, no device code, all integer:
//
//   1 byte  (GRAY8, NV12, I420: the luma plane)    gray = the byte
//   2 bytes (GRAY16, YUYV, UYVY, P010)             v = b0 | b1 << 8;  gray = min(255, (v & mask) >> shift)
//                                                  GRAY16: mask ffff, shift bits - 8;  P010, UYVY: ffff, 8;  YUYV: 00ff, 0
//   3 / 4   (BGR8, BGRA8, RGB8, RGBA8)             gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14, byte 3 ignored
//   limited range (not for the 3 / 4 byte formats) gray' = min(255, ((max(gray, 16) - 16) * 255 + 109) / 219)
//   Bayer mosaics (BAYER_*8 / *16: 1 / 2 bytes)    the sample s is the 1 / 2-byte value above (GRAY16's rule for *16); the gray value
//                                                  needs the pixel's neighbours: bayer_gray below, a whole frame at a time
//   packed 10 / 12 bits (GRAY*_MIPI, GRAY*P and     a row is bit-packed samples (packed_sample below: CSI-2 RAW10 / RAW12, PFNC lsb-packed); the
//   their BAYER_* forms)                            sample then counts as GRAY16's / BAYER_*16's with bits = 10 / 12.  No byte address for a pixel:
//                                                  samples are addressed by (row, x)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/xrslam_hip.h"

namespace xrh {

struct PixelFormat {
    int bpp = 1;              // bytes per pixel read
    uint32_t mask = 0xffffu;  // 2-byte formats
    uint32_t shift = 0;
    bool rgb = false;         // 3 / 4-byte formats: byte 0 is R
    bool limited = false;
    bool bayer = false;       // a colour-filter mosaic of 1 / 2-byte samples: the gray value is bayer_gray's, not reduce_pixel's
    int px = 0, py = 0;       // its pattern as a phase of RGGB: the colour site of (x, y) is RGGB's at ((x + px) & 1, (y + py) & 1)
    // bit-packed samples (bpp is 0 then): PACK_MIPI: groups of whole pixels with their low bits in the group's last byte (10 bits: 4 px
    // in 5 bytes; 12 bits: 2 px in 3); PACK_LSB: the row is one little-endian bit stream of `bits`-bit samples
    enum Packing { PACK_NONE = 0, PACK_MIPI, PACK_LSB };
    Packing packing = PACK_NONE;
    int bits = 0;             // of a packed sample: 10 or 12
    int group_px() const { return bits == 10 ? 4 : 2; }      // both packings start a byte every group_px pixels, group_bytes on
    int group_bytes() const { return bits == 10 ? 5 : 3; }
    // bytes that hold the first n pixels of a row
    long long row_bytes(long long n) const {
        if (packing == PACK_NONE) return n * bpp;
        if (packing == PACK_MIPI) return (n + group_px() - 1) / group_px() * group_bytes();
        return (n * bits + 7) / 8;
    }
};

// nullptr, or which argument is wrong and why (the callers put their own name in front)
inline const char *describe_pixel_format(int format, int bits, int limited_range, PixelFormat &out) {
    PixelFormat f;
    switch (format) {
        case XRHIP_PIXFMT_GRAY8: case XRHIP_PIXFMT_NV12: case XRHIP_PIXFMT_I420: f.bpp = 1; break;
        case XRHIP_PIXFMT_BGR8: f.bpp = 3; break;
        case XRHIP_PIXFMT_BGRA8: f.bpp = 4; break;
        case XRHIP_PIXFMT_RGB8: f.bpp = 3; f.rgb = true; break;
        case XRHIP_PIXFMT_RGBA8: f.bpp = 4; f.rgb = true; break;
        case XRHIP_PIXFMT_GRAY16:
            if (bits != 0 && (bits < 8 || bits > 16)) return "bits must be 0 (= 16) or 8..16";
            f.bpp = 2;
            f.shift = (uint32_t)((bits ? bits : 16) - 8);
            break;
        case XRHIP_PIXFMT_YUYV: f.bpp = 2; f.mask = 0xffu; break;
        case XRHIP_PIXFMT_UYVY: case XRHIP_PIXFMT_P010: f.bpp = 2; f.shift = 8; break;
        case XRHIP_PIXFMT_BAYER_RGGB8: case XRHIP_PIXFMT_BAYER_GRBG8: case XRHIP_PIXFMT_BAYER_GBRG8: case XRHIP_PIXFMT_BAYER_BGGR8:
        case XRHIP_PIXFMT_BAYER_RGGB16: case XRHIP_PIXFMT_BAYER_GRBG16: case XRHIP_PIXFMT_BAYER_GBRG16: case XRHIP_PIXFMT_BAYER_BGGR16: {
            const int pattern = (format - XRHIP_PIXFMT_BAYER_RGGB8) & 3;   // RGGB, GRBG, GBRG, BGGR = phase (0,0), (1,0), (0,1), (1,1)
            f.bayer = true;
            f.px = pattern & 1;
            f.py = pattern >> 1;
            if (format >= XRHIP_PIXFMT_BAYER_RGGB16) {   // the sample is reduced like GRAY16
                if (bits != 0 && (bits < 8 || bits > 16)) return "bits must be 0 (= 16) or 8..16";
                f.bpp = 2;
                f.shift = (uint32_t)((bits ? bits : 16) - 8);
            }
            break;
        }
        default: {
            const bool mono = format >= XRHIP_PIXFMT_GRAY10_MIPI && format <= XRHIP_PIXFMT_GRAY12P;
            if (!mono && !(format >= XRHIP_PIXFMT_BAYER_RGGB10_MIPI && format <= XRHIP_PIXFMT_BAYER_BGGR12P)) return "format is not one of XRHIP_PIXFMT_*";
            // GRAY: 32 + packing; BAYER: 40 + 4 * packing + pattern; packing: 10_MIPI, 12_MIPI, 10P, 12P.  `bits` is not read.
            const int packing = mono ? format - XRHIP_PIXFMT_GRAY10_MIPI : (format - XRHIP_PIXFMT_BAYER_RGGB10_MIPI) >> 2;
            f.bpp = 0;
            f.packing = packing < 2 ? PixelFormat::PACK_MIPI : PixelFormat::PACK_LSB;
            f.bits = (packing & 1) ? 12 : 10;
            f.shift = (uint32_t)(f.bits - 8);   // the sample is reduced like GRAY16 with bits = 10 / 12
            if (!mono) {
                const int pattern = (format - XRHIP_PIXFMT_BAYER_RGGB10_MIPI) & 3;
                f.bayer = true;
                f.px = pattern & 1;
                f.py = pattern >> 1;
            }
        }
    }
    if (limited_range && f.bpp >= 3) return "limited_range does not apply to the RGB / BGR formats";
    if (limited_range && f.bayer) return "limited_range does not apply to the Bayer formats";
    f.limited = limited_range != 0;
    out = f;
    return nullptr;
}

inline uint8_t expand_limited_range(uint32_t g) {
    return (uint8_t)std::min<uint32_t>(255u, ((std::max<uint32_t>(g, 16u) - 16u) * 255u + 109u) / 219u);
}

// One pixel at `p` (f.bpp bytes)
inline uint8_t reduce_pixel(const uint8_t *p, const PixelFormat &f) {
    uint32_t g;
    if (f.bpp == 1) g = p[0];
    else if (f.bpp == 2) g = std::min<uint32_t>(255u, ((((uint32_t)p[0] | ((uint32_t)p[1] << 8)) & f.mask) >> f.shift));
    else return (uint8_t)(((f.rgb ? p[2] : p[0]) * 1868 + p[1] * 9617 + (f.rgb ? p[0] : p[2]) * 4899 + 8192) >> 14);
    return f.limited ? expand_limited_range(g) : (uint8_t)g;
}

// Sample x of the packed row at `row` (xrslam_hip.h has the table): reads the bytes that hold its bits and nothing else
inline uint32_t packed_sample(const uint8_t *row, size_t x, const PixelFormat &f) {
    if (f.packing == PixelFormat::PACK_MIPI) {
        if (f.bits == 10) return (uint32_t)row[5 * (x >> 2) + (x & 3)] << 2 | ((uint32_t)row[5 * (x >> 2) + 4] >> (2 * (x & 3)) & 3u);
        return (uint32_t)row[3 * (x >> 1) + (x & 1)] << 4 | ((uint32_t)row[3 * (x >> 1) + 2] >> (4 * (x & 1)) & 15u);
    }
    const size_t bit = x * (size_t)f.bits, b = bit >> 3;   // (bit & 7) + bits <= 16: two bytes
    return (((uint32_t)row[b] | (uint32_t)row[b + 1] << 8) >> (bit & 7)) & ((1u << f.bits) - 1u);
}
// Pixel x of the row at `row`, of any format: reduce_pixel, or the packed sample reduced like GRAY16's
inline uint8_t row_pixel(const uint8_t *row, size_t x, const PixelFormat &f) {
    if (f.packing == PixelFormat::PACK_NONE) return reduce_pixel(row + x * (size_t)f.bpp, f);
    const uint32_t g = std::min<uint32_t>(255u, packed_sample(row, x, f) >> f.shift);
    return f.limited ? expand_limited_range(g) : (uint8_t)g;
}

// ------------------------------------------------------------------------------------------------ Bayer mosaics
// Bilinear demosaicing followed by the BGR weights, in exact integer arithmetic with one rounding (xrslam_hip.h has the definition;
// the device kernel k_upload_bayer and the numpy model tests/bayer_model.py give the same bits).  The frame is n_x x n_y samples;
// neighbours outside it mirror without repeating the edge (-1 -> 1, n -> n - 2), which keeps every neighbour on a site of the colour
// it stands for; n_x, n_y >= 2.  Every sum is four times the bilinear estimate; the weights sum to 16384.
inline int bayer_mirror(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }
// (x0: the frame's first column in the rows at `src`, for a crop of a packed frame)
inline uint8_t bayer_gray(const uint8_t *src, long long stride, int n_x, int n_y, int x, int y, const PixelFormat &f, int x0 = 0) {
    const int xl = bayer_mirror(x - 1, n_x), xr = bayer_mirror(x + 1, n_x), yu = bayer_mirror(y - 1, n_y), yd = bayer_mirror(y + 1, n_y);
    const auto s = [&](int xx, int yy) -> uint32_t { return row_pixel(src + (size_t)yy * (size_t)stride, (size_t)x0 + (size_t)xx, f); };
    const uint32_t C = 4 * s(x, y), Hh = 2 * (s(xl, y) + s(xr, y)), Vv = 2 * (s(x, yu) + s(x, yd)), P = (Hh + Vv) / 2;
    const uint32_t X = s(xl, yu) + s(xr, yu) + s(xl, yd) + s(xr, yd);
    const int cx = (x + f.px) & 1, cy = (y + f.py) & 1;   // RGGB's site: (0,0) red, (1,1) blue, (1,0) green between reds, (0,1) between blues
    uint32_t R4, G4, B4;
    if (cx == cy) {
        G4 = P;
        R4 = cx ? X : C;
        B4 = cx ? C : X;
    } else {
        G4 = C;
        R4 = cy ? Vv : Hh;
        B4 = cy ? Hh : Vv;
    }
    return (uint8_t)((4899u * R4 + 9617u * G4 + 1868u * B4 + 32768u) >> 16);
}
// The format of the crop of `g` taken as a Bayer frame of its own: the pattern phase shifts with the crop's origin
inline PixelFormat crop_pixel_format(PixelFormat f, const xrhip_frame_geometry &g) {
    if (f.bayer) {
        f.px ^= g.crop_x & 1;
        f.py ^= g.crop_y & 1;
    }
    return f;
}

// `rows` rows of `cols` pixels at `src` (rows `stride` bytes apart, any alignment) into the dense gray plane `dst`: reads
// cols * f.bpp bytes of each of the rows and nothing else.  A packed format: the pixels are columns x0 .. x0 + cols - 1 of the rows
// that start at `src`, and the bytes that hold their samples are read.
inline void reduce_frame(uint8_t *dst, const uint8_t *src, int stride, int cols, int rows, const PixelFormat &f, int x0 = 0) {
    if (f.bayer) {
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) dst[(size_t)y * cols + x] = bayer_gray(src, stride, cols, rows, x, y, f, x0);
        return;
    }
    for (int y = 0; y < rows; ++y) {
        const uint8_t *s = src + (size_t)y * stride;
        uint8_t *d = dst + (size_t)y * cols;
        for (int x = 0; x < cols; ++x) d[x] = row_pixel(s, (size_t)x0 + (size_t)x, f);
    }
}

// `rows` rows of `row_bytes` bytes, `stride` apart, packed back to back into `dst` (a pinned upload slot): the padding is not read
inline void pack_rows(uint8_t *dst, const uint8_t *src, int stride, size_t row_bytes, int rows) {
    for (int y = 0; y < rows; ++y) std::memcpy(dst + (size_t)y * row_bytes, src + (size_t)y * stride, row_bytes);
}

// ------------------------------------------------------------------------------------------------ frames larger than the working plane
// A frame geometry (xrslam_hip.h: xrhip_frame_geometry): the crop {crop_x, crop_y, cw, ch} of a src_width x src_height frame is
// area-averaged down to the W x H working plane.  Destination pixel (X, Y) is the exact mean of the per-pixel gray values over its
// footprint, rounded half up: in units where a source pixel is W wide the destination pixel spans [X*cw, (X+1)*cw), source column i
// covers [i*W, (i+1)*W), a_i is their overlap (the a_i sum to cw); b_j likewise with ch and H;
//   out = (sum_j b_j sum_i a_i g(i, j) + cw*ch / 2) / (cw*ch)
// cw*ch <= 2^24 keeps 255*cw*ch + cw*ch/2 inside 32 bits.  Plain C++, all integer: the device kernel (k_upload_scaled) and the numpy
// model (tests/scale_model.py) give the same bits.
constexpr long long SCALE_MAX_CROP_AREA = 1ll << 24;

// nullptr, or which argument is wrong and why
inline const char *check_frame_geometry(const xrhip_frame_geometry *g, int W, int H, int bpp, long long stride) {
    if (!g) return "geo is null";
    if (g->src_width < 1 || g->src_height < 1) return "geo: src_width and src_height must be positive";
    if (g->crop_width < 1 || g->crop_height < 1 || g->crop_x < 0 || g->crop_y < 0 ||
        (long long)g->crop_x + g->crop_width > g->src_width || (long long)g->crop_y + g->crop_height > g->src_height)
        return "geo: the crop rectangle lies outside the source frame";
    if (g->crop_width < W) return "geo: crop_width is smaller than the working width (no upscaling)";
    if (g->crop_height < H) return "geo: crop_height is smaller than the working height (no upscaling)";
    if ((long long)g->crop_width * g->crop_height > SCALE_MAX_CROP_AREA) return "geo: crop_width * crop_height exceeds 2^24";
    if (stride < (long long)g->src_width * bpp) return "stride_bytes < src_width * bytes per pixel";
    return nullptr;
}
// the same for any format: the stride holds the (packed) bytes of a source row
inline const char *check_frame_geometry(const xrhip_frame_geometry *g, int W, int H, const PixelFormat &f, long long stride) {
    if (f.packing == PixelFormat::PACK_NONE) return check_frame_geometry(g, W, H, f.bpp, stride);
    const char *why = check_frame_geometry(g, W, H, 0, stride);
    if (!why && stride < f.row_bytes(g->src_width)) why = "stride_bytes < the packed bytes of a row of src_width pixels";
    return why;
}

// The crop's first byte in a frame whose row 0 starts at `pixels`
inline const uint8_t *crop_origin(const uint8_t *pixels, long long stride, const xrhip_frame_geometry &g, int bpp) {
    return pixels + (size_t)g.crop_y * (size_t)stride + (size_t)g.crop_x * bpp;
}
// The same for any format, as (rows, x0): a packed pixel has no byte address, so the crop is columns x0 .. of the rows that start at
// the returned byte -- the byte at which the group of crop_x starts (both packings start a byte every group_px pixels), x0 the
// crop's first column counted from there.  Other formats: crop_origin and x0 = 0.
inline const uint8_t *crop_rows(const uint8_t *pixels, long long stride, const xrhip_frame_geometry &g, const PixelFormat &f, int &x0) {
    if (f.packing == PixelFormat::PACK_NONE) {
        x0 = 0;
        return crop_origin(pixels, stride, g, f.bpp);
    }
    x0 = g.crop_x % f.group_px();
    return pixels + (size_t)g.crop_y * (size_t)stride + (size_t)(g.crop_x / f.group_px()) * (size_t)f.group_bytes();
}

// `src`: the crop's first byte (rows `stride` bytes apart, cw x ch pixels of f.bpp bytes) -> the dense W x H plane `dst`.  Reads the
// cw * f.bpp bytes of each of the ch rows and nothing else.  A Bayer crop (f: crop_pixel_format) is a Bayer frame of its own: it is
// demosaiced whole, its neighbours mirrored at the crop's edges, and the gray crop is scaled.  A packed format: (src, col0) are
// crop_rows', and the bytes that hold the crop's samples are read.
inline void scale_frame(uint8_t *dst, int W, int H, const uint8_t *src, long long stride, int cw, int ch, const PixelFormat &f, int col0 = 0) {
    if (f.bayer) {
        std::vector<uint8_t> gray((size_t)cw * ch);
        reduce_frame(gray.data(), src, (int)stride, cw, ch, f, col0);
        return scale_frame(dst, W, H, gray.data(), cw, cw, ch, PixelFormat());
    }
    const uint32_t area = (uint32_t)cw * (uint32_t)ch, half = area / 2;
    for (int Y = 0; Y < H; ++Y) {
        const long long y0 = (long long)Y * ch, y1 = y0 + ch;
        const int j0 = (int)(y0 / H), j1 = (int)((y1 + H - 1) / H);
        for (int X = 0; X < W; ++X) {
            const long long x0 = (long long)X * cw, x1 = x0 + cw;
            const int i0 = (int)(x0 / W), i1 = (int)((x1 + W - 1) / W);
            uint32_t acc = 0;
            for (int j = j0; j < j1; ++j) {
                const uint32_t b = (uint32_t)(std::min<long long>((long long)(j + 1) * H, y1) - std::max<long long>((long long)j * H, y0));
                const uint8_t *row = src + (size_t)j * (size_t)stride;
                uint32_t r = 0;
                for (int i = i0; i < i1; ++i) {
                    const uint32_t a = (uint32_t)(std::min<long long>((long long)(i + 1) * W, x1) - std::max<long long>((long long)i * W, x0));
                    r += a * row_pixel(row, (size_t)col0 + (size_t)i, f);
                }
                acc += b * r;
            }
            dst[(size_t)Y * W + X] = (uint8_t)((acc + half) / area);
        }
    }
}

// Intrinsics {fx, fy, cx, cy} of the source frame -> those of the W x H working plane, pixel centres at integer coordinates:
// a source coordinate u maps to (u + 0.5 - crop_x) * W / cw - 0.5.  Distortion coefficients act on normalised coordinates: unchanged.
inline void scale_intrinsics(const double src[4], const xrhip_frame_geometry &g, int W, int H, double out[4]) {
    const double sx = (double)W / g.crop_width, sy = (double)H / g.crop_height;
    const double fx = src[0] * sx, fy = src[1] * sy;
    const double cx = (src[2] + 0.5 - g.crop_x) * sx - 0.5, cy = (src[3] + 0.5 - g.crop_y) * sy - 0.5;
    out[0] = fx; out[1] = fy; out[2] = cx; out[3] = cy;
}

// ------------------------------------------------------------------------------------------------ turned and mirrored frames
// An orientation (xrslam_hip.h: xrhip_klt_set_orientation) is o = r + 4 f, 0..7: the cw x ch gray crop is mirrored left to right if f,
// then turned r quarter turns clockwise; the turned crop (ch x cw for odd r) is what is scaled to the plane.
inline bool orientation_valid(int o) { return o >= 0 && o <= 7; }
inline int orientation_from_exif(int exif) {   // EXIF tag 274
    static const int table[9] = {-1, 0, 4, 2, 6, 7, 1, 5, 3};
    return exif >= 1 && exif <= 8 ? table[exif] : -1;
}
// Where pixel (i, j) of the cw x ch crop lies in the turned crop
inline void orient_point(int o, int cw, int ch, long long i, long long j, long long &X, long long &Y) {
    if (o & 4) i = cw - 1 - i;
    switch (o & 3) {
        case 0: X = i; Y = j; break;
        case 1: X = ch - 1 - j; Y = i; break;
        case 2: X = cw - 1 - i; Y = ch - 1 - j; break;
        default: X = j; Y = cw - 1 - i; break;
    }
}
// The dense gray plane `src` (sw x sh, the source's orientation) turned into the dense plane `dst` (sh x sw for odd r): what the
// device's k_orient computes, for a build without it
inline void orient_plane(uint8_t *dst, const uint8_t *src, int sw, int sh, int o) {
    const int W = (o & 1) ? sh : sw;
    for (int j = 0; j < sh; ++j)
        for (int i = 0; i < sw; ++i) {
            long long X, Y;
            orient_point(o, sw, sh, i, j, X, Y);
            dst[(size_t)Y * W + (size_t)X] = src[(size_t)j * sw + i];
        }
}
// Intrinsics {fx, fy, cx, cy} of the source frame -> those of the W x H working plane through crop (g; nullptr: the whole frame, which
// is H x W for odd r), orientation and scale, pixel centres at integer coordinates (XRSLAM.h: XRSLAMAmdOrientIntrinsics has the
// formulas).  R, row-major 3 x 3: a ray of the source camera -> the working camera's.
inline void orient_intrinsics(const double src[4], const xrhip_frame_geometry *g, int o, int W, int H, double out[4], double R[9]) {
    const int cw = g ? g->crop_width : (o & 1) ? H : W, ch = g ? g->crop_height : (o & 1) ? W : H;
    const double x0 = g ? g->crop_x : 0, y0 = g ? g->crop_y : 0;
    // (X, Y) = P (i, j) + t, from the images of (0, 0), (1, 0) and (0, 1)
    long long tx, ty, ax, ay, bx, by;
    orient_point(o, cw, ch, 0, 0, tx, ty);
    orient_point(o, cw, ch, 1, 0, ax, ay);
    orient_point(o, cw, ch, 0, 1, bx, by);
    const double P[2][2] = {{(double)(ax - tx), (double)(bx - tx)}, {(double)(ay - ty), (double)(by - ty)}};
    const double sx = (double)W / ((o & 1) ? ch : cw), sy = (double)H / ((o & 1) ? cw : ch);
    const double ci = src[2] - x0, cj = src[3] - y0;
    out[0] = sx * (std::abs(P[0][0]) * src[0] + std::abs(P[0][1]) * src[1]);
    out[1] = sy * (std::abs(P[1][0]) * src[0] + std::abs(P[1][1]) * src[1]);
    out[2] = sx * (P[0][0] * ci + P[0][1] * cj + (double)tx + 0.5) - 0.5;
    out[3] = sy * (P[1][0] * ci + P[1][1] * cj + (double)ty + 0.5) - 0.5;
    const double r[9] = {P[0][0], P[0][1], 0, P[1][0], P[1][1], 0, 0, 0, 1};
    std::memcpy(R, r, sizeof(r));
}

}   // namespace xrh
