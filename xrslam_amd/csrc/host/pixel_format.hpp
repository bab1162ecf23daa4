// Camera pixel formats (include/xrslam_hip.h: XRHIP_PIXFMT_*): what a format means, in one place for the device upload's argument
// block (klt_api.hip), for the host reduction of a build without the device upload (Pipeline::make_image in the CPU reference build)
// and for the stand-alone host check (tests/host_check/pixfmt_host.cpp).  Plain C++, no device code, all integer:
//
//   1 byte  (GRAY8, NV12, I420: the luma plane)    gray = the byte
//   2 bytes (GRAY16, YUYV, UYVY, P010)             v = b0 | b1 << 8;  gray = min(255, (v & mask) >> shift)
//                                                  GRAY16: mask ffff, shift bits - 8;  P010, UYVY: ffff, 8;  YUYV: 00ff, 0
//   3 / 4   (BGR8, BGRA8, RGB8, RGBA8)             gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14, byte 3 ignored
//   limited range (not for the 3 / 4 byte formats) gray' = min(255, ((max(gray, 16) - 16) * 255 + 109) / 219)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../../include/xrslam_hip.h"

namespace xrh {

struct PixelFormat {
    int bpp = 1;              // bytes per pixel read
    uint32_t mask = 0xffffu;  // 2-byte formats
    uint32_t shift = 0;
    bool rgb = false;         // 3 / 4-byte formats: byte 0 is R
    bool limited = false;
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
        default: return "format is not one of XRHIP_PIXFMT_*";
    }
    if (limited_range && f.bpp >= 3) return "limited_range does not apply to the RGB / BGR formats";
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

// `rows` rows of `cols` pixels at `src` (rows `stride` bytes apart, any alignment) into the dense gray plane `dst`: reads
// cols * f.bpp bytes of each of the rows and nothing else
inline void reduce_frame(uint8_t *dst, const uint8_t *src, int stride, int cols, int rows, const PixelFormat &f) {
    for (int y = 0; y < rows; ++y) {
        const uint8_t *s = src + (size_t)y * stride;
        uint8_t *d = dst + (size_t)y * cols;
        for (int x = 0; x < cols; ++x) d[x] = reduce_pixel(s + (size_t)x * f.bpp, f);
    }
}

// `rows` rows of `row_bytes` bytes, `stride` apart, packed back to back into `dst` (a pinned upload slot): the padding is not read
inline void pack_rows(uint8_t *dst, const uint8_t *src, int stride, size_t row_bytes, int rows) {
    for (int y = 0; y < rows; ++y) std::memcpy(dst + (size_t)y * row_bytes, src + (size_t)y * stride, row_bytes);
}

}   // namespace xrh
