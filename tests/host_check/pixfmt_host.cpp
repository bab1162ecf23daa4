// Stand-alone check of the host side of the camera pixel formats (xrslam_amd/csrc/host/pixel_format.hpp): the reduction the CPU
// reference build applies in Pipeline::make_image and the row packing of the pinned upload slots, over odd widths, strides and
// base offsets.  Every source buffer is a heap block of exactly the bytes the contract names -- offset + stride * (height - 1) +
// width * bytes per pixel -- so that, built with -fsanitize=address,undefined (tests/test_pixfmt_host.py), a read of one byte more
// ends the program.  The expected values are restated here per format, not taken from the header.  No GPU code; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../xrslam_amd/csrc/host/pixel_format.hpp"

static uint32_t rng_state = 12345u;
static uint8_t next_byte() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

static int limited(int g) {
    if (g < 16) g = 16;
    int v = ((g - 16) * 255 + 109) / 219;
    return v > 255 ? 255 : v;
}

// the issue's table, one format at a time
static int expect(const uint8_t *p, int format, int bits, int lim) {
    int g = 0;
    switch (format) {
        case XRHIP_PIXFMT_GRAY8: case XRHIP_PIXFMT_NV12: case XRHIP_PIXFMT_I420: case XRHIP_PIXFMT_YUYV: g = p[0]; break;
        case XRHIP_PIXFMT_UYVY: case XRHIP_PIXFMT_P010: g = p[1]; break;
        case XRHIP_PIXFMT_BGR8: case XRHIP_PIXFMT_BGRA8: return (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14;
        case XRHIP_PIXFMT_RGB8: case XRHIP_PIXFMT_RGBA8: return (p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + 8192) >> 14;
        case XRHIP_PIXFMT_GRAY16: {
            const int v = p[0] | (p[1] << 8);
            g = v >> ((bits ? bits : 16) - 8);
            if (g > 255) g = 255;
            break;
        }
    }
    return lim ? limited(g) : g;
}

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static void check_frame(int format, int bits, int lim, int w, int h, int pad, int offset) {
    xrh::PixelFormat pf;
    CHECK(xrh::describe_pixel_format(format, bits, lim, pf) == nullptr);
    const int stride = w * pf.bpp + pad;
    const size_t need = (size_t)offset + (size_t)stride * (h - 1) + (size_t)w * pf.bpp;
    uint8_t *block = static_cast<uint8_t *>(std::malloc(need));   // exactly the frame: first byte to last byte
    for (size_t i = 0; i < need; ++i) block[i] = next_byte();
    const uint8_t *src = block + offset;
    std::vector<uint8_t> gray((size_t)w * h, 0x5a);
    xrh::reduce_frame(gray.data(), src, stride, w, h, pf);
    int bad = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            bad += gray[(size_t)y * w + x] != expect(src + (size_t)y * stride + (size_t)x * pf.bpp, format, bits, lim);
    CHECK(bad == 0);
    // the pinned slot's rows: w * bpp bytes each, back to back, in a block of exactly that size
    const size_t row = (size_t)w * pf.bpp;
    uint8_t *slot = static_cast<uint8_t *>(std::malloc(row * h));
    xrh::pack_rows(slot, src, stride, row, h);
    for (int y = 0; y < h; ++y) bad += std::memcmp(slot + (size_t)y * row, src + (size_t)y * stride, row) != 0;
    CHECK(bad == 0);
    // and the packed rows reduce to the same plane (what the device reads is the slot)
    std::vector<uint8_t> again((size_t)w * h);
    xrh::reduce_frame(again.data(), slot, (int)row, w, h, pf);
    CHECK(again == gray);
    std::free(slot);
    std::free(block);
}

int main() {
    xrh::PixelFormat pf;
    // arguments
    CHECK(xrh::describe_pixel_format(-1, 0, 0, pf) != nullptr);
    CHECK(xrh::describe_pixel_format(11, 0, 0, pf) != nullptr);
    CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY16, 7, 0, pf) != nullptr);
    CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY16, 17, 0, pf) != nullptr);
    for (int f : {XRHIP_PIXFMT_BGR8, XRHIP_PIXFMT_BGRA8, XRHIP_PIXFMT_RGB8, XRHIP_PIXFMT_RGBA8})
        CHECK(xrh::describe_pixel_format(f, 0, 1, pf) != nullptr);
    CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY16, 0, 0, pf) == nullptr && pf.bpp == 2 && pf.shift == 8);
    // the range expansion at its corners
    const int in[] = {0, 15, 16, 17, 126, 234, 235, 236, 255}, out[] = {0, 0, 0, 1, 128, 254, 255, 255, 255};
    for (int i = 0; i < 9; ++i) CHECK(xrh::expand_limited_range((uint32_t)in[i]) == out[i]);
    // GRAY16 saturates above its significant bits
    for (int bits : {8, 10, 12, 16}) {
        CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY16, bits, 0, pf) == nullptr);
        const int top = (1 << bits) - 1, over = bits == 16 ? 65535 : 1 << bits;
        const uint8_t s[4][2] = {{0, 0}, {(uint8_t)top, (uint8_t)(top >> 8)}, {(uint8_t)over, (uint8_t)(over >> 8)}, {255, 255}};
        CHECK(xrh::reduce_pixel(s[0], pf) == 0 && xrh::reduce_pixel(s[1], pf) == 255 && xrh::reduce_pixel(s[2], pf) == 255 &&
              xrh::reduce_pixel(s[3], pf) == 255);
    }
    // frames: every format, odd widths, padded rows, every base offset
    const int sizes[][2] = {{96, 7}, {97, 6}, {33, 5}, {1, 3}};
    for (int format = 0; format <= XRHIP_PIXFMT_P010; ++format)
        for (int lim = 0; lim < 2; ++lim) {
            if (lim && format >= XRHIP_PIXFMT_BGR8 && format <= XRHIP_PIXFMT_RGBA8) continue;
            for (int bits : {0, 8, 10, 12, 16}) {
                if (bits && format != XRHIP_PIXFMT_GRAY16) continue;
                for (const auto &sz : sizes)
                    for (int pad : {0, 1, 5, 64})
                        for (int offset = 0; offset < 4; ++offset) check_frame(format, bits, lim, sz[0], sz[1], pad, offset);
            }
        }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
