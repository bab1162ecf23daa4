// Stand-alone check of the host side of the frame scaling (xrslam_amd/csrc/host/pixel_format.hpp): scale_frame, the plain-C++ crop
// and area mean of the CPU reference build, and the staging of a cropped host frame into a pinned slot (crop_origin + pack_rows:
// rows of cw * bpp bytes).  Every source buffer is a heap block that starts at the frame's row 0 (plus a base offset) and ENDS with
// the crop's last needed byte -- stride * (crop_y + ch - 1) + (crop_x + cw) * bytes per pixel -- so that, built with
// -fsanitize=address,undefined (tests/test_scale_host.py), a read of one byte more ends the program.  The expected plane is
// restated here in 64-bit arithmetic from the definition (overlap weights per axis, rounded half up), not taken from the header.
// No GPU code; prints "ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../xrslam_amd/csrc/host/pixel_format.hpp"

static uint32_t rng_state = 2463534242u;
static uint8_t next_byte() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// overlap of output cell o = [o*n_in, (o+1)*n_in) with input cell i = [i*n_out, (i+1)*n_out)
static long long overlap(long long o, long long i, long long n_out, long long n_in) {
    return std::max(0ll, std::min((i + 1) * n_out, (o + 1) * n_in) - std::max(i * n_out, o * n_in));
}

static void expected_plane(std::vector<uint8_t> &out, int W, int H, const std::vector<uint8_t> &gray, int cw, int ch) {
    out.assign((size_t)W * H, 0);
    const long long area = (long long)cw * ch;
    // the non-zero weights of every output column / row (found by looking at every input cell)
    std::vector<std::vector<std::pair<int, long long>>> ax(W), by(H);
    for (int X = 0; X < W; ++X)
        for (int i = 0; i < cw; ++i)
            if (const long long a = overlap(X, i, W, cw)) ax[X].push_back({i, a});
    for (int Y = 0; Y < H; ++Y)
        for (int j = 0; j < ch; ++j)
            if (const long long b = overlap(Y, j, H, ch)) by[Y].push_back({j, b});
    for (int Y = 0; Y < H; ++Y)
        for (int X = 0; X < W; ++X) {
            long long acc = 0, sa = 0, sb = 0;
            for (const auto &jb : by[Y]) {
                sb += jb.second;
                for (const auto &ia : ax[X]) acc += jb.second * ia.second * gray[(size_t)jb.first * cw + ia.first];
            }
            for (const auto &ia : ax[X]) sa += ia.second;
            CHECK(sa == cw && sb == ch);
            out[(size_t)Y * W + X] = (uint8_t)((acc + area / 2) / area);
        }
}

static void check_geometry(int format, int bits, int lim, int W, int H, const xrhip_frame_geometry &g, int pad, int offset) {
    xrh::PixelFormat pf;
    CHECK(xrh::describe_pixel_format(format, bits, lim, pf) == nullptr);
    const int stride = g.src_width * pf.bpp + pad;
    CHECK(xrh::check_frame_geometry(&g, W, H, pf.bpp, stride) == nullptr);
    const int cw = g.crop_width, ch = g.crop_height;
    const size_t need = (size_t)offset + (size_t)stride * (g.crop_y + ch - 1) + (size_t)(g.crop_x + cw) * pf.bpp;
    uint8_t *block = static_cast<uint8_t *>(std::malloc(need));   // the frame from row 0 to the crop's last byte
    for (size_t i = 0; i < need; ++i) block[i] = next_byte();
    const uint8_t *src = block + offset;
    const uint8_t *origin = xrh::crop_origin(src, stride, g, pf.bpp);
    CHECK(origin == src + (size_t)g.crop_y * stride + (size_t)g.crop_x * pf.bpp);
    // per-pixel gray of the crop, then the definition
    std::vector<uint8_t> gray((size_t)cw * ch), want, got((size_t)W * H, 0x5a);
    for (int j = 0; j < ch; ++j)
        for (int i = 0; i < cw; ++i) gray[(size_t)j * cw + i] = xrh::reduce_pixel(origin + (size_t)j * stride + (size_t)i * pf.bpp, pf);
    expected_plane(want, W, H, gray, cw, ch);
    xrh::scale_frame(got.data(), W, H, origin, stride, cw, ch, pf);
    CHECK(got == want);
    // the pinned slot of a cropped host frame: ch rows of cw * bpp bytes, in a block of exactly that size
    const size_t row = (size_t)cw * pf.bpp;
    uint8_t *slot = static_cast<uint8_t *>(std::malloc(row * ch));
    xrh::pack_rows(slot, origin, stride, row, ch);
    int bad = 0;
    for (int j = 0; j < ch; ++j) bad += std::memcmp(slot + (size_t)j * row, origin + (size_t)j * stride, row) != 0;
    CHECK(bad == 0);
    // ... and what the device computes from the slot (a cw x ch frame, rows back to back) is the same plane
    std::vector<uint8_t> again((size_t)W * H, 0xa5);
    xrh::scale_frame(again.data(), W, H, slot, (long long)row, cw, ch, pf);
    CHECK(again == want);
    std::free(slot);
    std::free(block);
}

int main() {
    // arguments
    {
        const int W = 98, H = 65, sw = 203, sh = 135;
        const xrhip_frame_geometry good = {sw, sh, 3, 1, 196, 130};
        CHECK(xrh::check_frame_geometry(&good, W, H, 4, sw * 4) == nullptr);
        CHECK(xrh::check_frame_geometry(nullptr, W, H, 4, sw * 4) != nullptr);
        CHECK(xrh::check_frame_geometry(&good, W, H, 4, sw * 4 - 1) != nullptr);
        const xrhip_frame_geometry bad[] = {{sw, sh, 8, 1, 196, 130}, {sw, sh, 3, 6, 196, 130}, {sw, sh, -1, 1, 196, 130}, {sw, sh, 3, -1, 196, 130},
                                            {sw, sh, 0, 0, W - 1, 130}, {sw, sh, 0, 0, 196, H - 1}, {0, 0, 0, 0, 0, 0},
                                            {4097, 4096, 0, 0, 4097, 4096}, {0x7fffffff, 2, 0x7ffffff0, 0, 0x7fffffff, 2}};
        for (const auto &g : bad) CHECK(xrh::check_frame_geometry(&g, W, H, 1, 0x7fffffffll * 4) != nullptr);
        const xrhip_frame_geometry edge = {4096, 4096, 0, 0, 4096, 4096};
        CHECK(xrh::check_frame_geometry(&edge, 64, 64, 1, 4096) == nullptr);
    }
    // rounding half up at an exact tie; the largest sum
    {
        xrh::PixelFormat pf;
        const uint8_t t1[4] = {0, 0, 0, 2}, t2[4] = {0, 0, 1, 1}, t3[4] = {0, 0, 0, 1};
        uint8_t o = 9;
        xrh::scale_frame(&o, 1, 1, t1, 2, 2, 2, pf);
        CHECK(o == 1);
        xrh::scale_frame(&o, 1, 1, t2, 2, 2, 2, pf);
        CHECK(o == 1);
        xrh::scale_frame(&o, 1, 1, t3, 2, 2, 2, pf);
        CHECK(o == 0);
        std::vector<uint8_t> all((size_t)4096 * 4096, 255), out(4, 0);
        xrh::scale_frame(out.data(), 1, 1, all.data(), 4096, 4096, 4096, pf);   // cw * ch = 2^24: 255 * 2^24 + 2^23 < 2^32
        CHECK(out[0] == 255);
    }
    // intrinsics
    {
        const xrhip_frame_geometry g = {1920, 1080, 114, 0, 1692, 1080};
        const double K[4] = {1400.5, 1399.25, 961.75, 538.5};
        double o[4];
        xrh::scale_intrinsics(K, g, 752, 480, o);
        const double want[4] = {K[0] * 752.0 / 1692.0, K[1] * 480.0 / 1080.0, (K[2] + 0.5 - 114) * 752.0 / 1692.0 - 0.5,
                                (K[3] + 0.5) * 480.0 / 1080.0 - 0.5};
        for (int k = 0; k < 4; ++k) CHECK(std::fabs(o[k] - want[k]) < 1e-9);
    }
    // the geometry list of tests/test_scale_gpu.py per working plane, one format per byte class and flag route
    const int planes[][2] = {{96, 67}, {97, 66}, {98, 65}, {99, 64}};
    const int variants[][3] = {{XRHIP_PIXFMT_GRAY8, 0, 0}, {XRHIP_PIXFMT_GRAY8, 0, 1}, {XRHIP_PIXFMT_GRAY16, 10, 0}, {XRHIP_PIXFMT_YUYV, 0, 0},
                               {XRHIP_PIXFMT_UYVY, 0, 0}, {XRHIP_PIXFMT_P010, 0, 1}, {XRHIP_PIXFMT_RGB8, 0, 0}, {XRHIP_PIXFMT_BGRA8, 0, 0}};
    int n = 0;
    for (const auto &pl : planes) {
        const int W = pl[0], H = pl[1];
        const xrhip_frame_geometry geos[] = {{W + 9, H + 6, 5, 3, W, H},
                                             {2 * W, 2 * H, 0, 0, 2 * W, 2 * H},
                                             {(3 * W + 1) / 2 + 2, (3 * H + 1) / 2, 2, 0, (3 * W + 1) / 2, (3 * H + 1) / 2},
                                             {W + 40, H + 36, 6, 1, W + 34, H + 35},
                                             {8 * W + 4, 8 * H + 1, 1, 0, 8 * W + 3, 8 * H + 1},
                                             {2 * W + 1, H + 1, 0, 1, 2 * W, H},
                                             {W + W / 3 + 8, H + H / 5 + 8, 3, 5, W + W / 3, H + H / 5}};
        for (const auto &g : geos)
            for (const auto &v : variants) {
                const int pads[] = {0, 5, 64};
                check_geometry(v[0], v[1], v[2], W, H, g, pads[n % 3], n % 4);
                ++n;
            }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
