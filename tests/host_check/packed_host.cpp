// Stand-alone check of the host side of the packed 10 / 12-bit formats (xrslam_amd/csrc/host/pixel_format.hpp): the unpacking the
// CPU reference build applies in Pipeline::make_image (reduce_frame, scale_frame through crop_rows) over frames that
// tests/test_packed_cpu.py writes to a file, and the argument rules of describe_pixel_format and check_frame_geometry.  Every source
// buffer is a heap block of exactly the bytes the contract names -- base offset + stride * (last needed row) + the packed bytes that
// hold that row's last needed pixel -- so that, built with -fsanitize=address,undefined, a read of one byte more ends the program.
// No GPU code.  Prints one "case <k> <fnv1a-64 of the plane, hex>" line per case and "ok".
//
// The case file: int32 little-endian words {format, limited_range, stride, offset, scaled, W, H, src_width, src_height, crop_x, crop_y,
// cw, ch, nbytes} followed by nbytes bytes (the block, base offset included), repeated.  Not scaled: the frame is W x H.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../xrslam_amd/csrc/host/pixel_format.hpp"

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static unsigned long long fnv1a(const std::vector<uint8_t> &v) {
    unsigned long long h = 1469598103934665603ull;
    for (uint8_t b : v) h = (h ^ b) * 1099511628211ull;
    return h;
}

int main(int argc, char **argv) {
    xrh::PixelFormat pf;
    // the numbers between the formats, and behind them, are not formats
    for (int f : {-1, 11, 12, 13, 14, 15, 24, 25, 26, 27, 28, 29, 30, 31, 36, 37, 38, 39, 56, 57, 64}) {
        const char *why = xrh::describe_pixel_format(f, 0, 0, pf);
        CHECK(why != nullptr && std::strstr(why, "format") != nullptr);
    }
    for (int f = XRHIP_PIXFMT_GRAY10_MIPI; f <= XRHIP_PIXFMT_GRAY12P; ++f) {
        const int p = f - XRHIP_PIXFMT_GRAY10_MIPI;
        for (int bits : {0, 7, 10, 17})   // (not read)
            for (int lim : {0, 1}) {
                CHECK(xrh::describe_pixel_format(f, bits, lim, pf) == nullptr);
                CHECK(!pf.bayer && pf.limited == (lim != 0) && pf.bits == ((p & 1) ? 12 : 10) && pf.shift == (uint32_t)pf.bits - 8);
                CHECK(pf.packing == (p < 2 ? xrh::PixelFormat::PACK_MIPI : xrh::PixelFormat::PACK_LSB));
            }
    }
    for (int f = XRHIP_PIXFMT_BAYER_RGGB10_MIPI; f <= XRHIP_PIXFMT_BAYER_BGGR12P; ++f) {
        const int p = (f - 40) >> 2, pattern = (f - 40) & 3;
        const char *why = xrh::describe_pixel_format(f, 0, 1, pf);
        CHECK(why != nullptr && std::strstr(why, "limited_range") != nullptr);
        CHECK(xrh::describe_pixel_format(f, 17, 0, pf) == nullptr);
        CHECK(pf.bayer && pf.px == (pattern & 1) && pf.py == (pattern >> 1) && pf.bits == ((p & 1) ? 12 : 10));
        CHECK(pf.packing == (p < 2 ? xrh::PixelFormat::PACK_MIPI : xrh::PixelFormat::PACK_LSB));
    }
    // row bytes, and the stride rule: the packed bytes of a row of src_width pixels
    {
        CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY10_MIPI, 0, 0, pf) == nullptr);
        CHECK(pf.row_bytes(1) == 5 && pf.row_bytes(4) == 5 && pf.row_bytes(5) == 10 && pf.row_bytes(752) == 940);
        const xrhip_frame_geometry g{70, 67, 3, 5, 61, 59};
        CHECK(xrh::check_frame_geometry(&g, 32, 32, pf, 90) == nullptr);
        const char *why = xrh::check_frame_geometry(&g, 32, 32, pf, 89);
        CHECK(why != nullptr && std::strstr(why, "stride") != nullptr);
        CHECK(xrh::check_frame_geometry(nullptr, 32, 32, pf, 90) != nullptr);
        CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY12_MIPI, 0, 0, pf) == nullptr);
        CHECK(pf.row_bytes(1) == 3 && pf.row_bytes(2) == 3 && pf.row_bytes(3) == 6 && pf.row_bytes(752) == 1128);
        CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY10P, 0, 0, pf) == nullptr);
        CHECK(pf.row_bytes(1) == 2 && pf.row_bytes(3) == 4 && pf.row_bytes(4) == 5 && pf.row_bytes(5) == 7);
        CHECK(xrh::check_frame_geometry(&g, 32, 32, pf, 88) == nullptr && xrh::check_frame_geometry(&g, 32, 32, pf, 87) != nullptr);
        CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY12P, 0, 0, pf) == nullptr);
        CHECK(pf.row_bytes(1) == 2 && pf.row_bytes(2) == 3 && pf.row_bytes(3) == 5);
        // the unpacked formats keep theirs
        CHECK(xrh::describe_pixel_format(XRHIP_PIXFMT_GRAY16, 10, 0, pf) == nullptr && pf.packing == xrh::PixelFormat::PACK_NONE && pf.row_bytes(7) == 14);
        CHECK(xrh::check_frame_geometry(&g, 32, 32, pf, 140) == nullptr && xrh::check_frame_geometry(&g, 32, 32, pf, 139) != nullptr);
    }
    if (argc < 2) {
        std::printf("usage: packed_host <case file>\n");
        return 2;
    }
    std::FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t hd[14];
    int k = 0;
    while (std::fread(hd, sizeof(int32_t), 14, fp) == 14) {
        const int format = hd[0], lim = hd[1], stride = hd[2], offset = hd[3], scaled = hd[4], W = hd[5], H = hd[6];
        const xrhip_frame_geometry geo{hd[7], hd[8], hd[9], hd[10], hd[11], hd[12]};
        const size_t nbytes = (size_t)hd[13];
        uint8_t *block = static_cast<uint8_t *>(std::malloc(nbytes));   // exactly the frame: first byte to last needed byte
        if (std::fread(block, 1, nbytes, fp) != nbytes) {
            std::printf("case %d: short file\n", k);
            return 2;
        }
        CHECK(xrh::describe_pixel_format(format, 0, lim, pf) == nullptr);
        std::vector<uint8_t> plane((size_t)W * H, 0x5a);
        if (scaled) {
            CHECK(xrh::check_frame_geometry(&geo, W, H, pf, stride) == nullptr);
            CHECK(nbytes == (size_t)offset + (size_t)stride * (geo.crop_y + geo.crop_height - 1) + (size_t)pf.row_bytes(geo.crop_x + geo.crop_width));
            int x0 = -1;
            const uint8_t *rows = xrh::crop_rows(block + offset, stride, geo, pf, x0);
            CHECK(x0 >= 0 && x0 < pf.group_px());
            xrh::scale_frame(plane.data(), W, H, rows, stride, geo.crop_width, geo.crop_height, xrh::crop_pixel_format(pf, geo), x0);
            // staged like a host frame's crop: the byte groups that hold a crop pixel, packed (pack_rows), give the same plane
            const size_t row = (size_t)pf.row_bytes(x0 + geo.crop_width);
            uint8_t *slot = static_cast<uint8_t *>(std::malloc(row * geo.crop_height));
            xrh::pack_rows(slot, rows, stride, row, geo.crop_height);
            std::vector<uint8_t> again((size_t)W * H, 0xa5);
            xrh::scale_frame(again.data(), W, H, slot, (long long)row, geo.crop_width, geo.crop_height, xrh::crop_pixel_format(pf, geo), x0);
            CHECK(again == plane);
            std::free(slot);
        } else {
            CHECK(nbytes == (size_t)offset + (size_t)stride * (H - 1) + (size_t)pf.row_bytes(W));
            xrh::reduce_frame(plane.data(), block + offset, stride, W, H, pf);
        }
        std::printf("case %d %016llx\n", k, fnv1a(plane));
        std::free(block);
        ++k;
    }
    std::fclose(fp);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
