// Stand-alone check of the player's --mask loader (xrslam_amd/csrc/player/euroc_io.hpp: decode_pgm, load_mask): its own main, no GPU
// code, never loaded into Python; tests/test_mask_cpu.py builds it with AddressSanitizer and UBSan.
//   mask_host W H FILE...   per file one line: "ok <w> <h> <fnv1a of the pixels> <nonzero bytes>" or "error <message>"
// The file's bytes live in a heap block of exactly the file's size (read_file), so a read past a truncated file is reported.
#include <cstdio>
#include <cstdlib>

#include "../../xrslam_amd/csrc/player/euroc_io.hpp"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
    for (int i = 3; i < argc; ++i) {
        try {
            const xrplayer::GrayImage m = xrplayer::load_mask(xrplayer::read_file(argv[i]), w, h);
            unsigned long long hash = 1469598103934665603ull;
            long nz = 0;
            for (uint8_t b : m.px) {
                hash = (hash ^ b) * 1099511628211ull;
                nz += b != 0;
            }
            std::printf("ok %d %d %016llx %ld\n", m.w, m.h, hash, nz);
        } catch (const std::exception &e) {
            std::printf("error %s\n", e.what());
        }
    }
    return 0;
}
