// Stand-alone check of the PNG decode core (satlas_super_resolution_amd/csrc/png_inflate.h) for sanitizer builds:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -I satlas_super_resolution_amd/csrc tools/png_inflate_check.cpp -o png_inflate_check
//     ./png_inflate_check cases.bin
//
// cases.bin (written by tests/test_png_device_host.py from the corpus and the malformed set) is a sequence of records:
//     int32 width, height, channels, stream bytes, expected bytes (0: a damaged stream, only "returns, stays in bounds" is asked)
//     the stream, the expected pixels
// Every buffer is a heap block of exactly the size the decoder may touch, so a read or write outside an item's ranges is an
// AddressSanitizer report.  Exit 0: every record with expected pixels decoded to them with status 0 and every record returned.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_inflate.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int n = 0, failed = 0, statuses[16] = {0};
    int32_t head[5];
    pngi_work wk;
    while (std::fread(head, sizeof(int32_t), 5, f) == 5) {
        const int32_t w = head[0], h = head[1], c = head[2], src_len = head[3], exp_len = head[4];
        if (w < 1 || h < 1 || (c != 1 && c != 3) || src_len < 0 || (exp_len != 0 && exp_len != w * h * c)) {
            std::fprintf(stderr, "record %d: bad header\n", n);
            return 2;
        }
        // exact-size heap blocks (malloc(0) may be null: one spare byte is never handed to the decoder as length)
        uint8_t* src = static_cast<uint8_t*>(std::malloc(src_len ? src_len : 1));
        uint8_t* raw = static_cast<uint8_t*>(std::malloc((size_t)h * ((size_t)w * c + 1)));
        uint8_t* dst = static_cast<uint8_t*>(std::malloc((size_t)h * w * c));
        std::vector<uint8_t> expect(exp_len);
        if ((src_len && std::fread(src, 1, src_len, f) != (size_t)src_len) ||
            (exp_len && std::fread(expect.data(), 1, exp_len, f) != (size_t)exp_len)) {
            std::fprintf(stderr, "record %d: short file\n", n);
            return 2;
        }
        const int st = pngi_decode_image(src, (uint32_t)src_len, (uint32_t)w, (uint32_t)h, (uint32_t)c, raw, dst, &wk, 0, 1);
        if (st >= 0 && st < 16) statuses[st]++;
        if (exp_len && (st != PNGI_OK || std::memcmp(dst, expect.data(), exp_len) != 0)) {
            std::fprintf(stderr, "record %d (%d x %d x %d): status %d%s\n", n, w, h, c, st, st == PNGI_OK ? ", pixels differ" : "");
            ++failed;
        }
        std::free(src);
        std::free(raw);
        std::free(dst);
        ++n;
    }
    std::fclose(f);
    std::printf("%d records, %d failed; statuses:", n, failed);
    for (int k = 0; k < 13; ++k) std::printf(" %d:%d", k, statuses[k]);
    std::printf("\n");
    return failed ? 1 : 0;
}
