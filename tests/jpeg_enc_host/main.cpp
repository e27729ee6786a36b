// A stand-alone driver for the host half of the JPEG encoder in csrc/jpeg.cpp (quality scaling, Annex K tables, derived codes, header
// writer), built with g++ -fsanitize=address,undefined by tests/test_jpeg_encode_cpu.py.  For every quality 0..101 and every size of
// {1, 7, 8, 4096} squared it builds the tables and writes one record to the output file:
//     int32 width, int32 height, int32 quality, 328 header bytes, 64 uint16 divisors, 12 uint32 DC codes, 256 uint32 AC codes
// It checks what must hold for any input itself: the divisors are 8 .. 2040 and multiples of 8, the codes are prefix-free with lengths
// 1..16 and 162 + 12 of them, the size bound is a multiple of 16 that holds header, worst-case payload and EOI, and bad sizes are refused.
#include <cstdio>
#include <cstring>
#include <vector>

#include "jpeg.h"

static int fail(const char* what, int a, int b, int c) {
    std::printf("jpeg enc host: FAILED %s (%d, %d, %d)\n", what, a, b, c);
    return 1;
}

static bool prefix_free(const std::vector<uint32_t>& codes) {
    for (size_t i = 0; i < codes.size(); ++i)
        for (size_t j = 0; j < codes.size(); ++j) {
            if (i == j) continue;
            const uint32_t li = codes[i] & 255u, lj = codes[j] & 255u;
            if (li <= lj && (codes[j] >> 8) >> (lj - li) == (codes[i] >> 8)) return false;
        }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    const int sizes[4] = {1, 7, 8, 4096};
    int records = 0;
    for (int q = 0; q <= 101; ++q)
        for (int si = 0; si < 4; ++si) {
            const int w = sizes[si], h = sizes[si];
            cvjpeg::EncTables t;
            std::memset(&t, 0xA5, sizeof t);
            if (cvjpeg::encoder_tables(w, h, q, &t) != cvjpeg::kOk) return fail("encoder_tables", w, h, q);
            uint16_t qt[64];
            cvjpeg::quant_table(q, qt);
            for (int k = 0; k < 64; ++k) {
                if (qt[k] < 1 || qt[k] > 255) return fail("quant range", q, k, qt[k]);
                if (t.divisor[k] < 8 || t.divisor[k] > 2040 || t.divisor[k] % 8) return fail("divisor", q, k, t.divisor[k]);
            }
            if (cvjpeg::clamp_quality(q) != (q < 1 ? 1 : q > 100 ? 100 : q)) return fail("clamp", q, 0, 0);
            std::vector<uint32_t> dc, ac;
            for (int k = 0; k < 12; ++k) dc.push_back(t.dc[k]);
            for (int k = 0; k < 256; ++k) if (t.ac[k]) ac.push_back(t.ac[k]);
            if (ac.size() != 162) return fail("ac count", (int)ac.size(), 0, 0);
            for (uint32_t c : dc) if ((c & 255u) < 1 || (c & 255u) > 9) return fail("dc length", (int)c, 0, 0);
            for (uint32_t c : ac) if ((c & 255u) < 1 || (c & 255u) > 16) return fail("ac length", (int)c, 0, 0);
            if (!prefix_free(dc) || !prefix_free(ac)) return fail("prefix", q, 0, 0);
            const size_t blocks = (size_t)((w + 7) / 8) * ((h + 7) / 8), cap = cvjpeg::gray_max_bytes(w, h);
            if (cap % 16 || cap < 328 + 2 * ((blocks * cvjpeg::kEncMaxBlockBits + 7) / 8) + 2) return fail("bound", w, h, (int)cap);
            const int32_t head[3] = {w, h, q};
            std::fwrite(head, 4, 3, f);
            std::fwrite(t.header, 1, sizeof t.header, f);
            std::fwrite(t.divisor, 2, 64, f);
            std::fwrite(t.dc, 4, 12, f);
            std::fwrite(t.ac, 4, 256, f);
            ++records;
        }
    cvjpeg::EncTables t;
    if (cvjpeg::encoder_tables(0, 8, 50, &t) == cvjpeg::kOk || cvjpeg::encoder_tables(8, 65536, 50, &t) == cvjpeg::kOk ||
        cvjpeg::encoder_tables(8, 8, 50, nullptr) == cvjpeg::kOk)
        return fail("bad sizes accepted", 0, 0, 0);
    std::fclose(f);
    std::printf("jpeg enc host: ok records: %d\n", records);
    return 0;
}
