// A stand-alone driver for the host half of the COLOUR JPEG encoder in csrc/jpeg.cpp (the second table set, the 623-byte header, the
// size bounds), built with g++ -fsanitize=address,undefined by tests/test_jpeg_colour_encode_cpu.py.  For every quality 0..101, every
// size of {1, 7, 8, 4096} squared and the three subsamplings it builds the tables and writes one record to the output file:
//     int32 width, height, quality, hs, vs, 623 header bytes, 2 x 64 uint16 divisors, 2 x 12 uint32 DC codes, 2 x 256 uint32 AC codes
// It checks what must hold for any input itself: divisors 8 .. 2040 and multiples of 8, both code sets prefix-free with 12 + 162 codes
// (DC lengths up to 9 for luma, 11 for chroma), set 0 equal to the gray encoder's, the bounds multiples of 16 that hold header,
// worst-case payload (dummy blocks counted) and EOI, a gray scan's tables carried over unchanged, and bad arguments refused.
#include <cstdio>
#include <cstring>
#include <vector>

#include "jpeg.h"

static int fail(const char* what, int a, int b, int c) {
    std::printf("jpeg enc colour host: FAILED %s (%d, %d, %d)\n", what, a, b, c);
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
    const int subs[3][2] = {{2, 2}, {2, 1}, {1, 1}};
    int records = 0;
    for (int q = 0; q <= 101; ++q)
        for (int si = 0; si < 4; ++si)
            for (int ss = 0; ss < 3; ++ss) {
                const int w = sizes[si], h = sizes[si], hs = subs[ss][0], vs = subs[ss][1];
                cvjpeg::ScanTables t;
                std::memset(&t, 0xA5, sizeof t);
                if (cvjpeg::colour_encoder_tables(w, h, q, hs, vs, &t) != cvjpeg::kOk) return fail("colour_encoder_tables", w, q, ss);
                if (t.header_bytes != cvjpeg::kColourHeaderBytes || t.header[cvjpeg::kColourHeaderBytes] != 0) return fail("header length", w, q, ss);
                cvjpeg::EncTables g;
                if (cvjpeg::encoder_tables(w, h, q, &g) != cvjpeg::kOk) return fail("encoder_tables", w, h, q);
                if (std::memcmp(g.divisor, t.divisor[0], sizeof g.divisor) || std::memcmp(g.dc, t.dc[0], sizeof g.dc) ||
                    std::memcmp(g.ac, t.ac[0], sizeof g.ac))
                    return fail("set 0 is not the gray encoder's", w, q, ss);
                uint16_t qt[64];
                cvjpeg::chroma_quant_table(q, qt);
                for (int k = 0; k < 64; ++k) {
                    if (qt[k] < 1 || qt[k] > 255) return fail("quant range", q, k, qt[k]);
                    for (int s = 0; s < 2; ++s)
                        if (t.divisor[s][k] < 8 || t.divisor[s][k] > 2040 || t.divisor[s][k] % 8) return fail("divisor", q, k, t.divisor[s][k]);
                }
                for (int s = 0; s < 2; ++s) {
                    std::vector<uint32_t> dc, ac;
                    for (int k = 0; k < 12; ++k) dc.push_back(t.dc[s][k]);
                    for (int k = 0; k < 256; ++k) if (t.ac[s][k]) ac.push_back(t.ac[s][k]);
                    if (ac.size() != 162) return fail("ac count", (int)ac.size(), s, 0);
                    for (uint32_t c : dc) if ((c & 255u) < 1 || (c & 255u) > (s ? 11u : 9u)) return fail("dc length", (int)c, s, 0);
                    for (uint32_t c : ac) if ((c & 255u) < 1 || (c & 255u) > 16) return fail("ac length", (int)c, s, 0);
                    if (!prefix_free(dc) || !prefix_free(ac)) return fail("prefix", q, s, 0);
                }
                const size_t mcus = (size_t)((w + 8 * hs - 1) / (8 * hs)) * ((h + 8 * vs - 1) / (8 * vs));
                const size_t bits = mcus * ((size_t)hs * vs * cvjpeg::kEncMaxBlockBits + 2 * (size_t)cvjpeg::kEncMaxChromaBlockBits);
                const size_t cap = cvjpeg::colour_max_bytes(w, h, hs, vs);
                if (cvjpeg::colour_coded_blocks(w, h, hs, vs) != mcus * (size_t)(hs * vs + 2)) return fail("blocks", w, h, ss);
                if (cvjpeg::colour_max_bits(w, h, hs, vs) != bits) return fail("bits", w, h, ss);
                if (cap % 16 || cap < 623 + 2 * ((bits + 7) / 8) + 2 || cap >= ((size_t)1 << 31)) return fail("bound", w, h, ss);
                const int32_t head[5] = {w, h, q, hs, vs};
                std::fwrite(head, 4, 5, f);
                std::fwrite(t.header, 1, cvjpeg::kColourHeaderBytes, f);
                std::fwrite(t.divisor, 2, 128, f);
                std::fwrite(t.dc, 4, 24, f);
                std::fwrite(t.ac, 4, 512, f);
                cvjpeg::ScanTables s;
                std::memset(&s, 0xA5, sizeof s);
                cvjpeg::scan_tables_of(g, &s);
                if (s.header_bytes != cvjpeg::kGrayHeaderBytes || std::memcmp(s.header, g.header, cvjpeg::kGrayHeaderBytes) ||
                    std::memcmp(s.divisor[0], g.divisor, sizeof g.divisor) || std::memcmp(s.ac[0], g.ac, sizeof g.ac) || s.ac[1][1] != 0 ||
                    s.header[cvjpeg::kGrayHeaderBytes] != 0)
                    return fail("scan_tables_of", w, h, q);
                ++records;
            }
    cvjpeg::ScanTables t;
    if (cvjpeg::colour_encoder_tables(0, 8, 50, 2, 2, &t) == cvjpeg::kOk || cvjpeg::colour_encoder_tables(8, 65536, 50, 2, 2, &t) == cvjpeg::kOk ||
        cvjpeg::colour_encoder_tables(8, 8, 50, 2, 2, nullptr) == cvjpeg::kOk || cvjpeg::colour_encoder_tables(8, 8, 50, 1, 2, &t) == cvjpeg::kOk ||
        cvjpeg::colour_encoder_tables(8, 8, 50, 4, 1, &t) == cvjpeg::kOk || cvjpeg::colour_encoder_tables(8, 8, 50, 0, 0, &t) == cvjpeg::kOk)
        return fail("bad arguments accepted", 0, 0, 0);
    std::fclose(f);
    std::printf("jpeg enc colour host: ok records: %d\n", records);
    return 0;
}
