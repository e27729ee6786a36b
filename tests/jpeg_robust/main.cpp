// Robustness driver for csrc/jpeg.cpp, built with -fsanitize=address,undefined by tests/test_jpeg_robust_cpu.py and run as an ordinary
// child process.  Input: a file of streams (u32 little-endian length + bytes, repeated).  For every stream it feeds the decoder
// every truncation length and 2000 seeded single-byte corruptions.  The decoder must answer kOk or kInvalid every time; the output
// arrays are heap blocks of exactly the size the parsed header asks for, so that a write past either end is the sanitizer's to report.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "jpeg.h"

namespace {

struct Counts { long long calls = 0, ok = 0, refused = 0, big = 0; };

bool drive(const uint8_t* data, size_t len, Counts& n) {
    // the decoder sees a heap copy of exactly `len` bytes: reading data[len] is an error the sanitizer reports
    std::vector<uint8_t> copy(data, data + len);
    const uint8_t* p = copy.empty() ? reinterpret_cast<const uint8_t*>("") : copy.data();
    cvjpeg::Info info;
    if (cvjpeg::parse_info(p, len, &info) != cvjpeg::kOk) return false;
    if (std::memchr(info.reason, 0, sizeof info.reason) == nullptr) return false;
    ++n.calls;
    size_t count = 64, comps = 3;
    if (info.supported) {
        const cvjpeg::Layout lay = cvjpeg::layout_of(info);
        count = lay.blocks * 64;
        comps = (size_t)info.components;
        if (count > ((size_t)1 << 24)) { count = 1; ++n.big; }          // a corrupted header may ask for gigabytes: too small a buffer
    }                                                                   // is a refusal of its own ("coefficient buffer too small")
    std::vector<int16_t> coeffs(count);
    std::vector<uint16_t> qt(comps * 64);
    char err[200] = "";
    const int rc = cvjpeg::entropy_decode(p, len, coeffs.data(), count, qt.data(), nullptr, err, sizeof err);
    if (rc == cvjpeg::kOk) { ++n.ok; return info.supported != 0; }
    if (rc != cvjpeg::kInvalid || err[0] == 0) return false;
    ++n.refused;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s STREAMS\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<std::vector<uint8_t>> streams;
    for (;;) {
        uint8_t l4[4];
        if (std::fread(l4, 1, 4, f) != 4) break;
        const size_t len = (size_t)l4[0] | (size_t)l4[1] << 8 | (size_t)l4[2] << 16 | (size_t)l4[3] << 24;
        std::vector<uint8_t> s(len);
        if (len && std::fread(s.data(), 1, len, f) != len) { std::fprintf(stderr, "short stream file\n"); return 2; }
        streams.push_back(std::move(s));
    }
    std::fclose(f);
    // streams are independent: a few threads take them in turn (the decoder keeps no state between calls); every stream has its own seed
    const unsigned n_threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<Counts> counts(n_threads);
    std::atomic<size_t> next_stream{0};
    std::atomic<int> failed{0};
    auto work = [&](unsigned t) {
        Counts& n = counts[t];
        for (size_t i = next_stream++; i < streams.size() && !failed; i = next_stream++) {
            std::vector<uint8_t> s = streams[i];
            uint64_t rng = 0x9E3779B97F4A7C15ull * (i + 1);
            auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
            for (size_t cut = 0; cut <= s.size(); ++cut)
                if (!drive(s.data(), cut, n)) { std::printf("stream %zu: bad answer at truncation %zu\n", i, cut); failed = 1; return; }
            for (int k = 0; k < 2000 && !s.empty(); ++k) {
                const size_t at = (size_t)(next() % s.size());
                const uint8_t old = s[at];
                s[at] = (uint8_t)(old ^ (1 + next() % 255));
                const bool fine = drive(s.data(), s.size(), n);
                s[at] = old;
                if (!fine) { std::printf("stream %zu: bad answer with byte %zu corrupted\n", i, at); failed = 1; return; }
            }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < n_threads; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
    if (failed) return 1;
    Counts n;
    for (const Counts& c : counts) { n.calls += c.calls; n.ok += c.ok; n.refused += c.refused; n.big += c.big; }
    std::printf("streams: %zu\ncalls: %lld ok %lld refused %lld oversized %lld\njpeg robust: ok\n", streams.size(), n.calls, n.ok, n.refused, n.big);
    return 0;
}
