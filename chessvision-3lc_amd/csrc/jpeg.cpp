// jpeg.cpp -- marker parser and Huffman stage of the JPEG decoder (ITU-T T.81, baseline / extended sequential Huffman, 8 bit).
//
// The serial half of a decode: one image per host thread, quantised coefficients out.  Everything after it (dequantise, inverse
// DCT, chroma up-sampling, colour conversion) is arithmetic with no data dependence between blocks and lives in jpeg.hip.
//
// The input is an untrusted upload.  Every read goes through a position that is compared with the buffer length first, every table
// index is masked or range-checked, every loop bound comes from the validated header, and a stream that needs one bit more than
// the buffer holds is refused: nothing partial is returned.
#include "jpeg.h"

#include <cstdio>
#include <cstring>

namespace cvjpeg {
namespace {

const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

const int kLook = 9;                       // look-ahead bits: one table access resolves every code of up to 9 bits

struct HuffTable {
    bool defined = false;
    uint16_t look[1 << kLook];             // (length << 8) | symbol for codes of <= kLook bits, 0 otherwise
    int32_t maxcode[17];                   // largest code of each length, -1 when the length has none
    int32_t valoffset[17];                 // index of a length's first symbol minus its first code
    uint8_t vals[256];
};

struct Decoder {
    const uint8_t* p;
    size_t len;
    size_t pos = 0;
    Info info;
    uint16_t qt[4][64];                    // natural order
    bool qt_def[4] = {false, false, false, false};
    HuffTable dc[4], ac[4];
    int comp_id[3], comp_tq[3], comp_td[3], comp_ta[3];
    bool have_sof = false, adobe = false;
    int adobe_transform = 0;
    // bit reader: `bits` low bits of acc are unread; the lowest `fake` of them are zeros fed past the end of the entropy data
    uint64_t acc = 0;
    int bits = 0;
    long long fake = 0;
    bool at_end = false;

    Decoder(const uint8_t* data, size_t n) : p(data), len(n) { std::memset(&info, 0, sizeof info); }

    int refuse(size_t offset, const char* why) {
        if (len && offset >= len) offset = len - 1;
        std::snprintf(info.reason, sizeof info.reason, "%s at byte %zu", why, offset);
        info.supported = 0;
        return kInvalid;
    }
    static unsigned be16(const uint8_t* q) { return (unsigned)q[0] << 8 | q[1]; }

    void exif_orientation(const uint8_t* t, size_t n) {       // t: the TIFF header inside an APP1 "Exif" segment
        if (n < 8) return;
        const bool le = t[0] == 'I' && t[1] == 'I';
        if (!le && !(t[0] == 'M' && t[1] == 'M')) return;
        auto r16 = [&](size_t o) -> unsigned { return le ? (unsigned)t[o] | (unsigned)t[o + 1] << 8 : (unsigned)t[o] << 8 | t[o + 1]; };
        auto r32 = [&](size_t o) -> size_t { return le ? (size_t)r16(o) | (size_t)r16(o + 2) << 16 : (size_t)r16(o) << 16 | r16(o + 2); };
        if (r16(2) != 42) return;
        const size_t ifd = r32(4);
        if (ifd > n || n - ifd < 2) return;
        const unsigned count = r16(ifd);
        for (unsigned i = 0; i < count; ++i) {
            const size_t e = ifd + 2 + (size_t)12 * i;
            if (e > n || n - e < 12) return;
            if (r16(e) == 0x0112 && r16(e + 2) == 3 && r32(e + 4) == 1) {
                const unsigned v = r16(e + 8);
                if (v >= 1 && v <= 8) info.orientation = (int32_t)v;
                return;
            }
        }
    }

    int define_huffman(const uint8_t* seg, size_t n, size_t at) {
        while (n > 0) {
            if (n < 17) return refuse(at, "corrupt DHT segment");
            const int tc = seg[0] >> 4, th = seg[0] & 15;
            if (tc > 1 || th > 3) return refuse(at, "corrupt DHT segment (table class or id)");
            int total = 0;
            for (int i = 1; i <= 16; ++i) total += seg[i];
            if (total > 256 || (size_t)total > n - 17) return refuse(at, "corrupt DHT segment (symbol count)");
            HuffTable& t = tc ? ac[th] : dc[th];
            std::memset(t.look, 0, sizeof t.look);
            std::memset(t.vals, 0, sizeof t.vals);
            std::memcpy(t.vals, seg + 17, (size_t)total);
            int code = 0, k = 0;
            for (int l = 1; l <= 16; ++l) {
                const int cnt = seg[l];
                t.valoffset[l] = k - code;
                if (code + cnt > (1 << l)) return refuse(at, "corrupt DHT segment (code lengths over-subscribed)");
                if (l <= kLook)
                    for (int i = 0; i < cnt; ++i) {
                        const int first = (code + i) << (kLook - l);
                        for (int j = 0; j < (1 << (kLook - l)); ++j) t.look[first + j] = (uint16_t)(l << 8 | t.vals[k + i]);
                    }
                code += cnt;
                k += cnt;
                t.maxcode[l] = cnt ? code - 1 : -1;
                code <<= 1;
            }
            t.defined = true;
            seg += 17 + total;
            n -= 17 + (size_t)total;
        }
        return kOk;
    }

    int define_quant(const uint8_t* seg, size_t n, size_t at) {
        while (n > 0) {
            const int pq = seg[0] >> 4, tq = seg[0] & 15;
            if (pq > 1 || tq > 3) return refuse(at, "corrupt DQT segment (precision or id)");
            const size_t need = 1 + (pq ? 128u : 64u);
            if (n < need) return refuse(at, "corrupt DQT segment (short table)");
            for (int i = 0; i < 64; ++i) qt[tq][kNatural[i]] = (uint16_t)(pq ? be16(seg + 1 + 2 * i) : seg[1 + i]);
            qt_def[tq] = true;
            seg += need;
            n -= need;
        }
        return kOk;
    }

    int start_of_frame(const uint8_t* seg, size_t n, size_t at) {
        if (have_sof) return refuse(at, "corrupt stream (second frame header)");
        if (n < 6) return refuse(at, "corrupt SOF segment");
        const int prec = seg[0], nf = seg[5];
        const unsigned hh = be16(seg + 1), ww = be16(seg + 3);
        if (prec == 12) return refuse(at, "12-bit precision is not supported");
        if (prec != 8) return refuse(at, "unsupported sample precision");
        if (nf == 4) return refuse(at, "4-component (CMYK/YCCK) streams are not supported");
        if (nf != 1 && nf != 3) return refuse(at, "unsupported component count");
        if (n != (size_t)6 + 3 * (size_t)nf) return refuse(at, "corrupt SOF segment (length)");
        if (hh == 0) return refuse(at, "frame height 0 (DNL) is not supported");
        if (ww == 0) return refuse(at, "corrupt SOF segment (width 0)");
        if ((uint64_t)ww * hh > ((uint64_t)1 << 28)) return refuse(at, "image of more than 2^28 pixels");
        int hs[3], vs[3];
        for (int c = 0; c < nf; ++c) {
            comp_id[c] = seg[6 + 3 * c];
            hs[c] = seg[7 + 3 * c] >> 4;
            vs[c] = seg[7 + 3 * c] & 15;
            comp_tq[c] = seg[8 + 3 * c];
            if (hs[c] < 1 || hs[c] > 4 || vs[c] < 1 || vs[c] > 4 || comp_tq[c] > 3) return refuse(at, "corrupt SOF segment (component)");
        }
        info.luma_h = info.luma_v = 1;      // a 1-component scan is not interleaved: its sampling factors mean nothing
        if (nf == 3) {
            const bool luma_ok = (hs[0] == 1 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 2);
            if (!luma_ok || hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1)
                return refuse(at, "unsupported sampling factors (luma 1x1, 2x1 or 2x2 with chroma 1x1 only)");
            info.luma_h = hs[0];
            info.luma_v = vs[0];
        }
        info.width = (int32_t)ww;
        info.height = (int32_t)hh;
        info.components = nf;
        have_sof = true;
        return kOk;
    }

    int start_of_scan(const uint8_t* seg, size_t n, size_t at) {
        if (!have_sof) return refuse(at, "corrupt stream (scan before frame header)");
        if (n < 1) return refuse(at, "corrupt SOS segment");
        const int ns = seg[0];
        if (ns < 1 || ns > 4 || n != (size_t)4 + 2 * (size_t)ns) return refuse(at, "corrupt SOS segment (length)");
        if (ns != info.components) return refuse(at, "multi-scan sequential streams are not supported");
        for (int c = 0; c < ns; ++c) {
            if (seg[1 + 2 * c] != comp_id[c]) return refuse(at, "unsupported scan component order");
            comp_td[c] = seg[2 + 2 * c] >> 4;
            comp_ta[c] = seg[2 + 2 * c] & 15;
            if (comp_td[c] > 3 || comp_ta[c] > 3 || !dc[comp_td[c]].defined || !ac[comp_ta[c]].defined)
                return refuse(at, "corrupt stream (scan names an undefined Huffman table)");
            if (!qt_def[comp_tq[c]]) return refuse(at, "corrupt stream (component names an undefined quantisation table)");
        }
        const uint8_t* tail = seg + 1 + 2 * ns;
        if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return refuse(at, "progressive scan parameters in a sequential frame");
        if (adobe && info.components == 3 && adobe_transform != 1) return refuse(at, "Adobe RGB streams (transform 0) are not supported");
        return kOk;
    }

    // markers up to and including the first SOS; pos is left on the first byte of entropy data
    int header() {
        if (len == 0 || (len == 1 && p[0] == 0xFF)) return refuse(0, "truncated inside SOI");
        if (len < 2 || p[0] != 0xFF || p[1] != 0xD8) return refuse(0, "not a JPEG stream (no SOI)");
        pos = 2;
        for (;;) {
            const size_t at = pos;
            if (pos >= len) return refuse(len, "truncated before the scan");
            if (p[pos] != 0xFF) return refuse(at, "corrupt stream (marker expected)");
            while (pos < len && p[pos] == 0xFF) ++pos;
            if (pos >= len) return refuse(at, "truncated inside a marker");
            const int m = p[pos++];
            if (m == 0x01) continue;                                                     // TEM
            if (m == 0xD9) return refuse(at, "corrupt stream (EOI before any scan)");
            if (m == 0x00 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7)) return refuse(at, "corrupt stream (unexpected marker)");
            if (len - pos < 2) return refuse(at, "truncated inside a marker");
            const size_t seg_len = be16(p + pos);
            if (seg_len < 2) return refuse(at, "corrupt segment length");
            if (len - pos < seg_len) return refuse(at, m == 0xC4 || m == 0xDB ? "truncated inside a table" : "truncated inside a marker segment");
            const uint8_t* seg = p + pos + 2;
            const size_t n = seg_len - 2;
            pos += seg_len;
            int rc = kOk;
            switch (m) {
                case 0xC0: case 0xC1: rc = start_of_frame(seg, n, at); break;
                case 0xC2: return refuse(at, "progressive streams are not supported");
                case 0xC3: case 0xC7: case 0xCB: case 0xCF: return refuse(at, "lossless streams are not supported");
                case 0xC5: case 0xC6: case 0xCD: case 0xCE: return refuse(at, "hierarchical (differential) streams are not supported");
                case 0xC9: case 0xCA: case 0xCC: return refuse(at, "arithmetic-coded streams are not supported");
                case 0xC8: return refuse(at, "corrupt stream (reserved marker)");
                case 0xDE: case 0xDF: return refuse(at, "hierarchical streams are not supported");
                case 0xDC: return refuse(at, "DNL is not supported");
                case 0xC4: rc = define_huffman(seg, n, at); break;
                case 0xDB: rc = define_quant(seg, n, at); break;
                case 0xDD:
                    if (n != 2) return refuse(at, "corrupt DRI segment");
                    info.restart_interval = (int32_t)be16(seg);
                    break;
                case 0xE1:
                    if (n >= 6 && std::memcmp(seg, "Exif\0\0", 6) == 0) exif_orientation(seg + 6, n - 6);
                    break;
                case 0xEE:
                    if (n >= 12 && std::memcmp(seg, "Adobe", 5) == 0) { adobe = true; adobe_transform = seg[11]; }
                    break;
                case 0xDA:
                    if ((rc = start_of_scan(seg, n, at)) != kOk) return rc;
                    info.supported = 1;
                    info.reason[0] = 0;
                    return kOk;
                default: break;                                                          // APPn, COM, JPGn: skipped
            }
            if (rc != kOk) return rc;
        }
    }

    // ---- entropy data ----------------------------------------------------------------------------------------------
    inline void fill() {
        if (!at_end && bits <= 32 && len - pos >= 4) {          // four bytes at once when none of them is FF (no stuffing, no marker)
            const uint32_t w = (uint32_t)p[pos] << 24 | (uint32_t)p[pos + 1] << 16 | (uint32_t)p[pos + 2] << 8 | p[pos + 3];
            const uint32_t inv = ~w;
            if (((inv - 0x01010101u) & ~inv & 0x80808080u) == 0) {
                acc = acc << 32 | w;
                bits += 32;
                pos += 4;
                return;                                         // >= 32 bits: what a code and its extra bits need at the most
            }
        }
        while (bits <= 56) {
            uint32_t b = 0;
            if (!at_end) {
                if (pos < len) {
                    b = p[pos];
                    if (b != 0xFF) ++pos;
                    else if (len - pos >= 2 && p[pos + 1] == 0) pos += 2;                // stuffed zero after a data byte FF
                    else { at_end = true; b = 0; }                                      // a marker (or the buffer's end) stops the feed
                } else {
                    at_end = true;
                }
            }
            if (at_end) fake += 8;
            acc = acc << 8 | b;
            bits += 8;
        }
    }
    inline uint32_t peek(int n) const { return (uint32_t)(acc >> (bits - n)) & ((1u << n) - 1u); }
    inline int symbol(const HuffTable& t) {                    // needs bits >= 16
        const uint16_t e = t.look[peek(kLook)];
        if (e) { bits -= e >> 8; return e & 255; }
        for (int l = kLook + 1; l <= 16; ++l) {
            const int32_t code = (int32_t)peek(l);
            if (code <= t.maxcode[l]) { bits -= l; return t.vals[(code + t.valoffset[l]) & 255]; }
        }
        return -1;
    }
    inline int receive_extend(int s) {                        // 1 <= s <= 16, needs bits >= s
        const int v = (int)peek(s);
        bits -= s;
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }

    int block(int16_t* out, const HuffTable& dct, const HuffTable& act, uint32_t* pred) {
        if (bits < 32) fill();
        int s = symbol(dct);
        if (s < 0) return refuse(pos, "corrupt scan (Huffman code not in the DC table)");
        if (s > 15) return refuse(pos, "corrupt scan (DC category)");
        if (s) *pred += (uint32_t)receive_extend(s);
        out[0] = (int16_t)(uint16_t)*pred;
        for (int k = 1; k < 64; ++k) {
            if (bits < 32) fill();
            const int rs = symbol(act);
            if (rs < 0) return refuse(pos, "corrupt scan (Huffman code not in the AC table)");
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
                if (r != 15) break;                                                      // end of block
                k += 15;
                continue;
            }
            k += r;
            if (k > 63) return refuse(pos, "corrupt scan (coefficient index past 63)");
            out[kNatural[k]] = (int16_t)receive_extend(s);
        }
        if (bits < fake) return refuse(pos, "truncated inside the scan");
        return kOk;
    }

    int restart(int expect) {
        if (bits - fake >= 8) return refuse(pos, "corrupt scan (data where a restart marker belongs)");
        const size_t at = pos;
        if (pos >= len) return refuse(at, "truncated inside the scan");
        if (p[pos] != 0xFF) return refuse(at, "corrupt scan (restart marker expected)");
        while (pos < len && p[pos] == 0xFF) ++pos;
        if (pos >= len) return refuse(at, "truncated inside the scan");
        if (p[pos] != 0xD0 + expect) return refuse(at, p[pos] == 0xD9 ? "truncated inside the scan (EOI before the last MCU)" : "wrong restart marker");
        ++pos;
        acc = 0; bits = 0; fake = 0; at_end = false;
        return kOk;
    }

    int scan(int16_t* coeffs, const Layout& lay) {
        const int nc = info.components;
        const int hs = nc == 3 ? info.luma_h : 1, vs = nc == 3 ? info.luma_v : 1;
        const int mcus_x = lay.blocks_w[0] / hs, mcus_y = lay.blocks_h[0] / vs;
        uint32_t pred[3] = {0, 0, 0};
        const int ri = info.restart_interval;
        int until_restart = ri, next_rst = 0;
        for (int my = 0; my < mcus_y; ++my)
            for (int mx = 0; mx < mcus_x; ++mx) {
                if (ri) {
                    if (until_restart == 0) {
                        const int rc = restart(next_rst);
                        if (rc != kOk) return rc;
                        next_rst = (next_rst + 1) & 7;
                        until_restart = ri;
                        pred[0] = pred[1] = pred[2] = 0;
                    }
                    --until_restart;
                }
                for (int c = 0; c < nc; ++c) {
                    const int ch = c == 0 ? hs : 1, cvv = c == 0 ? vs : 1;
                    const HuffTable& dct = dc[comp_td[c]];
                    const HuffTable& act = ac[comp_ta[c]];
                    for (int v = 0; v < cvv; ++v)
                        for (int h = 0; h < ch; ++h) {
                            const size_t b = lay.block_off[c] + (size_t)(my * cvv + v) * lay.blocks_w[c] + (size_t)(mx * ch + h);
                            const int rc = block(coeffs + b * 64, dct, act, &pred[c]);
                            if (rc != kOk) return rc;
                        }
                }
            }
        // the scan must be followed by EOI: another scan, or no marker at all, is a stream this decoder does not take
        for (size_t q = pos; q + 1 < len; ++q) {
            if (p[q] != 0xFF || p[q + 1] == 0x00 || p[q + 1] == 0xFF) continue;
            if (p[q + 1] == 0xD9) return kOk;
            if (p[q + 1] == 0xDA || p[q + 1] == 0xC4 || p[q + 1] == 0xDB) return refuse(q, "multi-scan sequential streams are not supported");
            return refuse(q, "corrupt stream (unexpected marker after the scan)");
        }
        return refuse(len, "truncated: no EOI after the scan");
    }
};

}  // namespace

Layout layout_of(const Info& info) {
    Layout l;
    std::memset(&l, 0, sizeof l);
    l.ncomp = info.components;
    const int hs = info.components == 3 ? info.luma_h : 1, vs = info.components == 3 ? info.luma_v : 1;
    const int mcus_x = (info.width + 8 * hs - 1) / (8 * hs), mcus_y = (info.height + 8 * vs - 1) / (8 * vs);
    size_t off = 0;
    for (int c = 0; c < l.ncomp; ++c) {
        l.blocks_w[c] = mcus_x * (c == 0 ? hs : 1);
        l.blocks_h[c] = mcus_y * (c == 0 ? vs : 1);
        l.block_off[c] = off;
        off += (size_t)l.blocks_w[c] * l.blocks_h[c];
    }
    l.blocks = off;
    return l;
}

int parse_info(const uint8_t* data, size_t len, Info* info) {
    if (!info) return kInvalid;
    if (!data) {
        std::memset(info, 0, sizeof *info);
        std::snprintf(info->reason, sizeof info->reason, "null buffer");
        return kInvalid;
    }
    Decoder d(data, len);
    (void)d.header();
    *info = d.info;
    return kOk;
}

int entropy_decode(const uint8_t* data, size_t len, int16_t* coeffs, size_t capacity, uint16_t* qtables, Info* info_out, char* err,
                   size_t err_len) {
    auto say = [&](const char* msg) { if (err && err_len) std::snprintf(err, err_len, "%s", msg); };
    if (!data || !coeffs || !qtables) { say("null argument"); return kInvalid; }
    Decoder d(data, len);
    int rc = d.header();
    if (rc == kOk) {
        const Layout lay = layout_of(d.info);
        if (lay.blocks * 64 > capacity) {
            say("coefficient buffer too small for this stream");
            if (info_out) *info_out = d.info;
            return kInvalid;
        }
        std::memset(coeffs, 0, lay.blocks * 64 * sizeof(int16_t));
        for (int c = 0; c < d.info.components; ++c) std::memcpy(qtables + 64 * c, d.qt[d.comp_tq[c]], 64 * sizeof(uint16_t));
        rc = d.scan(coeffs, lay);
    }
    if (info_out) *info_out = d.info;
    if (rc != kOk) say(d.info.reason);
    return rc;
}

// ---- encoder: quality scaling, Annex K tables, derived codes, header ---------------------------------------------------------------
namespace {

const uint8_t kLumaQuant[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92, 95, 98,  112, 100, 103, 99};
const uint8_t kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// Annex C: the codes of a table given as its sixteen counts and its symbols, as (code << 8) | length at out[symbol]
void derive_codes(const uint8_t bits[16], const uint8_t* vals, int nvals, uint32_t* out, int nout) {
    uint32_t code = 0;
    int at = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int k = 0; k < bits[len - 1] && at < nvals; ++k, ++at, ++code)
            if (vals[at] < nout) out[vals[at]] = (code << 8) | (uint32_t)len;
        code <<= 1;
    }
}

}  // namespace

int clamp_quality(int quality) { return quality < 1 ? 1 : quality > 100 ? 100 : quality; }

void quant_table(int quality, uint16_t out[64]) {
    const int q = clamp_quality(quality);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; ++i) {
        const int v = (kLumaQuant[i] * scale + 50) / 100;
        out[i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

size_t gray_max_bytes(int width, int height) {
    const size_t blocks = (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
    const size_t payload = (blocks * kEncMaxBlockBits + 7) / 8;
    return (kGrayHeaderBytes + 2 * payload + 2 + 15) & ~(size_t)15;
}

int encoder_tables(int width, int height, int quality, EncTables* t) {
    if (!t || width < 1 || height < 1 || width > 65535 || height > 65535) return kInvalid;
    std::memset(t, 0, sizeof *t);
    uint16_t qt[64];
    quant_table(quality, qt);
    for (int k = 0; k < 64; ++k) t->divisor[k] = (uint16_t)(qt[kNatural[k]] << 3);
    derive_codes(kDcBits, kDcVals, 12, t->dc, 12);
    derive_codes(kAcBits, kAcVals, 162, t->ac, 256);
    uint8_t* p = t->header;
    const uint8_t app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    std::memcpy(p, app0, 20); p += 20;
    const uint8_t dqt[5] = {0xff, 0xdb, 0, 67, 0};
    std::memcpy(p, dqt, 5); p += 5;
    for (int k = 0; k < 64; ++k) *p++ = (uint8_t)qt[kNatural[k]];
    const uint8_t sof[13] = {0xff, 0xc0, 0, 11, 8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 1, 1, 0x11, 0};
    std::memcpy(p, sof, 13); p += 13;
    const uint8_t dht_dc[5] = {0xff, 0xc4, 0, 31, 0x00};
    std::memcpy(p, dht_dc, 5); p += 5;
    std::memcpy(p, kDcBits, 16); p += 16;
    std::memcpy(p, kDcVals, 12); p += 12;
    const uint8_t dht_ac[5] = {0xff, 0xc4, 0, 181, 0x10};
    std::memcpy(p, dht_ac, 5); p += 5;
    std::memcpy(p, kAcBits, 16); p += 16;
    std::memcpy(p, kAcVals, 162); p += 162;
    const uint8_t sos[10] = {0xff, 0xda, 0, 8, 1, 1, 0x00, 0, 63, 0};
    std::memcpy(p, sos, 10); p += 10;
    return (p - t->header) == kGrayHeaderBytes ? kOk : kInvalid;
}

// ---- colour: the second table set and the three-component header ---------------------------------------------------------------
namespace {

const uint8_t kChromaQuant[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kDc1Bits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kAc1Bits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAc1Vals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

int quality_scale(int quality) {
    const int q = clamp_quality(quality);
    return q < 50 ? 5000 / q : 200 - 2 * q;
}

uint8_t* put(uint8_t* p, const uint8_t* bytes, size_t n) {
    std::memcpy(p, bytes, n);
    return p + n;
}

uint8_t* put_dht(uint8_t* p, uint8_t cls_id, const uint8_t bits[16], const uint8_t* vals, int nvals) {
    const uint8_t head[5] = {0xff, 0xc4, 0, (uint8_t)(19 + nvals), cls_id};
    return put(put(put(p, head, 5), bits, 16), vals, (size_t)nvals);
}

}  // namespace

bool subsampling_ok(int hs, int vs) { return (hs == 2 && vs == 2) || (hs == 2 && vs == 1) || (hs == 1 && vs == 1); }

void chroma_quant_table(int quality, uint16_t out[64]) {
    const int scale = quality_scale(quality);
    for (int i = 0; i < 64; ++i) {
        const int v = (kChromaQuant[i] * scale + 50) / 100;
        out[i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

void scan_tables_of(const EncTables& gray, ScanTables* t) {
    std::memset(t, 0, sizeof *t);
    std::memcpy(t->divisor[0], gray.divisor, sizeof gray.divisor);
    std::memcpy(t->dc[0], gray.dc, sizeof gray.dc);
    std::memcpy(t->ac[0], gray.ac, sizeof gray.ac);
    std::memcpy(t->header, gray.header, kGrayHeaderBytes);
    t->header_bytes = kGrayHeaderBytes;
}

size_t colour_coded_blocks(int width, int height, int hs, int vs) {
    const size_t mcus = (size_t)((width + 8 * hs - 1) / (8 * hs)) * (size_t)((height + 8 * vs - 1) / (8 * vs));
    return mcus * (size_t)(hs * vs + 2);
}

size_t colour_max_bits(int width, int height, int hs, int vs) {
    const size_t mcus = colour_coded_blocks(width, height, hs, vs) / (size_t)(hs * vs + 2);
    return mcus * ((size_t)(hs * vs) * kEncMaxBlockBits + 2 * (size_t)kEncMaxChromaBlockBits);
}

size_t colour_max_bytes(int width, int height, int hs, int vs) {
    const size_t payload = (colour_max_bits(width, height, hs, vs) + 7) / 8;
    return (kColourHeaderBytes + 2 * payload + 2 + 15) & ~(size_t)15;
}

int colour_encoder_tables(int width, int height, int quality, int hs, int vs, ScanTables* t) {
    if (!t || width < 1 || height < 1 || width > 65535 || height > 65535 || !subsampling_ok(hs, vs)) return kInvalid;
    std::memset(t, 0, sizeof *t);
    uint16_t qt[2][64];
    quant_table(quality, qt[0]);
    chroma_quant_table(quality, qt[1]);
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 64; ++k) t->divisor[s][k] = (uint16_t)(qt[s][kNatural[k]] << 3);
    derive_codes(kDcBits, kDcVals, 12, t->dc[0], 12);
    derive_codes(kAcBits, kAcVals, 162, t->ac[0], 256);
    derive_codes(kDc1Bits, kDcVals, 12, t->dc[1], 12);
    derive_codes(kAc1Bits, kAc1Vals, 162, t->ac[1], 256);
    const uint8_t app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    uint8_t* p = put(t->header, app0, 20);
    for (int s = 0; s < 2; ++s) {
        const uint8_t dqt[5] = {0xff, 0xdb, 0, 67, (uint8_t)s};
        p = put(p, dqt, 5);
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)qt[s][kNatural[k]];
    }
    const uint8_t sof[19] = {0xff, 0xc0, 0, 17, 8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 3,
                             1, (uint8_t)((hs << 4) | vs), 0, 2, 0x11, 1, 3, 0x11, 1};
    p = put(p, sof, 19);
    p = put_dht(p, 0x00, kDcBits, kDcVals, 12);
    p = put_dht(p, 0x10, kAcBits, kAcVals, 162);
    p = put_dht(p, 0x01, kDc1Bits, kDcVals, 12);
    p = put_dht(p, 0x11, kAc1Bits, kAc1Vals, 162);
    const uint8_t sos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    p = put(p, sos, 14);
    t->header_bytes = kColourHeaderBytes;
    return (p - t->header) == kColourHeaderBytes ? kOk : kInvalid;
}

}  // namespace cvjpeg
