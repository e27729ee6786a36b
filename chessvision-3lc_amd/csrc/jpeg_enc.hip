// jpeg_enc.hip -- the JPEG encoder on the device, gray and colour, for gfx950: n images of one size in, n complete baseline files out,
// byte for byte what libjpeg writes with its defaults (the tables and the 328- / 623-byte headers come from jpeg.cpp:
// cvjpeg::encoder_tables, cvjpeg::colour_encoder_tables).
//
// Baseline encoding has no serial stage: a block's code depends on its own coefficients and the DC of the block before it, so code
// LENGTHS are a per-block function, bit offsets a prefix sum over them, and byte stuffing a second prefix sum over the packed bytes.
// One pass over a chunk of images is this fixed sequence of launches:
//
//   jpeg_fdct_quant_kernel   edge replication, level shift, jfdctint.c's "islow" forward DCT (rows then columns, int32), division with
//                            rounding by q << 3; int16 coefficients in zigzag order, [image][block_row][block_col][64]
//     or, for a colour image,
//   jpeg_colour_front_kernel jccolor.c's RGB -> YCbCr, jcsample.c's box reduction of chroma with libjpeg's padding, then the same
//                            DCT and quantiser per component; coefficients in CODED order, [image][mcu][block in mcu][64], the
//                            dummy luma blocks of partial MCUs written as such (the DC of the block before, no AC)
//   jpeg_block_bits_kernel   bits of each block's Huffman code (DC difference against the previous block OF ITS COMPONENT in coded
//                            order; the table set follows from the block's position in its MCU.  Gray: one block per MCU)
//   jpeg_bit_offsets_kernel  exclusive prefix sum per image (in place); payload bytes per image = bits rounded up to a byte
//   jpeg_zero_bits_kernel    zeroes the words of the bit buffer that the image will use
//   jpeg_pack_kernel         every block writes its bits at its offset, most significant bit first; the last block of an image
//                            fills the final byte with 1-bits
//   jpeg_count_ff_kernel     0xFF bytes per 1 KB tile of the packed payload
//   jpeg_frame_kernel        prefix sum of the tile counts per image (in place); file length = header + payload + stuffed + EOI
//   jpeg_offsets_kernel      where each file starts in the output (16-byte steps, running across passes)
//   jpeg_scatter_kernel      header, payload with FF 00 stuffing, FF D9
//
// Blocks that share a 32-bit word of the bit buffer combine with integer atomicOr on the zeroed word, so the buffer does not depend on
// arrival order and the output is a pure function of pixels and quality.  The gray scan stores the words a block fills alone plainly
// (only a block's first and last word can be shared), as it always has.  A colour scan ORs EVERY word in: with plain stores for
// whole words, 4:2:0 and 4:2:2 passes of more than 256 groups of blocks lost bits -- coefficients and bit offsets were right, and
// stretches of up to a cache line of the buffer held zeros where blocks had ORed their bits in, differently from run to run; with
// nothing but atomics between the buffer's zeroing and its reading every size is exact (profiles/jpeg_colour_encode.md has the
// measurements, and what of the mechanism is only supposed).  There is no float atomic anywhere.
//
// Bounds.  A block codes into at most cvjpeg::kEncMaxBlockBits = 20 + 63 * 26 bits (DC: 9-bit code + 11 bits; each AC: 16-bit code + 10
// bits: an 8-bit sample cannot give a larger category), a chroma block into cvjpeg::kEncMaxChromaBlockBits (its DC code has up to 11
// bits); the bit buffer holds that for every block, dummies included, and the caller's output holds header + twice that + EOI per
// image.  Every index below follows from the geometry or is compared with the buffer's size before it is used: the stores into the
// bit buffer and into the output are guarded by their capacities whatever the coefficients say.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "jpeg_enc_device.h"

namespace cv {

namespace {
namespace enc {

typedef uint32_t v2 __attribute__((ext_vector_type(2)));
typedef uint32_t v4 __attribute__((ext_vector_type(4)));

constexpr int kGroupBlocks = 32;           // 256 lanes, 8 per block
constexpr int kBlockWords = 72;            // a block in LDS: rows 9 words apart
constexpr unsigned kTileBytes = 1024;      // a stuffing tile: 256 lanes x one word
typedef cvjpeg::ScanTables Tables;

// NL: luma blocks of an MCU, 4 ("4:2:0"), 2 ("4:2:2") or 1 ("4:4:4"), followed by one Cb and one Cr block; 0: a gray scan, whose MCU
// is its one block.  The kernels that walk blocks are compiled once per NL, so the gray chain carries nothing of the colour one.
template <int NL>
struct Scan {
    static constexpr int kPer = NL ? NL + 2 : 1;                 // blocks of an MCU
    static constexpr int kSets = NL ? 2 : 1;                     // table sets the scan uses
};

struct Plan {
    int h, w, bw, bh;                      // bw, bh: the 8 x 8 blocks that hold real pixels of the (luma) plane
    int mw;                                // colour: MCUs in a row
    unsigned mcus;                         // colour: MCUs of one image
    unsigned blocks;                       // coded 8 x 8 blocks of one image (colour: dummies included)
    unsigned header;                       // bytes in front of the entropy-coded segment
    unsigned words;                        // words of one image's bit buffer (a multiple of 4)
    unsigned tiles;                        // stuffing tiles of one image
    unsigned cap;                          // bytes of one file at most (cvjpeg::gray_max_bytes / colour_max_bytes)
};

// where the pieces of the scratch block start (bytes; every piece 256-byte aligned)
struct Carve {
    size_t tables, total, nbytes, bitoff, tilecnt, coeffs, words, end;
};

__constant__ uint8_t kNaturalOf[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass of jfdctint.c's jpeg_fdct_islow, in place; the row pass (`first`) keeps 2 extra bits, the column pass removes them
__device__ __forceinline__ void fdct8(int32_t* d, bool first) {
    const int32_t tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int32_t tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int shift = first ? 11 : 15;
    d[0] = first ? (tmp10 + tmp11) << 2 : descale(tmp10 + tmp11, 2);
    d[4] = first ? (tmp10 - tmp11) << 2 : descale(tmp10 - tmp11, 2);
    int32_t z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270, shift);
    d[6] = descale(z1 - tmp12 * 15137, shift);
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d[7] = descale(t4 + z1 + z3, shift);
    d[5] = descale(t5 + z2 + z4, shift);
    d[3] = descale(t6 + z2 + z3, shift);
    d[1] = descale(t7 + z1 + z4, shift);
}

// zigzag positions 8j .. 8j + 7 of the block whose DCT output is in `mine`, divided with rounding, as eight int16 in four words
__device__ __forceinline__ v4 quantise8(const int32_t* mine, const uint16_t* __restrict__ divisor, int j) {
    const v4 dv = *reinterpret_cast<const v4*>(divisor + j * 8);
    v4 o = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int nat = kNaturalOf[j * 8 + k];
        const int32_t t = mine[(nat >> 3) * 9 + (nat & 7)];
        const uint32_t div = max((dv[k >> 1] >> ((k & 1) * 16)) & 0xffffu, 1u);
        const uint32_t mag = ((uint32_t)(t < 0 ? -t : t) + (div >> 1)) / div;
        const int32_t q = t < 0 ? -(int32_t)mag : (int32_t)mag;
        o[k >> 1] |= ((uint32_t)q & 0xffffu) << ((k & 1) * 16);
    }
    return o;
}

__global__ __launch_bounds__(256) void jpeg_enc_setup_kernel(Tables t, uint32_t* __restrict__ dst, unsigned long long* __restrict__ total) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&t);
    for (unsigned i = threadIdx.x; i < sizeof(Tables) / 4; i += 256) dst[i] = src[i];
    if (threadIdx.x == 0) *total = 0ull;
}

// A wave takes eight blocks, as the decoder's inverse DCT does: lane (block, j) loads row j of its block, runs the row pass and puts
// it into LDS; lane (block, c) runs the column pass on column c; lane (block, j) then quantises the zigzag positions 8j .. 8j + 7 and
// stores them with one 16-byte store.  `wide` (uniform): w is a multiple of 8 and src is 8-byte aligned, so a row is one 8-byte load.
__global__ __launch_bounds__(256) void jpeg_fdct_quant_kernel(const uint8_t* __restrict__ src, const Tables* __restrict__ tab,
                                                              int16_t* __restrict__ coeffs, Plan p, unsigned total_blocks, int wide) {
    __shared__ int32_t lds[kGroupBlocks * kBlockWords];
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const unsigned gb = blockIdx.x * kGroupBlocks + lb;
    const bool live = gb < total_blocks;                         // every lane reaches the barriers
    int32_t* mine = lds + lb * kBlockWords;
    int32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const unsigned img = gb / p.blocks, b = gb - img * p.blocks;
        const int by = (int)(b / (unsigned)p.bw), bx = (int)(b - (unsigned)by * (unsigned)p.bw);
        const int y = min(by * 8 + j, p.h - 1);                  // the last row and column are replicated into the padding
        const uint8_t* row = src + ((size_t)img * p.h + y) * (size_t)p.w;
        if (wide) {
            const v2 v = *reinterpret_cast<const v2*>(row + bx * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = (int32_t)((v[k >> 2] >> (8 * (k & 3))) & 255u) - 128;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = (int32_t)row[min(bx * 8 + k, p.w - 1)] - 128;
        }
    }
    fdct8(d, true);
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[j * 9 + k] = d[k];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = mine[r * 9 + j];          // column j: read and written back by this lane alone
    fdct8(d, false);
#pragma unroll
    for (int r = 0; r < 8; ++r) mine[r * 9 + j] = d[r];
    __syncthreads();
    if (!live) return;
    *reinterpret_cast<v4*>(coeffs + (size_t)gb * 64 + j * 8) = quantise8(mine, tab->divisor[0], j);
}

// The colour front end.  A group takes 32 / (HS * VS + 2) whole MCUs, eight lanes per block as above (the lanes left over idle but
// reach every barrier).  Lane (luma block (v, u), j) loads the 8 pixels of row j of its block -- three 8-byte loads where `wide`
// (uniform: w a multiple of 8 and src 8-byte aligned) and the block lies inside the row, else byte loads with the last pixel of the row
// replicated -- converts them (jccolor.c, 16 fractional bits), keeps Y for its own row pass and stages Cb and Cr in LDS, already
// summed over pixel pairs when HS = 2: `stage[mcu][Cb | Cr][row of the MCU][8]`, rows 9 words apart as the blocks are.  Behind a
// barrier lane (Cb | Cr block, j) finishes row j of its block from the stage (jcsample.c's h2v2 / h2v1 box: bias 1, 2, 1, 2 .. resp.
// 0, 1, 0, 1 ..).  libjpeg's padding is not symmetric, and all of it is index arithmetic here:
//   columns: the row's last pixel is replicated out to the MCU width BEFORE the reduction (x clamped to w - 1 in the load);
//   rows:    luma's last row is replicated (y clamped to h - 1 in the load); chroma's last INPUT row only completes a row group, then
//            the last REDUCED row is replicated: reduced row cy reads the staged rows 2 cy', 2 cy' + 1 with cy' = min(cy, ceil(h / 2) - 1)
//            (VS = 2), both of this MCU, and the clamp of the load has made row h of an odd height a copy of row h - 1.
// Dummy luma blocks (beyond the plane's own bw x bh blocks) stage their chroma like any other and are then written as what libjpeg
// codes for them: no AC, and the quantised DC of the nearest real block before them in the MCU (block 0 is always real).
template <int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_colour_front_kernel(const uint8_t* __restrict__ src, const Tables* __restrict__ tab,
                                                                int16_t* __restrict__ coeffs, Plan p, unsigned total_mcus, int wide, int r_at) {
    constexpr int NL = HS * VS, PER = NL + 2, MPG = kGroupBlocks / PER, SROWS = 8 * VS;
    __shared__ int32_t lds[kGroupBlocks * kBlockWords];
    __shared__ int32_t stage[MPG * 2 * SROWS * 9];
    __shared__ int32_t dcq[kGroupBlocks];
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int lm = lb / PER, k = lb - lm * PER;                  // MCU of the group, block of the MCU
    const unsigned gm = blockIdx.x * MPG + (unsigned)lm;
    const bool live = lm < MPG && gm < total_mcus;               // every lane reaches the barriers
    int32_t* mine = lds + lb * kBlockWords;
    int32_t* st = stage + (live ? lm : 0) * (2 * SROWS * 9);
    int32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned img = live ? gm / p.mcus : 0u, m = live ? gm - img * p.mcus : 0u;
    const int my = (int)(m / (unsigned)p.mw), mx = (int)(m - (unsigned)my * (unsigned)p.mw);
    const int v = k / HS, u = k - v * HS;                        // a luma block's place in the MCU
    const bool real = k >= NL || ((my * VS + v) < p.bh && (mx * HS + u) < p.bw);
    if (live && k < NL) {
        const int x0 = (mx * HS + u) * 8;
        const int y = min((my * VS + v) * 8 + j, p.h - 1);
        const uint8_t* row = src + ((size_t)img * p.h + y) * (size_t)p.w * 3;
        int32_t r[8], g[8], b[8];
        if (wide && x0 + 8 <= p.w) {
            const v2* q = reinterpret_cast<const v2*>(row + (size_t)x0 * 3);
            const v2 a0 = q[0], a1 = q[1], a2 = q[2];
            const uint32_t wd[6] = {a0[0], a0[1], a1[0], a1[1], a2[0], a2[1]};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int i0 = 3 * e, i1 = 3 * e + 1, i2 = 3 * e + 2;       // constants once unrolled: wd stays in registers
                const int32_t c0 = (int32_t)((wd[i0 >> 2] >> (8 * (i0 & 3))) & 255u);
                const int32_t c2 = (int32_t)((wd[i2 >> 2] >> (8 * (i2 & 3))) & 255u);
                r[e] = r_at ? c2 : c0;
                g[e] = (int32_t)((wd[i1 >> 2] >> (8 * (i1 & 3))) & 255u);
                b[e] = r_at ? c0 : c2;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint8_t* px = row + (size_t)min(x0 + e, p.w - 1) * 3;
                r[e] = px[r_at]; g[e] = px[1]; b[e] = px[2 - r_at];
            }
        }
        int32_t cb[8], cr[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            d[e] = ((19595 * r[e] + 38470 * g[e] + 7471 * b[e] + 32768) >> 16) - 128;
            cb[e] = (-11059 * r[e] - 21709 * g[e] + 32768 * b[e] + (128 << 16) + 32767) >> 16;
            cr[e] = (32768 * r[e] - 27439 * g[e] - 5329 * b[e] + (128 << 16) + 32767) >> 16;
        }
        int32_t* to = st + (v * 8 + j) * 9;
        if (HS == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                to[u * 4 + e] = cb[2 * e] + cb[2 * e + 1];
                to[SROWS * 9 + u * 4 + e] = cr[2 * e] + cr[2 * e + 1];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                to[e] = cb[e];
                to[SROWS * 9 + e] = cr[e];
            }
        }
    }
    __syncthreads();
    if (live && k >= NL) {
        const int32_t* from = st + (k - NL) * (SROWS * 9);
        if (VS == 2) {
            const int lr = min(my * 8 + j, ((p.h + 1) >> 1) - 1) - my * 8;       // 0 .. 7: this MCU starts inside the image
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = ((from[(2 * lr) * 9 + e] + from[(2 * lr + 1) * 9 + e] + 1 + (e & 1)) >> 2) - 128;
        } else if (HS == 2) {
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = ((from[j * 9 + e] + (e & 1)) >> 1) - 128;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = from[j * 9 + e] - 128;
        }
    }
    fdct8(d, true);
#pragma unroll
    for (int e = 0; e < 8; ++e) mine[j * 9 + e] = d[e];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = mine[r * 9 + j];
    fdct8(d, false);
#pragma unroll
    for (int r = 0; r < 8; ++r) mine[r * 9 + j] = d[r];
    __syncthreads();
    v4 o = {0, 0, 0, 0};
    if (live) o = quantise8(mine, tab->divisor[k >= NL ? 1 : 0], j);
    if (j == 0) dcq[lb] = (int32_t)(o[0] & 0xffffu);
    __syncthreads();
    if (!live) return;
    if (!real) {
        o = v4{0, 0, 0, 0};
        if (j == 0) {
            int kk = k - 1;                                      // k >= 1: block 0 of an MCU is real
            while (kk > 0 && !((my * VS + kk / HS) < p.bh && (mx * HS + kk % HS) < p.bw)) --kk;
            o[0] = (uint32_t)dcq[lb - k + kk];
        }
    }
    *reinterpret_cast<v4*>(coeffs + ((size_t)gm * PER + k) * 64 + j * 8) = o;
}

__device__ __forceinline__ int nbits(int32_t v) { return 32 - __clz(v < 0 ? -v : v); }     // __clz(0) = 32

// The Huffman code of one block, symbol by symbol, into `sink.put(value, bits)`.  `ac` and `dc` are the tables in LDS.
template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* __restrict__ c, int32_t prev_dc, const uint32_t* ac, const uint32_t* dc, Sink& sink) {
    int run = 0;
    const uint32_t zrl = ac[0xF0], eob = ac[0x00];
    for (int q = 0; q < 8; ++q) {
        const v4 v = *reinterpret_cast<const v4*>(c + q * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int32_t x = (int16_t)(v[e >> 1] >> ((e & 1) * 16));
            if (q == 0 && e == 0) {
                const int32_t diff = x - prev_dc;
                const int s = min(nbits(diff), 11);
                sink.put(dc[s] >> 8, (int)(dc[s] & 255u));
                sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
            } else if (x == 0) {
                ++run;
            } else {
                for (; run > 15; run -= 16) sink.put(zrl >> 8, (int)(zrl & 255u));
                const int s = min(nbits(x), 15);
                const uint32_t t = ac[((run << 4) | s) & 255];
                sink.put(t >> 8, (int)(t & 255u));
                sink.put((uint32_t)(x < 0 ? x - 1 : x) & ((1u << s) - 1u), s);
                run = 0;
            }
        }
    }
    if (run > 0) sink.put(eob >> 8, (int)(eob & 255u));
}

struct CountSink {
    uint32_t bits = 0;
    __device__ __forceinline__ void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// Bits go in most significant first: bit k of an image's stream is bit 31 - (k & 31) of word k >> 5.
// PLAIN (the gray scan, as it always was): a word the block fills alone is stored plainly, only its first and last word, which it may
// share, are ORed in.  Colour scans OR every word in (the file header says why).
template <bool PLAIN>
struct PackSink {
    uint32_t* words;                       // the image's bit buffer
    uint32_t wi, limit;                    // next word, words of the buffer
    uint64_t acc = 0;
    int cnt;                               // bits of acc not yet stored (the first `cnt` of the first word belong to earlier blocks)
    bool shared;                           // the next word is shared with the block before
    __device__ __forceinline__ void put(uint32_t v, int n) {
        acc = (acc << n) | v;
        cnt += n;
        if (cnt >= 32) {
            cnt -= 32;
            const uint32_t word = (uint32_t)(acc >> cnt);
            if (wi < limit) {
                if (!PLAIN || shared) atomicOr(words + wi, word); else words[wi] = word;
            }
            shared = false;
            ++wi;
            acc &= (1ull << cnt) - 1ull;
        }
    }
    __device__ __forceinline__ void flush() {                    // the last, partial word
        if (cnt > 0 && wi < limit) atomicOr(words + wi, (uint32_t)(acc << (32 - cnt)));
    }
};

template <int SETS>
__device__ __forceinline__ void load_tables(const Tables* __restrict__ tab, uint32_t* ac, uint32_t* dc) {
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
        ac[s * 256 + threadIdx.x] = tab->ac[s][threadIdx.x];     // 256 lanes
        if (threadIdx.x < 12) dc[s * 12 + threadIdx.x] = tab->dc[s][threadIdx.x];
    }
    __syncthreads();
}

// Where block b of an image (gb among all images' blocks) stands in its scan: its table set, and the DC it is predicted from -- that
// of the block coded before it IN ITS COMPONENT, 0 for a component's first block.  Luma blocks follow each other inside an MCU and
// from the last one of the MCU before; a chroma block follows its like one MCU back.  Gray: the block before, set 0.
template <int NL>
__device__ __forceinline__ int32_t predecessor_dc(const int16_t* __restrict__ coeffs, unsigned gb, unsigned b, int* set) {
    constexpr unsigned PER = Scan<NL>::kPer;
    if (NL == 0) {
        *set = 0;
        return b ? (int32_t)coeffs[(size_t)(gb - 1) * 64] : 0;
    }
    const unsigned k = b % PER;
    *set = k >= (unsigned)NL ? 1 : 0;
    if (k > 0 && k < (unsigned)NL) return (int32_t)coeffs[(size_t)(gb - 1) * 64];
    if (b < PER) return 0;                                       // the first MCU of the image
    return (int32_t)coeffs[(size_t)(k == 0 ? gb - PER + (unsigned)NL - 1u : gb - PER) * 64];
}

template <int NL>
__global__ __launch_bounds__(256) void jpeg_block_bits_kernel(const int16_t* __restrict__ coeffs, const Tables* __restrict__ tab,
                                                              uint32_t* __restrict__ bitoff, Plan p, unsigned total_blocks) {
    __shared__ uint32_t ac[Scan<NL>::kSets * 256], dc[Scan<NL>::kSets * 12];
    load_tables<Scan<NL>::kSets>(tab, ac, dc);
    const unsigned gb = blockIdx.x * 256 + threadIdx.x;
    if (gb >= total_blocks) return;
    int set;
    const int32_t prev = predecessor_dc<NL>(coeffs, gb, gb % p.blocks, &set);
    CountSink sink;
    code_block(coeffs + (size_t)gb * 64, prev, ac + set * 256, dc + set * 12, sink);
    bitoff[gb] = min(sink.bits, (uint32_t)(set ? cvjpeg::kEncMaxChromaBlockBits : cvjpeg::kEncMaxBlockBits));
}

// exclusive prefix sum of v over the 256 lanes of the group; *total = the sum.  lds: 256 elements.
template <class T>
__device__ __forceinline__ T group_scan(T v, T* lds, T* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const T add = t >= d ? lds[t - d] : T(0);
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const T incl = lds[t];
    *total = lds[255];
    __syncthreads();
    return incl - v;
}

// a[0 .. n) -> its exclusive prefix sums, in place, by one group of 256 lanes (lane t takes a contiguous run); returns the sum
__device__ __forceinline__ uint32_t scan_in_place(uint32_t* __restrict__ a, unsigned n, uint32_t* lds) {
    const unsigned per = (n + 255) / 256;
    const unsigned lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
    uint32_t sum = 0;
    for (unsigned i = lo; i < hi; ++i) sum += a[i];
    uint32_t total;
    uint32_t at = group_scan<uint32_t>(sum, lds, &total);
    for (unsigned i = lo; i < hi; ++i) {
        const uint32_t v = a[i];
        a[i] = at;
        at += v;
    }
    return total;
}

__global__ __launch_bounds__(256) void jpeg_bit_offsets_kernel(uint32_t* __restrict__ bitoff, uint32_t* __restrict__ nbytes, Plan p) {
    __shared__ uint32_t lds[256];
    const unsigned img = blockIdx.x;
    const uint32_t bits = scan_in_place(bitoff + (size_t)img * p.blocks, p.blocks, lds);
    if (threadIdx.x == 0) nbytes[img] = min((bits + 7u) >> 3, (p.words - 1u) * 4u);
}

__global__ __launch_bounds__(256) void jpeg_zero_bits_kernel(uint32_t* __restrict__ words, const uint32_t* __restrict__ nbytes, Plan p) {
    const unsigned img = blockIdx.y;
    const unsigned w0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (w0 >= p.words || w0 * 4 >= nbytes[img] + 4u) return;      // words is a multiple of 4: w0 + 3 < words
    *reinterpret_cast<v4*>(words + (size_t)img * p.words + w0) = v4{0, 0, 0, 0};
}

template <int NL>
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t* __restrict__ coeffs, const Tables* __restrict__ tab,
                                                        const uint32_t* __restrict__ bitoff, uint32_t* __restrict__ words, Plan p,
                                                        unsigned total_blocks) {
    __shared__ uint32_t ac[Scan<NL>::kSets * 256], dc[Scan<NL>::kSets * 12];
    load_tables<Scan<NL>::kSets>(tab, ac, dc);
    const unsigned gb = blockIdx.x * 256 + threadIdx.x;
    if (gb >= total_blocks) return;
    const unsigned img = gb / p.blocks, b = gb - img * p.blocks;
    int set;
    const int32_t prev = predecessor_dc<NL>(coeffs, gb, b, &set);
    const uint32_t off = bitoff[gb];
    PackSink<NL == 0> sink;
    sink.words = words + (size_t)img * p.words;
    sink.limit = p.words;
    sink.wi = off >> 5;
    sink.cnt = (int)(off & 31u);
    sink.shared = sink.cnt != 0;
    code_block(coeffs + (size_t)gb * 64, prev, ac + set * 256, dc + set * 12, sink);
    if (b == p.blocks - 1) {                                     // the image's last block: 1-bits up to the byte boundary
        const int pad = (8 - (sink.cnt & 7)) & 7;
        sink.put((1u << pad) - 1u, pad);
    }
    sink.flush();
}

// the bytes of word `wi` of an image that belong to its payload, and how many of them are 0xFF
__device__ __forceinline__ uint32_t payload_word(const uint32_t* __restrict__ words, unsigned wi, unsigned limit, uint32_t nb, int* valid, int* ff) {
    const uint32_t word = wi < limit ? words[wi] : 0u;
    const uint32_t first = wi * 4u;
    *valid = first >= nb ? 0 : (int)min(nb - first, 4u);
    int count = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) count += (q < *valid && ((word >> (24 - 8 * q)) & 255u) == 255u) ? 1 : 0;
    *ff = count;
    return word;
}

__global__ __launch_bounds__(256) void jpeg_count_ff_kernel(const uint32_t* __restrict__ words, const uint32_t* __restrict__ nbytes,
                                                            uint32_t* __restrict__ tilecnt, Plan p) {
    __shared__ uint32_t lds[256];
    const unsigned img = blockIdx.y, tile = blockIdx.x;
    const uint32_t nb = nbytes[img];
    if ((size_t)tile * kTileBytes >= nb) return;                 // uniform: the whole group leaves
    int valid, ff;
    payload_word(words + (size_t)img * p.words, tile * 256 + threadIdx.x, p.words, nb, &valid, &ff);
    uint32_t total;
    group_scan<uint32_t>((uint32_t)ff, lds, &total);
    if (threadIdx.x == 0) tilecnt[(size_t)img * p.tiles + tile] = total;
}

__global__ __launch_bounds__(256) void jpeg_frame_kernel(uint32_t* __restrict__ tilecnt, const uint32_t* __restrict__ nbytes,
                                                         int32_t* __restrict__ lengths, Plan p) {
    __shared__ uint32_t lds[256];
    const unsigned img = blockIdx.x;
    const uint32_t nb = nbytes[img];
    const unsigned used = min((nb + kTileBytes - 1) / kTileBytes, p.tiles);
    const uint32_t ff = scan_in_place(tilecnt + (size_t)img * p.tiles, used, lds);
    if (threadIdx.x == 0) lengths[img] = (int32_t)min(p.header + nb + ff + 2u, p.cap);
}

// files start on 16-byte steps, in input order; `total` carries the end of the previous pass and leaves with the end of this one,
// which is also written behind the last offset (offsets has one element more than there are images)
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int32_t* __restrict__ lengths, int64_t* __restrict__ offsets,
                                                           unsigned long long* __restrict__ total, int count) {
    __shared__ unsigned long long lds[256];
    const int per = (count + 255) / 256;
    const int lo = min((int)threadIdx.x * per, count), hi = min(lo + per, count);
    const unsigned long long base = *total;
    unsigned long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += ((unsigned long long)lengths[i] + 15ull) & ~15ull;
    unsigned long long all;
    unsigned long long at = base + group_scan<unsigned long long>(sum, lds, &all);     // its barriers order every read of *total before the write
    for (int i = lo; i < hi; ++i) {
        offsets[i] = (int64_t)at;
        at += ((unsigned long long)lengths[i] + 15ull) & ~15ull;
    }
    if (threadIdx.x == 0) {
        offsets[count] = (int64_t)(base + all);
        *total = base + all;
    }
}

__global__ __launch_bounds__(256) void jpeg_scatter_kernel(const uint32_t* __restrict__ words, const uint32_t* __restrict__ nbytes,
                                                           const uint32_t* __restrict__ tilecnt, const Tables* __restrict__ tab,
                                                           const int32_t* __restrict__ lengths, const int64_t* __restrict__ offsets,
                                                           uint8_t* __restrict__ out, Plan p) {
    __shared__ uint32_t lds[256];
    const unsigned img = blockIdx.y, tile = blockIdx.x;
    const uint32_t nb = nbytes[img];
    if ((size_t)tile * kTileBytes >= nb) return;                 // uniform
    const unsigned wi = tile * 256 + threadIdx.x;
    int valid, ff;
    const uint32_t word = payload_word(words + (size_t)img * p.words, wi, p.words, nb, &valid, &ff);
    uint32_t total;
    const uint32_t before = group_scan<uint32_t>((uint32_t)ff, lds, &total) + tilecnt[(size_t)img * p.tiles + tile];
    uint8_t* dst = out + offsets[img];
    uint32_t pos = p.header + wi * 4u + before;
    for (int q = 0; q < valid; ++q) {
        const uint32_t byte = (word >> (24 - 8 * q)) & 255u;
        if (pos < p.cap) dst[pos] = (uint8_t)byte;
        ++pos;
        if (byte == 255u) {
            if (pos < p.cap) dst[pos] = 0;
            ++pos;
        }
    }
    if (tile == 0) {
        for (unsigned i = threadIdx.x; i < p.header; i += 256) dst[i] = tab->header[i];      // header <= cap, and <= sizeof tab->header
        if (threadIdx.x == 0) {
            const uint32_t len = (uint32_t)lengths[img];         // >= header + 1 + 2, <= cap (jpeg_frame_kernel)
            dst[len - 2] = 0xFF;
            dst[len - 1] = 0xD9;
        }
    }
}

// hs = 0: a gray image; else the luma sampling factors of a colour one
Plan plan_of(int h, int w, int hs, int vs) {
    Plan p;
    p.h = h; p.w = w; p.bw = (w + 7) / 8; p.bh = (h + 7) / 8;
    size_t bits;
    if (hs == 0) {
        p.mw = p.bw;
        p.mcus = p.blocks = (unsigned)p.bw * (unsigned)p.bh;
        p.header = cvjpeg::kGrayHeaderBytes;
        bits = (size_t)p.blocks * cvjpeg::kEncMaxBlockBits;
        p.cap = (unsigned)cvjpeg::gray_max_bytes(w, h);
    } else {
        p.mw = (w + 8 * hs - 1) / (8 * hs);
        p.blocks = (unsigned)cvjpeg::colour_coded_blocks(w, h, hs, vs);            // <= 3 * 512 * 512
        p.mcus = p.blocks / (unsigned)(hs * vs + 2);
        p.header = cvjpeg::kColourHeaderBytes;
        bits = cvjpeg::colour_max_bits(w, h, hs, vs);                              // < 2^31
        p.cap = (unsigned)cvjpeg::colour_max_bytes(w, h, hs, vs);
    }
    p.words = (unsigned)((((bits + 31) / 32 + 1) + 3) & ~(size_t)3);
    p.tiles = (unsigned)(((size_t)p.words * 4 + kTileBytes - 1) / kTileBytes);
    return p;
}

int chunk_of(int n, const Plan& p) {
    const int by_blocks = (int)std::max(1u, (unsigned)kJpegEncChunkBlocks / p.blocks);
    return std::min(n, std::min((int)kJpegEncChunkImages, by_blocks));
}

Carve carve_of(const Plan& p, int chunk) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    Carve c;
    c.tables = 0;
    c.total = up(sizeof(Tables));
    c.nbytes = c.total + 256;
    c.bitoff = c.nbytes + up((size_t)kJpegEncChunkImages * 4);
    c.tilecnt = c.bitoff + up((size_t)chunk * p.blocks * 4);
    c.coeffs = c.tilecnt + up((size_t)chunk * p.tiles * 4);
    c.words = c.coeffs + up((size_t)chunk * p.blocks * 128);
    c.end = c.words + up((size_t)chunk * p.words * 4);
    return c;
}

bool size_ok(int n, int h, int w) { return n >= 1 && h >= 1 && w >= 1 && h <= kJpegEncMaxSide && w <= kJpegEncMaxSide; }

// One scan layout's passes over the scratch: `front(src of the pass, coefficients, tables on the device, images of the pass)` launches
// the kernel that turns pixels into coded-order coefficients, everything behind it is the same chain.  pixel_bytes: one image of src.
template <int NL, class Front>
hipError_t encode_scan(const uint8_t* src, size_t pixel_bytes, int n, const Plan& p, const Tables& tables, void* scratch, uint8_t* out,
                       int64_t* offsets, int32_t* lengths, hipStream_t s, Front front) {
    const int chunk = chunk_of(n, p);
    const Carve c = carve_of(p, chunk);
    char* base = (char*)scratch;
    Tables* d_tab = (Tables*)(base + c.tables);
    unsigned long long* d_total = (unsigned long long*)(base + c.total);
    uint32_t* d_nbytes = (uint32_t*)(base + c.nbytes);
    uint32_t* d_bitoff = (uint32_t*)(base + c.bitoff);
    uint32_t* d_tilecnt = (uint32_t*)(base + c.tilecnt);
    int16_t* d_coeffs = (int16_t*)(base + c.coeffs);
    uint32_t* d_words = (uint32_t*)(base + c.words);
    hipLaunchKernelGGL(jpeg_enc_setup_kernel, dim3(1), dim3(256), 0, s, tables, (uint32_t*)d_tab, d_total);
    hipError_t e = hipGetLastError();
    for (int c0 = 0; c0 < n && e == hipSuccess; c0 += chunk) {
        const int m = std::min(chunk, n - c0);
        const unsigned total_blocks = (unsigned)m * p.blocks;                      // <= kJpegEncChunkBlocks, or one image's
        const dim3 by_block((total_blocks + 255) / 256), by_image((unsigned)m);
        const dim3 by_tile(p.tiles, (unsigned)m), by_quad((p.words / 4 + 255) / 256, (unsigned)m);
        front(src + (size_t)c0 * pixel_bytes, d_coeffs, d_tab, m);
        hipLaunchKernelGGL(jpeg_block_bits_kernel<NL>, by_block, dim3(256), 0, s, d_coeffs, d_tab, d_bitoff, p, total_blocks);
        hipLaunchKernelGGL(jpeg_bit_offsets_kernel, by_image, dim3(256), 0, s, d_bitoff, d_nbytes, p);
        hipLaunchKernelGGL(jpeg_zero_bits_kernel, by_quad, dim3(256), 0, s, d_words, d_nbytes, p);
        hipLaunchKernelGGL(jpeg_pack_kernel<NL>, by_block, dim3(256), 0, s, d_coeffs, d_tab, d_bitoff, d_words, p, total_blocks);
        hipLaunchKernelGGL(jpeg_count_ff_kernel, by_tile, dim3(256), 0, s, d_words, d_nbytes, d_tilecnt, p);
        hipLaunchKernelGGL(jpeg_frame_kernel, by_image, dim3(256), 0, s, d_tilecnt, d_nbytes, lengths + c0, p);
        hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, s, lengths + c0, offsets + c0, d_total, m);
        hipLaunchKernelGGL(jpeg_scatter_kernel, by_tile, dim3(256), 0, s, d_words, d_nbytes, d_tilecnt, d_tab, lengths + c0, offsets + c0, out, p);
        e = hipGetLastError();
    }
    return e;
}

template <int HS, int VS>
hipError_t encode_colour(const uint8_t* src, int n, const Plan& p, int r_at, const Tables& tables, void* scratch, uint8_t* out,
                         int64_t* offsets, int32_t* lengths, hipStream_t s) {
    constexpr int kGroupMcus = kGroupBlocks / (HS * VS + 2);
    return encode_scan<HS * VS>(src, (size_t)p.h * p.w * 3, n, p, tables, scratch, out, offsets, lengths, s,
                                [&](const uint8_t* src_c, int16_t* d_coeffs, const Tables* d_tab, int m) {
                                    const unsigned total_mcus = (unsigned)m * p.mcus;
                                    const int wide = (p.w % 8 == 0) && ((uintptr_t)src_c % 8 == 0);
                                    hipLaunchKernelGGL((jpeg_colour_front_kernel<HS, VS>), dim3((total_mcus + kGroupMcus - 1) / kGroupMcus),
                                                       dim3(256), 0, s, src_c, d_tab, d_coeffs, p, total_mcus, wide, r_at);
                                });
}

}  // namespace enc
}  // namespace

int jpeg_encode_chunk(int n, int h, int w) {
    if (!enc::size_ok(n, h, w)) return 0;
    return enc::chunk_of(n, enc::plan_of(h, w, 0, 0));
}

size_t jpeg_encode_scratch_bytes(int n, int h, int w) {
    if (!enc::size_ok(n, h, w)) return 0;
    const enc::Plan p = enc::plan_of(h, w, 0, 0);
    return enc::carve_of(p, enc::chunk_of(n, p)).end;
}

size_t jpeg_encode_colour_scratch_bytes(int n, int h, int w, int hs, int vs) {
    if (!enc::size_ok(n, h, w) || !cvjpeg::subsampling_ok(hs, vs)) return 0;
    const enc::Plan p = enc::plan_of(h, w, hs, vs);
    return enc::carve_of(p, enc::chunk_of(n, p)).end;
}

hipError_t jpeg_encode_gray_u8(const uint8_t* src, int n, int h, int w, const cvjpeg::EncTables& tables, void* scratch, uint8_t* out,
                               int64_t* offsets, int32_t* lengths, hipStream_t s) {
    using namespace enc;
    if (!size_ok(n, h, w) || !src || !scratch || !out || !offsets || !lengths || ((uintptr_t)scratch & 255u)) return hipErrorInvalidValue;
    const Plan p = plan_of(h, w, 0, 0);
    Tables scan;
    cvjpeg::scan_tables_of(tables, &scan);
    return encode_scan<0>(src, (size_t)h * w, n, p, scan, scratch, out, offsets, lengths, s,
                          [&](const uint8_t* src_c, int16_t* d_coeffs, const Tables* d_tab, int m) {
                              const unsigned total_blocks = (unsigned)m * p.blocks;
                              const int wide = (w % 8 == 0) && ((uintptr_t)src_c % 8 == 0);
                              hipLaunchKernelGGL(jpeg_fdct_quant_kernel, dim3((total_blocks + kGroupBlocks - 1) / kGroupBlocks), dim3(256), 0, s,
                                                 src_c, d_tab, d_coeffs, p, total_blocks, wide);
                          });
}

hipError_t jpeg_encode_colour_u8(const uint8_t* src, int n, int h, int w, int r_at, int hs, int vs, const cvjpeg::ScanTables& tables,
                                 void* scratch, uint8_t* out, int64_t* offsets, int32_t* lengths, hipStream_t s) {
    using namespace enc;
    if (!size_ok(n, h, w) || !cvjpeg::subsampling_ok(hs, vs) || (r_at != 0 && r_at != 2) || tables.header_bytes != cvjpeg::kColourHeaderBytes ||
        !src || !scratch || !out || !offsets || !lengths || ((uintptr_t)scratch & 255u))
        return hipErrorInvalidValue;
    const Plan p = plan_of(h, w, hs, vs);
    if (vs == 2) return encode_colour<2, 2>(src, n, p, r_at, tables, scratch, out, offsets, lengths, s);
    if (hs == 2) return encode_colour<2, 1>(src, n, p, r_at, tables, scratch, out, offsets, lengths, s);
    return encode_colour<1, 1>(src, n, p, r_at, tables, scratch, out, offsets, lengths, s);
}

}  // namespace cv
