// jpeg.h -- the host half of the JPEG decoder: marker parser and Huffman stage (jpeg.cpp).  Plain C++17, no HIP header: g++ alone
// compiles it.  The device half (dequantise + inverse DCT, up-sampling, colour) is jpeg.hip / jpeg_device.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cvjpeg {

enum { kOk = 0, kInvalid = 1 };            // kInvalid == CV_ERR_INVALID (asserted in cv_api.cpp)

// What the header of a stream says.  Mirrors cv_jpeg_info_t field for field (asserted in cv_api.cpp).
struct Info {
    int32_t width, height;
    int32_t components;                    // 1 or 3
    int32_t luma_h, luma_v;                // luma sampling factors: 1x1, 2x1 or 2x2 (1x1 for a 1-component stream)
    int32_t restart_interval;              // MCUs between restart markers, 0 = none
    int32_t orientation;                   // EXIF tag 0x0112 (1..8) as found, 0 = absent.  Reported; the oriented entries (cv_api.cpp) apply it.
    int32_t supported;                     // 0: `reason` says why not
    char reason[160];
};

// Geometry that follows from a supported Info: one plane of 8x8 blocks per component, padded to whole MCUs.
struct Layout {
    int ncomp;
    int blocks_w[3], blocks_h[3];          // blocks per row / rows of blocks of each component plane
    size_t block_off[3];                   // first block of each plane in the image's coefficient buffer
    size_t blocks;                         // blocks of one image; the buffer holds blocks * 64 int16
};
Layout layout_of(const Info& info);

// Parse the markers up to the first scan.  Always fills *info (supported = 0 and a reason naming the byte offset when the stream is
// refused, truncated or corrupt).  Returns kInvalid only for null arguments.
int parse_info(const uint8_t* data, size_t len, Info* info);

// The whole entropy stage of one image: quantised coefficients, de-zigzagged to natural order, [component][block_row][block_col][64]
// int16, and the quantisation tables uint16[component][64] in natural order.  `capacity` counts int16 elements of `coeffs`.
// kInvalid with a message in err (reason and byte offset) for every refused, truncated or corrupt stream; nothing partial is promised
// in coeffs then.  Reads nothing outside [data, data + len), writes nothing outside the two output arrays.
int entropy_decode(const uint8_t* data, size_t len, int16_t* coeffs, size_t capacity, uint16_t* qtables, Info* info_out, char* err,
                   size_t err_len);

// ---- the host half of the gray ENCODER (jpeg_enc.hip holds the kernels) ------------------------------------------------------------
// What libjpeg writes for a one-component image with its defaults: baseline, the Annex K luminance table scaled by
// jpeg_set_quality(quality, force_baseline = TRUE), the Annex K DC0 / AC0 Huffman tables, a JFIF 1.1 header.
enum { kGrayHeaderBytes = 328, kEncMaxBlockBits = 20 + 63 * 26 };

// everything the kernels read besides the pixels; handed to them by value, so nothing is uploaded or cached
struct EncTables {
    uint16_t divisor[64];                  // quantiser steps << 3 in ZIGZAG order (the forward DCT leaves its output scaled by 8)
    uint32_t dc[12];                       // (code << 8) | length of each DC category
    uint32_t ac[256];                      // (code << 8) | length of each (run << 4 | size) symbol, 0 where Annex K has none
    uint8_t header[kGrayHeaderBytes];      // SOI, APP0 (JFIF 1.1, no units, density 1 x 1), DQT, SOF0, DHT DC0, DHT AC0, SOS
};

int clamp_quality(int quality);                            // libjpeg's: below 1 is 1, above 100 is 100
void quant_table(int quality, uint16_t out[64]);           // natural order, every entry 1..255
// width, height 1..65535.  Fills every field of *t; returns kInvalid for a null pointer or a size outside that range.
int encoder_tables(int width, int height, int quality, EncTables* t);
// bytes a file of that size can reach at most: header, every block at kEncMaxBlockBits with every byte stuffed, EOI; a multiple of 16
size_t gray_max_bytes(int width, int height);

// ---- ... and of the COLOUR encoder ------------------------------------------------------------------------------------------------
// What libjpeg writes for an RGB image with its defaults: three components (YCbCr), luma sampled hs x vs = 2x2 ("4:2:0"), 2x1
// ("4:2:2") or 1x1 ("4:4:4") against chroma's 1x1, one interleaved scan; luma with table set 0 (the gray encoder's), chroma with set 1:
// the Annex K.2 chrominance quantiser scaled like the luminance one, the Annex K.3.3.2 / K.3.3.4 DC1 / AC1 Huffman tables.
// A chroma DC code is up to 11 bits long (luma: 9), so a chroma block reaches 22 + 63 * 26 bits.
enum { kColourHeaderBytes = 623, kEncMaxChromaBlockBits = 22 + 63 * 26 };

// What the kernels of a scan read besides the pixels, gray or colour: two table sets (a gray scan uses set 0 alone) and the header
// with its length.  About 3 KB: handed to the set-up kernel by value, under the 4 KB a kernel's arguments may take.
struct ScanTables {
    uint16_t divisor[2][64];               // quantiser steps << 3 in ZIGZAG order, luma / chroma
    uint32_t dc[2][12];                    // (code << 8) | length of each DC category
    uint32_t ac[2][256];                   // (code << 8) | length of each (run << 4 | size) symbol, 0 where Annex K has none
    uint8_t header[kColourHeaderBytes + 1];// gray: EncTables::header; colour: SOI, APP0, DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, SOS
    uint32_t header_bytes;                 // kGrayHeaderBytes or kColourHeaderBytes
};

bool subsampling_ok(int hs, int vs);                       // 2x2, 2x1 or 1x1
void chroma_quant_table(int quality, uint16_t out[64]);    // natural order, every entry 1..255
void scan_tables_of(const EncTables& gray, ScanTables* t); // a gray scan: set 0 and the 328-byte header, everything else 0
// width, height 1..65535, (hs, vs) as above.  Fills every byte of *t; returns kInvalid for a null pointer or an argument outside that.
int colour_encoder_tables(int width, int height, int quality, int hs, int vs, ScanTables* t);
// blocks of one image in coded order, the dummy luma blocks of partial MCUs included: MCUs x (hs * vs + 2)
size_t colour_coded_blocks(int width, int height, int hs, int vs);
// bits the scan of one image can reach at most: every luma block (dummies too) at kEncMaxBlockBits, every chroma block at
// kEncMaxChromaBlockBits
size_t colour_max_bits(int width, int height, int hs, int vs);
// bytes a file can reach at most: header, colour_max_bits with every byte stuffed, EOI; a multiple of 16
size_t colour_max_bytes(int width, int height, int hs, int vs);

}  // namespace cvjpeg
