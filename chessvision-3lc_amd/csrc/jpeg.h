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
    int32_t orientation;                   // EXIF tag 0x0112 (1..8) as found, 0 = absent.  Reported, never applied.
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

}  // namespace cvjpeg
