// jpeg_device.h -- launch wrapper of jpeg.hip (the device half of the JPEG decoder).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg.h"

namespace cv {

enum { kJpegBGR = 0, kJpegRGB = 1, kJpegGray = 2 };

// bytes of component planes that n images of this geometry need between the two launches (one byte per coefficient)
size_t jpeg_planes_bytes(const cvjpeg::Info& info, int n);

// n images of ONE geometry: coeffs = n x (layout_of(info).blocks * 64) int16, qtables = n x components x 64 uint16, both 16-byte
// aligned; planes = jpeg_planes_bytes(info, n) bytes, 8-byte aligned; dst = (n, h, w, 3) uint8, or (n, h, w) for kJpegGray.
// Two launches on `s`; allocates nothing, synchronises nothing.
hipError_t jpeg_reconstruct_u8(const int16_t* coeffs, const uint16_t* qtables, int n, const cvjpeg::Info& info, int order, uint8_t* planes,
                               uint8_t* dst, hipStream_t s);

// The same with the EXIF orientation tag applied in the colour stage's store: orientation 0 (absent) and 1 are jpeg_reconstruct_u8
// itself, 2..8 give dst = (n, h', w', 3 | 1) with (h', w') = (w, h) for the transposing tags 5..8; anything else is
// hipErrorInvalidValue.  Still two launches over the same planes.
hipError_t jpeg_reconstruct_oriented_u8(const int16_t* coeffs, const uint16_t* qtables, int n, const cvjpeg::Info& info, int order,
                                        int orientation, uint8_t* planes, uint8_t* dst, hipStream_t s);

}  // namespace cv
