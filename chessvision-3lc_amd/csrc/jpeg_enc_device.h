// jpeg_enc_device.h -- launch wrapper of jpeg_enc.hip (the gray JPEG encoder; its host half is in jpeg.cpp / jpeg.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg.h"

namespace cv {

enum { kJpegEncMaxSide = 4096,             // h, w of an image: 1..4096
       kJpegEncChunkBlocks = 262144,       // 8 x 8 blocks one pass works on at most: those of ONE 4096 x 4096 image, the least any bound must admit
       kJpegEncChunkImages = 1024 };       // ... and images: the per-image bookkeeping of a pass stays a few KB and a grid's y extent small

// images of one pass over (n, h, w): min(n, kJpegEncChunkImages, max(1, kJpegEncChunkBlocks / blocks per image))
int jpeg_encode_chunk(int n, int h, int w);
// bytes of scratch the encoder needs for ANY number of images of this size (one pass's worth, sized by the worst case of
// cvjpeg::kEncMaxBlockBits bits per block): at most ~90 MB, whatever n
size_t jpeg_encode_scratch_bytes(int n, int h, int w);

// n gray images (n, h, w) uint8 on the device -> n complete baseline JPEG files in `out`: file i is the `lengths[i]` bytes at
// `out + offsets[i]`; offsets are multiples of 16 in input order and offsets[n] is the end of the last file, rounded up.  `out` holds at
// least n * cvjpeg::gray_max_bytes(w, h) bytes (no file is longer, so nothing can be written past it), offsets n + 1 int64, lengths n
// int32, scratch jpeg_encode_scratch_bytes(n, h, w) bytes aligned to 256.  Launches on `s`, one fixed sequence per pass of
// jpeg_encode_chunk(n, h, w) images over the same scratch; allocates nothing, synchronises nothing.
hipError_t jpeg_encode_gray_u8(const uint8_t* src, int n, int h, int w, const cvjpeg::EncTables& tables, void* scratch, uint8_t* out,
                               int64_t* offsets, int32_t* lengths, hipStream_t s);

// The colour encoder: n images (n, h, w, 3) uint8, R at byte `r_at` of a pixel (0: RGB, 2: BGR), luma sampled hs x vs (2x2, 2x1, 1x1) ->
// n three-component files, libjpeg's byte for byte.  The same contract with cvjpeg::colour_max_bytes(w, h, hs, vs) per image in `out`
// and jpeg_encode_colour_scratch_bytes of scratch; `tables` from cvjpeg::colour_encoder_tables.  A pass takes
// min(n, kJpegEncChunkImages, max(1, kJpegEncChunkBlocks / coded blocks per image)) images, the dummy blocks of partial MCUs counted.
size_t jpeg_encode_colour_scratch_bytes(int n, int h, int w, int hs, int vs);
hipError_t jpeg_encode_colour_u8(const uint8_t* src, int n, int h, int w, int r_at, int hs, int vs, const cvjpeg::ScanTables& tables,
                                 void* scratch, uint8_t* out, int64_t* offsets, int32_t* lengths, hipStream_t s);

}  // namespace cv
