// pipeline.h -- launch wrappers and host-side table builders of pipeline.hip (the classical stages on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace cv {

hipError_t resize_area_u8(const uint8_t* src, int n, int h, int w, int c, uint8_t* dst, int oh, int ow, hipStream_t s);
void resize_area_table(int ssize, int dsize, std::vector<int>& ofs, std::vector<int>& si, std::vector<float>& alpha);
hipError_t resize_area_u8_tab(const uint8_t* src, int n, int h, int w, int c, uint8_t* dst, int oh, int ow, const int* xofs,
                              const int* xsi, const float* xa, const int* yofs, const int* ysi, const float* ya, hipStream_t s);
void resize_antialias_table(int ssize, int dsize, std::vector<int>& first, std::vector<int>& count, std::vector<float>& weights, int* stride);
hipError_t resize_antialias_f32(const uint8_t* src, int n, int h, int w, int c, float* dst, int oh, int ow, const int* xfirst,
                                const int* xcount, const float* xw, int xstride, const int* yfirst, const int* ycount, const float* yw,
                                int ystride, hipStream_t s);
hipError_t extract_squares_u8(const uint8_t* images, int n, int h, int w, const double* inv, uint8_t* squares,
                              uint8_t* boards, hipStream_t s);
hipError_t extract_squares_u8_one(const uint8_t* image, int h, int w, const double* inv_host, uint8_t* squares, uint8_t* board, hipStream_t s);

}  // namespace cv
