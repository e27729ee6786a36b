// host_stages.h -- the host-side classical stages (contour.cpp, position.cpp, homography.cpp) as their callers see them.
// Plain C++ with no HIP types: the three units are also compiled on their own, without the engine (tests/c_abi/host_sanitize.cpp).
#pragma once
#include <cstdint>

#include "../../include/chessvision_hip.h"      // plain C: the two score records

namespace cv {

// contour.cpp
bool find_quadrangle(const uint8_t* mask, int h, int w, int32_t quad[8]);
long find_contours_flat(const uint8_t* mask, int h, int w, bool tc89, int32_t* xy, long cap_pts, int32_t* counts, int32_t* holes,
                        long cap_contours);
double mask_completeness(const uint8_t* mask, int h, int w);
double quadrangle_regularity(const float quad[8]);

// position.cpp
void decode_positions(const float* probs, int n_boards, int flip, char* fen, char* original_fen, int8_t* labels,
                      int32_t* fixes, int32_t* n_fixes);
const char* fen_labels(const char* fen, int8_t* labels);
void classification_scores(const float* probs, const int8_t* labels, int n_boards, cv_square_score_t* per_square,
                           cv_board_score_t* per_board);

// homography.cpp
void board_homographies(const float* quads, int n, int out_w, int out_h, double* forward, double* inverse);

}  // namespace cv
