// pacmap.h -- host interface of the PaCMAP reduction of embedding tables (pacmap.hip): the three pair sets and the optimiser, and
// (last part) the placement of new rows into a fitted map.
//
// The definition is chessvision/embeddings.py (pacmap_pairs, pacmap_incidence, pacmap_schedule, pacmap_optimise), a reading of Wang,
// Huang, Rudin, Shaposhnik (JMLR 2021) and of the pacmap package's defaults; DESIGN.md section 4 "Embedding reduction".  Both device
// entries equal it exactly: the pairs index for index, the coordinates bit for bit.
//   pairs     embedding_neighbours (neighbours.hip, unchanged) for the kc exact candidates of every row, then
//             sigma     one lane per row: max(mean of sqrt(D) at candidate ranks 3, 4, 5, 1e-10) in double;
//             choose    one wave per row: the n_neighbors candidates with the smallest (D_ij / (sigma_i sigma_j), j);
//             mid-near  one lane per row, slots in turn: six distinct draws, D by the neighbour search's definition, second smallest;
//             further   one lane per row: n_FP distinct draws outside the row's neighbours.
//   optimise  one launch per iteration, one lane per point walking its incidence list in order (float32, no contraction), then Adam.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "neighbours.h"

namespace cv {

constexpr int kPacmapMaxNeighbours = 32;
constexpr int kPacmapMaxMidNear = 16;
constexpr int kPacmapMaxFurther = 64;
constexpr int kPacmapMidNearDraws = 6;      // candidates of one mid-near slot
constexpr int kPacmapExtraCandidates = 50;  // kc = min(n_neighbors + 50, kNeighbourMaxK, n - 1)
constexpr int kPacmapMaxDraws = 1 << 16;    // draws of one point in one stream before it gives up (sets draw_overflow)
constexpr int kPacmapKindShift = 28;        // an incidence entry: other point | kind << 28 (0 neighbour, 1 mid-near, 2 further)
constexpr int kPacmapMidNearFrom = 200;     // from this iteration on w_MN = 0 and the mid-near entries are skipped
static_assert(kNeighbourMaxRows <= (1 << kPacmapKindShift), "a point index fits under the kind bits");

struct PacmapStats {                        // == cv_pacmap_stats_t
    NeighbourStats neighbours;
    int64_t mid_near_draws, further_draws;  // draws of all points, rejected ones included
    int32_t draw_overflow;                  // 1 when a point reached kPacmapMaxDraws (its remaining partners are -1)
    int32_t candidates;                     // kc
    int32_t reserved[2];
};

struct PacmapPlan {
    int n, c, n_neighbors, n_mn, n_fp, kc;
    // byte offsets into the pairs scratch, each a multiple of 256
    size_t off_stats, off_cand_i, off_cand_d, off_sigma, off_search, pairs_bytes;
    // and into the optimiser's
    size_t off_m, off_v, off_y0, off_y1, optimise_bytes;
};

// n in [max(7, 6 + n_mn, n_neighbors + n_fp + 1), kNeighbourMaxRows], c in [1, kNeighbourMaxC], n_neighbors in [1, 32], n_mn in
// [0, 16], n_fp in [0, 64], and 2 n (n_neighbors + n_mn + n_fp) below 2^31 (the incidence lists' int32 offsets).
bool pacmap_in_limits(int n, int c, int n_neighbors, int n_mn, int n_fp);
// The scratch layout of both entries.  Arguments must be inside the limits.
PacmapPlan pacmap_plan(int n, int c, int n_neighbors, int n_mn, int n_fp);

// All pointers DEVICE.  pre (n, c) dense float32, every value finite; neighbours (n, n_neighbors), mid_near (n, n_mn), further
// (n, n_fp) int32 (a set of zero columns may be null); stats nullable, 8-byte aligned; scratch 16-byte aligned with at least
// pacmap_plan(...).pairs_bytes bytes.  Launches and hipMemsetAsync only: nothing is allocated, nothing synchronises.
hipError_t pacmap_pairs(const float* pre, int n, int c, int n_neighbors, int n_mn, int n_fp, uint64_t seed, int32_t* neighbours,
                        int32_t* mid_near, int32_t* further, PacmapStats* stats, void* scratch, hipStream_t s);

// init and out (n, 2) float32, 8-byte aligned, out != init; offsets (n + 1) int32 and entries (offsets[n]) int32: the incidence lists in
// the order of embeddings.pacmap_incidence WITH the mid-near entries (an entry whose point is outside [0, n) is skipped); scratch 16-byte
// aligned with at least pacmap_plan(...).optimise_bytes bytes.  One launch per iteration on s, the schedule computed on the host in
// double; nothing is allocated, nothing synchronises.
hipError_t pacmap_optimise(const float* init, int n, const int32_t* offsets, const int32_t* entries, int iterations, float* out,
                           void* scratch, hipStream_t s);

// Row `it` of embeddings.pacmap_schedule: lr_t, w_n, w_MN, w_FP.  Double multiply, square root and divide round correctly on both
// sides, so the host's optimiser loop and the placement kernel get the same bits from it.
__host__ __device__ void pacmap_schedule_row(int it, double& b1, double& b2, float out[4]);

// ---- placing new rows into a fitted map (embeddings.pacmap_place_pairs, pacmap_place; a reading of the package's transform) -----------
//   basis scale  the fit's candidate search and sigma kernel again, sigma written to the caller's (n,) array: what the map keeps;
//   place pairs  embedding_neighbours of the q new rows against the basis (kc = min(n_neighbors + 50, 64, n), no row excluded), the
//                sigma kernel over the q candidate rows, the choose kernel with sigma_q from those and sigma_j from the basis array;
//   place        ONE launch: one lane per new point, its partners' coordinates staged in LDS, every Adam step in registers.
struct PacmapPlacePlan {
    int q, n, c, n_neighbors, kc;
    size_t off_stats, off_cand_i, off_cand_d, off_sigma, off_search, pairs_bytes;   // the place-pairs scratch, offsets multiples of 256
    size_t scale_bytes;                                                             // the basis-scale scratch: pacmap_plan's pairs block
};

// q in [1, kNeighbourMaxRows]; n, c and n_neighbors as pacmap_in_limits(n, c, n_neighbors, 0, 0) has them.
bool pacmap_place_in_limits(int q, int n, int c, int n_neighbors);
PacmapPlacePlan pacmap_place_plan(int q, int n, int c, int n_neighbors);

// All pointers DEVICE; launches and hipMemsetAsync only on s, nothing is allocated, nothing synchronises.
// sigma (n,) double <- the scale of every row of pre (n, c) in pacmap_pairs' neighbour choice; scratch 16-byte aligned, scale_bytes.
hipError_t pacmap_basis_scale(const float* pre, int n, int c, int n_neighbors, double* sigma, void* scratch, hipStream_t s);
// neighbours (q, n_neighbors) int32 <- the partners in the basis pre (n, c) of the new rows pre_new (q, c), all values finite; sigma
// (n,) double as pacmap_basis_scale wrote it; stats nullable; scratch 16-byte aligned, pairs_bytes.
hipError_t pacmap_place_pairs(const float* pre_new, int q, const float* pre, int n, int c, int n_neighbors, const double* sigma,
                              int32_t* neighbours, NeighbourStats* stats, void* scratch, hipStream_t s);
// out (q, 2) <- init (q, 2) after `iterations` steps towards basis (n, 2) over neighbours (q, n_neighbors) (a partner outside [0, n)
// is skipped); float32, 8-byte aligned, out != init.  No scratch.  iterations == 0 copies init.
hipError_t pacmap_place(const float* init, int q, const float* basis, int n, const int32_t* neighbours, int n_neighbors, int iterations,
                        float* out, hipStream_t s);

}  // namespace cv
