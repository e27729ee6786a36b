// neighbours.h -- host interface of the exact k-nearest-neighbour search over embedding tables (neighbours.hip).
//
// D(a, b) = sum over ascending c of ((double)a[c] - (double)b[c])^2, product and sum each rounded to double, no contraction.  The
// result of query row i is the k eligible corpus rows with the smallest (D, j), ascending.  Three stages, all launched on one stream:
//   filter   float32 GEMM form on centred rows (exact-f32 MFMA), the KP = k + kNeighbourSlack smallest approximate distances per row
//            and T = the smallest approximate distance not kept; the corpus is split over workgroups, every split keeps its own list;
//   refine   merges the split lists, computes D for the KP candidates, sorts by (D, j), writes the first k and CERTIFIES the row when
//            D_k < T - E (E bounds |approximate - D| over the whole corpus, DESIGN.md section 4 "Embedding neighbours");
//   exact    one workgroup per query row: leaves at once when the row is certified, otherwise D against the whole corpus.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace cv {

constexpr int kNeighbourMaxK = 64;
constexpr int kNeighbourMaxC = 4096;
constexpr int kNeighbourMaxRows = 1 << 22;
// Candidates kept beyond k.  The filter's k-th and the true k-th neighbour differ by at most the rounding error E, so a handful of
// extra candidates covers the re-ordering; what the slack really buys is a T (the first distance NOT kept) that lies well above D_k,
// which is what certification needs.  16 certified every row of the iid, offset and clustered tables in the host emulation
// (tests/test_neighbours_cpu.py) and keeps a row's list at 80 entries = 640 bytes of LDS at k = 64.
constexpr int kNeighbourSlack = 16;
constexpr int kNeighbourTile = 64;          // query rows and corpus rows of one MFMA tile
constexpr int kNeighbourKStep = 32;         // channels per LDS stage; centred rows are zero-padded to a multiple of it
constexpr int kNeighbourMaxSplits = 1024;   // corpus splits per query tile
constexpr int kNeighbourTargetBlocks = 512;   // two workgroups of the filter fit a compute unit: one full round on 256 of them
constexpr int kNeighbourMeanChunks = 1024;  // row chunks of the channel-sum kernel

enum { kNeighbourExcludeSelf = 1, kNeighbourExactOnly = 2 };

struct NeighbourStats {                     // == cv_neighbour_stats_t
    int32_t query_rows, certified_rows, exact_rows, nonfinite_query_rows, nonfinite_corpus_rows, reserved[3];
};

struct NeighbourPlan {
    int q, n, c, k;
    int cp;                                 // channels padded to kNeighbourKStep
    int kp;                                 // candidates per row, k + kNeighbourSlack
    int qpad, npad;                         // rows padded to kNeighbourTile
    int qtiles, ntiles;
    int tiles_per_split, splits;            // corpus tiles of one workgroup, workgroups per query tile
    int mean_chunks, mean_rows;             // row chunks of the channel sums, rows per chunk
    // byte offsets into the scratch block, each a multiple of 256
    size_t off_stats, off_nbmax, off_rowbad, off_state, off_qflag, off_bflag, off_cnt, off_partial, off_mean, off_na, off_nb, off_a, off_b,
        off_pd, off_pi, off_pt, bytes;
};

// The launch plan and scratch layout of one call.  Arguments must be inside the limits above.
NeighbourPlan neighbour_plan(int q, int n, int c, int k);

// All pointers DEVICE; queries (q, c) and corpus (n, c) dense float32, 4-byte aligned; indices (q, k) int32; sq_distances (q, k) double,
// 8-byte aligned; stats nullable, 4-byte aligned; scratch 16-byte aligned with at least neighbour_plan(...).bytes bytes.  Launches
// and hipMemsetAsync only: nothing is allocated, nothing synchronises.
hipError_t embedding_neighbours(const float* queries, int q, const float* corpus, int n, int c, int k, int flags, int32_t* indices,
                                double* sq_distances, NeighbourStats* stats, void* scratch, hipStream_t s);

}  // namespace cv
