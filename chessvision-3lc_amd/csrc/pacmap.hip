// pacmap.hip -- PaCMAP on the device: scaled-distance neighbour choice, mid-near and further draws, the Adam optimiser; and the
// placement of new rows into a fitted map: their pairs into the basis and all Adam steps of every new point in one launch.
// The contract is in pacmap.h and include/chessvision_hip.h (cv_pacmap_pairs, cv_pacmap_optimise, cv_pacmap_basis_scale,
// cv_pacmap_place_pairs, cv_pacmap_place); the definition all are held to is chessvision/embeddings.py.  Every float operation that the definition rounds is rounded here: contraction is off in each
// function that computes, division and square root are the correctly rounded defaults (no fast-math in the Makefile).  This file is
// part of cv_api.cpp's translation unit.
#include <math.h>

#include "neighbours.h"
#include "pacmap.h"

namespace cv {
namespace {

constexpr int kPmBlock = 64;                // one lane per point: a wave per workgroup spreads few points over many compute units
constexpr int kPmBatch = 4;                 // incidence entries of a point whose loads are issued together

__device__ __forceinline__ bool pm_less(double d0, int j0, double d1, int j1) { return d0 < d1 || (d0 == d1 && j0 < j1); }

// ---- the counter-based generator (embeddings.pacmap_mix / pacmap_key / pacmap_draw) --------------------------------------------------
__host__ __device__ __forceinline__ uint64_t pm_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t pm_key(uint64_t seed, uint64_t stream, int i) { return pm_mix(seed ^ pm_mix((stream << 40) | (uint64_t)i)); }
__device__ __forceinline__ int pm_draw(uint64_t key, uint64_t t, int n) { return (int)(((pm_mix(key + t) >> 32) * (uint64_t)n) >> 32); }

// D of neighbours.h: double, ascending channel, product and sum each rounded
__device__ __forceinline__ double pm_exact_d(const float* __restrict__ a, const float* __restrict__ b, int c) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int ch = 0; ch < c; ++ch) {
        const double t = (double)a[ch] - (double)b[ch];
        const double p = t * t;
        s = s + p;
    }
    return s;
}

// ---- neighbour pairs -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPmBlock) void pm_sigma_kernel(const double* __restrict__ cand_d, int n, int kc, double* __restrict__ sigma,
                                                            PacmapStats* __restrict__ stats) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kPmBlock + threadIdx.x;
    if (i == 0) stats->candidates = kc;
    if (i >= n) return;
    const double* d = cand_d + (size_t)i * kc;
    double s;
    if (kc > 3) {
        const int hi = kc < 6 ? kc : 6;
        s = sqrt(d[3]);
        for (int r = 4; r < hi; ++r) s = s + sqrt(d[r]);
        s = s / (double)(hi - 3);
    } else {
        s = sqrt(d[kc - 1]);
    }
    sigma[i] = s > 1e-10 ? s : 1e-10;
}

// One wave per row, lane t holds candidate t (kc <= 64): its rank among the row's candidates by (scaled, j) is its output slot.
// sigma_row has `rows` entries, sigma_col n: the same array for a table against itself, the new rows' and the basis' for a placement.
__global__ __launch_bounds__(256) void pm_choose_kernel(const int32_t* __restrict__ cand_i, const double* __restrict__ cand_d,
                                                        const double* __restrict__ sigma_row, const double* __restrict__ sigma_col, int rows,
                                                        int n, int kc, int nn, int32_t* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    int j = 0x7fffffff;
    double sc = (double)__builtin_huge_valf();
    if (lane < kc) {
        const int cj = cand_i[(size_t)row * kc + lane];
        if (cj >= 0 && cj < n) {                             // finite tables have at least kc eligible rows: always
            j = cj;
            const double scale = sigma_row[row] * sigma_col[cj];
            sc = cand_d[(size_t)row * kc + lane] / scale;
        }
    }
    int rank = 0;
    for (int u = 0; u < kc; ++u) rank += pm_less(__shfl(sc, u), __shfl(j, u), sc, j) ? 1 : 0;
    if (lane < kc && rank < nn) out[(size_t)row * nn + rank] = j == 0x7fffffff ? -1 : j;
}

// ---- mid-near pairs: one lane per point, its slots in turn ----------------------------------------------------------------------------
__global__ __launch_bounds__(kPmBlock) void pm_mid_near_kernel(const float* __restrict__ pre, int n, int c, int nmn, uint64_t seed,
                                                               int32_t* __restrict__ out, PacmapStats* __restrict__ stats) {
    const int i = blockIdx.x * kPmBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = pm_key(seed, 1, i);
    int32_t* mine = out + (size_t)i * nmn;
    const float* a = pre + (size_t)i * c;
    uint64_t t = 0;
    bool overflow = false;
    for (int slot = 0; slot < nmn && !overflow; ++slot) {
        int held[kPacmapMidNearDraws] = {-1, -1, -1, -1, -1, -1};
        int count = 0;
        while (count < kPacmapMidNearDraws) {
            if (t >= (uint64_t)kPacmapMaxDraws) { overflow = true; break; }
            const int j = pm_draw(key, t++, n);
            bool ok = j != i;
#pragma unroll
            for (int u = 0; u < kPacmapMidNearDraws; ++u) ok = ok && !(u < count && held[u] == j);
            for (int u = 0; u < slot; ++u) ok = ok && mine[u] != j;
            if (ok) {
#pragma unroll
                for (int u = 0; u < kPacmapMidNearDraws; ++u)
                    if (u == count) held[u] = j;
                ++count;
            }
        }
        if (overflow) {
            for (int u = slot; u < nmn; ++u) mine[u] = -1;
            break;
        }
        double d[kPacmapMidNearDraws];
#pragma unroll
        for (int u = 0; u < kPacmapMidNearDraws; ++u) d[u] = pm_exact_d(a, pre + (size_t)held[u] * c, c);
        int partner = -1;
#pragma unroll
        for (int u = 0; u < kPacmapMidNearDraws; ++u) {      // the six (D, j) are distinct in j: exactly one has one entry below it
            int below = 0;
#pragma unroll
            for (int w = 0; w < kPacmapMidNearDraws; ++w) below += pm_less(d[w], held[w], d[u], held[u]) ? 1 : 0;
            if (below == 1) partner = held[u];
        }
        mine[slot] = partner;
    }
    atomicAdd(reinterpret_cast<unsigned long long*>(&stats->mid_near_draws), (unsigned long long)t);
    if (overflow) stats->draw_overflow = 1;                   // every writer stores the same value
}

// ---- further pairs: one lane per point; the row under construction is the rejection set ------------------------------------------------
__global__ __launch_bounds__(kPmBlock) void pm_further_kernel(const int32_t* __restrict__ nbr, int n, int nn, int nfp, uint64_t seed,
                                                              int32_t* __restrict__ out, PacmapStats* __restrict__ stats) {
    const int i = blockIdx.x * kPmBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = pm_key(seed, 2, i);
    int32_t* mine = out + (size_t)i * nfp;
    const int32_t* near = nbr + (size_t)i * nn;
    uint64_t t = 0;
    int count = 0;
    bool overflow = false;
    while (count < nfp) {
        if (t >= (uint64_t)kPacmapMaxDraws) { overflow = true; break; }
        const int j = pm_draw(key, t++, n);
        bool ok = j != i;
        for (int u = 0; u < nn; ++u) ok = ok && near[u] != j;
        for (int u = 0; u < count; ++u) ok = ok && mine[u] != j;
        if (ok) mine[count++] = j;
    }
    for (int u = count; u < nfp; ++u) mine[u] = -1;
    atomicAdd(reinterpret_cast<unsigned long long*>(&stats->further_draws), (unsigned long long)t);
    if (overflow) stats->draw_overflow = 1;
}

// ---- one iteration: gather over the incidence list, then Adam -------------------------------------------------------------------------
__global__ __launch_bounds__(kPmBlock) void pm_step_kernel(const float2* __restrict__ yin, float2* __restrict__ yout, float2* __restrict__ m,
                                                           float2* __restrict__ v, const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ entries, int n, float lr, float w_n, float w_mn, float w_fp,
                                                           int with_mid_near) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * kPmBlock + threadIdx.x;
    if (p >= n) return;
    const float2 yp = yin[p];
    float g0 = 0.f, g1 = 0.f;
    const int e1 = offsets[p + 1];
    // kPmBatch entries at a time: their loads, then their gathers, are in flight together; the sums stay in list order
    for (int e = offsets[p]; e < e1; e += kPmBatch) {
        int x[kPmBatch], kinds[kPmBatch];
        bool live[kPmBatch];
        float2 yq[kPmBatch];
#pragma unroll
        for (int u = 0; u < kPmBatch; ++u) x[u] = e + u < e1 ? entries[e + u] : -1;
#pragma unroll
        for (int u = 0; u < kPmBatch; ++u) {
            const int q = x[u] & ((1 << kPacmapKindShift) - 1);
            kinds[u] = x[u] >> kPacmapKindShift;
            live[u] = x[u] >= 0 && q < n && kinds[u] <= 2 && !(kinds[u] == 1 && !with_mid_near);
            yq[u] = yp;
            if (live[u]) yq[u] = yin[q];
        }
#pragma unroll
        for (int u = 0; u < kPmBatch; ++u) {
            if (!live[u]) continue;
            const int kind = kinds[u];
            const float add = kind == 0 ? 10.f : kind == 1 ? 10000.f : 1.f;
            const float num = kind == 0 ? 20.f : kind == 1 ? 20000.f : 2.f;
            const float wk = kind == 0 ? w_n : kind == 1 ? w_mn : w_fp;
            const float d0 = yp.x - yq[u].x, d1 = yp.y - yq[u].y;
            float d = 1.f;
            d = d + d0 * d0;
            d = d + d1 * d1;
            const float t = add + d;
            const float w = wk * (num / (t * t));
            const float s0 = w * d0, s1 = w * d1;
            g0 = kind == 2 ? g0 - s0 : g0 + s0;              // further pairs push apart
            g1 = kind == 2 ? g1 - s1 : g1 + s1;
        }
    }
    const float c1 = (float)(1.0 - 0.9), c2 = (float)(1.0 - 0.999), eps = 1e-7f;
    float2 mp = m[p], vp = v[p];
    mp.x = mp.x + c1 * (g0 - mp.x);
    mp.y = mp.y + c1 * (g1 - mp.y);
    vp.x = vp.x + c2 * (g0 * g0 - vp.x);
    vp.y = vp.y + c2 * (g1 * g1 - vp.y);
    m[p] = mp;
    v[p] = vp;
    float2 y;
    y.x = yp.x - (lr * mp.x) / (sqrtf(vp.x) + eps);
    y.y = yp.y - (lr * mp.y) / (sqrtf(vp.y) + eps);
    yout[p] = y;
}

// ---- placement: every Adam step of a new point in one launch ---------------------------------------------------------------------------
// One lane per new point.  Its partners' coordinates never move: they are read once into LDS as [slot][lane] float2 (8-byte reads of
// consecutive lanes: conflict-free; a private array indexed by the slot would live in scratch memory) and walked `iterations` times
// with m and v in registers.  The schedule is pacmap_schedule_row, evaluated by every lane in double.
__global__ __launch_bounds__(kPmBlock) void pm_place_kernel(const float2* __restrict__ init, int q, const float2* __restrict__ basis, int n,
                                                            const int32_t* __restrict__ pairs, int nn, int iterations,
                                                            float2* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float2 partner[kPacmapMaxNeighbours][kPmBlock];
    const int lane = threadIdx.x, p = blockIdx.x * kPmBlock + lane;
    if (p >= q) return;                                       // no barrier below: a lane reads only the LDS column it wrote
    uint32_t live = 0;
    for (int u = 0; u < nn; ++u) {
        const int b = pairs[(size_t)p * nn + u];
        const bool ok = b >= 0 && b < n;
        if (ok) live |= 1u << u;
        partner[u][lane] = ok ? basis[b] : make_float2(0.f, 0.f);
    }
    float2 y = init[p];
    float m0 = 0.f, m1 = 0.f, v0 = 0.f, v1 = 0.f;
    const float c1 = (float)(1.0 - 0.9), c2 = (float)(1.0 - 0.999), eps = 1e-7f;
    double b1 = 1.0, b2 = 1.0;
    for (int it = 0; it < iterations; ++it) {
        float row[4];
        pacmap_schedule_row(it, b1, b2, row);
        const float lr = row[0], w_n = row[1];
        float g0 = 0.f, g1 = 0.f;
        for (int u = 0; u < nn; ++u) {
            const float2 yb = partner[u][lane];
            const float e0 = y.x - yb.x, e1 = y.y - yb.y;
            float d = 1.f;
            d = d + e0 * e0;
            d = d + e1 * e1;
            const float t = 10.f + d;
            const float w = w_n * (20.f / (t * t));
            const float s0 = w * e0, s1 = w * e1;
            if ((live >> u) & 1u) {
                g0 = g0 + s0;
                g1 = g1 + s1;
            }
        }
        m0 = m0 + c1 * (g0 - m0);
        m1 = m1 + c1 * (g1 - m1);
        v0 = v0 + c2 * (g0 * g0 - v0);
        v1 = v1 + c2 * (g1 * g1 - v1);
        y.x = y.x - (lr * m0) / (sqrtf(v0) + eps);
        y.y = y.y - (lr * m1) / (sqrtf(v1) + eps);
    }
    out[p] = y;
}

inline size_t pm_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

bool pacmap_in_limits(int n, int c, int n_neighbors, int n_mn, int n_fp) {
    if (n_neighbors < 1 || n_neighbors > kPacmapMaxNeighbours || n_mn < 0 || n_mn > kPacmapMaxMidNear || n_fp < 0 || n_fp > kPacmapMaxFurther)
        return false;
    if (c < 1 || c > kNeighbourMaxC || n > kNeighbourMaxRows) return false;
    if (n < 7 || n < kPacmapMidNearDraws + n_mn || n < n_neighbors + n_fp + 1) return false;
    return 2ll * n * (n_neighbors + n_mn + n_fp) < (1ll << 31);
}

PacmapPlan pacmap_plan(int n, int c, int n_neighbors, int n_mn, int n_fp) {
    PacmapPlan p{};
    p.n = n; p.c = c; p.n_neighbors = n_neighbors; p.n_mn = n_mn; p.n_fp = n_fp;
    p.kc = std::min(std::min(n_neighbors + kPacmapExtraCandidates, kNeighbourMaxK), n - 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += pm_up(bytes); return at; };
    p.off_stats = take(sizeof(PacmapStats));
    p.off_cand_i = take((size_t)n * p.kc * sizeof(int32_t));
    p.off_cand_d = take((size_t)n * p.kc * sizeof(double));
    p.off_sigma = take((size_t)n * sizeof(double));
    p.off_search = take(neighbour_plan(n, n, c, p.kc).bytes);
    p.pairs_bytes = o;
    o = 0;
    p.off_m = take((size_t)n * sizeof(float2));
    p.off_v = take((size_t)n * sizeof(float2));
    p.off_y0 = take((size_t)n * sizeof(float2));
    p.off_y1 = take((size_t)n * sizeof(float2));
    p.optimise_bytes = o;
    return p;
}

hipError_t pacmap_pairs(const float* pre, int n, int c, int n_neighbors, int n_mn, int n_fp, uint64_t seed, int32_t* neighbours,
                        int32_t* mid_near, int32_t* further, PacmapStats* stats, void* scratch, hipStream_t s) {
    if (!pre || !neighbours || (!mid_near && n_mn) || (!further && n_fp) || !scratch || ((uintptr_t)scratch & 15u) ||
        !pacmap_in_limits(n, c, n_neighbors, n_mn, n_fp))
        return hipErrorInvalidValue;
    const PacmapPlan p = pacmap_plan(n, c, n_neighbors, n_mn, n_fp);
    char* base = static_cast<char*>(scratch);
    PacmapStats* st = stats ? stats : reinterpret_cast<PacmapStats*>(base + p.off_stats);
    int32_t* cand_i = reinterpret_cast<int32_t*>(base + p.off_cand_i);
    double* cand_d = reinterpret_cast<double*>(base + p.off_cand_d);
    double* sigma = reinterpret_cast<double*>(base + p.off_sigma);
    hipError_t e;
    if ((e = hipMemsetAsync(st, 0, sizeof(PacmapStats), s)) != hipSuccess) return e;
    if ((e = embedding_neighbours(pre, n, pre, n, c, p.kc, kNeighbourExcludeSelf, cand_i, cand_d, &st->neighbours, base + p.off_search, s)) !=
        hipSuccess)
        return e;
    const dim3 lanes((n + kPmBlock - 1) / kPmBlock), block(kPmBlock);
    hipLaunchKernelGGL(pm_sigma_kernel, lanes, block, 0, s, cand_d, n, p.kc, sigma, st);
    hipLaunchKernelGGL(pm_choose_kernel, dim3((n + 3) / 4), dim3(256), 0, s, cand_i, cand_d, sigma, sigma, n, n, p.kc, n_neighbors, neighbours);
    if (n_mn) hipLaunchKernelGGL(pm_mid_near_kernel, lanes, block, 0, s, pre, n, c, n_mn, seed, mid_near, st);
    if (n_fp) hipLaunchKernelGGL(pm_further_kernel, lanes, block, 0, s, neighbours, n, n_neighbors, n_fp, seed, further, st);
    return hipGetLastError();
}

hipError_t pacmap_basis_scale(const float* pre, int n, int c, int n_neighbors, double* sigma, void* scratch, hipStream_t s) {
    if (!pre || !sigma || !scratch || ((uintptr_t)scratch & 15u) || !pacmap_in_limits(n, c, n_neighbors, 0, 0)) return hipErrorInvalidValue;
    const PacmapPlan p = pacmap_plan(n, c, n_neighbors, 0, 0);
    char* base = static_cast<char*>(scratch);
    PacmapStats* st = reinterpret_cast<PacmapStats*>(base + p.off_stats);
    int32_t* cand_i = reinterpret_cast<int32_t*>(base + p.off_cand_i);
    double* cand_d = reinterpret_cast<double*>(base + p.off_cand_d);
    hipError_t e;
    if ((e = embedding_neighbours(pre, n, pre, n, c, p.kc, kNeighbourExcludeSelf, cand_i, cand_d, &st->neighbours, base + p.off_search, s)) !=
        hipSuccess)
        return e;
    hipLaunchKernelGGL(pm_sigma_kernel, dim3((n + kPmBlock - 1) / kPmBlock), dim3(kPmBlock), 0, s, cand_d, n, p.kc, sigma, st);
    return hipGetLastError();
}

bool pacmap_place_in_limits(int q, int n, int c, int n_neighbors) {
    return q >= 1 && q <= kNeighbourMaxRows && pacmap_in_limits(n, c, n_neighbors, 0, 0);
}

PacmapPlacePlan pacmap_place_plan(int q, int n, int c, int n_neighbors) {
    PacmapPlacePlan p{};
    p.q = q; p.n = n; p.c = c; p.n_neighbors = n_neighbors;
    p.kc = std::min(std::min(n_neighbors + kPacmapExtraCandidates, kNeighbourMaxK), n);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += pm_up(bytes); return at; };
    p.off_stats = take(sizeof(PacmapStats));
    p.off_cand_i = take((size_t)q * p.kc * sizeof(int32_t));
    p.off_cand_d = take((size_t)q * p.kc * sizeof(double));
    p.off_sigma = take((size_t)q * sizeof(double));
    p.off_search = take(neighbour_plan(q, n, c, p.kc).bytes);
    p.pairs_bytes = o;
    p.scale_bytes = pacmap_plan(n, c, n_neighbors, 0, 0).pairs_bytes;
    return p;
}

hipError_t pacmap_place_pairs(const float* pre_new, int q, const float* pre, int n, int c, int n_neighbors, const double* sigma,
                              int32_t* neighbours, NeighbourStats* stats, void* scratch, hipStream_t s) {
    if (!pre_new || !pre || !sigma || !neighbours || !scratch || ((uintptr_t)scratch & 15u) || !pacmap_place_in_limits(q, n, c, n_neighbors))
        return hipErrorInvalidValue;
    const PacmapPlacePlan p = pacmap_place_plan(q, n, c, n_neighbors);
    char* base = static_cast<char*>(scratch);
    PacmapStats* st = reinterpret_cast<PacmapStats*>(base + p.off_stats);
    int32_t* cand_i = reinterpret_cast<int32_t*>(base + p.off_cand_i);
    double* cand_d = reinterpret_cast<double*>(base + p.off_cand_d);
    double* sigma_q = reinterpret_cast<double*>(base + p.off_sigma);
    hipError_t e;
    if ((e = embedding_neighbours(pre_new, q, pre, n, c, p.kc, 0, cand_i, cand_d, stats ? stats : &st->neighbours, base + p.off_search, s)) !=
        hipSuccess)
        return e;
    hipLaunchKernelGGL(pm_sigma_kernel, dim3((q + kPmBlock - 1) / kPmBlock), dim3(kPmBlock), 0, s, cand_d, q, p.kc, sigma_q, st);
    hipLaunchKernelGGL(pm_choose_kernel, dim3((q + 3) / 4), dim3(256), 0, s, cand_i, cand_d, sigma_q, sigma, q, n, p.kc, n_neighbors, neighbours);
    return hipGetLastError();
}

hipError_t pacmap_place(const float* init, int q, const float* basis, int n, const int32_t* neighbours, int n_neighbors, int iterations,
                        float* out, hipStream_t s) {
    if (!init || !basis || !neighbours || !out || out == init || ((uintptr_t)init & 7u) || ((uintptr_t)basis & 7u) || ((uintptr_t)out & 7u) ||
        q < 1 || q > kNeighbourMaxRows || n < 1 || n > kNeighbourMaxRows || n_neighbors < 1 || n_neighbors > kPacmapMaxNeighbours ||
        iterations < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pm_place_kernel, dim3((q + kPmBlock - 1) / kPmBlock), dim3(kPmBlock), 0, s, reinterpret_cast<const float2*>(init), q,
                       reinterpret_cast<const float2*>(basis), n, neighbours, n_neighbors, iterations, reinterpret_cast<float2*>(out));
    return hipGetLastError();
}

__host__ __device__ void pacmap_schedule_row(int it, double& b1, double& b2, float out[4]) {
#pragma clang fp contract(off)
    b1 = b1 * 0.9;
    b2 = b2 * 0.999;
    double w_n, w_mn;
    if (it < 100) {
        const double a = 1.0 - (double)it / 100.0, b = (double)it / 100.0;
        const double lo = a * 1000.0, hi = b * 3.0;
        w_n = 2.0;
        w_mn = lo + hi;
    } else if (it < kPacmapMidNearFrom) {
        w_n = 3.0;
        w_mn = 3.0;
    } else {
        w_n = 1.0;
        w_mn = 0.0;
    }
    out[0] = (float)(sqrt(1.0 - b2) / (1.0 - b1));
    out[1] = (float)w_n;
    out[2] = (float)w_mn;
    out[3] = 1.f;
}

hipError_t pacmap_optimise(const float* init, int n, const int32_t* offsets, const int32_t* entries, int iterations, float* out,
                           void* scratch, hipStream_t s) {
    if (!init || !offsets || !entries || !out || out == init || !scratch || ((uintptr_t)scratch & 15u) || ((uintptr_t)init & 7u) ||
        ((uintptr_t)out & 7u) || n < 7 || n > kNeighbourMaxRows || iterations < 0)
        return hipErrorInvalidValue;
    const PacmapPlan p = pacmap_plan(n, 1, 1, 0, 0);
    char* base = static_cast<char*>(scratch);
    float2* m = reinterpret_cast<float2*>(base + p.off_m);
    float2* v = reinterpret_cast<float2*>(base + p.off_v);
    float2* buf[2] = {reinterpret_cast<float2*>(base + p.off_y0), reinterpret_cast<float2*>(base + p.off_y1)};
    hipError_t e;
    if (iterations == 0) return hipMemcpyAsync(out, init, (size_t)n * sizeof(float2), hipMemcpyDeviceToDevice, s);
    if ((e = hipMemsetAsync(m, 0, (size_t)n * sizeof(float2), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(v, 0, (size_t)n * sizeof(float2), s)) != hipSuccess) return e;
    const float2* src = reinterpret_cast<const float2*>(init);
    double b1 = 1.0, b2 = 1.0;
    const dim3 lanes((n + kPmBlock - 1) / kPmBlock), block(kPmBlock);
    for (int it = 0; it < iterations; ++it) {
        float row[4];
        pacmap_schedule_row(it, b1, b2, row);
        float2* dst = it == iterations - 1 ? reinterpret_cast<float2*>(out) : buf[it & 1];
        hipLaunchKernelGGL(pm_step_kernel, lanes, block, 0, s, src, dst, m, v, offsets, entries, n, row[0], row[1], row[2], row[3],
                           it < kPacmapMidNearFrom ? 1 : 0);
        src = dst;
    }
    return hipGetLastError();
}

}  // namespace cv
