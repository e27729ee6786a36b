// neighbours.hip -- exact k-nearest neighbours over embedding tables: prepare, MFMA filter, refine + certify, exact path.
// The contract is in neighbours.h and include/chessvision_hip.h (cv_embedding_neighbours); the bound E and the certify-or-recompute
// argument are derived in DESIGN.md section 4 "Embedding neighbours".  This file is part of cv_api.cpp's translation unit.
#include <algorithm>

#include "cv_kernels.h"
#include "neighbours.h"

namespace cv {
namespace {

constexpr int kNbTile = kNeighbourTile;
constexpr int kNbLdk = kNeighbourKStep + 4;              // LDS row stride of a staged K slice: 144 bytes, 16-byte aligned, off the 128-byte period
constexpr int kNbKpMax = kNeighbourMaxK + kNeighbourSlack;
constexpr int kNbEmpty = 0x7fffffff;                     // index of an unfilled list entry (its distance is +inf)
static_assert(kNbKpMax <= 128, "a wave holds a list in two entries per lane");
static_assert(kNeighbourKStep == 32 && kNbTile == 64, "the filter's load and fragment maps are written for these");

template <class T> __device__ __forceinline__ bool nb_less(T d0, int j0, T d1, int j1) { return d0 < d1 || (d0 == d1 && j0 < j1); }
template <class T> __device__ __forceinline__ T nb_inf() { return (T)__builtin_huge_valf(); }
__device__ __forceinline__ bool nb_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float nb_wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

// One wave offers up to 64 candidates, one per lane, to a list of `cap` <= 128 entries in LDS that is sorted ascending by (distance,
// index); unfilled entries hold (+inf, kNbEmpty) and sort last.  Candidates are taken in lane order; one that does not beat the
// current last entry is dropped, one that does is inserted at its place and the last entry falls out.  `tmin` collects, per lane, the
// smallest distance this lane saw dropped or pushed out: the minimum over the wave is the smallest distance NOT in the list.
template <class T>
__device__ __forceinline__ void nb_offer(T* ld, int* li, int cap, T d, int j, bool valid, T& tmin, int lane) {
    T wd = ld[cap - 1];
    int wi = li[cap - 1];
    const bool pass = valid && nb_less(d, j, wd, wi);
    if (valid && !pass) tmin = d < tmin ? d : tmin;
    unsigned long long m = __ballot(pass);
    if (!m) return;
    // the list travels through registers while this offer lasts: entry t of lane t (and t + 64 where the list is longer than a wave)
    const bool two = cap > 64;                           // uniform
    const int t0 = lane, t1 = lane + 64, last = cap - 1;
    const bool in0 = t0 < cap, in1 = t1 < cap;
    T e0 = in0 ? ld[t0] : nb_inf<T>(), e1 = nb_inf<T>();
    int i0 = in0 ? li[t0] : kNbEmpty, i1 = kNbEmpty;
    if (two && in1) { e1 = ld[t1]; i1 = li[t1]; }
    while (m) {                                          // uniform: m, nd, nj, wd, wi are the same in every lane
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const T nd = __shfl(d, src);
        const int nj = __shfl(j, src);
        wd = two ? __shfl(e1, last - 64) : __shfl(e0, last);
        wi = two ? __shfl(i1, last - 64) : __shfl(i0, last);
        if (!nb_less(nd, nj, wd, wi)) {                  // the list moved on since the ballot
            if (lane == src) tmin = nd < tmin ? nd : tmin;
            continue;
        }
        if (lane == src && wi != kNbEmpty) tmin = wd < tmin ? wd : tmin;
        int p = __popcll(__ballot(in0 && nb_less(e0, i0, nd, nj)));
        if (two) p += __popcll(__ballot(in1 && nb_less(e1, i1, nd, nj)));
        // entry t > p takes its predecessor's value, entry p the candidate; the last entry falls out
        if (two) {
            T pe1 = __shfl_up(e1, 1);
            int pi1 = __shfl_up(i1, 1);
            const T c0 = __shfl(e0, 63);
            const int ci0 = __shfl(i0, 63);
            if (lane == 0) { pe1 = c0; pi1 = ci0; }
            if (in1 && t1 > p) { e1 = pe1; i1 = pi1; }
            else if (t1 == p) { e1 = nd; i1 = nj; }
        }
        const T pe0 = __shfl_up(e0, 1);
        const int pi0 = __shfl_up(i0, 1);
        if (in0 && t0 > p) { e0 = pe0; i0 = pi0; }
        else if (t0 == p) { e0 = nd; i0 = nj; }
    }
    if (in0) { ld[t0] = e0; li[t0] = i0; }
    if (two && in1) { ld[t1] = e1; li[t1] = i1; }
    wave_lds_sync();
}

// ---- prepare -----------------------------------------------------------------------------------------------------------------------
// flag[row] = 1 when the row holds a NaN or an infinity, and for the padding rows [rows, rows_pad).  One wave per row.
__global__ __launch_bounds__(256) void nb_flags_kernel(const float* __restrict__ x, int rows, int rows_pad, int c, uint8_t* __restrict__ flag,
                                                       int* __restrict__ state, int* __restrict__ counter) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_pad) return;
    if (row >= rows) {
        if (lane == 0) flag[row] = 1;
        return;
    }
    const float* p = x + (size_t)row * c;
    bool bad = false;
    for (int ch = lane; ch < c; ch += 64) bad |= !nb_finite(p[ch]);
    const bool any = __ballot(bad) != 0;
    if (lane == 0) {
        flag[row] = any ? 1 : 0;
        if (state) state[row] = any ? 2 : 0;             // 0: needs the exact path, 1: certified, 2: non-finite query row
        if (any && counter) atomicAdd(counter, 1);
    }
}

// partial[chunk][ch] = float64 sum over the finite rows of the chunk, ascending; cnt[chunk] = finite rows of the chunk
__global__ __launch_bounds__(256) void nb_colsum_kernel(const float* __restrict__ x, const uint8_t* __restrict__ flag, int n, int c, int cp,
                                                        int rows_per, double* __restrict__ partial, int* __restrict__ cnt) {
    const int ch = blockIdx.y * 256 + threadIdx.x, chunk = blockIdx.x;
    if (ch >= c) return;
    const int r0 = chunk * rows_per, r1 = min(n, r0 + rows_per);
    double s = 0.0;
    int live = 0;
    for (int r = r0; r < r1; ++r) {
        if (flag[r]) continue;
        s += (double)x[(size_t)r * c + ch];
        ++live;
    }
    partial[(size_t)chunk * cp + ch] = s;
    if (ch == 0) cnt[chunk] = live;
}

__global__ __launch_bounds__(256) void nb_mean_kernel(const double* __restrict__ partial, const int* __restrict__ cnt, int chunks, int c, int cp,
                                                      float* __restrict__ mean) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= cp) return;
    double s = 0.0;
    long long live = 0;
    if (ch < c)
        for (int k = 0; k < chunks; ++k) {
            s += partial[(size_t)k * cp + ch];
            live += cnt[k];
        }
    mean[ch] = live > 0 ? (float)(s / (double)live) : 0.f;
}

// out[row][0 .. cp) = x[row] - mean (float32), zero for padding channels, padding rows and non-finite rows; norm[row] = its squared
// length in float32; *nbmax (corpus only) = the largest norm as float bits.  One wave per row.
__global__ __launch_bounds__(256) void nb_centre_kernel(const float* __restrict__ x, const uint8_t* __restrict__ flag, const float* __restrict__ mean,
                                                        int rows, int rows_pad, int c, int cp, float* __restrict__ out, float* __restrict__ norm,
                                                        unsigned* __restrict__ nbmax) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_pad) return;
    const bool live = row < rows && !flag[row];
    const float* p = x + (size_t)(live ? row : 0) * c;
    float* o = out + (size_t)row * cp;
    float ss = 0.f;
    for (int ch = lane; ch < cp; ch += 64) {
        const float v = (live && ch < c) ? p[ch] - mean[ch] : 0.f;
        o[ch] = v;
        ss += v * v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
    if (lane == 0) {
        norm[row] = ss;
        // ss >= 0 or +inf: the bit patterns order as the values do.  Only a row above the maximum seen so far pays for the atomic
        // (the plain read may be stale, which costs an atomic, never the result).
        if (nbmax && live && __float_as_uint(ss) > *(volatile unsigned*)nbmax) atomicMax(nbmax, __float_as_uint(ss));
    }
}

// ---- filter ------------------------------------------------------------------------------------------------------------------------
// Workgroup (x, y): query tile x (64 rows) against corpus tiles [y * tps, (y + 1) * tps) of 64 rows.  Wave w owns query rows 16 w ..
// 16 w + 15 of the tile: four 16 x 16 accumulators per corpus tile, one row of fragments (lane (r = lane & 15, g = lane >> 4) holds
// channels 4 g .. 4 g + 3 of row r of a 16-channel step, the same map for both operands, so the pairing of channels is right whatever
// order the hardware walks them in).  approximate = (na + nb) - 2 a.b goes to LDS, then each of the wave's rows offers its 64 values
// to its list.
__global__ __launch_bounds__(256) void nb_filter_kernel(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ na,
                                                        const float* __restrict__ nb, const uint8_t* __restrict__ bflag, int q, int cp, int kp,
                                                        int tps, int ntiles, int exclude_self, float* __restrict__ pd, int* __restrict__ pi,
                                                        float* __restrict__ pt, int* __restrict__ rowbad) {
    __shared__ __attribute__((aligned(16))) float sA[kNbTile * kNbLdk];
    __shared__ __attribute__((aligned(16))) float sB[kNbTile * kNbLdk];
    __shared__ float sD[kNbTile * (kNbTile + 1)];
    __shared__ float lD[kNbTile * kNbKpMax];
    __shared__ int lI[kNbTile * kNbKpMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * kNbTile, split = blockIdx.y, S = gridDim.y;
    const int tile0 = split * tps, tile1 = min(ntiles, tile0 + tps);

    for (int t = lane; t < 16 * kp; t += 64) {           // the wave's own 16 lists
        lD[16 * wave * kp + t] = nb_inf<float>();
        lI[16 * wave * kp + t] = kNbEmpty;
    }
    wave_lds_sync();
    float tmin[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) tmin[i] = nb_inf<float>();

    const int lrow0 = tid >> 3, lc4 = (tid & 7) * 4;      // this thread stages rows lrow0 and lrow0 + 32, channels lc4 .. lc4 + 3
    const float* a_src = A + (size_t)(q0 + lrow0) * cp + lc4;
    for (int tile = tile0; tile < tile1; ++tile) {
        const int n0 = tile * kNbTile;
        const float* b_src = B + (size_t)(n0 + lrow0) * cp + lc4;
        f4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
        f4 ra0 = *reinterpret_cast<const f4*>(a_src), ra1 = *reinterpret_cast<const f4*>(a_src + (size_t)32 * cp);
        f4 rb0 = *reinterpret_cast<const f4*>(b_src), rb1 = *reinterpret_cast<const f4*>(b_src + (size_t)32 * cp);
        for (int k0 = 0; k0 < cp; k0 += kNeighbourKStep) {
            __syncthreads();                             // the previous step's fragments have been read
            *reinterpret_cast<f4*>(&sA[lrow0 * kNbLdk + lc4]) = ra0;
            *reinterpret_cast<f4*>(&sA[(lrow0 + 32) * kNbLdk + lc4]) = ra1;
            *reinterpret_cast<f4*>(&sB[lrow0 * kNbLdk + lc4]) = rb0;
            *reinterpret_cast<f4*>(&sB[(lrow0 + 32) * kNbLdk + lc4]) = rb1;
            __syncthreads();
            if (k0 + kNeighbourKStep < cp) {             // the next slice travels while this one is multiplied
                const int kn = k0 + kNeighbourKStep;
                ra0 = *reinterpret_cast<const f4*>(a_src + kn);
                ra1 = *reinterpret_cast<const f4*>(a_src + (size_t)32 * cp + kn);
                rb0 = *reinterpret_cast<const f4*>(b_src + kn);
                rb1 = *reinterpret_cast<const f4*>(b_src + (size_t)32 * cp + kn);
            }
#pragma unroll
            for (int kk = 0; kk < kNeighbourKStep; kk += 16) {
                const f4 fa = *reinterpret_cast<const f4*>(&sA[(16 * wave + r) * kNbLdk + kk + 4 * g]);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f4 fb = *reinterpret_cast<const f4*>(&sB[(16 * t + r) * kNbLdk + kk + 4 * g]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[j], fb[j], acc[t], 0, 0, 0);
                }
            }
        }
        // accumulator t, register i of lane (r, g): query row 16 wave + 4 g + i, corpus row n0 + 16 t + r
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float nbv = nb[n0 + 16 * t + r];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * wave + 4 * g + i;
                sD[row * (kNbTile + 1) + 16 * t + r] = (na[q0 + row] + nbv) - 2.f * acc[t][i];
            }
        }
        wave_lds_sync();
        const int j = n0 + lane;
        const bool corpus_ok = !bflag[j];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = 16 * wave + rr, qi = q0 + row;
            if (qi < q) {
                const float d = sD[row * (kNbTile + 1) + lane];
                const bool eligible = corpus_ok && !(exclude_self && j == qi);
                const bool finite = nb_finite(d);
                if (eligible && !finite) rowbad[qi] = 1;     // every writer stores the same value
                nb_offer<float>(lD + row * kp, lI + row * kp, kp, d, j, eligible && finite, tmin[rr], lane);
            }
        }
        wave_lds_sync();
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int row = 16 * wave + rr, qi = q0 + row;
        const float t = nb_wave_min(tmin[rr]);
        if (qi < q) {
            const size_t base = ((size_t)qi * S + split) * kp;
            for (int e = lane; e < kp; e += 64) {
                pd[base + e] = lD[row * kp + e];
                pi[base + e] = lI[row * kp + e];
            }
            if (lane == 0) pt[(size_t)qi * S + split] = t;
        }
    }
}

// ---- the definition ----------------------------------------------------------------------------------------------------------------
template <class PA>
__device__ __forceinline__ double nb_exact_d(PA a, const float* __restrict__ b, int c) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int ch = 0; ch < c; ++ch) {
        const double t = (double)a[ch] - (double)b[ch];
        const double p = t * t;
        s = s + p;
    }
    return s;
}

// ---- refine + certify: one wave per query row ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nb_refine_kernel(const float* __restrict__ queries, const float* __restrict__ corpus, int q, int c, int k,
                                                        int kp, int S, const float* __restrict__ pd, const int* __restrict__ pi,
                                                        const float* __restrict__ pt, const float* __restrict__ na,
                                                        const unsigned* __restrict__ nbmax, const int* __restrict__ rowbad, int* __restrict__ state,
                                                        int32_t* __restrict__ indices, double* __restrict__ dist, NeighbourStats* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ float lDs[4][kNbKpMax];
    __shared__ int lIs[4][kNbKpMax];
    __shared__ double sDDs[4][kNbKpMax];
    __shared__ double sDk[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x * 4 + wave;
    if (row >= q || state[row] == 2) return;
    float* lD = lDs[wave];
    int* lI = lIs[wave];
    double* sDD = sDDs[wave];
    for (int t = lane; t < kp; t += 64) {
        lD[t] = nb_inf<float>();
        lI[t] = kNbEmpty;
    }
    wave_lds_sync();
    float tmin = nb_inf<float>();
    for (int s = lane; s < S; s += 64) tmin = fminf(tmin, pt[(size_t)row * S + s]);
    // the split lists, 64 entries at a time; the next piece is on its way while this one is offered
    const int pieces = (kp + 63) / 64, total = S * pieces;
    auto fetch = [&](int u, float& d, int& j) {
        const int t = (u % pieces) * 64 + lane;
        const size_t at = ((size_t)row * S + u / pieces) * kp + t;
        j = t < kp ? pi[at] : kNbEmpty;
        d = t < kp ? pd[at] : nb_inf<float>();
    };
    float d = 0.f, dn = 0.f;
    int j = kNbEmpty, jn = kNbEmpty;
    fetch(0, d, j);
    for (int u = 0; u < total; ++u) {
        if (u + 1 < total) fetch(u + 1, dn, jn);
        nb_offer<float>(lD, lI, kp, d, j, j != kNbEmpty, tmin, lane);
        d = dn;
        j = jn;
    }
    const float T = nb_wave_min(tmin);
    const int t0 = lane, t1 = lane + 64;
    const int j0 = t0 < kp ? lI[t0] : kNbEmpty, j1 = t1 < kp ? lI[t1] : kNbEmpty;
    const int count = __popcll(__ballot(j0 != kNbEmpty)) + __popcll(__ballot(j1 != kNbEmpty));   // filled entries come first
    const float* a = queries + (size_t)row * c;
    double d0 = 0.0, d1 = 0.0;
    if (j0 != kNbEmpty) sDD[t0] = d0 = nb_exact_d(a, corpus + (size_t)j0 * c, c);
    if (j1 != kNbEmpty) sDD[t1] = d1 = nb_exact_d(a, corpus + (size_t)j1 * c, c);
    wave_lds_sync();
    int rank0 = 0, rank1 = 0;
    for (int u = 0; u < count; ++u) {
        const double du = sDD[u];
        const int ju = lI[u];
        rank0 += nb_less(du, ju, d0, j0) ? 1 : 0;
        rank1 += nb_less(du, ju, d1, j1) ? 1 : 0;
    }
    if (j0 != kNbEmpty && rank0 < k) { indices[(size_t)row * k + rank0] = j0; dist[(size_t)row * k + rank0] = d0; }
    if (j1 != kNbEmpty && rank1 < k) { indices[(size_t)row * k + rank1] = j1; dist[(size_t)row * k + rank1] = d1; }
    if (j0 != kNbEmpty && rank0 == k - 1) sDk[wave] = d0;
    if (j1 != kNbEmpty && rank1 == k - 1) sDk[wave] = d1;
    for (int t = count + lane; t < k; t += 64) { indices[(size_t)row * k + t] = -1; dist[(size_t)row * k + t] = (double)nb_inf<float>(); }
    wave_lds_sync();
    if (lane == 0) {
        const float an = na[row], bn = __uint_as_float(*nbmax);
        bool certified = !rowbad[row] && nb_finite(an) && nb_finite(bn);
        if (certified && nb_finite(T)) {
            // E = 2^-24 (2 C + 12) (|a~|^2 + max |b~|^2) + (4 C + 8) 2^-149 (the second term: products that underflow float32)
            const double e = ldexp((double)(2 * c + 12) * ((double)an + (double)bn), -24) + ldexp((double)(4 * c + 8), -149);
            certified = count >= k && sDk[wave] < (double)T - e;
        }
        if (certified) {
            state[row] = 1;
            atomicAdd(&stats->certified_rows, 1);
        }
    }
}

// ---- exact path: one workgroup per query row ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nb_exact_kernel(const float* __restrict__ queries, const float* __restrict__ corpus, int q, int n, int c, int k,
                                                       int exclude_self, const uint8_t* __restrict__ bflag, const int* __restrict__ state,
                                                       int32_t* __restrict__ indices, double* __restrict__ dist, NeighbourStats* __restrict__ stats) {
    __shared__ float sa[kNeighbourMaxC];
    __shared__ double sDD[256];
    __shared__ double lD[64];
    __shared__ int lI[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    if (row == 0 && tid == 0) stats->query_rows = q;
    const int st = state[row];
    if (st == 1) return;
    if (st == 2) {
        for (int t = tid; t < k; t += 256) { indices[(size_t)row * k + t] = -1; dist[(size_t)row * k + t] = __builtin_nan(""); }
        if (tid == 0) atomicAdd(&stats->nonfinite_query_rows, 1);
        return;
    }
    for (int ch = tid; ch < c; ch += 256) sa[ch] = queries[(size_t)row * c + ch];
    if (tid < 64) { lD[tid] = nb_inf<double>(); lI[tid] = kNbEmpty; }
    __syncthreads();
    double tmin = nb_inf<double>();                      // not used: nothing is certified here
    for (int base = 0; base < n; base += 256) {
        const int j = base + tid;
        double d = -1.0;                                 // D >= 0: a negative value marks "not eligible"
        if (j < n && !bflag[j] && !(exclude_self && j == row)) d = nb_exact_d(sa, corpus + (size_t)j * c, c);
        sDD[tid] = d;
        __syncthreads();
        if (wave == 0) {
            for (int u = 0; u < 256; u += 64) {
                const double du = sDD[u + lane];
                nb_offer<double>(lD, lI, k, du, base + u + lane, du >= 0.0, tmin, lane);
            }
        }
        __syncthreads();
    }
    if (tid < k) {
        const int j = lI[tid];
        indices[(size_t)row * k + tid] = j == kNbEmpty ? -1 : j;
        dist[(size_t)row * k + tid] = lD[tid];
    }
    if (tid == 0) atomicAdd(&stats->exact_rows, 1);
}

inline size_t nb_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

NeighbourPlan neighbour_plan(int q, int n, int c, int k) {
    NeighbourPlan p{};
    p.q = q; p.n = n; p.c = c; p.k = k;
    p.cp = (c + kNeighbourKStep - 1) / kNeighbourKStep * kNeighbourKStep;
    p.kp = k + kNeighbourSlack;
    p.qtiles = (q + kNbTile - 1) / kNbTile;
    p.ntiles = (n + kNbTile - 1) / kNbTile;
    p.qpad = p.qtiles * kNbTile;
    p.npad = p.ntiles * kNbTile;
    // enough workgroups for the whole device whatever the shape: a tall query table needs no split, a handful of queries splits the
    // corpus down to single tiles
    const int want = std::min(kNeighbourMaxSplits, std::max(1, (kNeighbourTargetBlocks + p.qtiles - 1) / p.qtiles));
    p.tiles_per_split = (p.ntiles + want - 1) / want;
    p.splits = (p.ntiles + p.tiles_per_split - 1) / p.tiles_per_split;
    p.mean_chunks = std::min(kNeighbourMeanChunks, (n + 127) / 128);
    p.mean_rows = (n + p.mean_chunks - 1) / p.mean_chunks;
    p.mean_chunks = (n + p.mean_rows - 1) / p.mean_rows;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += nb_up(bytes); return at; };
    p.off_stats = take(sizeof(NeighbourStats));
    p.off_nbmax = take(sizeof(unsigned));
    p.off_rowbad = take((size_t)p.qpad * sizeof(int));
    p.off_state = take((size_t)p.qpad * sizeof(int));
    p.off_qflag = take((size_t)p.qpad);
    p.off_bflag = take((size_t)p.npad);
    p.off_cnt = take((size_t)p.mean_chunks * sizeof(int));
    p.off_partial = take((size_t)p.mean_chunks * p.cp * sizeof(double));
    p.off_mean = take((size_t)p.cp * sizeof(float));
    p.off_na = take((size_t)p.qpad * sizeof(float));
    p.off_nb = take((size_t)p.npad * sizeof(float));
    p.off_a = take((size_t)p.qpad * p.cp * sizeof(float));
    p.off_b = take((size_t)p.npad * p.cp * sizeof(float));
    p.off_pd = take((size_t)p.qpad * p.splits * p.kp * sizeof(float));
    p.off_pi = take((size_t)p.qpad * p.splits * p.kp * sizeof(int));
    p.off_pt = take((size_t)p.qpad * p.splits * sizeof(float));
    p.bytes = o;
    return p;
}

hipError_t embedding_neighbours(const float* queries, int q, const float* corpus, int n, int c, int k, int flags, int32_t* indices,
                                double* sq_distances, NeighbourStats* stats, void* scratch, hipStream_t s) {
    if (!queries || !corpus || !indices || !sq_distances || !scratch || q < 1 || n < 1 || c < 1 || k < 1 || q > kNeighbourMaxRows ||
        n > kNeighbourMaxRows || c > kNeighbourMaxC || k > kNeighbourMaxK || ((uintptr_t)scratch & 15u))
        return hipErrorInvalidValue;
    const NeighbourPlan p = neighbour_plan(q, n, c, k);
    char* base = static_cast<char*>(scratch);
    auto at = [&](size_t off) { return static_cast<void*>(base + off); };
    NeighbourStats* st = stats ? stats : static_cast<NeighbourStats*>(at(p.off_stats));
    unsigned* nbmax = static_cast<unsigned*>(at(p.off_nbmax));
    int* rowbad = static_cast<int*>(at(p.off_rowbad));
    int* state = static_cast<int*>(at(p.off_state));
    uint8_t* qflag = static_cast<uint8_t*>(at(p.off_qflag));
    uint8_t* bflag = static_cast<uint8_t*>(at(p.off_bflag));
    const int exclude_self = (flags & kNeighbourExcludeSelf) ? 1 : 0;
    hipError_t e;
    if ((e = hipMemsetAsync(st, 0, sizeof(NeighbourStats), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(nbmax, 0, sizeof(unsigned), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(rowbad, 0, (size_t)p.qpad * sizeof(int), s)) != hipSuccess) return e;
    const dim3 b256(256);
    hipLaunchKernelGGL(nb_flags_kernel, dim3(p.npad / 4), b256, 0, s, corpus, n, p.npad, c, bflag, (int*)nullptr, &st->nonfinite_corpus_rows);
    hipLaunchKernelGGL(nb_flags_kernel, dim3(p.qpad / 4), b256, 0, s, queries, q, p.qpad, c, qflag, state, (int*)nullptr);   // counted by the exact kernel
    if (!(flags & kNeighbourExactOnly)) {
        int* cnt = static_cast<int*>(at(p.off_cnt));
        double* partial = static_cast<double*>(at(p.off_partial));
        float* mean = static_cast<float*>(at(p.off_mean));
        float* na = static_cast<float*>(at(p.off_na));
        float* nb = static_cast<float*>(at(p.off_nb));
        float* A = static_cast<float*>(at(p.off_a));
        float* B = static_cast<float*>(at(p.off_b));
        float* pd = static_cast<float*>(at(p.off_pd));
        int* pi = static_cast<int*>(at(p.off_pi));
        float* pt = static_cast<float*>(at(p.off_pt));
        hipLaunchKernelGGL(nb_colsum_kernel, dim3(p.mean_chunks, (c + 255) / 256), b256, 0, s, corpus, bflag, n, c, p.cp, p.mean_rows, partial, cnt);
        hipLaunchKernelGGL(nb_mean_kernel, dim3((p.cp + 255) / 256), b256, 0, s, partial, cnt, p.mean_chunks, c, p.cp, mean);
        hipLaunchKernelGGL(nb_centre_kernel, dim3(p.npad / 4), b256, 0, s, corpus, bflag, mean, n, p.npad, c, p.cp, B, nb, nbmax);
        hipLaunchKernelGGL(nb_centre_kernel, dim3(p.qpad / 4), b256, 0, s, queries, qflag, mean, q, p.qpad, c, p.cp, A, na, (unsigned*)nullptr);
        hipLaunchKernelGGL(nb_filter_kernel, dim3(p.qtiles, p.splits), b256, 0, s, A, B, na, nb, bflag, q, p.cp, p.kp, p.tiles_per_split, p.ntiles,
                           exclude_self, pd, pi, pt, rowbad);
        hipLaunchKernelGGL(nb_refine_kernel, dim3((q + 3) / 4), b256, 0, s, queries, corpus, q, c, k, p.kp, p.splits, pd, pi, pt, na, nbmax, rowbad,
                           state, indices, sq_distances, st);
    }
    hipLaunchKernelGGL(nb_exact_kernel, dim3(q), b256, 0, s, queries, corpus, q, n, c, k, exclude_self, bflag, state, indices, sq_distances, st);
    return hipGetLastError();
}

}  // namespace cv
