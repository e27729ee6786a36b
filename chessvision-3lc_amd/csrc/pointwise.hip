// pointwise.hip -- the HBM-bound kernels of the ChessVision hot path, hand-written for gfx950.
//
// Everything here moves 16 bytes per lane per access (8 f16 / 4 f32 channels of one NHWC pixel), is
// launched with >> 256 workgroups, and has no inter-block reuse, so there is nothing to tile: the bound is
// HBM bytes ((elements in + elements out) * dtype size).
//
// Reference ops replaced:  max_pool2d 2x2 (UNet Down), max_pool2d 3x3 s2 p1 (ResNet),
// upsample_bilinear2d(align_corners=True) (UNet Up, bilinear variant), conv2d 1x1 64->1 + bias (OutConv) fused
// with sigmoid/threshold (core.py:273, utils.py:101-112), conv 7x7 s2 p3 + BN + ReLU (ResNet stem),
// adaptive_avg_pool2d(1) + linear 512->13 (+ softmax, core.py:242), and the u8 HWC -> /255 -> NCHW input
// packing of core.py:215-216 / 236-237.
#include "pointwise.h"
#include "engine.h"        // env_switch

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace cv {

// A "group" = the channels one lane moves per access: 8 (f16: 16 B; split-f16: 16 B hi + 16 B lo) or 4 (f32: 16 B).
template <typename T> struct Grp;
template <> struct Grp<half_t> {
    static constexpr int N = 8, BYTES = 16;
    static __device__ __forceinline__ void load(const char* p, int, float* v) {
        const half8 h = *reinterpret_cast<const half8*>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
    }
    static __device__ __forceinline__ void store(char* p, int, const float* v) {
        half8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (half_t)v[j];
        *reinterpret_cast<half8*>(p) = h;
    }
    static __device__ __forceinline__ void store(char* p, int par, const float* v, float& bad) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bad = __builtin_fmaf((float)(half_t)v[j], 0.f, bad);
        store(p, par, v);
    }
};
template <> struct Grp<float> {
    static constexpr int N = 4, BYTES = 16;
    static __device__ __forceinline__ void load(const char* p, int, float* v) {
        const f4 h = *reinterpret_cast<const f4*>(p);
        v[0] = h[0]; v[1] = h[1]; v[2] = h[2]; v[3] = h[3];
    }
    static __device__ __forceinline__ void store(char* p, int, const float* v) {
        *reinterpret_cast<f4*>(p) = f4{v[0], v[1], v[2], v[3]};
    }
    static __device__ __forceinline__ void store(char* p, int par, const float* v, float& bad) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bad = __builtin_fmaf(v[j], 0.f, bad);
        store(p, par, v);
    }
};
template <> struct Grp<split_t> {              // [hi x8][lo x8] for even groups, [lo x8][hi x8] for odd ones
    static constexpr int N = 8, BYTES = 32;
    static __device__ __forceinline__ void load(const char* p, int parity, float* v) {
        const half8 hi = *reinterpret_cast<const half8*>(p + (parity ? 16 : 0));
        const half8 lo = *reinterpret_cast<const half8*>(p + (parity ? 0 : 16));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)hi[j] + (float)lo[j];
    }
    static __device__ __forceinline__ void store(char* p, int parity, const float* v) {
        typedef unsigned u4 __attribute__((ext_vector_type(4)));
        u4 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            unsigned hp, lp;
            split_pair(v[j], v[j + 1], hp, lp);             // cv_kernels.h: three vector instructions per pair
            hi[j / 2] = hp; lo[j / 2] = lp;
        }
        *reinterpret_cast<u4*>(p + (parity ? 16 : 0)) = hi;
        *reinterpret_cast<u4*>(p + (parity ? 0 : 16)) = lo;
    }
    static __device__ __forceinline__ void store(char* p, int parity, const float* v, float& bad) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bad = __builtin_fmaf((float)(half_t)v[j], 0.f, bad);   // inf / NaN -> NaN
        store(p, parity, v);
    }
};

// numeric guard (cv_kernels.h: ConvParams::flag): the lowest layer id that stored a non-finite value wins
__device__ __forceinline__ void report_bad(unsigned* flag, unsigned layer_id, float bad) {
    if (bad != bad && flag) atomicMin(flag, layer_id);
}

__device__ __forceinline__ size_t pix_index(const TensorRef& t, int n, int y, int x) {
    return (size_t)(n * (t.H + 2) + y + 1) * (t.W + 2) + (x + 1);
}
// byte address and hi/lo parity of group g (counted from the slice's first channel) of pixel `pix`
template <typename T> __device__ __forceinline__ char* grp_ptr(const TensorRef& t, size_t pix, int g, int* parity) {
    constexpr int ESZ = Grp<T>::BYTES / Grp<T>::N;
    *parity = (t.Coff / Grp<T>::N + g) & 1;
    return reinterpret_cast<char*>(t.base) + (pix * t.Cs + t.Coff) * ESZ + (size_t)g * Grp<T>::BYTES;
}

static inline unsigned grid_for(size_t work, int block = 256) {
    size_t g = (work + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : g);
}

// The one flat-index decode of this file.  A flat interior-pixel index of `t` (x fastest, then y, then the image) -> (n, y, x); the
// index is 64-bit, as every kernel's flat work index is.  What is left above the rows lands in n: the image, or image * C + channel
// for a walk over planes (unpack_nchw_f32_kernel).
struct Pix { int n, y, x; };
__device__ __forceinline__ Pix decode_pix(const TensorRef& t, size_t pix) {
    Pix r;
    r.x = (int)(pix % t.W); pix /= t.W;
    r.y = (int)(pix % t.H);
    r.n = (int)(pix / t.H);
    return r;
}
// a flat (pixel, group) work index of `t`, group fastest: the thread's own unless the kernel strides over several
struct PG : Pix { int g; bool live; };
template <typename T>
__device__ __forceinline__ PG decode_pg(const TensorRef& t, size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x) {
    const int groups = t.C / Grp<T>::N;
    PG r;
    r.live = idx < (size_t)t.N * t.H * t.W * groups;
    r.g = (int)(idx % groups);
    static_cast<Pix&>(r) = decode_pix(t, idx / groups);
    return r;
}

// ---- packing ----------------------------------------------------------------------------------------
template <typename T>
__global__ void pack_nchw_f32_kernel(const float* __restrict__ src, int c, TensorRef dst, float mul, unsigned* flag) {
    constexpr int GN = Grp<T>::N;
    const PG p = decode_pg<T>(dst);
    if (!p.live) return;
    float v[GN];
#pragma unroll
    for (int j = 0; j < GN; ++j) {
        const int ch = p.g * GN + j;
        v[j] = ch < c ? src[((size_t)(p.n * c + ch) * dst.H + p.y) * dst.W + p.x] * mul : 0.f;
    }
    int par;
    char* d = grp_ptr<T>(dst, pix_index(dst, p.n, p.y, p.x), p.g, &par);
    float bad = 0.f;
    Grp<T>::store(d, par, v, bad);
    report_bad(flag, 0u, bad);                               // layer id 0 = the caller's input tensor
}

template <typename T>
__global__ void pack_hwc3_u8_kernel(const uint8_t* __restrict__ src, TensorRef dst, float mul) {
    constexpr int GN = Grp<T>::N;
    const size_t total = (size_t)dst.N * dst.H * dst.W;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const Pix p = decode_pix(dst, idx);
    const uint8_t* s = src + idx * 3;
    // /255 first (the reference's arithmetic, core.py:215), then the power-of-two range factor (exact)
    const float f[8] = {(float)s[0] / 255.f * mul, (float)s[1] / 255.f * mul, (float)s[2] / 255.f * mul, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 8 / GN; ++g) {
        int par;
        char* d = grp_ptr<T>(dst, pix_index(dst, p.n, p.y, p.x), g, &par);
        Grp<T>::store(d, par, f + g * GN);
    }
}

template <typename T>
__global__ void unpack_nchw_f32_kernel(TensorRef src, float* __restrict__ dst, float mul) {
    constexpr int GN = Grp<T>::N;
    const size_t total = (size_t)src.N * src.C * src.H * src.W;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const Pix q = decode_pix(src, idx);                      // q.n: the plane, image * C + channel (< 2^31 as N * C is)
    const int c = q.n % src.C, n = q.n / src.C;
    int par;
    const char* p = grp_ptr<T>(src, pix_index(src, n, q.y, q.x), c / GN, &par);
    float v[GN];
    Grp<T>::load(p, par, v);
    float out = v[0];
#pragma unroll
    for (int j = 1; j < GN; ++j) out = (c % GN) == j ? v[j] : out;
    dst[idx] = out * mul;
}

// ---- range calibration: max |stored value| over the interior of a slice, as the bits of a non-negative float ------
// (unsigned order == float order there; NaN bit patterns sort above +inf, so "non-finite" reads as >= 0x7f800000)
template <typename T>
__global__ void absmax_kernel(TensorRef src, unsigned* __restrict__ out) {
    constexpr int GN = Grp<T>::N;
    unsigned m = 0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;; idx += (size_t)gridDim.x * blockDim.x) {
        const PG p = decode_pg<T>(src, idx);
        if (!p.live) break;
        int par;
        float v[GN];
        Grp<T>::load(grp_ptr<T>(src, pix_index(src, p.n, p.y, p.x), p.g, &par), par, v);
#pragma unroll
        for (int j = 0; j < GN; ++j) {
            const unsigned b = __float_as_uint(v[j]) & 0x7fffffffu;
            m = b > m ? b : m;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// ---- embeddings: per-image channel means of a stored tensor, out[n][c] = mul * mean over the H x W interior (pointwise.h:
// channel_means).  A lane owns 8 consecutive channels (one 16-B load for f16, two for split-f16 and f32) of one pixel SLICE: with
// P = H * W and S = channel_means_slices(P), lane (unit u, slice s) adds pixels s, s + S, s + 2 S, .. in that order, the i-th of them
// into accumulator i % 8; the 8 accumulators are joined by a fixed tree, and the S slices of a unit by a halving tree through LDS.
// unit u = n * (C / 8) + channel group; a workgroup holds 256 / S consecutive units in its low lane bits, so consecutive lanes read
// consecutive 16-B groups of one pixel.  The order of every addition follows from (H, W) alone -- not from N, the grid, or where in a
// chunk an image sits: an image's row has the same bits pooled alone or as image 63 of 64.  No atomics.
__host__ __device__ inline int channel_means_slices(int pixels) {
    int s = 1;
    while (s < 256 && pixels > 8 * s) s *= 2;               // at most 8 pixels per lane until the workgroup is one unit wide (256 x 256: 256)
    return s;
}

template <typename T>
__global__ __launch_bounds__(256) void channel_means_kernel(TensorRef src, int slices, float mul, float* __restrict__ out) {
    constexpr int GN = Grp<T>::N, GPL = 8 / GN;              // groups per lane: 1 (f16, split-f16) or 2 (f32)
    __shared__ float part[8][256];
    const int upb = 256 / slices;                            // units per workgroup
    const int ul = threadIdx.x % upb, sl = threadIdx.x / upb;
    const int cgs = src.C / 8, pixels = src.H * src.W;
    const size_t unit = (size_t)blockIdx.x * upb + ul;
    const bool live = unit < (size_t)src.N * cgs;
    const int n = live ? (int)(unit / cgs) : 0, cg = live ? (int)(unit % cgs) : 0;
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[a][j] = 0.f;
    if (live)
        for (int p0 = sl; p0 < pixels; p0 += 8 * slices) {
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const int p = p0 + a * slices;
                if (p < pixels) {
                    const size_t pix = pix_index(src, n, p / src.W, p % src.W);
#pragma unroll
                    for (int g = 0; g < GPL; ++g) {
                        int par;
                        float v[GN];
                        Grp<T>::load(grp_ptr<T>(src, pix, cg * GPL + g, &par), par, v);
#pragma unroll
                        for (int j = 0; j < GN; ++j) acc[a][g * GN + j] += v[j];
                    }
                }
            }
        }
    float s8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        s8[j] = ((acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j])) + ((acc[4][j] + acc[5][j]) + (acc[6][j] + acc[7][j]));
    if (slices > 1) {                                        // uniform over the launch
#pragma unroll
        for (int j = 0; j < 8; ++j) part[j][threadIdx.x] = s8[j];
        for (int h = slices / 2; h >= 1; h /= 2) {
            __syncthreads();
            if (sl < h) {
#pragma unroll
                for (int j = 0; j < 8; ++j) part[j][threadIdx.x] += part[j][threadIdx.x + h * upb];
            }
        }
        if (sl == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s8[j] = part[j][threadIdx.x];
        }
    }
    if (live && sl == 0) {
        const float count = (float)pixels;
        float* o = out + (size_t)n * src.C + cg * 8;
        *reinterpret_cast<f4*>(o) = f4{s8[0] * mul / count, s8[1] * mul / count, s8[2] * mul / count, s8[3] * mul / count};
        *reinterpret_cast<f4*>(o + 4) = f4{s8[4] * mul / count, s8[5] * mul / count, s8[6] * mul / count, s8[7] * mul / count};
    }
}

// ---- load-time rounding-bias calibration (engine.cpp: Engine::measure_tap_sums): per convolution tap and input channel, the sum of
// the stored f16 input over the slice's images and every output position -- out[slice][tap][c] = sum_n sum_(oy,ox) x(n, oy*stride +
// ky - pad, ox*stride + kx - pad, c), the zero border read as it is.  One lane = one channel (consecutive lanes read consecutive
// halves); slices are summed on the host in index order, so the result is the same from run to run.
__global__ __launch_bounds__(64) void tap_sums_f16_kernel(TensorRef src, int Ho, int Wo, int stride, int k, int n_per_slice, double* __restrict__ out) {
    const int tap = blockIdx.x, c = blockIdx.y * 64 + threadIdx.x, slice = blockIdx.z;
    if (c >= src.C) return;
    const int pad = (k - 1) / 2, ky = tap / k, kx = tap % k;
    const half_t* base = reinterpret_cast<const half_t*>(src.base) + src.Coff + c;
    const int n0 = slice * n_per_slice, n1 = min(src.N, n0 + n_per_slice);
    double total = 0.0;
    for (int n = n0; n < n1; ++n) {
        float part = 0.f;                                  // <= Ho * Wo terms of one image in f32, images in f64
        for (int oy = 0; oy < Ho; ++oy) {
            const size_t row = ((size_t)n * (src.H + 2) + (size_t)(oy * stride + ky - pad + 1)) * (src.W + 2);
            for (int ox = 0; ox < Wo; ++ox) part += (float)base[(row + (size_t)(ox * stride + kx - pad + 1)) * src.Cs];
        }
        total += (double)part;
    }
    out[((size_t)slice * (k * k) + tap) * src.C + c] = total;
}

// ---- pooling / upsampling --------------------------------------------------------------------------
template <typename T>
__global__ void maxpool2x2_kernel(TensorRef src, TensorRef dst) {
    constexpr int GN = Grp<T>::N;
    const PG p = decode_pg<T>(dst);
    if (!p.live) return;
    float m[GN], v[GN];
    int par;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const char* s = grp_ptr<T>(src, pix_index(src, p.n, 2 * p.y + (t >> 1), 2 * p.x + (t & 1)), p.g, &par);
        Grp<T>::load(s, par, v);
#pragma unroll
        for (int j = 0; j < GN; ++j) m[j] = t == 0 ? v[j] : fmaxf(m[j], v[j]);
    }
    char* d = grp_ptr<T>(dst, pix_index(dst, p.n, p.y, p.x), p.g, &par);
    Grp<T>::store(d, par, m);
}

template <typename T>
__global__ void maxpool3x3s2_kernel(TensorRef src, TensorRef dst) {
    constexpr int GN = Grp<T>::N;
    const PG p = decode_pg<T>(dst);
    if (!p.live) return;
    float m[GN], v[GN];
#pragma unroll
    for (int j = 0; j < GN; ++j) m[j] = -INFINITY;
    int par;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * p.y - 1 + ky;
        if (iy < 0 || iy >= src.H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * p.x - 1 + kx;
            if (ix < 0 || ix >= src.W) continue;
            const char* s = grp_ptr<T>(src, pix_index(src, p.n, iy, ix), p.g, &par);
            Grp<T>::load(s, par, v);
#pragma unroll
            for (int j = 0; j < GN; ++j) m[j] = fmaxf(m[j], v[j]);
        }
    }
    char* d = grp_ptr<T>(dst, pix_index(dst, p.n, p.y, p.x), p.g, &par);
    Grp<T>::store(d, par, m);
}

// acc + w * (the low | high f16 half of `packed`), the f16 read by the FMA itself (v_fma_mix_f32: no separate conversion).  The compiler
// does not form this instruction from (float)h * w + acc here; only for kernels without MFMAs (cv_kernels.h: split_pair's note).
__device__ __forceinline__ float fma_mix_f16(unsigned packed, int high, float w, float acc) {
    float r;
#if defined(__HIP_DEVICE_COMPILE__)
    if (high) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(packed), "v"(w), "v"(acc));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(packed), "v"(w), "v"(acc));
#else
    r = acc + w * (float)packed * 0.f + (float)high;      // host pass of the single-source compile: never executed
#endif
    return r;
}

// source pair and upper weight of one output index: torch's area_pixel_compute_source_index / compute_source_index_and_lambda with
// align_corners -- the product scale * index is ROUNDED before the integer part is taken off (no fused multiply-subtract: with
// contraction left to the compiler the two up-sample kernels below differed in the last bit of their weights)
__device__ __forceinline__ void bilinear_axis(float scale, int index, int in_size, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
    const float f = scale * (float)index;
    i0 = (int)f;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = f - (float)i0;
}

// ---- the split-f16 up-sample, shared by the two kernels below: one tap loader, one blend-and-store tail, hence the same bits ----------
// (round 5) With every tap converted to f32 (hi + lo) before the blend the kernel was bound by vector issue, not by HBM: ~200
// instructions per 32 stored bytes.  The taps stay f16: each of the eight products per value is one mixed-precision FMA that reads the
// f16 half directly (v_fma_mix_f32), the four weights ly * lx * mul are formed once per output and rounded once (the nested form of the
// other storage types rounds its partial sums: a last-bit difference; the parity bars are 1e-5 on the op, 1e-3 end to end), and the
// numeric guard runs on the packed hi pairs.
// The four taps (y0 | y1, x0 | x1) of group g, t[tap][0..3] the first 16-byte half of the group and t[tap][4..7] the second.  32-bit
// byte offsets from the (wave-uniform) tensor base: tensors stay below 4 GiB (checked by the engine), and the per-tap 64-bit address
// arithmetic was a third of the vector instructions.
__device__ __forceinline__ void upsample_split_load4(const TensorRef& src, int n, int y0, int y1, int x0, int x1, unsigned g, unsigned (&t)[4][8]) {
    const char* const sbase = reinterpret_cast<const char*>(src.base);
    const unsigned spix = (unsigned)src.Cs * 4u, goff = (unsigned)src.Coff * 4u + g * 32u;
    const unsigned r0 = (unsigned)pix_index(src, n, y0, 0), r1 = (unsigned)pix_index(src, n, y1, 0);
    const unsigned o00 = (r0 + (unsigned)x0) * spix + goff, o10 = (r1 + (unsigned)x0) * spix + goff, dxb = (unsigned)(x1 - x0) * spix;
    const unsigned off[4] = {o00, o00 + dxb, o10, o10 + dxb};
    typedef unsigned u4t __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u4t a = *reinterpret_cast<const u4t*>(sbase + off[q]), b = *reinterpret_cast<const u4t*>(sbase + off[q] + 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) { t[q][i] = a[i]; t[q][4 + i] = b[i]; }
    }
}
// one output pixel's group from its four taps: blend (taps 00, 01, 10, 11; of each the first half, then the second -- which of them
// holds hi and which lo does not matter to the sum), split, guard, store by the output group's parity
__device__ __forceinline__ void upsample_split_emit(const TensorRef& dst, size_t opix, unsigned g, const unsigned (&t)[4][8], float w00, float w01,
                                                    float w10, float w11, float& bad) {
    const float wt[4] = {w00, w01, w10, w11};
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
    // tap-major: the eight accumulators are independent, so no FMA waits for the one before it (value-major, the compiler padded every
    // dependent pair of these asm instructions with an s_nop)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = fma_mix_f16(t[k][j >> 1], j & 1, wt[k], o[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = fma_mix_f16(t[k][4 + (j >> 1)], j & 1, wt[k], o[j]);
    }
    const int opar = (dst.Coff / 8 + (int)g) & 1;
    char* const dp = reinterpret_cast<char*>(dst.base) + ((unsigned)opix * ((unsigned)dst.Cs * 4u) + (unsigned)dst.Coff * 4u + g * 32u);
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    u4 hi, lo;
    h2 g2 = {(half_t)0.f, (half_t)0.f};
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        unsigned hp, lp;
        split_pair(o[j], o[j + 1], hp, lp);                   // behind the FMAs that consume nothing else: no MFMA in these kernels
        g2 = __builtin_elementwise_fma(__builtin_bit_cast(h2, hp), h2{(half_t)0.f, (half_t)0.f}, g2);
        hi[j / 2] = hp; lo[j / 2] = lp;
    }
    bad = __builtin_fmaf((float)g2[0] + (float)g2[1], 0.f, bad);
    *reinterpret_cast<u4*>(dp + (opar ? 16 : 0)) = hi;
    *reinterpret_cast<u4*>(dp + (opar ? 0 : 16)) = lo;
}

// torch upsample_bilinear2d, align_corners=True: src = dst * (in-1)/(out-1); weights (1-l, l) in f32.
// Grid = (row segments, output rows, images): the row's source lines and vertical weights are wave-uniform and a thread finds its
// (column, channel group) with one 32-bit division (r03: the flat one-thread-per-element form decoded its index with three 64-bit
// divisions -- ~150 instructions around five 32-byte memory operations; a row-per-workgroup loop was slower still: fewer loads in flight).
template <typename T>
__global__ __launch_bounds__(256) void upsample_bilinear2x_kernel(TensorRef src, TensorRef dst, float mul, float sy, float sx, unsigned* flag, unsigned layer_id) {
    // sy, sx = (in - 1) / (out - 1) as float divisions done ONCE on the host (the same IEEE quotient torch's area_pixel_compute_scale
    // takes; per lane they were two software divisions, ~20 vector instructions)
    constexpr int GN = Grp<T>::N;
    const int y = blockIdx.y, n = blockIdx.z;
    const unsigned groups = (unsigned)(dst.C / GN);
    int y0, y1;
    float ly1;
    bilinear_axis(sy, y, src.H, y0, y1, ly1);
    const float ly0 = 1.f - ly1;
    const size_t row0 = pix_index(src, n, y0, 0), row1 = pix_index(src, n, y1, 0), orow = pix_index(dst, n, y, 0);
    float bad = 0.f;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (unsigned)dst.W * groups) {
        const unsigned x = idx / groups, g = idx - x * groups;
        int x0, x1;
        float lx1;
        bilinear_axis(sx, (int)x, src.W, x0, x1, lx1);
        const float lx0 = 1.f - lx1;
        if constexpr (__is_same(T, split_t)) {
            unsigned t[4][8];
            upsample_split_load4(src, n, y0, y1, x0, x1, g, t);
            upsample_split_emit(dst, orow + x, g, t, ly0 * lx0 * mul, ly0 * lx1 * mul, ly1 * lx0 * mul, ly1 * lx1 * mul, bad);   // mul = 2^k: exact
        } else {
        float v00[GN], v01[GN], v10[GN], v11[GN], o[GN];
        int par;
        Grp<T>::load(grp_ptr<T>(src, row0 + x0, g, &par), par, v00);
        Grp<T>::load(grp_ptr<T>(src, row0 + x1, g, &par), par, v01);
        Grp<T>::load(grp_ptr<T>(src, row1 + x0, g, &par), par, v10);
        Grp<T>::load(grp_ptr<T>(src, row1 + x1, g, &par), par, v11);
#pragma unroll
        for (int j = 0; j < GN; ++j)
            o[j] = (ly0 * (lx0 * v00[j] + lx1 * v01[j]) + ly1 * (lx0 * v10[j] + lx1 * v11[j])) * mul;   // mul = 2^k: exact
        Grp<T>::store(grp_ptr<T>(dst, orow + x, g, &par), par, o, bad);
        }
    }
    report_bad(flag, layer_id, bad);
}

// split-f16, 2 x 2 OUTPUT pixels per lane (round 5).  With align_corners=True and an exact factor of two the output rows 2k - 1 and 2k
// blend the SAME two source rows (k - 1, k) -- likewise the columns -- so a lane that owns the block {2k - 1, 2k} x {2j - 1, 2j} loads
// four source pixels (8 x 16 bytes) for four outputs instead of 32 x 16 bytes: the one-output-per-lane kernel above moved its bytes
// at 0.44 of the HBM rate on tap loads through L1, not on arithmetic.  Each output leaves through that kernel's own tail
// (upsample_split_emit, with weights formed by the same expression), so both kernels produce the same bits; a block whose rows or
// columns do NOT share their source pair (never for a factor of two; checked, not assumed: the indices come from the same float
// products torch forms) falls back to that order with its own loads.  Grid = (segments of (W_in + 1) x groups, H_in + 1, images).
__global__ __launch_bounds__(256) void upsample_bilinear2x_split2x2_kernel(TensorRef src, TensorRef dst, float mul, float sy, float sx,
                                                                           unsigned* flag, unsigned layer_id) {
    const int k = blockIdx.y, n = blockIdx.z;
    const unsigned groups = (unsigned)(dst.C / 8);
    float bad = 0.f;
    // the block's two output rows (wave-uniform): source pair and weights of each, from torch's float products
    int ry[2] = {2 * k - 1, 2 * k}, y0[2], y1[2];
    float ly1[2];
    bool rv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        rv[r] = ry[r] >= 0 && ry[r] < dst.H;
        bilinear_axis(sy, rv[r] ? ry[r] : 0, src.H, y0[r], y1[r], ly1[r]);
    }
    const int rbase = rv[0] ? 0 : 1;                          // the row whose source pair the lane loads
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (unsigned)(src.W + 1) * groups) {
        const unsigned j = idx / groups, g = idx - j * groups;
        int cx[2] = {2 * (int)j - 1, 2 * (int)j}, x0[2], x1[2];
        float lx1[2];
        bool cv_[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            cv_[c] = cx[c] >= 0 && cx[c] < dst.W;
            bilinear_axis(sx, cv_[c] ? cx[c] : 0, src.W, x0[c], x1[c], lx1[c]);
        }
        const int cbase = cv_[0] ? 0 : 1;
        unsigned t[4][8];
        upsample_split_load4(src, n, y0[rbase], y1[rbase], x0[cbase], x1[cbase], g, t);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (!rv[r]) continue;
            const bool rows_shared = y0[r] == y0[rbase] && y1[r] == y1[rbase];
            const float ly0 = 1.f - ly1[r];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (!cv_[c]) continue;
                const float lx0 = 1.f - lx1[c];
                const float w00 = ly0 * lx0 * mul, w01 = ly0 * lx1[c] * mul, w10 = ly1[r] * lx0 * mul, w11 = ly1[r] * lx1[c] * mul;   // mul = 2^k: exact
                const size_t opix = pix_index(dst, n, ry[r], cx[c]);
                if (rows_shared && x0[c] == x0[cbase] && x1[c] == x1[cbase]) {
                    upsample_split_emit(dst, opix, g, t, w00, w01, w10, w11, bad);
                } else {                                      // not reached for a factor of two; kept so that the kernel is exact for any geometry
                    unsigned u[4][8];
                    upsample_split_load4(src, n, y0[r], y1[r], x0[c], x1[c], g, u);
                    upsample_split_emit(dst, opix, g, u, w00, w01, w10, w11, bad);
                }
            }
        }
    }
    report_bad(flag, layer_id, bad);
}

// ---- OutConv 1x1 (C -> 1) + bias, fused sigmoid/threshold mask ------------------------------------
// C/N lanes share one pixel (one group each); xor-shuffle reduce inside the lane group.
template <typename T>
__global__ void outc_1x1_kernel(TensorRef src, const float* __restrict__ w, const float* __restrict__ bias, float mul,
                                float* __restrict__ logits, uint8_t* __restrict__ mask, float thr, unsigned* flag,
                                unsigned layer_id) {
    constexpr int GN = Grp<T>::N;
    const int lpp = src.C / GN;                               // power of two, <= 64
    const size_t npix = (size_t)src.N * src.H * src.W;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int part = (int)(idx % lpp);
    size_t pix = idx / lpp;
    const bool live = pix < npix;
    if (!live) pix = npix - 1;
    const Pix p = decode_pix(src, pix);
    float v[GN];
    int par;
    Grp<T>::load(grp_ptr<T>(src, pix_index(src, p.n, p.y, p.x), part, &par), par, v);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < GN; ++j) acc += v[j] * w[part * GN + j];
    for (int m = 1; m < lpp; m <<= 1) acc += __shfl_xor(acc, m);
    if (live && part == 0) {
        const float l = acc * mul + bias[0];
        logits[pix] = l;
        if (mask) mask[pix] = (1.f / (1.f + __expf(-l))) > thr ? 255 : 0;
        report_bad(flag, layer_id, l * 0.f);
    }
}

// ---- ResNet stem: conv 7x7 s2 p3, 1 -> 64, + BN affine + ReLU -------------------------------------
// One workgroup per 64x64 square.  The zero-bordered plane sits in LDS; each lane owns one output pixel at
// a time, holds its 7x7 patch in VGPRs and runs the 64x49 filter bank from the scalar cache (wave-uniform
// weights -> s_load + v_fma with an SGPR operand), i.e. a pure VALU f32 kernel.
// NORM (byte input only): the stored pixel is ((float)u8 / 255 - mean) / std, ToTensor + Normalize in torch's float32 arithmetic
// (two true divisions and a subtraction, in that order); the zero border stays zero, as torch pads after normalising.
template <typename T, typename XT, bool NORM = false>
__global__ __launch_bounds__(256) void stem7x7_kernel(const XT* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ shift, TensorRef dst, InputNorm norm) {
    constexpr int IN = 64, P = 3, LD = IN + 2 * P;            // 70
    constexpr int GN = Grp<T>::N;
    __shared__ float plane[LD * LD];
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < LD * LD; i += 256) plane[i] = 0.f;
    __syncthreads();
    const XT* xs = x + (size_t)n * IN * IN;
    for (int i = tid; i < IN * IN; i += 256) {
        float v = (float)xs[i];
        if (sizeof(XT) == 1) v = v / 255.f;
        if (NORM) v = (v - norm.mean) / norm.std;
        plane[(i / IN + P) * LD + (i % IN) + P] = v;
    }
    __syncthreads();
    constexpr int OUT = 32;
    for (int it = 0; it < OUT * OUT / 256; ++it) {
        const int pid = it * 256 + tid;
        const int oy = pid / OUT, ox = pid % OUT;
        float patch[49];
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) patch[ky * 7 + kx] = plane[(2 * oy + ky) * LD + 2 * ox + kx];
        const size_t opix = pix_index(dst, n, oy, ox);
        // 8 output channels per trip: 392 wave-uniform weights stream through SGPRs, results leave as
        // 16-B stores.  Not unrolled on purpose: keeps the scalar loads inside the loop (no LICM hoist).
#pragma unroll 1
        for (int cb = 0; cb < 64; cb += 8) {
            const float* wc = w + cb * 49;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < 49; ++k) a = __builtin_fmaf(patch[k], wc[c * 49 + k], a);
                a = a * scale[cb + c] + shift[cb + c];
                v[c] = a > 0.f ? a : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; i += GN) {
                int par;
                char* d = grp_ptr<T>(dst, opix, (cb + i) / GN, &par);
                Grp<T>::store(d, par, v + i);
            }
        }
    }
}

// ---- ResNet stem on the matrix cores, fused with the 3x3/s2/p1 max-pool (f16 and split-f16 engines) ----------
// conv 7x7 s2 p3 (1 -> 64) + BN + ReLU + max_pool2d(3, 2, 1):  (n,1,64,64) -> 64 ch @ 16x16, one pass, nothing but the
// pooled result leaves the CU.  GEMM view per square: D[ch][pix] = sum_k W[ch][k] * patch[pix][k], K = 7 rows x 8
// (kx padded 7 -> 8, ky padded 7 -> 8) = 64 = two 16x16x32 MFMA k-steps; lane group q of k-step ks owns filter row
// ky = 4*ks + q, whose 8 taps are 4 consecutive LDS dwords of the zero-bordered input plane -> the B fragment is four
// ds_read_b32, no packing.  One 16-lane pixel fragment = one pooled output row; the 9 pool-window positions are
// computed one after the other (2.25x recompute of the tiny conv instead of staging 32x32x64 outputs in LDS) and
// max-reduced in registers.  Out-of-range window positions contribute 0, which equals -inf padding after ReLU.
// SPLIT = split-f16 ARITHMETIC (hi + lo planes, three products); it is what a split_t tensor implies, and the f16r engine asks
// for it with T = half_t: its stem computes at f32 grade and leaves the pooled result twice, as the f16 tensor layer1.0.conv1
// consumes and as the f32 twin (dst.base32) the residual trunk starts from.
// NORM: the normalised byte input of stem7x7_kernel; |value| <= 2.30 for the training constants, times 2^7 well inside f16.
template <typename T, typename XT, bool SPLIT = sizeof(T) == 4, bool NORM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void stem_pool_mfma_kernel(const XT* __restrict__ x, int n,
                                                             const half8* __restrict__ wpk,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float in_mul, TensorRef dst,
                                                             unsigned* flag, unsigned layer_id, InputNorm norm) {
    constexpr int LD = 98, ROWS = 72, PAD = 5;              // LD/2 = 49 dwords: odd rows land on the other bank half
    constexpr int NPL = SPLIT ? 2 : 1;                      // hi (+ lo) plane
    // two sets of planes: square n+1 is fetched into registers before square n is computed and written to the other set after it,
    // so the global-load latency and the conversion pass hide behind the MFMA phase and one barrier per square is left (r03:
    // 42 % of the wave cycles were waits with a single set)
    __shared__ __attribute__((aligned(16))) half_t plane[2][NPL][ROWS * LD];
    __shared__ __attribute__((aligned(16))) char stage[4][16 * 272];      // one pooled row per wave on its way out (see the stores below)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, l15 = lane & 15;

    half8 ah[2][4], al[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            ah[ks][f] = wpk[((0 * 2 + ks) * 4 + f) * 64 + lane];
            al[ks][f] = SPLIT ? wpk[((1 * 2 + ks) * 4 + f) * 64 + lane] : ah[ks][f];
        }
    float sc[16], sh[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { sc[i] = scale[q * 16 + i]; sh[i] = shift[q * 16 + i]; }

    for (int i = tid; i < 2 * NPL * ROWS * LD; i += 256) (&plane[0][0][0])[i] = (half_t)0.f;

    XT pre[16];                                              // this thread's 16 pixels of the NEXT square
    auto fetch = [&](int sq) __attribute__((always_inline)) {
        const XT* xs = x + (size_t)sq * 4096;
#pragma unroll
        for (int k = 0; k < 16; ++k) pre[k] = xs[tid + 256 * k];
    };
    auto deposit = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = tid + 256 * k;
            float v = (float)pre[k];
            if (sizeof(XT) == 1) v = v / 255.f;
            if (NORM) v = (v - norm.mean) / norm.std;    // ToTensor + Normalize, bit for bit
            v *= in_mul;                                     // power-of-two range factor of the input plane (exact)
            const half_t hi = (half_t)v;
            const int at = ((i >> 6) + PAD) * LD + (i & 63) + PAD;
            plane[buf][0][at] = hi;
            if (SPLIT) plane[buf][NPL - 1][at] = (half_t)(v - (float)hi);
        }
    };
    float bad = 0.f;
    int buf = 0;
    if ((int)blockIdx.x < n) fetch(blockIdx.x);
    __syncthreads();                                         // the zero fill is complete
    if ((int)blockIdx.x < n) deposit(0);
    __syncthreads();
    for (int sq = blockIdx.x; sq < n; sq += gridDim.x, buf ^= 1) {
        const int nxt = sq + gridDim.x;
        if (nxt < n) fetch(nxt);                             // in flight during this square's MFMA phase
        const unsigned* p32h = reinterpret_cast<const unsigned*>(&plane[buf][0][0]);
        const unsigned* p32l = reinterpret_cast<const unsigned*>(&plane[buf][NPL - 1][0]);
        // Each wave owns four consecutive pooled rows = conv-output rows 8w-1 .. 8w+7.  A conv row is computed ONCE, as its
        // even-column and odd-column fragments (lane l15 <-> columns 2*l15 and 2*l15+1); the third pool-window column
        // (2*l15-1) is the odd fragment shifted by one lane (DPP row_shr:1, zero fill = the window's left padding), and the
        // conv row shared by two vertically adjacent windows is carried in registers: 9 x 2 fragment computations per four
        // pooled rows instead of the 4 x 9 of a window-by-window walk (r01).  Out-of-range rows / columns contribute 0, which
        // equals -inf padding after ReLU.
        auto conv_row_max = [&](int cy, float* hm) __attribute__((always_inline)) {   // max over the three window columns: 16 channels per lane
            float ev[16], od[16];
#pragma unroll
            for (int par = 0; par < 2; ++par) {
                f4 acc[4];
#pragma unroll
                for (int f = 0; f < 4; ++f) acc[f] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int row = 2 * cy + 2 + ks * 4 + q;                   // plane row of filter row ky = 4*ks+q
                    const int dw = (row * LD + 2 * (2 * l15 + par) + 2) >> 1;  // conv column 2*l15 + par
                    union { unsigned u[4]; half8 h; } bh, bl;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { bh.u[j] = p32h[dw + j]; bl.u[j] = SPLIT ? p32l[dw + j] : 0u; }
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks][f], bh.h, acc[f], 0, 0, 0);
                        if (SPLIT) {
                            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[ks][f], bh.h, acc[f], 0, 0, 0);
                            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks][f], bl.h, acc[f], 0, 0, 0);
                        }
                    }
                }
                typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int f = 0; f < 4; ++f)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        // BN affine only: max_pool(relu(x)) == relu(max_pool(x)), and the zero that stands for the pool's padding is
                        // harmless inside a maximum that is clamped at zero afterwards -- one ReLU per pooled value instead of one per
                        // conv value (2.25x fewer).  Two values per v_pk_fma_f32.
                        const f2 a = {acc[f][r], acc[f][r + 1]}, m = {sc[f * 4 + r], sc[f * 4 + r + 1]}, b = {sh[f * 4 + r], sh[f * 4 + r + 1]};
                        const f2 v = __builtin_elementwise_fma(a, m, b);
                        if (par == 0) { ev[f * 4 + r] = v[0]; ev[f * 4 + r + 1] = v[1]; } else { od[f * 4 + r] = v[0]; od[f * 4 + r + 1] = v[1]; }
                    }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float left = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(od[i]), 0x111, 0xf, 0xf, true));   // od of lane - 1
                hm[i] = __builtin_fmaxf(__builtin_fmaxf(ev[i], od[i]), left);
            }
        };
        float carry[16];
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) carry[i] = 0.f;                       // conv row -1: padding
        } else {
            conv_row_max(8 * wave - 1, carry);
        }
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int py = 4 * wave + j;
            float mid[16], low[16], best[16];
            conv_row_max(2 * py, mid);
            conv_row_max(2 * py + 1, low);
#pragma unroll
            for (int i = 0; i < 16; ++i) { best[i] = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(carry[i], mid[i]), low[i]), 0.f); carry[i] = low[i]; }
            // A pooled row of the square = 16 pixels x 64 channels = ONE contiguous run in memory (2-4 KB; the launcher checks that the
            // tensor holds exactly the stem's 64 channels).  The MFMA leaves a lane with 16 channels of one pixel, i.e. 64 scattered
            // 16-byte pieces per store instruction; through the wave's LDS corner the run leaves as 1 KB per instruction in full lines
            // (r05_tuning.md section 15).  Wave-private staging: DS operations of a wave execute in order.  The split-f16 instantiation keeps
            // its direct stores: there the staging costs 10-12 spilled registers and the kernel is bound by its matrix work anyway.
            const size_t opix = pix_index(dst, sq, py, l15);
            if constexpr (!__is_same(T, half_t)) {
#pragma unroll
                for (int i = 0; i < 16; i += Grp<T>::N) {
                    int par;
                    char* d = grp_ptr<T>(dst, opix, (q * 16 + i) / Grp<T>::N, &par);
                    Grp<T>::store(d, par, best + i, bad);
                }
            } else {
                constexpr int ESZ = Grp<T>::BYTES / Grp<T>::N, PB = 64 * ESZ, SRA = PB + 16;
                typedef unsigned u4 __attribute__((ext_vector_type(4)));
                char* const stg = &stage[wave][0];
#pragma unroll
                for (int i = 0; i < 16; i += Grp<T>::N)
                    Grp<T>::store(stg + l15 * SRA + (q * 16 + i) * ESZ, ((q * 16 + i) / Grp<T>::N) & 1, best + i, bad);
                wave_lds_sync();
                char* const grow = reinterpret_cast<char*>(dst.base) + pix_index(dst, sq, py, 0) * (size_t)PB;
#pragma unroll
                for (int t = 0; t < 16 * PB / 1024; ++t) {
                    const int o = t * 1024 + lane * 16;
                    *reinterpret_cast<u4*>(grow + o) = *reinterpret_cast<const u4*>(stg + (o / PB) * SRA + (o % PB));
                }
                wave_lds_sync();
                if constexpr (__is_same(T, half_t) && SPLIT) {
                    if (dst.base32) {
#pragma unroll
                        for (int i = 0; i < 16; i += 4)
                            *reinterpret_cast<f4*>(stg + l15 * 272 + (q * 16 + i) * 4) = f4{best[i], best[i + 1], best[i + 2], best[i + 3]};
                        wave_lds_sync();
                        char* const grow32 = reinterpret_cast<char*>(dst.base32) + pix_index(dst, sq, py, 0) * (size_t)256;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int o = t * 1024 + lane * 16;
                            *reinterpret_cast<u4*>(grow32 + o) = *reinterpret_cast<const u4*>(stg + (o / 256) * 272 + (o % 256));
                        }
                        wave_lds_sync();
                    }
                }
            }
        }
        if (nxt < n) deposit(buf ^ 1);                       // the other set: nobody reads it during this square
        __syncthreads();                                     // next square's planes visible; every read of this square's set done
    }
    report_bad(flag, layer_id, bad);
}


// ---- UNet first layer on the matrix cores, straight from the caller's image ---------------------------------------
// inc.double_conv.0: conv 3x3 p1 (3 -> 64) + BN + ReLU, fused with the input packing (u8 HWC / 255 or f32 NCHW -> internal
// layout).  The layer is 0.2 % of the network's MACs but writes 16.8 MB per image: it is bound by that store stream, and the
// generic implicit-GEMM kernel (three 128-byte K stages over an 8-channel padded copy of the image, one 128-pixel tile per
// workgroup) spent its time in per-workgroup prologues instead.  Here K = 3 x 3 x 3 = 27 -> 32 = ONE 16x16x32 MFMA k-step
// (x3 products for split-f16); a workgroup owns an 8-row band of one image, keeps the 10 x 258 x 3 input patch in LDS as
// f32, and every wave walks 2 rows x 16 fragments: eight ds_read_b32 build the B fragment (lane group q holds k = 8q..8q+7,
// k = (ky*3 + kx)*3 + c), 4 x (1 | 3) MFMAs give the lane 16 consecutive channels of its pixel, and the wave-private LDS
// transpose of conv_igemm.hip turns them into 2 KB-contiguous stores.  The 8-channel padded input tensor and its packing
// kernel disappear.
template <typename T, typename XT>
__global__ __launch_bounds__(256) void inc0_mfma_kernel(const XT* __restrict__ x, const half8* __restrict__ wpk,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float in_mul, TensorRef dst, unsigned* flag, unsigned layer_id) {
    constexpr bool SPLIT = sizeof(T) == 4;
    constexpr int W = 256, BAND = 8, PR = BAND + 2, PW = 260;      // patch rows / row pitch (floats): cols -1..256 + pad
    constexpr int SROW = 272;                                        // staging row pitch (bytes), as conv_igemm.hip
    __shared__ __attribute__((aligned(16))) float patch[3 * PR * PW + 4];
    __shared__ __attribute__((aligned(16))) char stage_mem[4 * 16 * SROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, l15 = lane & 15;
    const int n = blockIdx.x / (W / BAND), band = blockIdx.x % (W / BAND);
    const int y0 = band * BAND;

    // ---- input patch: rows y0-1 .. y0+8, all 256 columns, 3 channels; zero outside the image -------------------------
    float bad = 0.f;
    if (tid < 4) patch[3 * PR * PW + tid] = 0.f;                      // the zero slot the padded k indices read
    for (int i = tid; i < 3 * PR; i += 256) { patch[i * PW] = 0.f; patch[i * PW + W + 1] = 0.f; }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < PR; ++r) {
            const int gy = y0 - 1 + r;
            float v = 0.f;
            if (gy >= 0 && gy < W) {
                if (sizeof(XT) == 1) v = (float)x[((size_t)(n * W + gy) * W + tid) * 3 + c] / 255.f;
                else v = (float)x[((size_t)(n * 3 + c) * W + gy) * W + tid];
            }
            bad = __builtin_fmaf(v, 0.f, bad);
            patch[(c * PR + r) * PW + tid + 1] = v * in_mul;
        }
    report_bad(flag, 0u, bad);                                       // layer id 0 = the caller's input tensor

    // ---- per-lane constants ---------------------------------------------------------------------------------------------
    half8 ah[4], al[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        ah[f] = wpk[(0 * 4 + f) * 64 + lane];
        al[f] = SPLIT ? wpk[(1 * 4 + f) * 64 + lane] : ah[f];
    }
    float sc[16], sh[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { sc[i] = scale[q * 16 + i]; sh[i] = shift[q * 16 + i]; }
    int koff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = q * 8 + j;
        const int tap = k / 3, c = k - tap * 3, ky = tap / 3, kx = tap - ky * 3;
        koff[j] = k < 27 ? (c * PR + ky) * PW + kx : 3 * PR * PW;   // (float index relative to the pixel's patch origin) | zero slot
    }
    __syncthreads();

    char* const stg = stage_mem + wave * (16 * SROW);
    float out_bad = 0.f;
    for (int it = 0; it < 2 * (W / 16); ++it) {
        const int r = wave * 2 + it / (W / 16), cb = it % (W / 16);   // row of the band, 16-pixel block of the row
        const int pbase = r * PW + cb * 16 + l15;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = patch[(q * 8 + j < 27 ? pbase : 0) + koff[j]];
        half8 bh, bl;
#pragma unroll
        for (int j = 0; j < 8; ++j) { bh[j] = (half_t)v[j]; bl[j] = (half_t)(v[j] - (float)bh[j]); }
        f4 acc[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[f], bh, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            if (SPLIT) {
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[f], bh, acc[f], 0, 0, 0);
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[f], bl, acc[f], 0, 0, 0);
            }
        }
        // BN + ReLU, then the wave-private transpose: lane (pixel l15, group q) holds 16 consecutive channels
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            f4 t;
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = __builtin_fmaxf(acc[f][k] * sc[f * 4 + k] + sh[f * 4 + k], 0.f);
            *reinterpret_cast<f4*>(stg + l15 * SROW + (q * 16 + f * 4) * 4) = t;
        }
        wave_lds_sync();
        const size_t row_pix = pix_index(dst, n, y0 + r, cb * 16);
#pragma unroll
        for (int i = 0; i < 2; ++i) {                                  // 16 px x 8 groups of 8 channels = 128 units
            const int unit = lane + 64 * i, px = unit >> 3, g = unit & 7;
            float w[8];
#pragma unroll
            for (int j = 0; j < 8; j += 4) {
                const f4 t = *reinterpret_cast<const f4*>(stg + px * SROW + (g * 8 + j) * 4);
                w[j] = t[0]; w[j + 1] = t[1]; w[j + 2] = t[2]; w[j + 3] = t[3];
            }
            int par;
            char* d = grp_ptr<T>(dst, row_pix + px, g, &par);
            Grp<T>::store(d, par, w, out_bad);
        }
        wave_lds_sync();
    }
    report_bad(flag, layer_id, out_bad);
}

// ---- head: adaptive_avg_pool2d(1) + Linear(512 -> 13) (+ softmax) ----------------------------------
// Persistent waves, one square at a time.  Lane l always owns channels 8l .. 8l+7, so its 13 x 8 fc weights are loaded ONCE
// into registers and reused for every square the wave walks (r01 re-read them from L2 for each square: 104 vector loads per
// wave and square, which -- not the 2 KB of activations -- set the kernel's time).  Per square: 32-byte loads of the lane's
// channels at each pixel, 104 FMAs, then the 13 partial sums are reduced across the 64 lanes by a halving butterfly (each step
// exchanges half of the live values with the partner lane: 7 + 4 + 2 + 1 shuffles, then 2 for the last four lanes) instead of
// 13 full butterflies (78 shuffles); soft-max runs across the 13 lanes that end up holding one logit each.
template <typename T>
__global__ __launch_bounds__(256) void head_kernel(TensorRef src, const float* __restrict__ w,
                                                   const float* __restrict__ b, float mul, float* __restrict__ out,
                                                   int softmax, unsigned* flag, unsigned layer_id) {
    constexpr int NC = 13;
    constexpr int GN = Grp<T>::N, GPL = 8 / GN;              // groups per lane: 1 (f16, split-f16) or 2 (f32)
    const int lane = threadIdx.x & 63;
    const int wave0 = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    float wr[NC][8];
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
        for (int j = 0; j < 8; j += 4) {
            const f4 t = *reinterpret_cast<const f4*>(w + k * 512 + lane * 8 + j);
            wr[k][j] = t[0]; wr[k][j + 1] = t[1]; wr[k][j + 2] = t[2]; wr[k][j + 3] = t[3];
        }
    // which logit this lane holds after the halving butterfly, and its bias
    const int b5 = (lane >> 5) & 1, b4 = (lane >> 4) & 1, b3 = (lane >> 3) & 1, b2 = (lane >> 2) & 1;
    const int slot = b4 * 4 + b3 * 2 + b2;
    const bool holds = b5 ? slot < 6 : slot < 7;
    const int cls = b5 * 7 + slot;
    const float bias = holds ? b[cls] : 0.f;
    const float inv = mul / (float)(src.H * src.W);           // mul = 2^exp of the stored tensor (exact)
    float bad = 0.f;
    for (int n = wave0; n < src.N; n += nwaves) {
        float s8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s8[j] = 0.f;
        for (int y = 0; y < src.H; ++y)
            for (int x = 0; x < src.W; ++x) {
                const size_t pix = pix_index(src, n, y, x);
#pragma unroll
                for (int g = 0; g < GPL; ++g) {
                    int par;
                    float v[GN];
                    Grp<T>::load(grp_ptr<T>(src, pix, lane * GPL + g, &par), par, v);
#pragma unroll
                    for (int j = 0; j < GN; ++j) s8[g * GN + j] += v[j];
                }
            }
        float acc[NC + 1];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) a = __builtin_fmaf(s8[j] * inv, wr[k][j], a);
            acc[k] = a;
        }
        acc[NC] = 0.f;
        // halving butterfly: 14 -> 7 -> 4 -> 2 -> 1 live values, the upper lane of each pair keeps the upper half
        float v7[8];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const float r = __shfl_xor(b5 ? acc[i] : acc[7 + i], 32);
            v7[i] = (b5 ? acc[7 + i] : acc[i]) + r;
        }
        v7[7] = 0.f;
        float v4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float r = __shfl_xor(b4 ? v7[i] : v7[4 + i], 16);
            v4[i] = (b4 ? v7[4 + i] : v7[i]) + r;
        }
        float v2[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float r = __shfl_xor(b3 ? v4[i] : v4[2 + i], 8);
            v2[i] = (b3 ? v4[2 + i] : v4[i]) + r;
        }
        float v = (b2 ? v2[1] : v2[0]) + __shfl_xor(b2 ? v2[0] : v2[1], 4);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 1);
        v += bias;
        if (holds) bad = __builtin_fmaf(v, 0.f, bad);
        if (softmax) {
            float mx = holds ? v : -INFINITY;
#pragma unroll
            for (int m = 32; m >= 4; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
            const float e = holds ? __expf(v - mx) : 0.f;
            float sum = e;
#pragma unroll
            for (int m = 32; m >= 4; m >>= 1) sum += __shfl_xor(sum, m);
            v = e / sum;
        }
        if (holds && (lane & 3) == 0) out[(size_t)n * NC + cls] = v;
    }
    report_bad(flag, layer_id, bad);
}

// ---- YOLOv8-cls stem: conv 3x3 s2 p1, 1 -> C0 (16 .. 80), + BN affine + SiLU ----------------------------------
// stem7x7_kernel's scheme on a 3x3 filter: one workgroup per 64x64 square, the zero-bordered plane in LDS, each lane one output pixel
// at a time with its 9-pixel patch in registers, the C0 x 9 filter bank wave-uniform through the scalar cache; float32 throughout, in
// every engine (the stem holds under 1 % of the smallest scale's MACs).  The three input channels of the checkpoint see the same plane
// (the reference repeats it), so the loader has summed their filters: one channel here.  `mul` = 2^-exp of the stored output, applied
// AFTER the SiLU (cv_kernels.h: silu_f32).  NORM as in stem7x7_kernel.
template <typename T, typename XT, bool NORM = false>
__global__ __launch_bounds__(256) void stem3x3s2_kernel(const XT* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        TensorRef dst, float mul, InputNorm norm, unsigned* flag, unsigned layer_id) {
    constexpr int IN = 64, LD = IN + 2, OUT = 32;
    constexpr int GN = Grp<T>::N;
    __shared__ float plane[LD * LD];
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < LD * LD; i += 256) plane[i] = 0.f;
    __syncthreads();
    const XT* xs = x + (size_t)n * IN * IN;
    for (int i = tid; i < IN * IN; i += 256) {
        float v = (float)xs[i];
        if (sizeof(XT) == 1) v = v / 255.f;
        if (NORM) v = (v - norm.mean) / norm.std;
        plane[(i / IN + 1) * LD + (i % IN) + 1] = v;
    }
    __syncthreads();
    float bad = 0.f;
    for (int it = 0; it < OUT * OUT / 256; ++it) {
        const int pid = it * 256 + tid;
        const int oy = pid / OUT, ox = pid % OUT;
        float patch[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) patch[ky * 3 + kx] = plane[(2 * oy + ky) * LD + 2 * ox + kx];
        const size_t opix = pix_index(dst, n, oy, ox);
#pragma unroll 1
        for (int cb = 0; cb < dst.C; cb += 8) {          // dst.C is a multiple of 8 (checked by the wrapper)
            const float* wc = w + cb * 9;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < 9; ++k) a = __builtin_fmaf(patch[k], wc[c * 9 + k], a);
                a = a * scale[cb + c] + shift[cb + c];
                v[c] = silu_f32(a) * mul;
            }
#pragma unroll
            for (int i = 0; i < 8; i += GN) {
                int par;
                char* d = grp_ptr<T>(dst, opix, (cb + i) / GN, &par);
                Grp<T>::store(d, par, v + i, bad);
            }
        }
    }
    report_bad(flag, layer_id, bad);
}

// ---- YOLOv8-cls head: adaptive_avg_pool2d(1) + Linear(C -> 13) (+ softmax) (+ the pooled features) ------------------------------
// head_kernel generalised to any C that is a multiple of 8 (C = 1280: 20 channels per lane, whose 13 x 20 weights do not fit in
// registers as the 13 x 8 of the 512-channel form do).  One wave walks kHeadQ squares at a time: for each of its channel groups
// (group = lane, lane + 64, ...) it loads the 13 x GN weights once and uses them for the kHeadQ squares, so the weights cross L2 ->
// CU once per kHeadQ squares.  Per square and channel: the H x W values summed in raster order, mean = sum * mul / (H W), 13 FMAs in
// channel order; the 64 lanes' partial sums meet in a xor butterfly (every lane ends with every logit).  A square's arithmetic does not
// depend on its place in the batch.  pooled (nullable): the means, (n, C) float32 -- the input of the linear layer.
constexpr int kHeadQ = 4;
template <typename T>
__global__ __launch_bounds__(256) void head_pool_fc_kernel(TensorRef src, const float* __restrict__ w, const float* __restrict__ b,
                                                           float mul, float* __restrict__ out, float* __restrict__ pooled, int softmax,
                                                           unsigned* flag, unsigned layer_id) {
    constexpr int NC = 13;
    constexpr int GN = Grp<T>::N;
    const int lane = threadIdx.x & 63;
    const int wave0 = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const int groups = src.C / GN;
    const float inv = mul / (float)(src.H * src.W);
    float bad = 0.f;
    for (int n0 = wave0 * kHeadQ; n0 < src.N; n0 += nwaves * kHeadQ) {
        float acc[kHeadQ][NC];
#pragma unroll
        for (int q = 0; q < kHeadQ; ++q)
#pragma unroll
            for (int k = 0; k < NC; ++k) acc[q][k] = 0.f;
        for (int g = lane; g < groups; g += 64) {
            float wr[NC][GN];
#pragma unroll
            for (int k = 0; k < NC; ++k)
#pragma unroll
                for (int j = 0; j < GN; j += 4) {
                    const f4 t = *reinterpret_cast<const f4*>(w + (size_t)k * src.C + g * GN + j);
                    wr[k][j] = t[0]; wr[k][j + 1] = t[1]; wr[k][j + 2] = t[2]; wr[k][j + 3] = t[3];
                }
#pragma unroll
            for (int q = 0; q < kHeadQ; ++q) {
                const int n = n0 + q;
                if (n >= src.N) break;                       // wave-uniform
                float sum[GN];
#pragma unroll
                for (int j = 0; j < GN; ++j) sum[j] = 0.f;
                for (int y = 0; y < src.H; ++y)
                    for (int xx = 0; xx < src.W; ++xx) {
                        int par;
                        float v[GN];
                        Grp<T>::load(grp_ptr<T>(src, pix_index(src, n, y, xx), g, &par), par, v);
#pragma unroll
                        for (int j = 0; j < GN; ++j) sum[j] += v[j];
                    }
#pragma unroll
                for (int j = 0; j < GN; ++j) sum[j] *= inv;
                if (pooled) {
#pragma unroll
                    for (int j = 0; j < GN; j += 4)
                        *reinterpret_cast<f4*>(pooled + (size_t)n * src.C + g * GN + j) = f4{sum[j], sum[j + 1], sum[j + 2], sum[j + 3]};
                }
#pragma unroll
                for (int k = 0; k < NC; ++k)
#pragma unroll
                    for (int j = 0; j < GN; ++j) acc[q][k] = __builtin_fmaf(sum[j], wr[k][j], acc[q][k]);
            }
        }
#pragma unroll
        for (int q = 0; q < kHeadQ; ++q) {
            const int n = n0 + q;
            if (n >= src.N) break;
            float mine = 0.f, mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                float v = acc[q][k];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
                v += b[k];
                acc[q][k] = v;
                mx = fmaxf(mx, v);
                if (lane == k) mine = v;
            }
            if (lane < NC) bad = __builtin_fmaf(mine, 0.f, bad);
            if (softmax) {
                float sum = 0.f, e_mine = 0.f;
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const float e = __expf(acc[q][k] - mx);
                    sum += e;
                    if (lane == k) e_mine = e;
                }
                mine = e_mine / sum;
            }
            if (lane < NC) out[(size_t)n * NC + lane] = mine;
        }
    }
    report_bad(flag, layer_id, bad);
}

__global__ void softmax13_kernel(const float* __restrict__ logits, int n, float* __restrict__ probs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[13];
    float mx = -3.4e38f;
#pragma unroll
    for (int j = 0; j < 13; ++j) { v[j] = logits[(size_t)i * 13 + j]; mx = fmaxf(mx, v[j]); }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 13; ++j) { v[j] = __expf(v[j] - mx); s += v[j]; }
    const float r = 1.f / s;
#pragma unroll
    for (int j = 0; j < 13; ++j) probs[(size_t)i * 13 + j] = v[j] * r;
}

// ---- per-square records of the classifier's validation pass ------------------------------------------------------------------------
// One thread per row of 13 logits (52 B in, 32 B out: the launch is bandwidth- and latency-bound, there is nothing to share between
// rows).  Every comparison is of the float32 logits themselves, so the integer fields equal a host restatement bit for bit; the sums
// run in ascending class order with expf / logf.  The grid-stride loop takes any n in one launch.
__global__ __launch_bounds__(256) void square_records_kernel(const float* __restrict__ logits, const int8_t* __restrict__ labels, int n,
                                                             SquareRecord* __restrict__ records) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += step) {
        float x[13];
        bool nan = false;
#pragma unroll
        for (int j = 0; j < 13; ++j) { x[j] = logits[i * 13 + j]; nan = nan || x[j] != x[j]; }
        int pred = 0;
        float m = x[0];
#pragma unroll
        for (int j = 1; j < 13; ++j)
            if (x[j] > m) { m = x[j]; pred = j; }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 13; ++j) s += expf(x[j] - m);
        const float ls = logf(s);
        const int given = labels ? (int)labels[i] : -1;
        const bool bad = given < -1 || given > 12;           // cannot be refused without reading device memory: flagged, scored as unlabelled
        const int t = bad ? -1 : given;
        int rank = -1;
        float xt = 0.f;
        if (t >= 0) {
            rank = 0;
#pragma unroll
            for (int j = 0; j < 13; ++j)
                if (j == t) xt = x[j];
#pragma unroll
            for (int j = 0; j < 13; ++j) rank += (x[j] > xt || (j > t && x[j] == xt)) ? 1 : 0;
        }
        const float qnan = __int_as_float(0x7fc00000);
        SquareRecord r;
        r.predicted = pred;
        r.rank = t < 0 ? -1 : nan ? 13 : rank;
        r.label = given;
        r.flags = (nan ? 1 : 0) | (bad ? 2 : 0);
        r.confidence = nan ? qnan : 1.f / s;
        r.loss = (t < 0 || nan) ? qnan : ls - (xt - m);
        r.max_logit = nan ? qnan : m;
        r.logsumexp = nan ? qnan : m + ls;
        records[i] = r;
    }
}

// ---- board-extraction quality scores: per-image reductions over the UNet's logits ------------------------------------------------
// One workgroup of 16 waves per image.  Sweep 0 reads the image once for the ten-bin histogram, the `> 0.5` count and mask, the NaN
// count and the first radix histogram; three more sweeps narrow the k-th largest value (k = count / 4) eight key bits at a time, and
// a last one sums |v - 0.5| above it.  The image (256 KB at 256x256) does not fit LDS: sweeps 1..4 re-read it through L2.  Every
// count is an integer and the float64 sum runs in a fixed order (thread, wave shuffle, waves in order), so a record is bit-identical
// run to run.
constexpr int kScoreThreads = 1024, kScoreWaves = kScoreThreads / 64;

template <int N> struct ScoreInt { static constexpr int value = N; };

template <int TR> __device__ __forceinline__ float score_value(float x) {
    return TR ? 1.f / (1.f + __expf(-x)) : x;                 // the expression of outc_1x1_kernel's mask
}

// order-preserving key of a float (larger value <=> larger key); -0.0 shares +0.0's key
__device__ __forceinline__ unsigned score_key(float v) {
    const unsigned u = __float_as_uint(v);
    const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return k == 0x7fffffffu ? 0x80000000u : k;
}
__device__ __forceinline__ float score_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The frame the three score kernels share.  A workgroup's image: `count` float32 of which `head` (< 4) come before the first 16-byte
// boundary, then `nvec` 16-byte pieces (the body), then the rest.  A byte stream that runs beside the image (labels, masks, levels: one
// byte per element, any alignment) moves four bytes at a time over the body where it is 4-aligned there.
struct ScoreSpan {
    const float* img;
    int count, head, nvec;
    __device__ ScoreSpan(const float* images, int count_) : img(images + (size_t)blockIdx.x * count_), count(count_) {
        head = min(count, (int)(((16u - (unsigned)((uintptr_t)img & 15u)) & 15u) >> 2));
        nvec = (count - head) >> 2;
    }
    __device__ bool aligned4(const uint8_t* bytes) const { return (((uintptr_t)(bytes + head)) & 3u) == 0; }
};
// m bytes at bytes[at]: one 4-byte access for a body piece (m == 4) of an aligned4 stream, single bytes otherwise
template <int m> __device__ __forceinline__ void load_bytes(const uint8_t* bytes, int at, bool aligned, uint8_t (&v)[m]) {
    if constexpr (m == 4) {
        if (aligned) {
            const uchar4 q = *reinterpret_cast<const uchar4*>(bytes + at);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < m; ++j) v[j] = bytes[at + j];
}
template <int m> __device__ __forceinline__ void store_bytes(uint8_t* bytes, int at, bool aligned, const uint8_t (&v)[m]) {
    if constexpr (m == 4) {
        if (aligned) { *reinterpret_cast<uchar4*>(bytes + at) = make_uchar4(v[0], v[1], v[2], v[3]); return; }
    }
#pragma unroll
    for (int j = 0; j < m; ++j) bytes[at + j] = v[j];
}

// f(values, ScoreInt<m>, index of values[0]): m = 4 for the 16-byte aligned body, 1 for the elements before and after it
template <int TR, class F>
__device__ __forceinline__ void score_sweep(const ScoreSpan& sp, F&& f) {
    const float4* body = reinterpret_cast<const float4*>(sp.img + sp.head);
    for (int i = threadIdx.x; i < sp.nvec; i += kScoreThreads) {
        const float4 q = body[i];
        const float v[4] = {score_value<TR>(q.x), score_value<TR>(q.y), score_value<TR>(q.z), score_value<TR>(q.w)};
        f(v, ScoreInt<4>(), sp.head + 4 * i);
    }
    const int tail = sp.head + 4 * sp.nvec;
    for (int i = threadIdx.x; i < sp.count - 4 * sp.nvec; i += kScoreThreads) {
        const int at = i < sp.head ? i : tail + (i - sp.head);
        const float v[1] = {score_value<TR>(sp.img[at])};
        f(v, ScoreInt<1>(), at);
    }
}

// Per-lane values -> workgroup totals in a fixed order, so that float64 sums are the same bits run to run: score_wave_totals adds the
// lanes of each wave by __shfl_down with d = 32 .. 1 and leaves lane 0's result in part[wave]; after a barrier, score_block_total adds
// the waves' column j in index order (one thread per total).
template <typename V, int K> __device__ __forceinline__ void score_wave_totals(V (&v)[K], V (*part)[K]) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] += __shfl_down(v[j], d);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < K; ++j) part[threadIdx.x >> 6][j] = v[j];
}
template <typename V, int K> __device__ __forceinline__ V score_block_total(const V (*part)[K], int j) {
    V s = 0;
    for (int w = 0; w < kScoreWaves; ++w) s += part[w][j];
    return s;
}

// One radix step (every thread of the block calls it): merge the per-wave histograms, let wave 0 find the bin that holds the
// `krem`-th largest of the candidates, clear the histograms for the next sweep.  Returns the bin; krem becomes the rank inside it.
__device__ __forceinline__ int score_select(int (*whist)[256], int* tot, int* sel, int& krem) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();
    if (tid < 256) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kScoreWaves; ++w) s += whist[w][tid];
        tot[tid] = s;
    }
    __syncthreads();
    if (tid < 64) {                                           // lane l owns bins 255-4l .. 252-4l: a scan from the largest key down
        const int hi = 255 - 4 * lane;
        const int b0 = tot[hi], b1 = tot[hi - 1], b2 = tot[hi - 2], b3 = tot[hi - 3];
        const int own = b0 + b1 + b2 + b3;
        int incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        int acc = incl - own;
        if (acc < krem && krem <= incl) {                     // exactly one lane
            int bin = hi;
            if (acc + b0 < krem) { acc += b0; bin = hi - 1;
                if (acc + b1 < krem) { acc += b1; bin = hi - 2;
                    if (acc + b2 < krem) { acc += b2; bin = hi - 3; } } }
            sel[0] = bin;
            sel[1] = krem - acc;
        }
    }
    for (int i = tid; i < kScoreWaves * 256; i += kScoreThreads) (&whist[0][0])[i] = 0;
    __syncthreads();
    krem = sel[1];
    return sel[0];
}

template <int TR>
__global__ __launch_bounds__(kScoreThreads) void extraction_scores_kernel(const float* __restrict__ values, int count,
                                                                          ScoreRecord* __restrict__ records,
                                                                          uint8_t* __restrict__ half_mask) {
    __shared__ int whist[kScoreWaves][256];
    __shared__ int tot[256];
    __shared__ int wstat[kScoreWaves][12];
    __shared__ int stat[12];
    __shared__ double wsum[kScoreWaves][1];
    __shared__ int sel[2];
    const int tid = threadIdx.x, wave = tid >> 6;
    const ScoreSpan sp(values, count);
    uint8_t* mk = half_mask ? half_mask + (size_t)blockIdx.x * count : nullptr;
    const bool mk4 = mk && sp.aligned4(mk);
    int* myhist = whist[wave];
    for (int i = tid; i < kScoreWaves * 256; i += kScoreThreads) (&whist[0][0])[i] = 0;
    __syncthreads();

    // sweep 0.  c[0] counts the values in [0, 1], c[j] those of them >= the float32 edge j/10 (numpy's float32 bin edges: a value is in
    // bin i iff e[i] <= v < e[i+1], v == 1 joins the last bin), c[10] the values > 0.5, c[11] the NaNs
    int c[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) c[j] = 0;
    score_sweep<TR>(sp, [&](const float* v, auto M, int at) {
        constexpr int m = decltype(M)::value;
        constexpr float edge[10] = {0.f, 0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f};
        uint8_t bits[m];
#pragma unroll
        for (int j = 0; j < m; ++j) {
            const float x = v[j];
            const bool in = x >= 0.f && x <= 1.f;
            c[0] += in;
#pragma unroll
            for (int e = 1; e < 10; ++e) c[e] += in && x >= edge[e];
            c[10] += x > 0.5f;
            c[11] += x != x;
            bits[j] = x > 0.5f ? 255 : 0;
            atomicAdd(&myhist[score_key(x) >> 24], 1);
        }
        if (mk) store_bytes<m>(mk, at, mk4, bits);
    });
    score_wave_totals(c, wstat);
    int krem = count >> 2;                                    // k: how many of the largest values are averaged
    const int k = krem;
    unsigned prefix = (unsigned)score_select(whist, tot, sel, krem);      // (its first barrier publishes wstat too)
    if (tid < 12) stat[tid] = score_block_total(wstat, tid);

    // sweeps 1..3: among the values whose key starts with `prefix`, histogram the next eight key bits
#pragma unroll 1
    for (int shift = 16; shift >= 0; shift -= 8) {
        score_sweep<TR>(sp, [&](const float* v, auto M, int) {
#pragma unroll
            for (int j = 0; j < decltype(M)::value; ++j) {
                const unsigned key = score_key(v[j]);
                if ((key >> (shift + 8)) == prefix) atomicAdd(&myhist[(key >> shift) & 255u], 1);
            }
        });
        prefix = (prefix << 8) | (unsigned)score_select(whist, tot, sel, krem);
    }

    // sweep 4: prefix is the key of the k-th largest value t; sum |v - 0.5| over the values above it.  The krem values equal to t
    // that complete the k are added once at the end (ties at t contribute (k - number strictly greater) * |t - 0.5|).
    double sum[1] = {0.0};
    score_sweep<TR>(sp, [&](const float* v, auto M, int) {
#pragma unroll
        for (int j = 0; j < decltype(M)::value; ++j)
            if (score_key(v[j]) > prefix) sum[0] += (double)fabsf(v[j] - 0.5f);
    });
    score_wave_totals(sum, wsum);
    __syncthreads();
    if (tid == 0) {
        ScoreRecord r;
        for (int i = 0; i < 9; ++i) r.hist[i] = stat[i] - stat[i + 1];
        r.hist[9] = stat[9];
        r.above_half = stat[10];
        r.n_nan = stat[11];
        r.top_sum = score_block_total(wsum, 0) + (double)krem * (double)fabsf(score_unkey(prefix) - 0.5f);
        r.top_count = k;
        r.reserved = 0;
        records[blockIdx.x] = r;
    }
}

// ---- segmentation scores: the UNet's logits against a label mask ---------------------------------------------------------------
// One workgroup of 16 waves per image, one sweep: the logits in 16-byte pieces (score_sweep's head / body / tail), the label bytes of
// a body piece as one 4-byte load where the image's label stream is aligned there.  Counts are integers; the three sums are float64
// per lane, a fixed shuffle tree per wave, then the waves in order through LDS -- no float atomics, a record is bit-identical run to
// run.  A NaN logit turns all three sums NaN by itself (v * 0 is NaN for the unlabelled pixel too).
__global__ __launch_bounds__(kScoreThreads) void segmentation_scores_kernel(const float* __restrict__ logits,
                                                                            const uint8_t* __restrict__ labels, int count, float thr,
                                                                            SegRecord* __restrict__ records) {
    __shared__ double wsum[kScoreWaves][3];
    __shared__ int wcnt[kScoreWaves][4];
    const ScoreSpan sp(logits, count);
    const uint8_t* lab = labels + (size_t)blockIdx.x * count;
    const bool lab4 = sp.aligned4(lab);
    int c[4] = {0, 0, 0, 0};                                            // n_label, n_pred, n_both, n_nan
    double s[3] = {0.0, 0.0, 0.0};                                      // bce_sum, sig_sum, sig_label_sum
    score_sweep<0>(sp, [&](const float* x, auto M, int at) {
        constexpr int m = decltype(M)::value;
        uint8_t t[m];
        load_bytes<m>(lab, at, lab4, t);
#pragma unroll
        for (int j = 0; j < m; ++j) {
            const float xv = x[j];
            const bool on = t[j] != 0;
            const float tf = on ? 1.f : 0.f;
            const float v = score_value<1>(xv);               // the expression of outc_1x1_kernel's mask
            const bool pred = v > thr;
            c[0] += on;
            c[1] += pred;
            c[2] += on && pred;
            c[3] += xv != xv;
            const float term = (xv > 0.f ? xv : 0.f) - xv * tf + log1pf(expf(-fabsf(xv)));
            s[0] += (double)term;
            s[1] += (double)v;
            s[2] += (double)(v * tf);
        }
    });
    score_wave_totals(s, wsum);
    score_wave_totals(c, wcnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        SegRecord r;
        r.n_label = score_block_total(wcnt, 0); r.n_pred = score_block_total(wcnt, 1);
        r.n_both = score_block_total(wcnt, 2); r.n_nan = score_block_total(wcnt, 3);
        r.bce_sum = score_block_total(wsum, 0); r.sig_sum = score_block_total(wsum, 1); r.sig_label_sum = score_block_total(wsum, 2);
        r.count = count;
        for (int j = 0; j < 5; ++j) r.reserved[j] = 0;
        records[blockIdx.x] = r;
    }
}

// ---- threshold levels: every mask of an ascending threshold grid, and every grid point's counts, from one sweep -------------------
// level = #{k : v > thr[k]} with v = score_value<1>(x), the mask expression of outc_1x1_kernel; the thresholds ascend, so the mask
// at thr[k] is (level > k) and one byte per pixel carries all of them.  One workgroup of 16 waves per image, score_sweep's head /
// body / tail; label bytes come in and level bytes go out four at a time where the image's byte stream is aligned at the body.  The
// level is a data-dependent index, so the histogram [label != 0][level] lives in LDS: private to a wave, in kLevelReps copies chosen
// by the lane's low bits (a crisp mask sends most lanes of a wave to ONE bin; an LDS add to one address serialises over its lanes),
// rows one word longer than the bins so that the copies start in different banks.  Integer LDS adds only, copies and waves summed
// at the end: a record is bit-identical run to run.  The thresholds are wave-uniform LDS reads (broadcast).
constexpr int kLevelReps = 8, kLevelBins = 2 * (kMaxLevelThresholds + 1), kLevelRow = kLevelBins + 1;

__global__ __launch_bounds__(kScoreThreads) void threshold_levels_kernel(const float* __restrict__ logits,
                                                                         const uint8_t* __restrict__ labels, int count,
                                                                         LevelThresholds thr, int nthr, uint8_t* __restrict__ levels,
                                                                         LevelRecord* __restrict__ records) {
    __shared__ int whist[kScoreWaves][kLevelReps][kLevelRow];
    __shared__ int wnan[kScoreWaves][1];
    __shared__ float sthr[kMaxLevelThresholds];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ScoreSpan sp(logits, count);
    const uint8_t* lab = labels ? labels + (size_t)blockIdx.x * count : nullptr;
    uint8_t* lev = levels + (size_t)blockIdx.x * count;
    const bool lab4 = lab && sp.aligned4(lab), lev4 = sp.aligned4(lev);
    for (int i = tid; i < kScoreWaves * kLevelReps * kLevelRow; i += kScoreThreads) (&whist[0][0][0])[i] = 0;
#pragma unroll
    for (int k = 0; k < kMaxLevelThresholds; ++k)
        if (tid == k) sthr[k] = thr.t[k];                     // constant indices: the by-value argument stays in the kernel-argument segment
    __syncthreads();
    int* myhist = whist[wave][lane & (kLevelReps - 1)];
    int nan[1] = {0};
    score_sweep<1>(sp, [&](const float* v, auto M, int at) {
        constexpr int m = decltype(M)::value;
        // the label bytes are load_bytes written out, with "no labels" read as zeros: through the helper (behind `if (lab)`, or with the
        // null test inside it) this kernel measured 2 % slower, twice (profiles/pointwise_one_scaffold.md)
        uint8_t t[m], out[m];
        bool loaded = false;
        if constexpr (m == 4) {
            if (lab4) {
                const uchar4 q = *reinterpret_cast<const uchar4*>(lab + at);
                t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
                loaded = true;
            }
        }
        if (!loaded) {
#pragma unroll
            for (int j = 0; j < m; ++j) t[j] = lab ? lab[at + j] : (uint8_t)0;
        }
#pragma unroll
        for (int j = 0; j < m; ++j) {
            const float x = v[j];
            int level = 0;
            for (int k = 0; k < nthr; ++k) level += x > sthr[k];          // a NaN compares false everywhere: level 0, as the fused mask
            nan[0] += x != x;
            out[j] = (uint8_t)level;
            atomicAdd(&myhist[(t[j] != 0 ? kMaxLevelThresholds + 1 : 0) + level], 1);
        }
        store_bytes<m>(lev, at, lev4, out);
    });
    score_wave_totals(nan, wnan);
    __syncthreads();
    LevelRecord* r = records + blockIdx.x;
    if (tid < kLevelBins) {
        int s = 0;
        for (int w = 0; w < kScoreWaves; ++w)
#pragma unroll
            for (int c = 0; c < kLevelReps; ++c) s += whist[w][c][tid];
        (&r->hist[0][0])[tid] = s;
    } else if (tid < kLevelBins + (int)(sizeof(r->reserved) / sizeof(int32_t))) {
        r->reserved[tid - kLevelBins] = 0;
    } else if (tid == kScoreThreads - 1) {
        r->count = count;
        r->n_thresholds = nthr;
        r->n_nan = score_block_total(wnan, 0);
    }
}

// ---- MFMA lane-map probes (same fragment addressing as conv_igemm.hip) ---------------------------
__global__ void mfma_probe_f16_kernel(const half_t* a, const half_t* b, float* d) {
    const int lane = threadIdx.x, q = lane >> 4, r = lane & 15;
    const half8 fa = *reinterpret_cast<const half8*>(a + r * 32 + q * 8);
    const half8 fb = *reinterpret_cast<const half8*>(b + r * 32 + q * 8);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb, acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[(q * 4 + i) * 16 + r] = acc[i];      // D[row = A row][col = B row]
}
__global__ void mfma_probe_f32_kernel(const float* a, const float* b, float* d) {
    const int lane = threadIdx.x, q = lane >> 4, r = lane & 15;
    const f4 fa = *reinterpret_cast<const f4*>(a + r * 16 + q * 4);
    const f4 fb = *reinterpret_cast<const f4*>(b + r * 16 + q * 4);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[j], fb[j], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[(q * 4 + i) * 16 + r] = acc[i];
}

// ---- host wrappers ----------------------------------------------------------------------------------
// The one storage-type switch: f(Tag<T>()) with T = half_t (kF16), split_t (kSplit) or float (kF32 and anything else); the lambda
// names its kernel with T.  A wrapper whose kernel does not exist for float refuses kF32 first and leaves that case empty
// (`if constexpr`), so nothing is instantiated for it.
template <typename T> struct Tag { using type = T; };
template <class G> using tag_t = typename G::type;
template <class F> static inline void with_dtype(int dt, F&& f) {
    if (dt == kF16) f(Tag<half_t>());
    else if (dt == kSplit) f(Tag<split_t>());
    else f(Tag<float>());
}
// The caller's image beside it: f(typed pointer, NORM) -- float, u8 (/255 in the kernel), or u8 that is normalised as well.
template <class P> using pointee_t = std::remove_const_t<std::remove_pointer_t<P>>;
template <class F> static inline void with_input(const void* x, bool x_is_u8, bool norm, F&& f) {
    if (norm) f((const uint8_t*)x, std::true_type());
    else if (x_is_u8) f((const uint8_t*)x, std::false_type());
    else f((const float*)x, std::false_type());
}

static inline float pow2f(int e) { return ldexpf(1.f, e); }

hipError_t pack_nchw_f32(int dt, const float* src, int c, const TensorRef& dst, unsigned* flag, hipStream_t s) {
    if (dst.C % dtype_group(dt) || dst.Coff % dtype_group(dt)) return hipErrorInvalidValue;
    const dim3 g(grid_for((size_t)dst.N * dst.H * dst.W * (dst.C / dtype_group(dt)))), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(pack_nchw_f32_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, c, dst, pow2f(-dst.exp), flag); });
    return hipGetLastError();
}
hipError_t pack_hwc3_u8(int dt, const uint8_t* src, const TensorRef& dst, hipStream_t s) {
    if (dst.C != 8 || dst.Coff % 8) return hipErrorInvalidValue;
    const dim3 g(grid_for((size_t)dst.N * dst.H * dst.W)), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(pack_hwc3_u8_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, dst, pow2f(-dst.exp)); });
    return hipGetLastError();
}
hipError_t unpack_nchw_f32(int dt, const TensorRef& src, float* dst, hipStream_t s) {
    if (src.Coff % dtype_group(dt)) return hipErrorInvalidValue;
    const dim3 g(grid_for((size_t)src.N * src.C * src.H * src.W)), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(unpack_nchw_f32_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, dst, pow2f(src.exp)); });
    return hipGetLastError();
}
hipError_t absmax(int dt, const TensorRef& src, unsigned* out, hipStream_t s) {
    if (src.C % dtype_group(dt) || src.Coff % dtype_group(dt)) return hipErrorInvalidValue;
    const size_t work = (size_t)src.N * src.H * src.W * (src.C / dtype_group(dt));
    const dim3 g((unsigned)std::min<size_t>(grid_for(work), 4096)), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(absmax_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, out); });
    return hipGetLastError();
}
hipError_t channel_means(int dt, const TensorRef& src, float* out, hipStream_t s) {
    if (src.f32_only) dt = kF32;
    if (!src.base || !out || ((uintptr_t)out & 15u) || src.N < 1 || src.H < 1 || src.W < 1 || src.C < 8 || src.C % 8 || src.Coff % dtype_group(dt) ||
        src.split)
        return hipErrorInvalidValue;
    const int slices = channel_means_slices(src.H * src.W);
    const size_t units = (size_t)src.N * (src.C / 8);
    const dim3 g(grid_for(units, 256 / slices)), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(channel_means_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, slices, pow2f(src.exp), out); });
    return hipGetLastError();
}
hipError_t tap_sums_f16(const TensorRef& src, int Ho, int Wo, int stride, int k, int slices, double* out, hipStream_t s) {
    if (slices < 1 || (k != 1 && k != 3) || (Ho - 1) * stride + k - (k - 1) / 2 > src.H + 1 || (Wo - 1) * stride + k - (k - 1) / 2 > src.W + 1)
        return hipErrorInvalidValue;
    const int per = (src.N + slices - 1) / slices;
    hipLaunchKernelGGL(tap_sums_f16_kernel, dim3((unsigned)(k * k), (unsigned)((src.C + 63) / 64), (unsigned)slices), dim3(64), 0, s, src, Ho, Wo,
                       stride, k, per, out);
    return hipGetLastError();
}
hipError_t maxpool2x2(int dt, const TensorRef& src, const TensorRef& dst, hipStream_t s) {
    const dim3 g(grid_for((size_t)dst.N * dst.H * dst.W * (dst.C / dtype_group(dt)))), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(maxpool2x2_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, dst); });
    return hipGetLastError();
}
hipError_t maxpool3x3s2(int dt, const TensorRef& src, const TensorRef& dst, hipStream_t s) {
    const dim3 g(grid_for((size_t)dst.N * dst.H * dst.W * (dst.C / dtype_group(dt)))), b(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(maxpool3x3s2_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, dst); });
    return hipGetLastError();
}
hipError_t upsample_bilinear2x(int dt, const TensorRef& src, const TensorRef& dst, unsigned* flag, unsigned layer_id,
                               hipStream_t s) {
    const dim3 g((unsigned)((dst.W * (dst.C / dtype_group(dt)) + 255) / 256), (unsigned)dst.H, (unsigned)dst.N), b(256);
    const float mul = pow2f(src.exp - dst.exp);
    const float sy = dst.H > 1 ? (float)(src.H - 1) / (float)(dst.H - 1) : 0.f;
    const float sx = dst.W > 1 ? (float)(src.W - 1) / (float)(dst.W - 1) : 0.f;
    static const bool block2x2 = env_switch("CV_UPSAMPLE_2X2", true);    // read once per process
    if (dt == kSplit && block2x2 && dst.H == 2 * src.H && dst.W == 2 * src.W) {
        const dim3 g2((unsigned)(((src.W + 1) * (dst.C / 8) + 255) / 256), (unsigned)(src.H + 1), (unsigned)dst.N);
        hipLaunchKernelGGL(upsample_bilinear2x_split2x2_kernel, g2, b, 0, s, src, dst, mul, sy, sx, flag, layer_id);
    } else {
        with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(upsample_bilinear2x_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, dst, mul, sy, sx, flag, layer_id); });
    }
    return hipGetLastError();
}
hipError_t outc_1x1(int dt, const TensorRef& src, const float* w, const float* bias, float* logits,
                    uint8_t* mask, float threshold, unsigned* flag, unsigned layer_id, hipStream_t s) {
    const int lpp = src.C / dtype_group(dt);
    if (lpp < 1 || lpp > 64 || (lpp & (lpp - 1))) return hipErrorInvalidValue;
    const dim3 g(grid_for((size_t)src.N * src.H * src.W * lpp)), b(256);
    with_dtype(dt, [&](auto t) {
        hipLaunchKernelGGL(outc_1x1_kernel<tag_t<decltype(t)>>, g, b, 0, s, src, w, bias, pow2f(src.exp), logits, mask, threshold, flag, layer_id);
    });
    return hipGetLastError();
}
hipError_t stem7x7(int dt, const void* x, bool x_is_u8, int n, const float* w, const float* scale,
                   const float* shift, const TensorRef& dst, hipStream_t s, const InputNorm* norm) {
    if (dst.C != 64 || dst.H != 32 || dst.W != 32 || dst.Coff != 0 || (norm && !x_is_u8)) return hipErrorInvalidValue;
    const dim3 g((unsigned)n), b(256);
    const InputNorm nm = norm ? *norm : InputNorm{0.f, 1.f};
    with_dtype(dt, [&](auto t) {
        with_input(x, x_is_u8, norm != nullptr, [&](auto* px, auto NORM) {
            hipLaunchKernelGGL((stem7x7_kernel<tag_t<decltype(t)>, pointee_t<decltype(px)>, decltype(NORM)::value>), g, b, 0, s, px, w, scale, shift, dst, nm);
        });
    });
    return hipGetLastError();
}
hipError_t stem_pool_mfma(int dt, const void* x, bool x_is_u8, int n, const void* wpk, const float* scale,
                          const float* shift, int in_exp, const TensorRef& dst, unsigned* flag, unsigned layer_id,
                          hipStream_t s, const InputNorm* norm) {
    if (dt == kF32 || dst.C != 64 || dst.Cs != 64 || dst.H != 16 || dst.W != 16 || dst.Coff != 0 || (norm && !x_is_u8))
        return hipErrorInvalidValue;                     // rows of the tensor are contiguous runs
    const dim3 g((unsigned)(n < 2048 ? n : 2048)), b(256);
    const half8* w = reinterpret_cast<const half8*>(wpk);
    const float im = pow2f(-in_exp);
    const InputNorm nm = norm ? *norm : InputNorm{0.f, 1.f};
    with_dtype(dt, [&](auto t) {
        using T = tag_t<decltype(t)>;
        if constexpr (!std::is_same_v<T, float>) with_input(x, x_is_u8, norm != nullptr, [&](auto* px, auto NORM) {
            auto launch = [&](auto SPLIT) {
                hipLaunchKernelGGL((stem_pool_mfma_kernel<T, pointee_t<decltype(px)>, decltype(SPLIT)::value, decltype(NORM)::value>), g, b, 0, s, px, n, w,
                                   scale, shift, im, dst, flag, layer_id, nm);
            };
            if constexpr (std::is_same_v<T, split_t>) launch(std::true_type());
            else if (dst.base32) launch(std::true_type());    // f16r engine: split-f16 arithmetic, f16 tensor + f32 twin out
            else launch(std::false_type());
        });
    });
    return hipGetLastError();
}
hipError_t inc0_mfma(int dt, const void* x, bool x_is_u8, int n, const void* wpk, const float* scale, const float* shift,
                     int in_exp, const TensorRef& dst, unsigned* flag, unsigned layer_id, hipStream_t s) {
    if (dt == kF32 || dst.C != 64 || dst.H != 256 || dst.W != 256 || dst.Coff != 0 || dst.Cs != 64) return hipErrorInvalidValue;
    const dim3 g((unsigned)(n * 32)), b(256);
    const half8* w = reinterpret_cast<const half8*>(wpk);
    const float im = pow2f(-in_exp);
    with_dtype(dt, [&](auto t) {
        using T = tag_t<decltype(t)>;
        if constexpr (!std::is_same_v<T, float>) with_input(x, x_is_u8, false, [&](auto* px, auto) {
            hipLaunchKernelGGL((inc0_mfma_kernel<T, pointee_t<decltype(px)>>), g, b, 0, s, px, w, scale, shift, im, dst, flag, layer_id);
        });
    });
    return hipGetLastError();
}
hipError_t head_avgpool_fc(int dt, const TensorRef& src, const float* w, const float* b, float* out,
                           int softmax, unsigned* flag, unsigned layer_id, hipStream_t s) {
    if (src.C != 512 || src.Coff != 0 || src.Cs != 512) return hipErrorInvalidValue;      // the kernel keeps lane l on channels 8l..8l+7
    const int blocks = (src.N + 3) / 4;
    const dim3 g((unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks)), blk(256);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(head_kernel<tag_t<decltype(t)>>, g, blk, 0, s, src, w, b, pow2f(src.exp), out, softmax, flag, layer_id); });
    return hipGetLastError();
}
hipError_t stem3x3s2(int dt, const void* x, bool x_is_u8, int n, const float* w, const float* scale, const float* shift,
                     const TensorRef& dst, unsigned* flag, unsigned layer_id, hipStream_t s, const InputNorm* norm) {
    if (n < 1 || dst.N < n || dst.C % 8 || dst.C < 8 || dst.C != dst.Cs || dst.Coff != 0 || dst.H != 32 || dst.W != 32 || (norm && !x_is_u8))
        return hipErrorInvalidValue;
    const dim3 g((unsigned)n), b(256);
    const InputNorm nm = norm ? *norm : InputNorm{0.f, 1.f};
    with_dtype(dt, [&](auto t) {
        with_input(x, x_is_u8, norm != nullptr, [&](auto* px, auto NORM) {
            hipLaunchKernelGGL((stem3x3s2_kernel<tag_t<decltype(t)>, pointee_t<decltype(px)>, decltype(NORM)::value>), g, b, 0, s, px, w, scale, shift,
                               dst, pow2f(-dst.exp), nm, flag, layer_id);
        });
    });
    return hipGetLastError();
}
hipError_t head_pool_fc(int dt, const TensorRef& src, const float* w, const float* b, float* out, float* pooled, int softmax,
                        unsigned* flag, unsigned layer_id, hipStream_t s) {
    if (src.N < 1 || src.C % 8 || src.C < 8 || src.Coff != 0 || src.Cs != src.C || src.split || ((uintptr_t)pooled & 15u)) return hipErrorInvalidValue;
    const int blocks = (src.N + 4 * kHeadQ - 1) / (4 * kHeadQ);
    const dim3 g((unsigned)(blocks > 2048 ? 2048 : blocks)), blk(256);
    with_dtype(dt, [&](auto t) {
        hipLaunchKernelGGL(head_pool_fc_kernel<tag_t<decltype(t)>>, g, blk, 0, s, src, w, b, pow2f(src.exp), out, pooled, softmax, flag, layer_id);
    });
    return hipGetLastError();
}
hipError_t extraction_scores(const float* values, int n, int count, int transform, ScoreRecord* records, uint8_t* half_mask,
                             hipStream_t s) {
    if (!values || !records || n < 1 || count < 4 || count > (1 << 24) || ((uintptr_t)values & 3u) || (transform != 0 && transform != 1))
        return hipErrorInvalidValue;
    if (transform) hipLaunchKernelGGL(extraction_scores_kernel<1>, dim3((unsigned)n), dim3(kScoreThreads), 0, s, values, count, records, half_mask);
    else hipLaunchKernelGGL(extraction_scores_kernel<0>, dim3((unsigned)n), dim3(kScoreThreads), 0, s, values, count, records, half_mask);
    return hipGetLastError();
}
hipError_t segmentation_scores(const float* logits, const uint8_t* labels, int n, int count, float threshold, SegRecord* records,
                               hipStream_t s) {
    if (!logits || !labels || !records || n < 1 || count < 1 || count > (1 << 24) || ((uintptr_t)logits & 3u) || !(threshold - threshold == 0.f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(segmentation_scores_kernel, dim3((unsigned)n), dim3(kScoreThreads), 0, s, logits, labels, count, threshold, records);
    return hipGetLastError();
}
hipError_t threshold_levels(const float* logits, const uint8_t* labels, int n, int count, const float* thresholds, int n_thresholds,
                            uint8_t* levels, LevelRecord* records, hipStream_t s) {
    if (!logits || !thresholds || !levels || !records || n < 1 || count < 1 || count > (1 << 24) || ((uintptr_t)logits & 3u) ||
        ((uintptr_t)records & 3u) || n_thresholds < 1 || n_thresholds > kMaxLevelThresholds)
        return hipErrorInvalidValue;
    LevelThresholds thr;
    for (int k = 0; k < kMaxLevelThresholds; ++k) {
        thr.t[k] = k < n_thresholds ? thresholds[k] : 2.f;    // past the grid: above every sigmoid, never read
        if (k < n_thresholds && (!(thr.t[k] >= 0.f && thr.t[k] <= 1.f) || (k > 0 && !(thr.t[k] > thr.t[k - 1])))) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(threshold_levels_kernel, dim3((unsigned)n), dim3(kScoreThreads), 0, s, logits, labels, count, thr, n_thresholds,
                       levels, records);
    return hipGetLastError();
}
hipError_t softmax13(const float* logits, int n, float* probs, hipStream_t s) {
    hipLaunchKernelGGL(softmax13_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, s, logits, n, probs);
    return hipGetLastError();
}
hipError_t square_records(const float* logits, const int8_t* labels, int n, SquareRecord* records, hipStream_t s) {
    if (!logits || !records || n < 1 || ((uintptr_t)logits & 3u) || ((uintptr_t)records & 7u)) return hipErrorInvalidValue;
    const dim3 g_(std::min(grid_for((size_t)n), 4096u)), b_(256);
    hipLaunchKernelGGL(square_records_kernel, g_, b_, 0, s, logits, labels, n, records);
    return hipGetLastError();
}
hipError_t mfma_probe_f16(const half_t* a, const half_t* b, float* d, hipStream_t s) {
    hipLaunchKernelGGL(mfma_probe_f16_kernel, dim3(1), dim3(64), 0, s, a, b, d);
    return hipGetLastError();
}
hipError_t mfma_probe_f32(const float* a, const float* b, float* d, hipStream_t s) {
    hipLaunchKernelGGL(mfma_probe_f32_kernel, dim3(1), dim3(64), 0, s, a, b, d);
    return hipGetLastError();
}

}  // namespace cv
