// conv1x1_lds.hip -- the LDS-resident 1x1 GEMM: kernels, weight packer, exponent fold and launch (conv1x1_lds.h).
//
// One GEMM shape -- K = Cin in {64, 128, 256}, 2 Cin rows, three split-f16 MFMA products per MAC -- serves the ResNet stage-boundary
// shortcuts (f32 twins of the f16r engine, split-f16 tensors of the f16x3 engine) and the UNet transposed convolutions up3.up / up4.up.
// Unlike the rest of the small kernels (pointwise.hip) it has something to keep on the chip: up to 128 KB of weights in LDS under
// eight persistent waves.
#include "conv1x1_lds.h"
#include "conv_device.h"   // OutVec (split-f16 store units)

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace cv {

// ---- f16r engine: ResNet stage-boundary shortcut (conv 1x1 / stride 2 + BN) from f32 twin to f32 twin ---------------------------
// reference: timm BasicBlock.downsample = [Conv2d(C, 2C, 1, stride 2, bias=False), BatchNorm2d] (notebooks/model-summary.ipynb).
// The shortcut IS the residual trunk at a stage boundary, so it runs at f32 grade: both operands are split into f16 hi + lo (the
// pixel values on the fly from the f32 twin, the weights at load time, rows normalised) and every k-step is three f16 MFMAs
// hi.hi + lo.hi + hi.lo with f32 accumulation -- the arithmetic of the f16x3 engine.  Round 4 ran these three layers on the f32-input
// MFMA through the generic implicit-GEMM kernel: 0.28 + 0.20 + 0.16 ms per 16384 squares for 1.1 % of the network's MACs (K = Cin is
// two to eight stages: all prologue); here a wave owns 16 output pixels x 128 channels, reads each pixel's Cin floats once and
// streams the packed weight fragments from L2; HBM-bound (Cin floats in, 2 Cin floats out per output pixel).
template <int CIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void shortcut1x1s2_kernel(const float* __restrict__ x, int n, int H, int W, const half8* __restrict__ wpk,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            float* __restrict__ y, unsigned* flag, unsigned layer_id) {
    constexpr int COUT = 2 * CIN, KS = CIN / 32, CG = COUT / 128;
    const int Ho = H / 2, Wo = W / 2, M = n * Ho * Wo;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
    const int task = blockIdx.x * 4 + wave;                      // (group of 16 output pixels, group of 128 output channels)
    const int cg = task % CG, pg = task / CG;
    if (pg * 16 >= M) return;
    int m = pg * 16 + l15;
    const bool live = m < M;
    if (!live) m = M - 1;
    const int ox = m % Wo, oy = (m / Wo) % Ho, img = m / (Wo * Ho);
    const float* const xp = x + ((size_t)(img * (H + 2) + 2 * oy + 1) * (W + 2) + 2 * ox + 1) * CIN + q * 8;
    f4 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = f4{0.f, 0.f, 0.f, 0.f};
    // Two k-steps at a time, every load of the batch issued before its first MFMA (4 pixel + 32 weight-fragment loads = 144
    // registers in flight): left to itself the compiler interleaves load / wait / MFMA one fragment at a time and a wave spends its
    // life in ~32 dependent L2 round trips (measured: 0.38 ms per 16384 squares for layer2.0, slower than the generic kernel).
#pragma unroll
    for (int kb = 0; kb < KS; kb += 2) {
        f4 xv[2][2];
        half8 wa[2][16];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            xv[u][0] = *reinterpret_cast<const f4*>(xp + (kb + u) * 32);
            xv[u][1] = *reinterpret_cast<const f4*>(xp + (kb + u) * 32 + 4);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const half8* const wp = wpk + ((size_t)(cg * KS + kb + u) * 16) * 64 + lane;      // [cg][ks][fragment 8][hi | lo][lane]
#pragma unroll
            for (int i = 0; i < 16; ++i) wa[u][i] = wp[i * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            // B fragment: k = 8 q + j of this k-step = eight consecutive input channels of pixel l15, split into f16 hi + lo.  Plain C on
            // purpose: the inline-asm pair conversion (cv_kernels.h: split_pair) next to independent MFMAs gave run-to-run different
            // results here -- the compiler cannot see the hazard between an in-flight MFMA's source registers and an asm's output
            half8 bh, bl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = j < 4 ? xv[u][0][j] : xv[u][1][j - 4];
                bh[j] = (half_t)v;
                bl[j] = (half_t)(v - (float)bh[j]);
            }
#pragma unroll
            for (int f = 0; f < 8; ++f) {
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[u][2 * f], bh, acc[f], 0, 0, 0);
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[u][2 * f + 1], bh, acc[f], 0, 0, 0);
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[u][2 * f], bl, acc[f], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // lane (q, l15): channels 128 cg + 32 q + 4 f + r of pixel l15 (the weight rows were packed in that order): 128 contiguous bytes
    const int c0 = cg * 128 + q * 32;
    float* const yp = y + ((size_t)(img * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * COUT + c0;
    float bad = 0.f;
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        const f4 sc = *reinterpret_cast<const f4*>(scale + c0 + f * 4), sh = *reinterpret_cast<const f4*>(shift + c0 + f * 4);
        f4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) { o[r] = acc[f][r] * sc[r] + sh[r]; bad = __builtin_fmaf(o[r], 0.f, bad); }
        if (live) *reinterpret_cast<f4*>(yp + f * 4) = o;
    }
    if (live && bad != bad && flag) atomicMin(flag, layer_id);
}

// Second form (round 5, late): the weights of the workgroup's 128-channel group live in LDS (KS x 16 KB, staged once), eight PERSISTENT
// waves walk the pixel groups and read their weight fragments from LDS -- in the first form every wave streamed those 32-128 KB from L2
// for 16 pixels of work (2.1 GB of L2 traffic per launch against 0.2-0.8 GB of HBM bytes: that, not the stride-2 read, was what the
// launch waited for).  The next pixel group's floats are fetched while the current one is multiplied (CIN <= 128: 16-32 registers).
// Same arithmetic, same operation order per output as the first form: same bits.
// SPLIT (round 6: the headline engine's shortcuts): x and y are split-f16 tensors instead of f32 twins.  A channel group is 32 bytes
// either way, so every address is the same; the two 16-byte chunks a lane fetches per k-step ARE its hi and lo operand (no conversion),
// and the staged epilogue writes each group's hi and lo chunk from the lane pair that shares the group -- still one contiguous KB per
// store instruction.  Products and their order (w_hi x_hi, w_lo x_hi, w_hi x_lo per 32-channel k-step) are those of conv_igemm_kernel
// on split_t: bit-identical to the generic launch it replaces.
// CONVT (round 6, SPLIT only): the same GEMM shape -- K = Cin, 2 Cin rows -- is a k2 / s2 transposed convolution whose rows are (dy, dx, co),
// 4 x Cin/2 of them: UNet up3.up (256 -> 128) and up4.up (128 -> 64).  Differences to the shortcut: the input pixels are dense (stride
// 1: 16 consecutive pixels are 8-16 KB of contiguous memory), and a staged row group leaves as a PIXEL SHUFFLE -- rows of class (dy, dx)
// go to output pixel (2 y + dy, 2 x + dx), channel slice [yCoff, yCoff + cout) of a buffer with yCs channels per pixel (the concatenated
// skip | up tensor).  The generic 256 x 256 tile moves these two layers' bytes at 3.2 / 4.0 TB/s: a 4- or 8-stage K loop, then 256 KB of
// stores per tile with nothing else resident on the CU; here the weights stay in LDS and eight persistent waves alternate loads, MFMAs
// and full-line stores.  Products and their order are the generic kernel's: bit-identical.
template <int CIN, bool STAGE, bool SPLIT = false, bool CONVT = false>
__global__ __launch_bounds__(512) void shortcut1x1s2_lds_kernel(
    const float* __restrict__ x, int n, int H, int W, const half8* __restrict__ wpk, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ y, unsigned* flag, unsigned layer_id, int yCs = 0, int yCoff = 0, int cout = 0) {
    static_assert(!CONVT || (SPLIT && STAGE), "the transposed-convolution form exists for split-f16 tensors, staged stores");
    constexpr int COUT = 2 * CIN, KS = CIN / 32, NW = 8;        // eight waves (four, and the next pixel group fetched after the stores
                                                                // instead of under the MFMAs: measured no better, profiles/r05_tuning.md)
    extern __shared__ __attribute__((aligned(16))) char smem_sc[];
    half8* const wl = reinterpret_cast<half8*>(smem_sc);
    const int cg = blockIdx.y;
    for (int i = threadIdx.x; i < KS * 16 * 64; i += 64 * NW) wl[i] = wpk[(size_t)cg * KS * 16 * 64 + i];
    // the group's BN scale / shift next to the weights: read from LDS in the epilogue.  As global loads they sat BEHIND the previous
    // iteration's stores in the wave's in-order memory counter, so every iteration waited for its predecessor's stores to retire
    // (7.7 us per iteration for 0.4 us of MFMAs)
    float* const sl = reinterpret_cast<float*>(smem_sc + (size_t)KS * 16 * 1024);
    if (threadIdx.x < 128) { sl[threadIdx.x] = scale[cg * 128 + threadIdx.x]; sl[128 + threadIdx.x] = shift[cg * 128 + threadIdx.x]; }
    __syncthreads();
    const int Ho = CONVT ? H : H / 2, Wo = CONVT ? W : W / 2, M = n * Ho * Wo, ngroups = (M + 15) / 16;   // GEMM pixels = output pixels of the shortcut | INPUT pixels of the transposed convolution
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
    const int c0 = cg * 128 + q * 32;
    auto src_of = [&](int pg) {
        int m = pg * 16 + l15;
        m = m < M ? m : M - 1;
        const int ox = m % Wo, oy = (m / Wo) % Ho, img = m / (Wo * Ho);
        if constexpr (CONVT) return x + ((size_t)(img * (H + 2) + oy + 1) * (W + 2) + ox + 1) * CIN + q * 8;
        else return x + ((size_t)(img * (H + 2) + 2 * oy + 1) * (W + 2) + 2 * ox + 1) * CIN + q * 8;
    };
    auto fetch = [&](const float* xp, f4 (&xv)[KS][2]) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            xv[k][0] = *reinterpret_cast<const f4*>(xp + k * 32);
            xv[k][1] = *reinterpret_cast<const f4*>(xp + k * 32 + 4);
        }
    };
    float bad = 0.f;
    const int stride = gridDim.x * NW;
    int pg = blockIdx.x * NW + wave;
    f4 xn[KS][2];
    if (pg < ngroups) fetch(src_of(pg), xn);
    for (; pg < ngroups; pg += stride) {
        f4 xv[KS][2];
#pragma unroll
        for (int k = 0; k < KS; ++k) { xv[k][0] = xn[k][0]; xv[k][1] = xn[k][1]; }
        if (pg + stride < ngroups) fetch(src_of(pg + stride), xn);
        f4 acc[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) acc[f] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            half8 bh, bl;                                    // plain C conversion: see the first form
            if constexpr (SPLIT) {                           // group k*4 + q: even groups are stored [hi, lo], odd ones [lo, hi]
                const half8 a = __builtin_bit_cast(half8, xv[k][0]), b = __builtin_bit_cast(half8, xv[k][1]);
                bh = (q & 1) ? b : a;
                bl = (q & 1) ? a : b;
            } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = j < 4 ? xv[k][0][j] : xv[k][1][j - 4];
                bh[j] = (half_t)v;
                bl[j] = (half_t)(v - (float)bh[j]);
            }
            }
            // weight fragments four channel fragments at a time (32 registers live; left alone the compiler hoists every LDS read of
            // every k-step to the top of the iteration and spills 200-400 registers)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                half8 wa[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) wa[i] = wl[(k * 16 + h * 8 + i) * 64 + lane];
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    acc[h * 4 + f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[2 * f], bh, acc[h * 4 + f], 0, 0, 0);
                    acc[h * 4 + f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[2 * f + 1], bh, acc[h * 4 + f], 0, 0, 0);
                    acc[h * 4 + f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[2 * f], bl, acc[h * 4 + f], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const int m = pg * 16 + l15;
        const bool live = m < M;
        const int mm = live ? m : M - 1;
        const int ox = mm % Wo, oy = (mm / Wo) % Ho, img = mm / (Wo * Ho);
        // shortcut: the output pixel; transposed convolution: output pixel (2 oy, 2 ox) of the 2H x 2W plane, class (dy, dx) adds dy rows + dx
        const size_t opix = CONVT ? (size_t)(img * (2 * Ho + 2) + 2 * oy + 1) * (2 * Wo + 2) + 2 * ox + 1
                                  : (size_t)(img * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1;
        if constexpr (STAGE) {
            // the accumulators leave each lane with 32 channels of ONE pixel: eight store instructions of 64 scattered 16-byte pieces.  Park
            // the wave's 16 x 128 tile in its own LDS corner (rows padded to 528 B) and read it back two whole pixel rows per instruction:
            // every store instruction then writes 1 KB in full lines.  Wave-private: DS operations of a wave execute in order.
            // SR pixel rows per pass (16 = the whole tile; Cin = 256 keeps 128 KB of weights in LDS and stages 4 rows at a time).
            constexpr int SROW = 528, SR = CIN <= 128 ? 16 : 4;
            char* const stg = smem_sc + (size_t)KS * 16 * 1024 + 1024 + (size_t)wave * (SR * SROW + 64);
            unsigned* const pixw = reinterpret_cast<unsigned*>(stg + SR * SROW);
            f4 o[8];
#pragma unroll
            for (int f = 0; f < 8; ++f) {
                const f4 sc = *reinterpret_cast<const f4*>(sl + q * 32 + f * 4), sh = *reinterpret_cast<const f4*>(sl + 128 + q * 32 + f * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) { o[f][r] = acc[f][r] * sc[r] + sh[r]; bad = __builtin_fmaf(o[f][r], 0.f, bad); }
            }
#pragma unroll
            for (int ps = 0; ps < 16 / SR; ++ps) {
                if (SR == 16 || (l15 / SR) == ps) {
#pragma unroll
                    for (int f = 0; f < 8; ++f) *reinterpret_cast<f4*>(stg + (l15 % SR) * SROW + (q * 32 + f * 4) * 4) = o[f];
                    if (q == 0) pixw[l15 % SR] = live ? (unsigned)opix : 0xffffffffu;
                }
                wave_lds_sync();
#pragma unroll
                for (int j = 0; j < SR / 2; ++j) {
                    const int px = 2 * j + (lane >> 5), part = lane & 31;
                    const unsigned op = pixw[px];
                    if constexpr (SPLIT) {
                        // lanes 2g and 2g + 1 share channel group g of the pixel: one writes the group's first 16-byte chunk, the other the second
                        const int gl = part >> 1, par = gl & 1;                  // (cg * 16 + gl) & 1: a 128-channel group starts on an even group
                        const f4 v0 = *reinterpret_cast<const f4*>(stg + px * SROW + gl * 32), v1 = *reinterpret_cast<const f4*>(stg + px * SROW + gl * 32 + 16);
                        const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                        if ((part & 1) == 0) {                                   // range guard on the f16 hi halves, once per group
#pragma unroll
                            for (int i = 0; i < 8; ++i) bad = __builtin_fmaf((float)(half_t)v[i], 0.f, bad);
                        }
                        if constexpr (CONVT) {
                            const int row = cg * 128 + gl * 8, cls = row / cout, co = row - cls * cout, ch0 = yCoff + co;
                            if (op != 0xffffffffu)
                                OutVec<split_t, 8>::store_half(reinterpret_cast<split_t*>(y) + ((size_t)op + (size_t)((cls >> 1) * (2 * Wo + 2) + (cls & 1))) * yCs + ch0,
                                                               ch0, v, (part & 1) == ((ch0 >> 3) & 1));
                        } else {
                        if (op != 0xffffffffu)
                            OutVec<split_t, 8>::store_half(reinterpret_cast<split_t*>(y) + (size_t)op * COUT + cg * 128 + gl * 8, gl * 8, v, (part & 1) == par);
                        }
                    } else {
                    const f4 v = *reinterpret_cast<const f4*>(stg + px * SROW + part * 16);
                    if (op != 0xffffffffu) *reinterpret_cast<f4*>(y + (size_t)op * COUT + cg * 128 + part * 4) = v;
                    }
                }
                wave_lds_sync();
            }
        } else {
        float* const yp = y + opix * COUT + c0;
        float ov[32];
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const f4 sc = *reinterpret_cast<const f4*>(sl + q * 32 + f * 4), sh = *reinterpret_cast<const f4*>(sl + 128 + q * 32 + f * 4);
            f4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) { o[r] = acc[f][r] * sc[r] + sh[r]; bad = __builtin_fmaf(o[r], 0.f, bad); ov[f * 4 + r] = o[r]; }
            if (!SPLIT && live) *reinterpret_cast<f4*>(yp + f * 4) = o;
        }
        if (SPLIT && live) OutVec<split_t, 32>::store(reinterpret_cast<split_t*>(yp), c0, ov, bad);
        }
    }
    if (bad != bad && flag) atomicMin(flag, layer_id);
}

// ---- host side: the packed matrix, its epilogue constants, the launch ------------------------------------------------------------
Status Lds1x1::pack(int rows, int K, const std::function<float(int, int)>& element, const std::function<float(int)>& row_scale,
                    const std::function<float(int)>& row_shift, const std::string& name_) {
    name = name_;
    std::vector<int> rex((size_t)rows, 0);
    h_scale.assign((size_t)rows, 0.f); h_shift.assign((size_t)rows, 0.f);
    for (int r = 0; r < rows; ++r) {
        float mx = 0.f;
        for (int k = 0; k < K; ++k) {
            const float v = element(r, k);
            if (!std::isfinite(v)) return fail(1, name + ": non-finite weight in the state dict");
            mx = std::max(mx, std::fabs(v));
        }
        if (mx > 0.f) (void)std::frexp(mx, &rex[r]);
        h_scale[r] = std::ldexp(row_scale(r), rex[r]);
        h_shift[r] = row_shift(r);
    }
    const int KS = K / 32, CG = rows / 128;
    std::vector<_Float16> pk((size_t)CG * KS * 16 * 64 * 8);
    for (int cg = 0; cg < CG; ++cg)
        for (int ks = 0; ks < KS; ++ks)
            for (int f = 0; f < 8; ++f)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 15, q = lane >> 4;
                    const int r = cg * 128 + (i / 4) * 32 + f * 4 + (i % 4);
                    for (int j = 0; j < 8; ++j) {
                        const float v = std::ldexp(element(r, ks * 32 + q * 8 + j), -rex[r]);
                        const _Float16 hi = (_Float16)v;
                        const size_t at = ((((size_t)(cg * KS + ks) * 8 + f) * 2) * 64 + lane) * 8 + j;
                        pk[at] = hi;
                        pk[at + 64 * 8] = (_Float16)(v - (float)hi);
                    }
                }
    CV_TRY(wpk.upload(pk.data(), pk.size() * sizeof(_Float16)));
    CV_TRY(scale.alloc((size_t)rows * sizeof(float), false));
    CV_TRY(shift.alloc((size_t)rows * sizeof(float), false));
    on = true;
    return Status();
}

Status Lds1x1::set_exps(int in_exp_, int out_exp_, hipStream_t s) {
    if (in_exp_ == in_exp && out_exp_ == out_exp) return Status();
    CV_TRY(fold_exps(name, h_scale, h_shift, scale.ptr, shift.ptr, in_exp_, out_exp_, s));
    in_exp = in_exp_; out_exp = out_exp_;
    return Status();
}

// the ten forms with weights in dynamic LDS, by (mode, Cin, staged stores)
using LdsKernel = void (*)(const float*, int, int, int, const half8*, const float*, const float*, float*, unsigned*, unsigned, int, int, int);
static const struct { Lds1x1Mode mode; int cin; bool stage; LdsKernel kern; } kLdsForms[] = {
    {kShortcutF32, 64, true, shortcut1x1s2_lds_kernel<64, true>},    {kShortcutF32, 64, false, shortcut1x1s2_lds_kernel<64, false>},
    {kShortcutF32, 128, true, shortcut1x1s2_lds_kernel<128, true>},  {kShortcutF32, 128, false, shortcut1x1s2_lds_kernel<128, false>},
    {kShortcutF32, 256, true, shortcut1x1s2_lds_kernel<256, true>},  {kShortcutF32, 256, false, shortcut1x1s2_lds_kernel<256, false>},
    {kShortcutSplit, 64, true, shortcut1x1s2_lds_kernel<64, true, true>}, {kShortcutSplit, 128, true, shortcut1x1s2_lds_kernel<128, true, true>},
    {kConvT, 128, true, shortcut1x1s2_lds_kernel<128, true, true, true>}, {kConvT, 256, true, shortcut1x1s2_lds_kernel<256, true, true, true>}};

hipError_t conv1x1_lds_prepare() {
    for (const auto& f : kLdsForms) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(f.kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

static hipError_t launch_lds1x1(const Lds1x1& L, Lds1x1Mode mode, const TensorRef& x, const TensorRef& y, unsigned* flag, hipStream_t s) {
    const int cin = x.C;
    long long M;                                        // GEMM pixels
    if (mode == kConvT) {
        const int cout = y.C;
        if ((cin != 128 && cin != 256) || 2 * cout != cin || x.Coff || x.Cs != cin || x.f32_only || y.f32_only || y.H != 2 * x.H || y.W != 2 * x.W ||
            y.N != x.N || y.Coff % 8 || y.Cs % 8 || cout % 8)
            return hipErrorInvalidValue;
        M = (long long)x.N * x.H * x.W;
        if (M <= 0 || (long long)y.N * (y.H + 2) * (y.W + 2) >= (1ll << 32)) return hipErrorInvalidValue;
    } else {
        const bool split = mode == kShortcutSplit;
        if ((!split && (!x.f32_only || !y.f32_only)) || (split && (x.f32_only || y.f32_only)) || x.Coff || y.Coff || x.Cs != x.C || y.Cs != y.C || y.C != 2 * x.C ||
            x.H != 2 * y.H || x.W != 2 * y.W || x.N != y.N)
            return hipErrorInvalidValue;
        M = x.N * y.H * y.W;
    }
    const float* xb = reinterpret_cast<const float*>(x.base);
    float* yb = reinterpret_cast<float*>(y.base);
    const half8* w = reinterpret_cast<const half8*>(L.wpk.ptr);
    const float *scale = reinterpret_cast<const float*>(L.scale.ptr), *shift = reinterpret_cast<const float*>(L.shift.ptr);
    const int cgs = 2 * cin / 128, groups = (int)((M + 15) / 16);
    // the f32-twin shortcut's other two forms, kept as cross-checks of the default one (same bits): CV_SHORTCUT_LDS=0 = first form,
    // CV_SHORTCUT_STAGE=0 = unstaged stores
    static const bool lds_form = [] { const char* v = std::getenv("CV_SHORTCUT_LDS"); return !(v && v[0] == '0'); }();
    static const bool stage_knob = [] { const char* v = std::getenv("CV_SHORTCUT_STAGE"); return !(v && *v) || std::atoi(v) != 0; }();
    if (mode == kShortcutF32 && !lds_form) {
        const dim3 grid((unsigned)((groups * cgs + 3) / 4)), block(256);
        if (cin == 64) hipLaunchKernelGGL(shortcut1x1s2_kernel<64>, grid, block, 0, s, xb, x.N, x.H, x.W, w, scale, shift, yb, flag, L.layer_id);
        else if (cin == 128) hipLaunchKernelGGL(shortcut1x1s2_kernel<128>, grid, block, 0, s, xb, x.N, x.H, x.W, w, scale, shift, yb, flag, L.layer_id);
        else if (cin == 256) hipLaunchKernelGGL(shortcut1x1s2_kernel<256>, grid, block, 0, s, xb, x.N, x.H, x.W, w, scale, shift, yb, flag, L.layer_id);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    const bool stage = mode != kShortcutF32 || stage_knob;
    constexpr int nw = 8;
    int wgx = (256 + cgs - 1) / cgs;                                    // persistent: about one workgroup per CU over all row groups
    if (wgx > (groups + nw - 1) / nw) wgx = (groups + nw - 1) / nw;
    if (wgx < 1) wgx = 1;
    const size_t lds = (size_t)(cin / 32) * 16 * 1024 + 1024 + (stage ? (size_t)nw * ((cin <= 128 ? 16 : 4) * 528 + 64) : 0);   // weights + scale / shift (+ staging)
    for (const auto& f : kLdsForms)
        if (f.mode == mode && f.cin == cin && f.stage == stage) {
            hipLaunchKernelGGL(f.kern, dim3((unsigned)wgx, (unsigned)cgs), dim3(64 * nw), lds, s, xb, x.N, x.H, x.W, w, scale, shift, yb, flag, L.layer_id,
                               y.Cs, y.Coff, y.C);
            return hipGetLastError();
        }
    return hipErrorInvalidValue;
}

Status conv1x1_lds(Engine& e, Lds1x1& L, Lds1x1Mode mode, const TensorRef& x, const TensorRef& y, hipStream_t s) {
    CV_TRY(L.set_exps(x.exp, y.exp, s));
    if (e.profiling) {
        // GEMM pixels x K x rows; tensors at 4 bytes per element (f32 twin | split-f16) + the weights
        const double px = (double)x.N * (mode == kConvT ? x.H * x.W : y.H * y.W), K = x.C, rows = 2 * x.C;
        e.prof_begin(L.name, true, px * K * rows, s, px * (K + rows) * 4.0 + K * rows * 4.0);
        e.prof.back().kernel = (mode == kConvT ? "convt2x2_lds_kernel<" : "shortcut1x1s2_kernel<") + std::to_string(x.C) + (mode == kShortcutF32 ? ">" : ",split>");
    }
    const hipError_t err = launch_lds1x1(L, mode, x, y, e.guard_ptr(), s);
    if (e.profiling) e.prof_end(s);
    if (err != hipSuccess) return hip_fail(err, mode == kConvT ? "convt2x2_lds" : mode == kShortcutSplit ? "shortcut1x1s2 (split)" : "shortcut1x1s2");
    return Status();
}

}  // namespace cv
