// pointwise.h -- host interface of the bandwidth-bound kernels (pointwise.hip).  `dt` is a cv::DType.
#pragma once
#include <hip/hip_runtime.h>
#include "cv_kernels.h"

namespace cv {

// NCHW float32 (n, c, h, w) -> PHWC slice `dst` (dst.C >= c; channels [c, dst.C) are written as zero)
// Range scaling: a TensorRef carries `exp` (stored = real * 2^-exp); packers multiply by 2^-dst.exp, readers that leave the
// internal layout by 2^src.exp -- powers of two, so exact.  `flag` / `layer_id`: numeric guard (cv_kernels.h), nullable.
hipError_t pack_nchw_f32(int dt, const float* src, int c, const TensorRef& dst, unsigned* flag, hipStream_t s);
// (n, h, w, 3) uint8 -> PHWC slice with value/255 (core.py:215); dst.C == 8, channels 3..7 zero
hipError_t pack_hwc3_u8(int dt, const uint8_t* src, const TensorRef& dst, hipStream_t s);
// PHWC slice -> NCHW float32
hipError_t unpack_nchw_f32(int dt, const TensorRef& src, float* dst, hipStream_t s);

hipError_t maxpool2x2(int dt, const TensorRef& src, const TensorRef& dst, hipStream_t s);
hipError_t maxpool3x3s2(int dt, const TensorRef& src, const TensorRef& dst, hipStream_t s);
hipError_t upsample_bilinear2x(int dt, const TensorRef& src, const TensorRef& dst, unsigned* flag, unsigned layer_id,
                               hipStream_t s);
// max |stored value| of the slice, as float bits (>= 0x7f800000: a non-finite value is present); *out must start at 0
hipError_t absmax(int dt, const TensorRef& src, unsigned* out, hipStream_t s);

// Embeddings: per-image channel means of a stored tensor, out[n][c] (float32, row-major src.N x src.C, 16-byte aligned) =
// 2^src.exp * mean over the H x W interior of elem(n, y, x, c) -- what 3LC's EmbeddingsMetricsCollector keeps of a hooked (B, C, H, W)
// output.  src.f32_only: read as f32 whatever `dt` says.  src.C a multiple of 8, src.Coff of the dtype's group; a slice across both
// halves of a concatenated buffer (src.split) is refused.  The summation order depends on (H, W) only: an image's row is
// bit-identical for every N and every position in the batch.  Asynchronous on `s`; allocates nothing.
hipError_t channel_means(int dt, const TensorRef& src, float* out, hipStream_t s);

// rounding-bias calibration: out[slice][tap][c] (double, slices x k*k x src.C) = sum of the stored f16 input under tap (ky, kx) over
// the slice's images and all Ho x Wo output positions of a k x k / stride / pad (k-1)/2 convolution (f16 tensors only)
hipError_t tap_sums_f16(const TensorRef& src, int Ho, int Wo, int stride, int k, int slices, double* out, hipStream_t s);

// 1x1 conv C -> 1 (+bias): logits (n,1,h,w) float32; mask (nullable) = sigmoid(logit) > thr ? 255 : 0
hipError_t outc_1x1(int dt, const TensorRef& src, const float* w, const float* bias, float* logits,
                    uint8_t* mask, float threshold, unsigned* flag, unsigned layer_id, hipStream_t s);

// ResNet stem: conv 7x7 s2 p3 (1 -> 64, no bias) + BN affine + ReLU.  x: (n,1,64,64) f32 or (n,64,64) u8
// (u8 is scaled by /255 first, core.py:237; then normalised when `norm` is given -- u8 only, cv_kernels.h: InputNorm).  w: [64][49] f32, scale/shift [64].
// dst: 64 ch @ 32x32.
hipError_t stem7x7(int dt, const void* x, bool x_is_u8, int n, const float* w, const float* scale,
                   const float* shift, const TensorRef& dst, hipStream_t s, const InputNorm* norm = nullptr);

// Fused stem for the f16 / split-f16 engines: conv 7x7 s2 p3 + BN + ReLU + max_pool2d(3,2,1) on the MFMA.
// wpk: packed filter bank [hi|lo][k-step 2][fragment 4][lane 64] x half8 (packed by resnet.cpp: resnet_load).  dst: 64 ch @ 16x16.
// in_exp: the input plane is held as x * 2^-in_exp inside the kernel (x in [0,1] -> in_exp = -7 keeps the lo halves normal)
hipError_t stem_pool_mfma(int dt, const void* x, bool x_is_u8, int n, const void* wpk, const float* scale,
                          const float* shift, int in_exp, const TensorRef& dst, unsigned* flag, unsigned layer_id,
                          hipStream_t s, const InputNorm* norm = nullptr);

// UNet first layer for the f16 / split-f16 engines, fused with the input packing: conv 3x3 p1 (3 -> 64) + BN + ReLU straight from
// the caller's image (x: (n,3,256,256) f32 or (n,256,256,3) u8, scaled by /255).  wpk: [hi|lo][fragment 4][lane 64] x half8
// (packed by unet.cpp: unet_load), k = (ky*3 + kx)*3 + c.  dst: 64 ch @ 256x256, whole buffer (Cs == 64).
hipError_t inc0_mfma(int dt, const void* x, bool x_is_u8, int n, const void* wpk, const float* scale, const float* shift,
                     int in_exp, const TensorRef& dst, unsigned* flag, unsigned layer_id, hipStream_t s);

// global average pool + Linear(C -> 13) (+ optional softmax).  w: [13][C] f32, b: [13]
hipError_t head_avgpool_fc(int dt, const TensorRef& src, const float* w, const float* b, float* out,
                           int softmax, unsigned* flag, unsigned layer_id, hipStream_t s);
hipError_t softmax13(const float* logits, int n, float* probs, hipStream_t s);

// YOLOv8-cls stem: conv 3x3 s2 p1 (1 -> dst.C, no bias) + BN affine + SiLU, float32 arithmetic in every engine.  x as stem7x7's
// (float, u8 scaled by /255, u8 normalised); w: [dst.C][9] f32 (the checkpoint's three input channels summed), scale / shift: [dst.C]
// TRUE constants (no range factors: 2^-dst.exp is applied after the SiLU).  dst: the whole 32 x 32 tensor, dst.C a multiple of 8.
hipError_t stem3x3s2(int dt, const void* x, bool x_is_u8, int n, const float* w, const float* scale, const float* shift,
                     const TensorRef& dst, unsigned* flag, unsigned layer_id, hipStream_t s, const InputNorm* norm = nullptr);
// head_avgpool_fc for any channel count that is a multiple of 8 (YOLOv8-cls: 1280): global average pool + Linear(C -> 13)
// (+ optional softmax); pooled (nullable, (n, C) float32, 16-byte aligned) receives the pooled features.  w: [13][C] f32, b: [13]
hipError_t head_pool_fc(int dt, const TensorRef& src, const float* w, const float* b, float* out, float* pooled, int softmax,
                        unsigned* flag, unsigned layer_id, hipStream_t s);

// Board-extraction quality scores (the per-image reductions behind the reference's `confidence` and `distribution` columns,
// scripts/process_new_raw/process_pipeline.py:357-377, 460-467).  values: n images of `count` contiguous float32 (4 <= count <= 2^24);
// transform 0 scores them as given, 1 scores v = 1 / (1 + __expf(-x)) (outc_1x1's mask expression).  One record per image:
//   hist       np.histogram(v, bins=10, range=(0, 1)) of a float32 array: float32 edges 0.f, 0.1f, .. 1.f, e[i] <= v < e[i+1], v == 1 in
//              the last bin, NaN / inf / anything outside [0, 1] dropped
//   above_half number of v > 0.5f;  n_nan: number of NaNs
//   top_sum    sum of fabsf(v - 0.5f) over the top_count = count / 4 largest values, selected exactly (ties at the smallest selected
//              value t contribute (top_count - number of values > t) * |t - 0.5|), accumulated in float64 in a fixed order
// half_mask (nullable, n x count uint8) = v > 0.5f ? 255 : 0.  Asynchronous on `s`; allocates nothing.
struct ScoreRecord {
    int32_t hist[10];
    int32_t above_half, n_nan;
    double  top_sum;
    int32_t top_count, reserved;
};
static_assert(sizeof(ScoreRecord) == 64, "one 64-byte record per image");
hipError_t extraction_scores(const float* values, int n, int count, int transform, ScoreRecord* records, uint8_t* half_mask,
                             hipStream_t s);

// Segmentation scores against a label mask (the per-image reductions behind the reference's LossCollector column, scripts/train/
// unet_loss_collector.py:19-48, and train_unet.py's val_dice).  logits: n images of `count` contiguous float32 (4-byte aligned, 1 <=
// count <= 2^24); labels: n x count uint8, any alignment, "board" iff the byte is non-zero; threshold finite.  One record per image:
//   n_label / n_pred / n_both   label bytes != 0 / pixels with v > threshold, v = 1 / (1 + __expf(-x)) (outc_1x1's mask expression) / both
//   n_nan                       NaN logits (each of them turns the three sums NaN)
//   bce_sum                     float64 sum of the float32 terms max(x, 0) - x * t + log1pf(expf(-|x|)), t in {0, 1}
//   sig_sum, sig_label_sum      float64 sums of v over all pixels / over the label pixels
// Sums run in a fixed order (lane, wave shuffle tree, waves in order): bit-identical run to run.  Asynchronous on `s`; allocates nothing.
struct SegRecord {
    int32_t n_label, n_pred, n_both, n_nan;
    double  bce_sum, sig_sum, sig_label_sum;
    int32_t count, reserved[5];
};
static_assert(sizeof(SegRecord) == 64, "one 64-byte record per image");
hipError_t segmentation_scores(const float* logits, const uint8_t* labels, int n, int count, float threshold, SegRecord* records,
                               hipStream_t s);

// Threshold levels: every mask of a threshold grid and every grid point's segmentation counts from one sweep over the logits (the
// reference sweeps `--threshold`, scripts/eval/evaluate.py, scripts/plot_sweep.py).  logits: n images of `count` contiguous float32
// (4-byte aligned, 1 <= count <= 2^24); labels: n x count uint8, any alignment, "board" iff non-zero, or null = no labels;
// thresholds: n_thresholds float32 on the HOST (read before the call returns), in [0, 1], strictly ascending, 1 <= n_thresholds <= 32.
//   levels[i]   #{k : v > thresholds[k]}, v = 1 / (1 + __expf(-x)) (outc_1x1's mask expression): the mask at thresholds[k] is
//               (level > k); a NaN logit gives 0.  n x count uint8, any alignment.
//   record      hist[b][l] = pixels at level l whose label byte is zero (b = 0; all pixels without labels) / non-zero (b = 1)
// Integer counts only: bit-identical run to run.  Asynchronous on `s`; allocates nothing.
constexpr int kMaxLevelThresholds = 32;
struct LevelThresholds { float t[kMaxLevelThresholds]; };
struct LevelRecord {
    int32_t count, n_thresholds, n_nan;
    int32_t hist[2][kMaxLevelThresholds + 1];
    int32_t reserved[11];
};
static_assert(sizeof(LevelRecord) == 320, "one 320-byte record per image");
hipError_t threshold_levels(const float* logits, const uint8_t* labels, int n, int count, const float* thresholds, int n_thresholds,
                            uint8_t* levels, LevelRecord* records, hipStream_t s);

// Per-square records of the classifier's validation pass (train_classifier.py: validate(), the classification collector).  logits:
// n rows of 13 float32 on the device; labels: n int8 on the device (0..12, -1 = unlabelled), or null = all unlabelled.  One thread per
// row, everything in float32 with expf / logf, sums in ascending class order.  The fields are documented at cv_square_record_t
// (include/chessvision_hip.h), whose layout this is.  Asynchronous on `s`; allocates nothing; one launch for any n >= 1.
struct SquareRecord {
    int32_t predicted, rank, label, flags;
    float   confidence, loss, max_logit, logsumexp;
};
static_assert(sizeof(SquareRecord) == 32, "one 32-byte record per square");
hipError_t square_records(const float* logits, const int8_t* labels, int n, SquareRecord* records, hipStream_t s);

// MFMA lane-map probes used by cv_selftest_mfma (D = A*B^T with A:16xK, B:16xK row-major)
hipError_t mfma_probe_f16(const half_t* a, const half_t* b, float* d, hipStream_t s);   // K = 32
hipError_t mfma_probe_f32(const float* a, const float* b, float* d, hipStream_t s);     // K = 16

}  // namespace cv
