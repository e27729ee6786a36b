// conv1x1_lds.h -- the 1x1 GEMM with K = Cin <= 256 as a dedicated split-f16 MFMA kernel (conv1x1_lds.hip): the ResNet stage-boundary
// shortcuts (conv 1x1 / stride 2 + BN; f16r and split-f16 engines) and the UNet k2 / s2 transposed convolutions up3.up / up4.up
// (split-f16 engine).  The generic layer of the same weights (ConvLayer) stays beside it for the calibration passes, small batches
// and the CV_SHORTCUT_FAST=0 / CV_CONVT_FAST=0 cross-checks.
#pragma once
#include <functional>

#include "engine.h"

namespace cv {

// a matrix packed for the kernel + the epilogue constants of its rows
struct Lds1x1 {
    bool on = false;
    std::string name;                               // of the generic layer it stands in for (errors, profile entries)
    DeviceBuffer wpk, scale, shift;
    std::vector<float> h_scale, h_shift;            // per GEMM row: scale with 2^(row exponent) folded in | shift (ConvLayer::h_scale)
    int in_exp = 1 << 20, out_exp = 1 << 20;        // exponents the device copies are folded for
    unsigned layer_id = 0;                          // numeric-guard id
    // Split-f16 image of a rows x K matrix (rows % 128 == 0, K % 32 == 0): rows normalised to [0.5, 1) as ConvLayer rows are
    // (engine.cpp: finish_layer; the exponent goes into the scale), hi / lo halves,
    // [row group of 128][k-step of 32][fragment 8][hi | lo][lane 64][8]; MFMA row i of fragment f = row 32 (i/4) + 4 f + i%4 of the group.
    Status pack(int rows, int K, const std::function<float(int, int)>& element, const std::function<float(int)>& row_scale,
                const std::function<float(int)>& row_shift, const std::string& name_);
    Status set_exps(int in_exp_, int out_exp_, hipStream_t s);   // as ConvLayer::set_exps
};

enum Lds1x1Mode {
    kShortcutF32,       // conv 1x1 / stride 2 between f32 twins (f32_only PHWC tensors; f16r engine), C in {64, 128, 256} -> 2 C
    kShortcutSplit,     // the same between split-f16 tensors, C in {64, 128}: products and their order are conv_igemm_kernel's on split_t
    kConvT              // conv_transpose2d k2 s2 + bias between split-f16 tensors: x (C in {128, 256}, own buffer) -> channel slice y (C/2
};                      // channels, 2H x 2W) of the concatenated tensor; GEMM row = (dy * 2 + dx) * C/2 + co

// folds the tensors' exponents if they changed, then one launch x -> y (with its profile entry when the engine is profiling)
Status conv1x1_lds(Engine& e, Lds1x1& L, Lds1x1Mode mode, const TensorRef& x, const TensorRef& y, hipStream_t s);
hipError_t conv1x1_lds_prepare();                   // raise the dynamic-LDS limits (once per device: cv_engine_create)

}  // namespace cv
