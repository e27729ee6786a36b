// models.h -- per-model state owned by an Engine (packed layers + activation workspace).
#pragma once
#include "conv1x1_lds.h"
#include "engine.h"

namespace cv {

// Workspaces are elastic: a model is loaded with no activation memory beyond what the range calibration needs and
// `reserve(n)` (re)allocates every tensor for min(n, engine chunk) images the first time a batch of that size arrives --
// a single-image server (the reference's Flask endpoint) stays under 1 GB, a throughput job grows once to its chunk.
struct Engine::UNet {
    bool bilinear = false;
    bool fuse_head = true;                          // OutConv fused into up4's last conv epilogue
    int cap = 0;                                    // images the workspace currently holds
    int max_cap = 64;                               // engine chunk: images per pass
    int last_n = 0;                                 // images in the most recent chunk
    // channel plan
    int c1 = 64, c2 = 128, c3 = 256, c4 = 512, c5 = 1024;
    ConvLayer inc0, inc1, d[4][2], upT[4], u[4][2];
    unsigned up_id[4] = {0, 0, 0, 0}, outc_id = 0;  // numeric-guard ids of the non-conv producers
    // split-f16 engine, throughput batches: up3.up / up4.up (K = 256 / 128: the whole weight block fits in LDS) on the persistent
    // LDS-resident-weights kernel (conv1x1_lds.h: kConvT) instead of the generic tile; upT[i] remains for calibration, small
    // batches (CV_CONVT_FAST_MIN) and CV_CONVT_FAST=0; up3.up takes it with CV_CONVT_FAST_256=1 only.  Same products in the same order:
    // bit-identical.  GEMM row (dy, dx, co): scale 1, shift = the bias.
    Lds1x1 fast_up[4];
    DeviceBuffer outc_w, outc_b;
    DeviceBuffer inc0_wpk;                          // f16-based engines: MFMA image of inc.double_conv.0 for the fused first-layer kernel
    DeviceBuffer inc0_wpk2;                         // split-f16: the same layer for the in-kernel producer of inc.double_conv.3 (conv_halo.hip: FUSE0)
    bool fused_inc0 = false;                        // first layer + input packing in one kernel (pointwise.hip: inc0_mfma)
    bool fused_inc = false;                         // first layer produced inside inc.double_conv.3's halo kernel
    // activations
    Activation in8, a_inc0, cat[4], pool[4], dmid[4], bott, umid[4], uout[4];
    std::vector<Activation*> acts;                  // every tensor above that exists in this variant
    std::map<std::string, TensorRef> taps;          // module name -> tensor produced (capacity-sized refs)
    int64_t macs = 0;
};

// timm's plain BasicBlock ResNets: the same stem, stage widths, shortcuts and head; only the number of blocks per stage differs
struct ResNetArch {
    const char* name;
    int depth[4];                                   // BasicBlocks per stage (layer1..layer4)
};
const ResNetArch* resnet_arch(const std::string& name);   // "resnet18" {2,2,2,2} | "resnet34" {3,4,6,3}; null otherwise

struct Engine::ResNet {
    const ResNetArch* arch = nullptr;
    int cap = 0;
    int max_cap = 16384;
    int last_n = 0;
    DeviceBuffer stem_w, stem_wpk, stem_scale, stem_shift, fc_w, fc_b;
    std::vector<float> h_stem_scale, h_stem_shift;  // row exponents of the normalised stem filters folded in (ConvLayer::h_scale)
    int stem_out_exp = 0;                           // exponent the device copies are currently folded for
    unsigned stem_id = 0, head_id = 0;
    struct Block {
        ConvLayer conv1, conv2, down;
        bool has_down = false;
        Activation mid, out, sc;                     // conv1 output, block output, shortcut (if downsampled)
        // f16r: the shortcut convolution as a dedicated split-f16 kernel between the f32 twins (conv1x1_lds.h: kShortcutF32; the f16x3
        // engine takes its kShortcutSplit form from CV_SHORTCUT_SPLIT_MIN squares); `down` (the same layer through the generic kernel)
        // remains for the calibration passes and CV_SHORTCUT_FAST=0.  CV_SHORTCUT_LDS=0 / CV_SHORTCUT_STAGE=0: the f32-twin kernel's
        // first form / unstaged stores (same bits).  GEMM row = output channel: the folded BN affine.
        Lds1x1 fast_sc;
    };
    std::unique_ptr<Block[]> blocks;                // layer1.0 .. layer4.(depth[3]-1), stage by stage
    int nblocks = 0;
    int first[5] = {0, 0, 0, 0, 0};                 // index of stage l's first block (first[4] = nblocks)
    Activation stem_out, pool_out;
    // f16r: the first chain_nb BasicBlocks of layer1 (2 * chain_nb 3x3 convolutions 64 -> 64 on 16 x 16 maps, chain_nb = 2 | 3) as ONE
    // launch with the image resident in LDS (conv_halo.hip: CHAIN).  chain_w = those layers' packed weight stages back to back.
    // CV_RESNET_CHAIN=0 switches it off; CV_RESNET_CHAIN_BLOCKS=2 chains two blocks of a three-block layer1 (the third runs layer by layer).
    DeviceBuffer chain_w;
    bool chain_ok = false;
    int chain_nb = 0;
    std::vector<Activation*> acts;
    std::map<std::string, TensorRef> taps;
    int64_t macs = 0;
};

// x in [0,1] is held as x * 2^7 inside the f16-based engines (both models' inputs)
constexpr int kInputExp = -7;

}  // namespace cv
