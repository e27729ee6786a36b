// models.h -- per-model state owned by an Engine (packed layers + activation workspace), and what the two model plans share:
// state-dict helpers, packing arithmetic, the elastic workspace, load-time calibration and the chunked forward driver.
#pragma once
#include <algorithm>

#include "conv1x1_lds.h"
#include "engine.h"

namespace cv {

// ---- state dict -> layers (engine.cpp) -----------------------------------------------------------------------------------------
Status need(const ParamMap& pm, const std::string& key, std::vector<int64_t> shape, const float** out);
// BatchNorm2d(eval): y = (x - mean) / sqrt(var + eps) * gamma + beta  ->  scale, shift
// (eps: torch's default 1e-5; ultralytics sets 1e-3 and a state dict does not carry it)
Status bn_fold(const ParamMap& pm, const std::string& prefix, int c, std::vector<float>& scale, std::vector<float>& shift, float eps = 1e-5f);
Status build_conv_bn(Engine& e, ConvLayer& L, const ParamMap& pm, const std::string& conv_key, const std::string& bn_key, int cout,
                     int cin, int k, int stride, int cinPad, int64_t pixels, int out_hw = 0, int layer_dt = -1, float bn_eps = 1e-5f);
void bn_keys(std::vector<std::string>& out, const std::string& p);       // appends the four keys of BatchNorm2d `p`
// `known` = every key the architecture defines, so that a checkpoint of a DIFFERENT architecture (extra / renamed keys: the
// reference's UNet is an un-vendored submodule on an `experimental` branch) is rejected instead of half-loaded
Status reject_unknown_keys(const ParamMap& pm, const std::vector<std::string>& known, const char* model);

// ---- packing arithmetic shared by ConvLayer rows and the three hand-laid MFMA images (stem, inc0, inc0 inside inc.double_conv.3) ---
// Row normalisation (f16 / split-f16): a weight row is stored as w * 2^-e with max |w| in [0.5, 1) and 2^e goes into the f32 epilogue
// scale -- exact, and it keeps the lo halves of small trained weights out of the f16 subnormals.
int row_exponent(const float* row, int n);          // e = frexp exponent of the row's largest magnitude; 0 for an all-zero row
int normalise_row(float* row, int n);               // row *= 2^-e in place; returns e
// hi / lo halves of a split-f16 value: hi = v rounded to f16, lo = the rounded remainder
inline _Float16 f16_half(float v, bool lo) {
    const _Float16 hi = (_Float16)v;
    return lo ? (_Float16)(v - (float)hi) : hi;
}
// MFMA row i (0..15) of 16-row fragment f, of nfrag fragments -> channel: the lane that owns rows 4q..4q+3 of every fragment ends up
// with 4 * nfrag consecutive channels (the conv epilogues' lane-contiguous order)
inline int frag_row_channel(int nfrag, int f, int i) { return 4 * nfrag * (i / 4) + 4 * f + i % 4; }

// ---- what both plans hold ----------------------------------------------------------------------------------------------------------
// Workspaces are elastic: a model is loaded with no activation memory beyond what the range calibration needs and
// `model_reserve` (re)allocates every tensor for min(n, engine chunk) items the first time a batch of that size arrives --
// a single-image server (the reference's Flask endpoint) stays under 1 GB, a throughput job grows once to its chunk.
struct ModelBase {
    int slot = 0;                                   // 0 = UNet, 1 = the classifier (ResNet | YOLOv8-cls): Engine::order_forward / ws_slot, GraphKey::model
    int cap = 0;                                    // items (images / squares) the workspace currently holds
    int max_cap = 0;                                // engine chunk: items per pass
    int last_n = 0;                                 // items in the most recent chunk
    std::vector<Activation*> acts;                  // every activation tensor that exists in this variant
    std::map<std::string, TensorRef> taps;          // module name -> tensor produced (capacity-sized refs)
    int64_t macs = 0;                               // algorithmic multiply-accumulates per item
    virtual ~ModelBase() = default;
    virtual void build_taps(const Engine& e, int S) = 0;   // fills `taps` for a workspace of S items (names follow the state-dict prefixes)
    bool tap(const std::string& name, TensorRef* out) const;   // the named tensor as the last chunk left it; false: no such tap
};
// (re)allocate the workspace for min(n, chunk) items; exponents survive, module taps are rebuilt
Status model_reserve(Engine& e, ModelBase& M, int n);

struct Engine::UNet : ModelBase {
    bool bilinear = false;
    bool fuse_head = true;                          // OutConv fused into up4's last conv epilogue
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
    void build_taps(const Engine& e, int S) override;
};

// timm's plain BasicBlock ResNets: the same stem, stage widths, shortcuts and head; only the number of blocks per stage differs
struct ResNetArch {
    const char* name;
    int depth[4];                                   // BasicBlocks per stage (layer1..layer4)
};
const ResNetArch* resnet_arch(const std::string& name);   // "resnet18" {2,2,2,2} | "resnet34" {3,4,6,3}; null otherwise

struct Engine::ResNet : ModelBase {
    ResNet() { slot = 1; }
    const ResNetArch* arch = nullptr;
    DeviceBuffer stem_w, stem_wpk, stem_scale, stem_shift, fc_w, fc_b;
    std::vector<float> h_stem_scale, h_stem_shift;  // row exponents of the normalised stem filters folded in (ConvLayer::h_scale)
    int stem_out_exp = 1 << 20;                     // exponent the device copies are currently folded for (no tensor carries this one)
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
    void build_taps(const Engine& e, int S) override;
};

// ultralytics YOLOv8-cls (yolov8-cls.yaml; Conv, C2f, Bottleneck, Classify of ultralytics.nn.modules), one input channel, 13 classes:
//   model.0 Conv(1, w0, 3, 2)  model.1 Conv(w0, w1, 3, 2)  model.2 C2f(w1, n0)  model.3 Conv(w1, w2, 3, 2)  model.4 C2f(w2, n1)
//   model.5 Conv(w2, w3, 3, 2)  model.6 C2f(w3, n2)  model.7 Conv(w3, w4, 3, 2)  model.8 C2f(w4, n3)
//   model.9 Classify: Conv(w4, 1280, 1) -> average pool -> Linear(1280, 13)
// Conv = Conv2d(bias=False) + BatchNorm2d(eps=1e-3) + SiLU.  C2f(w, n), c = w / 2: cv1 = Conv(w, 2c, 1) fills channels [0, 2c) of ONE
// (2 + n) c-channel tensor; Bottleneck i reads [(1+i)c, (2+i)c), writes [(2+i)c, (3+i)c) = input + Conv(c,c,3)(Conv(c,c,3)(input)) -- the add
// AFTER the SiLU, nothing after the add; cv2 = Conv((2+n)c, w, 1) reads the whole tensor.  The five scales differ in widths and depths.
struct YoloClsArch {
    const char* name;                               // "yolov8n-cls" ... "yolov8x-cls"
    int width[5];                                   // w0 .. w4
    int depth[4];                                   // Bottlenecks of the four C2f
};
const YoloClsArch* yolo_cls_arch(const std::string& name);    // null: not one of the five
constexpr int kYoloHeadC = 1280;

struct Engine::YoloCls : ModelBase {
    YoloCls() { slot = 1; }
    const YoloClsArch* arch = nullptr;
    DeviceBuffer stem_w, stem_scale, stem_shift, fc_w, fc_b;      // model.0 (float32 kernel, true BN constants), model.9.linear
    unsigned stem_id = 0, head_id = 0;
    struct Bottleneck { ConvLayer cv1, cv2; Activation mid; };
    struct Stage {                                  // model.(2s+1) and model.(2s+2)
        ConvLayer down, cv1, cv2;
        std::unique_ptr<Bottleneck[]> m;
        int n = 0, c = 0, hw = 0;
        Activation down_out, cat, out;              // model.(2s+1); the (2+n)c-channel concat tensor (one exponent); model.(2s+2)
    };
    Stage stage[4];
    ConvLayer head_conv;                            // model.9.conv
    Activation stem_out, head_out;
    void build_taps(const Engine& e, int S) override;
};

// x in [0,1] is held as x * 2^7 inside the f16-based engines (both models' inputs)
constexpr int kInputExp = -7;

// The classifier slot holds a ResNet or a YOLOv8-cls; what the C ABI's classifier entries need of whichever is loaded.
// classifier_calibration_squares: the loaders' calibration batch, n_range + n_bias squares of 64 x 64 floats in [0, 1] -- noise, flat grey
// levels, ramps and checkers for the ranges, then noise and smooth bilinear fields for the rounding-bias pass (resnet.cpp).
void classifier_calibration_squares(std::vector<float>& host, int n_range, int n_total);
const char* classifier_name(const Engine& e);                 // architecture name of the loaded classifier, or null
ModelBase* classifier_model(Engine& e);
int classifier_embedding_dim(const Engine& e);                // 512 | 1280 | 0: none loaded
const char* classifier_pool_tap(const Engine& e);             // the tensor whose channel means are the embedding: "layer4" | "model.9.conv"
Status classifier_forward(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding = nullptr,
                          const InputNorm* norm = nullptr);
Status classifier_activation(Engine& e, const std::string& name, TensorRef* out);
int64_t classifier_macs(Engine& e);
Status yolo_cls_load(Engine& e, const ParamMap& pm, const std::string& arch);
Status yolo_cls_forward(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding = nullptr,
                        const InputNorm* norm = nullptr);
Status yolo_cls_activation(Engine& e, const std::string& name, TensorRef* out);

// ---- chunks, load-time calibration, the forward driver -----------------------------------------------------------------------------
// chunk(offset, count) over n items, at most the workspace's capacity at a time
template <class Chunk>
Status for_chunks(Engine& e, ModelBase& M, int n, Chunk&& chunk) {
    for (int off = 0; off < n; off += M.cap) {
        M.last_n = std::min(M.cap, n - off);
        e.ws_slot = M.slot;
        CV_TRY(chunk(off, M.last_n));
    }
    return Status();
}

// Load-time calibration of the f16-based engines on a batch the loader generated and uploaded (x: device, x_stride floats per item):
// the ranges of every activation on the first n_range items (Engine::calibrate; the statistics accumulate over the chunks), then --
// exponents final -- the rounding bias of the f16 `layers` on the first n_bias, then a device synchronise.  chunk(x, n, out) runs one
// chunk into a scratch output of out_stride floats per item.
template <class Chunk>
Status calibrate_model(Engine& e, ModelBase& M, const std::vector<ConvLayer*>& layers, const float* x, size_t x_stride, int n_range,
                       int n_bias, size_t out_stride, const char* what, Chunk&& chunk) {
    DeviceBuffer out;
    CV_TRY(out.alloc((size_t)std::max(n_range, n_bias) * out_stride * sizeof(float), false));
    auto pass = [&](int n) {
        return for_chunks(e, M, n, [&](int off, int c) { return chunk(x + off * x_stride, c, (float*)out.ptr + off * out_stride); });
    };
    CV_TRY(e.calibrate(M.acts, [&] { return pass(n_range); }, nullptr, what));
    CV_TRY(e.calibrate_rounding_bias(layers, [&] { return pass(n_bias); }, nullptr));
    const hipError_t he = device_synchronize();
    return he != hipSuccess ? hip_fail(he, (std::string(what) + " calibration").c_str()) : Status();
}

// what differs between the two networks' forwards: the largest one-chunk batch that replays as a hipGraph, bytes per item of the
// input, floats per item of the output (a mask holds one byte per output element) and of the embedding
struct ForwardShape { int graph_max; size_t x_stride, out_stride, emb_stride; };
// n items through chunk(x, n, out, mask, emb, stream): argument check (`entry` names the caller), stream order, workspace, then ONE small
// chunk through a captured graph (`key` arrives with the entry's flags / threshold / normalisation) or the chunk loop
template <class Chunk>
Status forward_chunked(Engine& e, ModelBase& M, const ForwardShape& f, Engine::GraphKey key, const char* entry, const void* x, int n,
                       float* out, uint8_t* mask, float* emb, hipStream_t s, Chunk&& chunk) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(1, std::string(entry) + ": null tensor or negative batch");
    if (n == 0) return Status();
    CV_TRY(e.order_forward(M.slot, s));
    CV_TRY(model_reserve(e, M, n));
    if (n > M.cap || n > f.graph_max)
        return for_chunks(e, M, n, [&](int off, int c) {
            return chunk((const char*)x + off * f.x_stride, c, out + off * f.out_stride, mask ? mask + off * f.out_stride : nullptr,
                         emb ? emb + off * f.emb_stride : nullptr, s);
        });
    key.model = M.slot; key.n = n; key.x = x; key.out = out; key.mask = mask; key.emb = emb;
    M.last_n = n;                                    // a replay skips the chunk's host side: what cv_get_activation reports and the
    e.ws_slot = M.slot;                              // split-K buffer in use must not depend on whether this call replayed
    return e.run_graphed(key, s, [&](hipStream_t st) { return chunk(x, n, out, mask, emb, st); });
}

}  // namespace cv
