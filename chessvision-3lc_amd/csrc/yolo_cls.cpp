// yolo_cls.cpp -- ultralytics YOLOv8-cls (n / s / m / l / x; one input channel, 13 classes) plan: packing + forward schedule.
//
// A reading of yolov8-cls.yaml and of Conv, C2f, Bottleneck and Classify (ultralytics.nn.modules), restated in models.h at
// YoloClsArch; ultralytics itself is not needed.  Every Conv2d + BatchNorm2d(eps 1e-3) + SiLU is one implicit-GEMM launch with the
// SiLU in its epilogue (cv_kernels.h: ConvParams::act_*); a C2f's torch.chunk / torch.cat never move a byte: cv1 and the Bottlenecks
// write channel slices of one tensor and cv2 reads it whole; a Bottleneck's shortcut is its second conv's residual, added after the
// activation (ConvParams::act_first).  The 3-channel repeat of the grey square is folded into the stem's filters at load time.
// All launches are the generic implicit-GEMM family: SiLU does not exist in the halo kernels, and Engine::run_conv never picks them.
// Compiled as part of resnet.cpp, which includes this file at its end (as cv_api.cpp includes the JPEG codec): the host-sanitizer test
// links the library from a fixed list of translation units, and a unit of its own would be missing from that link.
#include <cmath>
#include <cstring>

#include "engine.h"
#include "models.h"
#include "pointwise.h"

namespace cv {

static const YoloClsArch kYoloClsArchs[] = {
    {"yolov8n-cls", {16, 32, 64, 128, 256}, {1, 2, 2, 1}},   {"yolov8s-cls", {32, 64, 128, 256, 512}, {1, 2, 2, 1}},
    {"yolov8m-cls", {48, 96, 192, 384, 768}, {2, 4, 4, 2}},  {"yolov8l-cls", {64, 128, 256, 512, 1024}, {3, 6, 6, 3}},
    {"yolov8x-cls", {80, 160, 320, 640, 1280}, {3, 6, 6, 3}},
};

const YoloClsArch* yolo_cls_arch(const std::string& name) {
    for (const YoloClsArch& a : kYoloClsArchs)
        if (name == a.name) return &a;
    return nullptr;
}

static Status yolo_cls_chunk(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding,
                             const InputNorm* norm);

namespace {
constexpr float kYoloBnEps = 1e-3f;                  // ultralytics: initialize_weights sets it; a state dict does not carry it

// The checkpoint is either as trained (`P.conv.weight` + the four `P.bn.*`) or as model.fuse() leaves it (`P.conv.weight` +
// `P.conv.bias`, the BatchNorm folded in: scale 1, shift = bias).  One form for the whole dict: a mixture is refused.
struct Loader {
    Engine& e;
    const ParamMap& pm;
    bool fused;
    std::vector<std::string> known;

    Status form_of(const std::string& P) const {
        const bool has_bias = pm.count(P + ".conv.bias") != 0;
        bool has_bn = false;
        for (const char* leaf : {".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"}) has_bn = has_bn || pm.count(P + leaf) != 0;
        if ((fused && has_bn) || (!fused && has_bias))
            return fail(1, "state dict mixes fused and unfused layers: '" + P + "' has " + (has_bn && has_bias ? "both a conv bias and BatchNorm keys" : fused ? "BatchNorm keys" : "a conv bias") +
                               " while 'model.0' is " + (fused ? "fused (conv.bias, no bn.*)" : "unfused (bn.*, no conv.bias)"));
        return Status();
    }
    // scale / shift of Conv `P` with `c` output channels
    Status affine(const std::string& P, int c, std::vector<float>& sc, std::vector<float>& sh) {
        CV_TRY(form_of(P));
        known.push_back(P + ".conv.weight");
        if (fused) {
            const float* b;
            CV_TRY(need(pm, P + ".conv.bias", {c}, &b));
            known.push_back(P + ".conv.bias");
            sc.assign(c, 1.f);
            sh.assign(b, b + c);
            return Status();
        }
        bn_keys(known, P + ".bn");
        return bn_fold(pm, P + ".bn", c, sc, sh, kYoloBnEps);
    }
    Status conv(ConvLayer& L, const std::string& P, int cout, int cin, int k, int stride, int64_t pixels, int out_hw) {
        if (!fused) {
            CV_TRY(form_of(P));
            known.push_back(P + ".conv.weight");
            bn_keys(known, P + ".bn");
            return build_conv_bn(e, L, pm, P + ".conv", P + ".bn", cout, cin, k, stride, cin, pixels, out_hw, -1, kYoloBnEps);
        }
        std::vector<float> sc, sh;
        CV_TRY(affine(P, cout, sc, sh));
        const float* w;
        CV_TRY(need(pm, P + ".conv.weight", {cout, cin, k, k}, &w));
        CV_TRY(L.build_conv(P + ".conv", e.dt, w, cout, cin, k, stride, sc.data(), sh.data(), cin, pixels, out_hw));
        L.layer_id = e.register_layer(P + ".conv");
        return Status();
    }
};
}  // namespace

Status yolo_cls_load(Engine& e, const ParamMap& pm, const std::string& arch) {
    const YoloClsArch* A = yolo_cls_arch(arch);
    if (!A) return fail(1, "unknown YOLOv8-cls architecture '" + arch + "' (supported: 'yolov8n-cls', 'yolov8s-cls', 'yolov8m-cls', 'yolov8l-cls', 'yolov8x-cls')");
    if (e.trunk32)
        return fail(1, "precision f16r is not available for a YOLOv8-cls classifier: its f32 residual trunk is ResNet's design -- "
                       "use precision f32, f16x3 or f16");
    auto m = std::make_unique<Engine::YoloCls>();
    Engine::YoloCls& Y = *m;
    Y.arch = A;
    const int dt = e.dt;
    CV_TRY(e.guard_init());
    Loader ld{e, pm, pm.count("model.0.conv.bias") != 0 && pm.count("model.0.bn.weight") == 0, {}};
    const int w0 = A->width[0];
    int64_t macs = 0;

    {   // model.0: Conv(ch, w0, 3, 2); ch = 3 (the reference repeats the grey square) is summed into one channel, ch = 1 taken as is
        const float* w = nullptr;
        auto it = pm.find("model.0.conv.weight");
        if (it == pm.end()) return fail(1, "state dict is missing key 'model.0.conv.weight'");
        const int ch = it->second.shape.size() == 4 ? (int)it->second.shape[1] : 0;
        if (ch != 1 && ch != 3) CV_TRY(need(pm, "model.0.conv.weight", {w0, 3, 3, 3}, &w));      // the shape error, in need()'s words
        CV_TRY(need(pm, "model.0.conv.weight", {w0, ch, 3, 3}, &w));
        std::vector<float> sc, sh;
        CV_TRY(ld.affine("model.0", w0, sc, sh));
        std::vector<float> w1((size_t)w0 * 9);
        for (int co = 0; co < w0; ++co)
            for (int k = 0; k < 9; ++k) {
                double acc = 0.0;                            // float64 sum of the input channels, rounded once
                for (int ci = 0; ci < ch; ++ci) acc += (double)w[((size_t)co * ch + ci) * 9 + k];
                w1[(size_t)co * 9 + k] = (float)acc;
                if (!std::isfinite(w1[(size_t)co * 9 + k])) return fail(1, "model.0.conv: non-finite weight in the state dict");
            }
        for (int co = 0; co < w0; ++co)
            if (!std::isfinite(sc[co]) || !std::isfinite(sh[co])) return fail(1, "model.0: non-finite BatchNorm scale/shift (running_var + eps <= 0?)");
        CV_TRY(Y.stem_w.upload(w1.data(), w1.size() * sizeof(float)));
        CV_TRY(Y.stem_scale.upload(sc.data(), sc.size() * sizeof(float)));
        CV_TRY(Y.stem_shift.upload(sh.data(), sh.size() * sizeof(float)));
        Y.stem_id = e.register_layer("model.0.conv");
        macs += 9LL * w0 * 32 * 32;
    }
    Y.stem_out.shape(32, 32, w0, dt);
    Y.acts.push_back(&Y.stem_out);

    // the workspace's largest tensor stays under the 4 GiB that the convolutions' 32-bit gather offsets address
    Y.max_cap = e.resnet_chunk;
    {
        uint64_t worst = (uint64_t)34 * 34 * w0;
        for (int s = 0; s < 4; ++s) {
            const uint64_t hw = (uint64_t)(16 >> s) + 2;
            worst = std::max(worst, hw * hw * (uint64_t)((2 + A->depth[s]) * (A->width[s + 1] / 2)));
        }
        worst = std::max(worst, (uint64_t)4 * 4 * kYoloHeadC);
        while (worst * 4 * (uint64_t)Y.max_cap >= (1ull << 32) && Y.max_cap > 1) Y.max_cap /= 2;
    }
    const int S = Y.max_cap;

    int cin = w0;
    for (int s = 0; s < 4; ++s) {
        Engine::YoloCls::Stage& St = Y.stage[s];
        const int w = A->width[s + 1], c = w / 2, n = A->depth[s], hw = 16 >> s;
        const int64_t px = (int64_t)S * hw * hw;
        const std::string pd = "model." + std::to_string(2 * s + 1), pc = "model." + std::to_string(2 * s + 2);
        St.n = n; St.c = c; St.hw = hw;
        St.m.reset(new Engine::YoloCls::Bottleneck[n]);
        CV_TRY(ld.conv(St.down, pd, w, cin, 3, 2, px, hw));
        CV_TRY(ld.conv(St.cv1, pc + ".cv1", 2 * c, w, 1, 1, px, hw));
        St.down_out.shape(hw, hw, w, dt);
        St.cat.shape(hw, hw, (2 + n) * c, dt);
        St.out.shape(hw, hw, w, dt);
        Y.acts.push_back(&St.down_out); Y.acts.push_back(&St.cat);
        macs += ((int64_t)9 * cin * w + (int64_t)w * 2 * c) * hw * hw;
        for (int i = 0; i < n; ++i) {
            Engine::YoloCls::Bottleneck& B = St.m[i];
            const std::string pb = pc + ".m." + std::to_string(i);
            CV_TRY(ld.conv(B.cv1, pb + ".cv1", c, c, 3, 1, px, hw));
            CV_TRY(ld.conv(B.cv2, pb + ".cv2", c, c, 3, 1, px, hw));
            B.mid.shape(hw, hw, c, dt);
            Y.acts.push_back(&B.mid);
            macs += 2 * (int64_t)9 * c * c * hw * hw;
        }
        CV_TRY(ld.conv(St.cv2, pc + ".cv2", w, (2 + n) * c, 1, 1, px, hw));
        Y.acts.push_back(&St.out);
        macs += (int64_t)(2 + n) * c * w * hw * hw;
        cin = w;
    }
    CV_TRY(ld.conv(Y.head_conv, "model.9.conv", kYoloHeadC, cin, 1, 1, (int64_t)S * 4, 2));
    Y.head_out.shape(2, 2, kYoloHeadC, dt);
    Y.acts.push_back(&Y.head_out);
    macs += (int64_t)cin * kYoloHeadC * 4;
    {
        const float *w, *b;
        CV_TRY(need(pm, "model.9.linear.weight", {13, kYoloHeadC}, &w));
        CV_TRY(need(pm, "model.9.linear.bias", {13}, &b));
        ld.known.push_back("model.9.linear.weight"); ld.known.push_back("model.9.linear.bias");
        for (int i = 0; i < 13 * kYoloHeadC; ++i)
            if (!std::isfinite(w[i])) return fail(1, "model.9.linear: non-finite weight in the state dict");
        for (int i = 0; i < 13; ++i)
            if (!std::isfinite(b[i])) return fail(1, "model.9.linear: non-finite bias in the state dict");
        CV_TRY(Y.fc_w.upload(w, (size_t)13 * kYoloHeadC * sizeof(float)));
        CV_TRY(Y.fc_b.upload(b, 13 * sizeof(float)));
        Y.head_id = e.register_layer("model.9.linear");
        macs += 13 * kYoloHeadC;
    }
    CV_TRY(reject_unknown_keys(pm, ld.known, (std::string(A->name) + " (13 classes)").c_str()));
    Y.macs = macs;

    std::unique_ptr<Engine::YoloCls> previous = std::move(e.yolo);
    e.yolo = std::move(m);
    Status st = model_reserve(e, Y, 128);
    if (st.ok() && dt != kF32 && calibration_enabled()) {
        constexpr int kCal = 128, kBias = 256;
        std::vector<float> host;
        classifier_calibration_squares(host, kCal, kBias);
        DeviceBuffer xin;
        st = xin.upload(host.data(), host.size() * sizeof(float));
        std::vector<ConvLayer*> layers;                      // the f16 layers of the rounding-bias pass
        for (Engine::YoloCls::Stage& St : Y.stage) {
            layers.push_back(&St.down); layers.push_back(&St.cv1);
            for (int i = 0; i < St.n; ++i) { layers.push_back(&St.m[i].cv1); layers.push_back(&St.m[i].cv2); }
            layers.push_back(&St.cv2);
        }
        layers.push_back(&Y.head_conv);
        if (st.ok())
            st = calibrate_model(e, Y, layers, (const float*)xin.ptr, 4096, kCal, kBias, 13, A->name,
                                 [&](const float* x, int n, float* out) { return yolo_cls_chunk(e, x, false, n, out, false, nullptr, nullptr, nullptr); });
    }
    if (!st.ok()) e.yolo = std::move(previous);
    else e.resnet.reset();                                   // the classifier slot holds one model
    return st;
}

void Engine::YoloCls::build_taps(const Engine&, int S) {
    taps["model.0"] = stem_out.ref(S);
    for (int s = 0; s < 4; ++s) {
        Stage& St = stage[s];
        const std::string pc = "model." + std::to_string(2 * s + 2);
        taps["model." + std::to_string(2 * s + 1)] = St.down_out.ref(S);
        taps[pc + ".cv1"] = St.cat.ref(S, 0, 2 * St.c);
        for (int i = 0; i < St.n; ++i) {
            taps[pc + ".m." + std::to_string(i) + ".cv1"] = St.m[i].mid.ref(S);
            taps[pc + ".m." + std::to_string(i)] = St.cat.ref(S, (2 + i) * St.c, St.c);
        }
        taps[pc] = St.out.ref(S);
    }
    taps["model.9.conv"] = head_out.ref(S);
}

Status yolo_cls_activation(Engine& e, const std::string& name, TensorRef* out) {
    if (!e.yolo) return fail(3, "YOLOv8-cls not loaded");
    if (!e.yolo->tap(name, out)) return fail(1, "unknown " + std::string(e.yolo->arch->name) + " activation '" + name + "'");
    return Status();
}

static Status yolo_cls_chunk(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding,
                             const InputNorm* norm) {
    Engine::YoloCls& Y = *e.yolo;
    const int dt = e.dt;
    const double esz = dtype_size(dt);
    const int w0 = Y.arch->width[0];
    e.timed_begin("stem3x3s2", s, (double)n * (4096 * (x_u8 ? 1.0 : 4.0) + 1024 * w0 * esz), 9.0 * w0 * 1024 * n);
    CV_TRY(e.timed_end("stem3x3s2", stem3x3s2(dt, x, x_u8, n, (const float*)Y.stem_w.ptr, (const float*)Y.stem_scale.ptr,
                                              (const float*)Y.stem_shift.ptr, Y.stem_out.ref(n), e.guard_ptr(), Y.stem_id, s, norm), s));
    if (e.calibrating) CV_TRY(e.measure(Y.stem_out.ref(n), s));
    TensorRef cur = Y.stem_out.ref(n);
    for (Engine::YoloCls::Stage& St : Y.stage) {
        const int c = St.c;
        CV_TRY(e.run_conv(St.down, cur, St.down_out.ref(n), nullptr, kActSilu, s));
        CV_TRY(e.run_conv(St.cv1, St.down_out.ref(n), St.cat.ref(n, 0, 2 * c), nullptr, kActSilu, s));
        for (int i = 0; i < St.n; ++i) {
            const TensorRef in = St.cat.ref(n, (1 + i) * c, c);
            CV_TRY(e.run_conv(St.m[i].cv1, in, St.m[i].mid.ref(n), nullptr, kActSilu, s));
            // x + cv2(cv1(x)): the SiLU first, then the shortcut, nothing after the add
            CV_TRY(e.run_conv(St.m[i].cv2, St.m[i].mid.ref(n), St.cat.ref(n, (2 + i) * c, c), &in, kActSilu, s, nullptr, nullptr, nullptr, true));
        }
        CV_TRY(e.run_conv(St.cv2, St.cat.ref(n), St.out.ref(n), nullptr, kActSilu, s));
        cur = St.out.ref(n);
    }
    CV_TRY(e.run_conv(Y.head_conv, cur, Y.head_out.ref(n), nullptr, kActSilu, s));
    // the pooled model.9.conv output -- the linear layer's input -- is the embedding; the head kernel has it in registers
    float* const pooled = e.calibrating ? nullptr : embedding;
    e.timed_begin("head_pool_fc", s, (double)n * (4 * kYoloHeadC * esz + 13 * 4 + (pooled ? kYoloHeadC * 4 : 0)), 13.0 * kYoloHeadC * n);
    return e.timed_end("head_pool_fc", head_pool_fc(dt, Y.head_out.ref(n), (const float*)Y.fc_w.ptr, (const float*)Y.fc_b.ptr, out, pooled,
                                                    softmax ? 1 : 0, e.guard_ptr(), Y.head_id, s), s);
}

Status yolo_cls_forward(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding,
                        const InputNorm* norm) {
    if (!e.yolo) return fail(3, "YOLOv8-cls weights not loaded (call cv_load_yolo_cls first)");
    if (norm && !x_u8) return fail(1, "yolo_cls_forward: only a byte input can be normalised");
    Engine::GraphKey key;
    key.flags = (x_u8 ? 1 : 0) | (softmax ? 2 : 0) | (norm ? 4 : 0);
    if (norm) std::memcpy(key.norm_bits, norm, sizeof(key.norm_bits));
    const ForwardShape shape{512, (size_t)64 * 64 * (x_u8 ? 1 : 4), 13, (size_t)kYoloHeadC};
    return forward_chunked(e, *e.yolo, shape, key, "cv_resnet18_forward", x, n, out, nullptr, embedding, s,
                           [&](const void* xc, int c, float* o, uint8_t*, float* emb, hipStream_t st) {
                               return yolo_cls_chunk(e, xc, x_u8, c, o, softmax, st, emb, norm);
                           });
}

// ---- the classifier slot: a ResNet or a YOLOv8-cls ---------------------------------------------------------------------------------
const char* classifier_name(const Engine& e) { return e.yolo ? e.yolo->arch->name : e.resnet ? e.resnet->arch->name : nullptr; }
ModelBase* classifier_model(Engine& e) { return e.yolo ? (ModelBase*)e.yolo.get() : (ModelBase*)e.resnet.get(); }
int classifier_embedding_dim(const Engine& e) { return e.yolo ? kYoloHeadC : e.resnet ? 512 : 0; }
const char* classifier_pool_tap(const Engine& e) { return e.yolo ? "model.9.conv" : "layer4"; }
Status classifier_forward(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding,
                          const InputNorm* norm) {
    return e.yolo ? yolo_cls_forward(e, x, x_u8, n, out, softmax, s, embedding, norm) : resnet_forward(e, x, x_u8, n, out, softmax, s, embedding, norm);
}
Status classifier_activation(Engine& e, const std::string& name, TensorRef* out) {
    return e.yolo ? yolo_cls_activation(e, name, out) : resnet_activation(e, name, out);
}
int64_t classifier_macs(Engine& e) { return e.yolo ? e.yolo->macs : resnet_macs(e); }

}  // namespace cv
