// unet.cpp -- UNet(3 -> 1) plan: packing from the reference state dict + the forward schedule.
//
// Follows the module tree the reference constructs at chessvision/core.py:88 (layout: SURVEY.md Appendix A):
//   inc -> down1..4 (MaxPool2d(2) + DoubleConv) -> up1..4 (ConvTranspose2d k2 s2 | bilinear x2, cat([skip, up]),
//   DoubleConv) -> outc (1x1).
// MI355X-first differences from the torch graph: BN+ReLU live in the conv epilogues; `torch.cat` does not exist
// (the encoder's second conv and the up-sampler write the two channel halves of one buffer); F.pad is a
// no-op at 256x256 and is not materialised; the batch is processed in chunks that keep every layer's grid
// at >= one full wave of workgroups while bounding the live working set.
#include <cmath>
#include <cstring>

#include "engine.h"
#include "models.h"
#include "pointwise.h"

namespace cv {

static void double_conv_keys(std::vector<std::string>& out, const std::string& p) {
    out.push_back(p + "0.weight"); bn_keys(out, p + "1");
    out.push_back(p + "3.weight"); bn_keys(out, p + "4");
}

static Status unet_chunk(Engine& e, const void* x, bool x_u8, int n, float* logits, uint8_t* mask, float thr, hipStream_t s,
                         float* embedding = nullptr);

// Two deterministic calibration images, NCHW f32 in [0,1]: uniform noise, and a structured frame (dark noise, a bright
// checkered quadrilateral, saturated white and black blocks) -- the extremes of what a photo can put into the network.
static void calibration_images(std::vector<float>& x) {
    x.assign((size_t)2 * 3 * 65536, 0.f);
    uint32_t st = 0x9E3779B9u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (st >> 24) & 0xffu; };
    for (size_t i = 0; i < (size_t)3 * 65536; ++i) x[i] = (float)rnd() / 255.f;
    float* im = x.data() + (size_t)3 * 65536;
    for (int y = 0; y < 256; ++y)
        for (int xx = 0; xx < 256; ++xx) {
            const bool board = xx > 40 + y / 16 && xx < 215 - y / 20 && y > 35 && y < 220;
            for (int c = 0; c < 3; ++c) {
                float v = (float)(rnd() % 40) / 255.f;
                if (board) v = ((((xx - 40) / 22 + (y - 35) / 23) & 1) ? 230.f : 165.f) / 255.f;
                if (xx < 32 && y < 32) v = 1.f;
                if (xx >= 224 && y >= 224) v = 0.f;
                im[((size_t)c * 256 + y) * 256 + xx] = v;
            }
        }
}

Status unet_load(Engine& e, const ParamMap& pm) {
    auto m = std::make_unique<Engine::UNet>();
    Engine::UNet& U = *m;
    const int dt = e.dt;
    CV_TRY(e.guard_init());
    U.bilinear = pm.find("up1.up.weight") == pm.end();
    U.fuse_head = env_switch("CV_FUSE_HEAD", true);   // =0 keeps OutConv a separate kernel (then the up4 output tensor can be read back)
    U.max_cap = e.unet_chunk;
    const int S = U.max_cap;                          // tile choices are made for full chunks
    const int f = U.bilinear ? 2 : 1;
    U.c5 = 1024 / f;
    const int enc_c[5] = {64, 128, 256, 512, U.c5};
    const int res[5] = {256, 128, 64, 32, 16};
    auto px = [&](int level) { return (int64_t)S * res[level] * res[level]; };

    std::vector<std::string> known;
    double_conv_keys(known, "inc.double_conv.");
    // encoder
    CV_TRY(build_conv_bn(e, U.inc0, pm, "inc.double_conv.0", "inc.double_conv.1", 64, 3, 3, 1, 8, px(0), 256));
    CV_TRY(build_conv_bn(e, U.inc1, pm, "inc.double_conv.3", "inc.double_conv.4", 64, 64, 3, 1, 64, px(0), 256));
    if (dt != kF32) {
        // the same layer for the fused first-layer kernel (pointwise.hip: inc0_mfma): rows normalised as ConvLayer rows are (the
        // epilogue constants of U.inc0 carry the row exponents), k = (ky*3 + kx)*3 + c, padded 27 -> 32
        U.fused_inc0 = env_switch("CV_INC0", true);
        const float* w;
        CV_TRY(need(pm, "inc.double_conv.0.weight", {64, 3, 3, 3}, &w));
        std::vector<float> wn((size_t)64 * 32, 0.f);
        for (int ch = 0; ch < 64; ++ch) {
            for (int k = 0; k < 27; ++k) wn[ch * 32 + k] = w[(ch * 3 + k % 3) * 9 + k / 3];
            (void)normalise_row(&wn[ch * 32], 32);
        }
        std::vector<_Float16> pk((size_t)2 * 4 * 64 * 8);
        for (int hl = 0; hl < 2; ++hl)
            for (int f = 0; f < 4; ++f)
                for (int lane = 0; lane < 64; ++lane) {
                    const int ch = frag_row_channel(4, f, lane & 15), q = lane >> 4;
                    for (int j = 0; j < 8; ++j) pk[(((size_t)hl * 4 + f) * 64 + lane) * 8 + j] = f16_half(wn[ch * 32 + q * 8 + j], hl);
                }
        CV_TRY(U.inc0_wpk.upload(pk.data(), pk.size() * sizeof(_Float16)));
        if (dt == kSplit) {
            // ... and for the producer inside inc.double_conv.3's kernel: two 16-row fragments per 32-channel block, lane
            // (i, q) of fragment f <-> channel 32*cb + 8*(i/4) + 4*f + i%4, so that a lane ends with the 8 channels of group q
            U.fused_inc = U.fused_inc0 && env_switch("CV_FUSE_INC", true);
            std::vector<_Float16> pk2((size_t)2 * 2 * 2 * 64 * 8);
            for (int cb = 0; cb < 2; ++cb)
                for (int f = 0; f < 2; ++f)
                    for (int hl = 0; hl < 2; ++hl)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int ch = 32 * cb + frag_row_channel(2, f, lane & 15), q = lane >> 4;
                            for (int j = 0; j < 8; ++j)
                                pk2[((((size_t)cb * 2 + f) * 2 + hl) * 64 + lane) * 8 + j] = f16_half(wn[ch * 32 + q * 8 + j], hl);
                        }
            CV_TRY(U.inc0_wpk2.upload(pk2.data(), pk2.size() * sizeof(_Float16)));
        }
    }
    for (int i = 0; i < 4; ++i) {
        const std::string p = "down" + std::to_string(i + 1) + ".maxpool_conv.1.double_conv.";
        double_conv_keys(known, p);
        CV_TRY(build_conv_bn(e, U.d[i][0], pm, p + "0", p + "1", enc_c[i + 1], enc_c[i], 3, 1, enc_c[i], px(i + 1), res[i + 1]));
        CV_TRY(build_conv_bn(e, U.d[i][1], pm, p + "3", p + "4", enc_c[i + 1], enc_c[i + 1], 3, 1, enc_c[i + 1], px(i + 1), res[i + 1]));
    }
    // decoder: up_i consumes the deeper tensor (channels deep_c) and skip level (3 - i)
    //   transposed: up: deep_c -> deep_c/2 ; conv: cat(skip, up) = deep_c -> out_c -> out_c
    //   bilinear  : up keeps deep_c (== skip channels) ; conv: 2*deep_c -> mid = deep_c -> out_c
    int deep_c = U.c5;
    int up_c[4];                                      // channels of the up-sampled half of cat[lvl], by decoder stage
    for (int i = 0; i < 4; ++i) {
        const int lvl = 3 - i;                       // skip level, output resolution res[lvl]
        const int skip_c = enc_c[lvl];
        const std::string p = "up" + std::to_string(i + 1);
        int cat_c, mid_c, out_c;
        if (!U.bilinear) {
            const float *w, *b;
            CV_TRY(need(pm, p + ".up.weight", {deep_c, deep_c / 2, 2, 2}, &w));
            CV_TRY(need(pm, p + ".up.bias", {deep_c / 2}, &b));
            known.push_back(p + ".up.weight"); known.push_back(p + ".up.bias");
            CV_TRY(U.upT[i].build_convT(p + ".up", dt, w, deep_c, deep_c / 2, b, px(lvl + 1)));
            U.upT[i].layer_id = e.register_layer(p + ".up");
            static const bool fast_on = env_switch("CV_CONVT_FAST", true), fast_256 = env_switch("CV_CONVT_FAST_256", false);
            // measured (r06_tuning.md section 7): up4.up (K = 128) 0.40 -> 0.36 ms per 64 boards; up3.up (K = 256: 128 KB of weights leave
            // room for four staged pixel rows per wave only) 0.255 -> 0.29 ms -- it stays on the generic tile unless CV_CONVT_FAST_256=1
            if (dt == kSplit && fast_on && (deep_c == 128 || (deep_c == 256 && fast_256))) {
                // the (dy, dx, co) x ci view of the weight
                const int cout = deep_c / 2;
                CV_TRY(U.fast_up[i].pack(4 * cout, deep_c, [&](int r, int ci) { const int d = r / cout, co = r - d * cout; return w[((size_t)ci * cout + co) * 4 + d]; },
                                         [](int) { return 1.f; }, [&](int r) { return b[r % cout]; }, U.upT[i].name));
                U.fast_up[i].layer_id = U.upT[i].layer_id;
            }
            cat_c = skip_c + deep_c / 2;
            out_c = skip_c;
            mid_c = out_c;
        } else {
            U.up_id[i] = e.register_layer(p + ".up");
            cat_c = skip_c + deep_c;
            mid_c = cat_c / 2;
            out_c = (i == 3) ? 64 : skip_c / 2;
        }
        up_c[i] = cat_c - skip_c;
        const std::string c = p + ".conv.double_conv.";
        double_conv_keys(known, c);
        U.u[i][0].keep_host_weights = dt != kF32;     // consumer of cat([skip, up]): the halves may end up with different exponents
        CV_TRY(build_conv_bn(e, U.u[i][0], pm, c + "0", c + "1", mid_c, cat_c, 3, 1, cat_c, px(lvl), res[lvl]));
        CV_TRY(build_conv_bn(e, U.u[i][1], pm, c + "3", c + "4", out_c, mid_c, 3, 1, mid_c, px(lvl), res[lvl]));
        deep_c = out_c;
    }
    {
        const float *w, *b;
        CV_TRY(need(pm, "outc.conv.weight", {1, 64, 1, 1}, &w));
        CV_TRY(need(pm, "outc.conv.bias", {1}, &b));
        known.push_back("outc.conv.weight"); known.push_back("outc.conv.bias");
        for (int i = 0; i < 64; ++i)
            if (!std::isfinite(w[i])) return fail(1, "outc.conv: non-finite weight in the state dict");
        if (!std::isfinite(b[0])) return fail(1, "outc.conv: non-finite bias in the state dict");
        CV_TRY(U.outc_w.upload(w, 64 * sizeof(float)));
        CV_TRY(U.outc_b.upload(b, sizeof(float)));
        U.outc_id = e.register_layer("outc.conv");
    }
    CV_TRY(reject_unknown_keys(pm, known, U.bilinear ? "UNet(3,1,bilinear=True)" : "UNet(3,1)"));

    // activation shapes (dedicated buffers: borders are zeroed once and stay zero); memory comes with model_reserve
    U.in8.shape(256, 256, 8, dt);
    U.in8.fixed_exp = true;
    U.in8.exp = dt == kF32 ? 0 : kInputExp;
    U.a_inc0.shape(256, 256, 64, dt);
    U.acts = {&U.a_inc0};
    if (!U.fused_inc0) U.acts.push_back(&U.in8);     // the packed 8-channel copy of the input exists on the generic path only
    for (int lvl = 0; lvl < 4; ++lvl) {
        const int skip_c = enc_c[lvl];
        U.cat[lvl].shape(res[lvl], res[lvl], skip_c + up_c[3 - lvl], dt);
        U.cat[lvl].split_c = dt == kF32 ? 0 : skip_c;   // [skip | up-sampled]: one exponent per half
        U.pool[lvl].shape(res[lvl + 1], res[lvl + 1], skip_c, dt);
        U.pool[lvl].tie = &U.cat[lvl];               // max-pool of the skip half: same scale
        U.dmid[lvl].shape(res[lvl + 1], res[lvl + 1], enc_c[lvl + 1], dt);
        U.acts.push_back(&U.cat[lvl]); U.acts.push_back(&U.pool[lvl]); U.acts.push_back(&U.dmid[lvl]);
    }
    U.bott.shape(16, 16, U.c5, dt);
    U.acts.push_back(&U.bott);
    for (int i = 0; i < 4; ++i) {
        const int lvl = 3 - i;
        U.umid[i].shape(res[lvl], res[lvl], U.u[i][0].cout, dt);
        U.uout[i].shape(res[lvl], res[lvl], U.u[i][1].cout, dt);
        U.acts.push_back(&U.umid[i]);
        if (!(i == 3 && U.fuse_head)) U.acts.push_back(&U.uout[i]);   // with the fused head the up4 output never reaches memory
    }

    // algorithmic multiply-accumulates per image (conv / conv-transpose / outc), true channel counts
    int64_t macs = 0;
    auto add = [&](const ConvLayer& L, int64_t out_pixels) { macs += L.macs_per_out_pixel() * out_pixels; };
    add(U.inc0, 65536); add(U.inc1, 65536);
    for (int i = 0; i < 4; ++i) { add(U.d[i][0], (int64_t)res[i + 1] * res[i + 1]); add(U.d[i][1], (int64_t)res[i + 1] * res[i + 1]); }
    for (int i = 0; i < 4; ++i) {
        const int lvl = 3 - i;
        if (!U.bilinear) add(U.upT[i], (int64_t)res[lvl + 1] * res[lvl + 1]);
        add(U.u[i][0], (int64_t)res[lvl] * res[lvl]); add(U.u[i][1], (int64_t)res[lvl] * res[lvl]);
    }
    macs += 64LL * 65536;
    U.macs = macs;

    e.unet = std::move(m);
    // calibration of the f16-based engines on two images: ranges, then the f16 layers' rounding bias on the same two
    Status st = model_reserve(e, U, 2);
    if (st.ok() && dt != kF32 && calibration_enabled()) {
        std::vector<float> host;
        calibration_images(host);
        DeviceBuffer xin;
        st = xin.upload(host.data(), host.size() * sizeof(float));
        std::vector<ConvLayer*> layers{&U.inc0, &U.inc1};
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) { layers.push_back(&U.d[i][j]); layers.push_back(&U.u[i][j]); }
        if (st.ok())
            st = calibrate_model(e, U, layers, (const float*)xin.ptr, (size_t)3 * 65536, 2, 2, 65536, "UNet",
                                 [&](const float* x, int n, float* out) { return unet_chunk(e, x, false, n, out, nullptr, 0.5f, nullptr); });
    }
    if (!st.ok()) e.unet.reset();
    return st;
}

// module-name taps for cv_get_activation
void Engine::UNet::build_taps(const Engine&, int S) {
    Engine::UNet& U = *this;
    const int enc_c[5] = {64, 128, 256, 512, U.c5};
    if (!U.fused_inc0) U.taps["input"] = U.in8.ref(S, 0, 8);
    if (!U.fused_inc) U.taps["inc.double_conv.2"] = U.a_inc0.ref(S);     // fused: the tensor exists only inside inc.double_conv.3's kernel
    U.taps["inc.double_conv.5"] = U.cat[0].ref(S, 0, 64);
    U.taps["inc"] = U.taps["inc.double_conv.5"];
    for (int i = 0; i < 4; ++i) {
        const std::string p = "down" + std::to_string(i + 1);
        U.taps[p + ".maxpool_conv.0"] = U.pool[i].ref(S);
        U.taps[p + ".maxpool_conv.1.double_conv.2"] = U.dmid[i].ref(S);
        TensorRef out = (i < 3) ? U.cat[i + 1].ref(S, 0, enc_c[i + 1]) : U.bott.ref(S);
        U.taps[p + ".maxpool_conv.1.double_conv.5"] = out;
        U.taps[p] = out;
    }
    for (int i = 0; i < 4; ++i) {
        const int lvl = 3 - i;
        const std::string p = "up" + std::to_string(i + 1);
        U.taps[p + ".up"] = U.cat[lvl].ref(S, enc_c[lvl], U.cat[lvl].C - enc_c[lvl]);
        U.taps[p + ".conv.double_conv.2"] = U.umid[i].ref(S);
        if (!(i == 3 && U.fuse_head)) {
            U.taps[p + ".conv.double_conv.5"] = U.uout[i].ref(S);
            U.taps[p] = U.uout[i].ref(S);
        }
    }
}

int64_t unet_macs(Engine& e) { return e.unet ? e.unet->macs : 0; }
int unet_embedding_dim(Engine& e) { return e.unet ? e.unet->c5 : 0; }

Status unet_activation(Engine& e, const std::string& name, TensorRef* out) {
    if (!e.unet) return fail(3, "UNet not loaded");
    return e.unet->tap(name, out) ? Status() : fail(1, "unknown UNet activation '" + name + "'");
}

static Status unet_chunk(Engine& e, const void* x, bool x_u8, int n, float* logits, uint8_t* mask, float thr,
                         hipStream_t s, float* embedding) {
    Engine::UNet& U = *e.unet;
    const int dt = e.dt;
    const int enc_c[5] = {64, 128, 256, 512, U.c5};
    const double esz = dtype_size(dt);

    const TensorRef pool0 = U.pool[0].ref(n);
    bool inc_done = false;
    if (U.fused_inc && !e.calibrating) {
        // inc.double_conv.0 produced inside inc.double_conv.3's kernel: the tensor between them never reaches memory.  (Calibration
        // runs the layers apart so that the intermediate's exponent is measured; launches the halo tile does not take fall back.)
        CV_TRY(U.inc0.set_exps(kInputExp, U.a_inc0.exp, s));
        const Engine::Fuse0 f0{x, x_u8, U.inc0_wpk2.ptr, (const float*)U.inc0.scale.ptr, (const float*)U.inc0.shift.ptr,
                               std::ldexp(1.f, -kInputExp), 27.0 * 64};
        Status st = e.run_conv(U.inc1, U.a_inc0.ref(n), U.cat[0].ref(n, 0, 64), nullptr, true, s, nullptr, &pool0, &f0);
        if (st.ok()) inc_done = true;
        else if (st.code != Engine::kNotFused) return st;
    }
    if (inc_done) {
    } else if (U.fused_inc0) {
        // first layer straight from the caller's image: no packed copy of the input, no separate packing kernel
        CV_TRY(U.inc0.set_exps(kInputExp, U.a_inc0.exp, s));
        if (e.profiling) e.prof_begin(U.inc0.name, true, 27.0 * 64 * 65536 * n, s, (double)n * 65536 * ((x_u8 ? 3 : 12) + 64 * esz) + 27 * 64 * esz);
        CV_TRY(e.timed_end("inc0_mfma", inc0_mfma(dt, x, x_u8, n, U.inc0_wpk.ptr, (const float*)U.inc0.scale.ptr, (const float*)U.inc0.shift.ptr,
                                                  kInputExp, U.a_inc0.ref(n), e.guard_ptr(), U.inc0.layer_id, s), s));
        if (e.calibrating) CV_TRY(e.measure(U.a_inc0.ref(n), s));
    } else {
        e.timed_begin("pack_input", s, (double)n * 65536 * ((x_u8 ? 3 : 12) + 8 * esz));
        if (x_u8) CV_TRY(e.timed_end("pack_hwc3_u8", pack_hwc3_u8(dt, (const uint8_t*)x, U.in8.ref(n, 0, 8), s), s));
        else      CV_TRY(e.timed_end("pack_nchw_f32", pack_nchw_f32(dt, (const float*)x, 3, U.in8.ref(n, 0, 8), e.guard_ptr(), s), s));
        CV_TRY(e.run_conv(U.inc0, U.in8.ref(n, 0, 8), U.a_inc0.ref(n), nullptr, true, s));
    }
    // every encoder level's second conv also emits its 2x2 max-pool (fused into the epilogue where the halo kernel runs)
    if (!inc_done) CV_TRY(e.run_conv(U.inc1, U.a_inc0.ref(n), U.cat[0].ref(n, 0, 64), nullptr, true, s, nullptr, &pool0));
    for (int i = 0; i < 4; ++i) {
        CV_TRY(e.run_conv(U.d[i][0], U.pool[i].ref(n), U.dmid[i].ref(n), nullptr, true, s));
        TensorRef out = (i < 3) ? U.cat[i + 1].ref(n, 0, enc_c[i + 1]) : U.bott.ref(n);
        const TensorRef pool_next = (i < 3) ? U.pool[i + 1].ref(n) : TensorRef();
        CV_TRY(e.run_conv(U.d[i][1], U.dmid[i].ref(n), out, nullptr, true, s, nullptr, i < 3 ? &pool_next : nullptr));
    }
    if (embedding && !e.calibrating) {
        // the embedding of the reference's hook (named_modules()[52] = down4.maxpool_conv.1.double_conv.5): channel means of the
        // bottleneck, pooled while this chunk's tensor is the one in the buffer -- inside the captured sequence of a small forward
        const TensorRef bott = U.bott.ref(n);
        e.timed_begin("embedding (channel means)", s, (double)n * bott.C * (bott.H * bott.W * esz + 4));
        CV_TRY(e.timed_end("channel_means", channel_means(dt, bott, embedding, s), s));
    }
    TensorRef deep = U.bott.ref(n);
    for (int i = 0; i < 4; ++i) {
        const int lvl = 3 - i;
        TensorRef up = U.cat[lvl].ref(n, enc_c[lvl], U.cat[lvl].C - enc_c[lvl]);
        static const int fast_min = env_int("CV_CONVT_FAST_MIN", 8);
        if (!U.bilinear && U.fast_up[i].on && !e.calibrating && n >= fast_min) {
            CV_TRY(conv1x1_lds(e, U.fast_up[i], kConvT, deep, up, s));
        } else if (!U.bilinear) {
            CV_TRY(e.run_conv(U.upT[i], deep, up, nullptr, false, s));
        } else {
            e.timed_begin("upsample_bilinear2x", s, (double)n * deep.H * deep.W * deep.C * esz * 5.0);     // 1 read + 4 written elements
            CV_TRY(e.timed_end("upsample_bilinear2x", upsample_bilinear2x(dt, deep, up, e.guard_ptr(), U.up_id[i], s), s));
            if (e.calibrating) CV_TRY(e.measure(up, s));
        }
        CV_TRY(e.run_conv(U.u[i][0], U.cat[lvl].ref(n), U.umid[i].ref(n), nullptr, true, s));
        if (i == 3 && U.fuse_head) {
            // OutConv (1x1, 64 -> 1, + bias) and the sigmoid/threshold mask ride in the epilogue of the last 3x3 conv:
            // the 64-channel full-resolution tensor is never written or re-read.
            const Engine::Head head{(const float*)U.outc_w.ptr, (const float*)U.outc_b.ptr, logits, mask, thr};
            CV_TRY(e.run_conv(U.u[i][1], U.umid[i].ref(n), U.uout[i].ref(n), nullptr, true, s, &head));
            return Status();
        }
        CV_TRY(e.run_conv(U.u[i][1], U.umid[i].ref(n), U.uout[i].ref(n), nullptr, true, s));
        deep = U.uout[i].ref(n);
    }
    e.timed_begin("outc_1x1", s, (double)n * 65536 * (64 * esz + 4 + (mask ? 1 : 0)));
    return e.timed_end("outc_1x1", outc_1x1(dt, deep, (const float*)U.outc_w.ptr, (const float*)U.outc_b.ptr, logits, mask, thr,
                                            e.guard_ptr(), U.outc_id, s), s);
}

Status unet_forward(Engine& e, const void* x, bool x_u8, int batch, float* logits, uint8_t* mask, float thr,
                    hipStream_t s, float* embedding) {
    if (!e.unet) return fail(3, "UNet weights not loaded (call cv_load_unet first)");
    Engine::GraphKey key;
    key.flags = x_u8 ? 1 : 0;
    std::memcpy(&key.thr_bits, &thr, sizeof(float));
    const ForwardShape shape{8, (size_t)3 * 256 * 256 * (x_u8 ? 1 : 4), 65536, (size_t)e.unet->c5};
    return forward_chunked(e, *e.unet, shape, key, "cv_unet_forward", x, batch, logits, mask, embedding, s,
                           [&](const void* xc, int n, float* lg, uint8_t* mk, float* emb, hipStream_t st) {
                               return unet_chunk(e, xc, x_u8, n, lg, mk, thr, st, emb);
                           });
}

}  // namespace cv
