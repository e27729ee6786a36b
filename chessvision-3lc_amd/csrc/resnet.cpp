// resnet.cpp -- timm ResNet-18 / ResNet-34 (in_chans=1, num_classes=13) plan: packing + forward schedule.
//
// Module tree per notebooks/model-summary.ipynb (reference) / SURVEY.md Appendix B:
//   conv1 7x7 s2 p3 -> bn1 -> ReLU -> maxpool 3x3 s2 p1 -> layer1..4 (BasicBlocks: {2,2,2,2} for resnet18, {3,4,6,3} for
//   resnet34; first block of layer2-4 has stride 2 and a [conv1x1 s2, BN] shortcut) -> global avg pool -> fc 512 -> 13.
// Everything below that depends on the depth (keys, taps, MACs, calibration, the chained layer1) is derived from ResNetArch.
// BasicBlock = conv1-bn1-ReLU-conv2-bn2-(+shortcut)-ReLU: both BNs, the residual add and both ReLUs are conv
// epilogues here; the squares of many boards are batched so the 2x2 / 4x4 stages still form large GEMMs.
#include <cmath>
#include <cstring>

#include "engine.h"
#include "models.h"
#include "pointwise.h"

namespace cv {

static const ResNetArch kResNetArchs[] = {{"resnet18", {2, 2, 2, 2}}, {"resnet34", {3, 4, 6, 3}}};

const ResNetArch* resnet_arch(const std::string& name) {
    for (const ResNetArch& a : kResNetArchs)
        if (name == a.name) return &a;
    return nullptr;
}

static Status layer1_chain(Engine& e, int n, hipStream_t s);
static Status resnet_chunk(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding = nullptr,
                           const InputNorm* norm = nullptr);

// form of the chained layer1 launch (f16r): 2 (default) = two workgroups per CU, block 0's f32 output written and read back; 1 = one
// workgroup per CU with 512 registers, the f32 trunk stays in registers -- no round trip, but nothing covers the workgroup's barriers,
// prologue and epilogues: 1.81 against 1.62 ms per 16384 squares (CV_CHAIN_WG=1; r05_tuning.md step 6)
static int chain_form() {
    static const int form = env_switch("CV_CHAIN_WG", false) ? 1 : 2;
    return form;
}

// split-f16 engine: squares from which the dedicated shortcut kernel replaces the generic launch (CV_SHORTCUT_SPLIT_MIN; below it the
// generic launch shares conv1's launch, Engine::PendingConv)
static int fast_sc_min_squares() {
    static const int v = env_int("CV_SHORTCUT_SPLIT_MIN", 1024);
    return v;
}

// fold the stem's output exponent into the device copies of its epilogue constants (ConvLayer::set_exps for the stem)
static Status stem_set_exp(Engine::ResNet& R, int dt, int out_exp, hipStream_t s) {
    if (out_exp == R.stem_out_exp) return Status();
    CV_TRY(fold_exps("conv1", R.h_stem_scale, R.h_stem_shift, R.stem_scale.ptr, R.stem_shift.ptr, dt == kF32 ? 0 : kInputExp, out_exp, s));
    R.stem_out_exp = out_exp;
    return Status();
}

void classifier_calibration_squares(std::vector<float>& host, int kCal, int kBias) {
    host.assign((size_t)kBias * 4096, 0.f);
    uint32_t rs = 0x2545F491u;
    auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return (rs >> 24) & 0xffu; };
    for (int q = 0; q < kCal; ++q)
        for (int y = 0; y < 64; ++y)
            for (int x = 0; x < 64; ++x) {
                float v;
                if (q < 48) v = (float)rnd();
                else if (q < 80) v = (float)((q - 48) * 8 + 3);                                   // flat levels 3..251
                else if (q < 104) v = (float)(((x * (q - 79)) + y * 3) & 255);                      // ramps
                else v = (((x >> (q & 3)) + (y >> ((q >> 2) & 3))) & 1) ? 235.f : (float)(20 + (q - 104) * 6);   // checkers
                host[((size_t)q * 64 + y) * 64 + x] = v / 255.f;
            }
    for (int q = kCal; q < kBias; ++q) {
        float grid[5][5];
        for (auto& row : grid) for (float& g : row) g = (float)rnd();
        for (int y = 0; y < 64; ++y)
            for (int x = 0; x < 64; ++x) {
                float v;
                if (q < kCal + 64) v = (float)rnd();
                else {                                                                               // bilinear, cell = 16 pixels
                    const int gy = y >> 4, gx = x >> 4;
                    const float fy = (float)(y & 15) / 16.f, fx = (float)(x & 15) / 16.f;
                    const float top = grid[gy][gx] * (1.f - fx) + grid[gy][gx + 1] * fx, bot = grid[gy + 1][gx] * (1.f - fx) + grid[gy + 1][gx + 1] * fx;
                    v = std::floor(top * (1.f - fy) + bot * fy + 0.5f);
                }
                host[((size_t)q * 64 + y) * 64 + x] = v / 255.f;
            }
    }
}

Status resnet_load(Engine& e, const ParamMap& pm, const std::string& arch) {
    const ResNetArch* A = resnet_arch(arch);
    if (!A) return fail(1, "unknown ResNet architecture '" + arch + "' (supported: 'resnet18', 'resnet34')");
    auto m = std::make_unique<Engine::ResNet>();
    Engine::ResNet& R = *m;
    R.arch = A;
    for (int l = 0; l < 4; ++l) R.first[l + 1] = R.first[l] + A->depth[l];
    R.nblocks = R.first[4];
    R.blocks.reset(new Engine::ResNet::Block[R.nblocks]);
    const int dt = e.dt;
    CV_TRY(e.guard_init());
    // the f32 engine materialises the 32x32x64 stem output (34 x 34 x 64 x 4 B per square with its border): keep that
    // tensor under the 4 GiB the 32-bit DMA offsets address
    R.max_cap = e.resnet_chunk;
    if (dt == kF32)
        while ((uint64_t)R.max_cap * 34 * 34 * 64 * 4 >= (1ull << 32) && R.max_cap > 1) R.max_cap /= 2;
    const int S = R.max_cap;
    std::vector<std::string> known;

    {   // stem: conv1 (64,1,7,7) + bn1
        const float* w;
        CV_TRY(need(pm, "conv1.weight", {64, 1, 7, 7}, &w));
        std::vector<float> sc, sh;
        CV_TRY(bn_fold(pm, "bn1", 64, sc, sh));
        known.push_back("conv1.weight"); bn_keys(known, "bn1");
        std::vector<float> wn(w, w + 64 * 49);
        R.h_stem_scale.assign(64, 0.f); R.h_stem_shift.assign(64, 0.f);
        for (int ch = 0; ch < 64; ++ch) {
            for (int k = 0; k < 49; ++k)
                if (!std::isfinite(w[ch * 49 + k])) return fail(1, "conv1: non-finite weight in the state dict");
            if (!std::isfinite(sc[ch]) || !std::isfinite(sh[ch])) return fail(1, "bn1: non-finite BatchNorm scale/shift (running_var + eps <= 0?)");
            const int ex = dt != kF32 ? normalise_row(&wn[ch * 49], 49) : 0;      // filter normalisation, as ConvLayer rows
            R.h_stem_scale[ch] = std::ldexp(sc[ch], ex);
            R.h_stem_shift[ch] = sh[ch];
        }
        CV_TRY(R.stem_w.upload(wn.data(), 64 * 49 * sizeof(float)));
        if (dt != kF32) {
            // MFMA A-operand image of the 64x(7x7) filter bank: k-slot (ks, q, j) = filter tap (ky = 4*ks + q, kx = j),
            // MFMA row i of fragment f = channel 16*(i/4) + 4*f + i%4 (the conv epilogue's lane-contiguous order)
            std::vector<_Float16> pk((size_t)2 * 2 * 4 * 64 * 8);
            for (int hl = 0; hl < 2; ++hl)
                for (int ks = 0; ks < 2; ++ks)
                    for (int f = 0; f < 4; ++f)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int ch = frag_row_channel(4, f, lane & 15), ky = ks * 4 + (lane >> 4);
                            for (int j = 0; j < 8; ++j)
                                pk[((((size_t)hl * 2 + ks) * 4 + f) * 64 + lane) * 8 + j] = f16_half((ky < 7 && j < 7) ? wn[ch * 49 + ky * 7 + j] : 0.f, hl);
                        }
            CV_TRY(R.stem_wpk.upload(pk.data(), pk.size() * sizeof(_Float16)));
        }
        R.stem_id = e.register_layer("conv1");
        CV_TRY(R.stem_scale.alloc(64 * sizeof(float), false));
        CV_TRY(R.stem_shift.alloc(64 * sizeof(float), false));
        CV_TRY(stem_set_exp(R, dt, 0, nullptr));
    }
    if (dt == kF32) { R.stem_out.shape(32, 32, 64, dt); R.acts.push_back(&R.stem_out); }   // other engines fuse stem + pool
    R.pool_out.shape(16, 16, 64, dt);
    R.pool_out.want32 = e.trunk32;
    R.acts.push_back(&R.pool_out);

    const int widths[4] = {64, 128, 256, 512};
    const int res[4] = {16, 8, 4, 2};
    int cin = 64;
    int64_t macs = 49LL * 64 * 32 * 32;
    for (int l = 0; l < 4; ++l) {
        for (int bi = 0; bi < A->depth[l]; ++bi) {
            Engine::ResNet::Block& B = R.blocks[R.first[l] + bi];
            const std::string p = "layer" + std::to_string(l + 1) + "." + std::to_string(bi);
            const int w = widths[l];
            const int stride = (bi == 0 && l > 0) ? 2 : 1;
            const int64_t px = (int64_t)S * res[l] * res[l];
            known.push_back(p + ".conv1.weight"); bn_keys(known, p + ".bn1");
            known.push_back(p + ".conv2.weight"); bn_keys(known, p + ".bn2");
            CV_TRY(build_conv_bn(e, B.conv1, pm, p + ".conv1", p + ".bn1", w, cin, 3, stride, cin, px, res[l]));
            CV_TRY(build_conv_bn(e, B.conv2, pm, p + ".conv2", p + ".bn2", w, w, 3, 1, w, px, res[l]));
            B.has_down = (stride != 1 || cin != w);
            if (B.has_down) {
                known.push_back(p + ".downsample.0.weight"); bn_keys(known, p + ".downsample.1");
                // f16r: the shortcut convolution IS the trunk at the stage boundaries -- f16 products there put their rounding
                // straight onto the skip path (CPU emulation of the arithmetic, 4096 squares: worst soft-max error 9.7e-4 with f16
                // shortcuts, 6.5e-4 with exact ones).  It holds 1.1 % of the network's MACs: run it on the f32 MFMA, f32 twin in,
                // f32 twin out; no f16 copy of the shortcut tensor exists.
                CV_TRY(build_conv_bn(e, B.down, pm, p + ".downsample.0", p + ".downsample.1", w, cin, 1, stride, cin, px, res[l],
                                     e.trunk32 ? (int)kF32 : -1));
                B.sc.shape(res[l], res[l], w, dt);
                B.sc.want32 = B.sc.only32 = e.trunk32;
                R.acts.push_back(&B.sc);
                // measured (profiles/r05_tuning.md sections 4 and 15): the first form of the dedicated kernel (weight fragments streamed from L2 by
                // every wave) 0.31 / 0.21 / 0.15 ms per 16384 squares against 0.27 / 0.19 / 0.16 for `down` on the f32-input MFMA; the second
                // form (weights resident in LDS, persistent waves, full-line stores) 0.145 / 0.085 / 0.084 -- ON by default;
                // CV_SHORTCUT_FAST=0 switches it off (the generic launch then rides with conv1 at single-board sizes, Engine::PendingConv)
                static const bool fast_on = env_switch("CV_SHORTCUT_FAST", true);
                // round 6: the headline engine (split-f16 tensors) takes the same kernel in its SPLIT form at throughput batch sizes -- there it
                // computes exactly what the generic launch computes (same products, same order: bit-identical), so the choice may follow the batch
                // (layer4's shortcut, 256 -> 512 on 2 x 2 maps, stays on the generic tile there: 0.071 against 0.090 ms per 16384 squares)
                if (((e.trunk32 && dt == kF16) || dt == kSplit) && fast_on && w == 2 * cin && (cin == 64 || cin == 128 || (cin == 256 && dt != kSplit))) {
                    const float* wd;
                    CV_TRY(need(pm, p + ".downsample.0.weight", {w, cin, 1, 1}, &wd));
                    std::vector<float> sc, sh;
                    CV_TRY(bn_fold(pm, p + ".downsample.1", w, sc, sh));
                    CV_TRY(B.fast_sc.pack(w, cin, [&](int ch, int k) { return wd[(size_t)ch * cin + k]; }, [&](int ch) { return sc[ch]; },
                                          [&](int ch) { return sh[ch]; }, B.down.name));
                    B.fast_sc.layer_id = B.down.layer_id;
                }
                macs += (int64_t)cin * w * res[l] * res[l];
            }
            B.mid.shape(res[l], res[l], w, dt);
            B.out.shape(res[l], res[l], w, dt);
            B.out.want32 = e.trunk32;                        // f16r: the residual trunk never rounds to f16 (Activation::buf32)
            R.acts.push_back(&B.mid); R.acts.push_back(&B.out);
            macs += ((int64_t)cin * 9 * w + (int64_t)w * 9 * w) * res[l] * res[l];
            cin = w;
        }
    }
    {
        const float *w, *b;
        CV_TRY(need(pm, "fc.weight", {13, 512}, &w));
        CV_TRY(need(pm, "fc.bias", {13}, &b));
        known.push_back("fc.weight"); known.push_back("fc.bias");
        for (int i = 0; i < 13 * 512; ++i)
            if (!std::isfinite(w[i])) return fail(1, "fc: non-finite weight in the state dict");
        for (int i = 0; i < 13; ++i)
            if (!std::isfinite(b[i])) return fail(1, "fc: non-finite bias in the state dict");
        CV_TRY(R.fc_w.upload(w, 13 * 512 * sizeof(float)));
        CV_TRY(R.fc_b.upload(b, 13 * sizeof(float)));
        R.head_id = e.register_layer("fc");
        macs += 13 * 512;
    }
    CV_TRY(reject_unknown_keys(pm, known, (std::string(A->name) + "(in_chans=1, num_classes=13)").c_str()));
    R.macs = macs;
    {   // f16r: layer1 as one chained launch -- the chained layers' weight stages (9 taps x 64 rows x 128 B each) back to back.
        // A three-block layer1 (resnet34) chains all three blocks by default; CV_RESNET_CHAIN_BLOCKS=2 chains the first two.
        static const bool on = env_switch("CV_RESNET_CHAIN", true);
        static const int max_nb = env_int("CV_RESNET_CHAIN_BLOCKS", 3);
        const int nb = std::min(A->depth[0], max_nb);
        std::vector<ConvLayer*> L;
        for (int b = 0; b < nb; ++b) { L.push_back(&R.blocks[b].conv1); L.push_back(&R.blocks[b].conv2); }
        bool fits = on && (nb == 2 || nb == 3) && e.trunk32 && dt == kF16;
        const size_t one = (size_t)9 * 64 * 128;
        for (ConvLayer* l : L) fits = fits && l->dt == kF16 && l->ct == 64 && l->rows == 64 && l->nStages == 9 && l->nCt == 1 && l->w.bytes >= one && l->halo_ok;
        if (fits) {
            CV_TRY(R.chain_w.alloc(L.size() * one, false));
            for (size_t i = 0; i < L.size(); ++i) CV_HIP(sync_memcpy((char*)R.chain_w.ptr + i * one, L[i]->w.ptr, one, hipMemcpyDeviceToDevice));
            R.chain_ok = true;
            R.chain_nb = nb;
        }
    }
    e.resnet = std::move(m);

    // range calibration on 128 squares: noise, flat grey levels, gradients and checkers (what board crops look like)
    // (the rounding-bias pass of the fp16 layers, ConvLayer::want_round_err, reads 128 more: 64 of noise and 64 smooth ones --
    // bilinear blow-ups of a random 4 x 4 grid, what a board crop looks like away from piece edges -- so that the channel means it
    // measures are not those of one texture)
    Status st = model_reserve(e, R, 128);
    if (st.ok() && dt != kF32 && calibration_enabled()) {
        constexpr int kCal = 128, kBias = 256;
        std::vector<float> host;
        classifier_calibration_squares(host, kCal, kBias);
        DeviceBuffer xin;
        st = xin.upload(host.data(), host.size() * sizeof(float));
        std::vector<ConvLayer*> layers;                                         // the f16 layers of the rounding-bias pass
        for (int b = 0; b < R.nblocks; ++b) {
            Engine::ResNet::Block& B = R.blocks[b];
            layers.push_back(&B.conv1); layers.push_back(&B.conv2);
            if (B.has_down) layers.push_back(&B.down);
        }
        if (st.ok())
            st = calibrate_model(e, R, layers, (const float*)xin.ptr, 4096, kCal, kBias, 13, A->name,
                                 [&](const float* x, int n, float* out) { return resnet_chunk(e, x, false, n, out, false, nullptr); });
    }
    if (!st.ok()) e.resnet.reset();
    else e.yolo.reset();                                 // the classifier slot holds one model
    return st;
}

void Engine::ResNet::build_taps(const Engine& e, int S) {
    Engine::ResNet& R = *this;
    // f16r: a trunk tensor (pool output, block outputs) IS its unrounded f32 twin -- what the residual adds and the head read; the f16
    // copy beside it is that tensor rounded once for the next convolution.  The taps report the twin: a tap of the copy is 2^-12 off
    // the head's input, more than the head kernel's own error
    auto trunk = [&](const Activation& a) { return a.want32 ? a.ref32(S) : a.ref(S); };
    if (e.dt == kF32) R.taps["act1"] = R.stem_out.ref(S);
    R.taps["maxpool"] = trunk(R.pool_out);
    for (int l = 0; l < 4; ++l) {
        for (int bi = 0; bi < R.arch->depth[l]; ++bi) {
            Engine::ResNet::Block& B = R.blocks[R.first[l] + bi];
            const std::string p = "layer" + std::to_string(l + 1) + "." + std::to_string(bi);
            // chained layer1 (f16r): conv1's output of every chained block and the f16 copies of the chained blocks' outputs but the last
            // live in LDS only -- no tap for the former, the latter are read from their f32 twins
            const bool chained = R.chain_ok && l == 0 && bi < R.chain_nb;
            if (!chained) R.taps[p + ".act1"] = B.mid.ref(S);
            if (chained && bi < R.chain_nb - 1) {            // an inner chained block's output: its f32 twin (form 2) or nowhere outside the kernel (form 1)
                if (chain_form() == 2) R.taps[p] = B.out.ref32(S);
            } else R.taps[p] = trunk(B.out);
            if (B.has_down) R.taps[p + ".downsample"] = B.sc.only32 ? B.sc.ref32(S) : B.sc.ref(S);
        }
        R.taps["layer" + std::to_string(l + 1)] = trunk(R.blocks[R.first[l + 1] - 1].out);
    }
}

int64_t resnet_macs(Engine& e) { return e.resnet ? e.resnet->macs : 0; }

Status resnet_activation(Engine& e, const std::string& name, TensorRef* out) {
    if (!e.resnet) return fail(3, "ResNet not loaded");
    const Engine::ResNet& R = *e.resnet;
    if (!R.tap(name, out)) {
        // the fp16 classifier runs the first chain_nb blocks of layer1 as ONE launch: their conv1 outputs (and, in the one-workgroup form,
        // the outputs of every chained block but the last) exist in LDS / registers only
        if (R.chain_ok) {
            std::string kept;
            bool hit = false;
            for (int b = 0; b < R.chain_nb; ++b) {
                const std::string p = "layer1." + std::to_string(b);
                kept += (b ? ", " : "") + p + ".act1";
                hit = hit || name == p + ".act1";
                if (b < R.chain_nb - 1 && chain_form() == 1) { kept += ", " + p; hit = hit || name == p; }
            }
            if (hit)
                return fail(1, "ResNet activation '" + name + "' is not materialised by precision f16r: layer1 runs " +
                               std::to_string(2 * R.chain_nb) + " convolutions as one chained launch and keeps " + kept +
                               " on the chip -- set CV_RESNET_CHAIN=0 before creating the engine to run layer1 layer by layer");
        }
        return fail(1, "unknown " + std::string(R.arch->name) + " activation '" + name + "'");
    }
    return Status();
}

static Status resnet_chunk(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding,
                           const InputNorm* norm) {
    Engine::ResNet& R = *e.resnet;
    const int dt = e.dt;
    const double esz = dtype_size(dt), in_b = x_u8 ? 1.0 : 4.0;
    if (dt == kF32) {
        e.timed_begin("stem7x7", s, (double)n * (4096 * in_b + 1024 * 64 * esz), 49.0 * 64 * 1024 * n);
        CV_TRY(e.timed_end("stem7x7", stem7x7(dt, x, x_u8, n, (const float*)R.stem_w.ptr, (const float*)R.stem_scale.ptr,
                                              (const float*)R.stem_shift.ptr, R.stem_out.ref(n), s, norm), s));
        e.timed_begin("maxpool3x3s2", s, (double)n * (1024 + 256) * 64 * esz);
        CV_TRY(e.timed_end("maxpool3x3s2", maxpool3x3s2(dt, R.stem_out.ref(n), R.pool_out.ref(n), s), s));
    } else {
        CV_TRY(stem_set_exp(R, dt, R.pool_out.exp, s));
        e.timed_begin("stem7x7+maxpool (mfma)", s, (double)n * (4096 * in_b + 256 * 64 * (esz + (R.pool_out.want32 ? 4.0 : 0.0))), 49.0 * 64 * 1024 * n);
        CV_TRY(e.timed_end("stem_pool_mfma", stem_pool_mfma(dt, x, x_u8, n, R.stem_wpk.ptr, (const float*)R.stem_scale.ptr,
                                                            (const float*)R.stem_shift.ptr, kInputExp, R.pool_out.ref(n),
                                                            e.guard_ptr(), R.stem_id, s, norm), s));
        if (e.calibrating) CV_TRY(e.measure(R.pool_out.ref(n), s));
    }
    TensorRef cur = R.pool_out.ref(n);
    int first_block = 0;
    if (R.chain_ok && !e.calibrating) {                // the calibration passes run layer by layer (every tensor is measured)
        CV_TRY(layer1_chain(e, n, s));
        cur = R.blocks[R.chain_nb - 1].out.ref(n);
        first_block = R.chain_nb;
    }
    for (int i = first_block; i < R.nblocks; ++i) {
        Engine::ResNet::Block& B = R.blocks[i];
        TensorRef shortcut = cur;
        bool conv1_done = false;
        // the shortcut convolution and conv1 both read the block input and do not depend on each other: at single-board sizes neither
        // fills the chip, and they go out as ONE launch (Engine::PendingConv; three launches of ~7-10 us fewer per forward)
        auto down_beside_conv1 = [&](const TensorRef& down_in, const TensorRef& down_out) -> Status {
            Engine::PendingConv pa, pb;
            e.defer = &pa; e.defer_first = true;
            Status st = e.run_conv(B.down, down_in, down_out, nullptr, false, s);
            e.defer = &pb; e.defer_first = false;
            if (st.ok()) st = e.run_conv(B.conv1, cur, B.mid.ref(n), nullptr, true, s);
            e.defer = nullptr;
            CV_TRY(st);
            conv1_done = true;
            return e.flush_pending(pa, pb, s);
        };
        if (B.has_down) {
            if (B.sc.only32) {                                 // f16r: f32-grade convolution from the trunk's twin to the shortcut's
                TensorRef in32 = cur;
                in32.base = cur.base32; in32.base32 = nullptr; in32.f32_only = 1;
                // every launch size takes the same kernel: results across batch shapes agree to 1e-4 (only f32 summation
                // orders differ), and the generic f32-MFMA shortcut differs from this one by up to 1e-3 -- a switch at 1024 squares made the
                // 8-rank test's single-photo recomputations disagree with the FENs of its 256-board jobs
                if (B.fast_sc.on && !e.calibrating) CV_TRY(conv1x1_lds(e, B.fast_sc, kShortcutF32, in32, B.sc.ref32(n), s));
                else CV_TRY(down_beside_conv1(in32, B.sc.ref32(n)));
            } else if (B.fast_sc.on && dt == kSplit && !e.calibrating && n >= fast_sc_min_squares()) {
                // split-f16 tensors in, split-f16 tensors out; below the threshold the generic launch rides with conv1 (one launch fewer)
                CV_TRY(conv1x1_lds(e, B.fast_sc, kShortcutSplit, cur, B.sc.ref(n), s));
            } else {
                CV_TRY(down_beside_conv1(cur, B.sc.ref(n)));
            }
            shortcut = B.sc.ref(n);
        }
        if (!conv1_done) CV_TRY(e.run_conv(B.conv1, cur, B.mid.ref(n), nullptr, true, s));
        CV_TRY(e.run_conv(B.conv2, B.mid.ref(n), B.out.ref(n), &shortcut, true, s));
        cur = B.out.ref(n);
    }
    int head_dt = dt;
    if (cur.base32) { cur.base = cur.base32; head_dt = kF32; }   // f16r: pool the trunk's f32 twin
    if (embedding && !e.calibrating) {
        // the embedding of the reference's hook (named_modules()[90] = global_pool): channel means of the tensor the head pools
        e.timed_begin("embedding (channel means)", s, (double)n * 512 * (cur.H * cur.W * dtype_size(head_dt) + 4));
        CV_TRY(e.timed_end("channel_means", channel_means(head_dt, cur, embedding, s), s));
    }
    e.timed_begin("head_avgpool_fc", s, (double)n * (cur.H * cur.W * 512 * dtype_size(head_dt) + 13 * 4), 13.0 * 512 * n);
    return e.timed_end("head_avgpool_fc", head_avgpool_fc(head_dt, cur, (const float*)R.fc_w.ptr, (const float*)R.fc_b.ptr, out,
                                                          softmax ? 1 : 0, e.guard_ptr(), R.head_id, s), s);
}

// the first chain_nb blocks of layer1 in one launch (f16r engine): pool_out (f16 copy + f32 twin) -> blocks[nb-1].out (f16 copy + f32 twin),
// the inner blocks' f32 output twins as the only intermediates in memory (two-workgroup form; in the one-workgroup form they stay in
// registers).  Same arithmetic as the 2 nb run_conv launches: f16 products, f32 accumulation, BN affine and residual in f32, one rounding
// to f16 per tensor.
static Status layer1_chain(Engine& e, int n, hipStream_t s) {
    Engine::ResNet& R = *e.resnet;
    const int nb = R.chain_nb;
    Engine::ResNet::Block& BL = R.blocks[nb - 1];
    const TensorRef x = R.pool_out.ref(n), yl = BL.out.ref(n);
    if (!x.base || !x.base32 || !yl.base || !yl.base32 || x.Cs != 64 || yl.Cs != 64 || x.H != 16 || x.W != 16)
        return fail(3, "layer1 chain: trunk tensors are not in the f16r layout");
    // tensor exponents exactly as the layer-by-layer path folds them
    ConvLayer* L[6];
    int in_exp = x.exp;
    for (int b = 0; b < nb; ++b) {
        Engine::ResNet::Block& B = R.blocks[b];
        if (!B.out.ref(n).base32) return fail(3, "layer1 chain: trunk tensors are not in the f16r layout");
        CV_TRY(B.conv1.set_exps(in_exp, B.mid.exp, s));
        CV_TRY(B.conv2.set_exps(B.mid.exp, B.out.exp, s));
        L[2 * b] = &B.conv1; L[2 * b + 1] = &B.conv2;
        in_exp = B.out.exp;
    }
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = reinterpret_cast<const char*>(x.base);
    p.w = reinterpret_cast<const char*>(R.chain_w.ptr);
    p.y = reinterpret_cast<char*>(yl.base);
    p.y32 = reinterpret_cast<char*>(yl.base32);
    p.M = n * 256; p.Ho = 16; p.Wo = 16;
    p.xHp = 18; p.xWp = 18; p.stride = 1; p.xCs = 64; p.xCoffBytes = 0;
    p.yHp = 18; p.yWp = 18; p.yCs = 64; p.yCoff = 0;
    p.Cout = 64; p.rows = 64; p.nStages = 18 * nb; p.nCt = 1; p.relu = 1;
    p.flag = e.guard_ptr();
    p.layer_id = BL.conv2.layer_id;
    p.chain = chain_form();
    for (int i = 0; i < 2 * nb; ++i) {
        p.ch_scale[i] = reinterpret_cast<const float*>(L[i]->scale.ptr);
        p.ch_shift[i] = reinterpret_cast<const float*>(L[i]->shift.ptr);
        p.ch_layer_id[i] = L[i]->layer_id;
    }
    p.ch_res0 = reinterpret_cast<const char*>(x.base32);
    for (int b = 0; b + 1 < nb; ++b) p.ch_y32_mid[b] = reinterpret_cast<char*>(R.blocks[b].out.ref(n).base32);
    in_exp = x.exp;
    for (int b = 0; b < nb; ++b) { p.ch_res_mul[b] = std::ldexp(1.f, in_exp - R.blocks[b].out.exp); in_exp = R.blocks[b].out.exp; }
    // the last convolution's epilogue is the kernel's ordinary one (two-workgroup form): its constants in the ordinary fields, the residual
    // is the previous block's f32 output
    p.scale = p.ch_scale[2 * nb - 1]; p.shift = p.ch_shift[2 * nb - 1];
    p.res = p.ch_y32_mid[nb - 2]; p.res_f32 = 1; p.res_mul = p.ch_res_mul[nb - 1]; p.rCs = 64; p.rCoff = 0;
    if (e.profiling) {
        // compulsory bytes: f16 input + its f32 twin, each inner block's f32 output written and read back, f32 + f16 output, weights
        const double px = (double)n * 256 * 64;
        e.prof_begin(("layer1 (" + std::to_string(2 * nb) + " convs, chained)").c_str(), true, 2.0 * nb * 9 * 64 * 64 * 256 * (double)n, s,
                     px * (2 + 4 + 8 * (nb - 1) + 4 + 2) + 2.0 * nb * 9 * 64 * 64 * 2);
        e.prof.back().kernel = "conv3x3_halo_kernel<half_t,64,16x16,CHAIN" + std::to_string(2 * nb) + ">";
    }
    return e.timed_end("layer1 chain launch", conv_halo_chain_launch(p, n, s), s);
}

Status resnet_forward(Engine& e, const void* x, bool x_u8, int n, float* out, bool softmax, hipStream_t s, float* embedding,
                      const InputNorm* norm) {
    if (!e.resnet) return fail(3, "ResNet weights not loaded (call cv_load_resnet or cv_load_resnet18 first)");
    if (norm && !x_u8) return fail(1, "resnet_forward: only a byte input can be normalised");
    Engine::GraphKey key;
    key.flags = (x_u8 ? 1 : 0) | (softmax ? 2 : 0) | (norm ? 4 : 0);
    if (norm) std::memcpy(key.norm_bits, norm, sizeof(key.norm_bits));   // baked into the captured stem launch
    const ForwardShape shape{512, (size_t)64 * 64 * (x_u8 ? 1 : 4), 13, 512};   // one small chunk: a board's 64 squares
    return forward_chunked(e, *e.resnet, shape, key, "cv_resnet18_forward", x, n, out, nullptr, embedding, s,
                           [&](const void* xc, int c, float* o, uint8_t*, float* emb, hipStream_t st) {
                               return resnet_chunk(e, xc, x_u8, c, o, softmax, st, emb, norm);
                           });
}

}  // namespace cv

// the classifier slot's other model rides in this translation unit (Makefile: YOLO; why: the head of yolo_cls.cpp)
#include "yolo_cls.cpp"
