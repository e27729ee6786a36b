// engine.cpp -- weight packing, device buffers, conv launch plumbing and profiling hooks.
#include "engine.h"
#include <algorithm>
#include "models.h"
#include "pointwise.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace cv {

// ---- error plumbing: thread-local message, never abort (SURVEY.md section 8b "Errors") -------------
static thread_local std::string g_err;
static thread_local bool g_capturing = false;
bool& capture_flag() { return g_capturing; }
void set_error(const std::string& msg) { g_err = msg; }
const char* get_error() { return g_err.c_str(); }
Status fail(int code, const std::string& msg) {
    set_error(msg);
    Status s; s.code = code;
    return s;
}
Status hip_fail(hipError_t e, const char* what) {
    return fail(2, std::string(what) + ": " + hipGetErrorString(e));
}

// ---- legacy-stream operations vs graph capture (engine.h) ----------------------------------------
std::shared_mutex& capture_mutex() {
    static std::shared_mutex mu;
    return mu;
}
std::mutex& legacy_mutex() {
    static std::mutex mu;
    return mu;
}
std::shared_mutex& graph_mutex() {
    static std::shared_mutex mu;
    return mu;
}
static std::mutex g_grave_mu;
static std::vector<std::pair<hipGraphExec_t, hipGraph_t>> g_grave;
void graph_bury(hipGraphExec_t exec, hipGraph_t graph) {
    if (!exec && !graph) return;
    { std::lock_guard<std::mutex> lk(g_grave_mu); g_grave.emplace_back(exec, graph); }
    graph_drain();
}
void graph_drain() {
    std::unique_lock<std::shared_mutex> quiet(graph_mutex(), std::try_to_lock);     // nobody is inside hipGraphLaunch
    if (!quiet.owns_lock()) return;
    std::vector<std::pair<hipGraphExec_t, hipGraph_t>> dead;
    { std::lock_guard<std::mutex> lk(g_grave_mu); dead.swap(g_grave); }
    for (auto& d : dead) {
        if (d.first) (void)hipGraphExecDestroy(d.first);
        if (d.second) (void)hipGraphDestroy(d.second);
    }
}
hipError_t sync_memcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    if (capture_flag()) return hipErrorStreamCaptureUnsupported;         // this thread is recording: its caller falls back to an eager run
    std::shared_lock<std::shared_mutex> lk(capture_mutex());
    std::lock_guard<std::mutex> one(legacy_mutex());
    return hipMemcpy(dst, src, n, kind);
}
hipError_t sync_memset(void* dst, int value, size_t n) {
    if (capture_flag()) return hipErrorStreamCaptureUnsupported;
    std::shared_lock<std::shared_mutex> lk(capture_mutex());
    std::lock_guard<std::mutex> one(legacy_mutex());
    const hipError_t e = hipMemset(dst, value, n);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);          // a fill of device memory may return before it has run
}
hipError_t device_synchronize() {
    if (capture_flag()) return hipErrorStreamCaptureUnsupported;
    std::shared_lock<std::shared_mutex> lk(capture_mutex());
    std::lock_guard<std::mutex> one(legacy_mutex());
    return hipDeviceSynchronize();
}
hipError_t copy_to_host_sync(void* dst_pageable, const void* src_dev, size_t n, hipStream_t s) {
    if (capture_flag()) return hipErrorStreamCaptureUnsupported;
    std::shared_lock<std::shared_mutex> lk(capture_mutex());
    std::lock_guard<std::mutex> one(legacy_mutex());
    const hipError_t e = hipMemcpyAsync(dst_pageable, src_dev, n, hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// ---- device memory -------------------------------------------------------------------------------
namespace {
struct BlockCache {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void*> idle[2];       // [host]: (device, block bytes) -> block
    size_t held[2] = {0, 0};
};
BlockCache& block_cache() {
    static BlockCache* c = new BlockCache();                    // never destroyed: engines may be released during process exit
    return *c;
}
bool block_cache_on() {
    static const bool on = env_int("CV_MEM_CACHE", 1) != 0;
    return on;
}
size_t block_cache_limit() {
    static const size_t lim = (size_t)env_int("CV_MEM_CACHE_MB", 16384) << 20;
    return lim;
}
}  // namespace

static int& release_synced_depth() {
    static thread_local int depth = 0;
    return depth;
}
ReleaseAlreadySynced::ReleaseAlreadySynced() { ++release_synced_depth(); }
ReleaseAlreadySynced::~ReleaseAlreadySynced() { --release_synced_depth(); }

hipError_t block_alloc(void** ptr, size_t n, size_t* cap, bool host) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (block_cache_on()) {
        BlockCache& c = block_cache();
        std::lock_guard<std::mutex> lk(c.mu);
        auto it = c.idle[host].lower_bound({dev, n});           // smallest idle block of this device that fits ...
        if (it != c.idle[host].end() && it->first.first == dev && it->first.second <= n + n / 4 + 4096) {   // ... without wasting > 25 %
            *ptr = it->second; *cap = it->first.second;
            c.held[host] -= *cap;
            c.idle[host].erase(it);
            return hipSuccess;
        }
    }
    *cap = n;
    for (int attempt = 0;; ++attempt) {
        hipError_t e;
        {
            std::lock_guard<std::mutex> one(legacy_mutex());
            e = host ? hipHostMalloc(ptr, n, hipHostMallocDefault) : hipMalloc(ptr, n);
        }
        if (e == hipSuccess || attempt == 1) return e;
        (void)hipGetLastError();
        if (block_cache_trim() == 0) return e;                  // out of memory with idle blocks in the cache: hand them back, once
    }
}
void block_release(void* ptr, size_t cap, bool host) {
    if (!ptr) return;
    if (block_cache_on()) {
        // what hipFree did implicitly: nothing queued anywhere still uses the block when its next owner fills it on another stream
        if (release_synced_depth() == 0) (void)device_synchronize();
        int dev = 0;
        (void)hipGetDevice(&dev);
        BlockCache& c = block_cache();
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.held[host] + cap <= block_cache_limit()) {
            c.idle[host].insert({{dev, cap}, ptr});
            c.held[host] += cap;
            return;
        }
    }
    std::lock_guard<std::mutex> one(legacy_mutex());
    if (host) (void)hipHostFree(ptr); else (void)hipFree(ptr);
}
size_t block_cache_trim() {
    BlockCache& c = block_cache();
    std::multimap<std::pair<int, size_t>, void*> dead[2];
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(c.mu);
        for (int h = 0; h < 2; ++h) { dead[h].swap(c.idle[h]); bytes += c.held[h]; c.held[h] = 0; }
    }
    std::lock_guard<std::mutex> one(legacy_mutex());
    (void)hipDeviceSynchronize();
    for (int h = 0; h < 2; ++h)
        for (auto& b : dead[h]) { if (h) (void)hipHostFree(b.second); else (void)hipFree(b.second); }
    return bytes;
}

static bool poison_alloc() {
    static const bool on = env_int("CV_POISON_ALLOC", 0) != 0;
    return on;
}
static int guard_alloc_mode() {
    static const int mode = env_int("CV_GUARD_ALLOC", 0);
    return mode;
}
void DeviceBuffer::release() {
    if (!ptr) return;
    if (!guard_base) { block_release(ptr, cap_bytes, false); ptr = nullptr; cap_bytes = 0; return; }
    std::lock_guard<std::mutex> one(legacy_mutex());
    if (guard_base) {
        (void)hipDeviceSynchronize();
        const size_t guard = (guard_span - guard_mapped) / 2;
        (void)hipMemUnmap((char*)guard_base + guard, guard_mapped);
        (void)hipMemRelease((hipMemGenericAllocationHandle_t)guard_handle);
        // CV_GUARD_KEEP_VA=1: the address range is NOT handed back.  A later reservation can get the same addresses, and kernels then
        // read and write through the translations of the PREVIOUS mapping on this stack (round 6: the second and third precision of
        // an op test got the first one's addresses and computed on its freed pages -- fills and copies, which go another way, saw the
        // new ones; with the ranges kept, all 104 op tests compute the right numbers under the guards).  Keeping every range costs
        // address space and a model load aborts inside the runtime after a few hundred reservations, hence a knob: keep them for
        // numbers on small cases, free them (default) to run whole models for FAULTS only.
        if (!env_int("CV_GUARD_KEEP_VA", 0)) (void)hipMemAddressFree(guard_base, guard_span);
        guard_base = nullptr; guard_handle = nullptr; guard_span = guard_mapped = 0;
        ptr = nullptr;
        return;
    }
    ptr = nullptr;
}
DeviceBuffer::~DeviceBuffer() { release(); }
Status DeviceBuffer::alloc(size_t n, bool zero) {
    release();
    bytes = n;
    if (n == 0) return Status();
    hipError_t e;
    if (const int mode = guard_alloc_mode()) {
        std::lock_guard<std::mutex> one(legacy_mutex());
        int dev = 0;
        (void)hipGetDevice(&dev);
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev;
        size_t gran = 0;
        e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
        if (e != hipSuccess || gran == 0) return fail(4, std::string("CV_GUARD_ALLOC: hipMemGetAllocationGranularity: ") + hipGetErrorString(e));
        const size_t guard = ((size_t)env_int("CV_GUARD_MB", 64) << 20) / gran * gran;             // unmapped bytes on either side
        const size_t mapped = (n + gran - 1) / gran * gran, span = mapped + 2 * guard;
        void* base = nullptr;
        hipMemGenericAllocationHandle_t h{};
        e = hipMemAddressReserve(&base, span, gran, nullptr, 0);
        if (e == hipSuccess) e = hipMemCreate(&h, mapped, &prop, 0);
        if (e == hipSuccess) e = hipMemMap((char*)base + guard, mapped, 0, h, 0);
        hipMemAccessDesc acc{};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        if (e == hipSuccess) e = hipMemSetAccess((char*)base + guard, mapped, &acc, 1);
        if (e != hipSuccess) return fail(4, std::string("CV_GUARD_ALLOC: virtual-memory mapping of ") + std::to_string(n) + " bytes: " + hipGetErrorString(e));
        const size_t align = (size_t)env_int("CV_GUARD_ALIGN", 256);
        guard_base = base; guard_span = span; guard_mapped = mapped; guard_handle = (void*)h;
        ptr = (char*)base + guard + (mode == 1 ? (mapped - n) / align * align : 0);
        if (env_int("CV_GUARD_LOG", 0))
            std::fprintf(stderr, "[guard] buffer %p .. %p (%zu bytes) in reserve %p .. %p\n", ptr, (void*)((char*)ptr + n), n, base, (void*)((char*)base + span));
    } else {
        e = block_alloc(&ptr, n, &cap_bytes, false);
        if (e != hipSuccess) { ptr = nullptr; cap_bytes = 0; return fail(4, std::string("hipMalloc(") + std::to_string(n) + "): " + hipGetErrorString(e)); }
    }
    if (zero) CV_HIP(sync_memset(ptr, 0, n));
    if (zero && guard_base && env_int("CV_GUARD_VERIFY", 0)) {          // debugging the debugging aid: did the fill land where the kernels will read?
        std::vector<unsigned char> back(n, 1);
        CV_HIP(sync_memcpy(back.data(), ptr, n, hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (unsigned char b : back) bad += b != 0;
        std::fprintf(stderr, "[guard] zero fill of %zu bytes at %p: %zu bytes not zero\n", n, ptr, bad);
    }
    else if (!zero && poison_alloc()) CV_HIP(sync_memset(ptr, 0xff, n));     // CV_POISON_ALLOC=1 (debugging): whoever relies on fresh memory being zero reads NaNs
    return Status();
}
Status DeviceBuffer::upload(const void* host, size_t n) {
    CV_TRY(alloc(n, false));
    CV_HIP(sync_memcpy(ptr, host, n, hipMemcpyHostToDevice));
    return Status();
}

Status ResizeTables::replace(const int geom_[4], hipStream_t st, const std::vector<int>& x0, const std::vector<int>& x1, const std::vector<float>& x2,
                             const std::vector<int>& y0, const std::vector<int>& y1, const std::vector<float>& y2, int xstride, int ystride) {
    if (capture_flag()) return fail(3, "resize tables rebuilt during graph capture");
    CV_HIP(hipStreamSynchronize(st));
    std::vector<char> blob;
    const void* const data[6] = {x0.data(), x1.data(), x2.data(), y0.data(), y1.data(), y2.data()};
    const size_t count[6] = {x0.size(), x1.size(), x2.size(), y0.size(), y1.size(), y2.size()};
    size_t at[6];
    for (int i = 0; i < 6; ++i) {                         // ints and floats alike: four bytes per element
        at[i] = blob.size();
        blob.resize(at[i] + ((count[i] * 4 + 15) & ~(size_t)15));
        std::memcpy(blob.data() + at[i], data[i], count[i] * 4);
    }
    std::memset(geom, 0, sizeof geom);                    // no geometry while the upload can still fail
    CV_TRY(buf.upload(blob.data(), blob.size()));
    std::memcpy(off, at, sizeof off);
    stride[0] = xstride; stride[1] = ystride;
    std::memcpy(geom, geom_, sizeof geom);
    return Status();
}

Status Activation::reserve(int cap_) {
    std::vector<Activation*> one{this};
    return reserve_all(one, cap_);
}

Status Activation::reserve_all(const std::vector<Activation*>& acts, int cap_) {
    std::vector<DeviceBuffer> fresh(acts.size()), fresh32(acts.size());
    for (size_t i = 0; i < acts.size(); ++i) {
        const Activation& a = *acts[i];
        const size_t total = a.bytes_per_image() * (size_t)cap_;
        if (total >= ((size_t)1 << 32))
            return fail(1, "activation buffer >= 4 GiB: lower the chunk size (32-bit DMA offsets)");
        if (!a.only32) CV_TRY(fresh[i].alloc(total, /*zero=*/true));   // zero border, written never again
        if (a.want32) {
            const size_t t32 = (size_t)(a.H + 2) * (a.W + 2) * a.C * sizeof(float) * (size_t)cap_;
            if (t32 >= ((size_t)1 << 32)) return fail(1, "f32 trunk buffer >= 4 GiB: lower the chunk size");
            CV_TRY(fresh32[i].alloc(t32, true));
        }
    }
    // nothing can fail from here on: swap the new buffers in, the old ones are freed with `fresh`
    for (size_t i = 0; i < acts.size(); ++i) {
        acts[i]->buf.swap(fresh[i]);
        acts[i]->buf32.swap(fresh32[i]);
        acts[i]->cap = cap_;
    }
    return Status();
}

// ---- implicit-GEMM weight packing ----------------------------------------------------------------
// LDS row R of a channel tile holds the weights of channel tile*CT + conv_row_to_channel(R): inside each
// 64-row wave slab the (fragment f, quad q) fields are swapped so that the lane that owns MFMA rows
// 4q..4q+3 of fragments f = 0..3 ends up with 16 consecutive channels (conv_igemm.hip epilogue).
static inline int conv_row_to_channel(int R) {
    const int slab = R / 64, within = R % 64;
    return slab * 64 + frag_row_channel(kConvFC, within / 16, within % 16);
}

int row_exponent(const float* row, int n) {
    float m = 0.f;
    for (int k = 0; k < n; ++k) m = std::max(m, std::fabs(row[k]));
    int e = 0;
    if (m > 0.f) (void)std::frexp(m, &e);
    return e;
}
int normalise_row(float* row, int n) {
    const int e = row_exponent(row, n);
    if (e != 0)
        for (int k = 0; k < n; ++k) row[k] = std::ldexp(row[k], -e);
    return e;
}

// A K row is a sequence of 16-byte chunks.  chunk_k0 / chunk_is_lo describe what chunk kc of the row holds:
//   f16  : 8 values k0..k0+7             f32 : 4 values k0..k0+3
//   split: K-group kg = kc/2 (8 values); even kg = [hi chunk, lo chunk], odd kg = [lo chunk, hi chunk]
static inline int chunks_for(int dt, int K) { return dt == kF32 ? (K + 3) / 4 : dt == kF16 ? (K + 7) / 8 : 2 * ((K + 7) / 8); }
static inline int chunk_k0(int dt, int kc) { return dt == kF32 ? kc * 4 : dt == kF16 ? kc * 8 : (kc / 2) * 8; }
static inline bool chunk_is_lo(int dt, int kc) { return dt == kSplit && ((kc & 1) != ((kc / 2) & 1)); }

static void pack_rows(int dt, std::vector<char>& out, int CT, int nCt, int nStages, int rows, int K,
                      const std::vector<float>& Wk /* [rows][K] */) {
    out.assign((size_t)nCt * nStages * CT * 128, 0);
    const int per = dt == kF32 ? 4 : 8;                    // values per chunk
    for (int t = 0; t < nCt; ++t)
        for (int s = 0; s < nStages; ++s)
            for (int R = 0; R < CT; ++R) {
                const int row = t * CT + conv_row_to_channel(R);
                for (int pos = 0; pos < 8; ++pos) {
                    const int kc = s * 8 + (pos ^ (R & 7));
                    char* d = out.data() + (((size_t)(t * nStages + s) * CT + R) * 8 + pos) * 16;
                    const int k0 = chunk_k0(dt, kc);
                    const bool lo = chunk_is_lo(dt, kc);
                    for (int e = 0; e < per; ++e) {
                        const int kk = k0 + e;
                        const float v = (row < rows && kk < K) ? Wk[(size_t)row * K + kk] : 0.f;
                        if (dt == kF32) reinterpret_cast<float*>(d)[e] = v;
                        else reinterpret_cast<_Float16*>(d)[e] = f16_half(v, lo);
                    }
                }
            }
}

static Status finish_layer(ConvLayer& L, std::vector<float>& Wk, int K, const std::vector<float>& scale,
                           const std::vector<float>& shift) {
    if (L.keep_host_weights && L.Wk0.empty()) { L.Wk0 = Wk; L.b_scale = scale; L.b_shift = shift; L.Kdim = K; }
    // experiment knob: channel tile of the k2 s2 transposed convolutions (64 -> the 80 KB 64x256 tile, two workgroups per CU)
    static const int convt_ct = env_int("CV_CONVT_CT", 0);
    const int CT = L.ct = (L.shuffle && (convt_ct == 64 || convt_ct == 128) && L.rows % convt_ct == 0)
                              ? convt_ct : choose_ct(L.rows, L.pixels_hint, L.halo_ok);
    L.nStages = (chunks_for(L.dt, K) + 7) / 8;
    L.nCt = (L.rows + CT - 1) / CT;
    L.rowsPad = L.nCt * CT;
    // Loud failure instead of silent NaNs downstream: a checkpoint with non-finite weights or a BatchNorm whose
    // running_var + eps is not positive cannot be evaluated in any precision.
    for (size_t i = 0; i < Wk.size(); ++i)
        if (!std::isfinite(Wk[i])) return fail(1, L.name + ": non-finite weight in the state dict");
    for (int r = 0; r < L.rows; ++r)
        if (!std::isfinite(scale[r]) || !std::isfinite(shift[r]))
            return fail(1, L.name + ": non-finite BatchNorm scale/shift for output channel " + std::to_string(r) +
                           " (running_var + eps <= 0, or non-finite statistics)");
    // Row normalisation (models.h: normalise_row; |w| ~ 1e-2 would otherwise keep 17 of its 22 bits, |w| ~ 1e-3 only 14)
    L.h_scale.assign(L.rowsPad, 0.f);
    L.h_shift.assign(L.rowsPad, 0.f);
    for (int r = 0; r < L.rows; ++r) {
        const int e = L.dt != kF32 ? normalise_row(&Wk[(size_t)r * K], K) : 0;
        L.h_scale[r] = std::ldexp(scale[r], e);
        L.h_shift[r] = shift[r];
        if (!std::isfinite(L.h_scale[r])) return fail(1, L.name + ": weight magnitude x BatchNorm scale leaves the f32 range");
    }
    L.h_shift_base = L.h_shift;
    if (L.want_round_err && L.dt == kF16) {             // (w - w_hat) of the normalised rows, for the rounding-bias correction
        L.Kerr = K;
        L.h_round_err.resize((size_t)L.rows * K);
        for (size_t i = 0; i < L.h_round_err.size(); ++i) L.h_round_err[i] = Wk[i] - (float)(_Float16)Wk[i];
        L.tap_sum.clear(); L.tap_count = 0;
    }
    std::vector<char> packed;
    pack_rows(L.dt, packed, CT, L.nCt, L.nStages, L.rows, K, Wk);
    CV_TRY(L.w.upload(packed.data(), packed.size()));
    if (CT == 256) {
        // small launches (single boards, tail chunks) cannot fill the chip with 256x256 workgroups: keep a second copy
        // packed for 128-row tiles and pick per launch
        pack_rows(L.dt, packed, 128, L.rows / 128, L.nStages, L.rows, K, Wk);
        CV_TRY(L.w_small.upload(packed.data(), packed.size()));
    }
    L.in_exp = L.out_exp = 0;
    CV_TRY(L.scale.upload(L.h_scale.data(), L.h_scale.size() * sizeof(float)));
    CV_TRY(L.shift.upload(L.h_shift.data(), L.h_shift.size() * sizeof(float)));
    L.koff.clear();
    return Status();
}

static inline void k_decode(int kgroup, int ntaps, int kk, int* tap, int* ci);

// Consumer of a concatenated buffer whose halves carry different exponents: input channels >= split are held 2^delta smaller than
// the first half's scale says, so their weights take the factor (a power of two: exact), then the rows are re-normalised and
// re-packed.  Happens during load-time calibration only.
Status ConvLayer::set_input_split(int split, int delta, hipStream_t s) {
    if (split == in_split && delta == in_delta) return Status();
    if (capture_flag()) return fail(1, name + ": weights re-packed during graph capture");
    if (Wk0.empty()) return fail(1, name + ": the halves of its concatenated input need different exponents but the layer kept no host weights");
    CV_HIP(hipStreamSynchronize(s));
    std::vector<float> Wk = Wk0;
    const int ntaps = k * k;
    if (delta != 0)
        for (int kk = 0; kk < Kdim; ++kk) {
            int tap, ci;
            k_decode(kgroup, ntaps, kk, &tap, &ci);
            if (ci < split) continue;
            for (int r = 0; r < rows; ++r) Wk[(size_t)r * Kdim + kk] = std::ldexp(Wk[(size_t)r * Kdim + kk], delta);
        }
    in_split = split; in_delta = delta;
    return finish_layer(*this, Wk, Kdim, b_scale, b_shift);
}

// shift[r] += scale[r] * sum_k (w - w_hat)[r][k] * mean(x_stored[k]) * 2^in_exp -- see ConvLayer::want_round_err
Status ConvLayer::fold_rounding_bias() {
    if (h_round_err.empty() || tap_sum.empty() || tap_count <= 0 || (int)tap_sum.size() != Kerr || h_shift_base.size() != h_shift.size())
        return Status();
    for (int r = 0; r < rows; ++r) {
        const float* e = h_round_err.data() + (size_t)r * Kerr;
        double acc = 0.0;
        for (int k = 0; k < Kerr; ++k) acc += (double)e[k] * tap_sum[(size_t)k];
        const double corr = std::ldexp(acc / tap_count * (double)h_scale[r], tap_in_exp);
        if (!std::isfinite(corr)) return fail(1, name + ": rounding-bias correction is not finite");
        h_shift[r] = (float)((double)h_shift_base[r] + corr);
    }
    in_exp = out_exp = 1 << 20;                         // no tensor carries this exponent: the next set_exps re-uploads
    return Status();
}

Status fold_exps(const std::string& name, const std::vector<float>& h_scale, const std::vector<float>& h_shift, void* scale, void* shift,
                 int in_exp, int out_exp, hipStream_t s) {
    if (capture_flag()) return fail(1, name + ": epilogue constants re-folded during graph capture");
    CV_HIP(hipStreamSynchronize(s));                     // launches that still read the old constants
    std::vector<float> sc(h_scale.size()), sh(h_shift.size());
    for (size_t i = 0; i < sc.size(); ++i) {
        sc[i] = std::ldexp(h_scale[i], in_exp - out_exp);
        sh[i] = std::ldexp(h_shift[i], -out_exp);
        if (!std::isfinite(sc[i]) || !std::isfinite(sh[i])) return fail(1, name + ": range factors leave the f32 range");
    }
    CV_HIP(sync_memcpy(scale, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice));
    CV_HIP(sync_memcpy(shift, sh.data(), sh.size() * sizeof(float), hipMemcpyHostToDevice));
    return Status();
}

// Re-fold the tensor exponents into the device copies of the epilogue constants (only when they change: calibration).
Status ConvLayer::set_exps(int in_exp_, int out_exp_, hipStream_t s) {
    if (in_exp_ == in_exp && out_exp_ == out_exp) return Status();
    CV_TRY(fold_exps(name, h_scale, h_shift, scale.ptr, shift.ptr, in_exp_, out_exp_, s));
    in_exp = in_exp_; out_exp = out_exp_;
    return Status();
}

// K ordering of a k x k convolution: K = [channel block cb][tap][channel inside the block], with blocks of
// kgroup = one 128-byte line of input channels (32 f32/split values, 64 f16 values).  All k*k taps of a channel
// block are therefore read in consecutive stages: the 9-fold re-read of an input line by the implicit GEMM hits
// L2 instead of going back to the fabric (measured r01: 7.6x algorithmic fetch traffic with tap-major order).
static int kgroup_for(int dt, int cinPad) {
    const int line = 128 / dtype_size(dt);
    return cinPad % line == 0 ? line : cinPad;
}
static inline int k_index(int kgroup, int ntaps, int tap, int ci) {
    return ((ci / kgroup) * ntaps + tap) * kgroup + ci % kgroup;
}
static inline void k_decode(int kgroup, int ntaps, int kk, int* tap, int* ci) {
    const int cb = kk / (ntaps * kgroup), rem = kk % (ntaps * kgroup);
    *tap = rem / kgroup;
    *ci = cb * kgroup + rem % kgroup;
}

Status ConvLayer::build_conv(const std::string& name_, int dt_, const float* w_oihw, int cout_, int cin_, int k_,
                             int stride_, const float* scale_, const float* shift_, int cinPad_, int64_t pixels_hint_, int out_hw_) {
    name = name_; dt = dt_; cin = cin_; cinPad = cinPad_; cout = cout_; k = k_; stride = stride_;
    shuffle = false; rows = cout_; pixels_hint = pixels_hint_;
    want_round_err = dt_ == kF16 && calibration_enabled() && bias_correction_enabled();
    halo_ok = k_ == 3 && stride_ == 1 && out_hw_ > 0 && (out_hw_ % 16 == 0 || (out_hw_ == 8 && cout_ % 128 == 0)) &&
              cinPad_ % (128 / dtype_size(dt_)) == 0;
    if (cinPad % 8 || cinPad < cin) return fail(1, name + ": input channel padding must be a multiple of 8");
    if (k != 1 && k != 3) return fail(1, name + ": implicit-GEMM path supports 1x1 and 3x3 kernels");
    if (cout % 16) return fail(1, name + ": output channels must be a multiple of 16");
    const int K = k * k * cinPad;
    kgroup = kgroup_for(dt, cinPad);
    std::vector<float> Wk((size_t)rows * K, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx)
                    Wk[(size_t)co * K + k_index(kgroup, k * k, ky * k + kx, ci)] = w_oihw[(((size_t)co * cin + ci) * k + ky) * k + kx];
    std::vector<float> sc(scale_, scale_ + cout), sh(shift_, shift_ + cout);
    return finish_layer(*this, Wk, K, sc, sh);
}

Status ConvLayer::build_convT(const std::string& name_, int dt_, const float* w_iohw, int cin_, int cout_,
                              const float* bias, int64_t pixels_hint_) {
    name = name_; dt = dt_; cin = cin_; cinPad = cin_; cout = cout_; k = 1; stride = 1;
    shuffle = true; rows = 4 * cout_; pixels_hint = pixels_hint_;
    if (cin % 8) return fail(1, name + ": transposed-conv input channels must be a multiple of 8");
    if (cout % 16) return fail(1, name + ": transposed-conv output channels must be a multiple of 16");
    const int K = cin;
    kgroup = cin;
    std::vector<float> Wk((size_t)rows * K, 0.f), sc(rows, 1.f), sh(rows, 0.f);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int d = 0; d < 4; ++d)      // d = dy*2 + dx
                Wk[(size_t)(d * cout + co) * K + ci] = w_iohw[((size_t)ci * cout + co) * 4 + d];
    for (int d = 0; d < 4; ++d)
        for (int co = 0; co < cout; ++co) sh[d * cout + co] = bias[co];
    return finish_layer(*this, Wk, K, sc, sh);
}

// byte offset of every 16-B K chunk relative to the address of the pixel's top-left tap
Status ConvLayer::get_koff(const TensorRef& x, const int** chunks, const int** bases) {
    const KoffKey key{x.W + 2, x.Cs, x.Coff};
    auto it = koff.find(key);
    if (it == koff.end()) {
        if (capture_flag()) return fail(1, name + ": offset table created during graph capture");
        const int esz = dtype_size(dt);
        const int K = k * k * cinPad;
        const int pad = (k - 1) / 2;
        std::vector<int> tab((size_t)nStages * 8, 0);
        for (int kc = 0; kc < nStages * 8; ++kc) {
            int kk = chunk_k0(dt, kc);
            if (kk >= K) kk = 0;                         // zero weights there; keep the gather on real data
            int tap, ci;
            k_decode(kgroup, k * k, kk, &tap, &ci);
            const int ky = tap / k, kx = tap % k;
            long long off = ((long long)((ky + 1 - pad) * key.xWp + (kx + 1 - pad)) * x.Cs + x.Coff + ci) * esz;
            if (dt == kSplit) {                          // pick the hi or lo chunk of the 32-byte channel group
                const bool odd_group = (((x.Coff + ci) / 8) & 1) != 0;
                const bool want_lo = chunk_is_lo(dt, kc);
                off += (want_lo != odd_group) ? 16 : 0;  // even group: [hi, lo]; odd group: [lo, hi]
            }
            tab[kc] = (int)off;
        }
        auto kt = std::make_unique<KoffTab>();
        CV_TRY(kt->chunks.upload(tab.data(), tab.size() * sizeof(int)));
        std::vector<int> base((size_t)nStages);
        kt->separable = true;
        for (int s = 0; s < nStages; ++s) {
            base[s] = tab[(size_t)s * 8];
            for (int c = 0; c < 8; ++c) kt->separable = kt->separable && tab[(size_t)s * 8 + c] == base[s] + 16 * c;
        }
        if (kt->separable) { CV_TRY(kt->bases.upload(base.data(), base.size() * sizeof(int))); kt->h_bases = base; }
        it = koff.emplace(key, std::move(kt)).first;
    }
    *chunks = reinterpret_cast<const int*>(it->second->chunks.ptr);
    *bases = it->second->separable ? reinterpret_cast<const int*>(it->second->bases.ptr) : nullptr;
    return Status();
}

// Position-major launches: for every output position (oy, ox) the list of K stages whose tap (ky, kx) lands on a real input pixel --
// iy = oy * stride + ky - 1 in [0, H), ix likewise -- in K order, each as {stage index (selects the weight slab), gather base of that
// stage}.  Stages of taps that would read the zero border contribute exact zeros and are left out.  3x3 / pad-1 layers whose stages hold
// one tap each (Cin a multiple of the 128-byte line, i.e. table-free offsets) only.
Status ConvLayer::get_pos(const TensorRef& x, int Ho, int Wo, const int** tab, const int** count, const int** order, double* live) {
    const PosKey key{x.H + 2, x.W + 2, x.Cs, x.Coff};
    auto it = pos.find(key);
    if (it == pos.end()) {
        if (capture_flag()) return fail(1, name + ": position table created during graph capture");
        const int* chunks = nullptr;
        const int* bases = nullptr;
        CV_TRY(get_koff(x, &chunks, &bases));
        const auto kt = koff.find(KoffKey{x.W + 2, x.Cs, x.Coff});
        if (k != 3 || shuffle || !bases || kt == koff.end() || (int)kt->second->h_bases.size() != nStages || nStages % 9 != 0)
            return fail(1, name + ": layer cannot run position-major");
        std::vector<int> t((size_t)Ho * Wo * nStages * 2, 0), cnt((size_t)Ho * Wo, 0);
        long long total = 0;
        for (int oy = 0; oy < Ho; ++oy)
            for (int ox = 0; ox < Wo; ++ox) {
                const int ps = oy * Wo + ox;
                int n = 0;
                for (int s = 0; s < nStages; ++s) {
                    int tap, ci;
                    k_decode(kgroup, 9, chunk_k0(dt, s * 8), &tap, &ci);      // a stage = one tap of one channel block
                    const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
                    if (iy < 0 || iy >= x.H || ix < 0 || ix >= x.W) continue;
                    t[((size_t)ps * nStages + n) * 2] = s;
                    t[((size_t)ps * nStages + n) * 2 + 1] = kt->second->h_bases[(size_t)s];
                    ++n;
                }
                cnt[(size_t)ps] = n;
                total += n;
            }
        auto pt = std::make_unique<PosTab>();
        CV_TRY(pt->tab.upload(t.data(), t.size() * sizeof(int)));
        CV_TRY(pt->count.upload(cnt.data(), cnt.size() * sizeof(int)));
        std::vector<int> ord((size_t)Ho * Wo);                      // positions by falling stage count (ties: raster order)
        for (size_t i = 0; i < ord.size(); ++i) ord[i] = (int)i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return cnt[(size_t)a] > cnt[(size_t)b]; });
        CV_TRY(pt->order.upload(ord.data(), ord.size() * sizeof(int)));
        pt->live = (double)total / ((double)Ho * Wo * nStages);
        it = pos.emplace(key, std::move(pt)).first;
    }
    *tab = reinterpret_cast<const int*>(it->second->tab.ptr);
    *count = reinterpret_cast<const int*>(it->second->count.ptr);
    *order = reinterpret_cast<const int*>(it->second->order.ptr);
    *live = it->second->live;
    return Status();
}

// experiment switches (documented in DESIGN.md / r01_tuning.md); each is read from the environment once per process
int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}
bool env_switch(const char* name, bool dflt) {
    const char* v = std::getenv(name);
    return v && (v[0] == '0' || v[0] == '1') ? v[0] == '1' : dflt;
}
struct Knobs {
    int halo = env_int("CV_HALO", 1), ct256 = env_int("CV_CT256", 1), ct256_min_blocks = env_int("CV_CT256_MIN_BLOCKS", 256);
    int n64 = env_int("CV_N64", 1), sep = env_int("CV_CONV_SEP", 1), fuse_pool = env_int("CV_FUSE_POOL", 1);
    // split-K for launches that cannot fill the chip (single boards, the 64-square classifier batch; r04_tuning.md):
    //   splitk            0 = off
    //   splitk_max_tiles  launches with at least this many output tiles run unsplit
    //   splitk_target     workgroups the chip runs at once (2 per CU): more than that and the K loops queue behind each other
    int splitk = env_int("CV_SPLITK", 1), splitk_max_tiles = env_int("CV_SPLITK_MAX_TILES", 192);
    int splitk_target = env_int("CV_SPLITK_TARGET", 512);
    int splitk_force = env_int("CV_SPLITK_FORCE", 0);   // tests: this many splits on every launch that can take them
    int halo_th8 = env_int("CV_HALO_TH8", 1), halo_th8_max_tiles = env_int("CV_HALO_TH8_MAX_TILES", 384);
    int splitk_halo = env_int("CV_SPLITK_HALO", 1);     // 3x3 layers on maps >= 16 x 16 split inside the halo kernel (by channel blocks)
    int splitk_halo_stage_ns = env_int("CV_SPLITK_HALO_STAGE_NS", 500);
    // two independent layers in one launch (Engine::PendingConv): only while their workgroups together leave the chip unfilled
    int pair = env_int("CV_PAIR", 1), pair_max_blocks = env_int("CV_PAIR_MAX_BLOCKS", 512);
    // position-major rows + live-tap stage lists (ConvParams::ptab): 0 = off; at least pos_min_tiles pixel tiles of images per position;
    // maps up to pos_max_hw on a side
    int pos = env_int("CV_POS", 1), pos_min_tiles = env_int("CV_POS_MIN_TILES", 1), pos_max_hw = env_int("CV_POS_MAX_HW", 8);
    int pos_small_ct = env_int("CV_POS_SMALL_CT", 1);   // 128-row tiles for position-major launches of under two rounds with unequal positions
};
static const Knobs& knobs() {
    static const Knobs k;
    return k;
}

// Tile / ring-depth choice, from the r01 sweeps on MI355X (profiles/r01_tuning.md):
//   Cout % 128 == 0, >= 256 workgroups of 128x256 : 8-wave 128x256 tile, ring 3 (two waves per SIMD in ONE workgroup)
//   Cout % 128 == 0, fewer pixels                 : 4-wave 128x128 tile; ring 3 at <= 1 workgroup per CU, else ring 2
//   Cout == 64 (full-resolution UNet, ResNet layer1): 4-wave 64x256 tile, ring 2, table-free offsets (80 KB -> two
//                                                   workgroups per CU); 64x128 ring 3 for short K or few pixels
// CV_CONV_W8 / CV_CONV_PT / CV_CONV_NS override for experiments.
static int64_t blocks_for(int rows, int64_t pixels, int ct, int pt) {
    return ((pixels + pt - 1) / pt) * ((rows + ct - 1) / ct);
}

static int env_cached(int idx) {                      // 0: CV_CONV_W8, 1: CV_CONV_PT, 2: CV_CONV_NS
    static const int v[3] = {env_int("CV_CONV_W8", -1), env_int("CV_CONV_PT", 0), env_int("CV_CONV_NS", 0)};
    return v[idx];
}

// channel-tile height of a layer: fixed at pack time (weights are packed per channel tile).  256-row tiles (fewest
// L2->LDS bytes per MFMA: the r01 ablation shows the DMA side alone costs 60-85 % of a layer's time) are used when
// the layer still fills the chip with 256x256 workgroups at the engine's chunk size.
int choose_ct(int rows, int64_t pixels_hint, bool halo_ok) {
    // The 64-row halo tile (4 waves, single halo buffer, two workgroups per CU) beats the 128-row 8-wave tile on every UNet layer it
    // was tried on, 64 to 1024 output channels (r02_tuning.md step 14: two resident workgroups cover each other's barrier, DMA-issue
    // and epilogue phases; the halo of a patch is simply fetched once per 64-channel tile, from L2), and on the packed 8x8-image
    // mode (ResNet-18 layer2): +3-7 %.  It is the halo kernel's only channel tile.
    if (halo_ok && knobs().halo) return 64;
    if (rows % 256 == 0 && knobs().ct256 && blocks_for(rows, pixels_hint, 256, 256) >= knobs().ct256_min_blocks)
        return 256;
    return rows % 128 == 0 ? 128 : 64;
}

// per-launch tile choice among the configurations that share the layer's channel tile
int choose_cfg(int ct, int rows, int64_t pixels, int n_stages) {
    if (ct == 256) return kCfg256x256w8;
    const bool wide = ct == 128;
    const int w8 = env_cached(0), force_pt = env_cached(1);
    if (force_pt == 128 || force_pt == 256)
        return force_pt == 256 ? (wide ? kCfg128x256w8 : kCfg64x256) : (wide ? kCfg128x128 : kCfg64x128);
    if (!wide) {
        if (knobs().n64 == 1 && n_stages > 4 && blocks_for(rows, pixels, 64, 256) >= 512) return kCfg64x256;
        return kCfg64x128;
    }
    if (w8 != 0 && blocks_for(rows, pixels, 128, 256) >= 256) return kCfg128x256w8;
    return kCfg128x128;
}

int choose_ns(int cfg, int dt, int rows, int64_t pixels, int n_stages) {
    (void)dt;
    const int forced = env_cached(2);
    if ((forced == 2 || forced == 3) && conv_cfg_has_ns(cfg, forced)) return forced;
    if (cfg == kCfg128x128) return blocks_for(rows, pixels, 128, 128) > 256 ? 2 : 3;
    if (cfg == kCfg64x256) return 2;                    // 80 KB table-free -> two workgroups per CU
    if (cfg == kCfg64x128 && n_stages <= 4) return 2;   // 3-stage first layer: 48 KB -> three workgroups per CU (+14 %, r01 step 23)
    return conv_cfg_has_ns(cfg, 3) ? 3 : 2;
}

bool calibration_enabled() {
    static const bool on = env_int("CV_CALIBRATE", 1) != 0;
    return on;
}
bool bias_correction_enabled() {
    static const bool on = env_int("CV_BIAS_CORR", 1) != 0;
    return on;
}

// ---- engine --------------------------------------------------------------------------------------
Engine::Engine() {
    layer_names.push_back("input tensor");
    graphs_on = env_int("CV_GRAPH", 1) != 0;
}
Engine::~Engine() {
    prof_clear();
    graph_clear();
    if (capture_stream) (void)hipStreamDestroy(capture_stream);
    if (pipe_host) block_release(pipe_host, pipe_host_cap, true);
    if (pipe_event) (void)hipEventDestroy(pipe_event);
    if (pipe_event2) (void)hipEventDestroy(pipe_event2);
    if (pipe_event3) (void)hipEventDestroy(pipe_event3);
    if (jpeg_enc_done) (void)hipEventDestroy(jpeg_enc_done);
    if (pipe_side) (void)hipStreamDestroy(pipe_side);
}

void Engine::graph_clear() {
    for (auto& g : graphs) {
        graph_bury(g.exec, g.graph);
    }
    graphs.clear();
}

Status Engine::order_forward(int model, hipStream_t s) {
    const int m = model & 1;
    if (last_stream_set[m] && last_stream[m] != s) {
        if (capture_flag()) return fail(1, "stream change during graph capture");
        const hipError_t e = hipStreamSynchronize(last_stream[m]);           // the previous forward of this model has left the workspace
        if (e != hipSuccess) (void)hipGetLastError();                        // (a stream destroyed meanwhile has nothing in flight)
    }
    last_stream[m] = s;
    last_stream_set[m] = true;
    return Status();
}

unsigned Engine::register_layer(const std::string& name) {
    for (size_t i = 0; i < layer_names.size(); ++i)
        if (layer_names[i] == name) return (unsigned)i;
    layer_names.push_back(name);
    return (unsigned)(layer_names.size() - 1);
}

Status Engine::guard_init() {
    if (guard.ptr) return Status();
    CV_TRY(guard.alloc(sizeof(unsigned), false));
    CV_HIP(sync_memset(guard.ptr, 0xff, sizeof(unsigned)));
    CV_TRY(cal_word.alloc(sizeof(unsigned), true));
    return Status();
}

// The same check in two halves for callers that synchronise anyway (cv_process_image): the guard word travels to PAGE-LOCKED memory with
// the call's other downloads and is looked at after the caller's own synchronisation -- guard_check's copy into pageable memory plus
// its stream synchronisation cost ~15-20 us per engine on an otherwise finished stream.
Status Engine::guard_read_async(unsigned* pinned, hipStream_t s) {
    *pinned = 0xffffffffu;
    if (!guard.ptr) return Status();
    CV_HIP(hipMemcpyAsync(pinned, guard.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    return Status();
}

Status Engine::guard_eval(unsigned v) {
    if (v == 0xffffffffu) return Status();
    CV_HIP(sync_memset(guard.ptr, 0xff, sizeof(unsigned)));
    const std::string who = v < layer_names.size() ? layer_names[v] : ("layer #" + std::to_string(v));
    if (v == 0) return fail(5, "non-finite value (NaN / inf) in the input tensor");
    return fail(5, "non-finite value produced by '" + who + "': an activation left the range the " +
                       (dt == kF32 ? std::string("f32") : std::string("f16-based")) +
                       " engine can hold (|x| > 65504 * 2^exp after calibration) or a NaN reached it; results of this "
                       "call are invalid -- use precision f32 for this checkpoint");
}

Status Engine::guard_check(hipStream_t s) {
    if (!guard.ptr) return Status();
    unsigned v = 0xffffffffu;
    CV_HIP(copy_to_host_sync(&v, guard.ptr, sizeof(v), s));
    return guard_eval(v);
}

// calibration: real-valued absolute maximum of the tensor just produced
Status Engine::measure(const TensorRef& t, hipStream_t s) {
    Activation* a = static_cast<Activation*>(t.owner);
    if (!a) return Status();
    CV_HIP(hipMemsetAsync(cal_word.ptr, 0, sizeof(unsigned), s));
    CV_HIP(absmax(t.f32_only ? (int)kF32 : dt, t, reinterpret_cast<unsigned*>(cal_word.ptr), s));
    unsigned bits = 0;
    CV_HIP(copy_to_host_sync(&bits, cal_word.ptr, sizeof(bits), s));
    const bool second = a->split_c && t.Coff >= a->split_c;         // producers write one half of a concatenation each
    if (bits >= 0x7f800000u) { (second ? a->seen_bad2 : a->seen_bad) = true; return Status(); }
    float stored;
    std::memcpy(&stored, &bits, sizeof(stored));
    float& seen = second ? a->seen_max2 : a->seen_max;
    seen = std::max(seen, std::ldexp(stored, t.exp));
    return Status();
}

// rounding-bias calibration: accumulate, for K index k = (channel block, tap, channel), the sum of the layer's stored input under that
// tap over this launch's images and output positions (in units of the FIRST half's exponent: a concatenated input's second half is
// held 2^exp_delta smaller, and its weights carry that factor -- ConvLayer::set_input_split -- so stored values are what the MFMA sees)
Status Engine::measure_tap_sums(ConvLayer& L, const TensorRef& x, int Ho, int Wo, hipStream_t s) {
    if (L.h_round_err.empty() || L.dt != kF16 || L.shuffle || x.f32_only) return Status();
    const int taps = L.k * L.k, C = x.C;
    if (L.Kerr != taps * L.cinPad || C != L.cinPad) return Status();
    const int slices = std::min(x.N, 64);
    const size_t need = (size_t)slices * taps * C * sizeof(double);
    if (bias_ws.bytes < need) CV_TRY(bias_ws.alloc(std::max(need, (size_t)1 << 20), false));
    CV_HIP(tap_sums_f16(x, Ho, Wo, L.stride, L.k, slices, reinterpret_cast<double*>(bias_ws.ptr), s));
    std::vector<double> part((size_t)slices * taps * C);
    CV_HIP(copy_to_host_sync(part.data(), bias_ws.ptr, need, s));
    if (L.tap_sum.empty()) { L.tap_sum.assign((size_t)L.Kerr, 0.0); L.tap_in_exp = x.exp; }
    if (L.tap_in_exp != x.exp) return fail(1, L.name + ": input exponent changed inside the rounding-bias pass");
    for (int kk = 0; kk < L.Kerr; ++kk) {
        int tap, ci;
        k_decode(L.kgroup, taps, kk, &tap, &ci);
        double t = 0.0;
        for (int sl = 0; sl < slices; ++sl) t += part[((size_t)sl * taps + tap) * C + ci];      // fixed order: reproducible
        L.tap_sum[(size_t)kk] += t;
    }
    L.tap_count += (double)x.N * Ho * Wo;
    return Status();
}

size_t Engine::workspace_bytes() const {
    size_t total = 0;
    for (const ModelBase* M : {(const ModelBase*)unet.get(), (const ModelBase*)resnet.get(), (const ModelBase*)yolo.get()})
        if (M) for (const Activation* a : M->acts) total += a->buf.bytes + a->buf32.bytes;
    return total;
}

// ---- what the model plans share (models.h) ---------------------------------------------------------------------------------------
Status need(const ParamMap& pm, const std::string& key, std::vector<int64_t> shape, const float** out) {
    auto it = pm.find(key);
    if (it == pm.end()) return fail(1, "state dict is missing key '" + key + "'");
    if (it->second.shape != shape) {
        std::string got, want;
        for (auto d : it->second.shape) got += std::to_string(d) + ",";
        for (auto d : shape) want += std::to_string(d) + ",";
        return fail(1, "state dict key '" + key + "' has shape (" + got + ") expected (" + want + ")");
    }
    *out = it->second.data;
    return Status();
}

Status bn_fold(const ParamMap& pm, const std::string& prefix, int c, std::vector<float>& scale, std::vector<float>& shift, float eps) {
    const float *g, *b, *m, *v;
    CV_TRY(need(pm, prefix + ".weight", {c}, &g));
    CV_TRY(need(pm, prefix + ".bias", {c}, &b));
    CV_TRY(need(pm, prefix + ".running_mean", {c}, &m));
    CV_TRY(need(pm, prefix + ".running_var", {c}, &v));
    scale.resize(c); shift.resize(c);
    for (int i = 0; i < c; ++i) {
        const float s = g[i] / std::sqrt(v[i] + eps);
        scale[i] = s;
        shift[i] = b[i] - m[i] * s;
    }
    return Status();
}

Status build_conv_bn(Engine& e, ConvLayer& L, const ParamMap& pm, const std::string& conv_key, const std::string& bn_key, int cout,
                     int cin, int k, int stride, int cinPad, int64_t pixels, int out_hw, int layer_dt, float bn_eps) {
    const float* w;
    CV_TRY(need(pm, conv_key + ".weight", {cout, cin, k, k}, &w));
    std::vector<float> sc, sh;
    CV_TRY(bn_fold(pm, bn_key, cout, sc, sh, bn_eps));
    CV_TRY(L.build_conv(conv_key, layer_dt < 0 ? e.dt : layer_dt, w, cout, cin, k, stride, sc.data(), sh.data(), cinPad, pixels, out_hw));
    L.layer_id = e.register_layer(conv_key);
    return Status();
}

void bn_keys(std::vector<std::string>& out, const std::string& p) {
    for (const char* leaf : {".weight", ".bias", ".running_mean", ".running_var"}) out.push_back(p + leaf);
}

Status reject_unknown_keys(const ParamMap& pm, const std::vector<std::string>& known, const char* model) {
    for (const auto& kv : pm) {
        bool ok = false;
        for (const auto& k : known)
            if (kv.first == k) { ok = true; break; }
        if (!ok) return fail(1, std::string("state dict has key '") + kv.first + "' that " + model + " does not define");
    }
    return Status();
}

Status model_reserve(Engine& e, ModelBase& M, int n) {
    const int want = std::min(M.max_cap, std::max(n, 1));
    if (want <= M.cap) return Status();
    CV_HIP(device_synchronize());                    // nothing may still read the buffers about to be replaced
    e.graph_invalidate();                            // captured launches hold the old buffers
    CV_TRY(Activation::reserve_all(M.acts, want));
    M.cap = want;
    M.taps.clear();
    M.build_taps(e, want);
    return Status();
}

bool ModelBase::tap(const std::string& name, TensorRef* out) const {
    auto it = taps.find(name);
    if (it == taps.end()) return false;
    *out = it->second;
    out->exp = static_cast<Activation*>(out->owner)->exp_of(out->Coff);   // per half of a concatenation; `exp` of any other tensor
    out->N = last_n;
    return true;
}

static bool halo_th8_for(const ConvLayer& L, const ConvParams& p, int ct, int Ho, bool fused) {
    const int64_t wgs = blocks_for(L.rows, p.M, ct, 256) * (p.ksplit > 1 ? p.ksplit : 1);
    return !fused && Ho != 8 && knobs().halo_th8 && wgs < knobs().halo_th8_max_tiles;
}

bool Engine::epilogue_plan_ok(int act, bool act_first, bool head, bool pool, bool fuse0, bool shuffle) {
    if (act != kActNone && act != kActRelu && act != kActSilu) return false;
    return !((act == kActSilu || act_first) && (head || pool || fuse0 || shuffle));
}

Status Engine::run_conv(ConvLayer& L, const TensorRef& x, const TensorRef& y, const TensorRef* res, int act,
                        hipStream_t s, const Head* head, const TensorRef* pool_out, const Fuse0* fuse0, bool act_first) {
    if (act != kActNone && act != kActRelu && act != kActSilu) return fail(1, L.name + ": unknown epilogue activation " + std::to_string(act));
    // SiLU and the activation-first order exist in the generic implicit-GEMM family only (plain, position-major, split-K; not the pair): the
    // planner below never picks the halo kernel for them, and what is written for post-ReLU values is refused outright
    const bool generic_only = act == kActSilu || act_first;
    if (!epilogue_plan_ok(act, act_first, head != nullptr, pool_out != nullptr, fuse0 != nullptr, L.shuffle))
        return fail(1, L.name + ": the fused head, the fused pool, the fused first layer and the pixel shuffle take ReLU-after-residual epilogues only");
    if (x.C != L.cinPad) return fail(1, L.name + ": input slice has " + std::to_string(x.C) + " channels, layer packs " + std::to_string(L.cinPad));
    // a layer normally runs in the engine's arithmetic; the f16r engine runs the ResNet shortcut convolutions in f32 on the
    // trunk's f32 twins (L.dt == kF32, x / y = Activation::ref32)
    const int dt = L.dt;
    if ((x.f32_only != 0) != (dt == kF32 && this->dt != kF32) || x.f32_only != y.f32_only)
        return fail(1, L.name + ": layer precision and tensor storage disagree");
    const int esz = dtype_size(dt);
    if (dt == kSplit && (x.Coff % 8 || y.Coff % 8 || (res && res->Coff % 8)))
        return fail(1, L.name + ": split-f16 slices must start on an 8-channel group");
    if ((x.Cs * esz) % 16 || (x.Coff * esz) % 16 || (y.Cs * esz) % 16 || (y.Coff * esz) % 16)
        return fail(1, L.name + ": channel strides/offsets must keep 16-byte alignment");
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    const int pad = (L.k - 1) / 2;
    int Ho, Wo;
    if (L.shuffle) { Ho = x.H; Wo = x.W; if (y.H != 2 * x.H || y.W != 2 * x.W) return fail(1, L.name + ": output must be 2x the input"); }
    else {
        Ho = (x.H + 2 * pad - L.k) / L.stride + 1; Wo = (x.W + 2 * pad - L.k) / L.stride + 1;
        if (y.H != Ho || y.W != Wo) return fail(1, L.name + ": output extent mismatch");
    }
    if (y.C != L.cout || y.N != x.N) return fail(1, L.name + ": output slice mismatch");
    const int* koff = nullptr;
    const int* kbase = nullptr;
    CV_TRY(L.get_koff(x, &koff, &kbase));
    p.x = reinterpret_cast<const char*>(x.base);
    p.w = reinterpret_cast<const char*>(L.w.ptr);
    p.koff = koff;
    p.kbase = knobs().sep ? kbase : nullptr;
    // tensor exponents (Activation): the fused head writes f32 logits, i.e. an output at exponent 0
    const int out_exp = head ? 0 : y.exp;
    if (x.exp_delta != 0 || L.in_delta != 0) CV_TRY(L.set_input_split(x.split, x.exp_delta, s));
    if (bias_measuring) CV_TRY(measure_tap_sums(L, x, Ho, Wo, s));
    CV_TRY(L.set_exps(x.exp, out_exp, s));
    p.scale = reinterpret_cast<const float*>(L.scale.ptr);
    p.shift = reinterpret_cast<const float*>(L.shift.ptr);
    p.res = nullptr;
    p.res_mul = 1.f;
    if (res) {
        if (res->H != y.H || res->W != y.W || res->C != y.C) return fail(1, L.name + ": residual shape mismatch");
        p.res = reinterpret_cast<const char*>(res->base); p.rCs = res->Cs; p.rCoff = res->Coff;
        p.res_mul = std::ldexp(1.f, res->exp - out_exp);
        if (trunk32 && dt == kF16 && res->base32) { p.res = reinterpret_cast<const char*>(res->base32); p.res_f32 = 1; }
        else if (!res->base) return fail(1, L.name + ": residual tensor has no storage in this precision");
    }
    if (trunk32 && dt == kF16 && y.base32 && !head) p.y32 = reinterpret_cast<char*>(y.base32);
    p.flag = guard_ptr();
    p.layer_id = L.layer_id;
    p.y = reinterpret_cast<char*>(y.base);
    p.M = x.N * Ho * Wo; p.Ho = Ho; p.Wo = Wo;
    p.xHp = x.H + 2; p.xWp = x.W + 2; p.stride = L.stride; p.xCs = x.Cs; p.xCoffBytes = x.Coff * esz;
    p.yHp = y.H + 2; p.yWp = y.W + 2; p.yCs = y.Cs; p.yCoff = y.Coff;
    p.Cout = L.cout; p.rows = L.rows; p.nStages = L.nStages; p.nCt = L.nCt; p.relu = act; p.shuffle = L.shuffle ? 1 : 0;
    p.act_first = act_first ? 1 : 0;
    p.act_in = p.act_out = 1.f;
    if (act == kActSilu) { p.act_in = std::ldexp(1.f, out_exp); p.act_out = std::ldexp(1.f, -out_exp); }
    if (head) {
        if (L.rows != 64 || L.shuffle) return fail(1, L.name + ": the fused 1x1 head needs a 64-channel layer");
        p.head_w = head->w; p.head_b = head->b; p.head_logits = head->logits; p.head_mask = head->mask; p.head_thr = head->thr;
    }
    int ct = L.ct;
    if (ct == 256 && blocks_for(L.rows, p.M, 256, 256) < 192) {     // under ~3/4 of a wave of 256x256 workgroups
        ct = 128;
        p.w = reinterpret_cast<const char*>(L.w_small.ptr);
    }
    int cfg = choose_cfg(ct, L.rows, p.M, L.nStages);
    int ns = choose_ns(cfg, dt, L.rows, p.M, L.nStages);
    p.nCt = (L.rows + conv_cfg_ct(cfg) - 1) / conv_cfg_ct(cfg);
    // 3x3 / stride-1 layers whose patch grid divides the image keep the input patch in LDS across the nine taps
    const bool halo_capable = L.k == 3 && L.stride == 1 && !L.shuffle && kbase != nullptr && L.nStages % 9 == 0 &&
                              knobs().halo && ct == 64 && conv_halo_supported(Ho, Wo) && !generic_only;
    // few patches: the generic kernel's smaller tiles give more workgroups (with the 8 x 16 patch variant the halo kernel doubles its own)
    bool halo = halo_capable && blocks_for(L.rows, p.M, ct, 256) >= ((knobs().halo_th8 && Ho != 8) ? 64 : 128);
    // Split-K: a launch with fewer output tiles than CUs leaves most of the chip idle while every workgroup walks a long K loop
    // alone (UNet B=1 down4: 16 tiles x 288 stages; ResNet-18 layer4 at 64 squares: 8 tiles x 144 stages).  Such launches deal their
    // K loop to several workgroups per tile -- the halo kernel by input-channel blocks (3x3 layers on maps of 16 x 16 and up: the
    // patch stays resident, only weights stream), the generic kernel by 128-byte K stages (everything else) -- and a second pass sums
    // the f32 partials in split order and runs the epilogue.
    int split_kind = 0;                                               // 0 none | 1 generic kernel | 2 halo kernel
    if (knobs().splitk && !head && !fuse0 && !calibrating) {
        const int64_t tiles_igemm = blocks_for(L.rows, p.M, conv_cfg_ct(cfg), conv_cfg_pt(cfg));
        const int64_t tiles_halo = blocks_for(L.rows, p.M, ct, 256);
        const int64_t tiles_now = halo ? tiles_halo : tiles_igemm;
        const bool halo_split_ok = halo_capable && Ho != 8 && knobs().splitk_halo;   // not the packed-image mode
        const int nCb = L.nStages / 9;
        const double bytes_igemm = 2.0 * (double)p.M * (double)p.nCt * conv_cfg_ct(cfg) * sizeof(float);   // one split's partials, written + read
        const double bytes_halo = 2.0 * (double)p.M * (double)((L.rows + ct - 1) / ct * ct) * sizeof(float);
        int want = 1;
        if (knobs().splitk_force > 1) {
            split_kind = halo_split_ok ? 2 : 1;
            want = std::min(knobs().splitk_force, split_kind == 2 ? nCb : L.nStages);
        } else if (tiles_now < knobs().splitk_max_tiles) {
            // Cost model in microseconds, fitted to single-board launches on MI355X (profiles/r04_tuning.md): a launch costs ~7 us
            // before its first stage and after its last; a workgroup alone on its CU walks a 128-byte K stage in ~0.45 us (generic
            // 64x128 / 128x128 tiles; the halo tile does twice the MFMAs per stage in ~0.5 us); a second pass costs another launch plus
            // the partials through L2 / Infinity Cache at ~3 TB/s.
            const double t_launch = 7.0, t_stage = conv_cfg_ct(cfg) >= 128 ? 0.6 : 0.45, t_stage_halo = knobs().splitk_halo_stage_ns * 1e-3, bw = 3.0e6;
            const double t_unsplit = t_launch + (halo ? 0.5 : t_stage) * L.nStages;
            double best = t_unsplit * 0.8;                            // a split must win clearly: it also costs the fused pool
            for (int k = 2; k <= std::min(L.nStages, 64); ++k) {
                const int kper = (L.nStages + k - 1) / k, ks = (L.nStages + kper - 1) / kper;
                if (ks != k) continue;
                const double waves = std::max(1.0, (double)(tiles_igemm * ks) / (double)knobs().splitk_target);
                const double t = 2.0 * t_launch + t_stage * kper * waves + ks * bytes_igemm / bw;
                if (t < best) { best = t; want = ks; split_kind = 1; }
            }
            if (halo_split_ok)
                for (int k = 2; k <= std::min(nCb, 64); ++k) {
                    const int kper = (nCb + k - 1) / k, ks = (nCb + kper - 1) / kper;
                    if (ks != k) continue;
                    // the 8 x 16 patch doubles the workgroups (and halves a stage) while the chip is not full
                    const bool th8 = knobs().halo_th8 && tiles_halo * ks < knobs().halo_th8_max_tiles;
                    const double wgs = (double)tiles_halo * ks * (th8 ? 2 : 1);
                    const double waves = std::max(1.0, wgs / (double)knobs().splitk_target);
                    const double t = 2.0 * t_launch + t_stage_halo * (th8 ? 0.6 : 1.0) * 9.0 * kper * waves + ks * bytes_halo / bw;
                    if (t < best) { best = t; want = ks; split_kind = 2; }
                }
        }
        const double sb = split_kind == 2 ? bytes_halo : bytes_igemm;
        while (want > 1 && (double)want * sb / 2.0 > (double)((size_t)256 << 20)) --want;
        if (want > 1) {
            const int units = split_kind == 2 ? nCb : L.nStages;      // what is dealt out: channel blocks (halo) / K stages (generic)
            const int kper = (units + want - 1) / want;
            p.ksplit = (units + kper - 1) / kper;                     // every split non-empty
            p.kper = kper;
            p.prow = split_kind == 2 ? (L.rows + ct - 1) / ct * ct : p.nCt * conv_cfg_ct(cfg);
            const size_t need = (size_t)p.ksplit * (size_t)p.M * (size_t)p.prow * sizeof(float);
            DeviceBuffer& ws = splitk_ws[ws_slot & 1];
            if (ws.bytes < need) {
                if (capture_flag()) return fail(1, "split-K buffer growth during graph capture");   // run_graphed falls back to an eager run
                graph_invalidate();
                CV_HIP(hipStreamSynchronize(s));                      // earlier launches may still read the old buffer
                CV_TRY(ws.alloc(std::max(need, (size_t)32 << 20), false));
            }
            p.partial = reinterpret_cast<float*>(ws.ptr);
            if (p.ksplit > 1) halo = split_kind == 2;
            else { p.ksplit = 0; p.partial = nullptr; split_kind = 0; }
        } else split_kind = 0;
    }
    if (halo && split_kind == 2) p.nCt = (L.rows + ct - 1) / ct;      // the halo kernel's channel tiles
    // Position-major rows (round 6): the generic kernel's 3x3 launches on small maps -- ResNet-18 layer3 / layer4 and the stride-2 conv1
    // of layer2-4 -- multiply the zero border at every border position: 5 of 9 taps everywhere on a 2x2 map, 31 % of the stages on 4x4.
    // With at least a pixel tile of images per position the rows are ordered [position][image] and each tile walks its live taps only.
    bool pos_major = false;
    if (knobs().pos && !halo && L.k == 3 && !L.shuffle && p.kbase && p.ksplit <= 1 && !head && !fuse0 && conv_cfg_has_pos(cfg) &&
        x.N >= conv_cfg_pt(cfg) * knobs().pos_min_tiles && std::min(Ho, Wo) <= knobs().pos_max_hw && L.nStages % 9 == 0) {
        const int* ptab = nullptr;
        const int* pcount = nullptr;
        const int* porder = nullptr;
        double live = 1.0;
        CV_TRY(L.get_pos(x, Ho, Wo, &ptab, &pcount, &porder, &live));
        // Unequal positions need more tiles than CUs for the longest-first walk to have anything to balance: a 256-row launch of
        // under two rounds (4096 squares: layer3 = 16 positions x 16 image tiles = 256 workgroups, the 9-tap ones ARE the launch)
        // takes the 128-row packing instead -- twice the tiles, each half as long (f16x3 layer3 at 4096 squares: 0.172 / 0.161 /
        // 0.168 -> 0.153 / 0.140 / 0.147 ms; with equal positions or enough rounds the 256-row tile stays: fewest L2 -> LDS bytes per MFMA)
        if (ct == 256 && L.w_small.ptr && live < 0.75 && blocks_for(L.rows, (int64_t)x.N, 256, 256) * Ho * Wo < 512 /* two rounds on 256 CUs */ &&
            knobs().pos_small_ct) {
            const int cfg2 = choose_cfg(128, L.rows, p.M, L.nStages);
            if (conv_cfg_has_pos(cfg2) && x.N >= conv_cfg_pt(cfg2)) {
                ct = 128;
                p.w = reinterpret_cast<const char*>(L.w_small.ptr);
                cfg = cfg2;
                ns = choose_ns(cfg, dt, L.rows, p.M, L.nStages);
                p.nCt = (L.rows + conv_cfg_ct(cfg) - 1) / conv_cfg_ct(cfg);
            }
        }
        p.ptab = ptab; p.pcount = pcount; p.porder = porder; p.posN = x.N; p.nPtPer = (x.N + conv_cfg_pt(cfg) - 1) / conv_cfg_pt(cfg);
        pos_major = true;
    }
    if (fuse0) {
        if (!halo || !conv_halo_can_fuse_first_layer(dt)) { Status ns; ns.code = kNotFused; return ns; }   // caller runs the layers apart
        p.f0_x = fuse0->x; p.f0_u8 = fuse0->u8 ? 1 : 0; p.f0_w = fuse0->w; p.f0_scale = fuse0->scale; p.f0_shift = fuse0->shift;
        p.f0_in_mul = fuse0->in_mul;
    }
    // the pooled copy comes from the halo kernel's epilogue, or from the second pass of a split launch (either kernel)
    const bool fuse_pool = pool_out && !head && knobs().fuse_pool && (p.ksplit > 1 ? (Ho % 2 == 0 && Wo % 2 == 0 && !L.shuffle) : halo);
    if (pool_out) {
        if (pool_out->H * 2 != y.H || pool_out->W * 2 != y.W || pool_out->C != y.C || pool_out->N != y.N)
            return fail(1, L.name + ": pooled output shape mismatch");
        if (fuse_pool) {
            p.pool_y = reinterpret_cast<char*>(pool_out->base);
            p.pHp = pool_out->H + 2; p.pWp = pool_out->W + 2; p.pCs = pool_out->Cs; p.pCoff = pool_out->Coff;
        }
    }
    // diagnostic (library built with -DCV_STAMP=1, CV_STAMP_LAYER=<layer name>|all): in-kernel cycle stamps of the K loop
    static const char* const stamp_layer = std::getenv("CV_STAMP_LAYER");
    unsigned long long* stamp_dev = nullptr;
    size_t stamp_n = 0;
    if (halo && stamp_layer && (L.name == stamp_layer || std::string(stamp_layer) == "all")) {
        stamp_n = ((size_t)p.M / 128 + 1) * (size_t)p.nCt * 8 * 8;
        if (hipMalloc(&stamp_dev, stamp_n * 8) == hipSuccess) { (void)hipMemsetAsync(stamp_dev, 0, stamp_n * 8, s); p.stamp = stamp_dev; }
    }
    if (profiling) {
        // compulsory bytes: the input slice once (a strided 1x1 touches every other pixel only), output (+ pooled copy,
        // + residual) once, weights once -- at the engine's storage width; the fused head writes one f32 (+ mask byte)
        const double in_px = (L.k == 1 && L.stride == 2) ? (double)p.M : (double)x.N * x.H * x.W;
        const double out_px = L.shuffle ? 4.0 * p.M : (double)p.M;
        double b = (fuse0 ? in_px * (fuse0->u8 ? 3.0 : 12.0) : in_px * L.cinPad * esz) + (double)L.rows * L.k * L.k * L.cin * esz;
        b += head ? (double)p.M * (4 + (head->mask ? 1 : 0)) : out_px * L.cout * esz;
        if (res) b += out_px * L.cout * (p.res_f32 ? 4 : esz);
        if (p.y32) b += out_px * L.cout * 4;                 // f16r: the trunk's f32 twin
        if (pool_out) b += out_px / 4 * L.cout * esz;
        prof_begin(fuse0 ? "inc.double_conv.0+3 (fused)" : L.name, true,
                   ((double)L.macs_per_out_pixel() + (fuse0 ? fuse0->macs_per_pixel : 0.0)) * (double)p.M, s, b);
        const char* tn = dt == kF32 ? "float" : dt == kF16 ? "half_t" : "split_t";
        if (halo)
            prof.back().kernel = std::string("conv3x3_halo_kernel<") + tn + "," + std::to_string(ct) + (halo_th8_for(L, p, ct, Ho, fuse0 != nullptr) ? ",8x16" : ",16x16") +
                                 (Ho == 8 ? ",IMG8" : "") + (fuse0 ? ",FUSE0" : "") + (p.ksplit > 1 ? ",splitK" + std::to_string(p.ksplit) : std::string()) + ">";   // template parameters only: a fused pool / 1x1 head is
                                                                                              // a run-time option of the same instantiation
        else
            prof.back().kernel = std::string("conv_igemm_kernel<") + tn + "," + std::to_string(conv_cfg_ct(cfg)) + "x" +
                                 std::to_string(conv_cfg_pt(cfg)) + ",ring" + std::to_string(ns) + (L.shuffle ? ",shuffle" : "") +
                                 (p.ksplit > 1 ? ",splitK" + std::to_string(p.ksplit) : std::string()) + (pos_major ? ",POS" : "") + ">";
    }
    if (defer && knobs().pair && !generic_only && !halo && !pos_major && !profiling && !calibrating && !stamp_dev && !head && !fuse0 && p.kbase && !(pool_out && !fuse_pool) &&
        !(defer_first && p.ksplit > 1) &&
        blocks_for(L.rows, p.M, conv_cfg_ct(cfg), conv_cfg_pt(cfg)) * (p.ksplit > 1 ? p.ksplit : 1) <= knobs().pair_max_blocks) {
        defer->held = true; defer->cfg = cfg; defer->ns = ns; defer->dt = dt; defer->p = p; defer->name = L.name;
        defer->blocks = blocks_for(L.rows, p.M, conv_cfg_ct(cfg), conv_cfg_pt(cfg)) * (p.ksplit > 1 ? p.ksplit : 1);
        return Status();                                              // issued by flush_pending
    }
    // launches with fewer 16 x 16 patches than the chip holds workgroups (2 per CU) take the 8 x 16 patch: twice the workgroups
    const int th = (halo && halo_th8_for(L, p, ct, Ho, fuse0 != nullptr)) ? 8 : 16;
    hipError_t e = halo ? conv_halo_launch(dt, p, x.N, s, th) : pos_major ? conv_igemm_pos_launch(cfg, ns, dt, p, s) : conv_igemm_launch(cfg, ns, dt, p, s);
    if (e == hipSuccess && p.ksplit > 1) e = conv_splitk_reduce_launch(dt, p, s);
    if (profiling) prof_end(s);
    if (stamp_dev) {
        std::vector<unsigned long long> h(stamp_n);
        (void)hipStreamSynchronize(s);
        (void)sync_memcpy(h.data(), stamp_dev, stamp_n * 8, hipMemcpyDeviceToHost);
        (void)hipFree(stamp_dev);
        std::vector<double> cyc, clk, wfrac, hd, is, tl, ep;
        double stages = 0;
        for (size_t i = 0; i + 7 < stamp_n; i += 8) {
            if (!h[i + 3] || !h[i + 1]) continue;
            cyc.push_back((double)h[i]); clk.push_back((double)h[i] / (double)h[i + 1] * 0.1);
            wfrac.push_back((double)h[i + 2] / (double)h[i]); stages = (double)h[i + 3];
            hd.push_back((double)h[i + 4] / (double)h[i]); is.push_back((double)h[i + 5] / (double)h[i]);
            tl.push_back((double)h[i + 6] / (double)h[i]); ep.push_back((double)h[i + 7]);
        }
        if (!cyc.empty()) {
            auto med = [](std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
            auto mean = [](const std::vector<double>& v) { double t = 0; for (double x : v) t += x; return t / (double)v.size(); };
            const double c = med(cyc), k = med(clk);
            std::fprintf(stderr, "[stamp] %-40s ct=%d waves=%zu stages=%.0f loop=%.0f cyc (%.1f cyc/stage) clock=%.3f GHz wait+barrier=%.1f %% pre-loop=%.0f cyc | epilogue: rendezvous %.0f, stores issued %.0f, drained %.0f cyc\n",
                         L.name.c_str(), ct, cyc.size(), stages, c, c / stages, k, 100.0 * mean(wfrac), mean(is) * c, mean(hd) * c, mean(tl) * c, mean(ep));
        }
    }
    if (e != hipSuccess) return hip_fail(e, ("conv launch " + L.name).c_str());
    if (calibrating && !head) CV_TRY(measure(y, s));
    if (pool_out && pool_out->exp != y.exp) return fail(1, L.name + ": pooled copy must share the exponent of its source");
    if (pool_out && !fuse_pool) {
        if (profiling) prof_begin("maxpool2x2", false, 0, s);
        e = maxpool2x2(dt, y, *pool_out, s);
        if (profiling) prof_end(s);
        if (e != hipSuccess) return hip_fail(e, "maxpool2x2");
    }
    return Status();
}

Status Engine::flush_pending(PendingConv& a, PendingConv& b, hipStream_t s) {
    hipError_t e = hipSuccess;
    const bool dt_ok = a.dt == b.dt || (a.dt == kF32 && b.dt == kF16);     // the fp16 classifier's shortcuts run in f32
    if (a.held && b.held && a.cfg == b.cfg && a.ns == b.ns && dt_ok && !(a.p.ksplit > 1 && b.p.ksplit > 1) &&
        a.blocks + b.blocks <= knobs().pair_max_blocks) {
        e = conv_igemm_pair_launch(a.cfg, a.ns, a.dt, b.dt, a.p, b.p, s);
        if (e == hipSuccess && a.p.ksplit > 1) e = conv_splitk_reduce_launch(a.dt, a.p, s);
        if (e == hipSuccess && b.p.ksplit > 1) e = conv_splitk_reduce_launch(b.dt, b.p, s);
        a.held = b.held = false;
        if (e != hipSuccess) return hip_fail(e, ("conv pair launch " + a.name + " + " + b.name).c_str());
        return Status();
    }
    for (PendingConv* q : {&a, &b}) {
        if (!q->held) continue;
        q->held = false;
        e = conv_igemm_launch(q->cfg, q->ns, q->dt, q->p, s);
        if (e == hipSuccess && q->p.ksplit > 1) e = conv_splitk_reduce_launch(q->dt, q->p, s);
        if (e != hipSuccess) return hip_fail(e, ("conv launch " + q->name).c_str());
    }
    return Status();
}

void Engine::prof_begin(const std::string& name, bool is_conv, double macs, hipStream_t s, double bytes) {
    ProfileEntry pe;
    pe.name = name; pe.is_conv = is_conv; pe.macs = macs; pe.bytes = bytes;
    (void)hipEventCreate(&pe.e0);
    (void)hipEventCreate(&pe.e1);
    (void)hipEventRecord(pe.e0, s);
    prof.push_back(pe);
}
void Engine::prof_end(hipStream_t s) {
    if (!prof.empty()) (void)hipEventRecord(prof.back().e1, s);
}
Status Engine::prof_collect() {
    for (auto& pe : prof) {
        if (!pe.e0) continue;
        CV_HIP(hipEventSynchronize(pe.e1));
        CV_HIP(hipEventElapsedTime(&pe.ms, pe.e0, pe.e1));
        (void)hipEventDestroy(pe.e0); (void)hipEventDestroy(pe.e1);
        pe.e0 = pe.e1 = nullptr;
    }
    return Status();
}
void Engine::prof_clear() {
    for (auto& pe : prof) {
        if (pe.e0) (void)hipEventDestroy(pe.e0);
        if (pe.e1) (void)hipEventDestroy(pe.e1);
    }
    prof.clear();
}

}  // namespace cv
