// cv_api.cpp -- the extern "C" surface declared in include/chessvision_hip.h.
#include "../../include/chessvision_hip.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <thread>

#include "engine.h"
#include "host_stages.h"
#include "jpeg.h"
#include "jpeg_device.h"
#include "jpeg_enc_device.h"
#include "models.h"
#include "neighbours.h"
#include "pacmap.h"
#include "pipeline.h"
#include "pointwise.h"

static_assert(sizeof(cv_score_record_t) == sizeof(cv::ScoreRecord) && offsetof(cv_score_record_t, top_sum) == offsetof(cv::ScoreRecord, top_sum) &&
              offsetof(cv_score_record_t, top_count) == offsetof(cv::ScoreRecord, top_count), "cv_score_record_t is the kernel's record");
static_assert(sizeof(cv_seg_record_t) == sizeof(cv::SegRecord) && offsetof(cv_seg_record_t, bce_sum) == offsetof(cv::SegRecord, bce_sum) &&
              offsetof(cv_seg_record_t, sig_label_sum) == offsetof(cv::SegRecord, sig_label_sum) &&
              offsetof(cv_seg_record_t, count) == offsetof(cv::SegRecord, count), "cv_seg_record_t is the kernel's record");
static_assert(sizeof(cv_square_record_t) == sizeof(cv::SquareRecord) && offsetof(cv_square_record_t, confidence) == offsetof(cv::SquareRecord, confidence) &&
              offsetof(cv_square_record_t, logsumexp) == offsetof(cv::SquareRecord, logsumexp), "cv_square_record_t is the kernel's record");
static_assert(sizeof(cv_level_record_t) == sizeof(cv::LevelRecord) && sizeof(cv_level_record_t) % 64 == 0 && CV_MAX_THRESHOLDS == cv::kMaxLevelThresholds &&
              offsetof(cv_level_record_t, hist) == offsetof(cv::LevelRecord, hist) && offsetof(cv_level_record_t, reserved) == offsetof(cv::LevelRecord, reserved),
              "cv_level_record_t is the kernel's record");
static_assert(sizeof(cv_jpeg_info_t) == sizeof(cvjpeg::Info) && offsetof(cv_jpeg_info_t, luma_h) == offsetof(cvjpeg::Info, luma_h) &&
              offsetof(cv_jpeg_info_t, orientation) == offsetof(cvjpeg::Info, orientation) && offsetof(cv_jpeg_info_t, supported) == offsetof(cvjpeg::Info, supported) &&
              offsetof(cv_jpeg_info_t, reason) == offsetof(cvjpeg::Info, reason) && (int)CV_ERR_INVALID == (int)cvjpeg::kInvalid &&
              (int)CV_JPEG_BGR == (int)cv::kJpegBGR && (int)CV_JPEG_RGB == (int)cv::kJpegRGB && (int)CV_JPEG_GRAY == (int)cv::kJpegGray,
              "cv_jpeg_info_t is the parser's record");
static_assert(sizeof(cv_neighbour_stats_t) == sizeof(cv::NeighbourStats) && sizeof(cv_neighbour_stats_t) == 32 &&
              offsetof(cv_neighbour_stats_t, nonfinite_corpus_rows) == offsetof(cv::NeighbourStats, nonfinite_corpus_rows) &&
              (int)CV_NEIGHBOURS_EXCLUDE_SELF == (int)cv::kNeighbourExcludeSelf && (int)CV_NEIGHBOURS_EXACT_ONLY == (int)cv::kNeighbourExactOnly,
              "cv_neighbour_stats_t is the kernels' record");
static_assert(sizeof(cv_pacmap_stats_t) == sizeof(cv::PacmapStats) && sizeof(cv_pacmap_stats_t) == 64 &&
              offsetof(cv_pacmap_stats_t, mid_near_draws) == offsetof(cv::PacmapStats, mid_near_draws) &&
              offsetof(cv_pacmap_stats_t, candidates) == offsetof(cv::PacmapStats, candidates),
              "cv_pacmap_stats_t is the kernels' record");
static_assert(sizeof(cv_pacmap_place_plan_t) == 40 && offsetof(cv_pacmap_place_plan_t, scale_scratch_bytes) == 24,
              "cv_pacmap_place_plan_t is the layout the Python binding mirrors");
static_assert(sizeof(cv_square_score_t) == 24 && sizeof(cv_board_score_t) == 64, "layouts the Python binding mirrors");

using namespace cv;

struct cv_engine {
    Engine impl;
};

// ---- what two or more entry points share (may throw: std::vector / std::map / std::string allocations) ----------------------
namespace {

struct DeviceGuard {                       // every entry point runs on the engine's device
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// No C++ exception may unwind through the C boundary (ctypes / cgo callers would abort): every entry point runs inside
// this wrapper.  The out-of-memory message fits the small-string buffer, so reporting it allocates nothing.
template <class F> int guarded(const char* what, F&& body) noexcept {
    try {
        const Status s = body();
        return s.code;
    } catch (const std::bad_alloc&) {
        try { set_error("out of memory"); } catch (...) {}
        return CV_ERR_NOMEM;
    } catch (const std::length_error&) {
        try { set_error("out of memory"); } catch (...) {}
        return CV_ERR_NOMEM;
    } catch (const std::exception& ex) {
        try { set_error(std::string(what) + ": " + ex.what()); } catch (...) {}
        return CV_ERR_INVALID;
    } catch (...) {
        try { set_error("unknown C++ exception"); } catch (...) {}
        return CV_ERR_INVALID;
    }
}

Status to_map(const cv_param_t* params, int n, ParamMap& pm) {
    if (n < 0 || (n > 0 && !params)) return fail(CV_ERR_INVALID, "null parameter table");
    for (int i = 0; i < n; ++i) {
        const cv_param_t& p = params[i];
        if (!p.name) return fail(CV_ERR_INVALID, "malformed cv_param_t entry " + std::to_string(i) + " (null name)");
        const size_t nl = std::strlen(p.name);
        if (nl >= 19 && std::strcmp(p.name + nl - 19, "num_batches_tracked") == 0) continue;   // a full torch state dict may carry them
                                                                                              // (int64 scalars: data / shape are not looked at)
        if (!p.data || p.ndim < 0 || p.ndim > 4) return fail(CV_ERR_INVALID, std::string("malformed cv_param_t entry '") + p.name + "'");
        ParamView v;
        v.data = p.data;
        for (int d = 0; d < p.ndim; ++d) v.shape.push_back(p.shape[d]);
        pm[p.name] = v;
    }
    return Status();
}

Status check_engine(cv_engine_t* eng) {
    if (!eng) return fail(CV_ERR_INVALID, "null engine handle");
    return Status();
}

// Model loads are serialised process-wide.  A load packs, uploads and calibrates through the legacy stream (hundreds of synchronous
// allocations, fills and copies, calibration forwards on stream 0); two of them side by side in one process -- a second instance created
// while another loads, or beside the background replica of a request slot -- ended in a GPU memory access fault in 50-80 % of the
// soak runs (tests/dev/slots_soak.py; forwards beside ONE load never did, in any number of runs).  Loads take seconds and happen once
// per engine: one at a time costs nothing.
std::mutex& load_mutex() {
    static std::mutex mu;
    return mu;
}

Status load_resnet(cv_engine_t* eng, const char* arch, const cv_param_t* params, int n_params) {
    CV_TRY(check_engine(eng));
    if (!arch || !resnet_arch(arch))
        return fail(CV_ERR_INVALID, "cv_load_resnet: arch must be 'resnet18' or 'resnet34', got " +
                                        (arch ? "'" + std::string(arch) + "'" : std::string("NULL")));
    std::lock_guard<std::mutex> load_lk(load_mutex());
    std::lock_guard<std::mutex> lk(eng->impl.mu);
    DeviceGuard g(eng->impl.device);
    ParamMap pm;
    CV_TRY(to_map(params, n_params, pm));
    return resnet_load(eng->impl, pm, arch);
}

Status load_yolo_cls(cv_engine_t* eng, const char* arch, const cv_param_t* params, int n_params) {
    CV_TRY(check_engine(eng));
    if (!arch || !yolo_cls_arch(arch))
        return fail(CV_ERR_INVALID, "cv_load_yolo_cls: arch must be 'yolov8n-cls', 'yolov8s-cls', 'yolov8m-cls', 'yolov8l-cls' or 'yolov8x-cls', got " +
                                        (arch ? "'" + std::string(arch) + "'" : std::string("NULL")));
    std::lock_guard<std::mutex> load_lk(load_mutex());
    std::lock_guard<std::mutex> lk(eng->impl.mu);
    DeviceGuard g(eng->impl.device);
    ParamMap pm;
    CV_TRY(to_map(params, n_params, pm));
    return yolo_cls_load(eng->impl, pm, arch);
}

// by-name entry points: "unet" | the loaded classifier's architecture name (a ResNet or a YOLOv8-cls).  Sets *is_resnet -- "the
// classifier slot" -- ; a known name of a model that is not the loaded one fails with CV_ERR_STATE naming what is loaded, an unknown
// name with CV_ERR_INVALID.
Status model_by_name(const Engine& e, const char* model, bool* is_resnet) {
    *is_resnet = false;
    if (std::strcmp(model, "unet") == 0) return Status();
    if (!resnet_arch(model) && !yolo_cls_arch(model)) return fail(CV_ERR_INVALID, "model must be 'unet', 'resnet18', 'resnet34' or 'yolov8{n,s,m,l,x}-cls'");
    *is_resnet = true;
    const char* held = classifier_name(e);
    if (held && std::strcmp(held, model) != 0)
        return fail(CV_ERR_STATE, "model '" + std::string(model) + "' is not loaded: this engine holds " + held);
    return Status();
}

// the tensor `name` of the model `model`, as it stands after the model's last forward (caller holds the engine mutex)
Status activation_by_name(Engine& e, const char* model, const char* name, TensorRef* t) {
    bool is_resnet = false;
    CV_TRY(model_by_name(e, model, &is_resnet));
    return is_resnet ? classifier_activation(e, name, t) : unet_activation(e, name, t);
}

Status check_embedding(const float* embedding) {
    if ((uintptr_t)embedding & 15u) return fail(CV_ERR_INVALID, "embedding must be 16-byte aligned");
    return Status();
}

// the five cv_unet_forward* entry points; those without a mask, a threshold or an embedding pass null, 0.5 and null
Status unet_entry(cv_engine_t* eng, const void* x, bool x_u8, int batch, float* logits, uint8_t* mask, float threshold, float* embedding,
                  void* stream) {
    CV_TRY(check_engine(eng));
    if (!(threshold >= 0.f && threshold <= 1.f)) return fail(CV_ERR_INVALID, "threshold must be between 0 and 1");
    CV_TRY(check_embedding(embedding));
    std::lock_guard<std::mutex> lk(eng->impl.mu);
    DeviceGuard g(eng->impl.device);
    return unet_forward(eng->impl, x, x_u8, batch, logits, mask, threshold, (hipStream_t)stream, embedding);
}

// the four cv_resnet18_forward* entry points (the u8 entries return probabilities, the float entries logits) and
// cv_resnet_forward_u8_norm, which says which it wants and has its bytes normalised in the stem
Status resnet_entry(cv_engine_t* eng, const void* x, bool x_u8, int n, float* out, float* embedding, void* stream, bool softmax,
                    const InputNorm* norm = nullptr) {
    CV_TRY(check_engine(eng));
    CV_TRY(check_embedding(embedding));
    if (norm && !(std::isfinite(norm->mean) && std::isfinite(norm->std) && norm->std > 0.f))
        return fail(CV_ERR_INVALID, "cv_resnet_forward_u8_norm: mean must be finite, std finite and > 0");
    std::lock_guard<std::mutex> lk(eng->impl.mu);
    DeviceGuard g(eng->impl.device);
    return classifier_forward(eng->impl, x, x_u8, n, out, softmax, (hipStream_t)stream, embedding, norm);
}

// ---- single-layer entry points (parity tests) -------------------------------------------------------
int round_up(int v, int m) { return (v + m - 1) / m * m; }

typedef hipError_t (*pool_fn)(int, const TensorRef&, const TensorRef&, hipStream_t);
hipError_t upsample_plain(int dt, const TensorRef& a, const TensorRef& b, hipStream_t s) {
    return upsample_bilinear2x(dt, a, b, nullptr, 0u, s);
}
Status pool_like(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, int ho, int wo, float* y, void* stream, pool_fn fn,
                 const char* what) {
    CV_TRY(check_engine(eng));
    if (!x || !y || n <= 0 || c <= 0 || h <= 0 || w_ <= 0 || ho <= 0 || wo <= 0) return fail(CV_ERR_INVALID, std::string(what) + ": bad argument");
    std::lock_guard<std::mutex> lk(eng->impl.mu);
    DeviceGuard g(eng->impl.device);
    Engine& e = eng->impl;
    hipStream_t st = (hipStream_t)stream;
    const int cp = round_up(c, 8);
    Activation ax, ay;
    Status s;
    if ((s = ax.create(n, h, w_, cp, e.dt)).ok() && (s = ay.create(n, ho, wo, cp, e.dt)).ok()) {
        hipError_t err = pack_nchw_f32(e.dt, x, c, ax.ref(n), e.guard_ptr(), st);
        if (err == hipSuccess) err = fn(e.dt, ax.ref(n), ay.ref(n), st);
        if (err == hipSuccess) err = unpack_nchw_f32(e.dt, ay.ref(n, 0, c), y, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) s = hip_fail(err, what);
    }
    return s;
}

// ---- classical stages either side of the CNNs -----------------------------------------
// Host threads for `n` masks.  A mask takes ~50 us since round 4 (run-based labelling): starting a thread costs about as much, so every
// thread gets at least eight masks (64 masks: 8 threads; a single board: none), and there are never more than 32.
int mask_threads(int n, int n_threads) {
    const int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(nt, std::min((n + 7) / 8, 32)));
}

// contiguous slices of [0, n) on up to `nt` host threads (every item costs about the same)
template <class F> void parallel_slices(int n, int nt, F&& work) {
    if (nt <= 1) { work(0, n); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) pool.emplace_back([&work, n, nt, t] { work((int)((long long)n * t / nt), (int)((long long)n * (t + 1) / nt)); });
    for (auto& th : pool) th.join();
}

Status mask_completenesses(const uint8_t* masks, int n, int h, int w, double* scores, int n_threads) {
    if (!masks || !scores || n < 0 || h <= 0 || w <= 0) return fail(CV_ERR_INVALID, "cv_mask_completenesses: bad argument");
    parallel_slices(n, mask_threads(n, n_threads), [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) scores[i] = mask_completeness(masks + (size_t)i * h * w, h, w);
    });
    return Status();
}

// Pytorch-UNet's dice_coeff for one image: (2 * inter + eps) / (sets_sum + eps), sets_sum == 0 -> 2 * inter
double dice_of(double inter, double sets_sum) {
    if (sets_sum == 0.0) sets_sum = 2.0 * inter;
    return (2.0 * inter + 1e-6) / (sets_sum + 1e-6);
}

// Dice, IoU and pixel accuracy of a thresholded mask against a label mask, from their integer counts (the formulas documented at
// cv_segmentation_scores_finish; cv_threshold_levels_finish applies them per threshold).  Any output may be null.
void hard_mask_scores(long long n_label, long long n_pred, long long n_both, long long count, double* dice, double* iou, double* pixel_accuracy) {
    const long long uni = n_pred + n_label - n_both;
    if (dice) *dice = dice_of((double)n_both, (double)n_pred + (double)n_label);
    if (iou) *iou = uni == 0 ? 1.0 : (double)n_both / (double)uni;
    if (pixel_accuracy) *pixel_accuracy = (double)(count - n_pred - n_label + 2LL * n_both) / (double)count;
}

// INTER_AREA on `st` with the engine's cached tables for fractional shrinks (caller holds the engine mutex)
Status resize_on_stream(Engine& en, const uint8_t* src, int n, int h, int w_, int channels, uint8_t* dst, int out_h, int out_w, hipStream_t st) {
    hipError_t e;
    const bool integer = h % out_h == 0 && w_ % out_w == 0;
    if (!integer && out_h <= h && out_w <= w_) {
        // fractional shrink: OpenCV's float32 table form; the two tables are built once per geometry and stay on the device
        ResizeTables& tabs = en.area_tabs;
        const int geom[4] = {h, w_, out_h, out_w};
        if (std::memcmp(tabs.geom, geom, sizeof geom) != 0) {
            std::vector<int> xo, xs, yo, ys;
            std::vector<float> xa, ya;
            resize_area_table(w_, out_w, xo, xs, xa);
            resize_area_table(h, out_h, yo, ys, ya);
            CV_TRY(tabs.replace(geom, st, xo, xs, xa, yo, ys, ya));
        }
        const char* base = (const char*)tabs.buf.ptr;
        e = resize_area_u8_tab(src, n, h, w_, channels, dst, out_h, out_w, (const int*)(base + tabs.off[0]), (const int*)(base + tabs.off[1]),
                               (const float*)(base + tabs.off[2]), (const int*)(base + tabs.off[3]), (const int*)(base + tabs.off[4]),
                               (const float*)(base + tabs.off[5]), st);
    } else {
        e = resize_area_u8(src, n, h, w_, channels, dst, out_h, out_w, st);
    }
    if (e != hipSuccess) return hip_fail(e, "resize_area_u8");
    return Status();
}

// antialiased bilinear resize to float32 NCHW with the engine's cached tap tables (caller holds the engine mutex)
Status resize_antialias_on_stream(Engine& en, const uint8_t* src, int n, int h, int w_, int channels, float* dst, int out_h, int out_w,
                                  hipStream_t st) {
    ResizeTables& tabs = en.aa_tabs;
    const int geom[4] = {h, w_, out_h, out_w};
    if (std::memcmp(tabs.geom, geom, sizeof geom) != 0) {
        std::vector<int> xf, xc, yf, yc;
        std::vector<float> xw, yw;
        int xs = 0, ys = 0;
        resize_antialias_table(w_, out_w, xf, xc, xw, &xs);
        resize_antialias_table(h, out_h, yf, yc, yw, &ys);
        CV_TRY(tabs.replace(geom, st, xf, xc, xw, yf, yc, yw, xs, ys));
    }
    const char* base = (const char*)tabs.buf.ptr;
    const hipError_t e = resize_antialias_f32(src, n, h, w_, channels, dst, out_h, out_w, (const int*)(base + tabs.off[0]),
                                              (const int*)(base + tabs.off[1]), (const float*)(base + tabs.off[2]), tabs.stride[0],
                                              (const int*)(base + tabs.off[3]), (const int*)(base + tabs.off[4]),
                                              (const float*)(base + tabs.off[5]), tabs.stride[1], st);
    if (e != hipSuccess) return hip_fail(e, "resize_antialias_f32");
    return Status();
}

// range calibration as data: the per-tensor exponents of a model, in the fixed order of its activation list (two per tensor: the
// tensor's exponent and the second half's exponent of a concatenated buffer)
Status engine_calibration(cv_engine_t* eng, const char* model, int32_t* exps, int capacity, int* count, int import) {
    CV_TRY(check_engine(eng));
    if (!model || !count) return fail(CV_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(eng->impl.mu);
    DeviceGuard g(eng->impl.device);
    Engine& e = eng->impl;
    std::vector<Activation*>* acts = nullptr;
    bool is_resnet = false;
    const Status s = model_by_name(e, model, &is_resnet);
    if (!s.ok()) return s.code == CV_ERR_INVALID ? fail(CV_ERR_STATE, "model must be a loaded 'unet', 'resnet18', 'resnet34' or 'yolov8{n,s,m,l,x}-cls'") : s;
    if (!is_resnet && e.unet) acts = &e.unet->acts;
    else if (is_resnet && classifier_model(e)) acts = &classifier_model(e)->acts;
    else return fail(CV_ERR_STATE, "model must be a loaded 'unet', 'resnet18', 'resnet34' or 'yolov8{n,s,m,l,x}-cls'");
    const int n = 2 * (int)acts->size();
    if (!import) {
        *count = n;
        if (!exps) return Status();                               // size query
        if (capacity < n) return fail(CV_ERR_INVALID, "calibration buffer too small");
        for (size_t i = 0; i < acts->size(); ++i) { exps[2 * i] = (*acts)[i]->exp; exps[2 * i + 1] = (*acts)[i]->exp2; }
        return Status();
    }
    if (!exps || capacity != n) return fail(CV_ERR_INVALID, "calibration vector does not match this model (" + std::to_string(n) + " entries expected)");
    if (e.dt == kF32) return Status();                            // the f32 engine stores real values: nothing to set
    // validate the WHOLE vector before the first write: a rejected import leaves the engine exactly as it was
    for (int i = 0; i < n; ++i)
        if (exps[i] < -60 || exps[i] > 60) return fail(CV_ERR_INVALID, "exponent out of range (entry " + std::to_string(i) + ")");
    bool changed = false;
    for (size_t i = 0; i < acts->size(); ++i) {
        Activation* a = (*acts)[i];
        if (a->fixed_exp) continue;
        if (a->exp != exps[2 * i] || (a->split_c && a->exp2 != exps[2 * i + 1])) changed = true;
        a->exp = exps[2 * i];
        if (a->split_c) a->exp2 = exps[2 * i + 1];
    }
    if (changed) {                                                // the layers re-fold their epilogue constants at their next launch
        hipError_t he = device_synchronize();
        if (he != hipSuccess) return hip_fail(he, "cv_engine_import_calibration");
        e.graph_invalidate();
        e.graph_clear();
    }
    *count = changed ? 1 : 0;
    return Status();
}

// ---- one image, host to host ---------------------------------------------------------------------------------------------
// A copy in flight on a side stream must not outlive the call that issued it.  Armed when the copy is issued, this waits for the side
// stream on the host at whatever exit the call takes; disarmed once the caller's stream has joined the side stream on the device and
// has itself been synchronised, so that the success path pays no second host synchronisation.
struct SideStreamJoin {
    hipStream_t side = nullptr;
    void arm(hipStream_t s) { side = s; }
    void disarm() { side = nullptr; }
    ~SideStreamJoin() { if (side) (void)hipStreamSynchronize(side); }
};

// the geometry a device launch may rely on: what parse_info accepts, restated on the caller's copy of the record
Status check_jpeg_info(const cvjpeg::Info& info) {
    if (!info.supported) return fail(CV_ERR_INVALID, std::string("unsupported JPEG stream: ") + std::string(info.reason, strnlen(info.reason, sizeof info.reason)));
    const bool luma_ok = (info.luma_h == 1 && info.luma_v == 1) || (info.luma_h == 2 && info.luma_v == 1) || (info.luma_h == 2 && info.luma_v == 2);
    if (info.width < 1 || info.height < 1 || info.width > 65535 || info.height > 65535 || (size_t)info.width * info.height > ((size_t)1 << 28) ||
        (info.components != 1 && info.components != 3) || !luma_ok || (info.components == 1 && info.luma_h != 1))
        return fail(CV_ERR_INVALID, "malformed cv_jpeg_info_t");
    return Status();
}

// The two fronts of the one-image pipeline: the caller's pixels (cv_process_image, cv_process_image_v2) or a JPEG stream
// (cv_process_jpeg, cv_process_jpeg_oriented), which the entropy stage decodes into the page-locked block and the device reconstructs
// into the image's place.
struct ImageFront {
    const uint8_t* image = nullptr;        // (h, w, 3) uint8, or
    const uint8_t* jpeg = nullptr;         // an encoded stream of jpeg_len bytes whose header is `info`
    size_t jpeg_len = 0;
    cvjpeg::Info info;
    int orientation = 0;                   // the EXIF tag the reconstruction applies (0, 1: none); h and w are then the ORIENTED photo's
};

Status process_image(cv_engine_t* ue, cv_engine_t* ce, const ImageFront& front, int h, int w_, float threshold, int flip, int fallback_quad,
                     cv_image_result_t* out, size_t out_size, void* stream) {
    const uint8_t* const image = front.image;
    // the caller's struct may be the shorter one of an earlier ABI: nothing at or beyond out_size is touched
    if (out && out_size < offsetof(cv_image_result_t, n_fixes) + sizeof(int32_t))
        return fail(CV_ERR_INVALID, "cv_process_image: result struct smaller than the ABI 3 layout");
    uint8_t* const out_squares = (out && out_size >= offsetof(cv_image_result_t, squares) + sizeof(uint8_t*)) ? out->squares : nullptr;
    CV_TRY(check_engine(ue));
    CV_TRY(check_engine(ce));
    if ((!image && !front.jpeg) || !out || h <= 0 || w_ <= 0 || (size_t)h * w_ > ((size_t)1 << 28)) return fail(CV_ERR_INVALID, "cv_process_image: bad argument");
    if (!(threshold >= 0.f && threshold <= 1.f)) return fail(CV_ERR_INVALID, "threshold must be between 0 and 1");
    if (ue->impl.device != ce->impl.device) return fail(CV_ERR_STATE, "cv_process_image: both engines must live on one device");
    Engine& U = ue->impl;
    Engine& C = ce->impl;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard g(U.device);
    out->found = 0;
    out->n_fixes = 0;
    const size_t img_b = (size_t)h * w_ * 3, small_b = 256 * 256 * 3, lg_b = 65536 * sizeof(float), mk_b = 65536, sq_b = 64 * 4096,
                 bd_b = 512 * 512, pr_b = 64 * 13 * sizeof(float), inv_b = 9 * sizeof(double), gd_b = 2 * sizeof(unsigned);
    // both staging blocks are carved into pieces that start on 256-byte boundaries; returns the size of the block
    auto carve = [](std::initializer_list<size_t> sizes, size_t* off) {
        size_t at = 0;
        for (size_t b : sizes) { *off++ = at; at += (b + 255) & ~(size_t)255; }
        return at;
    };
    // the JPEG front's pieces: coefficients and tables on both sides, component planes on the device; empty for the pixel front, whose
    // blocks and offsets are what they always were
    const size_t jpeg_blocks = front.jpeg ? cvjpeg::layout_of(front.info).blocks : 0;
    const size_t co_b = jpeg_blocks * 64 * sizeof(int16_t), qt_b = front.jpeg ? 3 * 64 * sizeof(uint16_t) : 0, pl_b = jpeg_blocks * 64;
    size_t h_off[9], d_off[9];
    // host block: image | mask | logits | board | probs | inv | two guard words (extractor, classifier) | coefficients | tables
    const size_t h_need = carve({front.jpeg ? (size_t)0 : img_b, mk_b, lg_b, bd_b, pr_b, inv_b, gd_b, co_b, qt_b}, h_off);
    // device block: image | small | logits | squares | board | inv | coefficients | tables | planes
    const size_t d_need = carve({img_b, small_b, lg_b, sq_b, bd_b, inv_b, co_b, qt_b, pl_b}, d_off);
    std::lock_guard<std::mutex> pipe_lock(U.pipe_mu);   // one request at a time per extractor engine: the staging blocks are shared
    {
        std::unique_lock<std::mutex> lk(U.mu);
        if (U.pipe_host_bytes < h_need) {
            hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_fail(e, "cv_process_image");
            if (U.pipe_host) block_release(U.pipe_host, U.pipe_host_cap, true);
            U.pipe_host = nullptr; U.pipe_host_bytes = 0; U.pipe_host_cap = 0;
            e = block_alloc(&U.pipe_host, h_need, &U.pipe_host_cap, true);
            if (e != hipSuccess) { U.pipe_host = nullptr; return fail(CV_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
            U.pipe_host_bytes = h_need;
        }
        if (U.pipe_dev.bytes < d_need) {
            hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_fail(e, "cv_process_image");
            U.graph_invalidate();
            CV_TRY(U.pipe_dev.alloc(d_need, false));
        }
    }
    char* hb = (char*)U.pipe_host;
    char* db = (char*)U.pipe_dev.ptr;
    uint8_t* d_img = (uint8_t*)(db + d_off[0]); uint8_t* d_small = (uint8_t*)(db + d_off[1]); float* d_lg = (float*)(db + d_off[2]);
    uint8_t* d_sq = (uint8_t*)(db + d_off[3]); uint8_t* d_bd = (uint8_t*)(db + d_off[4]);
    uint8_t* h_img = (uint8_t*)(hb + h_off[0]); uint8_t* h_mk = (uint8_t*)(hb + h_off[1]); float* h_lg = (float*)(hb + h_off[2]);
    uint8_t* h_bd = (uint8_t*)(hb + h_off[3]); float* h_pr = (float*)(hb + h_off[4]); double* h_inv = (double*)(hb + h_off[5]);
    unsigned* h_gd = (unsigned*)(hb + h_off[6]);

    hipError_t e;
    if (front.jpeg) {
        int16_t* h_co = (int16_t*)(hb + h_off[7]); uint16_t* h_qt = (uint16_t*)(hb + h_off[8]);
        int16_t* d_co = (int16_t*)(db + d_off[6]); uint16_t* d_qt = (uint16_t*)(db + d_off[7]); uint8_t* d_pl = (uint8_t*)(db + d_off[8]);
        char why[200];
        if (cvjpeg::entropy_decode(front.jpeg, front.jpeg_len, h_co, jpeg_blocks * 64, h_qt, nullptr, why, sizeof why) != cvjpeg::kOk)
            return fail(CV_ERR_INVALID, std::string("cv_process_jpeg: ") + why);
        e = hipMemcpyAsync(d_co, h_co, co_b, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_qt, h_qt, qt_b, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = jpeg_reconstruct_oriented_u8(d_co, d_qt, 1, front.info, kJpegBGR, front.orientation, d_pl, d_img, st);
    } else {
        std::memcpy(h_img, image, img_b);
        e = hipMemcpyAsync(d_img, h_img, img_b, hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) return hip_fail(e, "cv_process_image: upload");
    Status s;
    {
        // The mask (64 KB) and the probabilities (3.3 KB) are written by their kernels straight into the page-locked block, which the
        // device sees under its host address: over PCIe inside the kernel instead of a copy operation behind it (-18 us per call for the
        // mask, same-box A/B in profiles/r05_tuning.md section 14).
        std::lock_guard<std::mutex> lk(U.mu);
        s = resize_on_stream(U, d_img, 1, h, w_, 3, d_small, 256, 256, st);
        if (s.ok()) s = unet_forward(U, d_small, true, 1, d_lg, h_mk, threshold, st);
    }
    if (!s.ok()) return s;
    if (!U.pipe_event) e = hipEventCreateWithFlags(&U.pipe_event, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(U.pipe_event, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_lg, d_lg, lg_b, hipMemcpyDeviceToHost, st);     // travels while the host finds the quadrangle
    if (e == hipSuccess) e = hipEventSynchronize(U.pipe_event);
    if (e != hipSuccess) return hip_fail(e, "cv_process_image: mask");
    if (out->mask) std::memcpy(out->mask, h_mk, mk_b);
    int32_t quad[8];
    SideStreamJoin side;                                     // the board's download on U.pipe_side: every exit below waits for it
    bool found = find_quadrangle(h_mk, 256, 256, quad);
    if (!found && fallback_quad) {
        const int32_t whole[8] = {255, 0, 0, 0, 0, 255, 255, 255};            // TR, TL, BL, BR of the mask
        std::memcpy(quad, whole, sizeof(quad));
        found = true;
    }
    if (found) {
        // _scale_quadrangle (core.py:413-417): np.array(approx * (orig_h / 256.0), dtype=float32) -- a double product rounded to float
        float corners[8];
        const double factor = (double)h / 256.0;
        for (int i = 0; i < 8; ++i) { corners[i] = (float)((double)quad[i] * factor); out->quadrangle[i] = corners[i]; }
        board_homographies(corners, 1, 512, 512, nullptr, h_inv);
        e = extract_squares_u8_one(d_img, h, w_, h_inv, d_sq, d_bd, st);   // the matrix travels in the kernel arguments
        // the rectified board (256 KB) goes home on a side stream while the classifier runs: behind the classifier on `st` it was 16 us
        // at the end of every call
        if (e == hipSuccess && !U.pipe_side) e = hipStreamCreateWithFlags(&U.pipe_side, hipStreamNonBlocking);
        if (e == hipSuccess && !U.pipe_event2) e = hipEventCreateWithFlags(&U.pipe_event2, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(U.pipe_event2, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(U.pipe_side, U.pipe_event2, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(h_bd, d_bd, bd_b, hipMemcpyDeviceToHost, U.pipe_side);
        if (e == hipSuccess) side.arm(U.pipe_side);
        if (e == hipSuccess && !U.pipe_event3) e = hipEventCreateWithFlags(&U.pipe_event3, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(U.pipe_event3, U.pipe_side);
        if (e != hipSuccess) return hip_fail(e, "cv_process_image: warp");
        {
            std::lock_guard<std::mutex> lk(C.mu);
            // the 64 x 13 probabilities are written by the head kernel straight into the page-locked block (device-visible under
            // its host address): 3.3 KB over PCIe inside the kernel instead of one more copy operation at the end of the stream
            s = classifier_forward(C, d_sq, true, 64, h_pr, true, st);
        }
        if (!s.ok()) return s;
        // the side stream joins `st` on the DEVICE (the download finished long before the classifier): one host synchronisation per call
        e = hipStreamWaitEvent(st, U.pipe_event3, 0);
        if (e != hipSuccess) return hip_fail(e, "cv_process_image: download");
    }
    {   // the numeric guards ride with the downloads into page-locked memory; ONE synchronisation, then both words are judged
        std::lock_guard<std::mutex> lk(U.mu);
        s = U.guard_read_async(h_gd, st);
    }
    h_gd[1] = 0xffffffffu;
    if (s.ok() && found && &C != &U) {
        std::lock_guard<std::mutex> lk(C.mu);
        s = C.guard_read_async(h_gd + 1, st);
    }
    if (!s.ok()) return s;
    e = hipStreamSynchronize(st);                           // everything above has landed afterwards
    if (e != hipSuccess) return hip_fail(e, "cv_process_image: synchronise");
    side.disarm();                                          // ... the board too: `st` waited for it on the device
    {
        std::lock_guard<std::mutex> lk(U.mu);
        s = U.guard_eval(h_gd[0]);
    }
    if (s.ok() && found && &C != &U) {
        std::lock_guard<std::mutex> lk(C.mu);
        s = C.guard_eval(h_gd[1]);
    }
    if (!s.ok()) return s;
    if (out->logits) std::memcpy(out->logits, h_lg, lg_b);
    if (!found) return Status();
    if (out->board) std::memcpy(out->board, h_bd, bd_b);
    if (out_squares)                                         // extract_squares (core.py:419-439) on the host copy: 4096 rows of 64 bytes
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c)
                for (int y = 0; y < 64; ++y)
                    std::memcpy(out_squares + ((size_t)(r * 8 + c) * 64 + y) * 64, h_bd + (size_t)(r * 64 + y) * 512 + c * 64, 64);
    if (out->probabilities) std::memcpy(out->probabilities, h_pr, pr_b);
    int8_t labels[64];
    decode_positions(h_pr, 1, flip, out->fen, out->original_fen, labels, out->fixes, &out->n_fixes);
    if (out->labels) std::memcpy(out->labels, labels, sizeof(labels));
    out->found = 1;
    return Status();
}

// cv_jpeg_reconstruct_u8 and cv_jpeg_reconstruct_oriented_u8 (`entry` names the one in the messages)
Status jpeg_reconstruct_entry(const char* entry, cv_engine_t* eng, const int16_t* coeffs, const uint16_t* qtables, int n, const cv_jpeg_info_t* info,
                              int channel_order, int orientation, uint8_t* planes, size_t planes_bytes, uint8_t* dst, void* stream) {
    const std::string name(entry);
    CV_TRY(check_engine(eng));
    if (!coeffs || !qtables || !info || !planes || !dst || n <= 0) return fail(CV_ERR_INVALID, name + ": bad argument");
    const cvjpeg::Info& in = *reinterpret_cast<const cvjpeg::Info*>(info);
    CV_TRY(check_jpeg_info(in));
    if (channel_order != CV_JPEG_BGR && channel_order != CV_JPEG_RGB && channel_order != CV_JPEG_GRAY)
        return fail(CV_ERR_INVALID, name + ": unknown channel order");
    if (channel_order == CV_JPEG_GRAY && in.components != 1)
        return fail(CV_ERR_INVALID, name + ": gray output is for 1-component streams only");
    if (orientation < 0 || orientation > 8) return fail(CV_ERR_INVALID, name + ": orientation must be 0..8");
    if (((uintptr_t)coeffs & 15u) || ((uintptr_t)qtables & 15u) || ((uintptr_t)planes & 7u))
        return fail(CV_ERR_INVALID, name + ": coeffs and qtables must be 16-byte aligned, planes 8-byte aligned");
    if ((size_t)n > ((size_t)1 << 31) / cvjpeg::layout_of(in).blocks) return fail(CV_ERR_INVALID, name + ": batch too large");
    if (planes_bytes < jpeg_planes_bytes(in, n)) return fail(CV_ERR_INVALID, name + ": planes buffer too small");
    DeviceGuard g(eng->impl.device);
    const hipError_t e = jpeg_reconstruct_oriented_u8(coeffs, qtables, n, in, channel_order, orientation, planes, dst, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "jpeg_reconstruct_u8");
    return Status();
}

// cv_process_jpeg and cv_process_jpeg_oriented: the stream's header decides the geometry and, when asked, the orientation
Status process_jpeg_entry(const char* entry, cv_engine_t* ue, cv_engine_t* ce, const uint8_t* bytes, size_t len, float threshold, int flip,
                          int fallback_quad, int apply_orientation, cv_image_result_t* out, size_t out_size, void* stream) {
    if (!bytes) return fail(CV_ERR_INVALID, std::string(entry) + ": null stream");
    ImageFront front;
    front.jpeg = bytes;
    front.jpeg_len = len;
    cvjpeg::parse_info(bytes, len, &front.info);
    CV_TRY(check_jpeg_info(front.info));
    front.orientation = apply_orientation ? front.info.orientation : 0;         // the parser reports 0..8 and nothing else
    const bool transposed = front.orientation >= 5;
    return process_image(ue, ce, front, transposed ? front.info.width : front.info.height, transposed ? front.info.height : front.info.width,
                         threshold, flip, fallback_quad, out, out_size, stream);
}

}  // namespace

// ---- the exported C surface: every entry point is exception-tight -----------------------------------------------
extern "C" {

int cv_abi_version(void) { return CV_ABI_VERSION; }
const char* cv_last_error(void) { return get_error(); }

int cv_device_count(int* count) {
    return guarded("cv_device_count", [&]() -> Status {
        if (!count) return fail(CV_ERR_INVALID, "null count");
        hipError_t e = hipGetDeviceCount(count);
        if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
        return Status();
    });
}

int cv_trim_memory(size_t* bytes_freed) {
    return guarded("cv_trim_memory", [&]() -> Status {
        const size_t n = block_cache_trim();
        if (bytes_freed) *bytes_freed = n;
        return Status();
    });
}

int cv_engine_create(int device, int precision, cv_engine_t** out) {
    return guarded("cv_engine_create", [&]() -> Status {
        if (!out) return fail(CV_ERR_INVALID, "null out pointer");
        *out = nullptr;
        if (precision != CV_PREC_F32 && precision != CV_PREC_F16 && precision != CV_PREC_F16X3 && precision != CV_PREC_F16R)
            return fail(CV_ERR_INVALID, "unknown precision");
        static_assert((int)CV_PREC_F32 == (int)kF32 && (int)CV_PREC_F16 == (int)kF16 && (int)CV_PREC_F16X3 == (int)kSplit, "enum values must match");
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0)
            return fail(CV_ERR_HIP, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
        if (device < 0 || device >= count) return fail(CV_ERR_INVALID, "device ordinal out of range");
        DeviceGuard g(device);
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
            return fail(CV_ERR_STATE, std::string("libchessvision_hip is built for gfx950 (MI355X); device is ") + prop.gcnArchName);
        {
            // the dynamic-LDS limits of the conv kernels are raised ONCE per device and process, under a lock: repeating hipFuncSetAttribute
            // at every engine creation while other threads launch those very kernels (request slots: replicas are loaded in the background
            // of a serving instance) is not something the runtime promises to survive
            static std::mutex prep_mu;
            static bool prepared[64] = {};
            std::lock_guard<std::mutex> lk(prep_mu);
            if (device >= 64 || !prepared[device]) {
                if ((e = conv_igemm_prepare()) != hipSuccess) return hip_fail(e, "conv_igemm_prepare");
                if ((e = conv_halo_prepare()) != hipSuccess) return hip_fail(e, "conv_halo_prepare");
                if ((e = conv1x1_lds_prepare()) != hipSuccess) return hip_fail(e, "conv1x1_lds_prepare");
                if (device < 64) prepared[device] = true;
            }
        }
        cv_engine* eng = new (std::nothrow) cv_engine();
        if (!eng) return fail(CV_ERR_NOMEM, "out of host memory");
        eng->impl.device = device;
        eng->impl.dt = precision == CV_PREC_F16R ? (int)kF16 : precision;   // CV_PREC_F32 / F16 / F16X3 values equal cv::DType
        eng->impl.trunk32 = precision == CV_PREC_F16R;
        const Status gs = eng->impl.guard_init();
        if (!gs.ok()) { delete eng; return gs; }
        *out = eng;
        return Status();
    });
}

int cv_engine_destroy(cv_engine_t* eng) {
    return guarded("cv_engine_destroy", [&]() -> Status {
        if (!eng) return Status();
        DeviceGuard g(eng->impl.device);                // every block of the engine goes back to the cache under ITS device
        (void)device_synchronize();
        ReleaseAlreadySynced quiescent;                 // nothing can be queued on a dying engine's buffers from here on
        eng->impl.unet.reset();
        eng->impl.resnet.reset();
        eng->impl.yolo.reset();
        delete eng;
        return Status();
    });
}

int cv_engine_set_chunk(cv_engine_t* eng, int unet_images, int resnet_squares) {
    return guarded("cv_engine_set_chunk", [&]() -> Status {
        CV_TRY(check_engine(eng));
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        if (eng->impl.unet || eng->impl.resnet || eng->impl.yolo) return fail(CV_ERR_STATE, "cv_engine_set_chunk must precede cv_load_*");
        if (unet_images < 0 || resnet_squares < 0) return fail(CV_ERR_INVALID, "negative chunk");
        if (unet_images) eng->impl.unet_chunk = unet_images;
        if (resnet_squares) eng->impl.resnet_chunk = resnet_squares;
        return Status();
    });
}

int cv_load_unet(cv_engine_t* eng, const cv_param_t* params, int n_params) {
    return guarded("cv_load_unet", [&]() -> Status {
        CV_TRY(check_engine(eng));
        std::lock_guard<std::mutex> load_lk(load_mutex());
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        ParamMap pm;
        CV_TRY(to_map(params, n_params, pm));
        return unet_load(eng->impl, pm);
    });
}

int cv_load_resnet(cv_engine_t* eng, const char* arch, const cv_param_t* params, int n_params) {
    return guarded("cv_load_resnet", [&]() -> Status { return load_resnet(eng, arch, params, n_params); });
}

int cv_load_yolo_cls(cv_engine_t* eng, const char* arch, const cv_param_t* params, int n_params) {
    return guarded("cv_load_yolo_cls", [&]() -> Status { return load_yolo_cls(eng, arch, params, n_params); });
}

int cv_load_resnet18(cv_engine_t* eng, const cv_param_t* params, int n_params) {
    return guarded("cv_load_resnet18", [&]() -> Status { return load_resnet(eng, "resnet18", params, n_params); });
}

int cv_unet_forward(cv_engine_t* eng, const float* x, int batch, float* logits, void* stream) {
    return guarded("cv_unet_forward", [&]() -> Status { return unet_entry(eng, x, false, batch, logits, nullptr, 0.5f, nullptr, stream); });
}

int cv_unet_forward_u8(cv_engine_t* eng, const uint8_t* x_u8, int batch, float* logits, uint8_t* mask,
                       float threshold, void* stream) {
    return guarded("cv_unet_forward_u8", [&]() -> Status { return unet_entry(eng, x_u8, true, batch, logits, mask, threshold, nullptr, stream); });
}

int cv_unet_forward_emb(cv_engine_t* eng, const float* x, int batch, float* logits, float* embedding, void* stream) {
    return guarded("cv_unet_forward_emb", [&]() -> Status { return unet_entry(eng, x, false, batch, logits, nullptr, 0.5f, embedding, stream); });
}

int cv_unet_forward_u8_emb(cv_engine_t* eng, const uint8_t* x_u8, int batch, float* logits, uint8_t* mask,
                           float threshold, float* embedding, void* stream) {
    return guarded("cv_unet_forward_u8_emb", [&]() -> Status { return unet_entry(eng, x_u8, true, batch, logits, mask, threshold, embedding, stream); });
}

int cv_unet_forward_mask(cv_engine_t* eng, const float* x, int batch, float* logits, uint8_t* mask, float threshold, float* embedding,
                         void* stream) {
    return guarded("cv_unet_forward_mask", [&]() -> Status { return unet_entry(eng, x, false, batch, logits, mask, threshold, embedding, stream); });
}

int cv_resnet18_forward(cv_engine_t* eng, const float* x, int n, float* logits, void* stream) {
    return guarded("cv_resnet18_forward", [&]() -> Status { return resnet_entry(eng, x, false, n, logits, nullptr, stream, false); });
}

int cv_resnet18_forward_u8(cv_engine_t* eng, const uint8_t* squares_u8, int n, float* probs, void* stream) {
    return guarded("cv_resnet18_forward_u8", [&]() -> Status { return resnet_entry(eng, squares_u8, true, n, probs, nullptr, stream, true); });
}

int cv_resnet18_forward_emb(cv_engine_t* eng, const float* x, int n, float* logits, float* embedding, void* stream) {
    return guarded("cv_resnet18_forward_emb", [&]() -> Status { return resnet_entry(eng, x, false, n, logits, embedding, stream, false); });
}

int cv_resnet18_forward_u8_emb(cv_engine_t* eng, const uint8_t* squares_u8, int n, float* probs, float* embedding, void* stream) {
    return guarded("cv_resnet18_forward_u8_emb", [&]() -> Status { return resnet_entry(eng, squares_u8, true, n, probs, embedding, stream, true); });
}

int cv_resnet_forward_u8_norm(cv_engine_t* eng, const uint8_t* squares_u8, int n, float mean, float std, int softmax, float* out,
                              float* embedding, void* stream) {
    return guarded("cv_resnet_forward_u8_norm", [&]() -> Status {
        const InputNorm norm{mean, std};
        return resnet_entry(eng, squares_u8, true, n, out, embedding, stream, softmax != 0, &norm);
    });
}

int cv_embedding_dim(cv_engine_t* eng, const char* model, int* channels) {
    return guarded("cv_embedding_dim", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!model || !channels) return fail(CV_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        bool is_resnet = false;
        CV_TRY(model_by_name(eng->impl, model, &is_resnet));
        *channels = is_resnet ? classifier_embedding_dim(eng->impl) : unet_embedding_dim(eng->impl);
        if (*channels == 0) return fail(CV_ERR_STATE, "cv_embedding_dim: model '" + std::string(model) + "' is not loaded");
        return Status();
    });
}

int cv_activation_channel_means(cv_engine_t* eng, const char* model, const char* name, float* out_dev, size_t capacity_floats,
                                int64_t dims[2], void* stream) {
    return guarded("cv_activation_channel_means", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!model || !name || !dims) return fail(CV_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        TensorRef t;
        // "global_pool" (the classifier's hook, named_modules()[90]) is the mean of layer4's output: pooled here, it needs no tensor of
        // its own.  The UNet has no tensor of that name.
        const bool pooled_layer4 = std::strcmp(name, "global_pool") == 0 && std::strcmp(model, "unet") != 0;
        CV_TRY(activation_by_name(eng->impl, model, pooled_layer4 ? classifier_pool_tap(eng->impl) : name, &t));
        dims[0] = t.N; dims[1] = t.C;
        if (!out_dev) return Status();                        // shape query
        const std::string tap = "cv_activation_channel_means('" + std::string(name) + "')";
        if (t.N < 1) return fail(CV_ERR_INVALID, tap + ": no forward has run yet");
        if (capacity_floats < (size_t)t.N * t.C)
            return fail(CV_ERR_INVALID, tap + ": output buffer too small, " + std::to_string((size_t)t.N * t.C) + " floats needed");
        if ((uintptr_t)out_dev & 15u) return fail(CV_ERR_INVALID, tap + ": output must be 16-byte aligned");
        if (t.C % 8 || t.split) return fail(CV_ERR_INVALID, tap + ": the tensor's channel slice cannot be pooled");
        hipError_t e = channel_means(eng->impl.dt, t, out_dev, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, tap.c_str());
        return Status();
    });
}

int cv_softmax13(cv_engine_t* eng, const float* logits, int n, float* probs, void* stream) {
    return guarded("cv_softmax13", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (n < 0 || (n > 0 && (!logits || !probs))) return fail(CV_ERR_INVALID, "cv_softmax13: null tensor");
        if (n == 0) return Status();
        DeviceGuard g(eng->impl.device);
        hipError_t e = softmax13(logits, n, probs, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "softmax13");
        return Status();
    });
}

int cv_get_activation(cv_engine_t* eng, const char* model, const char* name, float* out_host, size_t out_capacity,
                      int64_t dims[4]) {
    return guarded("cv_get_activation", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!model || !name || !dims) return fail(CV_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        TensorRef t;
        CV_TRY(activation_by_name(eng->impl, model, name, &t));
        dims[0] = t.N; dims[1] = t.C; dims[2] = t.H; dims[3] = t.W;
        const size_t numel = (size_t)t.N * t.C * t.H * t.W;
        if (!out_host) return Status();                       // shape query
        if (out_capacity < numel) return fail(CV_ERR_INVALID, "output buffer too small");
        DeviceBuffer tmp;
        CV_TRY(tmp.alloc(numel * sizeof(float), false));
        hipError_t e = device_synchronize();
        if (e == hipSuccess) e = unpack_nchw_f32(t.f32_only ? (int)kF32 : eng->impl.dt, t, (float*)tmp.ptr, nullptr);
        if (e == hipSuccess) e = sync_memcpy(out_host, tmp.ptr, numel * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "cv_get_activation");
        return Status();
    });
}

int cv_get_activation_exponent(cv_engine_t* eng, const char* model, const char* name, int* exponent) {
    return guarded("cv_get_activation_exponent", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!model || !name || !exponent) return fail(CV_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        TensorRef t;
        CV_TRY(activation_by_name(eng->impl, model, name, &t));
        *exponent = t.exp;
        return Status();
    });
}

int cv_model_macs(cv_engine_t* eng, const char* model, int64_t* macs) {
    return guarded("cv_model_macs", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!model || !macs) return fail(CV_ERR_INVALID, "null argument");
        bool is_resnet = false;
        CV_TRY(model_by_name(eng->impl, model, &is_resnet));
        *macs = is_resnet ? classifier_macs(eng->impl) : unet_macs(eng->impl);
        if (*macs == 0) return fail(CV_ERR_STATE, "model not loaded");
        return Status();
    });
}

int cv_profile_convs(cv_engine_t* eng, const char* model, const void* x, int batch, void* out, int iters,
                     void* stream, float* conv_ms_total, int* conv_launches, float* all_ms_total) {
    return guarded("cv_profile_convs", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!model || iters <= 0) return fail(CV_ERR_INVALID, "bad profile arguments");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        bool is_resnet = false;
        CV_TRY(model_by_name(e, model, &is_resnet));
        e.prof_clear();
        e.profiling = true;
        Status s;
        for (int i = 0; i < iters && s.ok(); ++i) {
            if (is_resnet) s = classifier_forward(e, x, false, batch, (float*)out, false, (hipStream_t)stream);
            else s = unet_forward(e, x, false, batch, (float*)out, nullptr, 0.5f, (hipStream_t)stream);
        }
        e.profiling = false;
        if (s.ok()) s = e.prof_collect();
        if (!s.ok()) { e.prof_clear(); return s; }
        float conv = 0.f, all = 0.f;
        int n = 0;
        for (auto& pe : e.prof) { all += pe.ms; if (pe.is_conv) { conv += pe.ms; ++n; } }
        if (conv_ms_total) *conv_ms_total = conv;
        if (conv_launches) *conv_launches = n;
        if (all_ms_total) *all_ms_total = all;
        return Status();
    });
}

int cv_profile_entry(cv_engine_t* eng, int index, char* name, int name_cap, float* ms, double* macs, int* is_conv) {
    return guarded("cv_profile_entry", [&]() -> Status {
        CV_TRY(check_engine(eng));
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        if (index < 0 || index >= (int)eng->impl.prof.size()) return fail(CV_ERR_INVALID, "profile index out of range");
        const ProfileEntry& pe = eng->impl.prof[index];
        if (name && name_cap > 0) { std::strncpy(name, pe.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
        if (ms) *ms = pe.ms;
        if (macs) *macs = pe.macs;
        if (is_conv) *is_conv = pe.is_conv ? 1 : 0;
        return Status();
    });
}

int cv_profile_entry_bytes(cv_engine_t* eng, int index, double* bytes) {
    return guarded("cv_profile_entry_bytes", [&]() -> Status {
        CV_TRY(check_engine(eng));
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        if (!bytes || index < 0 || index >= (int)eng->impl.prof.size()) return fail(CV_ERR_INVALID, "profile index out of range");
        *bytes = eng->impl.prof[index].bytes;
        return Status();
    });
}

int cv_profile_entry_kernel(cv_engine_t* eng, int index, char* kernel, int kernel_cap) {
    return guarded("cv_profile_entry_kernel", [&]() -> Status {
        CV_TRY(check_engine(eng));
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        if (!kernel || kernel_cap <= 0 || index < 0 || index >= (int)eng->impl.prof.size()) return fail(CV_ERR_INVALID, "profile index out of range");
        const std::string& k = eng->impl.prof[index].kernel;
        const size_t n = std::min(k.size(), (size_t)kernel_cap - 1);
        std::memcpy(kernel, k.data(), n);
        kernel[n] = 0;
        return Status();
    });
}

int cv_engine_numeric_status(cv_engine_t* eng, void* stream) {
    return guarded("cv_engine_numeric_status", [&]() -> Status {
        CV_TRY(check_engine(eng));
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        return eng->impl.guard_check((hipStream_t)stream);
    });
}

int cv_engine_workspace_bytes(cv_engine_t* eng, size_t* bytes) {
    return guarded("cv_engine_workspace_bytes", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!bytes) return fail(CV_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        *bytes = eng->impl.workspace_bytes();
        return Status();
    });
}

int cv_engine_export_calibration(cv_engine_t* eng, const char* model, int32_t* exps, int capacity, int* count) {
    return guarded("cv_engine_export_calibration", [&]() -> Status { return engine_calibration(eng, model, exps, capacity, count, 0); });
}

int cv_engine_import_calibration(cv_engine_t* eng, const char* model, const int32_t* exps, int count, int* changed) {
    return guarded("cv_engine_import_calibration", [&]() -> Status {
        int ch = 0;
        const Status s = engine_calibration(eng, model, const_cast<int32_t*>(exps), count, &ch, 1);
        if (changed) *changed = ch;
        return s;
    });
}

// The single-layer convolution entry points run their one launch with the launch recorder on (Engine::profiling: run_conv then
// describes the launch it plans -- name, kernel form string, MACs, bytes -- exactly as it does for cv_profile_convs), so that a test can
// ask which kernel form a shape took: cv_profile_entry / cv_profile_entry_kernel describe that launch until the next recorded call.
// The recorder changes no planner choice: it only keeps run_conv from deferring a launch for pairing, which needs a `defer` slot
// that these entry points never set.
static Status run_conv_recorded(Engine& e, ConvLayer& L, const TensorRef& x, const TensorRef& y, const TensorRef* res, int act, hipStream_t st,
                                bool act_first = false) {
    e.prof_clear();
    e.profiling = true;
    Status s = e.run_conv(L, x, y, res, act, st, nullptr, nullptr, nullptr, act_first);
    e.profiling = false;
    if (s.ok()) s = e.prof_collect();
    if (!s.ok()) e.prof_clear();
    return s;
}

int cv_op_conv2d(cv_engine_t* eng, const float* x, int n, int cin, int h, int w_, const float* w_host, int cout,
                 int k, int stride, const float* scale_host, const float* shift_host, const float* residual,
                 int relu, float* y, void* stream) {
    return guarded("cv_op_conv2d", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!x || !w_host || !y || n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w_ <= 0 || stride <= 0)
            return fail(CV_ERR_INVALID, "cv_op_conv2d: bad argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        hipStream_t st = (hipStream_t)stream;
        const int pad = (k - 1) / 2;
        const int ho = (h + 2 * pad - k) / stride + 1, wo = (w_ + 2 * pad - k) / stride + 1;
        const int cinPad = round_up(cin, 8);
        std::vector<float> ones(cout, 1.f), zeros(cout, 0.f);
        ConvLayer L;
        e.ws_slot = 0;
        CV_TRY(L.build_conv("op_conv2d", e.dt, w_host, cout, cin, k, stride, scale_host ? scale_host : ones.data(),
                            shift_host ? shift_host : zeros.data(), cinPad, (int64_t)n * ho * wo, (ho == wo) ? ho : 0));
        Activation ax, ay, ar;
        Status s;
        if ((s = ax.create(n, h, w_, cinPad, e.dt)).ok() && (s = ay.create(n, ho, wo, cout, e.dt)).ok()) {
            hipError_t err = pack_nchw_f32(e.dt, x, cin, ax.ref(n), e.guard_ptr(), st);
            TensorRef rr;
            if (err == hipSuccess && residual) {
                s = ar.create(n, ho, wo, cout, e.dt);
                if (s.ok()) { err = pack_nchw_f32(e.dt, residual, cout, ar.ref(n), e.guard_ptr(), st); rr = ar.ref(n); }
            }
            if (s.ok() && err == hipSuccess) s = run_conv_recorded(e, L, ax.ref(n), ay.ref(n), residual ? &rr : nullptr, relu != 0, st);
            if (s.ok() && err == hipSuccess) err = unpack_nchw_f32(e.dt, ay.ref(n), y, st);
            if (s.ok() && err == hipSuccess) err = hipStreamSynchronize(st);
            if (s.ok() && err != hipSuccess) s = hip_fail(err, "cv_op_conv2d");
        }
        return s;
    });
}

int cv_op_conv2d_act(cv_engine_t* eng, const float* x, int n, int x_channels, int x_coff, int cin, int h, int w_, const float* w_host, int cout,
                     int k, int stride, const float* scale_host, const float* shift_host, int act, int act_first, float* y, int y_channels,
                     int y_coff, int res_coff, int in_exp, int out_exp, void* stream) {
    return guarded("cv_op_conv2d_act", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!x || !w_host || !y || n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w_ <= 0 || stride <= 0 || x_coff < 0 || y_coff < 0 ||
            x_coff + cin > x_channels || y_coff + cout > y_channels || x_channels % 8 || y_channels % 8 || cin % 8 ||
            (res_coff >= 0 && res_coff + cout > y_channels) || in_exp < -60 || in_exp > 60 || out_exp < -60 || out_exp > 60)
            return fail(CV_ERR_INVALID, "cv_op_conv2d_act: bad argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        if (e.dt == kF32 && (in_exp || out_exp)) return fail(CV_ERR_INVALID, "cv_op_conv2d_act: the f32 engine stores true values (exponents must be 0)");
        hipStream_t st = (hipStream_t)stream;
        const int pad = (k - 1) / 2;
        const int ho = (h + 2 * pad - k) / stride + 1, wo = (w_ + 2 * pad - k) / stride + 1;
        std::vector<float> ones(cout, 1.f), zeros(cout, 0.f);
        ConvLayer L;
        e.ws_slot = 0;
        CV_TRY(L.build_conv("op_conv2d_act", e.dt, w_host, cout, cin, k, stride, scale_host ? scale_host : ones.data(),
                            shift_host ? shift_host : zeros.data(), cin, (int64_t)n * ho * wo, (ho == wo) ? ho : 0));
        Activation ax, ay;
        ax.exp = in_exp; ay.exp = out_exp;
        CV_TRY(ax.create(n, h, w_, x_channels, e.dt));
        CV_TRY(ay.create(n, ho, wo, y_channels, e.dt));
        hipError_t err = pack_nchw_f32(e.dt, x, x_channels, ax.ref(n), e.guard_ptr(), st);
        if (err == hipSuccess) err = pack_nchw_f32(e.dt, y, y_channels, ay.ref(n), e.guard_ptr(), st);      // what the launch must leave alone
        if (err != hipSuccess) return hip_fail(err, "cv_op_conv2d_act");
        const TensorRef rr = ay.ref(n, res_coff < 0 ? 0 : res_coff, cout);
        CV_TRY(run_conv_recorded(e, L, ax.ref(n, x_coff, cin), ay.ref(n, y_coff, cout), res_coff >= 0 ? &rr : nullptr, act, st, act_first != 0));
        err = unpack_nchw_f32(e.dt, ay.ref(n), y, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        return err != hipSuccess ? hip_fail(err, "cv_op_conv2d_act") : Status();
    });
}

int cv_op_conv_epilogue_ok(int form, int act, int act_first, int with_head, int with_pool, int with_fuse0, int shuffle, int* ok) {
    return guarded("cv_op_conv_epilogue_ok", [&]() -> Status {
        if (!ok || form < 0 || form > 4) return fail(CV_ERR_INVALID, "cv_op_conv_epilogue_ok: bad argument");
        if (form == 4) {                                     // the planner's own check (Engine::run_conv)
            *ok = Engine::epilogue_plan_ok(act, act_first != 0, with_head != 0, with_pool != 0, with_fuse0 != 0, shuffle != 0) ? 1 : 0;
            return Status();
        }
        // the predicate every launcher of that form asks first (conv_igemm.h: conv_epilogue_ok); it reads the options and whether a
        // fused head / pool rides on the epilogue, never through a pointer
        static float dummy;
        ConvParams p;
        std::memset(&p, 0, sizeof(p));
        p.relu = act; p.act_first = act_first; p.act_in = p.act_out = 1.f;
        if (with_head) p.head_w = &dummy;
        if (with_pool) p.pool_y = reinterpret_cast<char*>(&dummy);
        *ok = conv_epilogue_ok(form, p) ? 1 : 0;
        return Status();
    });
}

int cv_op_stem3x3s2(cv_engine_t* eng, const void* x, int x_u8, int n, int c0, const float* w_host, const float* scale_host,
                    const float* shift_host, float mean, float std, int out_exp, float* y, void* stream) {
    return guarded("cv_op_stem3x3s2", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!x || !w_host || !scale_host || !shift_host || !y || n <= 0 || c0 < 8 || c0 % 8 || out_exp < -60 || out_exp > 60)
            return fail(CV_ERR_INVALID, "cv_op_stem3x3s2: bad argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        hipStream_t st = (hipStream_t)stream;
        DeviceBuffer w, sc, sh;
        CV_TRY(w.upload(w_host, (size_t)c0 * 9 * sizeof(float)));
        CV_TRY(sc.upload(scale_host, (size_t)c0 * sizeof(float)));
        CV_TRY(sh.upload(shift_host, (size_t)c0 * sizeof(float)));
        Activation ay;
        ay.exp = e.dt == kF32 ? 0 : out_exp;
        CV_TRY(ay.create(n, 32, 32, c0, e.dt));
        const InputNorm nm{mean, std};
        hipError_t err = stem3x3s2(e.dt, x, x_u8 != 0, n, (const float*)w.ptr, (const float*)sc.ptr, (const float*)sh.ptr, ay.ref(n),
                                   e.guard_ptr(), 0xfffffffeu, st, (x_u8 && std > 0.f) ? &nm : nullptr);
        if (err == hipSuccess) err = unpack_nchw_f32(e.dt, ay.ref(n), y, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        return err != hipSuccess ? hip_fail(err, "cv_op_stem3x3s2") : Status();
    });
}

int cv_op_head_pool_fc(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, const float* w_host, const float* bias_host,
                       int softmax, int in_exp, float* out, float* pooled, void* stream) {
    return guarded("cv_op_head_pool_fc", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!x || !w_host || !bias_host || !out || n <= 0 || c < 8 || c % 8 || h <= 0 || w_ <= 0 || in_exp < -60 || in_exp > 60)
            return fail(CV_ERR_INVALID, "cv_op_head_pool_fc: bad argument");
        CV_TRY(check_embedding(pooled));
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        hipStream_t st = (hipStream_t)stream;
        DeviceBuffer w, b;
        CV_TRY(w.upload(w_host, (size_t)13 * c * sizeof(float)));
        CV_TRY(b.upload(bias_host, 13 * sizeof(float)));
        Activation ax;
        ax.exp = e.dt == kF32 ? 0 : in_exp;
        CV_TRY(ax.create(n, h, w_, c, e.dt));
        hipError_t err = pack_nchw_f32(e.dt, x, c, ax.ref(n), e.guard_ptr(), st);
        if (err == hipSuccess)
            err = head_pool_fc(e.dt, ax.ref(n), (const float*)w.ptr, (const float*)b.ptr, out, pooled, softmax, e.guard_ptr(), 0xfffffffeu, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        return err != hipSuccess ? hip_fail(err, "cv_op_head_pool_fc") : Status();
    });
}

int cv_op_conv_transpose2x2(cv_engine_t* eng, const float* x, int n, int cin, int h, int w_, const float* w_host,
                            int cout, const float* bias_host, float* y, void* stream) {
    return guarded("cv_op_conv_transpose2x2", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!x || !w_host || !y || !bias_host || n <= 0) return fail(CV_ERR_INVALID, "cv_op_conv_transpose2x2: bad argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        hipStream_t st = (hipStream_t)stream;
        ConvLayer L;
        e.ws_slot = 0;
        CV_TRY(L.build_convT("op_convT", e.dt, w_host, cin, cout, bias_host, (int64_t)n * h * w_));
        Activation ax, ay;
        Status s;
        if ((s = ax.create(n, h, w_, cin, e.dt)).ok() && (s = ay.create(n, 2 * h, 2 * w_, cout, e.dt)).ok()) {
            hipError_t err = pack_nchw_f32(e.dt, x, cin, ax.ref(n), e.guard_ptr(), st);
            if (err == hipSuccess) s = run_conv_recorded(e, L, ax.ref(n), ay.ref(n), nullptr, false, st);
            if (s.ok() && err == hipSuccess) err = unpack_nchw_f32(e.dt, ay.ref(n), y, st);
            if (s.ok() && err == hipSuccess) err = hipStreamSynchronize(st);
            if (s.ok() && err != hipSuccess) s = hip_fail(err, "cv_op_conv_transpose2x2");
        }
        return s;
    });
}

// conv 1x1 C -> 1 + bias (+ sigmoid / threshold mask): the stand-alone OutConv kernel, as a single-layer entry point
int cv_op_outc_1x1(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, const float* w_host, const float* bias_host,
                   float threshold, float* logits, uint8_t* mask, void* stream) {
    return guarded("cv_op_outc_1x1", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!x || !w_host || !bias_host || !logits || n <= 0 || c <= 0 || h <= 0 || w_ <= 0)
            return fail(CV_ERR_INVALID, "cv_op_outc_1x1: bad argument");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        hipStream_t st = (hipStream_t)stream;
        const int cp = round_up(c, 8);
        const int lpp = cp / dtype_group(e.dt);
        if (lpp > 64 || (lpp & (lpp - 1))) return fail(CV_ERR_INVALID, "cv_op_outc_1x1: channel count must give a power-of-two lane group <= 64");
        std::vector<float> wpad(cp, 0.f);
        std::copy(w_host, w_host + c, wpad.begin());
        Activation ax;
        DeviceBuffer dw, db;
        Status s;
        if ((s = ax.create(n, h, w_, cp, e.dt)).ok() && (s = dw.upload(wpad.data(), cp * sizeof(float))).ok() &&
            (s = db.upload(bias_host, sizeof(float))).ok()) {
            hipError_t err = pack_nchw_f32(e.dt, x, c, ax.ref(n), e.guard_ptr(), st);
            if (err == hipSuccess)
                err = outc_1x1(e.dt, ax.ref(n), (const float*)dw.ptr, (const float*)db.ptr, logits, mask, threshold, e.guard_ptr(),
                               e.register_layer("op_outc_1x1"), st);
            if (err == hipSuccess) err = hipStreamSynchronize(st);
            if (err != hipSuccess) s = hip_fail(err, "cv_op_outc_1x1");
        }
        return s;
    });
}

int cv_op_maxpool2x2(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, float* y, void* stream) {
    return guarded("cv_op_maxpool2x2", [&]() -> Status { return pool_like(eng, x, n, c, h, w_, h / 2, w_ / 2, y, stream, maxpool2x2, "cv_op_maxpool2x2"); });
}

int cv_op_maxpool3x3s2(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, float* y, void* stream) {
    return guarded("cv_op_maxpool3x3s2", [&]() -> Status {
        return pool_like(eng, x, n, c, h, w_, (h + 2 - 3) / 2 + 1, (w_ + 2 - 3) / 2 + 1, y, stream, maxpool3x3s2, "cv_op_maxpool3x3s2");
    });
}

int cv_op_upsample_bilinear2x(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, float* y, void* stream) {
    return guarded("cv_op_upsample_bilinear2x", [&]() -> Status {
        return pool_like(eng, x, n, c, h, w_, 2 * h, 2 * w_, y, stream, upsample_plain, "cv_op_upsample_bilinear2x");
    });
}

int cv_selftest_mfma(cv_engine_t* eng, float* max_err_f16, float* max_err_f32) {
    return guarded("cv_selftest_mfma", [&]() -> Status {
        CV_TRY(check_engine(eng));
        DeviceGuard g(eng->impl.device);
        // asymmetric integer-valued operands: exact in f16 and f32, so the expected error is exactly 0
        _Float16 a16[16 * 32], b16[16 * 32];
        float a32[16 * 16], b32[16 * 16], ref16[256], ref32[256], got[256];
        for (int i = 0; i < 16; ++i)
            for (int k = 0; k < 32; ++k) { a16[i * 32 + k] = (_Float16)(float)((i * 3 + k * 5) % 7 - 3); b16[i * 32 + k] = (_Float16)(float)((i * 5 + k * 2 + 1) % 9 - 4); }
        for (int i = 0; i < 16; ++i)
            for (int k = 0; k < 16; ++k) { a32[i * 16 + k] = (float)((i * 3 + k * 5) % 7 - 3); b32[i * 16 + k] = (float)((i * 5 + k * 2 + 1) % 9 - 4); }
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                float s16 = 0, s32 = 0;
                for (int k = 0; k < 32; ++k) s16 += (float)a16[i * 32 + k] * (float)b16[j * 32 + k];
                for (int k = 0; k < 16; ++k) s32 += a32[i * 16 + k] * b32[j * 16 + k];
                ref16[i * 16 + j] = s16; ref32[i * 16 + j] = s32;
            }
        DeviceBuffer da, db, dd;
        float err16 = 0.f, err32 = 0.f;
        CV_TRY(da.upload(a16, sizeof(a16)));
        CV_TRY(db.upload(b16, sizeof(b16)));
        CV_TRY(dd.alloc(sizeof(got), true));
        hipError_t e = mfma_probe_f16((const half_t*)da.ptr, (const half_t*)db.ptr, (float*)dd.ptr, nullptr);
        if (e == hipSuccess) e = sync_memcpy(got, dd.ptr, sizeof(got), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "mfma_probe_f16");
        for (int i = 0; i < 256; ++i) err16 = std::max(err16, std::fabs(got[i] - ref16[i]));
        CV_TRY(da.upload(a32, sizeof(a32)));
        CV_TRY(db.upload(b32, sizeof(b32)));
        e = mfma_probe_f32((const float*)da.ptr, (const float*)db.ptr, (float*)dd.ptr, nullptr);
        if (e == hipSuccess) e = sync_memcpy(got, dd.ptr, sizeof(got), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "mfma_probe_f32");
        for (int i = 0; i < 256; ++i) err32 = std::max(err32, std::fabs(got[i] - ref32[i]));
        if (max_err_f16) *max_err_f16 = err16;
        if (max_err_f32) *max_err_f32 = err32;
        return Status();
    });
}

int cv_find_quadrangle(const uint8_t* mask, int h, int w, int32_t quad[8], int* found) {
    return guarded("cv_find_quadrangle", [&]() -> Status {
        if (!mask || !quad || !found || h <= 0 || w <= 0) return fail(CV_ERR_INVALID, "cv_find_quadrangle: bad argument");
        *found = find_quadrangle(mask, h, w, quad) ? 1 : 0;
        return Status();
    });
}

int cv_find_contours(const uint8_t* mask, int h, int w, int method, int32_t* xy, int64_t cap_points, int32_t* counts,
                     int32_t* holes, int64_t cap_contours, int64_t* n_contours) {
    return guarded("cv_find_contours", [&]() -> Status {
        if (!mask || !xy || !counts || !holes || !n_contours || h <= 0 || w <= 0 || cap_points < 0 || cap_contours < 0 ||
            (method != 0 && method != 1))
            return fail(CV_ERR_INVALID, "cv_find_contours: bad argument");
        const long n = find_contours_flat(mask, h, w, method == 1, xy, (long)cap_points, counts, holes, (long)cap_contours);
        if (n < 0) return fail(CV_ERR_INVALID, "cv_find_contours: output capacity too small");
        *n_contours = n;
        return Status();
    });
}

int cv_find_quadrangles(const uint8_t* masks, int n, int h, int w, int32_t* quads, int32_t* found, int n_threads) {
    return guarded("cv_find_quadrangles", [&]() -> Status {
        if (!masks || !quads || !found || n < 0 || h <= 0 || w <= 0) return fail(CV_ERR_INVALID, "cv_find_quadrangles: bad argument");
        parallel_slices(n, mask_threads(n, n_threads), [&](int lo, int hi) {
            for (int i = lo; i < hi; ++i) found[i] = find_quadrangle(masks + (size_t)i * h * w, h, w, quads + (size_t)i * 8) ? 1 : 0;
        });
        return Status();
    });
}

int cv_mask_completeness(const uint8_t* mask, int h, int w, double* score) {
    return guarded("cv_mask_completeness", [&]() -> Status { return mask_completenesses(mask, 1, h, w, score, 1); });
}

int cv_mask_completenesses(const uint8_t* masks, int n, int h, int w, double* scores, int n_threads) {
    return guarded("cv_mask_completenesses", [&]() -> Status { return mask_completenesses(masks, n, h, w, scores, n_threads); });
}

int cv_quadrangle_regularity(const float* quad, double* score) {
    return guarded("cv_quadrangle_regularity", [&]() -> Status {
        if (!score) return fail(CV_ERR_INVALID, "cv_quadrangle_regularity: null score");
        *score = quad ? quadrangle_regularity(quad) : 0.0;
        return Status();
    });
}

int cv_extraction_scores(cv_engine_t* eng, const float* values, int n, int count, int transform, cv_score_record_t* records,
                         uint8_t* half_mask, void* stream) {
    return guarded("cv_extraction_scores", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!values || !records) return fail(CV_ERR_INVALID, "cv_extraction_scores: null tensor");
        if (((uintptr_t)values & 3u) || ((uintptr_t)records & 7u)) return fail(CV_ERR_INVALID, "cv_extraction_scores: values must be 4-byte, records 8-byte aligned");
        if (n < 1) return fail(CV_ERR_INVALID, "cv_extraction_scores: n must be at least 1");
        if (count < 4 || count > (1 << 24)) return fail(CV_ERR_INVALID, "cv_extraction_scores: count must be in [4, 2^24]");
        if (transform != 0 && transform != 1) return fail(CV_ERR_INVALID, "cv_extraction_scores: transform must be 0 (as given) or 1 (sigmoid)");
        DeviceGuard g(eng->impl.device);
        hipError_t e = extraction_scores(values, n, count, transform, reinterpret_cast<ScoreRecord*>(records), half_mask, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "extraction_scores");
        return Status();
    });
}

int cv_extraction_scores_finish(const cv_score_record_t* records, int n, double* confidence, double* distribution) {
    return guarded("cv_extraction_scores_finish", [&]() -> Status {
        if (n < 0 || (n > 0 && (!records || !confidence || !distribution))) return fail(CV_ERR_INVALID, "cv_extraction_scores_finish: bad argument");
        const double nan = std::nan("");
        for (int i = 0; i < n; ++i) {
            const cv_score_record_t& r = records[i];
            // numpy's sort puts NaN last, so one NaN in the image reaches the top quarter and the mean
            confidence[i] = r.n_nan > 0 || r.top_count <= 0 ? nan : 2.0 * r.top_sum / (double)r.top_count;
            long long total = 0;
            for (int b = 0; b < 10; ++b) total += r.hist[b];
            if (total == 0) { distribution[i] = nan; continue; }           // 0 / 0 in the reference's hist / sum(hist)
            double entropy = 0.0;
            for (int b = 0; b < 10; ++b) {
                const double p = (double)r.hist[b] / (double)total;
                entropy -= p * std::log2(p + 1e-10);
            }
            distribution[i] = 1.0 - entropy / std::log2(10.0);
        }
        return Status();
    });
}

int cv_segmentation_scores(cv_engine_t* eng, const float* logits, const uint8_t* labels, int n, int count, float threshold,
                           cv_seg_record_t* records, void* stream) {
    return guarded("cv_segmentation_scores", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!logits || !labels || !records) return fail(CV_ERR_INVALID, "cv_segmentation_scores: null tensor");
        if (((uintptr_t)logits & 3u) || ((uintptr_t)records & 7u)) return fail(CV_ERR_INVALID, "cv_segmentation_scores: logits must be 4-byte, records 8-byte aligned");
        if (n < 1) return fail(CV_ERR_INVALID, "cv_segmentation_scores: n must be at least 1");
        if (count < 1 || count > (1 << 24)) return fail(CV_ERR_INVALID, "cv_segmentation_scores: count must be in [1, 2^24]");
        if (!std::isfinite(threshold)) return fail(CV_ERR_INVALID, "cv_segmentation_scores: threshold must be finite");
        DeviceGuard g(eng->impl.device);
        hipError_t e = segmentation_scores(logits, labels, n, count, threshold, reinterpret_cast<SegRecord*>(records), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "segmentation_scores");
        return Status();
    });
}

int cv_segmentation_scores_finish(const cv_seg_record_t* records, int n, double* bce, double* dice_loss, double* loss, double* dice,
                                  double* iou, double* pixel_accuracy) {
    return guarded("cv_segmentation_scores_finish", [&]() -> Status {
        if (n < 0 || (n > 0 && !records)) return fail(CV_ERR_INVALID, "cv_segmentation_scores_finish: bad argument");
        for (int i = 0; i < n; ++i) {
            const cv_seg_record_t& r = records[i];
            if (r.count < 1) return fail(CV_ERR_INVALID, "cv_segmentation_scores_finish: record " + std::to_string(i) + " has no pixels");
            const double b = r.bce_sum / (double)r.count;
            const double dl = 1.0 - dice_of(r.sig_label_sum, r.sig_sum + (double)r.n_label);
            if (bce) bce[i] = b;
            if (dice_loss) dice_loss[i] = dl;
            if (loss) loss[i] = dl + b;
            hard_mask_scores(r.n_label, r.n_pred, r.n_both, r.count, dice ? dice + i : nullptr, iou ? iou + i : nullptr,
                             pixel_accuracy ? pixel_accuracy + i : nullptr);
        }
        return Status();
    });
}

int cv_threshold_levels(cv_engine_t* eng, const float* logits, const uint8_t* labels, int n, int count, const float* thresholds,
                        int n_thresholds, uint8_t* levels, cv_level_record_t* records, void* stream) {
    return guarded("cv_threshold_levels", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!logits || !thresholds || !levels || !records) return fail(CV_ERR_INVALID, "cv_threshold_levels: null tensor");
        if (((uintptr_t)logits & 3u) || ((uintptr_t)records & 3u)) return fail(CV_ERR_INVALID, "cv_threshold_levels: logits and records must be 4-byte aligned");
        if (n < 1) return fail(CV_ERR_INVALID, "cv_threshold_levels: n must be at least 1");
        if (count < 1 || count > (1 << 24)) return fail(CV_ERR_INVALID, "cv_threshold_levels: count must be in [1, 2^24]");
        if (n_thresholds < 1 || n_thresholds > CV_MAX_THRESHOLDS)
            return fail(CV_ERR_INVALID, "cv_threshold_levels: n_thresholds must be in [1, " + std::to_string(CV_MAX_THRESHOLDS) + "]");
        for (int k = 0; k < n_thresholds; ++k) {
            if (!(thresholds[k] >= 0.f && thresholds[k] <= 1.f))
                return fail(CV_ERR_INVALID, "cv_threshold_levels: threshold " + std::to_string(k) + " is not in [0, 1]");
            if (k > 0 && !(thresholds[k] > thresholds[k - 1]))
                return fail(CV_ERR_INVALID, "cv_threshold_levels: thresholds must be strictly ascending (entry " + std::to_string(k) + ")");
        }
        DeviceGuard g(eng->impl.device);
        hipError_t e = threshold_levels(logits, labels, n, count, thresholds, n_thresholds, levels, reinterpret_cast<LevelRecord*>(records),
                                        (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "threshold_levels");
        return Status();
    });
}

int cv_threshold_levels_finish(const cv_level_record_t* records, int n, int labels_present, double* dice, double* iou,
                               double* pixel_accuracy) {
    return guarded("cv_threshold_levels_finish", [&]() -> Status {
        if (n < 0 || (n > 0 && !records)) return fail(CV_ERR_INVALID, "cv_threshold_levels_finish: bad argument");
        for (int i = 0; i < n; ++i) {
            const cv_level_record_t& r = records[i];
            const int T = records[0].n_thresholds;
            if (r.count < 1) return fail(CV_ERR_INVALID, "cv_threshold_levels_finish: record " + std::to_string(i) + " has no pixels");
            if (T < 1 || T > CV_MAX_THRESHOLDS || r.n_thresholds != T)
                return fail(CV_ERR_INVALID, "cv_threshold_levels_finish: record " + std::to_string(i) + " is not of the same threshold grid");
            long long n_label = 0, n_pred = 0, n_both = 0;
            if (labels_present)
                for (int l = 0; l <= T; ++l) n_label += r.hist[1][l];
            for (int k = T - 1; k >= 0; --k) {                // suffix sums: level k + 1 joins the mask at thresholds[k]
                n_pred += (long long)r.hist[0][k + 1] + r.hist[1][k + 1];
                if (labels_present) n_both += r.hist[1][k + 1];
                const size_t at = (size_t)i * T + k;
                hard_mask_scores(n_label, n_pred, n_both, r.count, dice ? dice + at : nullptr, iou ? iou + at : nullptr,
                                 pixel_accuracy ? pixel_accuracy + at : nullptr);
            }
        }
        return Status();
    });
}

int cv_fen_labels(const char* fen, int8_t* labels) {
    return guarded("cv_fen_labels", [&]() -> Status {
        if (!fen || !labels) return fail(CV_ERR_INVALID, "cv_fen_labels: null argument");
        int8_t out[64];
        const char* why = fen_labels(fen, out);
        if (why) return fail(CV_ERR_INVALID, std::string("cv_fen_labels: malformed piece placement (") + why + ")");
        std::memcpy(labels, out, 64);
        return Status();
    });
}

int cv_classification_scores(const float* probs, const int8_t* labels, int n_boards, cv_square_score_t* per_square,
                             cv_board_score_t* per_board) {
    return guarded("cv_classification_scores", [&]() -> Status {
        if (n_boards < 0 || (n_boards > 0 && (!probs || !labels || !per_square || !per_board)))
            return fail(CV_ERR_INVALID, "cv_classification_scores: bad argument");
        for (size_t i = 0; i < (size_t)n_boards * 64; ++i)
            if (labels[i] < 0 || labels[i] > 12)
                return fail(CV_ERR_INVALID, "cv_classification_scores: label " + std::to_string(i) + " is not a class index (0..12)");
        classification_scores(probs, labels, n_boards, per_square, per_board);
        return Status();
    });
}

int cv_square_records(cv_engine_t* eng, const float* logits, const int8_t* labels, int n, cv_square_record_t* records, void* stream) {
    return guarded("cv_square_records", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!logits || !records) return fail(CV_ERR_INVALID, "cv_square_records: null tensor");
        if (((uintptr_t)logits & 3u) || ((uintptr_t)records & 7u)) return fail(CV_ERR_INVALID, "cv_square_records: logits must be 4-byte, records 8-byte aligned");
        if (n < 1) return fail(CV_ERR_INVALID, "cv_square_records: n must be at least 1");
        DeviceGuard g(eng->impl.device);
        hipError_t e = square_records(logits, labels, n, reinterpret_cast<SquareRecord*>(records), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "square_records");
        return Status();
    });
}

int cv_square_records_finish(const cv_square_record_t* records, int n, int batch_size, cv_squares_summary_t* out) {
    return guarded("cv_square_records_finish", [&]() -> Status {
        if (!out || n < 0 || (n > 0 && !records)) return fail(CV_ERR_INVALID, "cv_square_records_finish: bad argument");
        std::memset(out, 0, sizeof(*out));
        out->n = n;
        const int bs = batch_size > 0 ? batch_size : std::max(n, 1);
        double running = 0.0;                                 // validate(): running_loss += criterion(output, target).item()
        for (int lo = 0; lo < n; lo += bs) {
            double batch_sum = 0.0;
            int batch_n = 0;
            for (int i = lo; i < std::min(n, lo + bs); ++i) {
                const cv_square_record_t& r = records[i];
                if (r.flags & 2) return fail(CV_ERR_INVALID, "cv_square_records_finish: record " + std::to_string(i) + " carries a label outside -1..12");
                if (r.flags & 1) ++out->n_nan;
                if (r.label < 0) continue;
                if (r.label > 12 || r.predicted < 0 || r.predicted > 12)
                    return fail(CV_ERR_INVALID, "cv_square_records_finish: record " + std::to_string(i) + " is not a record of cv_square_records");
                ++batch_n;
                batch_sum += (double)r.loss;
                if (!(r.flags & 1) && r.predicted == r.label) ++out->n_correct;
                for (int k = std::max(r.rank, 0); k < 13; ++k) ++out->hits[k];
                ++out->confusion[r.label * 13 + r.predicted];
            }
            if (!batch_n) continue;
            out->n_labelled += batch_n;
            out->loss_sum += batch_sum;
            running += batch_sum / (double)batch_n;
            ++out->n_batches;
        }
        const double nan = std::nan("");
        out->val_loss = out->n_batches ? running / (double)out->n_batches : nan;
        out->val_acc = out->n_labelled ? 100.0 * (double)out->n_correct / (double)out->n_labelled : nan;
        if (!out->n_labelled) out->loss_sum = nan;
        return Status();
    });
}

int cv_decode_positions(const float* probs, int n_boards, int flip, char* fen, char* original_fen, int8_t* labels,
                        int32_t* fixes, int32_t* n_fixes) {
    return guarded("cv_decode_positions", [&]() -> Status {
        if (n_boards < 0 || (n_boards > 0 && (!probs || !fen || !original_fen || !labels || !fixes || !n_fixes)))
            return fail(CV_ERR_INVALID, "cv_decode_positions: bad argument");
        decode_positions(probs, n_boards, flip, fen, original_fen, labels, fixes, n_fixes);
        return Status();
    });
}

int cv_board_homographies(const float* quads, int n, int out_w, int out_h, double* forward, double* inverse) {
    return guarded("cv_board_homographies", [&]() -> Status {
        if (n < 0 || out_w <= 0 || out_h <= 0 || (n > 0 && (!quads || (!forward && !inverse))))
            return fail(CV_ERR_INVALID, "cv_board_homographies: bad argument");
        board_homographies(quads, n, out_w, out_h, forward, inverse);
        return Status();
    });
}

int cv_resize_area_u8(cv_engine_t* eng, const uint8_t* src, int n, int h, int w_, int channels, uint8_t* dst, int out_h,
                      int out_w, void* stream) {
    return guarded("cv_resize_area_u8", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!src || !dst || n <= 0 || h <= 0 || w_ <= 0 || channels <= 0 || out_h <= 0 || out_w <= 0)
            return fail(CV_ERR_INVALID, "cv_resize_area_u8: bad argument");
        DeviceGuard g(eng->impl.device);
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        return resize_on_stream(eng->impl, src, n, h, w_, channels, dst, out_h, out_w, (hipStream_t)stream);
    });
}

int cv_resize_antialias_f32(cv_engine_t* eng, const uint8_t* src, int n, int h, int w_, int channels, float* dst, int out_h,
                            int out_w, void* stream) {
    return guarded("cv_resize_antialias_f32", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!src || !dst || n <= 0 || h <= 0 || w_ <= 0 || channels < 1 || channels > 4 || out_h <= 0 || out_w <= 0 || ((uintptr_t)dst & 3u) ||
            out_h > 65535 * 16)
            return fail(CV_ERR_INVALID, "cv_resize_antialias_f32: bad argument");
        DeviceGuard g(eng->impl.device);
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        return resize_antialias_on_stream(eng->impl, src, n, h, w_, channels, dst, out_h, out_w, (hipStream_t)stream);
    });
}

int cv_extract_squares_u8(cv_engine_t* eng, const uint8_t* images, int n, int h, int w_, const double* inv_host,
                          uint8_t* squares, uint8_t* boards, void* stream) {
    return guarded("cv_extract_squares_u8", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!images || !inv_host || !squares || n <= 0 || h <= 0 || w_ <= 0)
            return fail(CV_ERR_INVALID, "cv_extract_squares_u8: bad argument");
        if ((size_t)h * (size_t)w_ > ((size_t)1 << 30)) return fail(CV_ERR_INVALID, "cv_extract_squares_u8: image too large (32-bit byte offsets)");
        if (((uintptr_t)squares & 3) || ((uintptr_t)boards & 3)) return fail(CV_ERR_INVALID, "cv_extract_squares_u8: outputs must be 4-byte aligned");
        std::lock_guard<std::mutex> lk(eng->impl.mu);
        DeviceGuard g(eng->impl.device);
        Engine& e = eng->impl;
        const size_t bytes = (size_t)n * 9 * sizeof(double);
        if (e.scratch.bytes < bytes) CV_TRY(e.scratch.alloc(bytes, false));
        hipStream_t st = (hipStream_t)stream;
        hipError_t err = hipMemcpyAsync(e.scratch.ptr, inv_host, bytes, hipMemcpyHostToDevice, st);
        if (err == hipSuccess) err = extract_squares_u8(images, n, h, w_, (const double*)e.scratch.ptr, squares, boards, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);       // inv_host may be reused by the caller; scratch by the next call
        if (err != hipSuccess) return hip_fail(err, "extract_squares_u8");
        return Status();
    });
}

int cv_extract_squares_u8_dev(cv_engine_t* eng, const uint8_t* images, int n, int h, int w_, const double* inv_dev,
                              uint8_t* squares, uint8_t* boards, void* stream) {
    return guarded("cv_extract_squares_u8_dev", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!images || !inv_dev || !squares || n <= 0 || h <= 0 || w_ <= 0)
            return fail(CV_ERR_INVALID, "cv_extract_squares_u8_dev: bad argument");
        if ((size_t)h * (size_t)w_ > ((size_t)1 << 30)) return fail(CV_ERR_INVALID, "cv_extract_squares_u8_dev: image too large (32-bit byte offsets)");
        if (((uintptr_t)squares & 3) || ((uintptr_t)boards & 3) || ((uintptr_t)inv_dev & 7))
            return fail(CV_ERR_INVALID, "cv_extract_squares_u8_dev: outputs must be 4-byte aligned, matrices 8-byte aligned");
        DeviceGuard g(eng->impl.device);
        hipError_t err = extract_squares_u8(images, n, h, w_, inv_dev, squares, boards, (hipStream_t)stream);
        if (err != hipSuccess) return hip_fail(err, "extract_squares_u8");
        return Status();
    });
}

int cv_process_image_v2(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* image, int h, int w, float threshold,
                        int flip, int fallback_quad, cv_image_result_t* out, size_t out_size, void* stream) {
    return guarded("cv_process_image_v2", [&]() -> Status {
        ImageFront front;
        front.image = image;
        return process_image(unet_engine, classifier_engine, front, h, w, threshold, flip, fallback_quad, out, out_size, stream);
    });
}

int cv_process_image(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* image, int h, int w, float threshold,
                     int flip, int fallback_quad, cv_image_result_t* out, void* stream) {
    return guarded("cv_process_image", [&]() -> Status {      // the struct of ABI 3 / 4: `squares` did not exist
        ImageFront front;
        front.image = image;
        return process_image(unet_engine, classifier_engine, front, h, w, threshold, flip, fallback_quad, out,
                             offsetof(cv_image_result_t, squares), stream);
    });
}

// ---- JPEG decode: host entropy stage (jpeg.cpp), device reconstruction (jpeg.hip) ------------------------------------------
int cv_jpeg_info(const uint8_t* bytes, size_t len, cv_jpeg_info_t* info) {
    return guarded("cv_jpeg_info", [&]() -> Status {
        if (!bytes || !info) return fail(CV_ERR_INVALID, "cv_jpeg_info: null argument");
        cvjpeg::parse_info(bytes, len, reinterpret_cast<cvjpeg::Info*>(info));
        return Status();
    });
}

int cv_jpeg_entropy_decode(const uint8_t* bytes, size_t len, int16_t* coeffs, size_t capacity, uint16_t* qtables) {
    return guarded("cv_jpeg_entropy_decode", [&]() -> Status {
        if (!bytes || !coeffs || !qtables) return fail(CV_ERR_INVALID, "cv_jpeg_entropy_decode: null argument");
        char why[200];
        if (cvjpeg::entropy_decode(bytes, len, coeffs, capacity, qtables, nullptr, why, sizeof why) != cvjpeg::kOk)
            return fail(CV_ERR_INVALID, std::string("cv_jpeg_entropy_decode: ") + why);
        return Status();
    });
}

int cv_jpeg_reconstruct_u8(cv_engine_t* eng, const int16_t* coeffs, const uint16_t* qtables, int n, const cv_jpeg_info_t* info,
                           int channel_order, uint8_t* planes, size_t planes_bytes, uint8_t* dst, void* stream) {
    return guarded("cv_jpeg_reconstruct_u8", [&]() -> Status {
        return jpeg_reconstruct_entry("cv_jpeg_reconstruct_u8", eng, coeffs, qtables, n, info, channel_order, 0, planes, planes_bytes, dst, stream);
    });
}

int cv_jpeg_reconstruct_oriented_u8(cv_engine_t* eng, const int16_t* coeffs, const uint16_t* qtables, int n, const cv_jpeg_info_t* info,
                                    int channel_order, int orientation, uint8_t* planes, size_t planes_bytes, uint8_t* dst, void* stream) {
    return guarded("cv_jpeg_reconstruct_oriented_u8", [&]() -> Status {
        return jpeg_reconstruct_entry("cv_jpeg_reconstruct_oriented_u8", eng, coeffs, qtables, n, info, channel_order, orientation, planes,
                                      planes_bytes, dst, stream);
    });
}

int cv_process_jpeg(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* bytes, size_t len, float threshold, int flip,
                    int fallback_quad, cv_image_result_t* out, size_t out_size, void* stream) {
    return guarded("cv_process_jpeg", [&]() -> Status {
        return process_jpeg_entry("cv_process_jpeg", unet_engine, classifier_engine, bytes, len, threshold, flip, fallback_quad, 0, out, out_size,
                                  stream);
    });
}

int cv_process_jpeg_oriented(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* bytes, size_t len, float threshold,
                             int flip, int fallback_quad, int apply_orientation, cv_image_result_t* out, size_t out_size, void* stream) {
    return guarded("cv_process_jpeg_oriented", [&]() -> Status {
        return process_jpeg_entry("cv_process_jpeg_oriented", unet_engine, classifier_engine, bytes, len, threshold, flip, fallback_quad,
                                  apply_orientation, out, out_size, stream);
    });
}

}  // extern "C"

// ---- JPEG encode: tables and header on the host (jpeg.cpp), everything else on the device (jpeg_enc.hip) ---------------------------
int cv_jpeg_gray_max_bytes(int h, int w, size_t* bytes) {
    return guarded("cv_jpeg_gray_max_bytes", [&]() -> Status {
        if (!bytes || h < 1 || w < 1 || h > kJpegEncMaxSide || w > kJpegEncMaxSide)
            return fail(CV_ERR_INVALID, "cv_jpeg_gray_max_bytes: height and width must be 1..4096");
        *bytes = cvjpeg::gray_max_bytes(w, h);
        return Status();
    });
}

int cv_jpeg_gray_header(int h, int w, int quality, uint8_t* header, uint16_t* qtable) {
    return guarded("cv_jpeg_gray_header", [&]() -> Status {
        cvjpeg::EncTables t;
        if (!header || cvjpeg::encoder_tables(w, h, quality, &t) != cvjpeg::kOk)
            return fail(CV_ERR_INVALID, "cv_jpeg_gray_header: null header or a size outside 1..65535");
        std::memcpy(header, t.header, CV_JPEG_GRAY_HEADER_BYTES);
        if (qtable) cvjpeg::quant_table(quality, qtable);
        return Status();
    });
}

// What the two encode entries share: the engine's scratch has one user at a time ON THE DEVICE, so an encode starts behind the previous
// one, gray or colour, whatever stream that ran on.  `run(scratch, stream)` queues the launches.
template <class Run>
static Status jpeg_encode_on_engine(const char* name, cv_engine_t* eng, size_t need, void* stream, Run run) {
    Engine& E = eng->impl;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard g(E.device);
    std::lock_guard<std::mutex> lk(E.mu);
    hipError_t e = hipSuccess;
    if (!E.jpeg_enc_done) e = hipEventCreateWithFlags(&E.jpeg_enc_done, hipEventDisableTiming);
    else e = hipStreamWaitEvent(st, E.jpeg_enc_done, 0);
    if (e != hipSuccess) return hip_fail(e, name);
    if (E.jpeg_enc_scratch.bytes < need) {                       // grown for a larger geometry only: the previous encode must have left it
        e = hipEventSynchronize(E.jpeg_enc_done);
        if (e != hipSuccess) return hip_fail(e, name);
        CV_TRY(E.jpeg_enc_scratch.alloc(need, false));
    }
    e = run(E.jpeg_enc_scratch.ptr, st);
    if (e == hipSuccess) e = hipEventRecord(E.jpeg_enc_done, st);
    if (e != hipSuccess) return hip_fail(e, name);
    return Status();
}

int cv_jpeg_encode_gray_u8(cv_engine_t* eng, const uint8_t* src, int n, int h, int w, int quality, uint8_t* out, size_t out_capacity,
                           int64_t* offsets, int32_t* lengths, void* stream) {
    return guarded("cv_jpeg_encode_gray_u8", [&]() -> Status {
        CV_TRY(check_engine(eng));
        if (!src || !out || !offsets || !lengths || n < 1) return fail(CV_ERR_INVALID, "cv_jpeg_encode_gray_u8: bad argument");
        if (h < 1 || w < 1 || h > kJpegEncMaxSide || w > kJpegEncMaxSide)
            return fail(CV_ERR_INVALID, "cv_jpeg_encode_gray_u8: height and width must be 1..4096");
        const size_t each = cvjpeg::gray_max_bytes(w, h);
        if (out_capacity / each < (size_t)n) return fail(CV_ERR_INVALID, "cv_jpeg_encode_gray_u8: out holds less than n x cv_jpeg_gray_max_bytes");
        cvjpeg::EncTables tables;
        if (cvjpeg::encoder_tables(w, h, quality, &tables) != cvjpeg::kOk) return fail(CV_ERR_INVALID, "cv_jpeg_encode_gray_u8: bad size");
        return jpeg_encode_on_engine("cv_jpeg_encode_gray_u8", eng, jpeg_encode_scratch_bytes(n, h, w), stream, [&](void* scratch, hipStream_t st) {
            return jpeg_encode_gray_u8(src, n, h, w, tables, scratch, out, offsets, lengths, st);
        });
    });
}

// luma's sampling factors of a CV_JPEG_SUB_* value; false for any other
static bool jpeg_subsampling(int subsampling, int* hs, int* vs) {
    *hs = subsampling == CV_JPEG_SUB_444 ? 1 : 2;
    *vs = subsampling == CV_JPEG_SUB_420 ? 2 : 1;
    return subsampling == CV_JPEG_SUB_444 || subsampling == CV_JPEG_SUB_422 || subsampling == CV_JPEG_SUB_420;
}

int cv_jpeg_colour_max_bytes(int h, int w, int subsampling, size_t* bytes) {
    return guarded("cv_jpeg_colour_max_bytes", [&]() -> Status {
        int hs, vs;
        if (!bytes || h < 1 || w < 1 || h > kJpegEncMaxSide || w > kJpegEncMaxSide)
            return fail(CV_ERR_INVALID, "cv_jpeg_colour_max_bytes: height and width must be 1..4096");
        if (!jpeg_subsampling(subsampling, &hs, &vs)) return fail(CV_ERR_INVALID, "cv_jpeg_colour_max_bytes: subsampling must be CV_JPEG_SUB_444 / 422 / 420");
        *bytes = cvjpeg::colour_max_bytes(w, h, hs, vs);
        return Status();
    });
}

int cv_jpeg_colour_header(int h, int w, int quality, int subsampling, uint8_t* header, uint16_t* qtables) {
    return guarded("cv_jpeg_colour_header", [&]() -> Status {
        int hs, vs;
        cvjpeg::ScanTables t;
        if (!jpeg_subsampling(subsampling, &hs, &vs)) return fail(CV_ERR_INVALID, "cv_jpeg_colour_header: subsampling must be CV_JPEG_SUB_444 / 422 / 420");
        if (!header || cvjpeg::colour_encoder_tables(w, h, quality, hs, vs, &t) != cvjpeg::kOk)
            return fail(CV_ERR_INVALID, "cv_jpeg_colour_header: null header or a size outside 1..65535");
        std::memcpy(header, t.header, CV_JPEG_COLOUR_HEADER_BYTES);
        if (qtables) {
            cvjpeg::quant_table(quality, qtables);
            cvjpeg::chroma_quant_table(quality, qtables + 64);
        }
        return Status();
    });
}

int cv_jpeg_encode_colour_u8(cv_engine_t* eng, const uint8_t* src, int n, int h, int w, int channel_order, int subsampling, int quality,
                             uint8_t* out, size_t out_capacity, int64_t* offsets, int32_t* lengths, void* stream) {
    return guarded("cv_jpeg_encode_colour_u8", [&]() -> Status {
        CV_TRY(check_engine(eng));
        int hs, vs;
        if (!src || !out || !offsets || !lengths || n < 1) return fail(CV_ERR_INVALID, "cv_jpeg_encode_colour_u8: bad argument");
        if (h < 1 || w < 1 || h > kJpegEncMaxSide || w > kJpegEncMaxSide)
            return fail(CV_ERR_INVALID, "cv_jpeg_encode_colour_u8: height and width must be 1..4096");
        if (channel_order != CV_JPEG_BGR && channel_order != CV_JPEG_RGB)
            return fail(CV_ERR_INVALID, "cv_jpeg_encode_colour_u8: channel_order must be CV_JPEG_BGR or CV_JPEG_RGB");
        if (!jpeg_subsampling(subsampling, &hs, &vs))
            return fail(CV_ERR_INVALID, "cv_jpeg_encode_colour_u8: subsampling must be CV_JPEG_SUB_444 / 422 / 420");
        const size_t each = cvjpeg::colour_max_bytes(w, h, hs, vs);
        if (out_capacity / each < (size_t)n) return fail(CV_ERR_INVALID, "cv_jpeg_encode_colour_u8: out holds less than n x cv_jpeg_colour_max_bytes");
        cvjpeg::ScanTables tables;
        if (cvjpeg::colour_encoder_tables(w, h, quality, hs, vs, &tables) != cvjpeg::kOk) return fail(CV_ERR_INVALID, "cv_jpeg_encode_colour_u8: bad size");
        const int r_at = channel_order == CV_JPEG_RGB ? 0 : 2;
        return jpeg_encode_on_engine("cv_jpeg_encode_colour_u8", eng, jpeg_encode_colour_scratch_bytes(n, h, w, hs, vs), stream,
                                     [&](void* scratch, hipStream_t st) {
                                         return jpeg_encode_colour_u8(src, n, h, w, r_at, hs, vs, tables, scratch, out, offsets, lengths, st);
                                     });
    });
}

// ---- embedding neighbours (neighbours.hip) ----------------------------------------------------------------------------------------
static bool neighbours_in_limits(int q, int n, int c, int k) {
    return q >= 1 && q <= kNeighbourMaxRows && n >= 1 && n <= kNeighbourMaxRows && c >= 1 && c <= kNeighbourMaxC && k >= 1 && k <= kNeighbourMaxK;
}

size_t cv_embedding_neighbours_scratch_bytes(int q, int n, int c, int k) {
    return neighbours_in_limits(q, n, c, k) ? neighbour_plan(q, n, c, k).bytes : 0;
}

int cv_embedding_neighbours(cv_engine_t* eng, const float* queries, int q, const float* corpus, int n, int c, int k, int flags,
                            int32_t* indices, double* sq_distances, cv_neighbour_stats_t* stats, void* scratch, size_t scratch_bytes,
                            void* stream) {
    return guarded("cv_embedding_neighbours", [&]() -> Status {
        CV_TRY(check_engine(eng));
        const std::string me = "cv_embedding_neighbours: ";
        if (k < 1 || k > kNeighbourMaxK) return fail(CV_ERR_INVALID, me + "k must be in [1, 64], got " + std::to_string(k));
        if (c < 1 || c > kNeighbourMaxC) return fail(CV_ERR_INVALID, me + "c must be in [1, 4096], got " + std::to_string(c));
        if (q < 1 || q > kNeighbourMaxRows) return fail(CV_ERR_INVALID, me + "q must be in [1, 2^22], got " + std::to_string(q));
        if (n < 1 || n > kNeighbourMaxRows) return fail(CV_ERR_INVALID, me + "n must be in [1, 2^22], got " + std::to_string(n));
        if (flags & ~(CV_NEIGHBOURS_EXCLUDE_SELF | CV_NEIGHBOURS_EXACT_ONLY)) return fail(CV_ERR_INVALID, me + "flags holds an unknown bit");
        if ((flags & CV_NEIGHBOURS_EXCLUDE_SELF) && q != n) return fail(CV_ERR_INVALID, me + "flags: exclude-self needs q == n");
        if (!queries || ((uintptr_t)queries & 3u)) return fail(CV_ERR_INVALID, me + "queries must be a 4-byte aligned device pointer");
        if (!corpus || ((uintptr_t)corpus & 3u)) return fail(CV_ERR_INVALID, me + "corpus must be a 4-byte aligned device pointer");
        if (!indices || ((uintptr_t)indices & 3u)) return fail(CV_ERR_INVALID, me + "indices must be a 4-byte aligned device pointer");
        if (!sq_distances || ((uintptr_t)sq_distances & 7u)) return fail(CV_ERR_INVALID, me + "sq_distances must be an 8-byte aligned device pointer");
        if ((uintptr_t)stats & 3u) return fail(CV_ERR_INVALID, me + "stats must be 4-byte aligned");
        const size_t need = neighbour_plan(q, n, c, k).bytes;
        if (!scratch || ((uintptr_t)scratch & 15u)) return fail(CV_ERR_INVALID, me + "scratch must be a 16-byte aligned device pointer");
        if (scratch_bytes < need)
            return fail(CV_ERR_INVALID, me + "scratch_bytes is " + std::to_string(scratch_bytes) + ", " + std::to_string(need) + " needed");
        DeviceGuard g(eng->impl.device);
        hipError_t e = embedding_neighbours(queries, q, corpus, n, c, k, flags, indices, sq_distances, reinterpret_cast<NeighbourStats*>(stats),
                                            scratch, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "embedding_neighbours");
        return Status();
    });
}

// ---- embedding reduction: PaCMAP (pacmap.hip) ---------------------------------------------------------------------------------------
static Status pacmap_limits(const std::string& me, int n, int c, int n_neighbors, int n_mn, int n_fp) {
    if (n_neighbors < 1 || n_neighbors > kPacmapMaxNeighbours)
        return fail(CV_ERR_INVALID, me + "n_neighbors must be in [1, 32], got " + std::to_string(n_neighbors));
    if (n_mn < 0 || n_mn > kPacmapMaxMidNear) return fail(CV_ERR_INVALID, me + "n_mn must be in [0, 16], got " + std::to_string(n_mn));
    if (n_fp < 0 || n_fp > kPacmapMaxFurther) return fail(CV_ERR_INVALID, me + "n_fp must be in [0, 64], got " + std::to_string(n_fp));
    if (c < 1 || c > kNeighbourMaxC) return fail(CV_ERR_INVALID, me + "c must be in [1, 4096], got " + std::to_string(c));
    if (!pacmap_in_limits(n, c, n_neighbors, n_mn, n_fp))
        return fail(CV_ERR_INVALID, me + "n must be at least max(7, 6 + n_mn, n_neighbors + n_fp + 1) and at most 2^22, with 2 n (n_neighbors + "
                                         "n_mn + n_fp) below 2^31, got " + std::to_string(n));
    return Status();
}

int cv_pacmap_plan(int n, int c, int n_neighbors, int n_mn, int n_fp, cv_pacmap_plan_t* plan) {
    return guarded("cv_pacmap_plan", [&]() -> Status {
        if (!plan) return fail(CV_ERR_INVALID, "cv_pacmap_plan: plan is null");
        CV_TRY(pacmap_limits("cv_pacmap_plan: ", n, c, n_neighbors, n_mn, n_fp));
        const PacmapPlan p = pacmap_plan(n, c, n_neighbors, n_mn, n_fp);
        *plan = cv_pacmap_plan_t{n, c, n_neighbors, n_mn, n_fp, p.kc, (uint64_t)p.pairs_bytes, (uint64_t)p.optimise_bytes};
        return Status();
    });
}

int cv_pacmap_pairs(cv_engine_t* eng, const float* pre, int n, int c, int n_neighbors, int n_mn, int n_fp, uint64_t seed,
                    int32_t* neighbours, int32_t* mid_near, int32_t* further, cv_pacmap_stats_t* stats, void* scratch,
                    size_t scratch_bytes, void* stream) {
    return guarded("cv_pacmap_pairs", [&]() -> Status {
        CV_TRY(check_engine(eng));
        const std::string me = "cv_pacmap_pairs: ";
        CV_TRY(pacmap_limits(me, n, c, n_neighbors, n_mn, n_fp));
        if (!pre || ((uintptr_t)pre & 3u)) return fail(CV_ERR_INVALID, me + "pre must be a 4-byte aligned device pointer");
        if (!neighbours || ((uintptr_t)neighbours & 3u)) return fail(CV_ERR_INVALID, me + "neighbours must be a 4-byte aligned device pointer");
        if ((n_mn && !mid_near) || ((uintptr_t)mid_near & 3u)) return fail(CV_ERR_INVALID, me + "mid_near must be a 4-byte aligned device pointer");
        if ((n_fp && !further) || ((uintptr_t)further & 3u)) return fail(CV_ERR_INVALID, me + "further must be a 4-byte aligned device pointer");
        if ((uintptr_t)stats & 7u) return fail(CV_ERR_INVALID, me + "stats must be 8-byte aligned");
        const size_t need = pacmap_plan(n, c, n_neighbors, n_mn, n_fp).pairs_bytes;
        if (!scratch || ((uintptr_t)scratch & 15u)) return fail(CV_ERR_INVALID, me + "scratch must be a 16-byte aligned device pointer");
        if (scratch_bytes < need)
            return fail(CV_ERR_INVALID, me + "scratch_bytes is " + std::to_string(scratch_bytes) + ", " + std::to_string(need) + " needed");
        DeviceGuard g(eng->impl.device);
        hipError_t e = pacmap_pairs(pre, n, c, n_neighbors, n_mn, n_fp, seed, neighbours, mid_near, further,
                                    reinterpret_cast<PacmapStats*>(stats), scratch, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "pacmap_pairs");
        return Status();
    });
}

int cv_pacmap_optimise(cv_engine_t* eng, const float* init, int n, const int32_t* offsets, const int32_t* entries, int64_t n_entries,
                       int iterations, float* out, void* scratch, size_t scratch_bytes, void* stream) {
    return guarded("cv_pacmap_optimise", [&]() -> Status {
        CV_TRY(check_engine(eng));
        const std::string me = "cv_pacmap_optimise: ";
        if (n < 7 || n > kNeighbourMaxRows) return fail(CV_ERR_INVALID, me + "n must be in [7, 2^22], got " + std::to_string(n));
        if (iterations < 0) return fail(CV_ERR_INVALID, me + "iterations must not be negative, got " + std::to_string(iterations));
        if (n_entries < 1 || n_entries >= (int64_t(1) << 31))
            return fail(CV_ERR_INVALID, me + "n_entries must be in [1, 2^31), got " + std::to_string(n_entries));
        if (!init || ((uintptr_t)init & 7u)) return fail(CV_ERR_INVALID, me + "init must be an 8-byte aligned device pointer");
        if (!out || ((uintptr_t)out & 7u) || out == init) return fail(CV_ERR_INVALID, me + "out must be an 8-byte aligned device pointer other than init");
        if (!offsets || ((uintptr_t)offsets & 3u)) return fail(CV_ERR_INVALID, me + "offsets must be a 4-byte aligned device pointer");
        if (!entries || ((uintptr_t)entries & 3u)) return fail(CV_ERR_INVALID, me + "entries must be a 4-byte aligned device pointer");
        const size_t need = pacmap_plan(n, 1, 1, 0, 0).optimise_bytes;
        if (!scratch || ((uintptr_t)scratch & 15u)) return fail(CV_ERR_INVALID, me + "scratch must be a 16-byte aligned device pointer");
        if (scratch_bytes < need)
            return fail(CV_ERR_INVALID, me + "scratch_bytes is " + std::to_string(scratch_bytes) + ", " + std::to_string(need) + " needed");
        DeviceGuard g(eng->impl.device);
        hipError_t e = pacmap_optimise(init, n, offsets, entries, iterations, out, scratch, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "pacmap_optimise");
        return Status();
    });
}

// ---- placing new rows into a fitted map (pacmap.hip) --------------------------------------------------------------------------------
static Status pacmap_place_limits(const std::string& me, int q, int n, int c, int n_neighbors) {
    if (q < 1 || q > kNeighbourMaxRows) return fail(CV_ERR_INVALID, me + "q must be in [1, 2^22], got " + std::to_string(q));
    if (n_neighbors < 1 || n_neighbors > kPacmapMaxNeighbours)
        return fail(CV_ERR_INVALID, me + "n_neighbors must be in [1, 32], got " + std::to_string(n_neighbors));
    if (c < 1 || c > kNeighbourMaxC) return fail(CV_ERR_INVALID, me + "c must be in [1, 4096], got " + std::to_string(c));
    if (!pacmap_place_in_limits(q, n, c, n_neighbors))
        return fail(CV_ERR_INVALID, me + "n must be at least max(7, n_neighbors + 1) and at most 2^22, got " + std::to_string(n));
    return Status();
}

static Status pacmap_scratch(const std::string& me, const void* scratch, size_t scratch_bytes, size_t need) {
    if (!scratch || ((uintptr_t)scratch & 15u)) return fail(CV_ERR_INVALID, me + "scratch must be a 16-byte aligned device pointer");
    if (scratch_bytes < need)
        return fail(CV_ERR_INVALID, me + "scratch_bytes is " + std::to_string(scratch_bytes) + ", " + std::to_string(need) + " needed");
    return Status();
}

int cv_pacmap_place_plan(int q, int n, int c, int n_neighbors, cv_pacmap_place_plan_t* plan) {
    return guarded("cv_pacmap_place_plan", [&]() -> Status {
        if (!plan) return fail(CV_ERR_INVALID, "cv_pacmap_place_plan: plan is null");
        CV_TRY(pacmap_place_limits("cv_pacmap_place_plan: ", q, n, c, n_neighbors));
        const PacmapPlacePlan p = pacmap_place_plan(q, n, c, n_neighbors);
        *plan = cv_pacmap_place_plan_t{q, n, c, n_neighbors, p.kc, 0, (uint64_t)p.scale_bytes, (uint64_t)p.pairs_bytes};
        return Status();
    });
}

int cv_pacmap_basis_scale(cv_engine_t* eng, const float* pre, int n, int c, int n_neighbors, double* sigma, void* scratch,
                          size_t scratch_bytes, void* stream) {
    return guarded("cv_pacmap_basis_scale", [&]() -> Status {
        CV_TRY(check_engine(eng));
        const std::string me = "cv_pacmap_basis_scale: ";
        CV_TRY(pacmap_place_limits(me, 1, n, c, n_neighbors));
        if (!pre || ((uintptr_t)pre & 3u)) return fail(CV_ERR_INVALID, me + "pre must be a 4-byte aligned device pointer");
        if (!sigma || ((uintptr_t)sigma & 7u)) return fail(CV_ERR_INVALID, me + "sigma must be an 8-byte aligned device pointer");
        CV_TRY(pacmap_scratch(me, scratch, scratch_bytes, pacmap_place_plan(1, n, c, n_neighbors).scale_bytes));
        DeviceGuard g(eng->impl.device);
        hipError_t e = pacmap_basis_scale(pre, n, c, n_neighbors, sigma, scratch, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "pacmap_basis_scale");
        return Status();
    });
}

int cv_pacmap_place_pairs(cv_engine_t* eng, const float* pre_new, int q, const float* pre, int n, int c, int n_neighbors,
                          const double* sigma, int32_t* neighbours, cv_neighbour_stats_t* stats, void* scratch, size_t scratch_bytes,
                          void* stream) {
    return guarded("cv_pacmap_place_pairs", [&]() -> Status {
        CV_TRY(check_engine(eng));
        const std::string me = "cv_pacmap_place_pairs: ";
        CV_TRY(pacmap_place_limits(me, q, n, c, n_neighbors));
        if (!pre_new || ((uintptr_t)pre_new & 3u)) return fail(CV_ERR_INVALID, me + "pre_new must be a 4-byte aligned device pointer");
        if (!pre || ((uintptr_t)pre & 3u)) return fail(CV_ERR_INVALID, me + "pre must be a 4-byte aligned device pointer");
        if (!sigma || ((uintptr_t)sigma & 7u)) return fail(CV_ERR_INVALID, me + "sigma must be an 8-byte aligned device pointer");
        if (!neighbours || ((uintptr_t)neighbours & 3u)) return fail(CV_ERR_INVALID, me + "neighbours must be a 4-byte aligned device pointer");
        if ((uintptr_t)stats & 3u) return fail(CV_ERR_INVALID, me + "stats must be 4-byte aligned");
        CV_TRY(pacmap_scratch(me, scratch, scratch_bytes, pacmap_place_plan(q, n, c, n_neighbors).pairs_bytes));
        DeviceGuard g(eng->impl.device);
        hipError_t e = pacmap_place_pairs(pre_new, q, pre, n, c, n_neighbors, sigma, neighbours, reinterpret_cast<NeighbourStats*>(stats),
                                          scratch, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "pacmap_place_pairs");
        return Status();
    });
}

int cv_pacmap_place(cv_engine_t* eng, const float* init, int q, const float* basis, int n, const int32_t* neighbours, int n_neighbors,
                    int iterations, float* out, void* stream) {
    return guarded("cv_pacmap_place", [&]() -> Status {
        CV_TRY(check_engine(eng));
        const std::string me = "cv_pacmap_place: ";
        if (q < 1 || q > kNeighbourMaxRows) return fail(CV_ERR_INVALID, me + "q must be in [1, 2^22], got " + std::to_string(q));
        if (n < 1 || n > kNeighbourMaxRows) return fail(CV_ERR_INVALID, me + "n must be in [1, 2^22], got " + std::to_string(n));
        if (n_neighbors < 1 || n_neighbors > kPacmapMaxNeighbours)
            return fail(CV_ERR_INVALID, me + "n_neighbors must be in [1, 32], got " + std::to_string(n_neighbors));
        if (iterations < 0) return fail(CV_ERR_INVALID, me + "iterations must not be negative, got " + std::to_string(iterations));
        if (!init || ((uintptr_t)init & 7u)) return fail(CV_ERR_INVALID, me + "init must be an 8-byte aligned device pointer");
        if (!basis || ((uintptr_t)basis & 7u)) return fail(CV_ERR_INVALID, me + "basis must be an 8-byte aligned device pointer");
        if (!out || ((uintptr_t)out & 7u) || out == init) return fail(CV_ERR_INVALID, me + "out must be an 8-byte aligned device pointer other than init");
        if (!neighbours || ((uintptr_t)neighbours & 3u)) return fail(CV_ERR_INVALID, me + "neighbours must be a 4-byte aligned device pointer");
        DeviceGuard g(eng->impl.device);
        hipError_t e = pacmap_place(init, q, basis, n, neighbours, n_neighbors, iterations, out, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "pacmap_place");
        return Status();
    });
}

// ---- the JPEG decoder's two halves are part of this translation unit -------------------------------------------------------
// The library's list of units is fixed (every build of it, the host-only sanitizer builds included, compiles and links exactly
// that list).  jpeg.cpp stays a plain C++17 file that g++ compiles on its own; jpeg.hip holds the two kernels and their launch wrapper.
#include "jpeg.cpp"
#include "jpeg.hip"
#include "jpeg_enc.hip"
#include "neighbours.hip"
#include "pacmap.hip"
