/*
 * chessvision_hip.h -- C ABI of libchessvision_hip.so
 *
 * MI355X (gfx950 / CDNA4) implementation of the ChessVision CNN inference hot path:
 *   - UNet(3 -> 1) 256x256 board-segmentation forward
 *   - ResNet-18 (1 channel in, 13 classes) 64x64 square-classifier forward
 *
 * The reference (gudbrandtandberg/ChessVision-3LC) is pure Python and has no FFI of its own; the seam
 * this library sits behind is the reference's "callable model object" boundary:
 *     chessvision/core.py:220   logits = self.board_extractor(image_batch)      -> cv_unet_forward
 *     chessvision/core.py:241   predictions = self.classifier(batch)            -> cv_resnet18_forward
 *     chessvision/core.py:84-106, utils.py:42-86  model construction + checkpoint load
 *                                                                               -> cv_engine_create,
 *                                                                                  cv_load_unet, cv_load_resnet18
 *     chessvision/core.py:215-216 (u8 HWC /255 -> NCHW), core.py:273 + utils.py:101-112 (sigmoid,
 *     threshold -> 0/255 mask)                                                  -> cv_unet_forward_u8
 *     chessvision/core.py:236-237 (/=255), core.py:242 (softmax dim=1)          -> cv_resnet18_forward_u8
 * The ctypes binding a maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns CV_OK (0) or a CV_ERR_* code; cv_last_error() returns a thread-local,
 *     NUL-terminated description of the most recent failure on the calling thread.  Nothing aborts and no C++
 *     exception crosses the boundary (host allocation failures come back as CV_ERR_NOMEM).
 *   - all tensor arguments of the *_forward* functions are DEVICE pointers on the engine's device;
 *     `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous
 *     with respect to the host and ordered on `stream`.
 *   - the caller owns inputs and outputs; the engine owns its packed weights and its workspace and
 *     releases them in cv_engine_destroy.  The library never frees caller memory.
 *   - an engine serialises concurrent forward calls with an internal mutex (one workspace per engine and model).  Forwards of the
 *     SAME model may be enqueued on different streams: when the stream of a model's forward differs from that of its previous
 *     forward, the call first waits (on the host) for the previous stream, so the two never overlap on the shared workspace
 *     (rounds 1-5 left this to the caller; a soak in round 6 showed the library's own host layer getting it wrong).  Keep one
 *     stream per engine and the wait never happens.  A UNet forward and a ResNet-18 forward of one engine may run on two streams
 *     at once (separate workspaces and scratch).
 *   - a server that runs several engines side by side (one per request thread, each on its own stream) should send ONE warm-up
 *     request through each of them, one after the other, before the threads start: the HIP runtime binds a stream to a hardware
 *     queue at the stream's first use, and streams first used at the same moment end up sharing queues (measured on MI355X, round 6:
 *     four engine pairs 1850-1880 requests/s when first used together, 2340-2370 when first used in turn).  The Python host layer
 *     does this for its request slots (ChessVision._warm_slot).
 *   - engines of one process may be created, loaded, used and destroyed from different threads at the same time: loads are
 *     serialized process-wide, and memory released by cv_engine_destroy is cached for the next engine (cv_trim_memory).
 *   - plain C types only: no torch / C++ types cross this boundary.
 */
#ifndef CHESSVISION_HIP_H
#define CHESSVISION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CV_ABI_VERSION 6      /* 2: CV_PREC_F16R, CV_ERR_NUMERIC + cv_engine_numeric_status, cv_engine_set_chunk before cv_load_* only
                                 3: cv_board_homographies, cv_engine_export/import_calibration, cv_process_image (additions only)
                                 4: cv_find_contours (addition); cv_find_quadrangle follows CHAIN_APPROX_TC89_KCOS
                                 5: cv_image_result_t gains `squares` (appended; zero the struct before use, as before)
                                 6: cv_process_image_v2 (the caller states sizeof(cv_image_result_t) as IT was compiled); cv_process_image is
                                    the ABI 3 / 4 entry point again and never touches `squares` -- a binary built against the shorter struct
                                    of those versions is safe once more
                                 6 (addition, no version change): cv_load_resnet (timm "resnet18" | "resnet34"); consumers that need it
                                    detect it with dlsym(handle, "cv_load_resnet") -- a library without the symbol loads ResNet-18 only */

enum cv_status {
    CV_OK = 0,
    CV_ERR_INVALID = 1,   /* bad argument / shape / missing or mis-shaped parameter            */
    CV_ERR_HIP = 2,       /* a HIP runtime call failed (message carries hipGetErrorString)     */
    CV_ERR_STATE = 3,     /* model not loaded, wrong device, ...                               */
    CV_ERR_NOMEM = 4,
    CV_ERR_NUMERIC = 5    /* a layer produced a non-finite value (f16 range exceeded / NaN input): results invalid */
};

/* arithmetic type of the convolution path */
enum cv_precision {
    CV_PREC_F32 = 0,      /* f32 activations/weights, f32-input MFMA (exact f32 products, f32 accumulate) */
    CV_PREC_F16 = 1,      /* f16 activations/weights, f16 MFMA with f32 accumulate, f32 BN/bias epilogue  */
    CV_PREC_F16X3 = 2,    /* split-f16: every activation/weight carried as hi + lo f16 (>= 22 significant bits),
                             products formed as hi*hi + hi*lo + lo*hi on the f16 MFMA with f32 accumulate:
                             f32-grade results at up to 1/3 of the f16 MFMA rate (5.3x the f32 MFMA rate) */
    CV_PREC_F16R = 3      /* f16 with an f32 residual trunk (the classifier's fp16 mode, BASELINE configs[2]): f16
                             activations/weights and ONE f16 MFMA product per MAC, f32 accumulate, as CV_PREC_F16 -- but
                             the ResNet-18 stem is computed at f32 grade and every tensor of the residual trunk (pooled stem
                             output, block outputs, down-sampled shortcuts) keeps an unrounded f32 twin that the residual
                             adds read and the block epilogues write, so f16 rounding never accumulates along the
                             skip path; soft-max probabilities within 1e-3 of the fp32 reference.  The UNet (no
                             residuals) runs exactly as under CV_PREC_F16. */
};

typedef struct cv_engine cv_engine_t;     /* opaque */

/* One entry of a PyTorch state dict: name = state-dict key (reference key names, e.g.
 * "inc.double_conv.0.weight", "layer2.0.downsample.1.running_var", "fc.bias"); data = HOST pointer to
 * contiguous row-major float32.  BatchNorm "*.num_batches_tracked" entries may be omitted or passed (any shape):
 * they are ignored. */
typedef struct cv_param {
    const char*  name;
    const float* data;
    int32_t      ndim;
    int64_t      shape[4];
} cv_param_t;

/* ---- library / error ---------------------------------------------------------------------------- */
int         cv_abi_version(void);
const char* cv_last_error(void);
int         cv_device_count(int* count);

/* ---- engine lifecycle ---------------------------------------------------------------------------- */
/* device: HIP device ordinal; precision: enum cv_precision.  Replaces nn.Module.to(device)/.eval()
 * (core.py:105-106,149-150): an engine is always in inference mode. */
int cv_engine_create(int device, int precision, cv_engine_t** out);
int cv_engine_destroy(cv_engine_t* eng);

/* Device and page-locked blocks of a destroyed engine (weights, workspaces, staging) stay in a process-wide cache and are handed to
 * the next engine that asks for a block of that size, so a server that reloads models does not unmap device memory beside the
 * running forwards of its other engines (round 6: that combination ended in device faults).  The cache holds at
 * most CV_MEM_CACHE_MB (environment, default 16384) and CV_MEM_CACHE=0 switches it off.  cv_trim_memory waits for the device and
 * returns every cached block to the driver; *bytes_freed (may be NULL) receives their total size.  The reference has no counterpart:
 * torch's caching allocator plays this role there (torch.cuda.empty_cache()). */
int cv_trim_memory(size_t* bytes_freed);

/* Load + pack weights (host fp32 state dict -> device, BN folded to per-channel scale/shift applied in
 * the conv epilogue).  cv_load_unet auto-detects the transposed-conv vs bilinear variant from the
 * presence of "up1.up.weight" and validates every key/shape, failing with the offending key name.
 * Replaces model.load_state_dict(...) of utils.py:59-79. */
int cv_load_unet(cv_engine_t* eng, const cv_param_t* params, int n_params);
/* The piece classifier: timm's plain BasicBlock ResNet, arch = "resnet18" (blocks per stage {2,2,2,2}) or "resnet34" ({3,4,6,3}),
 * in_chans=1, num_classes=13.  Any other arch fails with CV_ERR_INVALID.  Validation as for the UNet: one missing, extra, renamed or
 * mis-shaped key fails and the message names it.  cv_load_resnet18(e, p, n) is cv_load_resnet(e, "resnet18", p, n).
 * An engine holds one ResNet at a time; cv_resnet18_forward, cv_resnet18_forward_u8, cv_process_image and cv_process_image_v2 run
 * whichever ResNet it holds, and the by-name entry points (cv_get_activation, cv_get_activation_exponent, cv_model_macs,
 * cv_profile_convs, cv_engine_export/import_calibration) take the loaded architecture's name -- the other ResNet name fails with
 * CV_ERR_STATE naming what is loaded. */
int cv_load_resnet(cv_engine_t* eng, const char* arch, const cv_param_t* params, int n_params);
int cv_load_resnet18(cv_engine_t* eng, const cv_param_t* params, int n_params);
/* The piece classifier as ultralytics' YOLOv8-cls: arch = "yolov8n-cls" | "yolov8s-cls" | "yolov8m-cls" | "yolov8l-cls" | "yolov8x-cls"
 * (any other fails with CV_ERR_INVALID and the message lists the five), 13 classes.  Keys are those of YOLO(path).model.state_dict():
 * model.0.conv.weight, model.0.bn.{weight,bias,running_mean,running_var}, model.2.cv1.conv.weight, model.2.m.0.cv1.conv.weight, ...,
 * model.9.conv.conv.weight, model.9.linear.{weight,bias}; BatchNorm eps is 1e-3.  The stem weight may have three input channels (summed
 * into one at load: the reference feeds the grey square three times) or one.  The form model.fuse() leaves (X.conv.weight + X.conv.bias,
 * no X.bn.*) is accepted too, a dict that mixes the two is refused; validation is as strict as cv_load_resnet's.
 * The classifier slot of an engine holds ONE model, a ResNet or a YOLOv8-cls: a successful load replaces whichever was there.  Every
 * classifier entry (cv_resnet18_forward*, cv_resnet_forward_u8_norm, cv_process_image*, cv_process_jpeg*) runs what the slot holds and
 * the by-name entries take the loaded architecture's name.  Input as the reference passes it: (n, 1, 64, 64) in [0, 1], no resize, no
 * crop; the float entries return logits, the u8 entries the softmax.  The embedding (cv_embedding_dim: 1280) is the pooled
 * model.9.conv output, the linear layer's input.  Precisions: f32, f16x3, f16; CV_PREC_F16R is refused (its f32 trunk is ResNet's). */
int cv_load_yolo_cls(cv_engine_t* eng, const char* arch, const cv_param_t* params, int n_params);

/* Largest number of images (UNet) / squares (ResNet) processed per internal pass; larger batches are
 * looped inside the forward call.  0 = keep default (64 images / 16384 squares).  Must be called before cv_load_*.
 * The activation workspace is elastic: it is sized for the largest batch seen so far (at most one chunk) and grows
 * on demand, so an engine that only ever serves single images (the reference's Flask endpoint,
 * app/computeroot/cv_endpoint.py:131-133) stays well under 1 GB while a throughput job grows once to its chunk. */
int cv_engine_set_chunk(cv_engine_t* eng, int unet_images, int resnet_squares);

/* Bytes of activation workspace currently allocated by the engine (both models). */
int cv_engine_workspace_bytes(cv_engine_t* eng, size_t* bytes);

/* Numeric guard.  The f16-based precisions hold every tensor as value * 2^-exp with a per-tensor exponent calibrated at
 * load time (2^11 head-room over the calibration maximum); a layer that nevertheless produces a non-finite value
 * (range exceeded, NaN/inf in the input) records itself on the device.  This call synchronises `stream`, returns
 * CV_ERR_NUMERIC with the name of the first such layer in cv_last_error() and re-arms the guard; CV_OK when every
 * forward since the previous check was clean.  The forward calls themselves stay asynchronous. */
int cv_engine_numeric_status(cv_engine_t* eng, void* stream);

/* The load-time range calibration as data (f16-based precisions): the per-tensor exponents of a loaded model, two int32 per tensor
 * in the engine's fixed tensor order.  export: exps == NULL returns the count only.  import: sets them (count must match; the
 * layers re-fold their epilogue constants at their next launch; *changed = 1 when any exponent differed).  Multi-GPU jobs
 * broadcast rank 0's vector so that every rank computes with IDENTICAL scalings even if a calibration pass were ever to differ
 * between ranks (chessvision/distributed.py: sync_calibration). */
int cv_engine_export_calibration(cv_engine_t* eng, const char* model, int32_t* exps, int capacity, int* count);
int cv_engine_import_calibration(cv_engine_t* eng, const char* model, const int32_t* exps, int count, int* changed);

/* ---- forward (the hot path) ----------------------------------------------------------------------
 * Reproducibility: a forward is bit-identical run to run, across engines, processes and ranks FOR THE SAME BATCH SHAPE.  The launch
 * plan depends on the batch (tile choice; launches too small to fill the chip split their K loop over several workgroups and sum
 * the f32 partials in a fixed order), so the same image inside a batch of 1 and inside a batch of 64 goes through different f32
 * summation orders: results agree to the f32 rounding of a dot product (logits within ~1e-5 for f16x3 / f32; within the storage
 * rounding, ~5e-3, for the f16 modes), arg-max and FEN agree, bits do not.  cv_process_image (batch 1 / 64 squares) and a job of
 * ChessVision.process_images (64 boards per pass) therefore agree to that tolerance, not bit for bit.  CV_SPLITK=0 in the
 * environment removes the split launches (the largest source of the variation) at the cost of single-image latency. */
/* x: (batch,3,256,256) float32 NCHW in [0,1]  ->  logits: (batch,1,256,256) float32.
 * Same tensor contract as `self.board_extractor(image_batch)` (core.py:220). */
int cv_unet_forward(cv_engine_t* eng, const float* x, int batch, float* logits, void* stream);

/* x: (n,1,64,64) float32 in [0,1]  ->  logits: (n,13) float32 (no softmax).
 * Same tensor contract as `self.classifier(batch)` (core.py:241).  Runs the loaded ResNet (18 or 34, cv_load_resnet). */
int cv_resnet18_forward(cv_engine_t* eng, const float* x, int n, float* logits, void* stream);

/* Fused variants for the batched pipeline (u8 in, pre/post-processing of core.py on device):
 * x_u8: (batch,256,256,3) uint8 HWC, channel order as given (no BGR->RGB swap, core.py:212-216);
 * logits: (batch,1,256,256) float32; mask (nullable): (batch,256,256) uint8 = 255 where
 * sigmoid(logit) > threshold else 0 (core.py:273, utils.py:101-112). */
int cv_unet_forward_u8(cv_engine_t* eng, const uint8_t* x_u8, int batch, float* logits, uint8_t* mask,
                       float threshold, void* stream);
/* squares_u8: (n,64,64) uint8 -> probs: (n,13) float32 = softmax(logits, dim=1) (core.py:236-242).  Runs the loaded ResNet. */
int cv_resnet18_forward_u8(cv_engine_t* eng, const uint8_t* squares_u8, int n, float* probs, void* stream);

/* ---- embeddings at the reference's 3LC hook points -------------------------------------------------------------------------
 * The reference collects embeddings with 3LC's EmbeddingsMetricsCollector at named_modules()[52] of the UNet
 * (down4.maxpool_conv.1.double_conv.5, the bottleneck; train_unet.py:219, process_pipeline.py:328-351) and at named_modules()[90] of
 * the classifier (global_pool; train_classifier.py:32,212).  The collector's default reduction of a hooked (B,C,H,W) output is the mean
 * over H and W, giving (B,C) -- this library's reading of it, DESIGN.md section 4 "Embeddings"; for global_pool the "flatten" alternative
 * is the same vector, for the bottleneck "flatten" needs the whole tensor (cv_get_activation).
 *
 * cv_embedding_dim: channels of `model`'s embedding -- "unet": 1024 (transposed-conv variant) or 512 (bilinear); "resnet18" /
 * "resnet34": 512.  CV_ERR_STATE when the model is not loaded.
 *
 * The four _emb entry points are their namesakes with one more argument: `embedding`, a DEVICE pointer to batch x channels float32
 * (row-major, 16-byte aligned), written by the time `stream` reaches the end of the call.  The channel means are taken inside the
 * forward, once per internal chunk while that chunk's tensor is in the workspace, by one extra launch per chunk (for the classifier on
 * the tensor the head pools: layer4's output, its f32 twin under CV_PREC_F16R); a small forward that replays as a hipGraph replays the
 * pooling with it.  Every other output is bit-identical to the namesake's.  A row's bits do not depend on the batch size or on the
 * image's position in the batch.  embedding == NULL: exactly the namesake -- same launches, same graph. */
int cv_embedding_dim(cv_engine_t* eng, const char* model, int* channels);
int cv_unet_forward_emb(cv_engine_t* eng, const float* x, int batch, float* logits, float* embedding, void* stream);
int cv_unet_forward_u8_emb(cv_engine_t* eng, const uint8_t* x_u8, int batch, float* logits, uint8_t* mask,
                           float threshold, float* embedding, void* stream);
/* The float-input sibling of cv_unet_forward_u8(_emb): x as for cv_unet_forward, mask (nullable) and threshold as for
 * cv_unet_forward_u8, embedding (nullable) as for cv_unet_forward_emb.  Logits and embedding are bit-identical to cv_unet_forward(_emb)'s
 * on the same x. */
int cv_unet_forward_mask(cv_engine_t* eng, const float* x, int batch, float* logits, uint8_t* mask, float threshold,
                         float* embedding, void* stream);
int cv_resnet18_forward_emb(cv_engine_t* eng, const float* x, int n, float* logits, float* embedding, void* stream);
int cv_resnet18_forward_u8_emb(cv_engine_t* eng, const uint8_t* squares_u8, int n, float* probs, float* embedding, void* stream);

/* Channel means of ANY activation cv_get_activation knows (the reference's --embedding_layer option for other layers), for the chunk
 * the last forward left in the workspace: out_dev (DEVICE, 16-byte aligned, capacity_floats >= N*C) receives the (N,C) float32 means
 * over H x W, dims = {N, C}.  Enqueued on `stream` (the stream of that forward, or one ordered behind it): no device-wide
 * synchronisation, no host copy.  out_dev == NULL: shape query.  For a ResNet, "global_pool" names the pooled "layer4".  An unknown tap, a tap a fused launch never writes, or too small a
 * capacity: CV_ERR_INVALID with a message naming the tap. */
int cv_activation_channel_means(cv_engine_t* eng, const char* model, const char* name, float* out_dev, size_t capacity_floats,
                                int64_t dims[2], void* stream);

/* (n,13) logits -> softmax probabilities, in place allowed (core.py:242). */
int cv_softmax13(cv_engine_t* eng, const float* logits, int n, float* probs, void* stream);

/* ---- introspection (tests, bench, profiling) ----------------------------------------------------- */
/* Copy an intermediate activation of the LAST forward chunk out of the workspace as float32 NCHW
 * (n,c,h,w written to dims[4]).  `name` is the producing module's state-dict prefix, e.g.
 * "inc.double_conv.3", "down4.maxpool_conv.1.double_conv.5" (= named_modules()[52],
 * train_unet.py:210), "up1.up", "layer1.0", "maxpool".  out_capacity in floats.  Synchronises.
 * Tensors a fused launch never writes have no tap: under CV_PREC_F16R the ResNet's layer1 runs as ONE chained launch, so
 * "layer1.B.act1" of the chained blocks do not exist and the inner blocks' outputs ("layer1.0", and "layer1.1" for resnet34) are read
 * from their f32 twins (CV_ERR_INVALID naming CV_RESNET_CHAIN=0, the switch that runs layer1 layer by layer and materialises them);
 * every other trunk tensor of that engine ("maxpool", the block outputs, "layerN") is likewise reported from its f32 twin, the tensor
 * the residual adds and the head read -- the f16 copy beside it is the twin rounded once for the next convolution;
 * `model` is "unet" or the loaded ResNet's architecture name ("resnet18" | "resnet34"); the UNet's fused first two convolutions
 * (CV_FUSE_INC=0 to split them) likewise leave "inc.double_conv.2" unwritten at the throughput sizes. */
int cv_get_activation(cv_engine_t* eng, const char* model, const char* name, float* out_host,
                      size_t out_capacity, int64_t dims[4]);

/* Power-of-two exponent the named activation is currently stored with (stored = value * 2^-exponent; 0 for f32). */
int cv_get_activation_exponent(cv_engine_t* eng, const char* model, const char* name, int* exponent);

/* Algorithmic work of one forward: multiply-accumulates per image (UNet) / per square (ResNet). */
int cv_model_macs(cv_engine_t* eng, const char* model, int64_t* macs);

/* Time the conv kernels of one forward with HIP events on `stream` (used by bench.py for the
 * roofline figure): runs the forward `iters` times on resident inputs and returns the summed
 * duration (ms) of all implicit-GEMM conv launches and their count. */
int cv_profile_convs(cv_engine_t* eng, const char* model, const void* x, int batch, void* out, int iters,
                     void* stream, float* conv_ms_total, int* conv_launches, float* all_ms_total);

/* Iterate the per-launch records of the last cv_profile_convs call (index 0 .. until CV_ERR_INVALID):
 * name = producing module, ms = event-timed duration, macs = algorithmic multiply-accumulates.
 * cv_op_conv2d and cv_op_conv_transpose2x2 record their own launch the same way: after either call the records describe
 * that one launch (and nothing else) until the next recorded call replaces them. */
int cv_profile_entry(cv_engine_t* eng, int index, char* name, int name_cap, float* ms, double* macs,
                     int* is_conv);

/* Algorithmic HBM bytes (inputs + outputs + weights, once each, at the engine's storage width) of record `index`. */
int cv_profile_entry_bytes(cv_engine_t* eng, int index, double* bytes);

/* Which kernel instantiation ran record `index` (conv family: "conv3x3_halo_kernel<split_t,64,16x16>", ...; empty for the
 * other kernels, whose record name already is the kernel).  Lets a caller rebuild the per-kernel roofline that
 * rocprofv3 --kernel-trace reports by template name. */
int cv_profile_entry_kernel(cv_engine_t* eng, int index, char* kernel, int kernel_cap);

/* Stand-alone single-layer entry points used by the parity tests (float32 NCHW device tensors in,
 * float32 NCHW out; packing to the internal layout happens inside, on `stream`).
 *   conv:  y = act( scale[c] * conv2d(x, w, stride, pad=(k-1)/2) + shift[c] (+ residual) )
 *          w: HOST (cout,cin,k,k) float32; scale/shift: HOST (cout); residual nullable (device).
 * The two convolution entry points run with the launch recorder on: cv_profile_entry / cv_profile_entry_kernel then name the
 * kernel form the launch planner chose for this shape ("conv_igemm_kernel<half_t,128x128,ring3,POS>", ...), so a test can
 * check that a shape still reaches the form it was written for.  Recording does not change the planner's choice. */
int cv_op_conv2d(cv_engine_t* eng, const float* x, int n, int cin, int h, int w_, const float* w_host,
                 int cout, int k, int stride, const float* scale_host, const float* shift_host,
                 const float* residual, int relu, float* y, void* stream);
/*   conv-transpose k2 s2:  y(n,cout,2h,2w) = convT(x, w) + bias;  w: HOST (cin,cout,2,2) */
/* cv_op_conv2d with the epilogue options and channel slices of the YOLOv8-cls plan.  x: (n, x_channels, h, w) device float32, the layer
 * reads channels [x_coff, x_coff + cin); y: (n, y_channels, ho, wo) device float32, IN and OUT: it is stored as given, the layer writes
 * channels [y_coff, y_coff + cout) and the whole tensor comes back -- channels outside the slice must return unchanged.  act: 0 none |
 * 1 ReLU | 2 SiLU; act_first: activation, then the residual, nothing after (default: residual, then activation).  res_coff >= 0: the
 * residual is channels [res_coff, res_coff + cout) of y as given (stride 1 only); < 0: none.  in_exp / out_exp: the tensors are stored
 * as value * 2^-exp in the f16-based engines (0 in the f32 engine).  Channel counts and offsets are multiples of 8.  The launch is
 * recorded as cv_op_conv2d's is. */
int cv_op_conv2d_act(cv_engine_t* eng, const float* x, int n, int x_channels, int x_coff, int cin, int h, int w_, const float* w_host, int cout,
                     int k, int stride, const float* scale_host, const float* shift_host, int act, int act_first, float* y, int y_channels,
                     int y_coff, int res_coff, int in_exp, int out_exp, void* stream);
/* Which epilogue options a launch form accepts -- the pure predicate its launcher asks before anything else (a refused launch returns
 * an error; no form ever runs an activation it was not asked for).  form 0: implicit-GEMM (plain / position-major / split-K second
 * pass), 1: the pair launch, 2: the halo kernel, 3: its chained launch, 4: the planner (Engine::run_conv).  act: 0 none | 1 ReLU |
 * 2 SiLU; act_first as in cv_op_conv2d_act; with_head / with_pool: a fused 1x1 head / fused pool rides on the epilogue; with_fuse0 /
 * shuffle (form 4 only): the fused first layer / the pixel-shuffle store.  *ok = 1 accepted, 0 refused.  Launches nothing. */
int cv_op_conv_epilogue_ok(int form, int act, int act_first, int with_head, int with_pool, int with_fuse0, int shuffle, int* ok);
/* The YOLOv8-cls stem alone: conv 3x3 s2 p1 (1 -> c0) + affine + SiLU.  x: (n, 64, 64) device float32 or uint8 (x_u8; std > 0: the bytes
 * are normalised ((u8 / 255) - mean) / std); w_host [c0][9], scale_host / shift_host [c0]; y: (n, c0, 32, 32) device float32. */
int cv_op_stem3x3s2(cv_engine_t* eng, const void* x, int x_u8, int n, int c0, const float* w_host, const float* scale_host,
                    const float* shift_host, float mean, float std, int out_exp, float* y, void* stream);
/* The YOLOv8-cls head alone: average pool over h x w + Linear(c -> 13) (+ softmax).  x: (n, c, h, w) device float32; w_host [13][c],
 * bias_host [13]; out: (n, 13) device float32; pooled: (n, c) device float32, 16-byte aligned, or NULL. */
int cv_op_head_pool_fc(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, const float* w_host, const float* bias_host,
                       int softmax, int in_exp, float* out, float* pooled, void* stream);
int cv_op_conv_transpose2x2(cv_engine_t* eng, const float* x, int n, int cin, int h, int w_,
                            const float* w_host, int cout, const float* bias_host, float* y, void* stream);
/*   conv 1x1 c -> 1 + bias: logits (n,1,h,w) float32; mask (nullable, n x h x w uint8) = sigmoid(logit) > threshold ? 255 : 0
 *   (the stand-alone OutConv kernel; the model path fuses it into the last conv's epilogue).  w: HOST (c), bias: HOST (1) */
int cv_op_outc_1x1(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, const float* w_host, const float* bias_host,
                   float threshold, float* logits, uint8_t* mask, void* stream);
int cv_op_maxpool2x2(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, float* y, void* stream);
int cv_op_maxpool3x3s2(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, float* y, void* stream);
int cv_op_upsample_bilinear2x(cv_engine_t* eng, const float* x, int n, int c, int h, int w_, float* y,
                              void* stream);

/* ---- classical stages either side of the CNNs (SURVEY.md section 8f "next" rows) ------------------------------ */
/* Binary mask (h*w uint8, 0 / non-0) -> board quadrangle, host-side C++: contours (outer + holes, RETR_CCOMP order) compressed
 * by CHAIN_APPROX_TC89_KCOS, the reference's area / bounding-box filter when more than one contour, closed-curve
 * Douglas-Peucker at 10 % of the (float-segment) perimeter, first 4-vertex result, reference vertex rotation.  Replaces
 * ChessVision._find_quadrangle (core.py:357-411: cv2.findContours, contourArea, boundingRect, arcLength, approxPolyDP), each in
 * OpenCV's own arithmetic and order.  quad = 4 x (x, y) in mask pixels; *found = 0 when none.  Needs no GPU and no engine. */
int cv_find_quadrangle(const uint8_t* mask, int h, int w, int32_t quad[8], int* found);
/* The same for n masks (n,h,w) on n_threads host threads (0 = hardware concurrency, capped at 32);
 * quads: n x 8 int32, found: n x int32. */
int cv_find_quadrangles(const uint8_t* masks, int n, int h, int w, int32_t* quads, int32_t* found, int n_threads);
/* The contours themselves, as cv2.findContours(mask, RETR_CCOMP, method)[0] lists them (core.py:360): method 0 =
 * CHAIN_APPROX_NONE, 1 = CHAIN_APPROX_TC89_KCOS.  Points of all contours back to back in xy (x, y pairs, room for cap_points
 * points), per contour its point count and a hole flag (room for cap_contours each); *n_contours receives the count.
 * CV_ERR_INVALID when a capacity is too small (h*w contours of 4*h*w points in total always suffice). */
int cv_find_contours(const uint8_t* mask, int h, int w, int method, int32_t* xy, int64_t cap_points, int32_t* counts,
                     int32_t* holes, int64_t cap_contours, int64_t* n_contours);

/* (n,h,w,channels) uint8 -> (n,out_h,out_w,channels) uint8, INTER_AREA semantics (cv2.resize at core.py:212), any channel
 * count and any h, w, out_h, out_w >= 1: exact box mean with round-half-up for integer shrink factors in both directions; any
 * other shrink is OpenCV's ResizeArea_Invoker in float32 (computeResizeAreaTab weights, horizontal pass first, round half to
 * even); enlarging in either direction is OpenCV's 8-bit bilinear resizer with the AREA coefficient rule.  Byte-exact against
 * chessvision/classical.py: resize_area and oracle/classical_ref.py.  DEVICE pointers, no alignment required. */
int cv_resize_area_u8(cv_engine_t* eng, const uint8_t* src, int n, int h, int w, int channels, uint8_t* dst,
                      int out_h, int out_w, void* stream);

/* (n,h,w,channels) uint8 HWC -> (n,channels,out_h,out_w) float32 NCHW in [0,1]: the antialiased bilinear resize the reference's
 * enrichment job puts in front of its UNet (v2.Resize((256,256), antialias=True) on a float image, process_pipeline.py:340-344 =
 * torch.nn.functional.interpolate(u8.float() / 255, size, mode="bilinear", antialias=True, align_corners=False)).  A separable
 * triangle filter with ATen's taps (support max(in/out, 1) per axis, weights normalised), pixel = float(u8) / 255.0f, horizontal pass
 * first, both passes in float32, taps added in ascending order; enlarging is two-tap bilinear, equal sizes are the identity.
 * channels 1..4, taken as given; any h, w >= 1.  DEVICE pointers, dst 4-byte aligned; one launch, asynchronous on `stream` (the tap
 * tables of a new geometry are built on the host and uploaded once).  An image's bits do not depend on the batch around it.  The
 * output is what cv_unet_forward / cv_unet_forward_mask take. */
int cv_resize_antialias_f32(cv_engine_t* eng, const uint8_t* src, int n, int h, int w, int channels, float* dst,
                            int out_h, int out_w, void* stream);

/* Quadrangles -> the matrices of the board warp, host side, in OpenCV's order of operations (utils.extract_perspective,
 * utils.py:115-132: cv2.getPerspectiveTransform(approx, dest) with dest = (0,0), (w,0), (w,h), (0,h); cv2.warpPerspective then
 * inverts the matrix).  quads: n x 4 x (x, y) float32 source-image pixels in the reference's vertex order (TR, TL, BL, BR);
 * forward (nullable): n x 9 doubles, row-major, m[8] = 1; inverse (nullable): n x 9 doubles = cv::invert(forward) = the map from
 * board pixels to source pixels that cv_extract_squares_u8 consumes.  Degenerate quadrangles give all-zero matrices (OpenCV's
 * behaviour: every board pixel then reads source pixel (0,0)).  Needs no GPU and no engine. */
int cv_board_homographies(const float* quads, int n, int out_w, int out_h, double* forward, double* inverse);

/* Per board: perspective warp to 512x512 (bilinear, zero border) + BGR->gray + horizontal flip + split into 64 squares
 * (utils.py:131-132, core.py:298-300, 419-439), fused.  images: DEVICE (n,h,w,3) uint8 BGR; inv_host: HOST n x 9
 * doubles = inverse of the getPerspectiveTransform matrix (board pixel -> source pixel); squares: DEVICE (n*64,64,64)
 * uint8 in a8..h1 order = the input of cv_resnet18_forward_u8; boards (nullable): DEVICE (n,512,512) uint8 gray board.
 * Byte-exact against cv2's fixed-point arithmetic as restated in oracle/classical_ref.py (1/32-pixel coordinates in
 * WarpPerspectiveInvoker's block order, integer bilinear weights, round half up, 15-bit gray).  Output pointers 4-byte aligned.
 * Synchronises `stream` before returning. */
int cv_extract_squares_u8(cv_engine_t* eng, const uint8_t* images, int n, int h, int w, const double* inv_host,
                          uint8_t* squares, uint8_t* boards, void* stream);

/* The same with the n x 9 matrices already on the DEVICE (inv_dev): fully asynchronous, nothing is staged or
 * synchronised -- the form the batched pipeline uses so that consecutive jobs overlap on the stream. */
int cv_extract_squares_u8_dev(cv_engine_t* eng, const uint8_t* images, int n, int h, int w, const double* inv_dev,
                              uint8_t* squares, uint8_t* boards, void* stream);

/* (n_boards,64,13) class probabilities (HOST, classifier order a8..h1, or h1..a8 when flip != 0) -> per board the
 * arg-max labels, the FEN piece placement before and after the reference's only live rule ("no_pawns_on_ends": a pawn on
 * rank 1 or 8 becomes the most probable non-pawn class).  Replaces, for a whole job, process_position_probabilities /
 * validate_position / board_fen (core.py:309-355, 441-469).  fen, original_fen: n_boards x 72 chars (NUL-terminated);
 * labels: n_boards x 64 validated class indices (order of constants.LABEL_NAMES = "BKNPQRbknpqrf"); fixes: capacity
 * n_boards x 16 records of {board, square index, original class, corrected class}; *n_fixes = records written.
 * Needs no GPU and no engine. */
int cv_decode_positions(const float* probs, int n_boards, int flip, char* fen, char* original_fen, int8_t* labels,
                        int32_t* fixes, int32_t* n_fixes);

/* ---- board-extraction quality scores (additions under ABI 6; detect with dlsym(handle, "cv_extraction_scores")) ------------------- */
/* The four floats the reference's enrichment job writes per image beside the FEN (scripts/process_new_raw/process_pipeline.py:287-311,
 * functions at 357-467): `confidence`, `distribution`, `completeness`, `quad_score`.  The first two are reductions over the UNet's
 * output and run on the device, where the logits already are; the other two are host geometry.
 *
 * cv_extraction_scores: values = n images of `count` contiguous float32 (DEVICE, 4-byte aligned; 4 <= count <= 2^24, n >= 1);
 * transform 0 scores the values as given (the reference's letter: it passes BoardExtractionResult.probabilities, which holds raw
 * logits), 1 scores v = 1 / (1 + exp(-x)) with the expression the UNet's mask uses, so `v > 0.5` agrees bit for bit with the mask of
 * cv_unet_forward_u8 at threshold 0.5.  records: n records (DEVICE, 8-byte aligned); half_mask (nullable, DEVICE, n x count uint8) =
 * 255 where v > 0.5 else 0.  Asynchronous on `stream`; allocates nothing and synchronises nothing.  A record is bit-identical run
 * to run (integer counts; the float64 sum runs in a fixed order, no float atomics). */
typedef struct cv_score_record {
    int32_t hist[10];     /* np.histogram(v, bins=10, range=(0, 1)) for a float32 array: float32 edges 0.f, 0.1f, .., 0.9f, 1.f; v is in
                             bin i iff e[i] <= v < e[i+1], v == 1 joins the last bin; NaN, +-inf and everything outside [0, 1] dropped */
    int32_t above_half;   /* number of values with v > 0.5f */
    int32_t n_nan;
    double  top_sum;      /* sum of |v - 0.5| (float32 subtraction, float64 sum) over the top_count largest values, selected exactly:
                             ties at the smallest selected value t contribute (top_count - number of values > t) * |t - 0.5| */
    int32_t top_count;    /* count / 4 */
    int32_t reserved;     /* 0; pads the record to 64 bytes */
} cv_score_record_t;
int cv_extraction_scores(cv_engine_t* eng, const float* values, int n, int count, int transform, cv_score_record_t* records,
                         uint8_t* half_mask, void* stream);
/* Records (HOST) -> the two scores, n doubles each: confidence = 2 * top_sum / top_count = np.mean(np.abs(np.sort(v)[-k:] - 0.5)) * 2
 * (NaN when the image holds a NaN, as numpy's sort puts NaN last); distribution = 1 - H / log2(10) with p = hist / sum(hist) and
 * H = -sum p log2(p + 1e-10) (NaN for an empty histogram, as numpy's 0 / 0).  Needs no GPU and no engine. */
int cv_extraction_scores_finish(const cv_score_record_t* records, int n, double* confidence, double* distribution);
/* Binary mask (h*w uint8, 0 / non-0) -> foreground pixels of the whole mask / pixels of the filled outer border of the 8-connected
 * component with the largest contourArea (cv2.findContours RETR_EXTERNAL, max by contourArea, drawContours thickness -1; ties go to
 * the first contour in OpenCV's order).  `Filled` = the component plus every pixel the image frame cannot reach by 4-connected steps
 * around it -- a restatement of drawContours, not measured against cv2.  0 for an empty mask; can exceed 1.  Host only. */
int cv_mask_completeness(const uint8_t* mask, int h, int w, double* score);
/* The same for n masks (n,h,w) on n_threads host threads (0 = hardware concurrency, capped at 32); scores: n doubles. */
int cv_mask_completenesses(const uint8_t* masks, int n, int h, int w, double* scores, int n_threads);
/* quad: 4 x (x, y) float32 in the order given, or NULL (no quadrangle: score 0).  score = 1 - 0.5 std(sides) / mean(sides)
 * - 0.5 std(angles) / (pi / 2), population standard deviations, in double.  Host only. */
int cv_quadrangle_regularity(const float* quad, double* score);

/* ---- ground-truth scores (additions under ABI 6; detect with dlsym(handle, "cv_segmentation_scores")) -------------------------- */
/* What the reference's evaluation side computes against labels: the LossCollector's per-image `loss` = soft Dice loss + mean
 * BCEWithLogitsLoss (scripts/train/unet_loss_collector.py:19-48), train_unet.py's val_dice (:333-338), and evaluate.py's per-square
 * ranks and top-k hits (scripts/eval/evaluate.py:89-140, 264-360).  The per-pixel reductions run on the device, on the logits where
 * the UNet left them; everything about the 64 x 13 probabilities is host code (they visit the host for the FEN anyway).
 *
 * cv_segmentation_scores: logits = n images of `count` contiguous float32 (DEVICE, 4-byte aligned -- an image need not be 16-byte
 * aligned, `count` need not be a multiple of 4; 1 <= count <= 2^24, n >= 1); labels = n x count uint8 (DEVICE, any alignment), a pixel
 * is "board" iff its byte is non-zero (the reference's masks are 0 / 255 and are divided by 255 before the loss); threshold finite.
 * records: n records (DEVICE, 8-byte aligned).  Asynchronous on `stream`; allocates nothing and synchronises nothing.  A record is
 * bit-identical run to run (integer counts; the float64 sums run in a fixed order, no float atomics).  Logits of +-inf are outside
 * the contract (they give NaN sums where 0 * inf arises); a NaN logit is counted and makes all three sums NaN. */
typedef struct cv_seg_record {
    int32_t n_label;        /* label bytes != 0 */
    int32_t n_pred;         /* pixels with v > threshold, v = 1 / (1 + exp(-x)) in the float32 expression the UNet's mask and
                               cv_extraction_scores' transform 1 use: == count_nonzero(mask of cv_unet_forward_u8) bit for bit */
    int32_t n_both;         /* pixels counted in both */
    int32_t n_nan;          /* NaN logits */
    double  bce_sum;        /* sum of the float32 terms max(x, 0) - x * t + log1pf(expf(-|x|)), t in {0, 1}; float64 sum */
    double  sig_sum;        /* sum of v (float32 values, float64 sum) */
    double  sig_label_sum;  /* sum of v over the label pixels */
    int32_t count;
    int32_t reserved[5];    /* 0; pads the record to 64 bytes */
} cv_seg_record_t;
int cv_segmentation_scores(cv_engine_t* eng, const float* logits, const uint8_t* labels, int n, int count, float threshold,
                           cv_seg_record_t* records, void* stream);
/* Records (HOST) -> six scores per image, n doubles each (any output may be NULL).  Needs no GPU and no engine.
 *   bce            = bce_sum / count                                   BCEWithLogitsLoss(reduction="none").mean((-1, -2))
 *   dice_loss      = 1 - (2 * sig_label_sum + 1e-6) / (S + 1e-6),  S = sig_sum + n_label, and S = 2 * sig_label_sum where S == 0
 *   loss           = dice_loss + bce                                    the LossCollector's column
 *   dice           = the same formula on the integer counts (n_both, n_pred + n_label): the per-image val_dice, 1 when both are empty
 *   iou            = n_both / (n_pred + n_label - n_both), 1 when the union is empty
 *   pixel_accuracy = (count - n_pred - n_label + 2 * n_both) / count
 * The Dice form is a READING: the reference calls dice_loss(..., reduction="none") from a vendored Pytorch-UNet submodule whose
 * directory is empty in the reference tree, so it could not be read.  This is upstream Pytorch-UNet's dice_coeff (epsilon 1e-6 in
 * numerator and denominator, the sets_sum == 0 -> 2 * inter rule) applied per image. */
int cv_segmentation_scores_finish(const cv_seg_record_t* records, int n, double* bce, double* dice_loss, double* loss, double* dice,
                                  double* iou, double* pixel_accuracy);
/* Piece-placement field of a FEN (anything after the first space is ignored) -> 64 class indices in a8..h1 order, classes in the
 * order of constants.LABEL_NAMES = "BKNPQRbknpqrf" (12 = empty).  CV_ERR_INVALID with a message for a malformed placement: not 8
 * ranks, a rank not summing to 8, an unknown symbol.  Host only. */
int cv_fen_labels(const char* fen, int8_t* labels);
/* probs: n_boards x 64 x 13 float32 (HOST); labels: n_boards x 64 true class indices (0..12), GIVEN PER ROW OF probs -- the caller
 * maps rows to squares (a8..h1, or h1..a8 for a flipped board).  per_square: n_boards x 64 records; per_board: n_boards records.
 *   predicted   the arg-max as cv_decode_positions computes it (first maximum)
 *   confidence  the largest probability
 *   rank        #{j: p_j > p_t} + #{j > t: p_j == p_t}: the position of the true class t from the top of np.argsort(kind="stable").
 *               The reference's np.argsort uses the default kind, which numpy 2.2 does not keep stable for 13 float32 columns, so
 *               its own order among EQUAL probabilities is undefined; this is the stable reading.  A square holding a NaN has rank 13
 *               (a miss at every k) and is counted in n_nan.
 *   loss        -log((double)p_t); +inf for 0
 *   hits[k-1]   squares of the board with rank < k (top-k accuracy = hits[k-1] / 64); mean_loss: mean of the 64 losses
 * Host only; needs no GPU and no engine. */
typedef struct cv_square_score {
    int32_t predicted;
    int32_t rank;
    float   confidence;
    int32_t reserved;       /* 0 */
    double  loss;
} cv_square_score_t;
typedef struct cv_board_score {
    int32_t hits[13];
    int32_t n_nan;          /* squares holding a NaN */
    double  mean_loss;
} cv_board_score_t;
int cv_classification_scores(const float* probs, const int8_t* labels, int n_boards, cv_square_score_t* per_square,
                             cv_board_score_t* per_board);

/* ---- threshold sweep (additions under ABI 6; detect with dlsym(handle, "cv_threshold_levels")) -------------------------------- */
/* The mask threshold is the inference-side hyperparameter the reference sweeps (scripts/eval/evaluate.py --threshold,
 * scripts/plot_sweep.py).  Nothing in the UNet depends on it: one pass over the logits gives every threshold's mask and counts.
 *
 * cv_threshold_levels: logits = n images of `count` contiguous float32 (DEVICE, 4-byte aligned; 1 <= count <= 2^24, n >= 1); labels =
 * n x count uint8 (DEVICE, any alignment, "board" iff non-zero) or NULL = no labels; thresholds = n_thresholds float32 on the HOST
 * (they are read and checked before the call returns and travel as a kernel argument: 1 <= n_thresholds <= CV_MAX_THRESHOLDS, every
 * value in [0, 1], strictly ascending as float32; CV_ERR_INVALID otherwise); levels = n x count uint8 (DEVICE, any alignment);
 * records = n records (DEVICE, 4-byte aligned).
 *   level = #{k : v > thresholds[k]}, v = 1 / (1 + exp(-x)) in the float32 expression of the UNet's mask.  The thresholds ascend, so
 *   (level > k) * 255 == the mask cv_unet_forward_u8 writes at thresholds[k], byte for byte; a NaN logit gives level 0.
 * Asynchronous on `stream`; allocates nothing and synchronises nothing.  Integer counts only: bit-identical run to run. */
#define CV_MAX_THRESHOLDS 32
typedef struct cv_level_record {            /* 320 bytes */
    int32_t count;
    int32_t n_thresholds;
    int32_t n_nan;                          /* NaN logits */
    int32_t hist[2][CV_MAX_THRESHOLDS + 1]; /* hist[b][l]: pixels at level l whose label byte is zero (b = 0; every pixel when there
                                               are no labels) or non-zero (b = 1).  At thresholds[k]:
                                               n_pred = sum_{l > k} hist[0][l] + hist[1][l], n_both = sum_{l > k} hist[1][l],
                                               n_label = sum_l hist[1][l] */
    int32_t reserved[11];                   /* 0; pads the record to a multiple of 64 bytes */
} cv_level_record_t;
int cv_threshold_levels(cv_engine_t* eng, const float* logits, const uint8_t* labels, int n, int count, const float* thresholds,
                        int n_thresholds, uint8_t* levels, cv_level_record_t* records, void* stream);
/* Records (HOST) -> dice, iou and pixel_accuracy of cv_segmentation_scores_finish for every (image, threshold): n x T doubles each,
 * row i = image i, T = the records' n_thresholds (all equal, CV_ERR_INVALID otherwise); any output may be NULL.  labels_present == 0:
 * the scores are those against an empty label mask.  Needs no GPU and no engine. */
int cv_threshold_levels_finish(const cv_level_record_t* records, int n, int labels_present, double* dice, double* iou,
                               double* pixel_accuracy);

/* ---- square-set evaluation (additions under ABI 6; detect with dlsym(handle, "cv_square_records")) ----------------------------- */
/* The classifier's own batched caller in the reference, scripts/train/train_classifier.py: validate() (:90-111, CrossEntropyLoss and
 * accuracy over a table of labelled 64 x 64 squares) and the tlc.collect_metrics pass (:274-292, batch 512) behind val_transforms
 * (:45-52: ToTensor + Normalize([0.564], [0.246])).  3LC's ClassificationMetricsCollector is not in the reference tree: loss /
 * predicted / confidence / accuracy per sample is this library's READING of it.  Out of scope: crops that are not 64 x 64 gray (PIL's
 * Resize / Grayscale), the training transforms, normalisation inside cv_process_image (the reference does not normalise there).
 *
 * cv_resnet_forward_u8_norm: cv_resnet18_forward_u8 / _emb with the byte normalised in the stem: the pixel enters the first
 * convolution as ((float)u8 / 255.f - mean) / std -- three float32 operations in that order, true divisions -- which is bit for bit
 * torchvision's ToTensor followed by Normalize([mean], [std]); the zero padding of the convolution stays zero (torch pads after the
 * transform).  The result equals cv_resnet18_forward on that float tensor bit for bit.  squares_u8: DEVICE (n,64,64); mean finite,
 * std finite and > 0 (CV_ERR_INVALID otherwise); softmax != 0: `out` receives probabilities instead of logits; embedding: nullable,
 * DEVICE (n,512), 16-byte aligned, as cv_resnet18_forward_emb.  Runs whichever ResNet is loaded, in the engine's chunks; batches up
 * to 512 replay as a captured graph whose key includes mean and std.  The f16-family engines hold the input plane as x * 2^7 in
 * f16: |x| <= 2.30 for the training constants; constants that push |x| beyond ~500 overflow it. */
int cv_resnet_forward_u8_norm(cv_engine_t* eng, const uint8_t* squares_u8, int n, float mean, float std, int softmax, float* out,
                              float* embedding, void* stream);
/* cv_square_records: logits = n rows of 13 float32 (DEVICE, 4-byte aligned), labels = n int8 (DEVICE, nullable = all unlabelled),
 * records = n records (DEVICE, 8-byte aligned), n >= 1.  Everything is float32 with expf / logf, sums in ascending class order.
 * Asynchronous on `stream`; allocates nothing and synchronises nothing; one launch for any n.  A label outside -1..12 cannot be
 * refused without reading device memory: the square is scored as unlabelled, its byte is kept in `label` and flag bit 1 is set
 * (cv_square_records_finish then returns CV_ERR_INVALID).  Logits of +-inf are outside the contract (inf - inf). */
typedef struct cv_square_record {   /* 32 bytes */
    int32_t predicted;   /* first maximum of the 13 logits (scan j = 0..12, `x_j > best`) */
    int32_t rank;        /* #{j: x_j > x_t} + #{j > t: x_j == x_t}, the stable reading documented at cv_classification_scores, on
                            logits; 13 when the row holds a NaN; -1 when unlabelled */
    int32_t label;       /* as given: 0..12, or -1 = unlabelled */
    int32_t flags;       /* bit 0: the row holds a NaN; bit 1: the label byte was outside -1..12 */
    float   confidence;  /* 1 / s, s = sum_j expf(x_j - m) added in ascending j, m = max: the largest soft-max probability */
    float   loss;        /* logf(s) - (x_t - m): CrossEntropyLoss(reduction="none"); NaN when unlabelled or NaN row */
    float   max_logit;   /* m */
    float   logsumexp;   /* m + logf(s) */
} cv_square_record_t;    /* a NaN row: confidence, loss, max_logit and logsumexp are all NaN */
int cv_square_records(cv_engine_t* eng, const float* logits, const int8_t* labels, int n, cv_square_record_t* records, void* stream);
/* Records (HOST) -> the aggregate of validate().  Needs no GPU and no engine.  Only labelled squares count below.
 *   val_loss   validate()'s running_loss / len(loader): the records are cut into consecutive batches of batch_size (the last one
 *              short; batch_size <= 0: one batch), each batch contributes the mean loss of its labelled squares (CrossEntropyLoss's
 *              reduction="mean"; a batch without a labelled square is skipped), val_loss is the mean of those; in float64.  A
 *              labelled NaN row makes it NaN, as it makes torch's.
 *   val_acc    100 * n_correct / n_labelled, n_correct = squares with predicted == label (output.max(1)); NaN rows are misses
 *   hits[k-1]  squares with rank < k;  hits[0] differs from n_correct only where the true class ties for the maximum with a later class
 *   confusion  13 x 13, row = true class, column = predicted;  loss_sum: float64 sum of the losses
 * CV_ERR_INVALID when a record carries flag bit 1 (a label byte outside -1..12). */
typedef struct cv_squares_summary {
    int64_t n, n_labelled, n_correct, n_nan;      /* n_nan: rows holding a NaN, labelled or not */
    int64_t hits[13];
    int64_t confusion[13 * 13];
    double  loss_sum, val_loss, val_acc;           /* NaN when nothing is labelled */
    int64_t n_batches;                             /* batches that held a labelled square */
} cv_squares_summary_t;
int cv_square_records_finish(const cv_square_record_t* records, int n, int batch_size, cv_squares_summary_t* out);

/* ---- embedding neighbours (additions under ABI 6; detect with dlsym(handle, "cv_embedding_neighbours")) ------------------------- */
/* The one thing the embeddings are collected for: the reference reduces the table with run.reduce_embeddings_by_foreign_table_url(...,
 * method="pacmap") (scripts/process_new_raw/process_pipeline.py:351, scripts/train/train_classifier.py:312) so that uploads and squares
 * can be browsed by similarity.  PaCMAP and UMAP both start from the k-nearest-neighbour graph of the table; this is that graph, exact.
 * The PaCMAP reduction built on it is the next section.  Other metrics (normalise the rows for cosine), approximate indices and
 * corpora that do not fit the device are out of scope.
 *
 * Definition, for float32 rows a (query) and b (corpus) of length c:
 *     D(a, b):  s = 0.0 (double);  for ch = 0 .. c-1 ascending:  t = (double)a[ch] - (double)b[ch];  p = t * t;  s = s + p;  return s
 *   the product rounded to double, then the sum rounded to double, never contracted into a fused multiply-add.
 * Order: the result of query row i is the k eligible corpus rows with the smallest (D, j) pairs, ascending -- distance first, corpus
 *   index second: the order of a stable sort of float64 brute force.  sq_distances holds D itself (squared, float64).
 * Eligibility: with flag bit 0 (exclude self; needs q == n) corpus row j == i is dropped BY INDEX, so an exact duplicate stored
 *   elsewhere stays visible at distance 0.0.  A corpus row holding a NaN or an infinity is never returned.  A query row holding one
 *   gets indices -1 and distances NaN.  When fewer than k rows are eligible the remaining slots are index -1, distance +inf.
 * How: a float32 MFMA filter on mean-centred rows keeps k + 16 candidates per row and the smallest approximate distance T it did not
 *   keep; the candidates are re-computed with D and sorted; the row is CERTIFIED when D_k < T - E, E a proven bound on |approximate - D|
 *   (DESIGN.md section 4 "Embedding neighbours") -- then no row outside the candidates can belong to the answer, tie order included.
 *   Every other row is recomputed against the whole corpus with D alone (the exact path; flag bit 1 sends every row there).  Either
 *   way the output is the definition's, bit for bit, and the same run to run.
 *
 * queries: DEVICE (q, c) float32, dense, 4-byte aligned; corpus: DEVICE (n, c) likewise; queries == corpus is allowed.
 * Limits: 1 <= k <= 64, 1 <= c <= 4096, 1 <= q, n <= 1 << 22.  flags: CV_NEIGHBOURS_EXCLUDE_SELF | CV_NEIGHBOURS_EXACT_ONLY.
 * indices: DEVICE (q, k) int32; sq_distances: DEVICE (q, k) double, 8-byte aligned; stats: DEVICE, nullable, 4-byte aligned;
 * scratch: DEVICE, 16-byte aligned, scratch_bytes >= cv_embedding_neighbours_scratch_bytes(q, n, c, k) (0 for arguments outside the
 * limits); the caller owns it and may reuse it once `stream` has passed the call.
 * Asynchronous on `stream`; allocates nothing and synchronises nothing.  CV_ERR_INVALID names the offending argument. */
enum { CV_NEIGHBOURS_EXCLUDE_SELF = 1, CV_NEIGHBOURS_EXACT_ONLY = 2 };
typedef struct cv_neighbour_stats {   /* 32 bytes, written with integer atomics and plain stores */
    int32_t query_rows;               /* q */
    int32_t certified_rows;           /* rows whose filter result was proven exact */
    int32_t exact_rows;               /* rows recomputed against the whole corpus */
    int32_t nonfinite_query_rows;     /* query_rows == certified_rows + exact_rows + nonfinite_query_rows */
    int32_t nonfinite_corpus_rows;
    int32_t reserved[3];              /* 0 */
} cv_neighbour_stats_t;
size_t cv_embedding_neighbours_scratch_bytes(int q, int n, int c, int k);
int cv_embedding_neighbours(cv_engine_t* eng, const float* queries, int q, const float* corpus, int n, int c, int k, int flags,
                            int32_t* indices, double* sq_distances, cv_neighbour_stats_t* stats, void* scratch, size_t scratch_bytes,
                            void* stream);

/* ---- embedding reduction: PaCMAP (additions under ABI 6; detect with dlsym(handle, "cv_pacmap_pairs")) -------------------------- */
/* The call the table is collected for, run.reduce_embeddings_by_foreign_table_url(..., method="pacmap"), as two device entries.  No
 * copy of the pacmap package is here: this is a READING of Wang, Huang, Rudin, Shaposhnik, "Understanding How Dimension Reduction Tools
 * Work" (JMLR 2021) and of the package's defaults, defined in numpy by chessvision/embeddings.py (pacmap_pairs, pacmap_incidence,
 * pacmap_schedule, pacmap_optimise) and derived in DESIGN.md section 4 "Embedding reduction".  Both entries equal that definition
 * exactly: the pairs index for index, the coordinates bit for bit, the same run to run.
 *
 * The host prepares two arrays (embeddings.pacmap_preprocess / pacmap_init, float64 LAPACK work that is an INPUT of the definition):
 *   pre  (n, c) float32, every value finite: the table projected onto its 100 leading principal axes (more than 100 channels) or
 *        scaled to [0, 1] and centred;     init (n, 2) float32: the starting coordinates.
 *
 * cv_pacmap_pairs -> three int32 arrays of partners per point:
 *   neighbours (n, n_neighbors)  the kc = min(n_neighbors + 50, 64, n - 1) exact nearest rows (cv_embedding_neighbours of pre against
 *       itself, exclude-self) re-ranked: sigma_i = max(mean of sqrt(D) at candidate ranks 3, 4, 5 (zero-based), 1e-10) in double, summed
 *       in rank order; row i keeps the n_neighbors candidates with the smallest (D_ij / (sigma_i * sigma_j), j), ascending.
 *   mid_near (n, n_mn)  slot by slot: draw until six distinct indices are held that are neither i nor an earlier mid-near partner of
 *       i; the partner is the SECOND smallest of the six by (D(i, .), j), D as cv_embedding_neighbours defines it.
 *   further (n, n_fp)  draw until n_fp distinct indices are held that are neither i nor in i's neighbour row, in the order drawn.
 *   Draws (all uint64, wrapping):  mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *       x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31).   key = mix(seed ^ mix((stream << 40) | i)), stream 1 for
 *       mid-near and 2 for further;  draw t of point i = ((mix(key + t) >> 32) * n) >> 32, t counting every draw of the point in the
 *       stream from 0, rejected ones included.  A point that reaches 65536 draws in a stream gives up: draw_overflow is set and its
 *       remaining partners are -1 (not reachable by chance inside the limits below).
 * Limits: 1 <= n_neighbors <= 32, 0 <= n_mn <= 16, 0 <= n_fp <= 64, 1 <= c <= 4096, max(7, 6 + n_mn, n_neighbors + n_fp + 1) <= n <=
 *   1 << 22, and 2 n (n_neighbors + n_mn + n_fp) < 2^31.  cv_pacmap_plan checks them and sizes both scratch blocks.
 *
 * cv_pacmap_optimise: `iterations` Adam steps (the package runs 450) over the incidence lists of the pairs, a CSR structure the caller
 *   builds from the three arrays (embeddings.pacmap_incidence; a counting sort): offsets (n + 1) int32, entries (offsets[n]) int32, an
 *   entry being other | kind << 28 (0 neighbour, 1 mid-near, 2 further).  Point p's list, in this order: its own neighbour pairs by
 *   slot, its own mid-near pairs, its own further pairs, then the entries where p is another point's partner, ordered by (kind, source
 *   point, slot).  The ORDER is part of the definition: float32 sums are taken in it.  Per iteration it = 0 .. iterations - 1, all
 *   points reading the previous iteration's Y, float32, every operation rounded once:
 *       g = (0, 0);  for each entry with other point q:   e = Y[p] - Y[q];  d = 1;  d = d + e0*e0;  d = d + e1*e1
 *           neighbour:  t = 10 + d;     w = w_n  * (20    / (t*t));  g = g + w*e
 *           mid-near:   t = 10000 + d;  w = w_MN * (20000 / (t*t));  g = g + w*e      (skipped from iteration 200 on, where w_MN = 0)
 *           further:    t = 1 + d;      w = w_FP * (2     / (t*t));  g = g - w*e
 *       m = m + c1*(g - m);  v = v + c2*(g*g - v);  Y = Y - (lr_t*m) / (sqrt(v) + 1e-7f),   c1 = (float)(1 - 0.9), c2 = (float)(1 - 0.999)
 *   Host scalars, double rounded to float: lr_t = sqrt(1 - b2) / (1 - b1), b1 = 0.9^(it+1) and b2 = 0.999^(it+1) as running products;
 *   it < 100: w_MN = (1 - it/100) * 1000 + (it/100) * 3, w_n = 2; it < 200: w_MN = 3, w_n = 3; then w_MN = 0, w_n = 1; w_FP = 1.
 *   An entry whose point lies outside [0, n) is skipped.  One plain launch per iteration on `stream`.
 *
 * pre, the pair arrays, init, out, offsets, entries, stats, scratch: DEVICE.  init and out 8-byte aligned, out != init; stats nullable,
 * 8-byte aligned; scratch 16-byte aligned, at least plan.pairs_scratch_bytes / plan.optimise_scratch_bytes (the latter depends on n
 * alone); a pair array of zero columns may be NULL.  The caller owns the scratch and may reuse it once `stream` has passed the call.
 * Asynchronous on `stream`; allocate nothing and synchronise nothing.  CV_ERR_INVALID names the offending argument. */
typedef struct cv_pacmap_stats {      /* 64 bytes */
    cv_neighbour_stats_t neighbours;  /* the candidate search's record */
    int64_t mid_near_draws;           /* draws of all points, rejected ones included */
    int64_t further_draws;
    int32_t draw_overflow;            /* 1: a point gave up drawing, the pairs are not usable */
    int32_t candidates;               /* kc */
    int32_t reserved[2];              /* 0 */
} cv_pacmap_stats_t;
typedef struct cv_pacmap_plan {
    int32_t n, c, n_neighbors, n_mn, n_fp;
    int32_t candidates;               /* kc */
    uint64_t pairs_scratch_bytes, optimise_scratch_bytes;
} cv_pacmap_plan_t;
int cv_pacmap_plan(int n, int c, int n_neighbors, int n_mn, int n_fp, cv_pacmap_plan_t* plan);
int cv_pacmap_pairs(cv_engine_t* eng, const float* pre, int n, int c, int n_neighbors, int n_mn, int n_fp, uint64_t seed,
                    int32_t* neighbours, int32_t* mid_near, int32_t* further, cv_pacmap_stats_t* stats, void* scratch,
                    size_t scratch_bytes, void* stream);
int cv_pacmap_optimise(cv_engine_t* eng, const float* init, int n, const int32_t* offsets, const int32_t* entries, int64_t n_entries,
                       int iterations, float* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- placing new rows into a fitted map (additions under ABI 6; detect with dlsym(handle, "cv_pacmap_place")) ------------------- */
/* The other half of run.reduce_embeddings_by_foreign_table_url: the reducer is fitted on one table (the entries above) and every other
 * table of the run is placed into the SAME map, the basis held still.  Again a READING, of the pacmap package's transform: pairs from
 * each new point to its nearest basis points by the scaled distance, the attraction term alone, the same 450-step schedule; defined
 * in numpy by chessvision/embeddings.py (pacmap_place_pairs, pacmap_place), derived in DESIGN.md section 4 "Placing new points".  The
 * entries equal that definition exactly: pairs index for index, coordinates bit for bit.  Deviations from the package: exact
 * neighbour candidates, at most 64 of them, the Adam bias powers as running products.
 *
 * What the caller keeps of a fit (embeddings.EmbeddingMap): pre (n, c) float32, the preprocessed basis; its coordinates (n, 2); and
 *   sigma (n) double, the rows' scale in cv_pacmap_pairs' neighbour choice, which cv_pacmap_basis_scale recomputes: the candidate
 *   search of cv_pacmap_pairs (kc = min(n_neighbors + 50, 64, n - 1), exclude-self) and max(mean of sqrt(D) at ranks 3, 4, 5, 1e-10).
 * New rows are preprocessed on the host with the fit's stored parameters (embeddings.pacmap_preprocess_new) -> pre_new (q, c).
 *
 * cv_pacmap_place_pairs -> neighbours (q, n_neighbors) int32: the kc = min(n_neighbors + 50, 64, n) exact nearest basis rows of
 *   every new row (cv_embedding_neighbours, flags 0: no row excluded); sigma_q by the rule above on the row's own candidates; the
 *   row keeps the n_neighbors candidates with the smallest (D_qj / (sigma_q * sigma[j]), j), ascending.  stats: the search's record.
 * cv_pacmap_place: ONE launch for all iterations, one lane per new point (no new point reads another: a batch equals its rows placed
 *   one at a time, bit for bit).  Per iteration it = 0 .. iterations - 1 and new point p, Yb = basis, float32, every operation
 *   rounded once:
 *       g = (0, 0);  for slot u in order (a partner outside [0, n) is skipped):
 *           e = Y[p] - Yb[b_u];  d = 1;  d = d + e0*e0;  d = d + e1*e1;  t = 10 + d;  w = w_n * (20 / (t*t));  g = g + w*e
 *       m = m + c1*(g - m);  v = v + c2*(g*g - v);  Y[p] = Y[p] - (lr_t*m) / (sqrt(v) + 1e-7f)
 *   with lr_t, w_n, c1, c2 as cv_pacmap_optimise has them (computed in the kernel, in double).  iterations == 0: out = init.
 * Limits: 1 <= q <= 1 << 22, 1 <= n_neighbors <= 32, 1 <= c <= 4096, max(7, n_neighbors + 1) <= n <= 1 << 22.  cv_pacmap_place_plan
 *   checks them and sizes the two scratch blocks; cv_pacmap_place needs none and takes any 1 <= n <= 1 << 22.
 *
 * All array arguments: DEVICE.  init, basis and out 8-byte aligned, out != init; sigma 8-byte aligned; stats nullable; scratch
 * 16-byte aligned, the caller's, reusable once `stream` has passed the call.  Asynchronous on `stream`; allocate nothing and
 * synchronise nothing.  CV_ERR_INVALID names the offending argument. */
typedef struct cv_pacmap_place_plan {
    int32_t q, n, c, n_neighbors;
    int32_t candidates;               /* kc of cv_pacmap_place_pairs */
    int32_t reserved;                 /* 0 */
    uint64_t scale_scratch_bytes;     /* cv_pacmap_basis_scale (depends on n, c, n_neighbors) */
    uint64_t pairs_scratch_bytes;     /* cv_pacmap_place_pairs */
} cv_pacmap_place_plan_t;
int cv_pacmap_place_plan(int q, int n, int c, int n_neighbors, cv_pacmap_place_plan_t* plan);
int cv_pacmap_basis_scale(cv_engine_t* eng, const float* pre, int n, int c, int n_neighbors, double* sigma, void* scratch,
                          size_t scratch_bytes, void* stream);
int cv_pacmap_place_pairs(cv_engine_t* eng, const float* pre_new, int q, const float* pre, int n, int c, int n_neighbors,
                          const double* sigma, int32_t* neighbours, cv_neighbour_stats_t* stats, void* scratch, size_t scratch_bytes,
                          void* stream);
int cv_pacmap_place(cv_engine_t* eng, const float* init, int q, const float* basis, int n, const int32_t* neighbours, int n_neighbors,
                    int iterations, float* out, void* stream);

/* ---- one image, host to host: the native form of ChessVision.process_image (core.py:152-195) ---------------------------------- */
/* Everything a cgo / JNI / C++ host needs for the reference's per-image entry point in ONE call: INTER_AREA resize to 256x256
 * (core.py:212), UNet forward, sigmoid / threshold mask (core.py:273, utils.py:101-112), contours -> quadrangle (core.py:357-411),
 * height-only scaling (core.py:413-417), perspective warp + gray + flip (utils.py:115-132, core.py:298-300), the 64-way split
 * (core.py:419-439), classifier forward + soft-max (core.py:236-242), arg-max, pawn rule and both FENs (core.py:309-355,
 * 441-469).  Same device stages, in the same order, as the Python class runs them; the results are bit-identical to it.
 *   unet_engine: engine with a UNet loaded; classifier_engine: engine with a ResNet-18 loaded (may be the same handle).
 *   image: HOST (h, w, 3) uint8, channels as given (BGR in the reference); flip != 0: the board is seen from black's side
 *   (square names h1..a8, constants.py:120-129); fallback_quad != 0: classify through the whole-image quadrangle when the mask
 *   yields none (not a reference behaviour: random-init weights in tests and benchmarks).
 *   out: HOST, caller-owned; every pointer may be NULL except the struct itself.  found = 0: no quadrangle, board / probabilities /
 *   FEN fields are left untouched.
 * The host waits twice (an event behind the UNet, `stream` itself at the end); the mask and the probabilities are written by their
 * kernels straight into the engine's page-locked block, the board travels on an engine-owned side stream that is joined into `stream`
 * before the final wait.  Staging buffers (page-locked host memory and device memory for the image and the results) belong to
 * unet_engine and are reused across calls: one call at a time per extractor engine (serialised internally). */
typedef struct cv_image_result {
    float*   logits;          /* 256 x 256 float32: BoardExtractionResult.probabilities (raw logits, core.py:287,306) */
    uint8_t* mask;            /* 256 x 256 uint8 0 / 255 */
    float    quadrangle[8];   /* 4 x (x, y) in image pixels, reference vertex order (TR, TL, BL, BR) */
    int32_t  found;           /* 1: a quadrangle was found (or taken as fallback) and the position fields are valid */
    uint8_t* board;           /* 512 x 512 uint8: the rectified, gray, flipped board image */
    float*   probabilities;   /* 64 x 13 float32 soft-max, squares in a8..h1 order */
    int8_t*  labels;          /* 64 validated class indices (order "BKNPQRbknpqrf") */
    char     fen[72];         /* piece placement after the pawn rule */
    char     original_fen[72];
    int32_t  fixes[16 * 4];   /* {0, square index, original class, corrected class} */
    int32_t  n_fixes;
    uint8_t* squares;         /* 64 x 64 x 64 uint8 or NULL: PositionResult.squares, the board cut into its squares a8..h1 (the
                                 reference's extract_squares, utils.py:115-132: tile (r, c) = board[64 r .. 64 r + 63][64 c .. 64 c + 63]) */
} cv_image_result_t;
/* The struct grew once (ABI 5 appended `squares`) and may grow again, so the entry point takes the size of the struct AS THE CALLER
 * COMPILED IT: fields at or beyond `out_size` are neither read nor written.  Pass sizeof(cv_image_result_t).  CV_ERR_INVALID when
 * out_size does not even cover the ABI 3 fields (through n_fixes). */
int cv_process_image_v2(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* image, int h, int w,
                        float threshold, int flip, int fallback_quad, cv_image_result_t* out, size_t out_size, void* stream);
/* ABI 3 / 4 entry point, kept for binaries built against the struct WITHOUT `squares`: identical to cv_process_image_v2 with out_size =
 * offsetof(cv_image_result_t, squares), i.e. `squares` is never touched whatever the caller's struct holds there. */
int cv_process_image(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* image, int h, int w,
                     float threshold, int flip, int fallback_quad, cv_image_result_t* out, void* stream);

/* ---- JPEG decode (additions under ABI 6: look the symbols up with dlsym; the version stays 6) ------------------------------------ */
/* Baseline / extended sequential Huffman JPEG, 8 bit, one interleaved scan; 1 component, or 3 components (YCbCr) with luma sampling
 * 1x1, 2x1 or 2x2 and chroma 1x1.  The decode is split where the hardware splits it: the serial Huffman stage on the host
 * (cv_jpeg_entropy_decode, one image per host thread), everything after it on the device (cv_jpeg_reconstruct_u8).  The pixels are
 * those of libjpeg with its defaults (JDCT_ISLOW, fancy up-sampling, fixed-point YCbCr tables), i.e. of cv2.imdecode without
 * EXIF rotation and of Pillow, byte for byte, on every stream an encoder writes.  The EXIF orientation tag is applied by the entries
 * that say so (cv_jpeg_reconstruct_oriented_u8, cv_process_jpeg_oriented) and by no other.  Progressive, arithmetic, lossless, hierarchical and
 * 12-bit streams, 4 components, Adobe RGB, other sampling factors, several scans and truncated or corrupt data are refused with
 * CV_ERR_INVALID and a message naming the reason and the byte offset; no partial image is ever returned. */
typedef struct cv_jpeg_info {
    int32_t width, height;
    int32_t components;          /* 1 or 3 */
    int32_t luma_h, luma_v;      /* luma sampling factors; 1 x 1 for a 1-component stream */
    int32_t restart_interval;    /* MCUs between restart markers, 0: none */
    int32_t orientation;         /* EXIF orientation tag (1..8), 0: absent.  Reported here; applied by
                                    cv_jpeg_reconstruct_oriented_u8 and cv_process_jpeg_oriented alone. */
    int32_t supported;           /* 0: this library does not decode the stream; `reason` says why */
    char    reason[160];         /* empty when supported */
} cv_jpeg_info_t;
enum { CV_JPEG_BGR = 0, CV_JPEG_RGB = 1, CV_JPEG_GRAY = 2 };

/* Parse the markers up to the first scan.  HOST only, no engine, no HIP call.  CV_OK whenever *info was filled: an unsupported,
 * truncated or corrupt header comes back as supported = 0 with its reason, not as an error code. */
int cv_jpeg_info(const uint8_t* bytes, size_t len, cv_jpeg_info_t* info);
/* The Huffman stage of one image.  HOST only, no engine, no HIP call; thread-safe; `coeffs` may be page-locked memory.
 *   coeffs: `capacity` int16 elements, at least 64 x the blocks of the stream: one plane of 8 x 8 blocks per component,
 *   [component][block_row][block_col][64], natural (de-zigzagged) order, padded to whole MCUs (MCU = 8 luma_h x 8 luma_v pixels;
 *   component 0 has luma_h x luma_v blocks per MCU, the others one; a 1-component stream has MCUs of one block).
 *   qtables: components x 64 uint16, natural order, the table of each component.
 * CV_ERR_INVALID with the reason and byte offset for every stream cv_jpeg_info reports as unsupported, for a capacity too small, and
 * for entropy data that is truncated or corrupt (a code that is not in its table, a coefficient index past 63, a wrong restart
 * marker, no EOI behind the scan); `coeffs` holds nothing of use then. */
int cv_jpeg_entropy_decode(const uint8_t* bytes, size_t len, int16_t* coeffs, size_t capacity, uint16_t* qtables);
/* Dequantise + inverse DCT, chroma up-sampling and colour conversion of n images of ONE geometry, asynchronously on `stream`: two
 * launches, no allocation, no synchronisation.
 *   coeffs: DEVICE, n x (64 x blocks) int16 as cv_jpeg_entropy_decode writes them, 16-BYTE ALIGNED; qtables: DEVICE, n x components
 *   x 64 uint16, 16-byte aligned (each image has its own tables); info: HOST, the geometry all n images share;
 *   planes: DEVICE scratch between the two launches, at least n x 64 x blocks bytes (planes_bytes says how many there are), 8-byte
 *   aligned; dst: DEVICE, (n, height, width, 3) uint8 in channel_order CV_JPEG_BGR / CV_JPEG_RGB (a 1-component stream is replicated
 *   into the three channels), or (n, height, width) for CV_JPEG_GRAY (1-component streams only), any alignment.
 * CV_ERR_INVALID for a misaligned pointer, a short planes buffer or an info record that is not supported. */
int cv_jpeg_reconstruct_u8(cv_engine_t* eng, const int16_t* coeffs, const uint16_t* qtables, int n, const cv_jpeg_info_t* info,
                           int channel_order, uint8_t* planes, size_t planes_bytes, uint8_t* dst, void* stream);
/* cv_jpeg_reconstruct_u8 with the EXIF orientation applied in the colour stage's store (no second pass over the batch, no further
 * buffer): `orientation` is the tag all n images share, 0..8 (what cv_jpeg_info reports; info->orientation itself is NOT read).  With
 * (H, W) = (info->height, info->width), dst[y][x] is
 *     0, 1: src[y][x]          2: src[y][W-1-x]      3: src[H-1-y][W-1-x]    4: src[H-1-y][x]         -- dst is (n, H, W, 3 | 1)
 *     5: src[x][y]             6: src[H-1-x][y]      7: src[H-1-x][W-1-y]    8: src[x][W-1-y]         -- dst is (n, W, H, 3 | 1)
 * where src is what cv_jpeg_reconstruct_u8 writes; 6 is the quarter turn clockwise, 8 counter-clockwise (the cases of
 * PIL.ImageOps.exif_transpose, against which they are tested, and -- as read in OpenCV's source, not run -- of the ExifTransform
 * behind cv2.imdecode).  0 and 1 launch exactly what cv_jpeg_reconstruct_u8 launches.  Every other argument, the two launches, and the
 * stream contract are cv_jpeg_reconstruct_u8's: asynchronous on `stream`, no allocation, no synchronisation.  CV_ERR_INVALID also for
 * an orientation outside 0..8. */
int cv_jpeg_reconstruct_oriented_u8(cv_engine_t* eng, const int16_t* coeffs, const uint16_t* qtables, int n, const cv_jpeg_info_t* info,
                                    int channel_order, int orientation, uint8_t* planes, size_t planes_bytes, uint8_t* dst, void* stream);
/* cv_process_image_v2 with a different front: `bytes` is a JPEG stream instead of decoded pixels.  The entropy stage writes into the
 * extractor engine's page-locked block, the coefficients are uploaded and reconstructed (BGR) into the device image where
 * cv_process_image_v2 copies the caller's pixels; everything after that is the same code.  The quadrangle is in the stream's pixel
 * coordinates; EXIF orientation is not applied (cv_process_jpeg_oriented applies it).  The engine's staging blocks grow by the coefficient pieces at the first call.
 * CV_ERR_INVALID with the parser's reason for a stream that is not supported. */
int cv_process_jpeg(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* bytes, size_t len, float threshold,
                    int flip, int fallback_quad, cv_image_result_t* out, size_t out_size, void* stream);
/* cv_process_jpeg with one more argument.  apply_orientation != 0: the stream's EXIF orientation tag (IFD0 of its first Exif APP1
 * segment; absent or 1: nothing changes) is applied while the photo is reconstructed, as cv_jpeg_reconstruct_oriented_u8 does, so the
 * device image, the resize, the quadrangle coordinates and the warp are all those of the upright photo: the result equals
 * cv_process_image_v2 of the oriented pixels bit for bit.  apply_orientation == 0 is cv_process_jpeg.  The result struct is unchanged. */
int cv_process_jpeg_oriented(cv_engine_t* unet_engine, cv_engine_t* classifier_engine, const uint8_t* bytes, size_t len, float threshold,
                             int flip, int fallback_quad, int apply_orientation, cv_image_result_t* out, size_t out_size, void* stream);

/* ---- JPEG encode (additions under ABI 6: look the symbols up with dlsym; the version stays 6) ------------------------------------ */
/* Gray images to complete baseline JPEG files, byte for byte what libjpeg writes for a one-component image with its defaults
 * (PIL.Image.fromarray(a, "L").save(f, "JPEG", quality=q)): Annex K luminance table scaled by jpeg_set_quality(q, TRUE), JDCT_ISLOW,
 * Annex K Huffman tables DC0 / AC0, JFIF 1.1 header, no restart markers.  quality is clamped to 1..100.  Colour, optimised tables,
 * progressive and EXIF are not written. */
#define CV_JPEG_GRAY_HEADER_BYTES 328
/* The bytes in front of the entropy-coded segment: SOI, APP0, DQT, SOF0, DHT, DHT, SOS.  header: CV_JPEG_GRAY_HEADER_BYTES bytes;
 * qtable: 64 uint16 in natural order, or NULL.  Host only, no engine.  h, w: 1..65535. */
int cv_jpeg_gray_header(int h, int w, int quality, uint8_t* header, uint16_t* qtable);
/* The largest file an h x w image (1..4096 each) can give: header + every 8x8 block at 20 + 63 * 26 bits with every byte stuffed
 * + EOI, a multiple of 16. */
int cv_jpeg_gray_max_bytes(int h, int w, size_t* bytes);
/* src: DEVICE, (n, h, w) uint8, n >= 1, h and w 1..4096.  out: DEVICE, out_capacity >= n * cv_jpeg_gray_max_bytes(h, w) bytes; offsets:
 * DEVICE, n + 1 int64; lengths: DEVICE, n int32.  File i is the lengths[i] bytes at out + offsets[i]; offsets are multiples of 16 in
 * input order and offsets[n] is the end of the last file rounded up, so a caller downloads out[0 .. offsets[n]) and never the capacity.
 * Launches only, on `stream`; images are worked through in fixed chunks over scratch of the engine (at most ~90 MB whatever n, grown
 * once per larger geometry), so n is unbounded.  The output is a pure function of pixels and quality.  Two encodes on one engine
 * are ordered on the device, whatever their streams. */
int cv_jpeg_encode_gray_u8(cv_engine_t* eng, const uint8_t* src, int n, int h, int w, int quality, uint8_t* out, size_t out_capacity,
                           int64_t* offsets, int32_t* lengths, void* stream);

/* ---- JPEG encode, colour: what libjpeg writes for an RGB image with its defaults, byte for byte --------------------------------
 * (PIL.Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=s); 4:2:0 is libjpeg's default and so cv2.imwrite's, which has not
 * been run here): three components, jccolor.c's YCbCr, jcsample.c's plain box for chroma with libjpeg's edge padding, one interleaved
 * scan, luma with the gray encoder's tables and chroma with the Annex K.2 quantiser and the K.3.3.2 / K.3.3.4 Huffman tables, a
 * 623-byte header (SOI, APP0, DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, SOS).  Smoothing, other sampling factors, optimised tables,
 * progressive, restart markers, EXIF and ICC are not written. */
#define CV_JPEG_COLOUR_HEADER_BYTES 623
enum { CV_JPEG_SUB_444 = 0, CV_JPEG_SUB_422 = 1, CV_JPEG_SUB_420 = 2 };     /* luma sampled 1x1, 2x1, 2x2 against chroma's 1x1 */
/* header: CV_JPEG_COLOUR_HEADER_BYTES bytes; qtables: 2 x 64 uint16 in natural order (luma, chroma), or NULL.  Host only, no engine.
 * h, w: 1..65535. */
int cv_jpeg_colour_header(int h, int w, int quality, int subsampling, uint8_t* header, uint16_t* qtables);
/* The largest file an h x w image (1..4096 each) can give: header + every coded block -- the dummy luma blocks of partial MCUs
 * included -- at 20 + 63 * 26 bits (luma) or 22 + 63 * 26 bits (chroma) with every byte stuffed + EOI, a multiple of 16. */
int cv_jpeg_colour_max_bytes(int h, int w, int subsampling, size_t* bytes);
/* src: DEVICE, (n, h, w, 3) uint8 in channel_order CV_JPEG_BGR / CV_JPEG_RGB (which only says which byte of a pixel is R), n >= 1, h
 * and w 1..4096.  out: DEVICE, out_capacity >= n * cv_jpeg_colour_max_bytes(h, w, subsampling) bytes; offsets: DEVICE, n + 1 int64;
 * lengths: DEVICE, n int32.  File i is the lengths[i] bytes at out + offsets[i]; offsets are multiples of 16 in input order and
 * offsets[n] is the end of the last file rounded up.  Launches only, on `stream`; images are worked through in fixed chunks over the
 * scratch the gray encoder uses (grown once per larger geometry), so n is unbounded, and gray and colour encodes of one engine are
 * ordered on the device, whatever their streams.  The output is a pure function of pixels, order, subsampling and quality. */
int cv_jpeg_encode_colour_u8(cv_engine_t* eng, const uint8_t* src, int n, int h, int w, int channel_order, int subsampling, int quality,
                             uint8_t* out, size_t out_capacity, int64_t* offsets, int32_t* lengths, void* stream);

/* MFMA lane-map self test: computes D = A(16xK) * B(Kx16) with the kernels' fragment loaders for both
 * precisions and returns the max abs error against a host reference (used by tests; 0 expected). */
int cv_selftest_mfma(cv_engine_t* eng, float* max_err_f16, float* max_err_f32);

#ifdef __cplusplus
}
#endif
#endif /* CHESSVISION_HIP_H */
