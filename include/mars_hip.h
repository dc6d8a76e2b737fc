/*
 * mars_hip.h -- additive extensions of the MI355X build.  Nothing in here
 * exists in the reference; nothing in here changes what the reference API
 * (nna.h, nna_memory.h, nna_tensor.h, mars_runtime.h, mxu_ops.h) does for a
 * single-frame caller.  Plain C ABI: pointers and sizes only.
 *
 * Why they exist:
 *  - the reference has no batch dimension (every kernel ignores shape[0],
 *    reference mars_runtime.c:566-589): mars_hip_set_batch() turns the model's
 *    I/O tensors into `n` independent frames, each computed exactly as one
 *    reference mars_run would compute it;
 *  - the detection tail (decode + NMS) lives in a demo program in the reference
 *    (src/mars/mars_yolo_test.c:80-130), not in its library;
 *  - HBM-resident I/O and one-shot parameter broadcast for one-process-per-GPU
 *    frame sharding.
 */
#ifndef MARS_HIP_H
#define MARS_HIP_H

#include "mars_runtime.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- batching */
/* Re-plans the model for `n` frames.  After the call mars_get_input()->vaddr
 * is a pinned host buffer of n * frame_bytes (frame-major, frames densely
 * packed; frame_bytes = mars_hip_tensor_frame_bytes), ->alloc_size says so; same for outputs.
 * Activations are re-zeroed.  With n == 1 (also the state after mars_load_*) ->alloc_size is what the reference
 * reports: the size of its shared working buffers, i.e. the largest 64-byte-rounded tensor_byte_size() of any
 * activation (reference mars_runtime.c:250-334), and the staging buffer is that large. */
mars_error_t mars_hip_set_batch(mars_model_t *model, int n);
int mars_hip_get_batch(const mars_model_t *model);

/* Bytes of one frame of a tensor by its shape and dtype (numel * element size). */
size_t mars_hip_tensor_frame_bytes(const mars_model_t *model, int tensor_index);
/* The reference's format-aware tensor size (static tensor_byte_size(), mars_runtime.c:80-124): NDHWC32 rounds
 * channels up to 32, NMHWSOIB2 counts 1024-byte blocks, UINT4 packs two per byte.  Host-only. */
size_t mars_hip_tensor_byte_size(const mars_tensor_t *desc);

/* mars_run() = upload + run_device + download.  The three parts: */
mars_error_t mars_hip_upload_inputs(mars_model_t *model);    /* pinned host -> HBM, waits */
mars_error_t mars_hip_run_device(mars_model_t *model);       /* enqueue all layers, waits */
mars_error_t mars_hip_run_device_async(mars_model_t *model); /* enqueue only */
mars_error_t mars_hip_download_outputs(mars_model_t *model); /* HBM -> pinned host, waits */
mars_error_t mars_hip_sync(void);
/* What mars_run() brings back.  MARS_HIP_OUTPUT_HEADS (default): the reference's behaviour, every graph output is copied to
 * mars_get_output()->vaddr (for the 640x640 detectors 2.1 MB per frame: at large batches that copy is what bounds
 * mars_run).  MARS_HIP_OUTPUT_ON_DEVICE: the outputs stay in HBM -- for callers that only want the detections
 * (mars_hip_detect reads the device tensors) or fetch single tensors themselves (mars_hip_read_tensor /
 * mars_hip_download_outputs); vaddr then keeps whatever an earlier download left there. */
#define MARS_HIP_OUTPUT_HEADS 0
#define MARS_HIP_OUTPUT_ON_DEVICE 1
mars_error_t mars_hip_set_output_mode(mars_model_t *model, int mode);

/* Device address / per-frame stride of any tensor (weights: stride 0). */
void *mars_hip_tensor_device(mars_model_t *model, int tensor_index, size_t *frame_stride);
/* Device layout of a tensor's pixel rows: 0 = dense (the reference's bytes).  Otherwise the tensor is a graph output
 * whose [pixels][*row_bytes] rows sit at the returned pitch in HBM (the 255-channel YOLO heads are kept at a 256-byte
 * pitch so that their convolutions store aligned rows); mars_get_output / mars_hip_read_tensor / the detection tail
 * already account for it, only code that reads mars_hip_tensor_device() pointers itself has to. */
int mars_hip_tensor_row_pitch(mars_model_t *model, int tensor_index, int *row_bytes);
/* Copy `bytes` of frame `frame` of any tensor to host memory (debug/parity). */
mars_error_t mars_hip_read_tensor(mars_model_t *model, int tensor_index, int frame, void *dst,
                                  size_t bytes);
/* Write one frame of an activation tensor from host memory (tests). */
mars_error_t mars_hip_write_tensor(mars_model_t *model, int tensor_index, int frame,
                                   const void *src, size_t bytes);

/* Fusion level: 0 = one kernel per reference layer, every tensor materialised
 * (per-layer parity); 1 (default) = conv epilogue fusion of the
 * conv->sigmoid->mul chain and ReLU, copies elided where bit-identical;
 * 2 = 1 + the C3 bottleneck's 1x1 evaluated inside the following 3x3's
 * launch (fewer launches: single-frame latency; no gain at large batches).
 * Must be set before mars_hip_set_batch / first run; re-plans. */
mars_error_t mars_hip_set_fusion(mars_model_t *model, int level);

/* Launch-policy knob of the convolution kernels (process-wide): "persist" (0|1), "persist_stages"
 * (2|3), "persist_maxk", "persist_slots" (0 = what the device holds at once), "stages", "bpx", "variant"
 * (force one launch variant wherever a layer has it); "f32_mfma" (float32 convolutions: 0 = the reference's summation
 * order everywhere, bit-identical; 1 = default: the f32 matrix cores -- fused rounding per tap, inside the 1e-4
 * tolerance of the float32 models -- for every convolution from which no byte-wise MAXPOOL over float bytes is
 * reachable; 2 = those matrix cores everywhere; 3 / 4 = everywhere on the bf16 matrix cores with every operand split,
 * exactly, into two / three bf16 pieces and three / six piece products per product -- same tolerance class, 2.7x the rate:
 * what bench.py --dtype f32 runs is 3); "rows" (default 1: the patch-staged deep-K kernel conv_i8_rows where it is ahead);
 * "few_wgs" (default 256: launches with fewer workgroups than this take the small-launch variant); "graph_max_batch" (default 8: at batches up to this the plan is captured into a
 * HIP graph after its first run and replayed with one call -- single frames are launch-bound; 0 = never);
 * "small_batch" (default 1: a launch whose large-batch tiling yields fewer workgroups than the device has CUs takes
 * smaller tiles -- what single frames want; 0 = the large-batch policy everywhere); "rgb_direct" (default 1: the RGB stem
 * loads its matrix-core operands straight from the image; 0 = the patch-staged form);
 * "dual_stream_min_batch" (default 64: a batch of at least this many frames is enqueued as two halves on two streams,
 * frames being independent, so that the gaps of one half's kernels are filled by the other's; 0 = never);
 * "dual_stream_ways" (2..4 parts, default 2: more parts measured slower).
 * "run_chunk" (default 128: mars_run on a batch of at least twice this many frames goes through in chunks of this size --
 * copy-in of chunk k+1, graph of chunk k and copy-out of chunk k-1 overlap; 0 = one piece).
 * The defaults are the measured optimum; tests use "persist_slots" to force the multi-tile walk
 * of the persistent kernel on small inputs.  Results never depend on these.  0 = ok, -1 = unknown key. */
int mars_hip_set_tuning(const char *key, int value);
int mars_hip_get_tuning(const char *key, int *value); /* the process-wide value in force; -1 = unknown key */
/* The same knobs per model: an override is kept on `model`, put in force for the duration of each of ITS runs (mars_run,
 * mars_hip_run_device[_async], the pipelined submit, mars_hip_autotune) and taken back afterwards, so models that want
 * different launch policies can share a process; mars_hip_set_tuning stays the process default.  At most 16 keys per
 * model.  mars_hip_model_get_tuning returns the override, or the process default where there is none.
 * THREADS: the runtime, like the reference's, is single-threaded: the overrides are put in force by rewriting the process
 * knobs around a run, so runs of different models must not overlap in time on different threads (one thread driving
 * several models, or several threads under one lock, is fine). */
int mars_hip_model_set_tuning(mars_model_t *model, const char *key, int value);
int mars_hip_model_get_tuning(mars_model_t *model, const char *key, int *value);
/* Times the launch variants of every int8 convolution of `model` on the device at the current batch
 * (`reps` launches each, <= 0: 3) and pins the fastest per layer until the plan is rebuilt
 * (set_fusion); call after mars_hip_set_batch.  A one-time load cost; outputs are unaffected. */
mars_error_t mars_hip_autotune(mars_model_t *model, int reps);

/* ------------------------------------------------------- per-layer timing */
/* on = 1: every kernel launch is timed with HIP events on the library's stream (one event per launch: a launch's stop
 * event is the next one's start); on = 2: one event per run of consecutive launches of the same kind -- the run's
 * total is reported on its last launch, the others report 0 (a few events per graph instead of one per launch: what
 * bench.py uses inside its timed region).  Read back after a run. */
void mars_hip_set_profiling(mars_model_t *model, int on);
int mars_hip_num_ops(const mars_model_t *model);
/* kind: 0 conv_i8, 1 conv_f32, 2 elementwise, 3 data movement, 4 other */
int mars_hip_op_info(const mars_model_t *model, int op, int *layer, int *kind, double *macs,
                     double *bytes, float *last_ms);
void *mars_hip_stream(void); /* hipStream_t of the library, as void* */

/* ------------------------------------------------------ parameter arena */
/* One contiguous HBM block holding everything derived from the weight blob
 * (blob mirror, packed conv weights, biases, LUTs).  Identical layout on every
 * rank that loaded the same descriptors, so rank 0 can broadcast it. */
#define MARS_HIP_LOAD_DEFER_WEIGHTS 1u /* parse descriptors, leave the arena unfilled */
#define MARS_HIP_DESCRIBE_FULL 2u      /* mars_hip_describe_plan only: the whole plan, not just kinds and flags (see there) */
/* The launch plan of a file as text, computed on the host only (no device needed: planner tests on the CPU, debugging): one line per launch
 * ("op I layer L KIND in T.. out T" + its flags: relayout / planar_store / lut / add / seg / pair_next / k_limit / in_rec / out_rec / rows_only ...)
 * and one per tensor that is not held as tagged on the device (nhwc_c / partial / zero_from / rec_c / pix_stride).  The tuning and environment in force
 * decide as for a load.  Returns the length of the text (cut at cap, always terminated); 0 = the loader rejects the file.
 * With MARS_HIP_DESCRIBE_FULL in `flags` the text only grows: behind " |" every op line carries every scalar field of the launch that the run path
 * reads (geometry, paddings, offsets into tensors and into the parameter arena, segment / chain / concat-view operands, work counts, scales as hex
 * floats) and every tensor line its sizes; lines that begin with "+" are extra: one per needed tensor the short form does not list, and a last one
 * with the plan's totals and the environment switches it was built under.  Two loads that print the same full text launch the same work.
 * Only the full form shows the 1x1 chained to a fused cv1 + cv2 launch (the bottleneck's m.cv1 evaluated inside the launch that carries
 * split_next): "split_chain S" behind "split_next", S = 0 for none, 1 / 2 for the side of the pair it reads, then the arena offset of its weight
 * image; the chained op keeps its own line and is not launched.  MARS_HIP_NO_CHAIN=1 in the environment switches that pass off ("no_chain" in the
 * last line); MARS_HIP_NO_SPLIT=1 and fusion level 0 switch it off together with the fused pair. */
size_t mars_hip_describe_plan(const void *data, size_t size, unsigned flags, char *out, size_t cap);
mars_error_t mars_hip_load_memory_ex(const void *data, size_t size, unsigned flags,
                                     mars_model_t **model);
void *mars_hip_param_arena(mars_model_t *model, size_t *bytes);

/* ------------------------------------------------------- detection tail */
/* Same record as det_t of reference mars_yolo_test.c:37 (24 bytes). */
typedef struct {
    float x, y, w, h, conf;
    int cls;
} mars_det_t;

#define MARS_YOLO_MAX_DET 1000 /* candidate cap of the reference demo (:187-189) */

/* Host-pointer forms with the reference's exact semantics (one frame):
 * parse_output (:80-104) and nms (:107-130), executed on the GPU. */
int mars_yolo_parse_output(const int8_t *data, int npred, float scale, mars_det_t *dets, int maxd);
int mars_yolo_nms(mars_det_t *dets, int n, float thresh);

/* Batched, device-resident: decode + NMS over the model's current batch.
 * The prediction list of a frame is the concatenation, in the order given, of
 * the listed output tensors, each viewed as rows of 85 int8 with its own
 * desc.scale.  dets: host buffer [batch][MARS_YOLO_MAX_DET]; counts: [batch]
 * (kept detections, sorted as the reference leaves them). */
mars_error_t mars_hip_detect(mars_model_t *model, const int *output_indices, int n_outputs,
                             float nms_thresh, mars_det_t *dets, int *counts);
/* Same, but results stay in HBM (no D2H) -- used by the benchmark loop. */
mars_error_t mars_hip_detect_device(mars_model_t *model, const int *output_indices, int n_outputs,
                                    float nms_thresh);

/* ------------------------------------------- anchor-based YOLOv5 Detect heads */
/* mars_hip_detect reads its outputs as rows of 85 values already decoded (the reference demo's parse_output).  A YOLOv5 graph
 * as exported ends in raw Detect-head convolutions instead: [3 * (5 + nc)] channels per grid cell, the box and score logits of
 * three anchors.  These calls decode such heads on the device into boxes in input pixels (or, through the letterbox of
 * mars_hip_preprocess, in source-image pixels), for any class count nc >= 1:
 *   prediction order: head (as listed; mars_yolo_find_heads lists them by ascending stride), anchor a, cell row gy, column gx;
 *   sig(q) = 1 / (1 + expf(-q * scale)) of the head's int8 byte q and its own scale;
 *   obj = sig(q4); best = first class of largest byte; conf = obj * sig(q_best); both obj and conf >= conf_thresh;
 *   cx = ((2 sig(q0) - 0.5) + gx) * stride, w = (2 sig(q2))^2 * anchor_w (cy, h alike); float32, no fused multiply-add;
 *   the first MARS_YOLO_MAX_DET candidates are kept, then the sort + class-wise NMS of mars_hip_detect; then, with src_w > 0,
 *   x' = (cx - px) * (src_w / nw), w' = w * (src_w / nw) (y, h alike) for the letterbox (nw, nh, px, py) of src_w x src_h frames.
 * The anchor-free DFL head (yolov5nu / YOLOv8 style: 64 box + nc class channels) has its own calls: "anchor-free DFL heads" below; no
 * tensor of it counts as a head here. */

/* The heads of a .mars file, found on the host (no device needed), sorted by stride: int8 outputs of CONV2D layers with
 * 3 * (5 + nc) channels (nc >= 1) that only no-op layers read (or that are graph outputs), whose grid divides the graph input
 * by the same factor on both axes (the stride).  Writes up to cap entries (tensor indices, strides, class counts; any array
 * may be NULL) and returns the number found: 0 = none, -1 = a file the loader rejects. */
int mars_yolo_find_heads(const void *data, size_t size, int *tensor_ids, int *strides, int *num_classes, int cap);

/* Zero-initialise; zero means default in every field. */
typedef struct {
    int n_heads;             /* 0: mars_yolo_find_heads on the loaded file */
    int head_tensors[4];     /* TENSOR indices (not output indices) */
    int strides[4];          /* 0: input height / head height */
    float anchors[4][3][2];  /* pixels; all zero: YOLOv5 P3-P5 defaults (10,13 16,30 33,23 | 30,61 62,45 59,119 | 116,90 156,198 373,326) */
    float conf_thresh;       /* 0: 0.25 */
    float nms_thresh;        /* 0: 0.45 */
    int src_w, src_h;        /* > 0: map boxes back through the letterbox of mars_hip_preprocess for frames of this size */
} mars_yolo_heads_t;
/* Decode + NMS over the model's current batch.  dets: host [batch][MARS_YOLO_MAX_DET]; counts: [batch].  heads may be NULL (all
 * defaults).  MARS_ERR_INVALID_TENSOR: no heads, or a head that is not int8, is only partly written, has no device buffer, has
 * scale <= 0 or a channel count that is not 3 * (5 + nc). */
mars_error_t mars_hip_detect_heads(mars_model_t *model, const mars_yolo_heads_t *heads, mars_det_t *dets, int *counts);
/* Same, results stay in HBM; runs on the auxiliary stream behind the graph, and the next run's head-writing layers wait for it
 * (as mars_hip_detect_device).  mars_hip_detect_results fetches them. */
mars_error_t mars_hip_detect_heads_device(mars_model_t *model, const mars_yolo_heads_t *heads);
/* The detections the last mars_hip_detect_device / mars_hip_detect_heads_device / mars_hip_detect_dfl_device call left in HBM (waits for them). */
mars_error_t mars_hip_detect_results(mars_model_t *model, mars_det_t *dets, int *counts);

/* -------------------------------------------------------- anchor-free DFL heads */
/* The Ultralytics "u" / YOLOv8 Detect head (Distribution Focal Loss): per scale a BOX convolution of 4 * R channels -- R = reg_max bins
 * for each of the sides left, top, right, bottom -- and a CLASS convolution of nc channels on the same grid, concatenated.  The exported
 * softmax / DFL-conv / dist2bbox chain behind the concats is not executed (the shipped yolov5nu.mars carries it with all-zero shapes);
 * these calls decode the two convolutions' int8 bytes themselves, one prediction per cell, float32, every operation rounded on its own:
 *   prediction order: head (as listed; mars_yolo_find_dfl_heads lists them by ascending stride), cell row gy, column gx;
 *   best = first class of largest byte q_b; conf = 1 / (1 + expf(-q_b * class scale)); kept iff conf >= conf_thresh (no objectness);
 *   side k: m = largest of the bytes of channels [k R, (k + 1) R), e_i = expf(-((m - q_i) * box scale)),
 *           dist_k = (0 e_0 + 1 e_1 + ... + (R - 1) e_{R-1}) / (e_0 + ... + e_{R-1}), both sums left to right;
 *   x1 = (gx + 0.5) - dist_l, x2 = (gx + 0.5) + dist_r; cx = ((x1 + x2) * 0.5) * stride, w = (x2 - x1) * stride (y1, y2, cy, h alike);
 *   the first MARS_YOLO_MAX_DET candidates are kept; then sort, class-wise NMS and the letterbox mapping as for the anchor heads.
 * The bytes are read where the plan left them (planes, pixel rows, a channel slice of the concat's buffer): no plan changes. */

/* The DFL heads of a .mars file, found on the host (no device needed), sorted by stride.  A head is a CONCAT layer that does something,
 * of exactly two inputs A, B: int8 activations written by CONV2D layers, of equal H x W that divides the graph input by the same factor
 * on both axes (the stride), read by nothing that does something but this CONCAT, whose own output is a graph output or is read only by
 * no-op layers; A has 4 R channels, 2 <= R <= 32 (the box tensor, reg_max = R), B has nc >= 1 (the class tensor).  Writes up to cap
 * entries per array (at most 4; box / class tensor indices, strides, class counts, reg_max; any array may be NULL) and returns the number
 * found: 0 = none, -1 = a file the loader rejects.  (The decode wants one reg_max for all heads it is given.) */
int mars_yolo_find_dfl_heads(const void *data, size_t size, int *box_ids, int *cls_ids, int *strides, int *num_classes, int *reg_max, int cap);

/* Zero-initialise; zero means default in every field. */
typedef struct {
    int n_heads;                       /* 0: mars_yolo_find_dfl_heads on the loaded file */
    int box_tensors[4], cls_tensors[4]; /* TENSOR indices */
    int strides[4];                    /* 0: input height / grid height */
    int reg_max;                       /* 0: box channels / 4 */
    float box_scales[4], cls_scales[4]; /* 0: the tensor's own desc.scale (the shipped yolov5nu.mars carries 1.0 everywhere) */
    float conf_thresh;                 /* 0: 0.25 */
    float nms_thresh;                  /* 0: 0.45 */
    int src_w, src_h;                  /* > 0: map boxes back through the letterbox of mars_hip_preprocess for frames of this size */
} mars_yolo_dfl_heads_t;
/* Decode + NMS over the model's current batch.  dets: host [batch][MARS_YOLO_MAX_DET]; counts: [batch].  heads may be NULL (all defaults).
 * MARS_ERR_INVALID_TENSOR: no heads; a head tensor that is not int8, is only partly written or has no addressable bytes; an effective
 * scale <= 0; box channels that are not 4 * reg_max with reg_max in 2 .. 32; box and class grids that differ. */
mars_error_t mars_hip_detect_dfl(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, mars_det_t *dets, int *counts);
/* Same, results stay in HBM for mars_hip_detect_results; streams and events as mars_hip_detect_heads_device (the next run's layers that
 * write a box or class tensor wait for the decode). */
mars_error_t mars_hip_detect_dfl_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads);

/* ------------------------------------------------------- pipelined host I/O */
/* mars_run() pays host->HBM copy, graph and HBM->host copy one after the other.  With an open pipe up to three batches are
 * in flight: batch k+1 uploads and batch k-1 downloads (on their own streams, from / into their own buffers) while batch k
 * is computed.  Usage (batch size = mars_hip_set_batch, unchanged while the pipe is open):
 *     mars_hip_pipe_open(model, &opts);
 *     for every batch:  fill mars_hip_pipe_input(model, 0)  ->  mars_hip_pipe_submit(model)
 *                       [from the third batch on]  mars_hip_pipe_wait(model, outs, &dets, &counts)  -> use results
 *     mars_hip_pipe_wait() once more per batch still in flight; mars_hip_pipe_close(model).
 * Results of a batch are bit for bit what mars_run() / mars_hip_detect() give for the same input. */
typedef struct {
    int download_outputs;   /* 1: the graph outputs come back (dense [batch][frame bytes] each, as mars_run leaves them) */
    int detect;             /* 1: decode + NMS on the device, detections come back ([batch][MARS_YOLO_MAX_DET] + counts) */
    int det_outputs[4];     /* detect: output indices forming the prediction list, as for mars_hip_detect */
    int n_det_outputs;
    float nms_thresh;
    int camera_w, camera_h; /* both > 0: CAMERA mode.  Graph input 0 (int8, 3 channels) is fed from uint8 RGB frames of camera_w x
                             * camera_h: mars_hip_pipe_input(model, 0) is then a pinned buffer of [batch][camera_h][camera_w][3] bytes,
                             * and a submit uploads it and runs the letterbox / px - 128 front-end (the reference's load_image(),
                             * src/mars/mars_yolo_test.c:40-77, as mars_hip_preprocess does it) on the main stream ahead of the graph
                             * (round 6: on the upload stream it held up the next batch's copy), into the
                             * slot's graph input -- the demo's whole loop (:132-214: load_image -> run -> parse_output -> nms),
                             * three batches in flight.  0 / 0: the graph inputs themselves are uploaded (as before).
                             * The struct has grown by these two fields (round 5): callers zero-initialise it (`= {0}` / memset) before
                             * setting what they use, so that a build against an older header still means "no camera" (ADVICE r5). */
    const mars_yolo_heads_t *heads; /* detect: non-NULL = decode these raw heads (mars_hip_detect_heads) instead of det_outputs; copied at
                             * open.  In camera mode a zero src_w / src_h means camera_w / camera_h: boxes come back in camera pixels */
    const mars_yolo_dfl_heads_t *dfl_heads; /* detect: non-NULL = decode these DFL heads (mars_hip_detect_dfl) instead; copied at open, camera mode as
                             * for heads.  Setting both heads and dfl_heads is an error (MARS_ERR_INVALID_TENSOR) */
    int camera_format;      /* camera mode: MARS_HIP_CAMERA_RGB (0, as before) or MARS_HIP_CAMERA_NV12: the frames are NV12 ("NV12 camera frames" below;
                             * camera_w and camera_h even), mars_hip_pipe_input(model, 0) is [batch][camera_w * camera_h * 3 / 2] bytes, the slot's
                             * device buffer and its upload are that small, and the submit runs mars_hip_preprocess_nv12_device where the RGB
                             * front-end runs.  Anything else: MARS_ERR_INVALID_FILE.  Not looked at outside camera mode */
    unsigned camera_flags;  /* camera mode, NV12: MARS_NV12_* bits; an unknown bit: MARS_ERR_INVALID_FILE */
} mars_hip_pipe_opts_t;
#define MARS_HIP_CAMERA_RGB 0
#define MARS_HIP_CAMERA_NV12 1
mars_error_t mars_hip_pipe_open(mars_model_t *model, const mars_hip_pipe_opts_t *opts);
/* pinned host buffer ([batch][frame bytes]) to fill for the NEXT submit; changes after every submit */
void *mars_hip_pipe_input(mars_model_t *model, int input_index);
/* queue upload + graph (+ tail) + download of the buffer just filled; returns at once.  At most three batches may be
 * in flight: MARS_ERR_ALLOC_FAILED asks for a mars_hip_pipe_wait first */
mars_error_t mars_hip_pipe_submit(mars_model_t *model);
/* block until the OLDEST submitted batch is complete.  outputs (may be NULL): array of mars_get_num_outputs() pointers,
 * set to that batch's host copies (download_outputs); dets / counts (may be NULL): its detections (detect).  The
 * buffers stay valid until the SECOND mars_hip_pipe_submit after this call returns (four buffer sets, three batches in
 * flight): in the steady-state loop "wait k; submit k+3; use results of k" the results are safe while k+3 is queued and
 * are overwritten by the submit after that. */
mars_error_t mars_hip_pipe_wait(mars_model_t *model, const void **outputs, const mars_det_t **dets, const int **counts);
void mars_hip_pipe_close(mars_model_t *model);
/* camera mode: device time (ms) of the image front-end kernel of the batch mars_hip_pipe_wait() handed out last; < 0 = not available */
float mars_hip_pipe_camera_ms(mars_model_t *model);

/* --------------------------------------------------- synthetic .mars writer */
/* Well-formed graphs (NHWC activations, OHWI int8 weights, int32 bias; or
 * NCHW/OIHW float32) with the YOLOv5 layer sequence and seeded weights, for
 * the model files the reference repo does not ship (.MISSING_LARGE_BLOBS).
 * Format restated from reference include/mars.h:103-221. */
typedef struct {
    int width_x16;   /* channel multiple: 4 = yolov5n (0.25), 8 = yolov5s (0.50) */
    int depth_x3;    /* depth multiple in thirds: 1 = n/s (0.33) */
    int input_hw;    /* square input, multiple of 32 */
    int float32;     /* 0: int8 NHWC; 1: float32 NCHW */
    int nchw_int8;   /* int8 only: emit NCHW/OIHW tags instead of NHWC/OHWI */
    unsigned seed;
    int tiny;        /* 1: 3-conv "tiny_160" chain instead of YOLOv5 */
    int vary_scales; /* 1: every convolution gets its own output / sigmoid / SiLU scales (x0.75 .. x1.35 of the nominal
                      * ones), so no two fused tables are equal; 0 keeps the files of earlier versions byte for byte */
} mars_synth_opts_t;
/* returns the file size; writes at most cap bytes (call with cap 0 to size) */
size_t mars_synth_model(const mars_synth_opts_t *opts, void *buf, size_t cap);
/* The same graphs with a chosen Detect head.  MARS_SYNTH_HEAD_ANCHOR: mars_synth_model's files byte for byte.  MARS_SYNTH_HEAD_DFL (int8
 * only, not tiny): per scale a box branch (conv3x3 + SiLU, conv3x3 + SiLU, conv1x1; 64 channels wide, 64 = 4 x 16 outputs) and a class
 * branch (the same, max(P3 channels, 80) wide, 80 outputs), concatenated; the three concats are the graph outputs.  The class
 * convolution's bias and scale put a few cells per frame, not hundreds, above a confidence of 0.25.  0 = options it rejects. */
#define MARS_SYNTH_HEAD_ANCHOR 0
#define MARS_SYNTH_HEAD_DFL 1
/* MARS_SYNTH_HEAD_SEG (int8 only, not tiny): the DFL twin plus, per scale, a coefficient branch (conv3x3 + SiLU, conv3x3 + SiLU, conv1x1 ->
 * 32 channels) and one prototype branch from the P3 feature (conv3x3 + SiLU, a 2x nearest upsample, conv3x3 + SiLU, conv1x1 -> 32 channels
 * at input / 4).  The file header has four output slots: graph outputs 0 - 2 are the concats and 3 the prototypes; the coefficient tensors
 * are internal tensors named "seg.coef0", "seg.coef1", "seg.coef2" (the prototype tensor: "seg.proto"), each read by one no-op RESHAPE. */
#define MARS_SYNTH_HEAD_SEG 2
/* MARS_SYNTH_HEAD_POSE (int8 only, not tiny): the DFL twin plus, per scale, a keypoint branch (conv3x3 + SiLU, conv3x3 + SiLU, conv1x1 -> 17 x 3
 * = 51 channels), built behind every box and class branch: the three graph outputs and the detections are the DFL twin's.  The keypoint
 * tensors are internal tensors named "pose.kpt0", "pose.kpt1", "pose.kpt2", each read by one no-op RESHAPE. */
#define MARS_SYNTH_HEAD_POSE 3
/* MARS_SYNTH_HEAD_OBB (int8 only, not tiny): the DFL twin plus, per scale, an angle branch (conv3x3 + SiLU, conv3x3 + SiLU, conv1x1 -> 1
 * channel), built behind every box and class branch: the three graph outputs are the DFL twin's.  The angle tensors are internal tensors
 * named "obb.ang0", "obb.ang1", "obb.ang2", each read by one no-op RESHAPE. */
#define MARS_SYNTH_HEAD_OBB 4
size_t mars_synth_model_head(const mars_synth_opts_t *opts, int head, void *buf, size_t cap);

/* ------------------------------------------------------- image front-end */
/* The reference's load_image() (src/mars/mars_yolo_test.c:40-77) after the file decode, on the GPU: letterbox
 * resize of a uint8 RGB image [h][w][3] to tw x th exactly as stbir_resize_uint8() of the vendored
 * stb_image_resize.h does it (Catmull-Rom up / Mitchell down, clamped edges, linear), grey (-17) padding,
 * px - 128.  out = int8 [th][tw][3] (nhwc != 0) or [3][th][tw].  Host pointers; 0 = ok, -1 = failure. */
int mars_yolo_letterbox(const unsigned char *rgb, int w, int h, int tw, int th, int nhwc, signed char *out);
/* Camera batch: `frames` RGB frames of w x h (host memory, contiguous) are letterboxed straight into frames
 * [first_frame, first_frame + frames) of graph input `input_index` in HBM, in the layout its format tag asks for
 * (mars_yolo_test.c:157-165); follow with mars_hip_run_device().  Input must be int8 with 3 channels. */
mars_error_t mars_hip_preprocess(mars_model_t *model, int input_index, const unsigned char *rgb_frames, int w, int h,
                                 int first_frame, int frames);
/* The same front-end on frames that are ALREADY in device memory (a capture card writing into HBM, or a caller's own upload):
 * rgb_dev = frames x [h][w][3] bytes, contiguous; enqueued on the library's current stream, no synchronisation. */
mars_error_t mars_hip_preprocess_device(mars_model_t *model, int input_index, const void *rgb_dev, int w, int h,
                                        int first_frame, int frames);

/* ------------------------------------------------------ NV12 camera frames */
/* The reference's cameras deliver NNA_FORMAT_NV12 (include/nna_types.h), the ISP's 4:2:0 output, not RGB.  The calls below take such frames
 * as they are -- half the bytes of RGB on the way to the device -- and convert on the GPU, inside the front-end.
 * A frame is w * h * 3 / 2 bytes, densely packed (no row pitch): the Y plane [h][w], directly behind it the chroma plane [h / 2][w / 2][2],
 * interleaved U, V.  w and h are even.  Pixel (x, y) takes the chroma pair at (x >> 1, y >> 1): nearest, no chroma interpolation.
 * Integer arithmetic, >> an arithmetic shift (floor), results clamped to [0, 255]; d = U - 128, e = V - 128:
 *   default, BT.601 limited range, c = Y - 16:   R = (298 c + 409 e + 128) >> 8
 *                                                G = (298 c - 100 d - 208 e + 128) >> 8
 *                                                B = (298 c + 516 d + 128) >> 8
 *   MARS_NV12_FULL_RANGE, BT.601 full range:     R = (256 Y + 359 e + 128) >> 8
 *                                                G = (256 Y - 88 d - 183 e + 128) >> 8
 *                                                B = (256 Y + 454 d + 128) >> 8
 *   MARS_NV12_VU: the chroma pairs are stored V, U (NV21).
 * The uint8 RGB image is then letterboxed exactly as by the RGB calls above: every call here writes, bit for bit, what its RGB counterpart
 * writes for the converted frame.  Odd sizes and unknown flag bits are refused before any device work (-1 / MARS_ERR_INVALID_FILE); the other
 * checks and error codes are those of the RGB calls. */
#define MARS_NV12_FULL_RANGE 1u
#define MARS_NV12_VU 2u
/* Bytes of one NV12 frame; 0 for odd or non-positive sizes.  Host only. */
size_t mars_hip_nv12_frame_bytes(int w, int h);
/* One frame -> uint8 RGB [h][w][3].  Host pointers, runs on the GPU; 0 = ok, -1 = failure. */
int mars_yolo_nv12_to_rgb(const unsigned char *nv12, int w, int h, unsigned flags, unsigned char *rgb);
/* mars_yolo_letterbox of one NV12 frame. */
int mars_yolo_letterbox_nv12(const unsigned char *nv12, int w, int h, int tw, int th, int nhwc, unsigned flags, signed char *out);
/* mars_hip_preprocess / mars_hip_preprocess_device of `frames` NV12 frames (contiguous, w * h * 3 / 2 bytes apart).  The device form keeps
 * one scratch buffer for geometries whose frames are converted before the resize: enqueue it on one stream. */
mars_error_t mars_hip_preprocess_nv12(mars_model_t *model, int input_index, const unsigned char *nv12_frames, int w, int h, unsigned flags,
                                      int first_frame, int frames);
mars_error_t mars_hip_preprocess_nv12_device(mars_model_t *model, int input_index, const void *nv12_dev, int w, int h, unsigned flags,
                                             int first_frame, int frames);

/* --------------------------------------------------------------- ROI crops */
/* The second stage of a camera deployment: every detected person, face or plate is cut out of its frame, resized and handed to a small
 * classifier or embedder (the reference ships such a shape: tiny_160_int8.mars, 3 x 160 x 160 int8).  The frames, the detections
 * (mars_hip_detect_*_device) and the second model's input are all in HBM; the calls below connect them on the device.  Everything that
 * touches a pixel is integer arithmetic, so the bytes are defined exactly:
 *
 * Box -> source rectangle.  A mars_det_t in source-frame pixels (centre x, y, size w, h), frames of W x H.  float32, every operation
 *   rounded on its own, no fused multiply-add:
 *     hw = (w * expand) * 0.5f;  x0f = max(x - hw, 0);  x1f = min(x + hw, (float)W);  x0 = (int)floorf(x0f);  x1 = (int)ceilf(x1f)
 *   (y alike with h, H);  cw = x1 - x0, ch = y1 - y0.  The box is SKIPPED when a float field is not finite, w <= 0, h <= 0, cw < min_size or
 *   ch < min_size.  expand == 0 means 1.0, min_size == 0 means 2.  (Before the conversions x0f is limited to W + 1 and x1f to -1, so that
 *   they are defined for boxes far outside the frame; such a box has cw < 0 either way.)
 * Target geometry for a tw x th input.  Stretch (default): nw = tw, nh = th, px = py = 0.  MARS_ROI_KEEP_ASPECT, integers only:
 *     cw * th >= ch * tw:  nw = tw, nh = max(1, (ch * tw + cw / 2) / cw);   otherwise:  nh = th, nw = max(1, (cw * th + ch / 2) / ch);
 *     px = (tw - nw) / 2, py = (th - nh) / 2.
 *   Pixels outside [px, px + nw) x [py, py + nh) are -17, the reference's grey, as in the letterbox.
 * Resize.  Bilinear, half-pixel centres, 8 fractional bits.  Output column i of [0, nw) (64-bit intermediates, / is floor: the
 *   numerator is not negative):
 *     pos = ((2 i + 1) * cw * 256) / (2 * nw) - 128, clamped to [0, (cw - 1) * 256];  i0 = pos >> 8, fx = pos & 255, i1 = min(i0 + 1, cw - 1)
 *   rows alike with ch, nh: j0, j1, fy.  Per channel, a, b = the crop's pixels (i0, j0), (i1, j0), c, d = (i0, j1), (i1, j1), each 0 .. 255:
 *     top = a * (256 - fx) + b * fx;  bot = c * (256 - fx) + d * fx;  v = (top * (256 - fy) + bot * fy + 32768) >> 16;  out = (int8)(v - 128)
 *   The output layout is the one the destination's format tag asks for ([th][tw][3] or [3][th][tw]), as mars_hip_preprocess decides it.
 * NV12 source.  The four taps are converted with the integer BT.601 formulas of "NV12 camera frames" above, the chroma pair taken at
 *   (x >> 1, y >> 1) in FRAME coordinates, all MARS_NV12_* flags apply; then the blend.  An NV12 crop equals the RGB crop of
 *   mars_yolo_nv12_to_rgb of that frame, bit for bit.
 * Area averaging (MARS_ROI_AREA).  Four taps skip most of the source at strong down-scales; with the flag an axis that has more source
 *   samples than outputs is box-filtered instead.  Box -> rectangle, the target geometry, the -17 bands, the layouts, the selection and the
 *   ROI table do not change.  Per axis, with n_in source samples (cw or ch) and n_out outputs (nw or nh), output sample i has a list of
 *   (source index, weight) taps and a denominator D:
 *     flag clear, or n_in <= n_out:  D = 256; the taps are (i0, 256 - f) and (i1, f) from pos, exactly as under "Resize";
 *     flag set and n_in > n_out:     D = n_in.  In units of 1 / n_out of a source sample, output i covers [i * n_in, (i + 1) * n_in) and
 *       source sample s covers [s * n_out, (s + 1) * n_out):  w(i, s) = min((s + 1) * n_out, (i + 1) * n_in) - max(s * n_out, i * n_in)
 *       for s from (i * n_in) / n_out to ((i + 1) * n_in + n_out - 1) / n_out - 1 (/ is floor).  Every such weight is positive, the weights
 *       of one output sum to n_in, there are at most (n_in + n_out - 1) / n_out + 1 of them, and a source sample feeds at most two
 *       outputs.  7 -> 3: weights (3, 3, 1), (2, 3, 2), (1, 3, 3) over the sources 0..2, 2..4, 4..6.
 *   Per pixel and channel, p = the crop's pixel, 0 .. 255, over 64-bit integers (S passes 2^32 once both axes are averaged and
 *   cw * ch > 16 843 009), both / floor:
 *     S = sum over the y taps of wy * (sum over the x taps of wx * p);  v = (S + (Dx * Dy) / 2) / (Dx * Dy);  out = (int8)(v - 128)
 *   With both axes interpolated this is the formula under "Resize" (Dx * Dy = 65536).  The axes are independent: a flat wide box is averaged
 *   along x and interpolated along y.  So: with the flag and no down-scaled axis the bytes are those without it; cw = k * nw, ch = l * nh
 *   gives the rounded mean of every k x l block; a constant crop gives a constant output.  NV12: every tap is converted to RGB first, as
 *   above, then weighted; an NV12 area crop equals the RGB area crop of mars_yolo_nv12_to_rgb of that frame, bit for bit.
 *   The rotated calls ("Rotated crops") refuse the flag.
 * Selection (the detection forms).  Boxes are visited by ascending frame, inside a frame in the order the tail left them.  A box is kept when
 *   conf >= min_conf, cls_count == 0 or cls_first <= cls < cls_first + cls_count, the rectangle rule does not skip it, and fewer than
 *   max_per_frame boxes of its frame are kept already (0: no limit).  Kept boxes fill the destination's frames 0, 1, ... in visiting
 *   order up to its current batch; the boxes beyond are counted as dropped.  Destination frames behind the last crop are filled with -17. */
typedef struct { int frame, det, x0, y0, x1, y1; } mars_roi_t; /* 24 bytes; det = index inside its frame's list (-1: a caller's box) */
#define MARS_ROI_KEEP_ASPECT 1u
#define MARS_ROI_AREA 4u /* "Area averaging"; not for the rotated calls */
/* Zero-initialise; zero means default in every field but the frame size. */
typedef struct {
    int src_w, src_h, src_format; unsigned src_flags; /* frames: MARS_HIP_CAMERA_RGB / _NV12, MARS_NV12_* (NV12 only) */
    float expand, min_conf; int min_size;
    int cls_first, cls_count, max_per_frame;
    unsigned flags;                                    /* MARS_ROI_KEEP_ASPECT | MARS_ROI_AREA */
} mars_hip_roi_opts_t;
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: no options or a NULL pointer, a non-positive size, an unknown
 * format or flag bit, odd NV12 sizes, a negative or non-finite expand / min_conf / min_size / cls_count / max_per_frame, frames or targets
 * too wide for the crop kernel's on-chip buffers (about 5000 pixels; with MARS_ROI_AREA also a target wider than 1280 pixels, or frames too
 * wide for the area kernel's buffers beside the target: about 4700 pixels at 1280, more at narrower targets -- frames up to 3840 wide into
 * targets up to 1280 wide always pass).  MARS_ERR_INVALID_TENSOR: det_model == dst_model, a destination input
 * that is not int8 with 3 channels, no detections in HBM, a model with an open pipe. */
/* The mars_yolo_letterbox of this feature: host pointers in and out, runs on the GPU.  `frames` = n_frames frames of opts->src_w x src_h,
 * densely packed; box i lies in frame frame_of_box[i].  Only the rectangle rule applies.  out = [n_boxes][tw * th * 3] int8 ([th][tw][3] with
 * nhwc != 0, else [3][th][tw]), a skipped box's crop is all -17 and rois[i].x1 == rois[i].x0 marks it (rois may be NULL). */
mars_error_t mars_yolo_crop_boxes(const unsigned char *frames, int n_frames, const mars_det_t *boxes, const int *frame_of_box, int n_boxes,
                                  const mars_hip_roi_opts_t *opts, int tw, int th, int nhwc, signed char *out, mars_roi_t *rois);
/* The device-only chain.  Reads the detections the last mars_hip_detect_device / _heads_device / _dfl_device of det_model left in HBM (as
 * mars_hip_detect_results would; they must be in source-frame pixels already, i.e. decoded with src_w / src_h set) and det_model's batch of
 * frames at frames_dev (densely packed, as for mars_hip_preprocess[_nv12]_device), selects, and writes the crops into input `input_index`
 * of dst_model, one per frame of its batch.  Enqueues only: the work goes on the library's main stream behind the event the detection tail
 * records (the one the next run's head-writing layers wait for), so it is ordered behind the tail, behind any earlier run of dst_model and
 * ahead of its next mars_hip_run_device[_async]. */
mars_error_t mars_hip_crop_detections_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index,
                                             const mars_hip_roi_opts_t *opts);
/* The same with the frames in host memory: uploads them, crops, waits. */
mars_error_t mars_hip_crop_detections(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index,
                                      const mars_hip_roi_opts_t *opts);
/* The ROI table of the last crop call into dst_model (waits for it): rois[k] = where frame k of the input came from, for the first
 * min(kept, cap) frames (rois may be NULL with cap 0); *n_kept crops were written, *n_dropped selected boxes found no frame. */
mars_error_t mars_hip_roi_results(mars_model_t *dst_model, mars_roi_t *rois, int cap, int *n_kept, int *n_dropped);

/* ---------------------------------------------------- Second-stage labels */
/* What a deployment wants from the second stage is a label or an embedding per box, not a feature map: tiny_160_int8.mars leaves a
 * 64 x 154 x 154 map, 1.5 MB per crop, to read back.  The graph cannot reduce it (GLOBAL_AVGPOOL and FC fail a run with
 * MARS_ERR_INVALID_LAYER, SOFTMAX is accepted and not executed: the reference's behaviour, kept).  The calls below are the classifier head
 * as a tail call outside the graph, like the Detect heads: a backbone, a 1 x 1 convolution to nc channels, then -- here -- the global
 * average pool, the ranking and the scores, on the device, defined to the bit.  The pooled sums alone are what an embedder returns.
 *
 * Feature tensor.  An int8 activation tensor T of the model, C channels on an H x W grid ([1, C, H, W], or [1, H, W, C] under the NHWC
 *   tag), 1 <= C <= 4096, 1 <= H * W <= 2^24; a graph output (output_index) or any TENSOR index (tensor > 0).  It is read where the plan
 *   left its bytes -- planes, pixel rows at the writing convolution's pitch, a channel slice of a concat's rows -- for every frame of the
 *   current batch; no plan changes.
 * Pooling.  sum[c] = the int32 sum of the H * W bytes of channel c.  Exact; it cannot overflow inside the limits above.
 * Ranking.  Channels by descending sum[c], ties to the lower channel; the first top_k are kept, 1 <= top_k <= MARS_CLS_MAX_TOPK
 *   (top_k == 0 means 1).  With C < top_k the entries behind the last channel are {cls = -1, score = 0}.
 * Score.  float32, every operation rounded on its own, no fused multiply-add:
 *     logit[c] = ((float)sum[c] / (float)(H * W)) * scale          scale == 0 in the options: the tensor's own desc.scale
 *   default:           score = logit[c]
 *   MARS_CLS_SOFTMAX:  e[c] = expf(logit[c] - logit[best]) with the host libm's expf (csrc/expf_exact.h restates it), best = the top-1 channel;
 *                      den = e[0] + e[1] + ... + e[C - 1], added left to right;  score = e[c] / den
 * Join.  Frame k of the second model is crop k of its ROI table (mars_hip_roi_results).  labels[roi.frame][roi.det] = the top-1 entry of
 *   crop k for k < kept; every other entry of the [batch][MARS_YOLO_MAX_DET] array is {-1, 0}.
 * Not covered: float32 feature tensors; pooling only the un-padded part of a MARS_ROI_KEEP_ASPECT crop; a fully-connected layer behind the
 *   pool; the pipelined mars_hip_pipe_* path.  (Matching the pooled sums against a gallery: "Gallery match" below.) */
#define MARS_CLS_MAX_TOPK 8
#define MARS_CLS_SOFTMAX 1u
typedef struct { int cls; float score; } mars_cls_t; /* 8 bytes */
/* Zero-initialise; zero means default in every field. */
typedef struct {
    int output_index;   /* graph output to pool ... */
    int tensor;         /* ... or, when > 0, this TENSOR index instead */
    int top_k;          /* 0: 1 */
    float scale;        /* 0: the tensor's desc.scale */
    unsigned flags;     /* MARS_CLS_SOFTMAX */
} mars_hip_cls_opts_t;
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: no options or a NULL pointer where one is needed, top_k
 * outside 0 .. 8, an unknown flag bit, a negative or non-finite scale, non-positive n, c, h or w.  MARS_ERR_INVALID_TENSOR: an index out
 * of range; a tensor that is not int8, is a weight, a graph input, only partly written or without addressable bytes (one a fusion pass
 * elided); C or H * W beyond the limits (more than 65535 maps or frames); an effective scale <= 0; *_results with nothing pending;
 * det_model == cls_model; no crop call into cls_model out of this det_model, no classify results on cls_model, no detections in HBM on
 * det_model; a model with an open pipe. */
/* The mars_yolo_crop_boxes of this feature: host pointers in and out, runs on the GPU.  maps = n dense maps, [h][w][c] (nhwc != 0) or
 * [c][h][w]; `scale` stands where a tensor's desc.scale would; top = [n][top_k]; sums = [n][c] or NULL. */
mars_error_t mars_yolo_classify_maps(const signed char *maps, int n, int c, int h, int w, int nhwc, float scale, const mars_hip_cls_opts_t *opts,
                                     mars_cls_t *top, int *sums);
/* The model's current batch; the results stay in HBM.  Enqueues only: the kernels run on the auxiliary stream behind the graph launches
 * enqueued so far (the hand-off of mars_hip_detect_*_device); of the next mars_hip_run_device[_async] only the layers that write T wait
 * for them. */
mars_error_t mars_hip_classify_device(mars_model_t *model, const mars_hip_cls_opts_t *opts);
/* Waits.  top = [batch][top_k], sums = [batch][C] or NULL, *channels = C (may be NULL), all as of the last mars_hip_classify_device. */
mars_error_t mars_hip_classify_results(mars_model_t *model, mars_cls_t *top, int *sums, int *channels);
/* mars_hip_classify_device + mars_hip_classify_results. */
mars_error_t mars_hip_classify(mars_model_t *model, const mars_hip_cls_opts_t *opts, mars_cls_t *top, int *sums);
/* Scatters cls_model's top-1 entries through its ROI table onto det_model's detection lists.  Enqueues only: ordered behind cls_model's
 * classify tail, det_model's detection tail and the crop call, and ahead of whatever next overwrites what it reads or writes -- the next
 * crop call into cls_model, the next classify call on it, the next detect call of det_model. */
mars_error_t mars_hip_label_detections_device(mars_model_t *det_model, mars_model_t *cls_model);
/* Waits.  labels = [batch of det_model][MARS_YOLO_MAX_DET]; entry i of frame f belongs to dets[f][i] of mars_hip_detect_results. */
mars_error_t mars_hip_label_results(mars_model_t *det_model, mars_cls_t *labels);

/* ----------------------------------------------------------- Gallery match */
/* The step behind an embedder: whose face, which plate.  A gallery holds enrolled embeddings with an id each; a query embedding -- the
 * pooled sums mars_hip_classify_device left in HBM, or a caller's vector -- is compared with every row by cosine similarity and the best
 * top_k rows come back as {id, score}.  The products run on the int8 matrix unit; everything is defined to the bit:
 *
 * Quantisation.  An embedding is C int32 values, 1 <= C <= 4096 (any int32, INT32_MIN included: magnitudes are taken in 64 bits).
 *   Integers only: m = max_c |v[c]|.  m == 0: the vector is NULL (it has no direction).  Otherwise
 *     q[c] = sign(v[c]) * ((|v[c]| * 127 + m / 2) / m)          64-bit product, / is floor (the numerator is not negative)
 *   so q[c] lies in [-127, 127] and the largest magnitude maps to +-127;  qq = sum_c q[c]^2 <= 127^2 * 4096 = 66 064 384 fits an int32.
 *   The same rule quantises gallery rows on the host and queries on the device (mars_yolo_embed_quantise states it on the host).
 * Gallery row r.  g_r[0 .. C) int8, an id id_r >= 0 and ginv_r = 1.0f / sqrtf((float)gg_r), gg_r the row's qq, computed on the host when
 *   the row is added.  A null vector cannot be added.
 * Dot.  dot_r = sum_c q[c] * g_r[c], an exact int32, |dot_r| <= 66 064 384.
 * Key and rank.  float32, every operation rounded on its own, no fused multiply-add:  key_r = (float)dot_r * ginv_r  (the conversion rounds
 *   to nearest-even: values above 2^24 do not fit).  Rows by descending key_r, ties to the lower row index; the first top_k are kept,
 *   1 <= top_k <= MARS_CLS_MAX_TOPK (top_k == 0 means 1).  (key, row) is a total order: the result does not depend on how the launcher
 *   cuts the gallery into chunks.
 * Score.  qinv = 1.0f / sqrtf((float)qq);  score_r = key_r * qinv: the cosine.  It may exceed 1 by an ulp and is not clamped.  An entry is
 *   {cls = id_r, score} in a mars_cls_t, the row index r beside it.  Entries with score < min_score are EMPTY: {-1, 0}, row -1
 *   (min_score == 0: no threshold, negative scores are entries too).  With fewer than top_k rows in the gallery the entries behind the
 *   last row are empty; for a null query all entries are empty.
 * Join.  As the label join: idents[roi.frame][roi.det] = the top-1 entry of crop k for k < kept; every other entry is {-1, 0}.
 * Not covered: enrolling rows straight from device results (enrol via mars_hip_classify_results -> mars_hip_gallery_add); centring or
 *   whitening of embeddings; de-duplicating ids inside a top-K (several rows may share an id); removing single rows; float32 embeddings;
 *   the pipelined mars_hip_pipe_* path.  (Tracking across frames: "Tracking" below.) */
typedef struct mars_hip_gallery mars_hip_gallery_t; /* opaque */
/* Zero-initialise; zero means default in every field. */
typedef struct {
    int top_k;          /* 0: 1 */
    float min_score;    /* 0: no threshold */
    unsigned flags;     /* none yet: must be 0 */
} mars_hip_match_opts_t;
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: no options or a NULL pointer where one is needed, a
 * non-positive channels, capacity or n, a negative id, top_k outside 0 .. 8, a negative or non-finite min_score, any flag bit.
 * MARS_ERR_INVALID_TENSOR: channels above 4096, a capacity above 2^24, more rows than the capacity holds, a null vector given to
 * mars_hip_gallery_add, more than 65535 queries, an empty gallery, a gallery whose channels differ from the classify results' C, no
 * classify / match results pending, det_model == cls_model, no crop call into cls_model out of this det_model, no detections in HBM, a
 * model with an open pipe. */
/* The rule on the host, no device needed: vectors = [n][c] int32 -> q = [n][c] int8, qq = [n] (may be NULL; 0 marks a null vector). */
mars_error_t mars_yolo_embed_quantise(const int *vectors, int n, int c, signed char *q, int *qq);
/* A gallery of up to `capacity` rows (1 .. 2^24) of `channels` values.  Its device image: int8 rows padded with zeros to a multiple of 64
 * channels, the ginv array and the id array. */
mars_error_t mars_hip_gallery_create(int channels, int capacity, mars_hip_gallery_t **out);
/* Quantises n vectors ([n][channels] int32) on the host and appends them with their ids (all or none).  Ordered behind every match enqueued
 * so far: it waits for the device. */
mars_error_t mars_hip_gallery_add(mars_hip_gallery_t *g, const int *vectors, const int *ids, int n);
int mars_hip_gallery_count(const mars_hip_gallery_t *g);      /* rows held; -1 without a gallery */
mars_error_t mars_hip_gallery_clear(mars_hip_gallery_t *g);   /* forgets every row; the capacity stays */
void mars_hip_gallery_free(mars_hip_gallery_t *g);            /* waits for the device first */
/* Gallery rows one workgroup of the match kernel walks for a gallery of `rows` rows (a function of `rows` alone): for tests that want row
 * counts around the cut.  0: rows out of range. */
int mars_hip_match_chunk(int rows);
/* The mars_yolo_classify_maps of this feature: host pointers in and out, runs on the GPU and waits.  vectors = [n][channels] int32;
 * top = [n][top_k]; rows = [n][top_k] row indices or NULL. */
mars_error_t mars_yolo_match_vectors(mars_hip_gallery_t *g, const int *vectors, int n, const mars_hip_match_opts_t *opts, mars_cls_t *top, int *rows);
/* Matches the [frames][C] sums the last mars_hip_classify_device of cls_model left in HBM; the results stay there.  Enqueues only, on the
 * auxiliary stream behind that classify tail and ahead of the next one. */
mars_error_t mars_hip_match_device(mars_model_t *cls_model, mars_hip_gallery_t *g, const mars_hip_match_opts_t *opts);
/* Waits.  top = [batch][top_k], rows = [batch][top_k] or NULL, as of the last mars_hip_match_device. */
mars_error_t mars_hip_match_results(mars_model_t *cls_model, mars_cls_t *top, int *rows);
/* mars_hip_match_device + mars_hip_match_results. */
mars_error_t mars_hip_match(mars_model_t *cls_model, mars_hip_gallery_t *g, const mars_hip_match_opts_t *opts, mars_cls_t *top, int *rows);
/* mars_hip_label_detections_device / mars_hip_label_results with cls_model's top-1 MATCH entries, into an array of their own: labels and
 * identities coexist.  Enqueues only, with the label scatter's ordering: behind cls_model's match, det_model's detection tail and the crop
 * call, ahead of the next crop call into cls_model, the next classify or match call on it and the next detect call of det_model. */
mars_error_t mars_hip_identify_detections_device(mars_model_t *det_model, mars_model_t *cls_model);
/* Waits.  idents = [batch of det_model][MARS_YOLO_MAX_DET]; entry i of frame f belongs to dets[f][i] of mars_hip_detect_results. */
mars_error_t mars_hip_identity_results(mars_model_t *det_model, mars_cls_t *idents);

/* ---------------------------------------------------------------- Tracking */
/* The step that connects frame t to frame t + 1.  A tracker holds the track tables of S camera streams in HBM, MARS_TRACK_SLOTS slots each.
 * A tail call associates every frame's detections with its stream's tracks and hangs a stable track id on each detection; optionally the
 * track also carries the best identity seen on it so far.  All arithmetic is float32, every operation rounded on its own, no fused
 * multiply-add; everything is defined to the bit:
 *
 * Frames -> streams.  A call over F frames and a tracker of S streams needs F % S == 0.  Default: frame f is stream f % S, step f / S.
 *   MARS_TRACK_STREAM_MAJOR: stream f / (F / S), step f % (F / S).  A stream's steps are processed in ascending order; streams are
 *   independent.  State persists between calls: one call over 2 T steps leaves exactly the state and outputs of two calls over T steps each.
 * Candidates of a frame with list d[0 .. n).  d[i] is VALID when all five float fields are finite, w > 0, h > 0, and cls_count == 0 or
 *   cls_first <= cls < cls_first + cls_count.  H = the valid detections with conf >= min_conf.  L exists only when low_conf > 0: the valid
 *   detections with low_conf <= conf < min_conf.  The first MARS_TRACK_MAX_CAND members of each set, by index, take part (in the matching and,
 *   for H, in the births); the rest add to the `overflow` counter.
 * Predict.  For every live track: px = x + vx, py = y + vy.
 * IoU(track, det).  The expression of the NMS kernel, a = (px, py, w, h) of the track, b = the detection: corners c -+ s / 2;
 *   x1 = fmaxf(ax1, bx1), y1 alike, x2 = fminf(ax2, bx2), y2 alike;  iw = fmaxf(0, x2 - x1), ih alike;  inter = iw * ih;
 *   uni = ((wa * ha + wb * hb) - inter) + 1e-6f;  iou = inter / uni.
 * Association.  A pair (slot s, detection i) is ELIGIBLE when the classes are equal or MARS_TRACK_ANY_CLASS is set, and iou >= thresh (a
 *   NaN fails the comparison: never eligible).  Eligible pairs are visited by (iou descending, slot ascending, detection index ascending);
 *   a pair is taken when both its track and its detection are still free: greedy matching on a strict total order.  Pass 1: all live
 *   tracks, the set H, iou_thresh.  Pass 2, only with low_conf > 0: the tracks pass 1 left unmatched, the set L, iou_thresh_low.
 * Update, in this order.
 *   Matched slot, with detection i:  dx = d.x - x, dy = d.y - y (x, y: the stored state, not the prediction);
 *     vx = hits == 1 ? dx : (vx + dx) * 0.5f, vy alike;  x, y, w, h, cls = the detection's;  hits += 1, miss = 0.  With
 *     MARS_TRACK_CARRY_IDENTITY: if idents[f][i].cls >= 0 and (ident.cls < 0 or idents[f][i].score >= ident.score) then ident = idents[f][i].
 *   Unmatched live slot:  x = px, y = py, miss += 1;  freed when miss > max_miss, and `deaths` grows by one.
 *   Births, after the deaths.  Each member of H that no pair took, by ascending index, is born into the lowest free slot (slots freed in
 *     this step count as free):  id = next_id++ (per stream, starts at 1, an int32), the state from the detection, vx = vy = 0, hits = 1,
 *     miss = 0, ident = that detection's entry under MARS_TRACK_CARRY_IDENTITY and {-1, 0} otherwise;  `births` grows by one.  With no
 *     free slot `dropped` grows by one (and no id is used).
 *   Output.  out[f][i] = {id, hits}, the values after the update, for every matched or born detection; every other entry up to the array's
 *     width is {-1, 0}.
 * Not covered: the pipelined mars_hip_pipe_* path; optimal (Hungarian) assignment; Kalman covariance (the motion model is the velocity
 *   average above); more than MARS_TRACK_SLOTS tracks per stream.  (An appearance term in the association: "Appearance in tracking"
 *   below.) */
#define MARS_TRACK_SLOTS 256          /* tracks per stream */
#define MARS_TRACK_MAX_CAND 256       /* candidates per frame and pass */
typedef struct { int id, hits; } mars_track_t;                       /* 8 bytes; {-1, 0}: no track */
typedef struct { int id, cls, hits, miss; float x, y, w, h, vx, vy; mars_cls_t ident; } mars_track_state_t; /* 48 bytes */
#define MARS_TRACK_ANY_CLASS 1u
#define MARS_TRACK_CARRY_IDENTITY 2u
#define MARS_TRACK_STREAM_MAJOR 4u
/* Zero-initialise; zero means default in every field. */
typedef struct {
    float min_conf;        /* 0: 0.5  (high set) */
    float low_conf;        /* 0: no second pass */
    float iou_thresh;      /* 0: 0.3  (pass 1) */
    float iou_thresh_low;  /* 0: 0.5  (pass 2) */
    int max_miss;          /* 0: 30 */
    int cls_first, cls_count;
    unsigned flags;
} mars_hip_track_opts_t;
typedef struct mars_hip_tracker mars_hip_tracker_t; /* opaque */
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: no options or a NULL pointer where one is needed (idents
 * under MARS_TRACK_CARRY_IDENTITY among them), non-positive streams, frames or max_det, a negative cap, a negative or non-finite option, a
 * threshold (min_conf, low_conf, iou_thresh, iou_thresh_low) above 1, low_conf >= the effective min_conf, an unknown flag bit.
 * MARS_ERR_INVALID_TENSOR: streams above 65535, max_det above MARS_YOLO_MAX_DET, F % S != 0, a stream index out of range, no detections in
 * HBM, MARS_TRACK_CARRY_IDENTITY without identity results on det_model, *_results with nothing pending, a model with an open pipe. */
mars_error_t mars_hip_tracker_create(int streams, mars_hip_tracker_t **out);      /* 1 .. 65535 */
mars_error_t mars_hip_tracker_reset(mars_hip_tracker_t *t);                       /* all tables empty, next id 1, counters 0; waits */
void         mars_hip_tracker_free(mars_hip_tracker_t *t);                        /* waits for the device first */
/* Waits.  The live tracks of one stream by ascending slot into states[0 .. cap) (states may be NULL with cap 0); *n_live = their number,
 * also where it exceeds cap; counters = births, deaths, overflow, dropped of that stream since the last reset.  n_live and counters may be NULL. */
mars_error_t mars_hip_tracker_read(mars_hip_tracker_t *t, int stream, mars_track_state_t *states, int cap, int *n_live, long long counters[4]);
/* The mars_yolo_match_vectors of this feature: host pointers in and out, runs the same kernel on the GPU and waits.  dets and out are
 * [frames][max_det], 1 <= max_det <= MARS_YOLO_MAX_DET; counts = [frames] (clamped to 0 .. max_det); idents = NULL or [frames][max_det]. */
mars_error_t mars_yolo_track_lists(mars_hip_tracker_t *t, const mars_det_t *dets, const int *counts, const mars_cls_t *idents,
                                   int frames, int max_det, const mars_hip_track_opts_t *opts, mars_track_t *out);
/* Tracks the detections the last mars_hip_detect_*_device call of det_model left in HBM (F = its batch) and, with
 * MARS_TRACK_CARRY_IDENTITY, reads the array mars_hip_identify_detections_device left.  Enqueues only, on the auxiliary stream with the label
 * scatter's ordering: behind the detection tail and the identity scatter, ahead of det_model's next detect call.  The result array lives on
 * det_model beside the labels and identities and is freed with the model. */
mars_error_t mars_hip_track_device(mars_model_t *det_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts);
/* Waits.  tracks = [batch of det_model][MARS_YOLO_MAX_DET]; entry i of frame f belongs to dets[f][i] of mars_hip_detect_results. */
mars_error_t mars_hip_track_results(mars_model_t *det_model, mars_track_t *tracks);
/* mars_hip_track_device + mars_hip_track_results. */
mars_error_t mars_hip_track(mars_model_t *det_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts, mars_track_t *tracks);

/* --------------------------------------------------- Appearance in tracking */
/* The second stage's embedding steers the association: two people cross, a box jumps after an occlusion, the frame rate drops -- the IoU
 * alone loses the track, and with it the identity it carried.  A tracker made by mars_hip_tracker_create_app holds an int8 embedding per
 * slot beside the tables; the calls below take an embedding per detection, compare every live track with every candidate of the high set
 * by cosine similarity on the int8 matrix unit, and let a high cosine stand in for a low IoU (the BoT-SORT / DeepSORT step).  Everything is
 * defined to the bit; "Tracking" above holds wherever this section does not say otherwise:
 *
 * Embeddings.  A detection's embedding is the int8 vector q[0 .. C) with qq = sum_c q[c]^2: the "Gallery match" quantisation of a C-vector
 *   of int32, 1 <= C <= 4096.  qq == 0 (a null vector), or no vector at all, means the detection has NONE.  A track slot holds e[0 .. C)
 *   int8 and ee; ee == 0 means the slot has none.
 * Cosine of slot s and detection i, defined only when ee_s > 0 and qq_i > 0.  dot = sum_c q[c] * e[c], an exact int32;
 *     cos = ((float)dot * einv) * qinv,   einv = 1.0f / sqrtf((float)ee),  qinv = 1.0f / sqrtf((float)qq)
 *   float32, every operation rounded on its own, no fused multiply-add: the arithmetic of "Gallery match" with the track where the gallery
 *   row stands.  It may exceed 1 by an ulp and is not clamped.
 * Pass 1, in the place of "Association" for pass 1 only.  iou = the IoU of the predicted track and the detection, as above.
 *     app = both have an embedding && cos >= app_thresh && iou >= app_min_iou
 *   A pair is ELIGIBLE when the classes are equal or MARS_TRACK_ANY_CLASS is set, and (iou >= iou_thresh || app).
 *     key = app ? fmaxf(iou, cos) : iou
 *   Eligible pairs are visited by (key descending, slot ascending, detection index ascending); a pair is taken when both its track and its
 *   detection are still free.  A strict total order in which a pair's key depends on that pair alone.  A NaN iou fails every comparison,
 *   app_min_iou's too: never eligible.
 * Pass 2 (the low set) is unchanged: IoU only.
 * Update.  The steps of "Tracking", and:
 *   A slot matched, in either pass, to a detection that has an embedding takes it: e = q, ee = qq.  With MARS_TRACK_APP_SMOOTH, when the
 *     slot already has one: v[c] = 3 * e[c] + q[c] in int32, and e, ee = the "Gallery match" quantisation of v (an all-zero v leaves the
 *     slot without an embedding).
 *   A slot matched to a detection without an embedding keeps what it has; so does a coasting slot.
 *   A slot that dies loses its embedding: ee = 0, bytes zeroed.
 *   A birth takes the detection's embedding, or none: never the previous occupant's.
 * Invariants.  With no detection carrying an embedding every output and every state is that of "Tracking".  One call over 2 T steps leaves
 *   exactly the state, embeddings included, and the outputs of two calls over T steps each.
 * Not covered: appearance in pass 2; association with no spatial gate at all (app_min_iou == 0 means 0.1); EMA weights other than 3 : 1;
 *   float32 embeddings; the pipelined mars_hip_pipe_* path; optimal (Hungarian) assignment. */
#define MARS_TRACK_APP_SMOOTH 1u
/* Zero-initialise; zero means default in every field. */
typedef struct {
    float app_thresh;      /* 0: 0.75 */
    float app_min_iou;     /* 0: 0.1 */
    unsigned flags;        /* MARS_TRACK_APP_SMOOTH */
} mars_hip_track_app_opts_t;
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: what "Tracking" refuses so; no appearance options, one of
 * them negative, non-finite or above 1, an unknown flag bit; non-positive channels, nt or nc; a negative n_vectors, or vectors / emb_index
 * NULL with n_vectors > 0; a negative cap.  MARS_ERR_INVALID_TENSOR: what "Tracking" refuses so; channels above 4096; nt or nc above 256;
 * a tracker without an embedding plane; a cosine asked of a side without an embedding; and, for the model forms, what
 * mars_hip_identify_detections_device refuses so (det_model == cls_model, an open pipe, no crop call into cls_model out of this det_model,
 * no classify results on cls_model, no detections in HBM) and classify results whose C differs from the tracker's channels. */
/* The rule's two pieces on the host, no device needed.  The cosine of a detection's (q, qq) and a slot's (e, ee), both C bytes. */
mars_error_t mars_yolo_track_cosine(const signed char *q, int qq, const signed char *e, int ee, int c, float *cos);
/* The MARS_TRACK_APP_SMOOTH update of a slot holding (e, ee) matched to a detection with (q, qq): -> out[0 .. C), *out_ee.  qq == 0: the
 * slot keeps (e, ee); ee == 0: it takes (q, qq).  e and q may be NULL where their sum of squares is 0. */
mars_error_t mars_yolo_embed_blend(const signed char *e, int ee, const signed char *q, int qq, int c, signed char *out, int *out_ee);
/* A tracker with an embedding plane: the tables of mars_hip_tracker_create plus [streams][MARS_TRACK_SLOTS][C rounded up to 64] int8 and
 * [streams][MARS_TRACK_SLOTS] int32 in HBM.  mars_hip_tracker_reset clears the plane too.  mars_yolo_track_lists and mars_hip_track_device
 * stay legal on it: they run this section's rule with no embedding supplied, so deaths and births keep the plane consistent. */
mars_error_t mars_hip_tracker_create_app(int streams, int channels, mars_hip_tracker_t **out);
/* Waits.  The embeddings of the live tracks of one stream by ascending slot, aligned with mars_hip_tracker_read: q = [cap][C] int8,
 * ee = [cap] (both may be NULL with cap 0); *n_live as there. */
mars_error_t mars_hip_tracker_read_embeddings(mars_hip_tracker_t *t, int stream, signed char *q, int *ee, int cap, int *n_live);
/* mars_yolo_track_lists with embeddings: vectors = [n_vectors][C] int32 (NULL with n_vectors == 0), quantised on the device with the bits
 * of mars_yolo_embed_quantise; emb_index = [frames][max_det] (may be NULL with n_vectors == 0): detection (f, i) uses row emb_index[f][i],
 * any value outside 0 .. n_vectors - 1 means none. */
mars_error_t mars_yolo_track_lists_app(mars_hip_tracker_t *t, const mars_det_t *dets, const int *counts, const mars_cls_t *idents, const int *vectors,
                                       int n_vectors, const int *emb_index, int frames, int max_det, const mars_hip_track_opts_t *opts,
                                       const mars_hip_track_app_opts_t *app, mars_track_t *out);
/* mars_hip_track_device with embeddings: takes the [frames][C] sums the last mars_hip_classify_device of cls_model left in HBM and the ROI
 * table of the crop call from det_model into cls_model; on the auxiliary stream it quantises the rows, gives row k < kept to detection
 * (roi.frame, roi.det), and tracks.  Enqueues only, with the identity scatter's ordering; MARS_TRACK_CARRY_IDENTITY works as before and
 * mars_hip_track_results returns the ids. */
mars_error_t mars_hip_track_app_device(mars_model_t *det_model, mars_model_t *cls_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts,
                                       const mars_hip_track_app_opts_t *app);
/* mars_hip_track_app_device + mars_hip_track_results. */
mars_error_t mars_hip_track_app(mars_model_t *det_model, mars_model_t *cls_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts,
                                const mars_hip_track_app_opts_t *app, mars_track_t *tracks);
/* Test hook: the tracking kernel's own matrix routine on the GPU, ungated.  track_q = [nt][C] int8 and track_ee = [nt] stand where slots
 * 0 .. nt - 1 would; vectors = [nc][C] int32 are quantised as above; out = [nt][nc] cosines, 0 where a side has no embedding.
 * 1 <= nt, nc <= 256.  Waits. */
mars_error_t mars_yolo_track_cosine_matrix(const signed char *track_q, const int *track_ee, const int *vectors, int nt, int nc, int c, float *out);

/* ---------------------------------------------------------- Instance masks */
/* The "-seg" sibling of the anchor-free DFL head (YOLOv8-seg style): beside the box and class convolutions every scale has a COEFFICIENT
 * convolution of nm channels on the same grid, and the graph has one PROTOTYPE tensor of nm channels at PH x PW (a quarter of the input in
 * the stock exports, nm = 32).  A detection's mask is sigmoid(coefficients . prototypes) > 0.5 cut to its box.  These calls run the DFL decode
 * + NMS with the origin of every kept detection recorded, and then compute the masks of the first detections of every frame on the device,
 * at the prototype tensor's size.  Integer dots, one float32 product and one compare: everything is defined to the bit.
 *
 * Setup for kept detection i of frame f.  Its origin is (head k, cell p = gy * W_k + gx), the prediction the decode made it from.
 *   a[c] = the byte of channel c of head k's coefficient tensor at cell p, c < nm;  P[c][y][x] = the prototype tensor's bytes of frame f.
 * Dot.        dot(x, y) = sum over c of a[c] * P[c][y][x], int32 (exact: |dot| <= 64 * 2^14).
 * Scale.      s = coef_scale[k] * proto_scale, ONE float32 product.  A scale of 0 in the options means the tensor's own desc.scale; an
 *             effective scale <= 0 (or not finite) is refused.
 * Bit.        bit = ((float)dot * s > logit_min).  logit_min defaults to 0: dot > 0, i.e. sigmoid > 0.5.  (The conversion is exact.)
 * Rectangle.  From the box (cx, cy, w, h) in GRAPH-INPUT pixels -- the record before any src_w / src_h letterbox mapping -- in float32, every
 *             operation rounded on its own, no fused multiply-add:  fx = (float)PW / (float)in_w;
 *               x0 = clamp((int)floorf((cx - w * 0.5f) * fx), 0, PW);  x1 = clamp((int)ceilf((cx + w * 0.5f) * fx), 0, PW);
 *             y0, y1 alike with fy = (float)PH / (float)in_h.  (A value beyond the int range lands on the bound it passed, a NaN on 0.)
 * Cut.        Pixel (x, y) is inside iff x0 <= x < x1 and y0 <= y < y1; bits outside are 0.  An empty rectangle: an all-zero mask, area 0.
 * Selection.  Frame by frame, in the order of the kept list: the detections with conf >= min_conf (default 0: all) until max_per_frame are
 *             taken.  max_per_frame defaults to 16; 1 .. MARS_SEG_MAX_PER_FRAME.  A function of the lists alone.
 * Output.     Per frame max_per_frame slots; slot j holds a mars_mask_t {det, x0, y0, x1, y1, area} -- det = the index in the frame's list,
 *             area = the number of set bits -- and PH rows of pitch = (PW + 31) / 32 uint32 words: pixel x is bit x & 31 of word x >> 5,
 *             padding bits are 0.  Unused slots: {-1, 0, 0, 0, 0, 0} and all-zero words.
 * Limits.     1 <= nm <= MARS_SEG_MAX_NM.  Coefficient tensors: int8, nm channels, on the grid of their head's box tensor.  Prototype tensor:
 *             int8, nm channels.  All of them tensors whose bytes are addressable after a run, as the DFL heads' (read where the plan left
 *             them: planes, pixel rows, a channel slice; no plan changes).  Anything else: MARS_ERR_INVALID_TENSOR.
 * Not covered: a file-level finder for seg heads (no shipped file has one: callers name the tensors); masks inside mars_hip_pipe_*; masks
 *   in the crop or track stages; nm > 64; float32 tensors; anchor-based seg heads.  (Masks at input or camera resolution: "Instance masks in
 *   frame pixels" below.) */
#define MARS_SEG_MAX_PER_FRAME 64
#define MARS_SEG_MAX_NM 64
typedef struct { int det, x0, y0, x1, y1, area; } mars_mask_t; /* 24 bytes */
/* Zero-initialise; zero means default in every field but the tensor indices. */
typedef struct {
    int coef_tensors[4];       /* TENSOR index per DFL head, in the heads' order */
    int proto_tensor;
    float coef_scales[4], proto_scale; /* 0: the tensor's own desc.scale */
    float logit_min, min_conf;
    int max_per_frame;         /* 0: 16 */
} mars_hip_seg_opts_t;
/* DFL decode + NMS of the model's current batch (mars_hip_detect_dfl_device with the same heads: mars_hip_detect_results returns the same
 * bytes, under src_w / src_h too), then the masks.  Enqueues only, on the auxiliary stream behind the graph; the next run's layers that write
 * a box, class, coefficient or prototype tensor wait for it on the device.  MARS_ERR_INVALID_TENSOR: what mars_hip_detect_dfl refuses, no
 * options, a condition of "Limits" or "Scale" above, a logit_min or min_conf that is not finite, max_per_frame outside 0 .. 64, a
 * coefficient grid that differs from its head's, a model with an open pipe. */
mars_error_t mars_hip_detect_seg_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *seg);
/* Waits.  recs = [batch][max_per_frame]; words = [batch][max_per_frame][PH][pitch]; any pointer may be NULL.  MARS_ERR_INVALID_TENSOR before
 * any seg call on this model. */
mars_error_t mars_hip_mask_results(mars_model_t *model, mars_mask_t *recs, uint32_t *words, int *ph, int *pw, int *pitch_words);
/* mars_hip_detect_seg_device + mars_hip_detect_results + mars_hip_mask_results. */
mars_error_t mars_hip_detect_seg(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *seg,
                                 mars_det_t *dets, int *counts, mars_mask_t *recs, uint32_t *words);
/* Device time (ms) of the mask stage alone (selection + masks) of the last mars_hip_detect_seg_device call, from events on the auxiliary
 * stream; waits for it.  < 0: not available. */
float mars_hip_mask_ms(mars_model_t *model);
/* Host pointers in and out, one frame, the same kernels on the GPU; waits.  coefs = [n][nm] rows, one per box, 0 <= n <= 64 (every box is
 * taken: slot i = box i); proto = [nm][ph][pw]; boxes in pixels of an in_w x in_h input; s = the product scale (> 0).  recs = [n], words =
 * [n][ph][(pw + 31) / 32].  0, or -1: an argument out of range, no device, or a failed launch. */
int mars_yolo_masks(const int8_t *coefs, int n, int nm, const int8_t *proto, int ph, int pw, const mars_det_t *boxes, int in_w, int in_h,
                    float s, float logit_min, mars_mask_t *recs, uint32_t *words);

/* ------------------------------------------- Instance masks in frame pixels */
/* The masks of "Instance masks" on the grid of the frame the caller sent: the letterbox undone, the prototype-size dots up-sampled (bilinear,
 * pixel centres aligned, weights in 1/256) and cut to the box, on the device.  Integers up to the one float32 product and compare of
 * "Instance masks": everything is defined to the bit.
 *
 * Grid.       out_w x out_h.  0 / 0 in the options: src_w x src_h of the DFL options when they map through the letterbox, otherwise the graph
 *             input in_w x in_h.  1 <= out_w, out_h <= MARS_MASK_NATIVE_MAX, and out_h * ((out_w + 31) / 32) <= 2^24 as for the prototype masks.
 * Geometry.   With the letterbox mapping (src_w > 0) (nw, nh, px, py) are the integers of the boxes' letterbox rule for src_w x src_h frames:
 *             scale = fminf((float)in_w / src_w, (float)in_h / src_h); nw = (int)(src_w * scale); nh = (int)(src_h * scale); px = (in_w - nw) / 2;
 *             py = (in_h - nh) / 2.  Without it nw = in_w, nh = in_h, px = py = 0.
 * Taps.       int64, exact.  Output column X: the centre of the pixel carried through the letterbox into prototype coordinates is u = N / D,
 *               N = (2X + 1) * nw * PW + 2 * out_w * px * PW - out_w * in_w;   D = 2 * out_w * in_w
 *             (the source frame's width cancels: the grid spans the letterboxed content).  i0 = floor(N / D), a true floor (N may be negative);
 *             r = N - i0 * D;  w1 = (r * 256) / D, in 0 .. 255;  w0 = 256 - w1;  ia = clamp(i0, 0, PW - 1);  ib = clamp(i0 + 1, 0, PW - 1).
 *             Output row Y alike with nh, py, PH, in_h and out_h.
 * Value.      With dot(x, y) the int32 dot of "Instance masks":
 *               S = wy0 * (wx0 * dot(ia, ja) + wx1 * dot(ib, ja)) + wy1 * (wx0 * dot(ia, jb) + wx1 * dot(ib, jb)),  int64, |S| <= 2^36.
 * Bit.        bit = ((float)S * s16 > logit_min).  (float)S rounds to nearest even; s16 = s * 1.52587890625e-05f (2^-16), ONE float32 product
 *             of the product scale s of "Instance masks".  The options mean what they mean there.
 * Rectangle.  From the record mars_hip_detect_results returns -- frame pixels under the mapping, graph-input pixels otherwise: the BASE grid
 *             base_w x base_h = src_w x src_h or in_w x in_h -- by the rule of "Instance masks" with fx = (float)out_w / (float)base_w, fy =
 *             (float)out_h / (float)base_h and the bounds clamped to 0 .. out_w and 0 .. out_h (the same floorf / ceilf, the same NaN rule).
 * Cut, selection, output.  As in "Instance masks": slot j holds a mars_mask_t in OUTPUT pixels and out_h rows of (out_w + 31) / 32 words,
 *             padding bits 0; unused slots {-1, 0, 0, 0, 0, 0} and all-zero words.
 * Refused.    Down-scaling: out_w * in_w < nw * PW or out_h * in_h < nh * PH.  A size out of range; an axis beyond 2^20 (in_w, in_h, PW, PH:
 *             the int64 terms stay exact below it); a set flag bit; everything mars_hip_detect_seg_device refuses.  MARS_ERR_INVALID_TENSOR.
 * Consequence.  Identity geometry and out = PW x PH: N / D = X exactly, w1 = 0, S = 65536 * dot, and every bit is the prototype mask's bit.
 * Not covered: down-scaled masks (area averaging is another feature); masks inside mars_hip_pipe_*; masks in the crop, tile-merge or track
 *   stages; run-length or box-relative output; float32 tensors; nm > 64.  ("Redaction" below consumes these masks on the device.) */
#define MARS_MASK_NATIVE_MAX 8192
/* Zero-initialise; there are no flags yet. */
typedef struct { int out_w, out_h; unsigned flags; } mars_hip_mask_native_opts_t;
typedef struct { int in_w, in_h, nw, nh, px, py, base_w, base_h, out_w, out_h; } mars_mask_geom_t; /* 40 bytes */
/* mars_hip_detect_seg_device with the masks on the output grid: DFL decode + NMS, the selection, the masks, on the auxiliary stream; the
 * ordering and the waits of the next run are those of mars_hip_detect_seg_device.  The results live in a block of their own: the
 * prototype-size results of an earlier mars_hip_detect_seg_device on the same model stay fetchable, and this call produces none.  native ==
 * NULL: every default.  Every refusal comes before anything is allocated or uploaded.  The first call, and every call whose geometry (frame
 * size, output grid, prototype size) differs from the call before, uploads the tap tables and WAITS for the device twice around that upload
 * (an earlier call may still read the old tables); calls that repeat the geometry only enqueue. */
mars_error_t mars_hip_detect_seg_native_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *seg,
                                               const mars_hip_mask_native_opts_t *native);
/* Waits.  recs = [batch][max_per_frame]; words = [batch][max_per_frame][out_h][pitch]; any pointer may be NULL.  MARS_ERR_INVALID_TENSOR before
 * any native seg call on this model. */
mars_error_t mars_hip_mask_native_results(mars_model_t *model, mars_mask_t *recs, uint32_t *words, int *out_h, int *out_w, int *pitch_words);
/* mars_hip_detect_seg_native_device + mars_hip_detect_results + mars_hip_mask_native_results. */
mars_error_t mars_hip_detect_seg_native(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *seg,
                                        const mars_hip_mask_native_opts_t *native, mars_det_t *dets, int *counts, mars_mask_t *recs, uint32_t *words);
/* Device time (ms) of the stage alone (selection + masks) of the last mars_hip_detect_seg_native_device call; waits for it.  < 0: not available. */
float mars_hip_mask_native_ms(mars_model_t *model);
/* Host only, no device: the tap table of one axis.  out_n output pixels over the n_content letterboxed pixels that start at `pad` inside an
 * in_n wide graph input, prototypes P wide: ia, ib, w1 = [out_n] each.  0, or -1: out_n outside 1 .. 8192, in_n or P outside 1 .. 2^20,
 * n_content < 1, pad < 0, pad + n_content > in_n, a NULL table, or down-scaling (out_n * in_n < n_content * P). */
int mars_yolo_mask_taps(int out_n, int in_n, int n_content, int pad, int P, int *ia, int *ib, int *w1);
/* Host pointers in and out, one frame, the same kernel on the GPU; waits.  As mars_yolo_masks, with the boxes in pixels of the geometry's base
 * grid: recs = [n], words = [n][out_h][(out_w + 31) / 32].  0, or -1: what mars_yolo_masks answers -1 to, or a geometry "Refused" above. */
int mars_yolo_masks_native(const int8_t *coefs, int n, int nm, const int8_t *proto, int ph, int pw, const mars_det_t *boxes,
                           const mars_mask_geom_t *geom, float s, float logit_min, mars_mask_t *recs, uint32_t *words);

/* ----------------------------------------------------------- Pose keypoints */
/* The "-pose" sibling of the anchor-free DFL head (YOLOv8-pose style): beside the box and class convolutions every scale has a KEYPOINT
 * convolution of K * D channels on the same grid (K keypoints of D = 2 or 3 numbers; 17 x 3 in the stock export).  A detection's keypoints
 * are the channels of the cell it was made from.  These calls run the DFL decode + NMS with the origin of every kept detection recorded, and
 * then gather and decode the keypoints of the first detections of every frame on the device.  float32, every operation rounded on its own,
 * no fused multiply-add: everything is defined to the bit.
 *
 * Origin.     For kept detection i of frame f: (head k, cell p = gy * W_k + gx), the prediction the decode made it from, as in "Instance
 *             masks".
 * Bytes.      q[c] = the byte of channel c of head k's keypoint tensor at cell p, c < K * D.  Keypoint j owns channels D * j (x), D * j + 1 (y)
 *             and, with D == 3, D * j + 2 (visibility).
 * Scale.      s_k = the head's keypoint scale.  A scale of 0 in the options means the tensor's own desc.scale; an effective scale <= 0 (or
 *             not finite) is refused.
 * Point.      ax = (float)q_x * s_k;  x = ((ax * 2.0f) + (float)gx) * (float)stride_k;  y alike from q_y and gy.  (Ultralytics'
 *             (a * 2 + (anchor - 0.5)) * stride with anchor = g + 0.5.)  Graph-input pixels.
 * Visibility. D == 3: v = 1.0f / (1.0f + expf((-(float)q_v) * s_k)), the function of (byte, scale) the DFL class confidence is, by the same
 *             expf (the host's, tabulated per head).  D == 2: v = 1.0f.
 * Mapping.    With src_w > 0 in the DFL options the keypoints go through the boxes' letterbox rule: x' = (x - px) * (src_w / nw), y' = (y - py) *
 *             (src_h / nh), the factors and paddings those of the boxes.  Without it they stay in graph-input pixels.  v is never mapped.
 * Selection.  Frame by frame, in the order of the kept list: the detections with conf >= min_conf (default 0: all) until max_per_frame are
 *             taken.  max_per_frame defaults to 32; 1 .. MARS_POSE_MAX_PER_FRAME.  A function of the lists alone.
 * Output.     Per frame max_per_frame slots; slot t holds a mars_pose_t {det, head, cell} -- det = the index in the frame's list -- and K
 *             records mars_kpt_t {x, y, v}.  Unused slots: {-1, -1, -1} and all-zero keypoints.
 * Limits.     1 <= K <= MARS_POSE_MAX_KPT, D = 2 or 3.  Keypoint tensors: int8, exactly K * D channels, on the grid of their head's box
 *             tensor, tensors whose bytes are addressable after a run as the DFL heads' (read where the plan left them: planes, pixel rows,
 *             a channel slice; no plan changes).  Anything else: MARS_ERR_INVALID_TENSOR.
 * Not covered: a file-level finder for pose heads (callers name the tensors); keypoints inside mars_hip_pipe_*; keypoints in the
 *   track stages (the crop stage takes them: "Aligned crops" below); OKS-based suppression (the boxes' NMS decides); float32 tensors; anchor-based pose heads. */
#define MARS_POSE_MAX_PER_FRAME 256
#define MARS_POSE_MAX_KPT 32
typedef struct { int det, head, cell; } mars_pose_t; /* 12 bytes */
typedef struct { float x, y, v; } mars_kpt_t;        /* 12 bytes */
/* Zero-initialise; zero means default in every field but the tensor indices and num_kpt. */
typedef struct {
    int kpt_tensors[4];     /* TENSOR index per DFL head, in the heads' order */
    int num_kpt, kpt_dim;   /* K; D (0: 3) */
    float kpt_scales[4];    /* 0: the tensor's own desc.scale */
    float min_conf;
    int max_per_frame;      /* 0: 32 */
} mars_hip_pose_opts_t;
/* DFL decode + NMS of the model's current batch (mars_hip_detect_dfl_device with the same heads: mars_hip_detect_results returns the same
 * bytes, under src_w / src_h too), then the keypoints.  Enqueues only, on the auxiliary stream behind the graph; the next run's layers that
 * write a box, class or keypoint tensor wait for it on the device.  Its results live in a block of their own: a mask call on the same model
 * leaves them alone (each call runs its own tail, the detections are those of the last one).  MARS_ERR_INVALID_TENSOR: what
 * mars_hip_detect_dfl refuses, no options, a condition of "Limits" or "Scale" above, a min_conf that is not finite, max_per_frame outside
 * 0 .. 256, K * D that is not the tensors' channel count, a keypoint grid that differs from its head's, a model with an open pipe. */
mars_error_t mars_hip_detect_pose_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_pose_opts_t *pose);
/* Waits.  recs = [batch][max_per_frame]; kpts = [batch][max_per_frame][K]; any pointer may be NULL; *num_kpt = K.  MARS_ERR_INVALID_TENSOR
 * before any pose call on this model. */
mars_error_t mars_hip_pose_results(mars_model_t *model, mars_pose_t *recs, mars_kpt_t *kpts, int *num_kpt);
/* mars_hip_detect_pose_device + mars_hip_detect_results + mars_hip_pose_results. */
mars_error_t mars_hip_detect_pose(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_pose_opts_t *pose,
                                  mars_det_t *dets, int *counts, mars_pose_t *recs, mars_kpt_t *kpts);
/* Device time (ms) of the keypoint stage alone (selection + gather) of the last mars_hip_detect_pose_device call, from events on the
 * auxiliary stream; waits for it.  < 0: not available. */
float mars_hip_pose_ms(mars_model_t *model);
/* Host pointers in and out, one frame, the same kernels on the GPU; waits.  rows = [n][K * D] bytes, one row per detection, 0 <= n <= 256
 * (every row is taken: slot i = row i); gx, gy, stride = [n], the cell and stride of every row; s = the keypoint scale (> 0); no mapping.
 * kpts = [n][K].  0, or -1: an argument out of range, no device, or a failed launch. */
int mars_yolo_keypoints(const int8_t *rows, int n, int K, int D, const int *gx, const int *gy, const int *stride, float s, mars_kpt_t *kpts);

/* ----------------------------------------------------------- Oriented boxes */
/* The "-obb" sibling of the anchor-free DFL head (YOLOv8-obb style): beside the box and class convolutions every scale has an ANGLE
 * convolution of 1 channel on the same grid, and rotated rectangles suppress each other by ProbIoU.  These calls decode, sort and suppress
 * on the device.  float32, every operation rounded on its own (parentheses below give the order), no fused multiply-add, division and
 * square root correctly rounded: everything is defined to the bit.  The reference has no such head, so nothing here restates it.
 *
 * Tables.     Per head, from the angle scale s (the tensor's own desc.scale, or the override; <= 0 or not finite is refused), built on the
 *             host with its libm and uploaded; for q = -128 .. 127:
 *               sg[q] = 1.0f / (1.0f + expf((-(float)q) * s));   ang[q] = (sg[q] - 0.25f) * 3.14159265f   (Ultralytics' rule: [-pi/4, 3pi/4))
 *               cs[q] = cosf(ang[q]);   sn[q] = sinf(ang[q])
 * Decode.     Prediction order, best class, conf and the side distances dist_l, dist_t, dist_r, dist_b: "anchor-free DFL heads" above.
 *             With q = the angle byte of the cell:
 *               xf = (dist_r - dist_l) * 0.5f;   yf = (dist_b - dist_t) * 0.5f
 *               cx = (((xf * cs) - (yf * sn)) + ((float)gx + 0.5f)) * (float)stride
 *               cy = (((xf * sn) + (yf * cs)) + ((float)gy + 0.5f)) * (float)stride
 *               w = (dist_l + dist_r) * (float)stride;   h = (dist_t + dist_b) * (float)stride;   angle = ang[q]
 *             The first MARS_YOLO_MAX_DET candidates in prediction order are kept.
 * Order.      Confidence descending, then prediction index ascending (for mars_yolo_obb_nms: position in the caller's list ascending): a
 *             plain stable order.  The reference demo's unstable exchange sort, which the upright tails reproduce, is NOT part of this
 *             contract -- the reference has no oriented head.  Confidences are >= 0 and never NaN here (a table of a finite positive scale
 *             holds none); mars_yolo_obb_nms refuses a list that holds a confidence that is NaN or negative (-0 included).
 * Covariance. Per box, with cs, sn its angle's cosine and sine (the tables' entries; for mars_yolo_obb_nms cosf(angle), sinf(angle) on the host):
 *               A = (w * w) / 12.0f;   B = (h * h) / 12.0f
 *               a = (A * (cs * cs)) + (B * (sn * sn));   b = (A * (sn * sn)) + (B * (cs * cs));   c = (A - B) * (cs * sn)
 *               v = (a * b) - (c * c);   d = v > 0 ? v : 0.0f          (a NaN v gives 0)
 * Pair.       For sorted boxes i < j of one class (of any class under MARS_OBB_AGNOSTIC), ProbIoU without a log or a second exp:
 *               sa = a_i + a_j;  sb = b_i + b_j;  sc = c_i + c_j;  dx = x_i - x_j;  dy = y_i - y_j
 *               den = (sa * sb) - (sc * sc)
 *               t1 = (((sa * (dy * dy)) + (sb * (dx * dx))) / den) * 0.25f
 *               t2 = (((sc * (-dx)) * dy) / den) * 0.5f
 *               X = den / (4.0f * sqrtf(d_i * d_j))
 *             i suppresses j iff  expf(-(t1 + t2)) > E * sqrtf(X),  E = (float)(1.0 - (1.0 - (double)T) * (1.0 - (double)T)) from
 *             nms_thresh T, computed once on the host.  This is 1 - sqrt(1 - exp(-(t1 + t2 + 0.5 log X))) > T rearranged.  expf is the host
 *             libm's, bit for bit (csrc/expf_exact.h on the device).  A comparison with a NaN operand is false: zero-area boxes suppress
 *             nothing and are not suppressed.
 * Greedy.     In sorted order; suppressed boxes suppress nothing.
 * Letterbox.  With src_w > 0 in the DFL options, after NMS: x' = (cx - px) * rx, y' = (cy - py) * ry (the boxes' rule and numbers);
 *             w' = w * rx and h' = h * rx -- BOTH by rx, they lie along the box's own axes; the angle is unchanged.
 * Result.     mars_obb_t per kept box, in sorted order; pred = its prediction index (cells of the heads before its head + its cell).
 * Detections. The model's ordinary detection list is filled too, index-aligned with the obb records, so mars_hip_detect_results and the
 *             crop, label and track stages work unchanged ("Rotated crops" below cuts along the box's own axes instead): entry i = the
 *             ENCLOSING UPRIGHT RECTANGLE of obb record i -- same x, y, conf, cls;  w_e = (w * |cs|) + (h * |sn|);  h_e = (w * |sn|) + (h * |cs|), from the mapped w, h.
 * Not covered: the pipelined mars_hip_pipe_* path; an exact polygon IoU; a file-level finder (callers name the angle tensors); float32 tensors; anchor-based obb heads. */
typedef struct { float x, y, w, h, conf; int cls; float angle; int pred; } mars_obb_t; /* 32 bytes */
#define MARS_OBB_AGNOSTIC 1u /* boxes of different classes suppress each other too */
/* Zero-initialise; zero means default in every field but the tensor indices. */
typedef struct {
    int angle_tensors[4];   /* TENSOR index per DFL head, in the heads' order: int8, 1 channel, on the grid of its head's box tensor */
    float angle_scales[4];  /* 0: the tensor's own desc.scale */
    unsigned flags;         /* MARS_OBB_AGNOSTIC */
} mars_hip_obb_opts_t;
/* Oriented decode + sort + rotated NMS of the model's current batch; results stay in HBM.  Enqueues only: streams and events as
 * mars_hip_detect_dfl_device (the auxiliary stream behind the graph; the next run's layers that write a box, class or angle tensor wait for
 * the decode).  The obb records live in a block of their own: a mask or pose call on the same model leaves them alone and the reverse (the
 * detections are those of the last call).  MARS_ERR_INVALID_TENSOR: what mars_hip_detect_dfl refuses; no options; an angle tensor that is
 * not int8, has not exactly 1 channel, whose grid differs from its head's, that is only partly written or has no addressable bytes; an
 * effective angle scale <= 0 or not finite; unknown flag bits; a model with an open pipe. */
mars_error_t mars_hip_detect_obb_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_obb_opts_t *obb);
/* Waits.  boxes = [batch][MARS_YOLO_MAX_DET], counts = [batch]; either may be NULL.  MARS_ERR_INVALID_TENSOR before any obb call on this model. */
mars_error_t mars_hip_obb_results(mars_model_t *model, mars_obb_t *boxes, int *counts);
/* mars_hip_detect_obb_device + mars_hip_detect_results (dets, counts: the enclosing rectangles) + mars_hip_obb_results (boxes). */
mars_error_t mars_hip_detect_obb(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_obb_opts_t *obb, mars_det_t *dets,
                                 int *counts, mars_obb_t *boxes);
/* Device time (ms) of the whole stage (decode + sort + NMS) of the last mars_hip_detect_obb_device call, from events on the auxiliary
 * stream; waits for it.  < 0: not available. */
float mars_hip_obb_ms(mars_model_t *model);
/* Host pointers in and out, the same sort + suppression kernel on the GPU; waits.  boxes = [n], 0 <= n <= MARS_YOLO_MAX_DET; cs, sn =
 * cosf(angle), sinf(angle) on the host; thresh = T (0: 0.45); no mapping; pred is carried.  The kept boxes are written back in order; returns
 * their number, or -1: an argument out of range, unknown flag bits, a confidence that is NaN or negative, no device, or a failed launch. */
int mars_yolo_obb_nms(mars_obb_t *boxes, int n, float thresh, unsigned flags);
/* Pure host code: the four corners of a box, xy = {x0, y0, .. x3, y3}, float32, one rounding per operation, cs = cosf(angle), sn = sinf(angle):
 *   ux = (w * 0.5f) * cs;  uy = (w * 0.5f) * sn;  vx = (h * 0.5f) * sn;  vy = (h * 0.5f) * cs
 *   corner 0 = (x - ux + vx, y - uy - vy);  1 = (x + ux + vx, y + uy - vy);  2 = (x + ux - vx, y + uy + vy);  3 = (x - ux - vx, y - uy + vy),
 * each sum left to right. */
void mars_yolo_obb_corners(const mars_obb_t *box, float xy[8]);

/* ------------------------------------------------------------ Rotated crops */
/* The crop stage for ORIENTED boxes ("Oriented boxes" above): a plate, a line of text or a vehicle seen from above is cut out along its own
 * axes and reaches the second model upright, without the background and the wrong aspect ratio of its enclosing rectangle.  Options
 * (mars_hip_roi_opts_t), selection, the ROI table and the label / identify / track joins are those of "ROI crops"; the sampler differs.
 * float32 with every operation rounded on its own, no fused multiply-add; integers wherever a pixel is touched:
 *
 * Box -> crop frame.  A mars_obb_t in source-frame pixels, frames of W x H; cs, sn = its angle's cosine and sine: in the device chain the decode
 *   tables' entries the obb stage carries per box, in the host-pointer form cosf(angle), sinf(angle) of the host libm.
 *     we = w * expand,  he = h * expand        (expand == 0 means 1.0, min_size == 0 means 2)
 *   The box is SKIPPED when a float field (x, y, w, h, conf, angle) is not finite, w <= 0 or h <= 0, we < min_size or he < min_size,
 *   we > 32768 or he > 32768, or the centre is outside the frame (x < 0, x > W, y < 0, y > H).  Behind this rule (and W, H <= 32767, which
 *   the calls require) every conversion below is defined and every Q16 value fits an int32.
 * Target geometry for a tw x th input.  Stretch: nw = tw, nh = th, px = py = 0.  MARS_ROI_KEEP_ASPECT: the integer rule of "ROI crops" with
 *   cw = max(1, (int)rintf(we)), ch = max(1, (int)rintf(he)).  Pixels outside [px, px + nw) x [py, py + nh) are -17.
 * Sample positions, Q16, per box (rintf = round to nearest even):
 *     sx = we / (float)(2 * nw),  sy = he / (float)(2 * nh)
 *     Ux = (int)rintf((sx * cs) * 65536.0f),     Uy = (int)rintf((sx * sn) * 65536.0f)
 *     Vx = (int)rintf((-(sy * sn)) * 65536.0f),  Vy = (int)rintf((sy * cs) * 65536.0f)
 *     X0 = (int)rintf((x - 0.5f) * 65536.0f),    Y0 = (int)rintf((y - 0.5f) * 65536.0f)
 *   Output column i of [0, nw), row j of [0, nh), in int64:  a = 2 i + 1 - nw,  b = 2 j + 1 - nh,
 *     PX = X0 + a * Ux + b * Vx,  PY = Y0 + a * Uy + b * Vy;   qx = PX >> 8 (arithmetic: floor), ix = qx >> 8, fx = qx & 255;  iy, fy alike.
 * Taps and blend.  Taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1).  A tap with ix outside [0, W) or iy outside [0, H) is 111
 *   in every channel (the grey, -17 after the - 128): a rotated box leaves the frame with a corner, and the corner is grey, not a smeared edge.
 *   There is no clamp.  The blend is that of "ROI crops": top, bot, v = (top * (256 - fy) + bot * fy + 32768) >> 16, out = (int8)(v - 128);
 *   the layout follows the destination's format tag.
 * NV12 source.  Every in-frame tap is converted with the integer BT.601 formulas of "NV12 camera frames", the chroma pair taken at
 *   (ix >> 1, iy >> 1), all MARS_NV12_* flags apply.  A rotated NV12 crop equals the rotated RGB crop of mars_yolo_nv12_to_rgb of the frame.
 * Consequences.  Angle 0, nw == we, we and x - we / 2 integers (rows alike): Ux = Vy = 32768, Uy = Vx = 0, every fx = fy = 0: an exact copy
 *   of the frame's pixels minus 128.  cs, sn of (float)(pi / 2): Ux rounds to 0 and the crop is an exact transposed copy (column i walks down
 *   the frame, row j walks left).
 * Selection (device chain).  The rules of "ROI crops" over the obb records in list order -- min_conf, class window, max_per_frame -- with
 *   the skip rule above in the rectangle rule's place.
 * ROI table.  frame and det as before; det indexes the obb records AND the detection list (they are index-aligned), so the label, identify
 *   and track joins work unchanged.  x0 .. y1 is for the caller's information only, the enclosing rectangle of the expanded box clipped to the
 *   frame:  ex = ((we * |cs|) + (he * |sn|)) * 0.5f,  ey = ((we * |sn|) + (he * |cs|)) * 0.5f,
 *     x0 = (int)floorf(max(x - ex, 0)),  x1 = (int)ceilf(min(x + ex, (float)W)),  y0, y1 alike with ey, H.
 *   A kept box has x1 > x0 and y1 > y0; a skipped box of the host-pointer form has all four zero (x1 == x0 marks it).
 * Refused: what the calls of "ROI crops" refuse, W or H above 32767 (MARS_ERR_INVALID_FILE), and MARS_ERR_INVALID_TENSOR when det_model
 *   holds no obb results (no mars_hip_detect_obb_device since its batch was set).
 * Not covered: the pipelined mars_hip_pipe_* path; area averaging (a strong down-scale samples four taps per output pixel; the upright
 *   crop has MARS_ROI_AREA for it, and the calls below refuse that flag with MARS_ERR_INVALID_FILE before anything else); rotated crops of merged tile lists; boxes whose centre is off-frame (skipped). */
/* mars_yolo_crop_boxes for oriented boxes: host pointers in and out, runs on the GPU.  Only the skip rule applies; a skipped box's crop is
 * all -17 and rois[i].x1 == rois[i].x0 marks it (rois may be NULL). */
mars_error_t mars_yolo_crop_obb(const unsigned char *frames, int n_frames, const mars_obb_t *boxes, const int *frame_of_box, int n_boxes,
                                const mars_hip_roi_opts_t *opts, int tw, int th, int nhwc, signed char *out, mars_roi_t *rois);
/* mars_hip_crop_detections_device over the obb records and (cos, sin) pairs the last mars_hip_detect_obb_device of det_model left in HBM
 * (decoded with src_w / src_h set: source-frame pixels).  Enqueues only; stream and event ordering are exactly those of
 * mars_hip_crop_detections_device, and mars_hip_roi_results serves this call too. */
mars_error_t mars_hip_crop_obb_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index,
                                      const mars_hip_roi_opts_t *opts);
/* The same with the frames in host memory: uploads them, crops, waits. */
mars_error_t mars_hip_crop_obb(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index,
                               const mars_hip_roi_opts_t *opts);

/* ------------------------------------------------------------ Aligned crops */
/* The crop stage for POSE detections ("Pose keypoints" above): an embedder behind the gallery match is trained on ALIGNED inputs -- the
 * five face landmarks, or shoulders and hips, moved onto fixed template positions by a similarity transform before the crop is taken.
 * These calls fit that transform to a detection's keypoints by least squares and cut the crop with the sampler of "Rotated crops".
 * Options (mars_hip_roi_opts_t), the ROI table and the label / identify / track joins are those of "ROI crops".  float32 with every
 * operation rounded on its own (parentheses give the order), no fused multiply-add, division and square root correctly rounded:
 *
 * Inputs per box.  K keypoints mars_kpt_t {x, y, v} in source-frame pixels, frames of W x H.  A template of K points (u_j, v_j) in target
 *   pixels, pixel centres at i + 0.5, the target tw x th.  A bit mask `use`: bit j set = keypoint j may take part; 0 means all K.  min_vis.
 * Participating set.  P = the j, ascending, with bit j of `use` set and kpt[j].v >= min_vis (a NaN v does not pass).
 * Skip rule.  The box is SKIPPED when |P| < 2, or when x, y or v of a participating keypoint is not finite.  A keypoint that does not
 *   participate may hold anything, NaN included.
 * Fit (template -> source; a complex least squares: no reflection is possible).  n = (float)|P|; every sum runs over P in ascending j and
 *   starts from 0.0f:
 *     qmx = (sum u_j) / n,  qmy = (sum v_j) / n,  pmx = (sum x_j) / n,  pmy = (sum y_j) / n
 *     dqx = u_j - qmx,  dqy = v_j - qmy,  dpx = x_j - pmx,  dpy = y_j - pmy
 *     A += (dqx * dpx) + (dqy * dpy);   B += (dqx * dpy) - (dqy * dpx);   D += (dqx * dqx) + (dqy * dqy)
 *   SKIPPED unless D > 0.   a = A / D,  b = B / D;   SKIPPED unless both are finite.   The crop's centre:
 *     ux = ((float)tw * 0.5f) - qmx,  uy = ((float)th * 0.5f) - qmy
 *     cx = pmx + ((a * ux) - (b * uy)),  cy = pmy + ((b * ux) + (a * uy))
 * Expand.  ae = a * expand,  be = b * expand  (expand == 0 means 1.0): the crop is scaled about its centre.
 * Size rule.  s = sqrtf((ae * ae) + (be * be));   we = s * (float)tw,  he = s * (float)th.  SKIPPED when we < min_size, he < min_size
 *   (min_size == 0 means 2), we > 32768, he > 32768, or the centre is outside the frame: unless 0 <= cx <= W and 0 <= cy <= H (a NaN centre
 *   is outside).  Behind this rule (and W, H <= 32767, which the calls require) every Q16 value below fits an int32.
 * Geometry, with q16(v) = (int)rintf(v * 65536.0f) (round to nearest even):
 *     ha = ae * 0.5f,  hb = be * 0.5f
 *     Ux = q16(ha),  Uy = q16(hb),  Vx = q16(-hb),  Vy = q16(ha),  X0 = q16(cx - 0.5f),  Y0 = q16(cy - 0.5f)
 *     nw = tw,  nh = th,  px = py = 0
 * Sampling.  From here the sample positions, the taps, the grey (111) taps outside the frame, the blend, the NV12 conversion and the layouts
 *   are exactly those of "Rotated crops" with these six integers.
 * Flags.  MARS_ROI_KEEP_ASPECT and MARS_ROI_AREA are refused (MARS_ERR_INVALID_FILE): the template fixes the geometry, the sampler has four taps.
 * ROI table.  frame as before; det = the pose record's det, the index in the frame's detection list, so the label, identify and track joins
 *   work unchanged (host-pointer form: -1).  x0 .. y1 is for the caller's information only, by the rule of "Rotated crops" around (cx, cy):
 *     ca = |ae| / s,  sa = |be| / s,  ex = ((we * ca) + (he * sa)) * 0.5f,  ey = ((we * sa) + (he * ca)) * 0.5f,
 *     x0 = (int)floorf(max(cx - ex, 0)),  x1 = (int)ceilf(min(cx + ex, (float)W)),  y0, y1 alike with cy, ey, H.
 *   A skipped box of the host-pointer form has all four zero.
 * Fit table.  Beside the ROI table one mars_align_t per slot: the six integers, used = the mask of P, n_used = |P|.  A skipped or empty slot
 *   is all zeros (a kept one has n_used >= 2).  It lets a caller map crop pixels back into the frame (the position formula of "Rotated
 *   crops") and see which keypoints carried the fit.
 * Selection (device chain).  Frame by frame the pose slots of det_model's last pose call are walked in slot order; a slot with det == -1
 *   ends its frame's list.  The slot's detection dets[f][det] must pass conf >= min_conf and the class window, and the box must not be
 *   skipped; the kept boxes of a frame stop at max_per_frame (0: no limit).  Kept boxes fill the destination's frames 0, 1, ... up to its
 *   batch, the rest are counted as dropped; destination frames behind the last crop are -17.  A function of the lists alone: no atomics.
 * Consequences.  4 participating points, template coordinates multiples of 1/4 and kpt = template + an integer shift: every sum is exact,
 *   a = 1 and b = 0 exactly, Ux = Vy = 32768, every fraction is 0 and the crop is an exact copy of the frame's pixels minus 128.  The same
 *   template turned a quarter turn about an integer centre: Ux = 0, Uy = 32768 and the crop is an exact transposed copy.  Exactness needs sums
 *   that are exact in float32; in general a is within rounding of 1 and the copy is not promised.
 * Contract.  The pose call was made with src_w / src_h set, so that keypoints and boxes are in camera pixels: what the other crop calls ask.
 * Refused.  MARS_ERR_INVALID_FILE, before any device work: what the calls of "Rotated crops" refuse about the options, the two flags, no
 *   align options, num_kpt outside 1 .. MARS_POSE_MAX_KPT, a `use` bit at or above num_kpt, a template value (of the first num_kpt) or a
 *   min_vis that is not finite.  MARS_ERR_INVALID_TENSOR: det_model holds no pose results (no mars_hip_detect_pose_device since its batch
 *   was set), K of that call != num_kpt, and what mars_hip_crop_obb_device refuses about the two models.
 * Not covered: the pipelined mars_hip_pipe_* path; affine or perspective fits; per-keypoint weights; area averaging; merged tile lists. */
typedef struct {
    int num_kpt;                            /* K: 1 .. MARS_POSE_MAX_KPT */
    float tmpl[MARS_POSE_MAX_KPT][2];       /* (u_j, v_j), target pixels; the first K are read */
    unsigned use;                           /* 0: all K */
    float min_vis;
} mars_hip_align_opts_t;
typedef struct { int X0, Y0, Ux, Uy, Vx, Vy; unsigned used; int n_used; } mars_align_t; /* 32 bytes */
/* Pure host code, no device: the fit of one keypoint set [K].  1 = kept (fit filled), 0 = skipped (fit zeroed), -1 = bad arguments (what is
 * "Refused" above about the options, no kpts, no fit).  roi may be NULL; only its x0 .. y1 are written (zeros for a skipped box). */
int mars_yolo_align_fit(const mars_kpt_t *kpts, const mars_hip_align_opts_t *align, const mars_hip_roi_opts_t *opts, int tw, int th,
                        mars_align_t *fit, mars_roi_t *roi);
/* The standard 5-point face template (the public ArcFace 112 x 112 positions: eyes, nose tip, mouth corners) scaled by tw / 112 and
 * th / 112 into tmpl[0 .. 4]; returns K = 5, or -1 without tmpl or with a non-positive size. */
int mars_yolo_align_template_face5(int tw, int th, float tmpl[][2]);
/* mars_yolo_crop_boxes for keypoint sets: host pointers in and out, runs on the GPU.  kpts = [n_boxes][K].  Only the skip rule applies; a
 * skipped box's crop is all -17, its ROI rectangle and its fit record are zeros.  rois and fits may be NULL. */
mars_error_t mars_yolo_crop_aligned(const unsigned char *frames, int n_frames, const mars_kpt_t *kpts, const int *frame_of_box, int n_boxes,
                                    const mars_hip_align_opts_t *align, const mars_hip_roi_opts_t *opts, int tw, int th, int nhwc,
                                    signed char *out, mars_roi_t *rois, mars_align_t *fits);
/* mars_hip_crop_detections_device over the keypoints the last mars_hip_detect_pose_device of det_model left in HBM.  Enqueues only; stream
 * and event ordering are exactly those of mars_hip_crop_detections_device (the pose stage's kernels run in front of the event that call
 * waits for), and mars_hip_roi_results serves this call too. */
mars_error_t mars_hip_crop_pose_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index,
                                       const mars_hip_roi_opts_t *opts, const mars_hip_align_opts_t *align);
/* The same with the frames in host memory: uploads them, crops, waits. */
mars_error_t mars_hip_crop_pose(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index,
                                const mars_hip_roi_opts_t *opts, const mars_hip_align_opts_t *align);
/* Waits.  The fit table of the last aligned crop call into dst_model, beside mars_hip_roi_results: min(cap, the batch of that call)
 * records, slot k beside ROI record k, zeros behind the kept ones.  MARS_ERR_INVALID_TENSOR unless the last crop call into dst_model was
 * an aligned one. */
mars_error_t mars_hip_align_results(mars_model_t *dst_model, mars_align_t *fits, int cap);

/* --------------------------------------------------------- Tiled inference */
/* Sliced inference for frames much larger than the graph input: a camera frame is cut into overlapping tiles, every tile is one frame of the
 * batch, and the per-tile detection lists are mapped back and merged on the device.  A batch of B frames with T = n_tiles needs B % T == 0;
 * it holds C = B / T camera frames, and model frame c * T + t is tile t of camera frame c.  The reference has no batch and no such step, so
 * nothing here restates it.  The merge is float32, every operation rounded on its own, no fused multiply-add, division correctly rounded:
 * everything is defined to the bit.
 *
 * Grid.       mars_tile_grid, per axis, with step = tile - overlap: the starts are k * step for every k >= 0 with k * step + tile < W, then one
 *             final start W - tile; a tile at least as large as the axis gives the single span [0, W).  Tiles are listed row-major, y outer
 *             and x inner.  1920 x 1080, 640 x 640 tiles, overlap 128: x-starts 0, 512, 1024, 1280, y-starts 0, 440: 8 tiles.  The calls take
 *             a TABLE, not a grid: a caller may append any other rectangle, typically the whole frame, so that objects larger than a tile
 *             are still seen.
 * Front-end.  Tile t of camera frame c is written into model frame c * T + t by the rules of "ROI crops" above: the crop rectangle is the
 *             tile's rectangle (no box arithmetic); the target geometry is stretch, or MARS_TILE_KEEP_ASPECT with the integer nw, nh, px, py
 *             rule and -17 bands; the "Resize" and "NV12 source" paragraphs apply; the layout is the one the input's format tag asks for.
 *             A tile whose size equals the input's gives pos = i * 256: an exact copy, pixel - 128.  MARS_TILE_AREA: the tile is resized by
 *             "Area averaging" of "ROI crops" (a whole-frame tile of 1920 x 1080 into 640 x 640 is a 3 x down-scale); a tile no larger than
 *             its target keeps its bytes, the exact copy included.  The merge calls accept the bit and ignore it.
 * Quota.      Tile t contributes the first q entries of its list, q = max_per_tile, or by default min(MARS_YOLO_MAX_DET,
 *             MARS_TILE_MAX_CAND / n_tiles); n_tiles * q <= MARS_TILE_MAX_CAND.  The entries beyond q are counted in `overflow`.
 * Validity.   An entry is dropped, and counted in `invalid`, when one of x, y, w, h, conf is not finite, or w <= 0, or h <= 0.
 * Map.        For a tile {x0, y0, x1, y1}: cw = x1 - x0, ch = y1 - y0, and nw, nh, px, py of the front-end's target geometry for the tw x th input:
 *               rx = (float)cw / (float)nw;   X = ((x - (float)px) * rx) + (float)x0;   Wd = w * rx;      Y, Hd alike with ry = (float)ch / (float)nh
 * Edge rule.  Only with edge_margin > 0.  l = X - (Wd * 0.5f), r = X + (Wd * 0.5f); tp, bt alike.  A side of the tile is interior when it is not
 *             on the frame border: x0 > 0, x1 < src_w, y0 > 0, y1 < src_h.  The entry is dropped, and counted in `edge`, when
 *             l - (float)x0 < edge_margin at an interior left side, (float)x1 - r < edge_margin at an interior right side, tp - (float)y0 <
 *             edge_margin at an interior top, or (float)y1 - bt < edge_margin at an interior bottom: a box cut by a tile edge is left to
 *             the neighbour that sees all of it.
 * Candidates. The remaining entries, numbered k = 0, 1, ... by ascending tile, then list index; each carries its tile t and list index i.
 *             `candidates` is their number.
 * Order.      Confidence descending, then k ascending: a strict total order.  Confidences compare as their float32 values, except that -0
 *             stands below +0 (the IEEE total order on finite values; detectors give none below their threshold).  This is deliberately NOT the
 *             reference demo's exchange-sort permutation, which the upright tails reproduce: no reference defines this step.
 * Suppression. Greedy in that order: a kept candidate a removes every later b with tile(a) != tile(b), equal classes (or any classes under
 *             MARS_TILE_AGNOSTIC) and m(a, b) > merge_thresh.  Candidates of one tile never remove each other: the tile's own NMS has decided
 *             those pairs.  With the mapped boxes, as in the detection tail (mars_yolo_nms):
 *               x1 = max(Xa - Wa / 2, Xb - Wb / 2);  y1 alike;  x2 = min(Xa + Wa / 2, Xb + Wb / 2);  y2 alike
 *               inter = max(0, x2 - x1) * max(0, y2 - y1)
 *               m = inter / ((((Wa * Ha) + (Wb * Hb)) - inter) + 1e-6f)                     (IoU, the default)
 *               m = inter / (fminf(Wa * Ha, Wb * Hb) + 1e-6f)                               (MARS_TILE_MATCH_IOS: intersection over the smaller)
 *             IOS catches a box cut by a tile edge that lies inside its full version.  A removed candidate removes nothing.  `suppressed`
 *             is the number removed.
 * Output.     The survivors in sorted order, the first MARS_YOLO_MAX_DET of them; the rest are counted in `truncated`.  Each gives a
 *             mars_det_t {X, Y, Wd, Hd, conf, cls} in camera pixels and an origin mars_tile_src_t {tile, det}.  Slots behind the last survivor
 *             are all-zero bytes.
 * Not covered: the mars_hip_pipe_* path; crop, label, identify, track, seg, pose and obb stages on merged lists (the host-list forms
 *   mars_yolo_crop_boxes and mars_yolo_track_lists take the merged lists); box fusion by averaging (WBF); per-camera-frame tile tables; more
 *   than MARS_TILE_MAX_CAND candidates per camera frame; float32 heads. */
typedef struct { int x0, y0, x1, y1; } mars_tile_t;   /* source pixels, half-open; 16 bytes */
typedef struct { int tile, det; } mars_tile_src_t;    /* 8 bytes: tile t, index inside that tile's list */
typedef struct { int candidates, overflow, invalid, edge, suppressed, truncated; } mars_tile_stats_t; /* 24 bytes */
#define MARS_TILE_MAX_TILES 64
#define MARS_TILE_MAX_CAND 2048
#define MARS_TILE_KEEP_ASPECT 1u
#define MARS_TILE_MATCH_IOS 2u
#define MARS_TILE_AGNOSTIC 4u
#define MARS_TILE_AREA 16u /* front-end: "Area averaging" of "ROI crops" */
/* Pure host code.  Writes the first min(count, cap) tiles (tiles may be NULL with cap 0) and returns the count, also when it exceeds cap;
 * -1: a non-positive size, a negative overlap, or overlap >= tile. */
int mars_tile_grid(int W, int H, int tile_w, int tile_h, int overlap_x, int overlap_y, mars_tile_t *tiles, int cap);
/* Zero-initialise; zero means default in every field but the frame size and the table. */
typedef struct {
    int src_w, src_h, src_format; unsigned src_flags;   /* camera frames, as mars_hip_roi_opts_t */
    int n_tiles; const mars_tile_t *tiles;              /* per camera frame, 1 .. MARS_TILE_MAX_TILES; copied by every call */
    unsigned flags;                                     /* MARS_TILE_KEEP_ASPECT | MARS_TILE_MATCH_IOS | MARS_TILE_AGNOSTIC | MARS_TILE_AREA */
    float merge_thresh;                                 /* 0: 0.5 */
    float edge_margin;                                  /* source pixels; 0: no edge rule */
    int max_per_tile;                                   /* 0: min(MARS_YOLO_MAX_DET, MARS_TILE_MAX_CAND / n_tiles) */
} mars_hip_tile_opts_t;
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: no options or a NULL table or pointer; n_tiles outside
 * 1 .. MARS_TILE_MAX_TILES; a tile that is empty or not inside [0, src_w) x [0, src_h); a non-positive frame or input size, an unknown format
 * or flag bit, odd NV12 sizes; a negative or non-finite merge_thresh or edge_margin, merge_thresh > 1; a negative max_per_tile, or n_tiles *
 * max_per_tile > MARS_TILE_MAX_CAND; (front-end) a frame or target too wide for the crop kernel (the limits of "ROI crops", those of MARS_ROI_AREA under MARS_TILE_AREA); (host-pointer forms) a non-positive n_frames,
 * n_frames * n_tiles > 65535, max_det outside 1 .. MARS_YOLO_MAX_DET.  MARS_ERR_INVALID_TENSOR: a batch that is no
 * multiple of n_tiles; an input that is not int8 with 3 channels; no detections in HBM; lists mapped with src_w > 0; *_results before any
 * merge; a model with an open pipe. */
/* Front-end.  `frames_dev` = C = batch / n_tiles camera frames of src_w x src_h, densely packed in HBM (RGB [h][w][3] or NV12).  Enqueues on
 * the library's current stream, like mars_hip_preprocess_device: behind an earlier run of the model, ahead of its next one. */
mars_error_t mars_hip_preprocess_tiles_device(mars_model_t *model, int input_index, const void *frames_dev, const mars_hip_tile_opts_t *opts);
/* The same with the frames in host memory: uploads them, runs, waits. */
mars_error_t mars_hip_preprocess_tiles(mars_model_t *model, int input_index, const unsigned char *frames, const mars_hip_tile_opts_t *opts);
/* Merge.  Reads the lists the last mars_hip_detect_device / _heads_device / _dfl_device of the model left in HBM; they must be in graph-input
 * pixels (the model records whether that tail ran with src_w > 0 and such lists are refused).  tw x th = the size of graph input 0.  Enqueues
 * only, on the auxiliary stream with the ordering of mars_hip_track_device: behind the tail, ahead of the model's next detect call.  The
 * merged arrays are the model's own: mars_hip_detect_results still returns the per-tile lists, byte for byte. */
mars_error_t mars_hip_merge_tiles_device(mars_model_t *model, const mars_hip_tile_opts_t *opts);
/* Waits.  dets = [C][MARS_YOLO_MAX_DET], counts = [C], origins = [C][MARS_YOLO_MAX_DET], stats = [C] of the last merge; any pointer may be NULL. */
mars_error_t mars_hip_tile_results(mars_model_t *model, mars_det_t *dets, int *counts, mars_tile_src_t *origins, mars_tile_stats_t *stats);
/* Camera frames C of the last merge on this model, the row count of what mars_hip_tile_results copies; 0: no merge yet (or no model). */
int mars_hip_tile_frames(mars_model_t *model);
/* mars_hip_merge_tiles_device + mars_hip_tile_results. */
mars_error_t mars_hip_merge_tiles(mars_model_t *model, const mars_hip_tile_opts_t *opts, mars_det_t *dets, int *counts, mars_tile_src_t *origins,
                                  mars_tile_stats_t *stats);
/* Device time (ms) of the last mars_hip_merge_tiles_device call's kernel, from events on the auxiliary stream; waits for it.  < 0: not available. */
float mars_hip_tile_ms(mars_model_t *model);
/* Host pointers in and out, the same kernels on the GPU without a model; they wait.  frames = n_frames camera frames, out = [n_frames * T]
 * [tw * th * 3] int8 ([th][tw][3] with nhwc != 0, else [3][th][tw]). */
mars_error_t mars_yolo_tile_frames(const unsigned char *frames, int n_frames, const mars_hip_tile_opts_t *opts, int tw, int th, int nhwc,
                                   signed char *out);
/* dets = [n_frames * T][max_det] in pixels of a tw x th input, 1 <= max_det <= MARS_YOLO_MAX_DET; counts = [n_frames * T], clamped to
 * 0 .. max_det.  out = [n_frames][MARS_YOLO_MAX_DET], out_counts = [n_frames], origins = [n_frames][MARS_YOLO_MAX_DET], stats = [n_frames];
 * origins and stats may be NULL. */
mars_error_t mars_yolo_merge_tiles(const mars_det_t *dets, const int *counts, int n_frames, int max_det, const mars_hip_tile_opts_t *opts,
                                   int tw, int th, mars_det_t *out, int *out_counts, mars_tile_src_t *origins, mars_tile_stats_t *stats);

/* --------------------------------------------------------------- Redaction */
/* Everything above reads camera frames; this writes them.  The first thing a camera deployment does with a person, face or plate detector is
 * hide what it found before a frame is encoded, stored or streamed.  The frames, the detections in frame pixels (mars_hip_detect_*_device
 * with src_w / src_h set), optionally the per-detection masks on the frame's own grid ("Instance masks in frame pixels") and the identity
 * hung on each detection ("Gallery match") are all in HBM after a batch; the calls below mosaic or fill the detected regions there, one
 * sparse pass over the pixels that change.  All integers except the rectangle rule, which is float32 and stated under "ROI crops".
 *
 * Frames.     F frames of W x H, densely packed (no row pitch): RGB [H][W][3] uint8, or NV12 as in "NV12 camera frames" (W, H even).
 *             src_format and src_flags mean what they mean in mars_hip_roi_opts_t.  Of the NV12 flags only MARS_NV12_VU matters, and only
 *             for the fill colour; MARS_NV12_FULL_RANGE is accepted and ignored: nothing is converted.
 * Regions.    Every selected detection gives one region.  Its rectangle R = (x0, y0, x1, y1) is "Box -> source rectangle" of "ROI crops"
 *             with the options' expand (0 means 1.0).  The region is SKIPPED when a float field is not finite, w <= 0, h <= 0, cw < 1 or
 *             ch < 1: there is no min_size here.  A region without a mask is all of R.  A region with a mask is the pixels of R whose bit
 *             is set in that detection's mask words: pixel x is bit x & 31 of word x >> 5 of its row, pitch = (W + 31) / 32 words, as in
 *             "Instance masks in frame pixels".  Bits outside R are ignored.
 * Union.      U(f) is the union of the regions of frame f.  A pixel is redacted iff it is in U; overlapping regions make no difference
 *             beyond that.
 * Cells.      cell = B in {2, 4, 8, 16, 32, 64}; 0 means 16.  Cell (cx, cy) is the pixels [cx * B, min(W, (cx + 1) * B)) x [cy * B,
 *             min(H, (cy + 1) * B)), anchored at the frame's origin, not at the box; n is its pixel count (edge cells are clipped).
 * Mosaic (mode MARS_REDACT_MOSAIC = 0, the default), RGB.  Per channel: S = the sum of the ORIGINAL bytes over the whole cell, whether or not
 *             those pixels are redacted; v = (S + n / 2) / n, floor -- the rounding of "Area averaging".  Every redacted pixel of the cell
 *             becomes v; every other byte keeps its value.
 * Mosaic, NV12.  The luma plane follows the RGB rule with one channel.  Chroma sample (i, j) covers the pixels (2i .. 2i + 1, 2j .. 2j + 1)
 *             and is redacted iff any of those four pixels is in U.  Its value is the rounded mean, by the same formula, of the original
 *             samples of its cell: cell (cx, cy) holds the chroma samples [cx * B / 2, ...) x [cy * B / 2, ...), clipped to the plane, n
 *             their count.  U and V are averaged separately.
 * Fill (mode MARS_REDACT_FILL = 1).  RGB: redacted pixels become fill[0 .. 2] = R, G, B.  NV12: redacted luma becomes fill[0], redacted
 *             chroma samples the pair U = fill[1], V = fill[2], stored V, U under MARS_NV12_VU.
 * Output.     In place (dst NULL or == the frames) or into a second buffer of the same size, of which every byte is written (unredacted
 *             bytes are copied).  A dst that overlaps the source without being equal to it is refused.  Either way the result is a function
 *             of the original frames alone.
 * Selection (device form).  Every listed detection is visited and every selected one counts; there is no cap below MARS_YOLO_MAX_DET.
 *             Selected: conf >= min_conf (0: all); cls_count == 0 or cls_first <= cls < cls_first + cls_count, as in "ROI crops"; under
 *             MARS_REDACT_SPARE_IDENTIFIED not the detections whose identity entry (mars_hip_identify_detections_device) has cls >= 0 and
 *             score >= ident_min -- "hide everyone who is not enrolled"; the flag needs identity results of this batch on the model.
 *             Under MARS_REDACT_USE_MASKS a selected detection that has a slot among the native mask results -- the mars_mask_t.det entries
 *             of the last mars_hip_detect_seg_native_device, whose grid must be W x H -- uses its mask; one without a slot falls back to
 *             its rectangle: the privacy-safe side is to hide more.
 * Statistics. Per frame {regions, masked, skipped, pixels}: the regions formed, how many of them used a mask, the selected detections
 *             the rectangle rule skipped, |U|.
 * Not covered: Gaussian blur; mask dilation; "only the identified"; selection by track id; oriented or keypoint-shaped regions; the merged
 *   lists of "Tiled inference"; the mars_hip_pipe_* path; frames with a row pitch. */
#define MARS_REDACT_MOSAIC 0
#define MARS_REDACT_FILL 1
#define MARS_REDACT_USE_MASKS 1u
#define MARS_REDACT_SPARE_IDENTIFIED 2u
/* Zero-initialise; zero means default in every field but the frame size. */
typedef struct {
    int src_w, src_h, src_format; unsigned src_flags; /* frames: MARS_HIP_CAMERA_RGB / _NV12, MARS_NV12_* (NV12 only) */
    int mode, cell; unsigned char fill[3];
    float expand, min_conf, ident_min;
    int cls_first, cls_count;
    unsigned flags;                                    /* MARS_REDACT_USE_MASKS | MARS_REDACT_SPARE_IDENTIFIED (the device form) */
} mars_hip_redact_opts_t;
typedef struct { int regions, masked, skipped, pixels; } mars_redact_stats_t; /* 16 bytes */
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: no options or a NULL pointer where one is needed, a
 * non-positive size, an unknown format, mode or flag bit, odd NV12 sizes, a cell outside the set, a negative or non-finite expand, min_conf
 * or ident_min, ident_min > 1, a negative cls_count, a dst that overlaps the source in part.  MARS_ERR_INVALID_TENSOR: W or H above 8192, no
 * detections in HBM, a model with an open pipe, MARS_REDACT_USE_MASKS without native mask results of this batch or with a mask grid that is
 * not W x H, MARS_REDACT_SPARE_IDENTIFIED without identity results of this batch. */
/* Host pointers in and out, the same kernels on the GPU; waits.  `frames` = n_frames frames of opts->src_w x src_h; box i lies in frame
 * frame_of_box[i] (a box whose index names no frame is left out).  Every box is taken: only the rectangle rule applies, opts->flags are not
 * looked at beyond the check.  mask_of_box = NULL, or [n_boxes]: an index into mask_words[.][H][(W + 31) / 32], or -1 for the rectangle alone.
 * n_boxes may be 0 (0 .. 65535, n_frames 1 .. 65535).  out = the redacted frames; out == frames runs the in-place form.  stats = [n_frames],
 * or NULL. */
mars_error_t mars_yolo_redact_frames(const unsigned char *frames, int n_frames, const mars_det_t *boxes, const int *frame_of_box, int n_boxes,
                                     const uint32_t *mask_words, const int *mask_of_box, const mars_hip_redact_opts_t *opts, unsigned char *out,
                                     mars_redact_stats_t *stats);
/* The device form.  Reads the detections the last mars_hip_detect_*_device of det_model left in HBM (in frame pixels) and redacts det_model's
 * batch of frames at frames_dev into dst_dev (NULL or == frames_dev: in place).  Enqueues only, on the auxiliary stream: behind the detection
 * tail, the native masks and the identity scatter, which that stream carries.  Ordering against the main stream, both ways: the redaction
 * first waits for an event recorded on the main stream at the call, so crops the library enqueued EARLIER from the same frames
 * (mars_hip_crop_*_device, mars_hip_preprocess*_device) read the original pixels; and it records an event the main stream waits for, so
 * library work enqueued LATER, and every *_results call, sees the redacted frames.  Work of the caller's own on other streams is the
 * caller's to order (mars_hip_sync). */
mars_error_t mars_hip_redact_device(mars_model_t *det_model, void *frames_dev, void *dst_dev, const mars_hip_redact_opts_t *opts);
/* Waits.  stats = [batch] of the last mars_hip_redact_device call (may be NULL: only waits).  MARS_ERR_INVALID_TENSOR before any such call. */
mars_error_t mars_hip_redact_results(mars_model_t *det_model, mars_redact_stats_t *stats);
/* The same with the frames in host memory, in place: uploads them, redacts, downloads them, waits. */
mars_error_t mars_hip_redact(mars_model_t *det_model, unsigned char *frames, const mars_hip_redact_opts_t *opts, mars_redact_stats_t *stats);
/* Device time (ms) of the last mars_hip_redact_device call (selection + pixels), from events on the auxiliary stream; waits for it.  < 0: not
 * available. */
float mars_hip_redact_ms(mars_model_t *det_model);

/* --------------------------------------------------------------- Overlay */
/* The counterpart of "Redaction": not hiding what was found but showing it -- box, label, track id, mask tint and keypoints painted into
 * the frame before it is encoded, stored or streamed.  Everything it draws is in HBM next to the frames after a batch: the detections in
 * frame pixels, the track ids ("Tracking"), the masks on the frame's own grid ("Instance masks in frame pixels") and the keypoints ("Pose
 * keypoints").  The reference draws on the host only, with PIL in a test script (mgk-decompiler/test_yolo_inference.py, draw_detections: a
 * rectangle and a text per box).  Everything that touches a pixel is integer arithmetic; the only float32 steps are the rectangle rule, the
 * confidence percentage and the keypoint floorf.
 *
 * Frames.     As in "Redaction": F frames of W x H (each at most 8192), densely packed, RGB [H][W][3] or NV12 (W, H even); src_format and
 *             src_flags as there.
 * Output.     In place (dst NULL or == the frames) or into a second buffer of the same size, of which every byte is written.  A dst that
 *             overlaps the source without being equal to it is refused.  Either way the result is a function of the original frames alone.
 * Palette.    P entries of RGB, 1 <= P <= 256, the caller's; palette == NULL: the built-in table of 16 (mars_overlay_default_palette):
 *               (255,64,64) (64,200,64) (64,128,255) (255,200,0) (255,0,255) (0,220,220) (255,128,0) (128,64,255)
 *               (160,255,64) (255,128,192) (0,128,128) (128,0,0) (0,0,160) (128,128,0) (192,192,192) (96,96,96)
 * NV12 colours.  For NV12 frames the host converts every colour once (mars_overlay_rgb_to_yuv; >> is an arithmetic shift, results clamped
 *             to 0 .. 255) and uploads the converted table; the kernels are format-blind about colour.  Limited range (the default):
 *               Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16, U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128, V = ((112 R - 94 G - 18 B + 128) >> 8) + 128;
 *             MARS_NV12_FULL_RANGE:
 *               Y = (77 R + 150 G + 29 B + 128) >> 8, U = ((-43 R - 85 G + 128 B + 128) >> 8) + 128, V = ((128 R - 107 G - 21 B + 128) >> 8) + 128.
 *             MARS_NV12_VU swaps the stored chroma pair.
 * Colour of a detection.  color_by = MARS_OVERLAY_BY_CLASS (0: key = cls), _BY_TRACK (key = the track id) or _FIXED (key = 0).  key >= 0:
 *             palette[key % P]; key < 0: the options' no_key colour.  The host-pointer form takes a key per box instead where it is given
 *             one; without keys, _BY_TRACK there gives every box the key -1.
 * Text colour.  Black where the luma (77 R + 150 G + 29 B + 128) >> 8 of the RGB colour under it is >= 128, else white.
 * Selection (device form).  conf >= min_conf (0: all) and the class window cls_first / cls_count, as in "Redaction"; with
 *             MARS_OVERLAY_TRACKED_ONLY only detections whose track entry has id >= 0 and hits >= min_hits (0 means 1).
 * Elements.   Every selected detection gives one element.  Its rectangle R = (x0, y0, x1, y1) is "Box -> source rectangle" of "ROI crops"
 *             with expand 1.0 and min_size 1.  A selected detection the rectangle rule skips counts in `skipped` and paints nothing.
 *             Elements keep the list's order; the element index below is the rank among the frame's elements.
 * Layers.     layers is a bit set of MARS_OVERLAY_MASKS, _BOXES, _KEYPOINTS, _LABELS; 0 means _BOXES | _LABELS.  Within a layer a pixel
 *             that several elements cover belongs to the one with the lowest element index -- for markers the lowest (element index,
 *             keypoint index); lists are sorted by confidence, so the most confident is on top.  Across layers: LABELS over KEYPOINTS over
 *             BOXES over MASKS over the source pixel.
 * MASKS (tint).  The pixels of R whose bit is set in the element's frame-pixel mask: the words of "Instance masks in frame pixels", pitch
 *             (W + 31) / 32.  An element without a mask slot has no tint.  Per channel out = (src * (256 - a) + col * a + 128) >> 8, a =
 *             alpha in 1 .. 256 (0 means 96), col the element's colour.
 * BOXES (outline).  The pixels of R that are not in (x0 + t, y0 + t, x1 - t, y1 - t); t = thickness in 1 .. 16 (0 means 2).  An empty
 *             inner rectangle makes all of R outline.  Opaque, the element's colour.
 * KEYPOINTS (markers).  Every keypoint j of an element that has a pose slot, with x and y finite and v >= kpt_min_v (0 means 0.5):
 *             cx = floorf(x), cy = floorf(y); the marker is dropped, before any conversion to int, when cx < -8.0f, cx > (float)(W + 8),
 *             cy < -8.0f or cy > (float)(H + 8); otherwise it is the square [cx - r, cx + r] x [cy - r, cy + r] cut to the frame (it may
 *             be empty then), r = radius in 1 .. 8 (0 means 2).  Opaque, colour palette[j % P].
 * LABELS.     A strip per element whose text has n > 0 bytes.  s = scale in 1 .. 8 (0 means 2); Wl = s * (6 n + 1), Hl = 9 s; lx = x0;
 *             ly = y0 - Hl where that is >= 0, else y0 (inside the box's top).  The strip [lx, lx + Wl) x [ly, ly + Hl) is cut to the
 *             frame.  For its pixel (x, y): u = x - lx - s, v = y - ly - s.  The pixel has the text colour when u >= 0, 0 <= v < 7 s,
 *             k = u / (6 s) < n, u % (6 s) < 5 s and bit 4 - (u % (6 s)) / s of row v / s of the glyph of byte k is set; every other pixel
 *             of the strip has the element's colour.  Opaque.
 * Font.       5 x 7, drawn for this project: 64 glyphs for the bytes 32 .. 95, seven row bytes each from the top, bit 4 the left column,
 *             bits 5 .. 7 clear (mars_overlay_glyph).  Bytes 96 .. 126 show the glyph of byte - 32 (lowercase shows as uppercase); every
 *             other byte shows as '?'.
 * Text (device form).  The parts that `text` chooses (MARS_OVERLAY_TEXT_CLASS | _TRACK | _CONF; 0 means _CLASS | _CONF), in that order,
 *             joined by one space; the first MARS_OVERLAY_TEXT_MAX bytes are kept.  CLASS: the bytes of names[cls] up to the first NUL
 *             where names is set, 0 <= cls < n_names and names[cls] is not empty, else the decimal of cls ('-' in front of a negative
 *             one).  names = n_names x MARS_OVERLAY_NAME_LEN bytes, NUL-padded (a name of exactly that length has no NUL), copied by
 *             every call.  TRACK: '#' and the decimal id; left out when id < 0.  CONF: p = (int)(conf * 100.0f + 0.5f), the two float32
 *             operations rounded on their own (no FMA), clamped to 0 .. 100 (a NaN gives 0); its decimal and '%'.  The device composes
 *             these bytes in the selection kernel; mars_overlay_text composes the same bytes on the host, with the same code.  The
 *             host-pointer form takes the label of a box from texts (up to the first NUL, at most MARS_OVERLAY_TEXT_MAX bytes) where it
 *             is given them, else composes it with id = -1.
 * NV12.       Luma is painted per pixel as above with the Y of every colour.  Chroma sample (i, j) follows pixel (2i, 2j): the chroma pair
 *             of the opaque element that owns that pixel, if any; else the tint's blend of both samples, if that pixel is tinted; else
 *             unchanged.
 * Statistics. Per frame {boxes, masked, labels, markers, skipped, pixels}: the elements; those with a mask slot (MASKS on); those with a
 *             text (LABELS on); the markers formed (KEYPOINTS on, dropped ones not counted); the selected detections the rectangle rule
 *             skipped; the frame pixels (luma positions) that any layer covers.
 * Not covered: skeleton limbs and any line drawing; oriented outlines; anti-aliasing; caller fonts and glyphs beyond the table; names of
 *   gallery identities; the mars_hip_pipe_* path; the merged lists of "Tiled inference"; frames with a row pitch. */
#define MARS_OVERLAY_MASKS 1u
#define MARS_OVERLAY_BOXES 2u
#define MARS_OVERLAY_KEYPOINTS 4u
#define MARS_OVERLAY_LABELS 8u
#define MARS_OVERLAY_BY_CLASS 0
#define MARS_OVERLAY_BY_TRACK 1
#define MARS_OVERLAY_FIXED 2
#define MARS_OVERLAY_TEXT_CLASS 1u
#define MARS_OVERLAY_TEXT_TRACK 2u
#define MARS_OVERLAY_TEXT_CONF 4u
#define MARS_OVERLAY_TRACKED_ONLY 1u
#define MARS_OVERLAY_TEXT_MAX 24
#define MARS_OVERLAY_NAME_LEN 16
#define MARS_OVERLAY_MAX_NAMES 4096
/* Zero-initialise; zero means default in every field but the frame size. */
typedef struct {
    int src_w, src_h, src_format; unsigned src_flags; /* frames: MARS_HIP_CAMERA_RGB / _NV12, MARS_NV12_* (NV12 only) */
    unsigned layers;                                   /* MARS_OVERLAY_MASKS | _BOXES | _KEYPOINTS | _LABELS */
    int color_by;                                      /* MARS_OVERLAY_BY_CLASS / _BY_TRACK / _FIXED */
    unsigned text;                                     /* MARS_OVERLAY_TEXT_CLASS | _TRACK | _CONF */
    int thickness, radius, scale, alpha;
    unsigned char no_key[3];                           /* R, G, B of a negative key */
    float min_conf, kpt_min_v;
    int cls_first, cls_count, min_hits;
    unsigned flags;                                    /* MARS_OVERLAY_TRACKED_ONLY (the device form) */
    int n_palette; const unsigned char *palette;       /* [n_palette][3] R, G, B; NULL (n_palette 0): the built-in table */
    int n_names; const char *names;                    /* [n_names][MARS_OVERLAY_NAME_LEN]; NULL (n_names 0): classes show as numbers */
} mars_hip_overlay_opts_t;
typedef struct { int boxes, masked, labels, markers, skipped, pixels; } mars_overlay_stats_t; /* 24 bytes */
/* Pure host code.  The built-in palette -> rgb = [16][3]; returns 16. */
int mars_overlay_default_palette(unsigned char *rgb);
/* Pure host code.  rgb = R, G, B -> yuv = Y and the chroma pair in its stored order (U, V; V, U under MARS_NV12_VU), by the formulas above;
 * flags = MARS_NV12_*. */
void mars_overlay_rgb_to_yuv(const unsigned char *rgb, unsigned flags, unsigned char *yuv);
/* Pure host code.  The seven rows of the glyph that `byte` shows as (any int: what is not 32 .. 126 shows as '?'). */
void mars_overlay_glyph(int byte, unsigned char rows[7]);
/* Pure host code.  The label of a detection as the device form composes it -> the number of bytes; out = MARS_OVERLAY_TEXT_MAX bytes, zero
 * behind the text.  text = MARS_OVERLAY_TEXT_* (0 means CLASS | CONF); names may be NULL; track_id < 0: untracked. */
int mars_overlay_text(unsigned text, const char *names, int n_names, int cls, int track_id, float conf, char *out);
/* Refused before any device work by every call below, in the order of "Redaction".  MARS_ERR_INVALID_FILE: no options or a NULL pointer
 * where one is needed, a non-positive size, an unknown format, layer, text, colour or flag bit, odd NV12 sizes, a thickness above 16, a
 * radius or scale above 8, an alpha above 256, any of them negative, a negative or non-finite min_conf or kpt_min_v, a negative cls_count
 * or min_hits, a palette of more than 256 or fewer than 1 entries or a count without a table, more than MARS_OVERLAY_MAX_NAMES names or a
 * count without a table, more than MARS_POSE_MAX_KPT keypoints a box, a dst that overlaps the source in part.  MARS_ERR_INVALID_TENSOR: W
 * or H above 8192, no detections in HBM, a model with an open pipe; where the options ask for them (MARS_OVERLAY_TRACKED_ONLY, _BY_TRACK or
 * _TEXT_TRACK; _MASKS; _KEYPOINTS): no track results of this batch, no native mask results of this batch or a mask grid that is not W x H,
 * no pose results of this batch. */
/* Host pointers in and out, the same kernels on the GPU; waits.  `frames` = n_frames frames of opts->src_w x src_h; box i lies in frame
 * frame_of_box[i] (a box whose index names no frame is left out).  Every box is taken: min_conf, the class window and opts->flags are not
 * looked at beyond the check.  Each of these may be NULL: keys = [n_boxes] colour keys; texts = [n_boxes][MARS_OVERLAY_TEXT_MAX] labels;
 * mask_of_box = [n_boxes] indices into mask_words[.][H][(W + 31) / 32], or -1 for no tint; kpts = [n_boxes][num_kpt] keypoints in frame
 * pixels (a box without any: v = 0).  n_boxes 0 .. 65535, n_frames 1 .. 65535.  out = the painted frames; out == frames runs the in-place
 * form.  stats = [n_frames], or NULL. */
mars_error_t mars_yolo_overlay_frames(const unsigned char *frames, int n_frames, const mars_det_t *boxes, const int *frame_of_box, int n_boxes,
                                      const int *keys, const char *texts, const uint32_t *mask_words, const int *mask_of_box, const mars_kpt_t *kpts,
                                      int num_kpt, const mars_hip_overlay_opts_t *opts, unsigned char *out, mars_overlay_stats_t *stats);
/* The device form.  Reads the detections the last mars_hip_detect_*_device of det_model left in HBM (in frame pixels) and paints det_model's
 * batch of frames at frames_dev into dst_dev (NULL or == frames_dev: in place).  Where the options ask for them it also reads the track
 * side array (mars_hip_track_device), the native mask results (mars_hip_detect_seg_native_device, whose grid must be W x H) and the pose
 * results (mars_hip_detect_pose_device with src_w / src_h set, so that the keypoints are in frame pixels); each must belong to this batch.
 * Enqueues only, on the auxiliary stream, with the redaction's event protocol in both directions: crops, front-end and motion the library
 * enqueued EARLIER have read the original pixels; library work enqueued LATER, and every *_results call, sees the painted ones.  An overlay
 * enqueued after a redaction paints over the redacted pixels.  The palette and the names are copied by the call: a call whose palette and
 * names differ from those of det_model's last overlay call waits for the device around their upload, every other call only enqueues. */
mars_error_t mars_hip_overlay_device(mars_model_t *det_model, void *frames_dev, void *dst_dev, const mars_hip_overlay_opts_t *opts);
/* Waits.  stats = [batch] of the last mars_hip_overlay_device call (may be NULL: only waits).  MARS_ERR_INVALID_TENSOR before any such call. */
mars_error_t mars_hip_overlay_results(mars_model_t *det_model, mars_overlay_stats_t *stats);
/* The same with the frames in host memory, in place: uploads them, paints, downloads them, waits. */
mars_error_t mars_hip_overlay(mars_model_t *det_model, unsigned char *frames, const mars_hip_overlay_opts_t *opts, mars_overlay_stats_t *stats);
/* Device time (ms) of the last mars_hip_overlay_device call (selection + pixels), from events on the auxiliary stream; waits for it.  < 0:
 * not available. */
float mars_hip_overlay_ms(mars_model_t *det_model);

/* --------------------------------------------------------------- Motion */
/* The first question a camera deployment asks of a frame: did anything move, and where?  The frames are in HBM for the front-end, the crops
 * and the redaction; the calls below read each of them once more (the Y plane of an NV12 frame, every byte of an RGB frame) and keep a
 * background per camera stream on the device, like the trackers keep their tables.  They tell a parked car from a moving one, idle streams
 * and tiles from busy ones, and count motion inside intrusion zones.  All integers except the rectangle rule, which is float32 and stated
 * under "ROI crops".
 *
 * Detector.   mars_hip_motion_t is made for S streams (1 .. 65535) of W x H frames (each at most 8192, as in "Redaction"), a format
 *             (MARS_HIP_CAMERA_RGB or _NV12; NV12 sizes are even; nothing is converted, so no NV12 flag matters) and a cell size B in
 *             {4, 8, 16, 32, 64}; 0 means 16.  Frames are densely packed, as in "Redaction".
 * Grid.       gw = (W + B - 1) / B, gh alike.  Cell (cx, cy) is the pixels [cx * B, min(W, (cx + 1) * B)) x [cy * B, min(H, (cy + 1) * B)),
 *             anchored at the frame's origin; n is its pixel count (edge cells are clipped).  Per stream the detector holds in HBM
 *             bg[gh][gw] as uint16 and an `initialised` flag.
 * Luma.       NV12: the Y byte.  RGB: (77 R + 150 G + 29 B + 128) >> 8, which is 0 .. 255.
 * Cell mean.  S = the sum of luma over the cell; m = (256 * S + n / 2) / n, floor: 8.8 fixed point, 0 .. 65280.
 * Frames -> streams.  The rule of "Tracking": F % S == 0; by default frame f is stream f % S, step f / S; with MARS_MOTION_STREAM_MAJOR
 *             stream f / (F / S), step f % (F / S).  A stream's steps are processed in ascending order; streams and cells are independent.
 *             One call over 2T steps leaves exactly the state and the outputs of two calls over T steps each.
 * Step, per cell.  Not initialised: bg = m, raw = 0 and the frame's `first` is 1; the stream is initialised after the step.  Initialised:
 *             delta = m - bg, raw = |delta| > 256 * threshold (1 .. 255; 0 means 8).  Then k = raw ? learn_active : learn (1 .. 16 each; 0
 *             means 4 and 8) and bg += sign(delta) * (|delta| >> k): an active cell is absorbed slowly.  A shift of 16 freezes the cell,
 *             since |delta| < 65536.  The shift truncates toward zero, so bg stalls within 2^k - 1 of m; this is by design.  Under
 *             MARS_MOTION_FRAME_DIFF bg = m after the comparison and the shifts are not looked at: plain frame differencing.
 * Filter.     active(cx, cy) = raw && (the number of raw cells among the up to 8 neighbours inside the grid >= min_neighbors); 0 .. 8, 0
 *             means no filter.  The background update uses raw, not active.
 * Map.        Per frame gh rows of pitch = (gw + 31) / 32 uint32 words; cell cx is bit cx & 31 of word cx >> 5, as in "Instance masks in
 *             frame pixels".  Bits at cx >= gw are zero.
 * Statistics. Per frame {active, x0, y0, x1, y1, first}: the number of active cells and their bounding box in pixels, x0 = min cx * B,
 *             x1 = min(W, (max cx + 1) * B), y alike; all four 0 without an active cell.
 * Zones.      Up to MARS_MOTION_MAX_ZONES rectangles of mars_tile_t ("Tiled inference"): half-open source pixels, not empty, inside the
 *             frame, so a tile table can be passed as it is.  zone_counts[f][z] = the number of active cells with cx in
 *             [x0 / B, (x1 - 1) / B] and cy in [y0 / B, (y1 - 1) / B]: the cells whose pixels meet the zone.
 * Detections. For frame f of a detection list and the map of frame f of the last motion call: the box's rectangle is "Box -> source
 *             rectangle" of "ROI crops" with expand (0 means 1.0) and min_size 1, its cells are those the zone rule gives for that
 *             rectangle, and the result is mars_motion_det_t {active, cells}.  A box the rule skips, and every entry behind the list, is
 *             {0, 0}.  The caller decides what share of the cells means "moving".
 * Not covered: device-side gating or compaction of the model batch; per-pixel models (MOG, ViBe); adaptive thresholds; camera-shake
 *   compensation; frames with a row pitch; the mars_hip_pipe_* path; the merged lists of "Tiled inference". */
#define MARS_MOTION_MAX_ZONES 64
#define MARS_MOTION_STREAM_MAJOR 1u
#define MARS_MOTION_FRAME_DIFF 2u
typedef struct mars_hip_motion mars_hip_motion_t; /* opaque */
/* Zero-initialise; zero means default in every field. */
typedef struct {
    int threshold, learn, learn_active, min_neighbors;
    unsigned flags;                                    /* MARS_MOTION_STREAM_MAJOR | MARS_MOTION_FRAME_DIFF */
    int n_zones; const mars_tile_t *zones;             /* 0 .. MARS_MOTION_MAX_ZONES; copied by every call */
} mars_hip_motion_opts_t;
typedef struct { int active, x0, y0, x1, y1, first; } mars_motion_stats_t; /* 24 bytes */
typedef struct { int active, cells; } mars_motion_det_t;                   /* 8 bytes */
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: NULL where a pointer is needed; a non-positive size, stream or
 * frame count; a cell outside the set; a threshold, shift, min_neighbors or zone count out of range; an unknown flag or format; odd NV12
 * sizes; a zone that is empty or not inside the frame; a negative or non-finite expand.  MARS_ERR_INVALID_TENSOR: W or H above 8192, more
 * than 65535 streams, F % S != 0, a stream out of range, *_results with nothing pending, no detections in HBM, a batch different from the
 * last motion call's F, a model with an open pipe.  A refused call leaves the detector's state as it was. */
mars_error_t mars_hip_motion_create(int streams, int w, int h, int format, int cell, mars_hip_motion_t **out);
mars_error_t mars_hip_motion_reset(mars_hip_motion_t *m, int stream);   /* that stream not initialised again; -1: all of them; waits */
void         mars_hip_motion_free(mars_hip_motion_t *m);                /* waits for the device first */
/* Pure host code: the grid of W x H frames at that cell size.  Any pointer may be NULL. */
mars_error_t mars_hip_motion_grid(int w, int h, int cell, int *gw, int *gh, int *pitch);
/* Waits.  bg = [gh][gw] of that stream (meaningless until it is initialised), *initialised = its flag; either may be NULL. */
mars_error_t mars_hip_motion_read(mars_hip_motion_t *m, int stream, uint16_t *bg, int *initialised);
/* Host pointers in and out, the same kernels on the GPU; waits.  frames = n_frames frames; maps = [n_frames][gh][pitch], stats = [n_frames],
 * zone_counts = [n_frames][n_zones]; any of the three may be NULL. */
mars_error_t mars_yolo_motion_frames(mars_hip_motion_t *m, const unsigned char *frames, int n_frames, const mars_hip_motion_opts_t *opts,
                                     uint32_t *maps, mars_motion_stats_t *stats, int *zone_counts);
/* The device form: n_frames frames at frames_dev.  Enqueues only, on the library's current stream, like mars_hip_preprocess_device.  A
 * redaction enqueued LATER on the same frames first waits for that stream, so motion has read the original pixels; one enqueued EARLIER has
 * made that stream wait for it, so motion sees the redacted ones. */
mars_error_t mars_hip_motion_device(mars_hip_motion_t *m, const void *frames_dev, int n_frames, const mars_hip_motion_opts_t *opts);
/* Waits.  The arrays of the last mars_hip_motion_device call, as in mars_yolo_motion_frames; any pointer may be NULL. */
mars_error_t mars_hip_motion_results(mars_hip_motion_t *m, uint32_t *maps, mars_motion_stats_t *stats, int *zone_counts);
/* Reads the lists the last mars_hip_detect_*_device of det_model left in HBM, boxes taken as frame pixels, against the maps of m's last
 * call, whose F must equal the batch.  Enqueues only, on the auxiliary stream with the label scatter's ordering: behind the detection tail
 * and behind the motion kernels the main stream has been given, ahead of the model's next detect call; m's next motion call waits for it.
 * The result array lives on det_model beside the tracks. */
mars_error_t mars_hip_motion_detections_device(mars_model_t *det_model, mars_hip_motion_t *m, float expand);
/* Waits.  out = [batch][MARS_YOLO_MAX_DET]: entry i of frame f belongs to detection i of mars_hip_detect_results. */
mars_error_t mars_hip_motion_det_results(mars_model_t *det_model, mars_motion_det_t *out);
/* The host-list form, against the maps of m's last call; waits.  Box i lies in frame frame_of_box[i]; one whose index names no frame gives
 * {0, 0}.  out = [n_boxes]. */
mars_error_t mars_yolo_motion_boxes(mars_hip_motion_t *m, const mars_det_t *boxes, const int *frame_of_box, int n_boxes, float expand,
                                    mars_motion_det_t *out);
/* Device time (ms) of the last mars_hip_motion_device call's two kernels, from events on its stream; waits for it.  < 0: not available. */
float mars_hip_motion_ms(mars_hip_motion_t *m);

/* --------------------------------------------------------------- Events */
/* What a deployment does with a track id: count objects over a line in each direction, know who is inside a zone, and raise an event when
 * something enters, leaves or stays too long.  "Motion" has zones but counts cells without memory; "Tracking" has memory but no geometry.
 * An events object holds, per camera stream and in HBM like the trackers' tables, the stream's rules, a table of MARS_TRACK_SLOTS slots, a
 * step counter that starts at 0 and running totals.  A call reads a batch's detection lists and track ids and leaves a record per
 * detection and counts per frame.  float32 appears only in the anchor, every operation rounded on its own, no fused multiply-add; from the
 * quantised anchor on everything is integers, and everything is defined to the bit:
 *
 * Rules of a stream.  Up to MARS_EVENTS_MAX_LINES directed segments A -> B with A != B, and up to MARS_EVENTS_MAX_ZONES polygons of 3 ..
 *   MARS_EVENTS_MAX_VERTS vertices each with a `dwell` step count (0: no dwell event).  Every coordinate is integer pixels in [-32768, 32768];
 *   a polygon need not be convex or simple (the even-odd rule below decides).  Vertices are multiplied by 16 to meet the anchors.
 * Slot.  {id, last_step, qx, qy, inside, dwelled, since[MARS_EVENTS_MAX_ZONES]}: the track id (0: the slot is free), the step it was last
 *   seen at, its anchor then, the mask of the zones it was inside then, the mask of the zones whose dwell event has fired since it entered,
 *   and per zone the step it entered at.
 * Frames -> streams.  The rule of "Tracking": a call over F frames and an object of S streams needs F % S == 0.  Default: frame f is stream
 *   f % S, step f / S.  MARS_EVENTS_STREAM_MAJOR: stream f / (F / S), step f % (F / S).  A stream's steps are processed in ascending order;
 *   streams are independent.  State persists between calls: one call over 2 T steps leaves exactly the state and outputs of two calls over
 *   T steps each.
 * Participants of a frame with lists d[0 .. n), tr[0 .. n).  Entry i is a CANDIDATE when tr[i].id >= 1, tr[i].hits >= min_hits and d[i].x,
 *   y, w, h are all finite.  A candidate whose id an earlier candidate (a lower index) of the frame brings too adds to `duplicates`; the
 *   others are the PARTICIPANTS.  The first MARS_TRACK_MAX_CAND participants by index are used, the rest add to `overflow`.  The record of
 *   every entry that is not a used participant, up to the array's width, is all zero.
 * Anchor.  ax = x;  ay = y, or under MARS_EVENTS_ANCHOR_BOTTOM ay = y + h * 0.5f (one multiply, one add).  For a in (ax, ay):
 *   c = fminf(fmaxf(a, -32768.0f), 32768.0f);  q = (int)floorf(c * 16.0f).  Q = (qx, qy), |q| <= 2^19.
 * Step, in this order, `step` being the stream's counter:
 *   1 Expiry.  Every used slot with step - last_step > max_gap is freed; `expired` grows by one and each zone of its `inside` adds one to
 *     that zone's `lost`.
 *   2 Lookup.  A used participant takes the slot that holds its id.  Those without one, by ascending index, take the free slots by ascending
 *     slot (slots freed in 1 count as free).  With no free slot `dropped` grows by one and the record is all zero.
 *   3 First sight (a slot just taken).  id = the participant's, qx, qy = Q, inside = zones(Q), since[z] = step for those zones, dwelled = 0;
 *     `first` grows by one.  The record is {zones = inside, everything else 0}: no enter event and no crossing.
 *   4 Seen again, P = (qx, qy) of the slot.  All products are int64 (the operands are below 2^21).  cross(u, v) = u.x * v.y - u.y * v.x.
 *     Lines.  side(X) = cross(B - A, X - A) >= 0.  Line l is crossed when side(P) != side(Q) and
 *       (cross(Q - P, A - P) >= 0) != (cross(Q - P, B - P) >= 0); it is `in` when side goes 0 -> 1 and `out` otherwise.  Both tests are
 *       half-open: a point on the line is on the positive side, and a path through an end point counts for exactly one of two segments
 *       that continue each other through it.  P == Q crosses nothing.
 *     Zones, the even-odd crossing number.  For every edge (V, W) of the polygon in order, the last vertex closing back to the first: if
 *       (V.y > Q.y) != (W.y > Q.y) then d = W.y - V.y, lhs = (Q.x - V.x) * d, rhs = (W.x - V.x) * (Q.y - V.y), and the parity toggles when
 *       d > 0 ? lhs < rhs : lhs > rhs.  now = the mask of the zones with odd parity (this is zones(Q) of 3 as well).
 *     Events.  entered = now & ~inside, exited = inside & ~now.  since[z] = step for the entered zones; the `dwelled` bits of entered and
 *       exited zones are cleared.  For z in now with dwell[z] > 0, step - since[z] >= dwell[z] and the bit clear in `dwelled`: the dwell
 *       event fires and the bit is set, so it fires once per stay.  Then inside = now, qx, qy = Q.  The record is {zones = now, entered,
 *       exited, dwelled = the events fired in this step, lines_in, lines_out}.
 *     A track seen again after a gap of at most max_gap steps is judged over the whole gap: P is where it was last seen.
 *   5 last_step = step for every slot seen.  Then step += 1.
 * Counts.  line_counts[f][l] = {in, out}: the number of the frame's records with bit l in lines_in, in lines_out.  zone_counts[f][z] =
 *   {inside, entered, exited, dwelled}: likewise over zones, entered, exited, dwelled.  Both arrays are MARS_EVENTS_MAX_LINES and _ZONES
 *   wide whatever the stream's rules hold; the rest is zero.
 * Totals, per stream since the last reset, int64: per line {in, out}; per zone {entered, exited, dwelled, lost}; the counters {first,
 *   expired, overflow, dropped, duplicates}.
 * Not covered: the mars_hip_pipe_* path; the merged lists of "Tiled inference"; polylines as one rule (give one line per segment: the
 *   half-open tests make them add up); zones from masks or oriented boxes; per-class rules; speed; an event queue (the caller reads the
 *   records and the counts); more than 2^31 steps per stream. */
#define MARS_EVENTS_MAX_LINES 32
#define MARS_EVENTS_MAX_ZONES 32
#define MARS_EVENTS_MAX_VERTS 8
#define MARS_EVENTS_STREAM_MAJOR 1u
#define MARS_EVENTS_ANCHOR_BOTTOM 2u
typedef struct { int ax, ay, bx, by; } mars_event_line_t;                                                   /* 16 bytes */
typedef struct { int n, dwell; int x[MARS_EVENTS_MAX_VERTS], y[MARS_EVENTS_MAX_VERTS]; } mars_event_zone_t;   /* 72 bytes */
typedef struct {
    int n_lines, n_zones;
    mars_event_line_t lines[MARS_EVENTS_MAX_LINES];
    mars_event_zone_t zones[MARS_EVENTS_MAX_ZONES];
} mars_hip_event_rules_t;                                                                                   /* 2824 bytes */
typedef struct { uint32_t zones, entered, exited, dwelled, lines_in, lines_out; } mars_event_t;             /* 24 bytes */
typedef struct { int id, last_step, qx, qy; uint32_t inside, dwelled; int since[MARS_EVENTS_MAX_ZONES]; } mars_event_slot_t; /* 152 bytes */
/* Zero-initialise; zero means default in every field. */
typedef struct {
    int max_gap;           /* 0: 30 */
    int min_hits;          /* 0: 1 */
    unsigned flags;        /* MARS_EVENTS_STREAM_MAJOR | MARS_EVENTS_ANCHOR_BOTTOM */
} mars_hip_events_opts_t;
typedef struct mars_hip_events mars_hip_events_t; /* opaque */
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: NULL where a pointer is needed; non-positive streams, frames
 * or max_det; a negative option; an unknown flag; a line or zone count out of range; a vertex count outside 3 .. MARS_EVENTS_MAX_VERTS; a
 * coordinate outside +-32768; a line with A == B; a negative dwell.  MARS_ERR_INVALID_TENSOR: streams above 65535, max_det above
 * MARS_YOLO_MAX_DET, F % S != 0, a stream out of range, no detections or no track results in HBM, *_results with nothing pending, a model
 * with an open pipe.  A refused call leaves the state as it was. */
mars_error_t mars_hip_events_create(int streams, mars_hip_events_t **out);       /* 1 .. 65535; no rules on any stream */
void         mars_hip_events_free(mars_hip_events_t *ev);                        /* waits for the device first */
/* That stream's table empty, its step and totals zero, its rules kept; -1: all streams; waits. */
mars_error_t mars_hip_events_reset(mars_hip_events_t *ev, int stream);
/* Waits, copies the rules and resets that stream; -1: all streams. */
mars_error_t mars_hip_events_set_rules(mars_hip_events_t *ev, int stream, const mars_hip_event_rules_t *rules);
/* Waits.  The totals and counters of one stream, the number of used slots and the step counter; any pointer may be NULL. */
mars_error_t mars_hip_events_read(mars_hip_events_t *ev, int stream, long long line_totals[MARS_EVENTS_MAX_LINES][2],
                                  long long zone_totals[MARS_EVENTS_MAX_ZONES][4], long long counters[5], int *n_used, int *step);
/* Waits.  The table of one stream, slots = [MARS_TRACK_SLOTS], in canonical form: a free slot is all zero, and since[z] is zero for every
 * zone the slot is not inside (nothing reads those). */
mars_error_t mars_hip_events_read_slots(mars_hip_events_t *ev, int stream, mars_event_slot_t *slots);
/* The mars_yolo_track_lists of this feature: host pointers in and out, runs the same kernel on the GPU and waits.  dets, tracks and records
 * are [frames][max_det], 1 <= max_det <= MARS_YOLO_MAX_DET; counts = [frames] (clamped to 0 .. max_det); line_counts =
 * [frames][MARS_EVENTS_MAX_LINES][2] and zone_counts = [frames][MARS_EVENTS_MAX_ZONES][4], either may be NULL. */
mars_error_t mars_yolo_event_lists(mars_hip_events_t *ev, const mars_det_t *dets, const mars_track_t *tracks, const int *counts, int frames, int max_det,
                                   const mars_hip_events_opts_t *opts, mars_event_t *records, int *line_counts, int *zone_counts);
/* Reads the detection lists and the track array the last mars_hip_track_device or mars_hip_track_app_device left on det_model in HBM (F =
 * its batch).  Enqueues only, on the auxiliary stream with the label scatter's ordering: behind the tracker, ahead of the model's next
 * detect call.  The record array lives on det_model beside the tracks and is freed with the model; the per-frame counts live on ev. */
mars_error_t mars_hip_events_device(mars_model_t *det_model, mars_hip_events_t *ev, const mars_hip_events_opts_t *opts);
/* Waits.  records = [batch of det_model][MARS_YOLO_MAX_DET]: entry i of frame f belongs to dets[f][i] of mars_hip_detect_results; the counts
 * as in mars_yolo_event_lists.  Any of the three may be NULL.  ev must be the object of det_model's last mars_hip_events_device call. */
mars_error_t mars_hip_events_results(mars_model_t *det_model, mars_hip_events_t *ev, mars_event_t *records, int *line_counts, int *zone_counts);
/* mars_hip_events_device + mars_hip_events_results. */
mars_error_t mars_hip_events(mars_model_t *det_model, mars_hip_events_t *ev, const mars_hip_events_opts_t *opts, mars_event_t *records,
                             int *line_counts, int *zone_counts);
/* Device time (ms) of the last call's kernel (either form), from events on its stream; waits for it.  < 0: not available. */
float mars_hip_events_ms(mars_hip_events_t *ev);

/* ------------------------------------------------------------ Best shots */
/* What a track looked like.  Every deployment that keeps track ids stores one picture per track: the frame in which the object was
 * largest, sharpest and most confidently seen.  The crops (the second model's input, as the crop calls wrote it), the join from crop to
 * detection (the ROI table) and the track ids are in HBM already; a shots object adds, per camera stream and in HBM, a table of `slots`
 * entries, a pixel plane [slots][tw * th * 3] int8 in the crops' layout, a step counter that starts at 0 and counters.  A call measures
 * every crop, keeps the best crop of every live track with its pixels, and hands a track's picture over once the track has ended.
 * Everything is integer arithmetic apart from one float-to-int conversion of the confidence, and everything is defined to the byte:
 *
 * Crop.  tw * th * 3 int8 bytes as the crop kernels write them: the pixel minus 128, [th][tw][3] (nhwc) or [3][th][tw].  u = byte + 128,
 *   0 .. 255, is the pixel.  ROI entry k = {frame, det, x0, y0, x1, y1} belongs to crop k; cw = x1 - x0, ch = y1 - y0 (differences and
 *   every product below in int64).
 * Content rectangle [px, px + nw) x [py, py + nh) of the target.  Without MARS_SHOT_KEEP_ASPECT the whole target: px = py = 0, nw = tw,
 *   nh = th.  With it, the integer rule of "ROI crops", "Target geometry", / floor:
 *     cw * th >= ch * tw:  nw = tw, nh = max(1, (ch * tw + cw / 2) / cw);   otherwise:  nh = th, nw = max(1, (cw * th + ch / 2) / ch);
 *     px = (tw - nw) / 2, py = (th - nh) / 2.
 *   A crop whose entry has x1 <= x0 or y1 <= y0, or a frame outside the call's frames, has NO CONTENT.
 * Luma.  Y = (77 * R + 150 * G + 29 * B + 128) >> 8 of the pixel's u values, 0 .. 255.
 * Metrics of a crop.  mean = (sum of Y over the content) / (nw * nh), / floor.  For every content pixel whose four neighbours lie inside
 *   the content:  L = 4 * Y(x, y) - Y(x - 1, y) - Y(x + 1, y) - Y(x, y - 1) - Y(x, y + 1), |L| <= 1020;
 *   sharp = (sum of L * L, int64) / ((nw - 2) * (nh - 2)), 0 when nw < 3 or nh < 3; sharp <= 1 040 400.  No content: mean = sharp = 0.
 * Score, int64 factors.  a = min(cw * ch, tw * th): source pixels beyond the target's size add nothing.
 *   c = (int)floorf(fminf(fmaxf(conf, 0.0f), 1.0f) * 1024.0f), the product rounded once, no fused multiply-add; a non-finite conf gives
 *   c = 0.  score = a * (sharp + 1) * c < 2^52.
 * Frames -> streams.  The rule of "Tracking": a call over F frames and an object of S streams needs F % S == 0.  Default: frame f is stream
 *   f % S, step f / S.  MARS_SHOT_STREAM_MAJOR: stream f / (F / S), step f % (F / S).  Every frame is a step of its stream even when it has
 *   no crop.  A stream's steps are processed in ascending order; streams are independent.  State persists between calls: one call over 2 T
 *   steps leaves exactly the state, plane and outputs of two calls over T steps each.
 * Candidates of a step.  Crops are visited by ascending crop index k.  Crop k is a CANDIDATE when k < kept (the number of crops written),
 *   its frame maps to this step, it has content, track.id >= 1 and track.hits >= min_hits, min_mean <= mean <= max_mean (0 in both fields:
 *   no window), sharp >= min_sharp and, under MARS_SHOT_INSIDE, its rectangle touches no border of the src_w x src_h frame: x0 > 0, y0 > 0,
 *   x1 < src_w, y1 < src_h.  A candidate whose id a candidate with a lower index of the same step brings too adds to `duplicates`.  The
 *   first MARS_TRACK_MAX_CAND of the remaining ones are the PARTICIPANTS, the others add to `overflow`.
 * Step, in this order, `step` being the stream's counter:
 *   1 Expiry.  Every LIVE slot with step - last_step > max_gap becomes DONE and keeps its shot; `finished` grows by one per slot.
 *   2 Lookup.  A participant takes the LIVE slot that holds its id.  Those without one, by ascending index, each take the lowest FREE slot;
 *     if there is none the lowest DONE slot (slots that 1 just finished included), whose shot is overwritten: `lost` grows by one; if there
 *     is none of either `dropped` grows by one and the crop's record names slot -1.
 *   3 First sight (a slot just taken).  The slot becomes LIVE: id, first_step = best_step = step, seen = taken = 1, the metrics, the
 *     score, conf, cls and the rectangle of this crop, and its pixels.
 *   4 Seen again.  seen += 1.  If score > the slot's score (strictly: a tie keeps the older shot) the slot takes this crop's metrics,
 *     score, conf, cls, rectangle, best_step = step and pixels, and taken += 1.
 *   5 last_step = step for every slot seen.  Then step += 1.
 *   The counter `taken` grows by one for every crop 3 or 4 stored.
 * Record per crop, mars_shot_t.  Every crop k < kept with content gets its metrics and its score, tracked or not; slot = the table slot of a
 *   participant that found one, else -1; taken = 1 where 3 or 4 stored the crop.  Entries at k >= kept and crops without content are
 *   {0, 0, 0, -1, 0}.
 * Slot, mars_shot_slot_t.  state: 0 FREE, 1 LIVE, 2 DONE.  A FREE slot reads back all zero.  Only mars_hip_shots_collect and a reset free
 *   a slot.
 * Not covered: the mars_hip_pipe_* path; MARS_SHOT_KEEP_ASPECT behind a rotated or aligned crop call (those calls have their own geometry:
 *   crop with stretch there); crops cut at a resolution of the shots object's own (the thumbnail is the second model's input); weights in
 *   the score; pose or frontality terms in the score; more than one shot per track; a second-model input kept at a row pitch (refused); a
 *   host write into the second model's input while a shots call is pending (wait first: only the crop calls wait by themselves); more than
 *   2^31 steps per stream. */
#define MARS_SHOT_STREAM_MAJOR 1u
#define MARS_SHOT_KEEP_ASPECT 2u
#define MARS_SHOT_INSIDE 4u
#define MARS_SHOT_FREE 0
#define MARS_SHOT_LIVE 1
#define MARS_SHOT_DONE 2
typedef struct { long long score; int sharp, mean, slot, taken; } mars_shot_t;                               /* 24 bytes */
typedef struct {
    int id, state, first_step, last_step, best_step, seen, taken, cls;
    float conf;
    int x0, y0, x1, y1, sharp, mean, pad;
    long long score;
} mars_shot_slot_t;                                                                                          /* 72 bytes */
/* Zero-initialise; zero means default in every field. */
typedef struct {
    int max_gap;            /* 0: 30 */
    int min_hits;           /* 0: 1 */
    int min_mean, max_mean; /* 0 .. 255, min_mean <= max_mean; both 0: no window */
    int min_sharp;
    int src_w, src_h;       /* the frames' size: needed by MARS_SHOT_INSIDE only */
    unsigned flags;         /* MARS_SHOT_STREAM_MAJOR | MARS_SHOT_KEEP_ASPECT | MARS_SHOT_INSIDE */
} mars_hip_shot_opts_t;                                                                                      /* 32 bytes */
typedef struct mars_hip_shots mars_hip_shots_t; /* opaque */
/* Refused before any device work by every call below.  MARS_ERR_INVALID_FILE: NULL where a pointer is needed; non-positive streams, slots,
 * sizes, crops or frames; a negative option; a mean outside 0 .. 255 or min_mean > max_mean; an unknown flag; MARS_SHOT_INSIDE without
 * src_w and src_h; a negative cap.  MARS_ERR_INVALID_TENSOR: streams above 65535, slots above MARS_TRACK_SLOTS, tw or th above 1280, more
 * than 65535 crops, F % S != 0, a stream or slot out of range, the pixels of a FREE slot, det_model == src_model, a model with an open
 * pipe, no detections or no track results in HBM, no crop call into src_model out of this det_model, an input that is not int8 with 3
 * channels, is kept at a row pitch (mars_hip_tensor_row_pitch), or whose size or layout is not the shots object's; *_results with nothing
 * pending.  A refused call leaves the state as it was. */
mars_error_t mars_hip_shots_create(int streams, int slots, int tw, int th, int nhwc, mars_hip_shots_t **out);
void         mars_hip_shots_free(mars_hip_shots_t *sh);                            /* waits for the device first */
/* That stream's table empty, its step and counters zero; -1: all streams; waits. */
mars_error_t mars_hip_shots_reset(mars_hip_shots_t *sh, int stream);
/* The end of a stream: waits, turns every LIVE slot DONE and adds them to `finished`; -1: all streams.  The step counter stays. */
mars_error_t mars_hip_shots_flush(mars_hip_shots_t *sh, int stream);
/* Waits.  counters = {finished, lost, dropped, overflow, duplicates, taken} of one stream, its LIVE and DONE slots and its step counter;
 * any pointer may be NULL. */
mars_error_t mars_hip_shots_read(mars_hip_shots_t *sh, int stream, long long counters[6], int *n_live, int *n_done, int *step);
/* Waits.  The table of one stream, slots = [the object's slots], in canonical form. */
mars_error_t mars_hip_shots_read_slots(mars_hip_shots_t *sh, int stream, mars_shot_slot_t *slots);
/* Waits.  The picture of a LIVE or DONE slot: rgb = uint8 [th][tw][3], byte + 128 with the layout undone. */
mars_error_t mars_hip_shots_read_pixels(mars_hip_shots_t *sh, int stream, int slot, unsigned char *rgb);
/* How a deployment receives a finished track's picture.  Waits, copies the DONE slots by ascending slot, up to `cap`, into slots_out =
 * [cap] with their pictures in rgb_out = [cap][th][tw][3] (either may be NULL with cap 0), and frees exactly those it copied.  *n = the
 * number of DONE slots there were. */
mars_error_t mars_hip_shots_collect(mars_hip_shots_t *sh, int stream, mars_shot_slot_t *slots_out, unsigned char *rgb_out, int cap, int *n);
/* The mars_yolo_event_lists of this feature: host pointers in and out, runs the same kernels on the GPU and waits.  One entry of each
 * array belongs to one crop: crops = [n_crops][tw * th * 3] int8 in the object's layout, rois, confs, cls, tracks and records = [n_crops];
 * every crop counts as written (kept = n_crops, at most 65535).  A crop whose rois[k].frame lies outside [0, frames) has no content. */
mars_error_t mars_yolo_shot_lists(mars_hip_shots_t *sh, const signed char *crops, const mars_roi_t *rois, const float *confs, const int *cls,
                                  const mars_track_t *tracks, int n_crops, int frames, const mars_hip_shot_opts_t *opts, mars_shot_t *records);
/* The device-only chain.  Reads the crops in input `input_index` of src_model and its ROI table as the last crop call out of det_model
 * left them, and det_model's detection lists and the track array of its last mars_hip_track_device / _track_app_device (F = det_model's
 * batch).  Enqueues only, on the auxiliary stream: behind the crop call (the main stream as given so far) and the tracker, ahead of
 * det_model's next detect call and, through an event of its own, ahead of the next crop call into src_model.  The record array lives on
 * src_model and is freed with it. */
mars_error_t mars_hip_shots_device(mars_model_t *det_model, mars_model_t *src_model, int input_index, mars_hip_shots_t *sh,
                                   const mars_hip_shot_opts_t *opts);
/* Waits.  records = [batch of src_model]: entry k belongs to rois[k] of mars_hip_roi_results.  sh must be the object of the last
 * mars_hip_shots_device call over src_model. */
mars_error_t mars_hip_shots_results(mars_model_t *src_model, mars_hip_shots_t *sh, mars_shot_t *records);
/* mars_hip_shots_device + mars_hip_shots_results. */
mars_error_t mars_hip_shots(mars_model_t *det_model, mars_model_t *src_model, int input_index, mars_hip_shots_t *sh,
                            const mars_hip_shot_opts_t *opts, mars_shot_t *records);
/* Device time (ms) of the last call's three kernels (either form), from events on its stream; waits for it.  < 0: not available. */
float mars_hip_shots_ms(mars_hip_shots_t *sh);

#ifdef __cplusplus
}
#endif
#endif /* MARS_HIP_H */
