/*
 * mars_internal.h -- private state of the MI355X .mars executor (host side).
 * The public prefix of mars_model_ext_t is the reference's mars_model_t
 * (include/mars_runtime.h), so a mars_model_t* handed to callers is also a
 * pointer to the private record.
 */
#ifndef MARS_INTERNAL_H
#define MARS_INTERNAL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_runtime.h"

enum {
    OP_CONV_I8 = 0,
    OP_CONV_F32,
    OP_RELU_BYTES,
    OP_LUT_I8,
    OP_BINARY_I8,
    OP_SIGMOID_F32,
    OP_BINARY_F32,
    OP_RELU_F32,
    OP_BN,
    OP_MAXPOOL,
    OP_CONCAT_SLICE,
    OP_UPSAMPLE,
    OP_UPSAMPLE_Q, OP_MAXPOOL_Q, /* UPSAMPLE / stride-1 MAXPOOL of an NCHW-tagged graph on tensors held pixels x channels (nhwc_internal) */
    OP_CONCAT_Q, /* a whole CONCAT layer of an NCHW-tagged graph on tensors held pixels x channels (nhwc_internal; mhip_concat_nchwq) */
    OP_CONV_F32_VHEAD, /* the first pixels of a conv_f32 that reads a never-materialised float CONCAT (virtual_concat_f32; mhip_conv_f32_vcat_head) */
    OP_FAIL, /* mars_run stops here with op->err, as the reference would at this layer */
};

#define NO_OFF ((size_t)-1)
#define MARS_MAX_IO 4 /* graph inputs / outputs (header arrays of the .mars format) */
#define MARS_MAX_MODEL_TUNE 16 /* per-model tuning overrides (mars_hip_model_set_tuning) */

typedef struct {
    size_t bytes;    /* numel * elemsize by shape */
    size_t extent;   /* largest byte offset + 1 any op touches (>= bytes) */
    size_t stride;   /* device bytes per frame (0 for weights) */
    uint8_t *dev;    /* device base */
    int is_weight;
    int needed;      /* touched by an op, or graph input/output */
    int io_in, io_out; /* 1-based graph input / output slot, 0 if none */
    uint8_t *host;   /* pinned staging for graph I/O: batch * bytes */
    uint8_t *dense_dev; /* padded rows only: batch * bytes, the dense copy made on the device before a download */
    int pix_c, pix_stride; /* pix_stride != 0: [pixels][pix_c] rows kept at a pix_stride-byte pitch on the device (pad_output_rows) */
    int rec_c, rec_hw;     /* rec_c != 0: a float tensor kept in RECORD format on the device (rec_pairs): [rec_c / 8][rec_hw] x 32 bytes */
    int nhwc_c, nhwc_hw;   /* nhwc_c != 0: an NCHW-tagged int8 tensor kept as [nhwc_hw][nhwc_c] (pixels x channels) on the device (nhwc_internal) */
    size_t zero_from;      /* != 0: bytes from this offset on are never written by any layer (zero_tail_f32 relies on it): mars_hip_write_tensor refuses non-zero bytes there */
    int partial;           /* only part of the tensor is ever written (virtual_concat_q keeps the first rows of a concat): not readable through mars_hip_read_tensor */
    int nhwc_pitch;        /* ... bytes between its pixels (0 = nhwc_c; a write-only 255-channel head is kept at 256) */
    int tail_read;         /* a raw-head decode (mars_hip_detect_heads_device / _dfl_device) reads it: a pending tail holds back its writer like a graph output's */
} mtensor_t;

/* One launch.  The operand model every planner pass and the run path rely on (plan_check enforces it on every plan):
 *   - a launch READS exactly the tensors t_in[0 .. n_in): add_t - 1, seg_t[0 .. nseg) and vc_t[0 .. vc_n) say which ROLE an entry of t_in
 *     plays (the folded Add's operand, the segments of a virtual concat, the first inputs of a float one), they name no further operand;
 *   - a launch WRITES t_out and chain_out[0 .. chain_n), where chain_n != 0 implies t_out == chain_out[chain_n - 1].
 * Ask through op_reads() / op_writes(); a new operand field must be mirrored into t_in, not scanned for. */
typedef struct {
    int kind, layer, err;
    int t_in[4], n_in, t_out; /* tensor indices, -1 if none */
    /* geometry (conv / pool / concat / upsample share these) */
    int in_h, in_w, in_c, out_h, out_w, out_c, kh, kw, sh, sw, pt, pl;
    int nchw, relu, is_mul, is_f32, leaky, safe; /* nchw (conv_i8): the INPUT is [C][H][W] bytes and is relaid into scratch before the launch */
    size_t in_byte_off, out_byte_off; /* conv_i8: added to the input / output tensor's address (virtual_concat_q: a convolution over a row range of a tensor) */
    int k_limit;   /* conv_f32 (1 x 1): input channels >= k_limit are exact zeros in every frame (zero_tail_f32): mhip_conv_f32_t.k_limit under modes 3 / 4; 0 = none */
    int vc_n, vc_t[3], vc_run, vc_shift; /* conv_f32 (1 x 1) over a float CONCAT that is never materialised (virtual_concat_f32): t_in[0] is the concat's LAST input, read
                      through a view vc_shift bytes in front of it, K loop = k_limit planes (required);  OP_CONV_F32_VHEAD: the concat's other inputs
                      (vc_n of them, runs of vc_run floats) and k_limit = planes to sum for the first vc_n * vc_run pixels */
    int rows_only; /* OP_CONCAT_Q: only the first `rows_only` map rows of the output are produced (the rest of it is never read: virtual_concat_q); 0 = all */
    int out_nchw;  /* conv_i8: the result is stored [O][H][W] (the reference's conv2d_int8_mxu); both set by the input's tag, cleared per side by nhwc_internal */
    int silu_f32;  /* conv_f32 with the float SIGMOID + MUL pair (ONNX SiLU) folded into its epilogue */
    int f32_exact; /* conv_f32 whose result reaches a byte-wise MAXPOOL over float bytes: keeps the reference's summation order */
    int variant; /* conv_i8 launch variant pinned by mars_hip_autotune (0 = default policy) */
    int add_t; float add_s_conv, add_s_other, add_inv; /* conv_i8 with a residual Add folded in: other operand (tensor index + 1, 0 = none) */
    int nseg, seg_t[4], seg_c[4], seg_up;
    int chain_n, chain_out[3]; /* OP_MAXPOOL heading a fused chain of stride-1 pools: every stage's output tensor */
    int pair_next; /* conv_i8: launched together with the NEXT op (same input, same geometry: C3's cv1 + cv2) */ /* conv_i8 reading a never-materialised concat: its segments (tensor, channels) */
    int pair_both; /* ... in the ONE-TILE form (conv_i8_persist<BOTH>: sides of 64 channels, the input staged once for both; pair_convs) */
    int both_chain; /* ... and the op behind the mate, a 1x1 from 64 to 64 channels that reads side both_chain - 1 (1 or 2, 0 = none: the bottleneck's
                       m.cv1), is evaluated in that side's waves (fuse_both_chain; conv_i8_persist<CHAIN>); it stays in the plan, is not launched */
    int both_elide; /* ... and that side has no other reader and is no graph output: it is not stored, its tensor is not allocated */
    int row_pad, oc_pad, c_pad;
    int ch_off, scale_h, scale_w, bn_n;
    int out_pix_stride, out_ch_off; /* producer writes a channel slice of a wider tensor (zero-copy concat) */
    int store_c; /* conv_i8 writing padded pixel rows: channels stored per pixel (the padded count), 0 = out_c */
    float cs, f0, f1, f2;
    size_t n;                 /* elements per frame for element-wise ops */
    size_t w_off, b_off, lut_off, s_off; /* offsets into the parameter arena */
    int pre;         /* fused bottleneck: a 1x1 + SiLU evaluated on the staged patch before this convolution (fuse_bottleneck) */
    size_t pre_w_off, pre_b_off, pre_lut2_off;
    float pre_cs;
    int post_next;   /* fused cv3: the NEXT op, a 1x1 over concat({this result, y2}), is evaluated on this convolution's result tile in the same launch
                        (fuse_post; conv_i8_patch<POST>); t_out is never written, y2's tensor is mirrored into t_in; the mate stays in the plan, is not launched */
    size_t post_w_off; /* ... its weights and bias rows as that kernel keeps them in LDS (mhip_conv_i8_post_pack) */
    int split_next;  /* fused cv1 + cv2: the NEXT TWO ops, a paired launch of 1x1s that alone read this convolution's result, are evaluated on its result
                        tile in the same launch (fuse_split; conv_i8_patch<SPLIT>); t_out is never written; both mates stay in the plan, are not launched */
    size_t split_w_off; /* ... their weights and bias rows as that kernel keeps them in LDS (mhip_conv_i8_split_pack) */
    int split_chain; /* ... and the op behind them, a 1x1 from 32 to 32 channels that reads side split_chain - 1 of the pair (1 or 2, 0 = none: the
                        bottleneck's m.cv1), is evaluated on that side's tile row in the same launch (fuse_split_chain; conv_i8_patch<CHAIN>); both
                        sides are still written; that op stays in the plan too, is not launched */
    size_t chain_w_off; /* ... its weights and bias rows as that kernel keeps them in LDS (mhip_conv_i8_chain_pack) */
    size_t w2_off;   /* a second image of the weights, or NO_OFF: the RGB stem's as conv_i8_rgb keeps them in LDS
                        (mhip_conv_i8_rgb_pack), or (w2_rows) a deep 3x3 layer's as conv_i8_rows streams them (mhip_conv_i8_rows_pack) */
    int w2_rows;
    int w2_planes;   /* conv_f32: bf16 planes packed into the w2 image at load (2: hi, mid -- f32_mfma 3; 3: + lo -- f32_mfma 4); 0 = none */
    size_t w3_off;   /* conv_f32: conv_f32_patch's image (unit table, schedule, two bf16 planes in its K order), or NO_OFF */
    int w3_stem;     /* ... that image is conv_f32_stem's */
    int in_rec, out_rec; /* conv_f32: the input / output tensor is in record format (rec_pairs; mhip_conv_f32_t.in_rec / out_rec) */
    size_t lut2_off; /* 512-entry half-step form of the fused LUT (4-instruction requantisation), or NO_OFF */
    size_t w_blob_off[2];     /* operands that live in the blob mirror */
    double macs, bytes;       /* algorithmic work per frame */
    int prof_kind;
    float last_ms;
    void *ev0, *ev1;
    int prof_rec;   /* profiling: this launch's stop event was recorded in the last run */
    void *ev_start; /* profiling: the event that marks this launch's start = the previous launch's ev1 (own ev0 for the first) */
} mars_op_t;

/* ---- tail stages (mars_stage.c): the records every stage behind the detection tail hangs on a model */
/* one result block on the device.  frames: those of the stage's last call, 0 = there was none (cleared before the launches, set after they
 * were enqueued); ev: timing events around the stage's launches on the auxiliary stream, created on first use where the stage has any */
typedef struct { void *dev; size_t bytes; int frames; void *ev[2]; } mars_block_t;
typedef struct { void *dst; size_t off, bytes; } mars_block_part_t; /* mars_block_fetch: a host destination (NULL: skipped) and the part of the block it gets */
/* one record per detection of THIS model: [cap][MARS_YOLO_MAX_DET] x record on the device; frames == 0: nothing has filled it yet */
typedef struct { void *dev; int cap, frames; } mars_det_side_t;
/* where the plan left an int8 activation tensor that a convolution wrote (mars_side_tensor) */
typedef struct { int buf; const int8_t *base; size_t stride; int c, h, w, pix_step, ch_step; } mars_side_tensor_t;
/* the (effective) scales the tables up on the device were built from, per head; n: tables that are up (0: none) */
typedef struct { float key[4][2]; int n; } mars_lut_cache_t;

/* Every environment switch the planner and alloc_batch obey, read in ONE place (plan_switches_read, mars_model.c): a plan is a function of
 * (file, batch, f32_mfma mode, this record).  build_plan and alloc_batch refresh it when they start; `fusion` is read at load only
 * (mars_hip_set_fusion changes it afterwards). */
typedef struct {
    int fusion; /* MARS_HIP_FUSION, default 1 */
    unsigned no_fuse_lut : 1, no_nhwc_internal : 1, no_vconcat_q : 1, no_pair_f32 : 1, no_rec : 1, no_zero_tail : 1, no_vconcat_f32 : 1,
        no_rowpad : 1, no_post : 1, no_split : 1, no_chain : 1, no_both : 1, no_both_chain : 1; /* MARS_HIP_NO_*: set = that pass is off */
    size_t rec_limit;        /* MARS_HIP_REC_LIMIT: bytes all frames of a tensor may span under 32-bit offsets (rec_pairs, virtual_concat_f32) */
    size_t vconcat_limit;    /* MARS_HIP_VCONCAT_LIMIT: ... the output of a segmented convolution (alloc_batch) */
    size_t bottleneck_limit; /* MARS_HIP_BOTTLENECK_LIMIT: largest batch that keeps fused bottlenecks, 0 = no limit (alloc_batch) */
} plan_switches_t;

typedef struct mars_model_ext {
    mars_model_t pub; /* MUST stay first */
    plan_switches_t sw;
    int batch, profiling, deferred;
    int plan_err;   /* first allocation failure while planning (build_plan returns it; 0 = none) */
    int no_vconcat; /* virtual concat switched off (a batch too large for 32-bit buffer offsets) */
    int no_download; /* mars_hip_set_output_mode(MARS_HIP_OUTPUT_ON_DEVICE): mars_run leaves the graph outputs in HBM */
    int no_bottleneck; /* fused bottlenecks (fusion level 2) switched off: one of them cannot launch at this batch */
    int no_post;       /* fused cv3 launches (fuse_post) switched off: one of them cannot launch at this batch (32-bit output offsets) */
    int no_split;      /* fused cv1 + cv2 launches (fuse_split) switched off: likewise */
    int no_chain;      /* the 1x1 chained to such a launch (fuse_split_chain) switched off: likewise */
    int no_both;       /* one-tile pairs (pair_convs, pair_both) switched off: likewise */
    int no_both_chain; /* the 1x1 chained to such a pair (fuse_both_chain) switched off: likewise */
    int rec_frames;    /* rec_pairs: the batch the record-format pairs were chosen for (0 = one frame); a pair whose tensors reach 4 GiB at that batch is left alone */
    int rec_skipped;   /* ... some pair was left alone for that reason (a smaller batch may take it) */
    size_t rec_max_frames; /* ... the largest batch every chosen pair still fits */
    mtensor_t *mt;
    mars_op_t *ops;
    int n_ops, cap_ops;
    /* parameter arena: host image + device copy */
    uint8_t *arena_host;
    size_t arena_size, arena_cap;
    uint8_t *arena_dev;
    size_t blob_mirror_bytes;
    /* activations */
    uint8_t *act_dev;
    size_t act_bytes;
    uint8_t *scratch_dev;
    size_t scratch_per_frame;
    int scratch_t, scratch_cpad, scratch_f0, scratch_n; /* what the relayout scratch holds: tensor (-1 = nothing), channel padding, frame range (enqueue_range) */
    /* detection tail */
    void *det_dev;
    int *det_counts_dev;
    float *det_lut_dev;
    int det_cap;
    mars_lut_cache_t det_lut; /* the output scales the uploaded decode LUTs were built for */
    int det_lut_mono[4];    /* value table of that segment strictly increasing (mhip_detect_t.mono) */
    float *heads_lut_dev;   /* raw-head decode: [head][256] sigmoid tables (mhip_heads_t.sig) */
    mars_lut_cache_t heads_lut;
    float *dfl_lut_dev;     /* DFL decode: [head][512] tables (mhip_dfl_heads_t.tab) */
    mars_lut_cache_t dfl_lut; /* effective (box, class) scales they were built for */
    void *ev_graph_done, *ev_tail_done; /* main->aux and aux->main hand-offs */
    int tail_pending;
    int frame0, run_frames; /* frame range the launches being enqueued cover (a large batch runs as two halves on two streams) */
    void *ev_fork, *ev_join[3];
    void *ev_chunk[2][8]; /* mars_run at large batches: [0] chunk uploaded, [1] chunk computed */
    void *graph_exec;   /* captured HIP graph of the plan at the current batch (small batches), or NULL */
    unsigned graph_gen; /* tuning generation it was captured under */
    int ran_plain;      /* the plan has run launch by launch at this batch: every launcher's one-time set-up is done */
    void *pipe; /* double-buffered I/O state (mars_pipe.c), NULL when closed */
    struct { char key[28]; int value, saved; } tune[MARS_MAX_MODEL_TUNE]; /* launch-policy overrides of this model */
    int n_tune, tune_depth;
    int plan_f32_mode; /* the f32_mfma mode build_plan ran under (weight images, record pairs): replan_for_f32_mode */
    unsigned char *layer_noop; /* [num_layers]: plan_layer emitted no launch for it (the runtime treats it as a no-op; mars_yolo_find_heads) */
    void *roi_dev;      /* ROI crops INTO this model (mars_roi.c): [kept, dropped, -, -][roi_cap_slots] x mars_roi_t[roi_cap_frames] x int, on the device */
    int roi_cap_slots, roi_cap_frames;
    int roi_slots;      /* slots of the last crop call (its batch then); 0 = there was none */
    struct mars_model_ext *roi_from; /* ... whose detections they were (compared, never followed: mars_free clears it) */
    void *roi_fit_dev;  /* "Aligned crops": [roi_cap_slots] x mars_align_t beside the table, from the first aligned crop call on; grown and released with it */
    int roi_fit_slots;  /* roi_slots if the last crop call was an aligned one, else 0 */
    /* second-stage labels (mars_classify.c) */
    mars_block_t cls;   /* pooled results of THIS model: [frames][nsplit][C] partial sums, [frames][C] sums, [frames][top_k] entries */
    size_t cls_sums_off, cls_top_off;
    int cls_c, cls_top_k; /* of the last classify call */
    void *ev_label_done; /* a label scatter (auxiliary stream) has read this model's ROI table and entries: the next crop call into it waits */
    int label_pending;
    mars_det_side_t label; /* labels of THIS model's detections: x mars_cls_t */
    /* gallery match (mars_gallery.c) */
    mars_block_t match; /* match results of THIS model: quantised queries, qq, qinv, the chunks' lists, [frames][top_k] entries, their rows */
    size_t match_top_off, match_row_off;
    int match_top_k;    /* of the last match call */
    mars_det_side_t ident; /* identities of THIS model's detections: x mars_cls_t */
    /* tracking (mars_track.c) */
    mars_det_side_t track; /* track ids of THIS model's detections: x mars_track_t */
    mars_block_t track_app; /* "Appearance in tracking", of THIS model's detections: the quantised rows [slots][cp], their qq [slots], the row
                             * index of every detection [frames][MARS_YOLO_MAX_DET] x int */
    /* instance masks (mars_seg.c) */
    mars_block_t seg;   /* candidate / kept prediction indices [frames][MARS_YOLO_MAX_DET] x int each, the kept boxes before the letterbox mapping,
                         * [frames][seg_max] x mars_mask_t, [frames][seg_max][seg_ph][pitch] x uint32 */
    size_t seg_rec_off, seg_word_off;
    int seg_max, seg_ph, seg_pw; /* of the last seg call */
    /* instance masks in frame pixels (mars_seg.c): a block of its own, so the prototype-size results above stay fetchable */
    mars_block_t segn;  /* the tap tables 6 x [MARS_MASK_NATIVE_MAX] x int (at its start: their place does not move with the batch), candidate /
                         * kept prediction indices, [frames][segn_max] x mars_mask_t, [frames][segn_max][segn_oh][pitch] x uint32 */
    size_t segn_rec_off, segn_word_off;
    int segn_max, segn_oh, segn_ow; /* of the last native seg call */
    int segn_key[10];   /* what the block's tap tables were built for: the mars_mask_geom_t's axes fields and PH, PW; segn_key[8] == 0: none */
    /* pose keypoints (mars_pose.c) */
    mars_block_t pose;  /* the visibility tables [4][256] x float, candidate / kept prediction indices [frames][MARS_YOLO_MAX_DET] x int each,
                         * [frames][pose_max] x mars_pose_t, [frames][pose_max][pose_k] x mars_kpt_t */
    size_t pose_rec_off, pose_kpt_off;
    int pose_max, pose_k; /* of the last pose call */
    mars_lut_cache_t pose_lut; /* the block's visibility tables */
    /* oriented boxes (mars_obb.c) */
    mars_block_t obb;   /* the angle tables [4][768] x float, kept and candidate counts [frames] x int each, candidate records
                         * [frames][MARS_YOLO_MAX_DET] x mars_obb_t, their (cos, sin) pairs, kept records [frames][MARS_YOLO_MAX_DET] x mars_obb_t,
                         * the kept records' (cos, sin) pairs (mars_roi.c cuts rotated crops along them) */
    size_t obb_cnt_off, obb_out_off, obb_csn_off;
    mars_lut_cache_t obb_lut; /* the block's angle tables */
    /* tiled inference (mars_tile.c) */
    int det_mapped;     /* the last detection tail of THIS model mapped its lists into source-frame pixels (src_w > 0): the tile merge refuses them */
    mars_block_t tile_roi; /* tiles INTO this model: [slots, 0, ...] in 256 bytes, then [batch] x mars_roi_t */
    mars_block_t tile;  /* merged lists of THIS model's detections: [frames][MARS_YOLO_MAX_DET] x mars_det_t, the same of mars_tile_src_t,
                         * [frames] x int, [frames] x mars_tile_stats_t; frames = camera frames of the last merge */
    size_t tile_off[4];
    /* redaction (mars_redact.c) */
    mars_block_t redact; /* of THIS model's detections: the region table [frames][MARS_YOLO_MAX_DET] x 5 int, its counts [frames] x int,
                          * [frames] x mars_redact_stats_t */
    size_t redact_stats_off;
    void *ev_redact_done; /* the redaction (auxiliary stream) has written the frames: the main stream waits for it */
    /* overlay (mars_overlay.c) */
    mars_block_t overlay; /* of THIS model's detections: the element table [frames][MARS_YOLO_MAX_DET] x 12 int, the marker table
                           * [frames][markers] x 4 int, both counts [frames] x int, [frames] x mars_overlay_stats_t, the packed palette [256] x
                           * uint32, the names */
    size_t overlay_stats_off;
    void *overlay_img;    /* host copy of the palette and names that are up in the block: a call with the same ones uploads nothing */
    size_t overlay_img_bytes;
    /* motion (mars_motion.c) */
    mars_det_side_t motion; /* moved cells of THIS model's detections: x mars_motion_det_t */
    /* events (mars_events.c) */
    mars_det_side_t event;  /* event records of THIS model's detections: x mars_event_t */
    /* best shots (mars_shots.c) */
    mars_block_t shot;      /* shot records of the crops in THIS model's input: [batch] x mars_shot_t */
    void *ev_shot_done;     /* a shots call (auxiliary stream) has read this model's input and ROI table: the next crop call into it waits */
    int shot_pending;
    struct mars_model_ext *live_next; /* every loaded model, newest first (mars_live_models): a process-wide mode change re-plans the float ones */
} mars_model_ext_t;

/* ---- launch groups: several planned ops that run as ONE launch.  The flags in mars_op_t are the stored truth (the dump prints them); these
 * helpers are the only place that reads them for grouping.  Derived on every call, never stored: passes move ops.  Host-only (tests/c/plan_groups.c).
 * A new form: the enum with its span in form_span and its flags in op_form, its case in conv_i8_group_records / conv_i8_group_fits and in
 * enqueue_range's switch, one row of alloc_batch's table, one plan_check clause, its pass ("Launch groups"). */
enum {
    FORM_PLAIN = 0,   /* {op} */
    FORM_PAIR,        /* {a, b}: side by side (pair_next; conv_i8_persist<PAIR>) */
    FORM_BOTH,        /* {a, b}: one tile (pair_both) */
    FORM_BOTH_CHAIN,  /* {a, b, d}: ... + the 1x1 behind side both_chain */
    FORM_POST,        /* {a, cv3} (post_next) */
    FORM_SPLIT,       /* {a, cv1, cv2} (split_next; cv1 keeps its pair_next) */
    FORM_SPLIT_CHAIN, /* {a, cv1, cv2, d}: ... + the 1x1 behind side split_chain */
    FORM_PAIR_F32,    /* {a, b}: conv_f32_split's pair form */
    FORM_BAD,         /* the flags of op i ask for mates beyond n_ops: an error wherever it is met (plan_check lets no such plan through) */
    FORM_COUNT
};
/* members of a form (FORM_BAD has what the plan has left: op_form); a form without an entry has none, so nothing indexes by it */
static inline int form_span(int form) {
    static const int span[FORM_COUNT] = {[FORM_PLAIN] = 1, [FORM_PAIR] = 2, [FORM_BOTH] = 2, [FORM_BOTH_CHAIN] = 3, [FORM_POST] = 2, [FORM_SPLIT] = 3,
                                         [FORM_SPLIT_CHAIN] = 4, [FORM_PAIR_F32] = 2, [FORM_BAD] = 1};
    return form >= 0 && form < FORM_COUNT ? span[form] : 0;
}
/* the form of the launch that STARTS at op i (i is taken to be a head); g[]: its members in plan order, -1 behind them.  FORM_BAD: the ops left */
static inline int op_form(const mars_model_ext_t *m, int i, int g[4]) {
    const mars_op_t *o = &m->ops[i];
    int form = FORM_PLAIN;
    if (o->split_next) form = o->split_chain ? FORM_SPLIT_CHAIN : FORM_SPLIT;
    else if (o->post_next) form = FORM_POST;
    else if (o->pair_next) form = o->kind == OP_CONV_F32 ? FORM_PAIR_F32 : !o->pair_both ? FORM_PAIR : o->both_chain ? FORM_BOTH_CHAIN : FORM_BOTH;
    int span = form_span(form);
    if (i + span > m->n_ops) { form = FORM_BAD; span = m->n_ops - i; }
    for (int k = 0; k < 4; k++) g[k] = k < span ? i + k : -1;
    return form;
}
static inline int op_span(const mars_model_ext_t *m, int i) {
    int g[4], n = 0;
    op_form(m, i, g);
    while (n < 4 && g[n] >= 0) n++;
    return n;
}
/* the head of the launch that owns op i: groups are laid out from op 0 on, so a flag on a mate (cv1 of a split group keeps pair_next) starts nothing */
static inline int op_head(const mars_model_ext_t *m, int i) {
    int h = 0;
    for (int s; h + (s = op_span(m, h)) <= i; h += s) {}
    return h;
}
static inline int op_is_mate(const mars_model_ext_t *m, int i) { return op_head(m, i) != i; }
/* op i's own flags ask for no mate (not op_span == 1: flags that ask for mates behind the plan's end span the ops left, which may be one) */
static inline int op_plain(const mars_model_ext_t *m, int i) {
    int g[4];
    return op_form(m, i, g) == FORM_PLAIN;
}
/* device address of tensor ti for the first frame of the range being enqueued (weights: one copy for every frame), and its frame stride */
static inline uint8_t *tdev(const mars_model_ext_t *m, int ti) {
    if (ti < 0 || !m->mt[ti].dev) return NULL;
    return m->mt[ti].dev + (m->mt[ti].is_weight ? 0 : (size_t)m->frame0 * m->mt[ti].stride);
}
static inline size_t tstride(const mars_model_ext_t *m, int ti) { return ti >= 0 ? m->mt[ti].stride : 0; }


/* ---- shared between mars_model.c (loader), mars_plan.c (planner) and mars_run.c (run paths); hidden from the library's ABI */
#define MARS_INTERNAL __attribute__((visibility("hidden")))
#define ALIGN_UP(x, a) (((x) + (size_t)(a) - 1) & ~((size_t)(a) - 1))
#define NO_TENSOR 0xFFFFFFFFu
#define MAX_DIM_PRODUCT ((size_t)1 << 40)
#define ARENA_MAX ((size_t)1 << 40) /* parameter arena: anything beyond is a corrupt file, not a model */
#define MAX_CHANNELS 65536    /* per-tensor channel count the planners accept */
MARS_INTERNAL int mars_verbose(void);
#define VLOG(...) do { if (mars_verbose()) fprintf(stderr, "Mars: " __VA_ARGS__); } while (0)
/* mars_model.c */
MARS_INTERNAL void drop_graph(mars_model_ext_t *m);
MARS_INTERNAL mars_model_ext_t *mars_live_models(void);
MARS_INTERNAL void plan_switches_read(plan_switches_t *sw, int at_load);
MARS_INTERNAL mars_error_t build_plan(mars_model_ext_t *m);
MARS_INTERNAL mars_error_t upload_params(mars_model_ext_t *m);
MARS_INTERNAL mars_error_t alloc_batch(mars_model_ext_t *m, int n);
/* mars_plan.c */
MARS_INTERNAL size_t elem_size(uint32_t dtype);
MARS_INTERNAL size_t shape_numel(const mars_tensor_t *d);
MARS_INTERNAL size_t reference_buffer_size(const mars_model_ext_t *m);
MARS_INTERNAL size_t arena_reserve(mars_model_ext_t *m, size_t bytes);
MARS_INTERNAL void blob_read(const mars_model_ext_t *m, size_t off, size_t n, void *dst);
MARS_INTERNAL int op_reads(const mars_op_t *o, int t);  /* t is one of t_in[0 .. n_in) */
MARS_INTERNAL int op_writes(const mars_op_t *o, int t); /* t is t_out or one of chain_out[0 .. chain_n) */
MARS_INTERNAL size_t planned_stride(const mtensor_t *t);
MARS_INTERNAL int conv_i8_pre_fits(const mars_op_t *op, int frames, size_t in_stride, size_t out_stride);
/* the launch records of a group, for the question "does the device code take it" (live = 0: stand-in addresses, planned strides; the members
 * are candidates, their flags need not be set yet) and for the launch itself (live = 1: device addresses of the frame range being enqueued) */
MARS_INTERNAL void conv_i8_group_records(const mars_model_ext_t *m, int form, const mars_op_t *g[4], int side, int frames, int live, mhip_conv_i8_t *p);
MARS_INTERNAL int conv_i8_group_fits(const mars_model_ext_t *m, int form, const mars_op_t *g[4], int side, int frames);
MARS_INTERNAL void fuse_both_chain(mars_model_ext_t *m);
/* ... the passes, in the order build_plan calls them (f32: 0 = the int8 form, 1 = the float32 form) */
MARS_INTERNAL void plan_layer(mars_model_ext_t *m, int li);
MARS_INTERNAL void fold_silu(mars_model_ext_t *m, int f32);
MARS_INTERNAL void fuse_lut(mars_model_ext_t *m);
MARS_INTERNAL void nhwc_internal(mars_model_ext_t *m);
MARS_INTERNAL void fold_add(mars_model_ext_t *m, int f32);
MARS_INTERNAL void virtual_concat(mars_model_ext_t *m);
MARS_INTERNAL void elide_concat(mars_model_ext_t *m);
MARS_INTERNAL void trim_concat(mars_model_ext_t *m);
MARS_INTERNAL void fuse_pool_chains(mars_model_ext_t *m);
MARS_INTERNAL void pair_convs(mars_model_ext_t *m);
MARS_INTERNAL void fuse_bottleneck(mars_model_ext_t *m);
MARS_INTERNAL void fuse_post(mars_model_ext_t *m);
MARS_INTERNAL void fuse_split(mars_model_ext_t *m);
MARS_INTERNAL void fuse_split_chain(mars_model_ext_t *m);
MARS_INTERNAL void pad_output_rows(mars_model_ext_t *m);
MARS_INTERNAL void virtual_concat_q(mars_model_ext_t *m);
MARS_INTERNAL void f32_policy(mars_model_ext_t *m);
MARS_INTERNAL void zero_tail_f32(mars_model_ext_t *m);
MARS_INTERNAL void pair_convs_f32(mars_model_ext_t *m);
MARS_INTERNAL void rec_pairs(mars_model_ext_t *m);
MARS_INTERNAL void virtual_concat_f32(mars_model_ext_t *m);
MARS_INTERNAL void plan_check(mars_model_ext_t *m);
/* mars_preproc.c */
MARS_INTERNAL int mars_preproc_prepare(int w, int h, int tw, int th); /* gather tables of a letterbox geometry, cached */
MARS_INTERNAL int mars_preproc_prepare_nv12(int w, int h, int tw, int th, int frames); /* the same + the conversion scratch, where NV12 frames need one */

/* mars_roi.c */
MARS_INTERNAL void mars_roi_release(mars_model_ext_t *m); /* the ROI table of a model whose device state goes away */

/* mars_stage.c: tail stages.  A new stage's host side starts from a mars_block_t, mars_side_tensor and mars_tail_on_aux; one that reads or
 * writes camera frames from mhip_frame_format_ok / mhip_frame_bytes (csrc/mhip.h), mars_pixel_input and mars_aux_behind_current */
static inline int mars_scale_ok(float s) { return s > 0 && isfinite(s); }
/* the device is up and no pipe is open (a pipe's slots own their buffers) */
static inline mars_error_t mars_stage_guard(const mars_model_ext_t *m) {
    if (!m->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    return m->pipe ? MARS_ERR_INVALID_TENSOR : MARS_OK;
}
/* a detection tail has left lists for the current batch in HBM */
static inline int mars_has_dets(const mars_model_ext_t *m) { return m->det_dev && m->det_counts_dev && m->det_cap >= m->batch; }
/* graph input `input_index` as the target of int8 pixels: three channels, [th][tw][3] (nhwc) or [3][th][tw], dev + frame * stride */
typedef struct { int tid, nhwc, tw, th; int8_t *dev; size_t stride; } mars_pixel_input_t;
/* INVALID_TENSOR: no such input, not three int8 channels of a positive size, or (unless geometry_only, which leaves dev and stride alone)
 * no device buffer whose stride holds a frame */
MARS_INTERNAL mars_error_t mars_pixel_input(const mars_model_ext_t *m, int input_index, int geometry_only, mars_pixel_input_t *out);
/* What the selected stream has been given so far -> the auxiliary stream: *ev (created where the slot is empty) is recorded on the selected
 * stream, then the auxiliary stream is selected and waits for it.  On a failure nothing was enqueued behind the record and the auxiliary
 * stream is not selected: ALLOC_FAILED (no event: nothing at all was enqueued) or LAYER_FAILED.  After MARS_OK the caller enqueues and
 * ends with mhip_select_aux(0) */
MARS_INTERNAL mars_error_t mars_aux_behind_current(void **ev);
MARS_INTERNAL size_t mars_block_layout(const size_t *sz, int n, size_t *off); /* parts of sz[i] bytes, each aligned to 256: their offsets -> the total */
/* the block holds `total` bytes (grown: synchronises, *fresh = 1, what it held is gone) and, with_events, its two events exist */
MARS_INTERNAL mars_error_t mars_block_reserve(mars_block_t *b, size_t total, int with_events, int *fresh);
MARS_INTERNAL void mars_block_release(mars_block_t *b);
MARS_INTERNAL float mars_block_ms(const mars_block_t *b); /* device time between the two events; -1: no call yet, or no events */
/* synchronise, (tail_pending != NULL: clear it,) copy every part with a destination, synchronise; INVALID_TENSOR before the stage's first call */
MARS_INTERNAL mars_error_t mars_block_fetch(const mars_block_t *b, const mars_block_part_t *parts, int n, int *tail_pending);
MARS_INTERNAL mars_error_t mars_side_reserve(mars_det_side_t *s, int frames, size_t rec);
MARS_INTERNAL void mars_side_release(mars_det_side_t *s);
MARS_INTERNAL mars_error_t mars_side_fetch(const mars_det_side_t *s, void *dst, size_t rec);
/* the entries [slot][top_k] at src + top_off of second-stage model m go through m's ROI table onto det's detections, into `side` of det */
MARS_INTERNAL mars_error_t mars_scatter_on_aux(mars_model_ext_t *det, mars_model_ext_t *m, const mars_block_t *src, size_t top_off, int top_k,
                                               mars_det_side_t *side);
/* int8 activation tensor T of want_c channels on a want_h x want_w grid (0: any) whose bytes the plan keeps: where they are, and that every
 * byte a kernel may touch lies inside the frame's stride */
MARS_INTERNAL mars_error_t mars_side_tensor(const mars_model_ext_t *m, int T, int want_c, int want_h, int want_w, mars_side_tensor_t *out);
MARS_INTERNAL int mars_lut_stale(const mars_lut_cache_t *c, int n, const float key[4][2]);
/* tables of n heads built for `key` go up to dst (nothing where they are up already): synchronises around the upload; c->n == 0 if it fails */
MARS_INTERNAL mars_error_t mars_lut_refresh(mars_lut_cache_t *c, void *dst, int n, const float key[4][2], const float *tab, size_t floats_per_head);
MARS_INTERNAL void mars_stages_release(mars_model_ext_t *m); /* every record above and the ROI table, of a model whose device state goes away */

/* mars_shots.c: its parts that need no device (tests/c/shots_host.c drives them under the sanitizers) */
MARS_INTERNAL mars_error_t mars_shots_opts(const mars_hip_shot_opts_t *o, mhip_shots_t *p); /* the checks, the defaults resolved into the launch record */
MARS_INTERNAL mars_error_t mars_shots_map(int streams, int frames, int *steps);             /* F % S == 0 -> the steps of every stream */
MARS_INTERNAL int mars_shots_frame(int streams, int steps, int stream_major, int stream, int step); /* the frame that is (stream, step) */
/* a stored crop, int8 [th][tw][3] or [3][th][tw], -> uint8 [th][tw][3]: byte + 128, the layout undone */
MARS_INTERNAL void mars_shots_relayout(const int8_t *src, int tw, int th, int nhwc, unsigned char *rgb);

/* mars_yolo.c, shared with mars_classify.c */
MARS_INTERNAL int mars_tensor_chw(const mars_tensor_t *d, int *c, int *h, int *w);
MARS_INTERNAL int mars_locate_i8(const mars_model_ext_t *m, int T, int ch, int hh, int ww, int any_writer, int *buf, int *off, int *pix_step, int *ch_step);
/* a tail (launch(m, cfg, m->det_dev, m->det_counts_dev) on the current stream) on the auxiliary stream behind the graph; sets tail_pending */
MARS_INTERNAL mars_error_t mars_own_det_buffers(mars_model_ext_t *m); /* the model's own detection buffers, large enough for the current batch */
MARS_INTERNAL mars_error_t mars_tail_on_aux(mars_model_ext_t *m, int (*launch)(struct mars_model_ext *, const void *, void *, int *), const void *cfg);

/* detection tail pieces shared with the pipelined I/O (mars_yolo.c) */
mars_error_t mars_detect_prepare(mars_model_ext_t *m, const int *output_indices, int n_outputs);
int mars_detect_launch(mars_model_ext_t *m, const int *output_indices, int n_outputs, float nms_thresh, void *dets_dev,
                       int *counts_dev);

/* raw anchor-based heads (mars_yolo.c): a mars_yolo_heads_t resolved against the loaded plan */
typedef struct {
    int n, ti[4], stride[4], nc[4], h[4], w[4], pix_step[4], ch_step[4];
    float anchors[4][3][2];
    float conf, nms;
    int map, px, py;
    float rx, ry;
    int internal; /* some head is not a graph output: one buffer for every batch in flight */
} mars_heads_cfg_t;
MARS_INTERNAL int mars_find_heads(const mars_model_ext_t *m, int *tensor_ids, int *strides, int *num_classes, int cap);
MARS_INTERNAL mars_error_t mars_heads_resolve(mars_model_ext_t *m, const mars_yolo_heads_t *h, mars_heads_cfg_t *c);
MARS_INTERNAL mars_error_t mars_heads_prepare(mars_model_ext_t *m, const mars_heads_cfg_t *c); /* sigmoid tables up; synchronises if they change */
MARS_INTERNAL int mars_heads_launch(mars_model_ext_t *m, const mars_heads_cfg_t *c, void *dets_dev, int *counts_dev); /* current stream */

/* raw anchor-free DFL heads (mars_yolo.c): a mars_yolo_dfl_heads_t resolved against the loaded plan.  A head tensor's bytes live in its own
 * buffer or, where the zero-copy concat made its convolution write a channel slice, inside the concat output's: buf = the tensor that owns
 * the buffer (the one the writing launch names, so the one tail_read goes on), off = the slice's first byte in it */
typedef struct {
    int n, reg_max, stride[4], nc[4], h[4], w[4];
    int box_t[4], cls_t[4], box_buf[4], cls_buf[4], box_off[4], cls_off[4];
    int box_pix_step[4], box_ch_step[4], cls_pix_step[4], cls_ch_step[4];
    float box_scale[4], cls_scale[4]; /* effective: the override, or the tensor's own */
    float conf, nms;
    int map, px, py;
    float rx, ry;
    int nw, nh;   /* with map: the letterboxed content's size inside the graph input (the integers px, py, rx and ry come from) */
    int internal; /* some buffer is not a graph output's: one buffer for every batch in flight */
    int *cand_pred, *kept_pred; /* device, or NULL (mars_dfl_resolve leaves NULL): mhip_dfl_heads_t's origin arrays */
    void *premap;               /* device, or NULL: mhip_dfl_heads_t.premap */
} mars_dfl_cfg_t;
MARS_INTERNAL int mars_find_dfl_heads(const mars_model_ext_t *m, int *box_ids, int *cls_ids, int *strides, int *num_classes, int *reg_max, int cap);
MARS_INTERNAL mars_error_t mars_dfl_resolve(mars_model_ext_t *m, const mars_yolo_dfl_heads_t *h, mars_dfl_cfg_t *c);
MARS_INTERNAL mars_error_t mars_dfl_prepare(mars_model_ext_t *m, const mars_dfl_cfg_t *c); /* tables up; synchronises if they change */
MARS_INTERNAL int mars_dfl_launch(mars_model_ext_t *m, const mars_dfl_cfg_t *c, void *dets_dev, int *counts_dev); /* current stream */

/* shared host helpers (mars_model.c) */
int32_t mars_trunc_x86(float x);
void mars_pack_conv_i8(const int8_t *w, size_t avail, int nchw, int out_c, int in_c, int kh, int kw,
                       int c_pad, int row_pad, int oc_pad, int8_t *dst);

#endif
