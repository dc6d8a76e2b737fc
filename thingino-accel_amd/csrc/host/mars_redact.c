/*
 * mars_redact.c -- host side of the redaction (include/mars_hip.h, "Redaction"): option checks, the result block hung on the detector (the
 * region table, its counts, the statistics), the stream ordering of the device form, its timing events, and the host-pointer form.  The
 * kernels are csrc/hip/redact.hip.  The reference stops at the boxes (src/mars/mars_yolo_test.c:132-214); hiding what was found is left to
 * its callers' CPUs.  There is no CPU pixel path here: without the device every entry point fails.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

#define REDACT_FLAGS (MARS_REDACT_USE_MASKS | MARS_REDACT_SPARE_IDENTIFIED)

/* the checks that need no device and no model, and the defaults resolved into the launch record */
static mars_error_t redact_opts(const mars_hip_redact_opts_t *o, mhip_redact_t *p) {
    memset(p, 0, sizeof(*p));
    if (!o || o->src_w <= 0 || o->src_h <= 0) return MARS_ERR_INVALID_FILE;
    if (!mhip_frame_format_ok(o->src_format, o->src_flags) || !mhip_frame_bytes(o->src_w, o->src_h, o->src_format)) return MARS_ERR_INVALID_FILE;
    if ((o->mode != MARS_REDACT_MOSAIC && o->mode != MARS_REDACT_FILL) || (o->flags & ~REDACT_FLAGS)) return MARS_ERR_INVALID_FILE;
    const int cell = o->cell ? o->cell : 16;
    int lg = 0;
    while ((1 << lg) < cell) lg++;
    if (cell < 2 || cell > 64 || (1 << lg) != cell) return MARS_ERR_INVALID_FILE;
    if (!isfinite(o->expand) || o->expand < 0 || !isfinite(o->min_conf) || o->min_conf < 0 || !isfinite(o->ident_min) || o->ident_min < 0 ||
        o->ident_min > 1 || o->cls_count < 0)
        return MARS_ERR_INVALID_FILE;
    if (o->src_w > MHIP_REDACT_MAX_DIM || o->src_h > MHIP_REDACT_MAX_DIM) return MARS_ERR_INVALID_TENSOR;
    p->w = o->src_w; p->h = o->src_h; p->fmt = o->src_format; p->nv12_flags = o->src_flags;
    p->frame_stride = mhip_frame_bytes(p->w, p->h, p->fmt);
    p->expand = o->expand != 0 ? o->expand : 1.0f;
    p->min_conf = o->min_conf; p->ident_min = o->ident_min;
    p->cls_first = o->cls_first; p->cls_count = o->cls_count;
    p->mode = o->mode; p->cell_log2 = lg;
    memcpy(p->fill, o->fill, 3);
    return MARS_OK;
}

/* a destination that shares bytes with the source without being the source */
static int partial_overlap(const void *src, const void *dst, size_t bytes) {
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    return a != b && a < b + bytes && b < a + bytes;
}

mars_error_t mars_yolo_redact_frames(const unsigned char *frames, int n_frames, const mars_det_t *boxes, const int *frame_of_box, int n_boxes,
                                     const uint32_t *mask_words, const int *mask_of_box, const mars_hip_redact_opts_t *opts, unsigned char *out,
                                     mars_redact_stats_t *stats) {
    mhip_redact_t p;
    const mars_error_t e = redact_opts(opts, &p);
    if (e != MARS_OK) return e;
    if (!frames || !out || n_frames <= 0 || n_frames > 65535 || n_boxes < 0 || n_boxes > 65535 || (n_boxes > 0 && (!boxes || !frame_of_box)))
        return MARS_ERR_INVALID_FILE;
    const size_t in_b = p.frame_stride * (size_t)n_frames;
    if (partial_overlap(frames, out, in_b)) return MARS_ERR_INVALID_FILE;
    int n_masks = 0;
    for (int i = 0; mask_of_box && i < n_boxes; i++)
        if (mask_of_box[i] >= n_masks) n_masks = mask_of_box[i] + 1;
    if (n_masks > 0 && !mask_words) return MARS_ERR_INVALID_FILE;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    /* the boxes as per-frame lists: frame f's are the counts[f] records from list_off[f] on, in the caller's order; a box whose frame index is
     * outside 0 .. n_frames - 1 belongs to no frame and is left out */
    const size_t nb1 = (size_t)(n_boxes > 0 ? n_boxes : 1);
    int *lists = (int *)calloc(2 * (size_t)n_frames + nb1, sizeof(int));
    mars_det_t *packed = (mars_det_t *)malloc(nb1 * sizeof(mars_det_t));
    if (!lists || !packed) {
        free(lists); free(packed);
        return MARS_ERR_ALLOC_FAILED;
    }
    int *list_off = lists, *counts = lists + n_frames, *mask_of = lists + 2 * (size_t)n_frames;
    for (int i = 0; i < n_boxes; i++)
        if (frame_of_box[i] >= 0 && frame_of_box[i] < n_frames) counts[frame_of_box[i]]++;
    for (int f = 0, acc = 0; f < n_frames; f++) { list_off[f] = acc; acc += counts[f]; counts[f] = 0; }
    for (int i = 0; i < n_boxes; i++) {
        const int f = frame_of_box[i];
        if (f < 0 || f >= n_frames) continue;
        const int k = list_off[f] + counts[f]++;
        packed[k] = boxes[i];
        mask_of[k] = mask_of_box ? mask_of_box[i] : -1;
    }
    /* one device block: [frames][out][boxes][list_off, counts, mask_of][table][table_n][stats][mask words] */
    const int oop = out != frames;
    const size_t mask_b = (size_t)n_masks * p.h * ((p.w + 31) / 32) * sizeof(uint32_t);
    const size_t sz[8] = {in_b, oop ? in_b : 0, nb1 * sizeof(mars_det_t), (2 * (size_t)n_frames + nb1) * sizeof(int), nb1 * 5 * sizeof(int),
                          (size_t)n_frames * sizeof(int), (size_t)n_frames * sizeof(mars_redact_stats_t), mask_b};
    size_t off[8];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 8, off));
    int rc = d ? 0 : -1;
    if (d) {
        p.frames = d; p.dst = oop ? d + off[1] : d; p.n_frames = n_frames;
        p.dets = d + off[2];
        p.list_off = (const int *)(d + off[3]); p.counts = p.list_off + n_frames; p.mask_of = n_masks ? p.list_off + 2 * (size_t)n_frames : NULL;
        p.select_all = 1;
        p.mask_words = n_masks ? (const uint32_t *)(d + off[7]) : NULL;
        p.table = (int *)(d + off[4]); p.table_n = (int *)(d + off[5]); p.stats = (int *)(d + off[6]);
        rc = mhip_h2d_async(d, frames, in_b);
        if (!rc) rc = mhip_h2d_async(d + off[2], packed, sz[2]);
        if (!rc) rc = mhip_h2d_async(d + off[3], lists, sz[3]);
        if (!rc && n_masks) rc = mhip_h2d_async(d + off[7], mask_words, mask_b);
        if (!rc) rc = mhip_redact_select(&p);
        if (!rc) rc = mhip_redact(&p);
        if (!rc) rc = mhip_d2h_async(out, p.dst, in_b);
        if (!rc && stats) rc = mhip_d2h_async(stats, p.stats, sz[6]);
        if (mhip_sync()) rc = -1;
        mhip_free(d);
    }
    free(lists); free(packed);
    return !d ? MARS_ERR_ALLOC_FAILED : rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_hip_redact_device(mars_model_t *det_model, void *frames_dev, void *dst_dev, const mars_hip_redact_opts_t *opts) {
    if (!det_model || !frames_dev || !opts) return MARS_ERR_INVALID_FILE;
    mhip_redact_t p;
    mars_error_t e = redact_opts(opts, &p);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)det_model;
    if ((e = mars_stage_guard(m)) != MARS_OK) return e;
    if (!dst_dev) dst_dev = frames_dev;
    const int B = m->batch;
    if (partial_overlap(frames_dev, dst_dev, p.frame_stride * (size_t)B)) return MARS_ERR_INVALID_FILE;
    if (!mars_has_dets(m) || B > 65535) return MARS_ERR_INVALID_TENSOR; /* no detections in HBM */
    if (opts->flags & MARS_REDACT_USE_MASKS) { /* the native mask results of this batch, on the frames' own grid */
        if (!m->segn.dev || m->segn.frames != B || m->segn_ow != p.w || m->segn_oh != p.h) return MARS_ERR_INVALID_TENSOR;
        p.mask_recs = (const uint8_t *)m->segn.dev + m->segn_rec_off;
        p.mask_words = (const uint32_t *)((const uint8_t *)m->segn.dev + m->segn_word_off);
        p.mask_max = m->segn_max;
    }
    if (opts->flags & MARS_REDACT_SPARE_IDENTIFIED) { /* the identities hung on this batch's detections */
        if (!m->ident.dev || m->ident.frames != B) return MARS_ERR_INVALID_TENSOR;
        p.idents = m->ident.dev;
    }
    /* the block: the region table (a region per detection at most), its counts, the statistics */
    const size_t sz[3] = {(size_t)B * MARS_YOLO_MAX_DET * 5 * sizeof(int), (size_t)B * sizeof(int), (size_t)B * sizeof(mars_redact_stats_t)};
    size_t off[3];
    e = mars_block_reserve(&m->redact, mars_block_layout(sz, 3, off), 1, NULL);
    if (e != MARS_OK) return e;
    if (!m->ev_redact_done && !(m->ev_redact_done = mhip_event_create_sync())) return MARS_ERR_ALLOC_FAILED;
    uint8_t *blk = (uint8_t *)m->redact.dev;
    p.frames = (const uint8_t *)frames_dev; p.dst = (uint8_t *)dst_dev; p.n_frames = B;
    p.dets = m->det_dev; p.counts = m->det_counts_dev; p.det_cap = MARS_YOLO_MAX_DET;
    p.table = (int *)blk; p.table_n = (int *)(blk + off[1]); p.stats = (int *)(blk + off[2]);
    m->redact.frames = 0;
    /* The auxiliary stream.  It carries the detection tail, the native masks and the identity scatter, so the redaction comes behind all
     * three.  The frames are read by work on the main stream (the front-end, crops enqueued earlier): the redaction waits for what that
     * stream has been given so far, and the main stream then waits for the redaction, so that whatever the library enqueues later sees the
     * redacted frames */
    mhip_select_stream(0);
    if ((e = mars_aux_behind_current(&m->ev_graph_done)) != MARS_OK) return e;
    int rc = mhip_event_record(m->redact.ev[0]);
    if (!rc) rc = mhip_redact_select(&p);
    if (!rc) rc = mhip_redact(&p);
    if (!rc) rc = mhip_event_record(m->redact.ev[1]);
    if (!rc) rc = mhip_event_record(m->ev_redact_done);
    mhip_select_aux(0);
    if (!rc) rc = mhip_stream_wait(0, m->ev_redact_done);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->redact.frames = B;
    m->redact_stats_off = off[2];
    return MARS_OK;
}

mars_error_t mars_hip_redact_results(mars_model_t *det_model, mars_redact_stats_t *stats) {
    if (!det_model) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)det_model;
    const mars_block_part_t part = {stats, m->redact_stats_off, (size_t)m->redact.frames * sizeof(mars_redact_stats_t)};
    return mars_block_fetch(&m->redact, &part, 1, &m->tail_pending);
}

mars_error_t mars_hip_redact(mars_model_t *det_model, unsigned char *frames, const mars_hip_redact_opts_t *opts, mars_redact_stats_t *stats) {
    if (!det_model || !frames || !opts) return MARS_ERR_INVALID_FILE;
    mhip_redact_t q;
    mars_error_t e = redact_opts(opts, &q);
    if (e != MARS_OK) return e;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const int n = mars_hip_get_batch(det_model);
    if (n <= 0) return MARS_ERR_INVALID_TENSOR;
    const size_t in_b = q.frame_stride * (size_t)n;
    uint8_t *d = (uint8_t *)mhip_malloc(in_b);
    if (!d) return MARS_ERR_ALLOC_FAILED;
    mhip_select_stream(0);
    if (mhip_h2d_async(d, frames, in_b)) e = MARS_ERR_LAYER_FAILED;
    if (e == MARS_OK) e = mars_hip_redact_device(det_model, d, NULL, opts);
    if (e == MARS_OK) e = mars_hip_redact_results(det_model, stats); /* waits for both streams */
    else (void)mhip_sync(); /* the upload may still be running */
    if (e == MARS_OK && (mhip_d2h_async(frames, d, in_b) || mhip_sync())) e = MARS_ERR_LAYER_FAILED;
    mhip_free(d);
    return e;
}

float mars_hip_redact_ms(mars_model_t *det_model) { return det_model ? mars_block_ms(&((mars_model_ext_t *)det_model)->redact) : -1.0f; }
