/*
 * mars_overlay.c -- host side of the overlay (include/mars_hip.h, "Overlay"): the built-in palette, the colour conversion, the font and text
 * functions for callers and tests, option checks, the result block hung on the detector (element table, marker table, their counts, the
 * statistics, the palette and names), the stream ordering of the device form, its timing events, and the host-pointer form.  The kernels
 * are csrc/hip/overlay.hip; the font and the text composition are csrc/overlay_rule.h, compiled into both.  The reference draws with PIL in
 * a test script (mgk-decompiler/test_yolo_inference.py, draw_detections).  There is no CPU pixel path here: without the device every entry
 * point that paints fails.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "../overlay_rule.h"
#include "mars_hip.h"
#include "mars_internal.h"

_Static_assert(MARS_OVERLAY_TEXT_MAX == MHIP_OVERLAY_TEXT_MAX && MARS_OVERLAY_NAME_LEN == MHIP_OVERLAY_NAME_LEN &&
                   MARS_OVERLAY_TEXT_CLASS == MHIP_OVERLAY_TEXT_CLASS && MARS_OVERLAY_TEXT_TRACK == MHIP_OVERLAY_TEXT_TRACK &&
                   MARS_OVERLAY_TEXT_CONF == MHIP_OVERLAY_TEXT_CONF && MARS_OVERLAY_MASKS == MHIP_OVERLAY_MASKS && MARS_OVERLAY_BOXES == MHIP_OVERLAY_BOXES &&
                   MARS_OVERLAY_KEYPOINTS == MHIP_OVERLAY_KEYPOINTS && MARS_OVERLAY_LABELS == MHIP_OVERLAY_LABELS &&
                   MARS_POSE_MAX_KPT == MHIP_OVERLAY_MAX_KPT && sizeof(mars_overlay_stats_t) == 6 * sizeof(int),
               "csrc/mhip.h and csrc/overlay_rule.h");

#define PALETTE_MAX 256
#define ALL_LAYERS (MARS_OVERLAY_MASKS | MARS_OVERLAY_BOXES | MARS_OVERLAY_KEYPOINTS | MARS_OVERLAY_LABELS)
#define ALL_TEXT (MARS_OVERLAY_TEXT_CLASS | MARS_OVERLAY_TEXT_TRACK | MARS_OVERLAY_TEXT_CONF)

static const unsigned char font[64][7] = MHIP_OVERLAY_FONT_ROWS;
static const unsigned char default_palette[16][3] = {{255, 64, 64}, {64, 200, 64},  {64, 128, 255},  {255, 200, 0}, {255, 0, 255}, {0, 220, 220},
                                                     {255, 128, 0}, {128, 64, 255}, {160, 255, 64},  {255, 128, 192}, {0, 128, 128}, {128, 0, 0},
                                                     {0, 0, 160},   {128, 128, 0},  {192, 192, 192}, {96, 96, 96}};

int mars_overlay_default_palette(unsigned char *rgb) {
    if (rgb) memcpy(rgb, default_palette, sizeof(default_palette));
    return 16;
}

void mars_overlay_glyph(int byte, unsigned char rows[7]) {
    if (rows) memcpy(rows, font[mhip_overlay_glyph_index(byte)], 7);
}

int mars_overlay_text(unsigned text, const char *names, int n_names, int cls, int track_id, float conf, char *out) {
    unsigned char buf[MARS_OVERLAY_TEXT_MAX];
    const int n = mhip_overlay_text(buf, (text & ALL_TEXT) ? (text & ALL_TEXT) : (MARS_OVERLAY_TEXT_CLASS | MARS_OVERLAY_TEXT_CONF), names,
                                    names ? n_names : 0, cls, track_id, conf);
    if (out) memcpy(out, buf, sizeof(buf));
    return n;
}

static unsigned char clamp_u8(int v) { return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }
/* an arithmetic shift by 8 of a value that may be negative: floor(v / 256) */
static int asr8(int v) { return v >= 0 ? v >> 8 : -((-v + 255) >> 8); }

void mars_overlay_rgb_to_yuv(const unsigned char *rgb, unsigned flags, unsigned char *yuv) {
    if (!rgb || !yuv) return;
    const int r = rgb[0], g = rgb[1], b = rgb[2];
    int y, u, v;
    if (flags & MARS_NV12_FULL_RANGE) {
        y = asr8(77 * r + 150 * g + 29 * b + 128);
        u = asr8(-43 * r - 85 * g + 128 * b + 128) + 128;
        v = asr8(128 * r - 107 * g - 21 * b + 128) + 128;
    } else {
        y = asr8(66 * r + 129 * g + 25 * b + 128) + 16;
        u = asr8(-38 * r - 74 * g + 112 * b + 128) + 128;
        v = asr8(112 * r - 94 * g - 18 * b + 128) + 128;
    }
    yuv[0] = clamp_u8(y);
    yuv[1] = clamp_u8(flags & MARS_NV12_VU ? v : u);
    yuv[2] = clamp_u8(flags & MARS_NV12_VU ? u : v);
}

/* an RGB colour as the kernels take it: the frame format's three bytes and, in bit 24, whether the text on it is white */
static uint32_t pack_colour(const unsigned char *rgb, int fmt, unsigned flags) {
    unsigned char c[3] = {rgb[0], rgb[1], rgb[2]};
    if (fmt) mars_overlay_rgb_to_yuv(rgb, flags, c);
    return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)mhip_overlay_text_white(rgb[0], rgb[1], rgb[2]) << 24;
}

/* the checks that need no device and no model, the defaults resolved into the launch record and the packed palette (n of them) */
static mars_error_t overlay_opts(const mars_hip_overlay_opts_t *o, mhip_overlay_t *p, uint32_t *pal) {
    memset(p, 0, sizeof(*p));
    if (!o || o->src_w <= 0 || o->src_h <= 0) return MARS_ERR_INVALID_FILE;
    if (!mhip_frame_format_ok(o->src_format, o->src_flags) || !mhip_frame_bytes(o->src_w, o->src_h, o->src_format)) return MARS_ERR_INVALID_FILE;
    if ((o->layers & ~ALL_LAYERS) || (o->text & ~ALL_TEXT) || (o->flags & ~MARS_OVERLAY_TRACKED_ONLY) || o->color_by < MARS_OVERLAY_BY_CLASS ||
        o->color_by > MARS_OVERLAY_FIXED)
        return MARS_ERR_INVALID_FILE;
    if (o->thickness < 0 || o->thickness > 16 || o->radius < 0 || o->radius > 8 || o->scale < 0 || o->scale > 8 || o->alpha < 0 || o->alpha > 256)
        return MARS_ERR_INVALID_FILE;
    if (!isfinite(o->min_conf) || o->min_conf < 0 || !isfinite(o->kpt_min_v) || o->kpt_min_v < 0 || o->cls_count < 0 || o->min_hits < 0)
        return MARS_ERR_INVALID_FILE;
    if (o->palette ? (o->n_palette < 1 || o->n_palette > PALETTE_MAX) : o->n_palette != 0) return MARS_ERR_INVALID_FILE;
    if (o->names ? (o->n_names < 1 || o->n_names > MARS_OVERLAY_MAX_NAMES) : o->n_names != 0) return MARS_ERR_INVALID_FILE;
    if (o->src_w > MHIP_OVERLAY_MAX_DIM || o->src_h > MHIP_OVERLAY_MAX_DIM) return MARS_ERR_INVALID_TENSOR;
    p->w = o->src_w; p->h = o->src_h; p->fmt = o->src_format;
    p->frame_stride = mhip_frame_bytes(p->w, p->h, p->fmt);
    p->layers = o->layers ? o->layers : (MARS_OVERLAY_BOXES | MARS_OVERLAY_LABELS);
    p->text = o->text ? o->text : (MARS_OVERLAY_TEXT_CLASS | MARS_OVERLAY_TEXT_CONF);
    p->color_by = o->color_by;
    p->thick = o->thickness ? o->thickness : 2; p->radius = o->radius ? o->radius : 2; p->scale = o->scale ? o->scale : 2;
    p->alpha = o->alpha ? o->alpha : 96;
    p->min_conf = o->min_conf; p->kpt_min_v = o->kpt_min_v != 0 ? o->kpt_min_v : 0.5f;
    p->cls_first = o->cls_first; p->cls_count = o->cls_count;
    p->tracked_only = (o->flags & MARS_OVERLAY_TRACKED_ONLY) != 0; p->min_hits = o->min_hits ? o->min_hits : 1;
    p->n_names = o->n_names; p->num_kpt = 1;
    const unsigned char *rgb = o->palette ? o->palette : &default_palette[0][0];
    p->n_palette = o->palette ? o->n_palette : 16;
    for (int i = 0; i < p->n_palette; i++) pal[i] = pack_colour(rgb + 3 * i, p->fmt, o->src_flags);
    const unsigned char black[3] = {0, 0, 0}, white[3] = {255, 255, 255};
    p->no_key = pack_colour(o->no_key, p->fmt, o->src_flags);
    p->text_col[0] = pack_colour(black, p->fmt, o->src_flags); p->text_col[1] = pack_colour(white, p->fmt, o->src_flags);
    return MARS_OK;
}

/* a destination that shares bytes with the source without being the source */
static int partial_overlap(const void *src, const void *dst, size_t bytes) {
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    return a != b && a < b + bytes && b < a + bytes;
}

mars_error_t mars_yolo_overlay_frames(const unsigned char *frames, int n_frames, const mars_det_t *boxes, const int *frame_of_box, int n_boxes,
                                      const int *keys, const char *texts, const uint32_t *mask_words, const int *mask_of_box, const mars_kpt_t *kpts,
                                      int num_kpt, const mars_hip_overlay_opts_t *opts, unsigned char *out, mars_overlay_stats_t *stats) {
    mhip_overlay_t p;
    uint32_t pal[PALETTE_MAX];
    const mars_error_t e = overlay_opts(opts, &p, pal);
    if (e != MARS_OK) return e;
    if (!frames || !out || n_frames <= 0 || n_frames > 65535 || n_boxes < 0 || n_boxes > 65535 || (n_boxes > 0 && (!boxes || !frame_of_box)) ||
        (kpts && (num_kpt < 1 || num_kpt > MARS_POSE_MAX_KPT)))
        return MARS_ERR_INVALID_FILE;
    const size_t in_b = p.frame_stride * (size_t)n_frames;
    if (partial_overlap(frames, out, in_b)) return MARS_ERR_INVALID_FILE;
    int n_masks = 0;
    for (int i = 0; mask_of_box && i < n_boxes; i++)
        if (mask_of_box[i] >= n_masks) n_masks = mask_of_box[i] + 1;
    if (n_masks > 0 && !mask_words) return MARS_ERR_INVALID_FILE;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const int K = kpts ? num_kpt : 1;
    /* the boxes as per-frame lists, as in mars_yolo_redact_frames, and everything that belongs to a box in the same order */
    const size_t nb1 = (size_t)(n_boxes > 0 ? n_boxes : 1);
    int *lists = (int *)calloc(2 * (size_t)n_frames + 2 * nb1, sizeof(int)); /* list_off, counts, mask_of, keys */
    mars_det_t *packed = (mars_det_t *)malloc(nb1 * sizeof(mars_det_t));
    char *ptexts = (char *)calloc(nb1, MARS_OVERLAY_TEXT_MAX);
    mars_kpt_t *pk = (mars_kpt_t *)calloc(nb1 * (size_t)K, sizeof(mars_kpt_t));
    if (!lists || !packed || !ptexts || !pk) {
        free(lists); free(packed); free(ptexts); free(pk);
        return MARS_ERR_ALLOC_FAILED;
    }
    int *list_off = lists, *counts = lists + n_frames, *mask_of = lists + 2 * (size_t)n_frames, *pkeys = mask_of + nb1;
    for (int i = 0; i < n_boxes; i++)
        if (frame_of_box[i] >= 0 && frame_of_box[i] < n_frames) counts[frame_of_box[i]]++;
    for (int f = 0, acc = 0; f < n_frames; f++) { list_off[f] = acc; acc += counts[f]; counts[f] = 0; }
    for (int i = 0; i < n_boxes; i++) {
        const int f = frame_of_box[i];
        if (f < 0 || f >= n_frames) continue;
        const int k = list_off[f] + counts[f]++;
        packed[k] = boxes[i];
        mask_of[k] = mask_of_box ? mask_of_box[i] : -1;
        if (keys) pkeys[k] = keys[i];
        if (texts) memcpy(ptexts + (size_t)k * MARS_OVERLAY_TEXT_MAX, texts + (size_t)i * MARS_OVERLAY_TEXT_MAX, MARS_OVERLAY_TEXT_MAX);
        if (kpts) memcpy(pk + (size_t)k * K, kpts + (size_t)i * K, (size_t)K * sizeof(mars_kpt_t));
    }
    /* one device block: [frames][out][boxes][lists][texts][keypoints][table][markers][table_n, marks_n][stats][palette][names][mask words] */
    const int oop = out != frames;
    const size_t mask_b = (size_t)n_masks * p.h * ((p.w + 31) / 32) * sizeof(uint32_t);
    const size_t names_b = opts->names ? (size_t)opts->n_names * MARS_OVERLAY_NAME_LEN : 0;
    const size_t sz[13] = {in_b, oop ? in_b : 0, nb1 * sizeof(mars_det_t), (2 * (size_t)n_frames + 2 * nb1) * sizeof(int), nb1 * MARS_OVERLAY_TEXT_MAX,
                           nb1 * K * sizeof(mars_kpt_t), nb1 * MHIP_OVERLAY_REC_INTS * sizeof(int), nb1 * K * 4 * sizeof(int), 2 * (size_t)n_frames * sizeof(int),
                           (size_t)n_frames * sizeof(mars_overlay_stats_t), PALETTE_MAX * sizeof(uint32_t), names_b, mask_b};
    size_t off[13];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 13, off));
    int rc = d ? 0 : -1;
    if (d) {
        p.frames = d; p.dst = oop ? d + off[1] : d; p.n_frames = n_frames;
        p.dets = d + off[2];
        p.list_off = (const int *)(d + off[3]); p.counts = p.list_off + n_frames; p.mask_of = n_masks ? p.list_off + 2 * (size_t)n_frames : NULL;
        p.keys = keys ? p.list_off + 2 * (size_t)n_frames + nb1 : NULL;
        p.select_all = 1; p.tracked_only = 0;
        p.texts = texts ? (const char *)(d + off[4]) : NULL;
        if (kpts) { p.kpts = d + off[5]; p.kpt_rows = 1; p.num_kpt = K; }
        p.table = (int *)(d + off[6]); p.marks = (int *)(d + off[7]);
        p.table_n = (int *)(d + off[8]); p.marks_n = p.table_n + n_frames; p.stats = (int *)(d + off[9]);
        p.palette = (const uint32_t *)(d + off[10]);
        p.names = names_b ? (const char *)(d + off[11]) : NULL;
        p.mask_words = n_masks ? (const uint32_t *)(d + off[12]) : NULL;
        rc = mhip_h2d_async(d, frames, in_b);
        if (!rc) rc = mhip_h2d_async(d + off[2], packed, sz[2]);
        if (!rc) rc = mhip_h2d_async(d + off[3], lists, sz[3]);
        if (!rc && texts) rc = mhip_h2d_async(d + off[4], ptexts, sz[4]);
        if (!rc && kpts) rc = mhip_h2d_async(d + off[5], pk, sz[5]);
        if (!rc) rc = mhip_h2d_async(d + off[10], pal, sz[10]);
        if (!rc && names_b) rc = mhip_h2d_async(d + off[11], opts->names, names_b);
        if (!rc && n_masks) rc = mhip_h2d_async(d + off[12], mask_words, mask_b);
        if (!rc) rc = mhip_overlay_select(&p);
        if (!rc) rc = mhip_overlay(&p);
        if (!rc) rc = mhip_d2h_async(out, p.dst, in_b);
        if (!rc && stats) rc = mhip_d2h_async(stats, p.stats, sz[9]);
        if (mhip_sync()) rc = -1;
        mhip_free(d);
    }
    free(lists); free(packed); free(ptexts); free(pk);
    return !d ? MARS_ERR_ALLOC_FAILED : rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_hip_overlay_device(mars_model_t *det_model, void *frames_dev, void *dst_dev, const mars_hip_overlay_opts_t *opts) {
    if (!det_model || !frames_dev || !opts) return MARS_ERR_INVALID_FILE;
    mhip_overlay_t p;
    uint32_t pal[PALETTE_MAX];
    mars_error_t e = overlay_opts(opts, &p, pal);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)det_model;
    if ((e = mars_stage_guard(m)) != MARS_OK) return e;
    if (!dst_dev) dst_dev = frames_dev;
    const int B = m->batch;
    if (partial_overlap(frames_dev, dst_dev, p.frame_stride * (size_t)B)) return MARS_ERR_INVALID_FILE;
    if (!mars_has_dets(m) || B > 65535) return MARS_ERR_INVALID_TENSOR; /* no detections in HBM */
    if (p.tracked_only || p.color_by == MARS_OVERLAY_BY_TRACK || ((p.layers & MARS_OVERLAY_LABELS) && (p.text & MARS_OVERLAY_TEXT_TRACK))) {
        if (!m->track.dev || m->track.frames != B) return MARS_ERR_INVALID_TENSOR; /* the track ids of this batch */
        p.tracks = m->track.dev;
    }
    if (p.layers & MARS_OVERLAY_MASKS) { /* the native mask results of this batch, on the frames' own grid */
        if (!m->segn.dev || m->segn.frames != B || m->segn_ow != p.w || m->segn_oh != p.h) return MARS_ERR_INVALID_TENSOR;
        p.mask_recs = (const uint8_t *)m->segn.dev + m->segn_rec_off;
        p.mask_words = (const uint32_t *)((const uint8_t *)m->segn.dev + m->segn_word_off);
        p.mask_max = m->segn_max;
    }
    size_t marks = 1;
    if (p.layers & MARS_OVERLAY_KEYPOINTS) { /* the pose results of this batch */
        if (!m->pose.dev || m->pose.frames != B || m->pose_max <= 0 || m->pose_k < 1 || m->pose_k > MARS_POSE_MAX_KPT) return MARS_ERR_INVALID_TENSOR;
        p.pose_recs = (const uint8_t *)m->pose.dev + m->pose_rec_off;
        p.kpts = (const uint8_t *)m->pose.dev + m->pose_kpt_off;
        p.pose_max = m->pose_max; p.num_kpt = m->pose_k;
        marks = (size_t)m->pose_max * m->pose_k;
    }
    /* the palette and the names as they go up: a call with the same ones as the last uploads nothing */
    const size_t names_b = opts->names ? (size_t)opts->n_names * MARS_OVERLAY_NAME_LEN : 0, img_b = sizeof(pal) + names_b;
    uint8_t *img = (uint8_t *)calloc(1, img_b);
    if (!img) return MARS_ERR_ALLOC_FAILED;
    memcpy(img, pal, (size_t)p.n_palette * sizeof(uint32_t));
    if (names_b) memcpy(img + sizeof(pal), opts->names, names_b);
    /* the block: palette + names (at its start: their place does not move with the batch), the element table (an element per detection at
     * most), the marker table, both counts, the statistics */
    const size_t sz[5] = {sizeof(pal) + (size_t)MARS_OVERLAY_MAX_NAMES * MARS_OVERLAY_NAME_LEN, (size_t)B * MARS_YOLO_MAX_DET * MHIP_OVERLAY_REC_INTS * sizeof(int),
                          (size_t)B * marks * 4 * sizeof(int), 2 * (size_t)B * sizeof(int), (size_t)B * sizeof(mars_overlay_stats_t)};
    size_t off[5];
    int fresh = 0;
    e = mars_block_reserve(&m->overlay, mars_block_layout(sz, 5, off), 1, &fresh);
    if (e == MARS_OK && !m->ev_redact_done && !(m->ev_redact_done = mhip_event_create_sync())) e = MARS_ERR_ALLOC_FAILED;
    if (e != MARS_OK) {
        free(img);
        return e;
    }
    uint8_t *blk = (uint8_t *)m->overlay.dev;
    const int same = !fresh && m->overlay_img && m->overlay_img_bytes == img_b && !memcmp(m->overlay_img, img, img_b);
    m->overlay.frames = 0;
    if (!same) { /* as mars_lut_refresh: an overlay enqueued earlier may still read the old tables, and `img` is the host's */
        free(m->overlay_img);
        m->overlay_img = NULL;
        if (mhip_sync() || mhip_h2d_async(blk, img, img_b) || mhip_sync()) {
            free(img);
            return MARS_ERR_LAYER_FAILED;
        }
        m->overlay_img = img; m->overlay_img_bytes = img_b;
    } else {
        free(img);
    }
    m->overlay_stats_off = off[4];
    p.frames = (const uint8_t *)frames_dev; p.dst = (uint8_t *)dst_dev; p.n_frames = B;
    p.dets = m->det_dev; p.counts = m->det_counts_dev; p.det_cap = MARS_YOLO_MAX_DET;
    p.table = (int *)(blk + off[1]); p.marks = (int *)(blk + off[2]); p.mark_stride = marks;
    p.table_n = (int *)(blk + off[3]); p.marks_n = p.table_n + B; p.stats = (int *)(blk + off[4]);
    p.palette = (const uint32_t *)blk;
    p.names = names_b ? (const char *)(blk + sizeof(pal)) : NULL;
    /* The auxiliary stream and the redaction's event protocol (mars_redact.c): behind the detection tail, the tracker, the native masks and
     * the pose tail, which that stream carries, and behind what the main stream has been given so far, which has read the frames; the main
     * stream then waits for the overlay, so that whatever the library enqueues later sees the painted frames */
    mhip_select_stream(0);
    if ((e = mars_aux_behind_current(&m->ev_graph_done)) != MARS_OK) return e;
    int rc = mhip_event_record(m->overlay.ev[0]);
    if (!rc) rc = mhip_overlay_select(&p);
    if (!rc) rc = mhip_overlay(&p);
    if (!rc) rc = mhip_event_record(m->overlay.ev[1]);
    if (!rc) rc = mhip_event_record(m->ev_redact_done);
    mhip_select_aux(0);
    if (!rc) rc = mhip_stream_wait(0, m->ev_redact_done);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->overlay.frames = B;
    return MARS_OK;
}

mars_error_t mars_hip_overlay_results(mars_model_t *det_model, mars_overlay_stats_t *stats) {
    if (!det_model) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)det_model;
    const mars_block_part_t part = {stats, m->overlay_stats_off, (size_t)m->overlay.frames * sizeof(mars_overlay_stats_t)};
    return mars_block_fetch(&m->overlay, &part, 1, &m->tail_pending);
}

mars_error_t mars_hip_overlay(mars_model_t *det_model, unsigned char *frames, const mars_hip_overlay_opts_t *opts, mars_overlay_stats_t *stats) {
    if (!det_model || !frames || !opts) return MARS_ERR_INVALID_FILE;
    mhip_overlay_t q;
    uint32_t pal[PALETTE_MAX];
    mars_error_t e = overlay_opts(opts, &q, pal);
    if (e != MARS_OK) return e;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const int n = mars_hip_get_batch(det_model);
    if (n <= 0) return MARS_ERR_INVALID_TENSOR;
    const size_t in_b = q.frame_stride * (size_t)n;
    uint8_t *d = (uint8_t *)mhip_malloc(in_b);
    if (!d) return MARS_ERR_ALLOC_FAILED;
    mhip_select_stream(0);
    if (mhip_h2d_async(d, frames, in_b)) e = MARS_ERR_LAYER_FAILED;
    if (e == MARS_OK) e = mars_hip_overlay_device(det_model, d, NULL, opts);
    if (e == MARS_OK) e = mars_hip_overlay_results(det_model, stats); /* waits for both streams */
    else (void)mhip_sync(); /* the upload may still be running */
    if (e == MARS_OK && (mhip_d2h_async(frames, d, in_b) || mhip_sync())) e = MARS_ERR_LAYER_FAILED;
    mhip_free(d);
    return e;
}

float mars_hip_overlay_ms(mars_model_t *det_model) { return det_model ? mars_block_ms(&((mars_model_ext_t *)det_model)->overlay) : -1.0f; }
