/*
 * mars_seg.c -- host side of the instance masks (include/mars_hip.h, "Instance masks"): argument checks, where the plan left the coefficient
 * and prototype tensors' bytes, the result block hung on the model, stream ordering, and the launches of csrc/hip/seg.hip behind the DFL
 * tail of csrc/hip/yolo_tail.hip (which records the origin of every kept detection for it).  The reference has no segmentation head.  There
 * is no CPU path: without the device every entry point fails.  The second half is "Instance masks in frame pixels": the same tail with the
 * masks of csrc/hip/seg_native.hip on the caller's grid, its geometry and tap tables made here, its results in a block of their own.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"
#include "nna.h"

typedef struct {
    mars_dfl_cfg_t dfl;
    mhip_seg_t seg;
    void *const *ev; /* the block's two timing events */
} seg_call_t;

typedef struct {
    seg_call_t call;
    mhip_seg_native_t nat;
} segn_call_t;

static int seg_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    const seg_call_t *c = (const seg_call_t *)cfg;
    int rc = mars_dfl_launch(m, &c->dfl, dets_dev, counts_dev);
    if (rc) return rc;
    mhip_seg_t p = c->seg;
    p.boxes = c->dfl.map ? c->dfl.premap : dets_dev; /* graph-input pixels: the records before the letterbox mapping */
    p.counts = counts_dev;
    rc = mhip_event_record(c->ev[0]);
    if (!rc) rc = mhip_seg(&p);
    if (!rc) rc = mhip_event_record(c->ev[1]);
    return rc;
}

/* the checks and everything of the call that does not depend on where the results go: the DFL heads, the mask tensors, the scales and the
 * options into *c, the buffers the tail reads besides the heads' into bufs[0 .. *nbuf).  Touches nothing on the device. */
static mars_error_t seg_resolve(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *s, seg_call_t *c, int bufs[5],
                                int *nbuf_out) {
    if (!model || !s) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mars_error_t e = mars_stage_guard(m);
    if (e != MARS_OK) return e;
    memset(c, 0, sizeof(*c));
    mhip_seg_t *p = &c->seg;
    int nbuf = 0;
    if (s->max_per_frame < 0 || s->max_per_frame > MARS_SEG_MAX_PER_FRAME || !isfinite(s->logit_min) || !isfinite(s->min_conf)) return MARS_ERR_INVALID_TENSOR;
    e = mars_dfl_resolve(m, heads, &c->dfl);
    if (e != MARS_OK) return e;
    int ic;
    if (m->batch > 65535 || model->header.num_inputs < 1 || model->header.input_tensor_ids[0] >= model->header.num_tensors ||
        mars_tensor_chw(&model->tensors[model->header.input_tensor_ids[0]].desc, &ic, &p->in_h, &p->in_w))
        return MARS_ERR_INVALID_TENSOR;
    /* 1 .. MARS_SEG_MAX_NM channels; a one-channel map whose channel step is not positive stays refused here (mars_side_tensor) */
    mars_side_tensor_t t;
    e = mars_side_tensor(m, s->proto_tensor, 0, 0, 0, &t);
    if (e != MARS_OK) return e;
    if (t.c > MARS_SEG_MAX_NM || t.ch_step <= 0) return MARS_ERR_INVALID_TENSOR;
    const int nm = t.c;
    p->ph = t.h; p->pw = t.w; p->proto = t.base; p->proto_frame_stride = t.stride; p->proto_pix_step = t.pix_step; p->proto_ch_step = t.ch_step;
    bufs[nbuf++] = t.buf;
    if ((long long)p->ph * ((p->pw + 31) / 32) > (1LL << 24)) return MARS_ERR_INVALID_TENSOR;
    const float ps = s->proto_scale != 0 ? s->proto_scale : model->tensors[s->proto_tensor].desc.scale;
    if (!mars_scale_ok(ps)) return MARS_ERR_INVALID_TENSOR;
    for (int k = 0; k < c->dfl.n; k++) {
        e = mars_side_tensor(m, s->coef_tensors[k], nm, c->dfl.h[k], c->dfl.w[k], &t);
        if (e != MARS_OK) return e;
        if (t.ch_step <= 0) return MARS_ERR_INVALID_TENSOR;
        p->coef[k] = t.base; p->coef_frame_stride[k] = t.stride; p->coef_pix_step[k] = t.pix_step; p->coef_ch_step[k] = t.ch_step;
        bufs[nbuf++] = t.buf;
        const float cs = s->coef_scales[k] != 0 ? s->coef_scales[k] : model->tensors[s->coef_tensors[k]].desc.scale;
        if (!mars_scale_ok(cs)) return MARS_ERR_INVALID_TENSOR;
        p->scale[k] = cs * ps; /* one float32 product (-ffp-contract=off) */
        p->cells[k] = t.h * t.w;
    }
    p->nheads = c->dfl.n;
    p->nm = nm;
    p->frames = m->batch;
    p->det_cap = MARS_YOLO_MAX_DET;
    p->logit_min = s->logit_min;
    p->min_conf = s->min_conf;
    p->max_per_frame = s->max_per_frame ? s->max_per_frame : 16;
    *nbuf_out = nbuf;
    return MARS_OK;
}

/* after every refusal: the detection buffers and the decode tables (allocates, uploads and synchronises where they change) */
static mars_error_t seg_prepare(mars_model_ext_t *m, const mars_dfl_cfg_t *d) {
    const mars_error_t e = mars_own_det_buffers(m);
    return e != MARS_OK ? e : mars_dfl_prepare(m, d);
}

/* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
static void seg_mark_reads(mars_model_ext_t *m, const mars_dfl_cfg_t *d, const int *bufs, int nbuf) {
    for (int k = 0; k < d->n; k++) m->mt[d->box_buf[k]].tail_read = m->mt[d->cls_buf[k]].tail_read = 1;
    for (int i = 0; i < nbuf; i++) m->mt[bufs[i]].tail_read = 1;
}

mars_error_t mars_hip_detect_seg_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *s) {
    seg_call_t c;
    int bufs[5], nbuf;
    mars_error_t e = seg_resolve(model, heads, s, &c, bufs, &nbuf);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mhip_seg_t *p = &c.seg;
    e = seg_prepare(m, &c.dfl);
    if (e != MARS_OK) return e;
    /* the block: candidate origins, kept origins, pre-map boxes, records, words */
    const size_t B = (size_t)m->batch, units = (size_t)p->ph * ((p->pw + 31) / 32);
    const size_t sz[5] = {B * MARS_YOLO_MAX_DET * sizeof(int), B * MARS_YOLO_MAX_DET * sizeof(int), B * MARS_YOLO_MAX_DET * sizeof(mars_det_t),
                          B * p->max_per_frame * sizeof(mars_mask_t), B * p->max_per_frame * units * sizeof(uint32_t)};
    size_t off[5];
    e = mars_block_reserve(&m->seg, mars_block_layout(sz, 5, off), 1, NULL);
    if (e != MARS_OK) return e;
    c.ev = m->seg.ev;
    uint8_t *blk = (uint8_t *)m->seg.dev;
    c.dfl.cand_pred = (int *)blk;
    c.dfl.kept_pred = (int *)(blk + off[1]);
    c.dfl.premap = blk + off[2];
    p->pred = c.dfl.kept_pred;
    p->recs = blk + off[3];
    p->words = (uint32_t *)(blk + off[4]);
    seg_mark_reads(m, &c.dfl, bufs, nbuf);
    m->seg.frames = 0;
    e = mars_tail_on_aux(m, seg_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = c.dfl.map;
    m->seg_rec_off = off[3]; m->seg_word_off = off[4];
    m->seg.frames = m->batch; m->seg_max = p->max_per_frame; m->seg_ph = p->ph; m->seg_pw = p->pw;
    return MARS_OK;
}

mars_error_t mars_hip_mask_results(mars_model_t *model, mars_mask_t *recs, uint32_t *words, int *ph, int *pw, int *pitch_words) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    const int pitch = (m->seg_pw + 31) / 32;
    const size_t slots = (size_t)m->seg.frames * m->seg_max;
    const mars_block_part_t parts[2] = {{recs, m->seg_rec_off, slots * sizeof(mars_mask_t)},
                                        {words, m->seg_word_off, slots * m->seg_ph * pitch * sizeof(uint32_t)}};
    const mars_error_t e = mars_block_fetch(&m->seg, parts, 2, &m->tail_pending);
    if (e != MARS_OK) return e;
    if (ph) *ph = m->seg_ph;
    if (pw) *pw = m->seg_pw;
    if (pitch_words) *pitch_words = pitch;
    return MARS_OK;
}

mars_error_t mars_hip_detect_seg(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *s, mars_det_t *dets, int *counts,
                                 mars_mask_t *recs, uint32_t *words) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_seg_device(model, heads, s);
    if (e == MARS_OK) e = mars_hip_detect_results(model, dets, counts);
    return e != MARS_OK ? e : mars_hip_mask_results(model, recs, words, NULL, NULL, NULL);
}

float mars_hip_mask_ms(mars_model_t *model) { return model ? mars_block_ms(&((mars_model_ext_t *)model)->seg) : -1.0f; }

int mars_yolo_masks(const int8_t *coefs, int n, int nm, const int8_t *proto, int ph, int pw, const mars_det_t *boxes, int in_w, int in_h, float s,
                    float logit_min, mars_mask_t *recs, uint32_t *words) {
    if (n < 0 || n > MARS_SEG_MAX_PER_FRAME || nm < 1 || nm > MARS_SEG_MAX_NM || ph <= 0 || pw <= 0 || in_w <= 0 || in_h <= 0 || !mars_scale_ok(s) ||
        !isfinite(logit_min) || (long long)ph * ((pw + 31) / 32) > (1LL << 24))
        return -1;
    if (n == 0) return 0;
    if (!coefs || !proto || !boxes || !recs || !words) return -1;
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) return -1;
    const size_t units = (size_t)ph * ((pw + 31) / 32);
    /* one scratch block: [coefs][proto][boxes][count][pred][recs][words] */
    const size_t sz[7] = {(size_t)n * nm, (size_t)nm * ph * pw, (size_t)n * sizeof(mars_det_t), sizeof(int), (size_t)n * sizeof(int),
                          (size_t)n * sizeof(mars_mask_t), (size_t)n * units * sizeof(uint32_t)};
    size_t off[7];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 7, off));
    if (!d) return -1;
    int pred[MARS_SEG_MAX_PER_FRAME];
    for (int i = 0; i < n; i++) pred[i] = i; /* box i's row is "cell" i of one head of n cells */
    mhip_seg_t p;
    memset(&p, 0, sizeof(p));
    p.coef[0] = (const int8_t *)d; p.coef_pix_step[0] = nm; p.coef_ch_step[0] = 1; p.cells[0] = n; p.scale[0] = s; p.nheads = 1;
    p.proto = (const int8_t *)(d + off[1]); p.proto_pix_step = 1; p.proto_ch_step = ph * pw;
    p.nm = nm; p.ph = ph; p.pw = pw; p.in_w = in_w; p.in_h = in_h;
    p.frames = 1;
    p.boxes = d + off[2]; p.counts = (const int *)(d + off[3]); p.pred = (const int *)(d + off[4]); p.det_cap = n;
    p.logit_min = logit_min; p.select_all = 1; p.max_per_frame = n;
    p.recs = d + off[5]; p.words = (uint32_t *)(d + off[6]);
    int rc = mhip_h2d_async(d, coefs, sz[0]);
    if (!rc) rc = mhip_h2d_async(d + off[1], proto, sz[1]);
    if (!rc) rc = mhip_h2d_async(d + off[2], boxes, sz[2]);
    if (!rc) rc = mhip_h2d_async(d + off[3], &n, sizeof(int));
    if (!rc) rc = mhip_h2d_async(d + off[4], pred, sz[4]);
    if (!rc) rc = mhip_seg(&p);
    if (!rc) rc = mhip_d2h_async(recs, p.recs, sz[5]);
    if (!rc) rc = mhip_d2h_async(words, p.words, sz[6]);
    if (mhip_sync()) rc = -1; /* (`n` and `pred` are on this stack frame) */
    mhip_free(d);
    return rc ? -1 : 0;
}

/* ---- instance masks in frame pixels */
#define MASK_AXIS_MAX (1 << 20) /* in_n and P: every int64 term of the taps stays below 2^56 */

int mars_yolo_mask_taps(int out_n, int in_n, int n_content, int pad, int P, int *ia, int *ib, int *w1) {
    if (out_n < 1 || out_n > MARS_MASK_NATIVE_MAX || in_n < 1 || in_n > MASK_AXIS_MAX || P < 1 || P > MASK_AXIS_MAX || n_content < 1 || pad < 0 ||
        (long long)pad + n_content > in_n || !ia || !ib || !w1 || (long long)out_n * in_n < (long long)n_content * P)
        return -1;
    const int64_t D = 2 * (int64_t)out_n * in_n, step = 2 * (int64_t)n_content * P;
    int64_t N = (int64_t)n_content * P + 2 * (int64_t)out_n * pad * P - (int64_t)out_n * in_n; /* X = 0; + step per column */
    for (int X = 0; X < out_n; X++, N += step) {
        int64_t i0 = N / D;
        if (N % D < 0) i0--; /* C division truncates: a true floor */
        const int64_t r = N - i0 * D;
        w1[X] = (int)((r * 256) / D);
        ia[X] = (int)(i0 < 0 ? 0 : i0 > P - 1 ? P - 1 : i0);
        ib[X] = (int)(i0 + 1 < 0 ? 0 : i0 + 1 > P - 1 ? P - 1 : i0 + 1);
    }
    return 0;
}

/* both axes' tables as seg_native.hip reads them: [ia][ib][w1] of out_w, then of out_h; tab holds 3 * (out_w + out_h) ints */
static int mask_tap_tables(const mars_mask_geom_t *g, int ph, int pw, int *tab) {
    int *x = tab, *y = tab + 3 * (size_t)g->out_w;
    return mars_yolo_mask_taps(g->out_w, g->in_w, g->nw, g->px, pw, x, x + g->out_w, x + 2 * (size_t)g->out_w) ||
           mars_yolo_mask_taps(g->out_h, g->in_h, g->nh, g->py, ph, y, y + g->out_h, y + 2 * (size_t)g->out_h);
}

/* the range checks of a geometry that the tap tables do not make */
static int mask_geom_ok(const mars_mask_geom_t *g) {
    return g->out_w >= 1 && g->out_w <= MARS_MASK_NATIVE_MAX && g->out_h >= 1 && g->out_h <= MARS_MASK_NATIVE_MAX && g->base_w > 0 && g->base_h > 0 &&
           (long long)g->out_h * ((g->out_w + 31) / 32) <= (1LL << 24);
}

static int segn_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    const segn_call_t *c = (const segn_call_t *)cfg;
    int rc = mars_dfl_launch(m, &c->call.dfl, dets_dev, counts_dev);
    if (rc) return rc;
    mhip_seg_native_t p = c->nat;
    p.seg.boxes = dets_dev; /* the records mars_hip_detect_results returns: the base grid is theirs */
    p.seg.counts = counts_dev;
    rc = mhip_event_record(c->call.ev[0]);
    if (!rc) rc = mhip_seg_native(&p);
    if (!rc) rc = mhip_event_record(c->call.ev[1]);
    return rc;
}

mars_error_t mars_hip_detect_seg_native_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *s,
                                               const mars_hip_mask_native_opts_t *nat) {
    segn_call_t c;
    int bufs[5], nbuf;
    mars_error_t e = seg_resolve(model, heads, s, &c.call, bufs, &nbuf);
    if (e != MARS_OK) return e;
    if (nat && (nat->flags || nat->out_w < 0 || nat->out_h < 0 || nat->out_w > MARS_MASK_NATIVE_MAX || nat->out_h > MARS_MASK_NATIVE_MAX))
        return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    const mars_dfl_cfg_t *d = &c.call.dfl;
    mhip_seg_t *p = &c.call.seg;
    mars_mask_geom_t g = {p->in_w, p->in_h, p->in_w, p->in_h, 0, 0, p->in_w, p->in_h, 0, 0};
    if (d->map) {
        g.nw = d->nw; g.nh = d->nh; g.px = d->px; g.py = d->py;
        g.base_w = heads->src_w; g.base_h = heads->src_h; /* (map != 0: heads is there and both are positive) */
    }
    g.out_w = nat && nat->out_w ? nat->out_w : g.base_w;
    g.out_h = nat && nat->out_h ? nat->out_h : g.base_h;
    if (!mask_geom_ok(&g)) return MARS_ERR_INVALID_TENSOR;
    const int key[10] = {g.in_w, g.in_h, g.nw, g.nh, g.px, g.py, p->ph, p->pw, g.out_w, g.out_h};
    /* the block: the tap tables (at its start: their place does not move with the batch), candidate origins, kept origins, records, words */
    const size_t B = (size_t)m->batch, units = (size_t)g.out_h * ((g.out_w + 31) / 32);
    const size_t sz[5] = {6 * MARS_MASK_NATIVE_MAX * sizeof(int), B * MARS_YOLO_MAX_DET * sizeof(int), B * MARS_YOLO_MAX_DET * sizeof(int),
                          B * p->max_per_frame * sizeof(mars_mask_t), B * p->max_per_frame * units * sizeof(uint32_t)};
    size_t off[5];
    /* the tables of this call's geometry: a down-scale is refused here, before the block is touched */
    const size_t ntab = 3 * ((size_t)g.out_w + g.out_h);
    int *tab = (int *)malloc(ntab * sizeof(int));
    if (!tab) return MARS_ERR_ALLOC_FAILED;
    if (mask_tap_tables(&g, p->ph, p->pw, tab)) {
        free(tab);
        return MARS_ERR_INVALID_TENSOR;
    }
    int fresh = 0;
    e = seg_prepare(m, d); /* every refusal is behind: from here on the call allocates and uploads */
    if (e == MARS_OK) e = mars_block_reserve(&m->segn, mars_block_layout(sz, 5, off), 1, &fresh);
    if (fresh) memset(m->segn_key, 0, sizeof(m->segn_key));
    uint8_t *blk = (uint8_t *)m->segn.dev;
    if (e == MARS_OK && memcmp(m->segn_key, key, sizeof(key))) {
        /* they depend only on the geometry: uploaded when it changes; synchronises around the upload, as the scale-keyed tables do (an
         * earlier call on the auxiliary stream may still read the old ones, and `tab` is released below) */
        m->segn.frames = 0;
        memset(m->segn_key, 0, sizeof(m->segn_key));
        if (mhip_sync() || mhip_h2d_async(blk, tab, ntab * sizeof(int)) || mhip_sync()) e = MARS_ERR_LAYER_FAILED;
        else memcpy(m->segn_key, key, sizeof(key));
    }
    free(tab);
    if (e != MARS_OK) return e;
    c.call.ev = m->segn.ev;
    c.call.dfl.cand_pred = (int *)(blk + off[1]);
    c.call.dfl.kept_pred = (int *)(blk + off[2]);
    p->pred = c.call.dfl.kept_pred;
    p->recs = blk + off[3];
    p->words = (uint32_t *)(blk + off[4]);
    p->in_w = g.base_w; p->in_h = g.base_h; /* the selection's rectangles: boxes on the base grid -> the output grid */
    for (int k = 0; k < p->nheads; k++) p->scale[k] = p->scale[k] * 1.52587890625e-05f; /* s16: one float32 product (exact but for underflow) */
    c.nat.seg = *p;
    c.nat.out_w = g.out_w; c.nat.out_h = g.out_h;
    c.nat.taps = (const int *)blk;
    seg_mark_reads(m, d, bufs, nbuf);
    m->segn.frames = 0;
    e = mars_tail_on_aux(m, segn_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = d->map;
    m->segn_rec_off = off[3]; m->segn_word_off = off[4];
    m->segn.frames = m->batch; m->segn_max = p->max_per_frame; m->segn_oh = g.out_h; m->segn_ow = g.out_w;
    return MARS_OK;
}

mars_error_t mars_hip_mask_native_results(mars_model_t *model, mars_mask_t *recs, uint32_t *words, int *out_h, int *out_w, int *pitch_words) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    const int pitch = (m->segn_ow + 31) / 32;
    const size_t slots = (size_t)m->segn.frames * m->segn_max;
    const mars_block_part_t parts[2] = {{recs, m->segn_rec_off, slots * sizeof(mars_mask_t)},
                                        {words, m->segn_word_off, slots * m->segn_oh * pitch * sizeof(uint32_t)}};
    const mars_error_t e = mars_block_fetch(&m->segn, parts, 2, &m->tail_pending);
    if (e != MARS_OK) return e;
    if (out_h) *out_h = m->segn_oh;
    if (out_w) *out_w = m->segn_ow;
    if (pitch_words) *pitch_words = pitch;
    return MARS_OK;
}

mars_error_t mars_hip_detect_seg_native(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *s,
                                        const mars_hip_mask_native_opts_t *nat, mars_det_t *dets, int *counts, mars_mask_t *recs, uint32_t *words) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_seg_native_device(model, heads, s, nat);
    if (e == MARS_OK) e = mars_hip_detect_results(model, dets, counts);
    return e != MARS_OK ? e : mars_hip_mask_native_results(model, recs, words, NULL, NULL, NULL);
}

float mars_hip_mask_native_ms(mars_model_t *model) { return model ? mars_block_ms(&((mars_model_ext_t *)model)->segn) : -1.0f; }

int mars_yolo_masks_native(const int8_t *coefs, int n, int nm, const int8_t *proto, int ph, int pw, const mars_det_t *boxes, const mars_mask_geom_t *g,
                           float s, float logit_min, mars_mask_t *recs, uint32_t *words) {
    if (n < 0 || n > MARS_SEG_MAX_PER_FRAME || nm < 1 || nm > MARS_SEG_MAX_NM || ph <= 0 || pw <= 0 || !g || !mask_geom_ok(g) || !mars_scale_ok(s) ||
        !isfinite(logit_min) || (long long)ph * ((pw + 31) / 32) > (1LL << 24))
        return -1;
    const size_t ntab = 3 * ((size_t)g->out_w + g->out_h);
    int *tab = (int *)malloc(ntab * sizeof(int));
    if (!tab) return -1;
    uint8_t *d = NULL;
    int rc = mask_tap_tables(g, ph, pw, tab) ? -1 : 0;
    if (rc || n == 0) goto done;
    rc = -1;
    if (!coefs || !proto || !boxes || !recs || !words) goto done;
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) goto done;
    {
        const size_t units = (size_t)g->out_h * ((g->out_w + 31) / 32);
        /* one scratch block: [coefs][proto][boxes][count][pred][taps][recs][words] */
        const size_t sz[8] = {(size_t)n * nm, (size_t)nm * ph * pw, (size_t)n * sizeof(mars_det_t), sizeof(int), (size_t)n * sizeof(int),
                              ntab * sizeof(int), (size_t)n * sizeof(mars_mask_t), (size_t)n * units * sizeof(uint32_t)};
        size_t off[8];
        d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 8, off));
        if (!d) goto done;
        int pred[MARS_SEG_MAX_PER_FRAME];
        for (int i = 0; i < n; i++) pred[i] = i; /* box i's row is "cell" i of one head of n cells */
        mhip_seg_native_t q;
        memset(&q, 0, sizeof(q));
        mhip_seg_t *p = &q.seg;
        p->coef[0] = (const int8_t *)d; p->coef_pix_step[0] = nm; p->coef_ch_step[0] = 1; p->cells[0] = n; p->nheads = 1;
        p->scale[0] = s * 1.52587890625e-05f;
        p->proto = (const int8_t *)(d + off[1]); p->proto_pix_step = 1; p->proto_ch_step = ph * pw;
        p->nm = nm; p->ph = ph; p->pw = pw; p->in_w = g->base_w; p->in_h = g->base_h;
        p->frames = 1;
        p->boxes = d + off[2]; p->counts = (const int *)(d + off[3]); p->pred = (const int *)(d + off[4]); p->det_cap = n;
        p->logit_min = logit_min; p->select_all = 1; p->max_per_frame = n;
        p->recs = d + off[6]; p->words = (uint32_t *)(d + off[7]);
        q.out_w = g->out_w; q.out_h = g->out_h; q.taps = (const int *)(d + off[5]);
        rc = mhip_h2d_async(d, coefs, sz[0]);
        if (!rc) rc = mhip_h2d_async(d + off[1], proto, sz[1]);
        if (!rc) rc = mhip_h2d_async(d + off[2], boxes, sz[2]);
        if (!rc) rc = mhip_h2d_async(d + off[3], &n, sizeof(int));
        if (!rc) rc = mhip_h2d_async(d + off[4], pred, sz[4]);
        if (!rc) rc = mhip_h2d_async(d + off[5], tab, sz[5]);
        if (!rc) rc = mhip_seg_native(&q);
        if (!rc) rc = mhip_d2h_async(recs, p->recs, sz[6]);
        if (!rc) rc = mhip_d2h_async(words, p->words, sz[7]);
        if (mhip_sync()) rc = -1; /* (`n`, `pred` and `tab` live until here) */
    }
done:
    if (d) mhip_free(d);
    free(tab);
    return rc ? -1 : 0;
}
