/*
 * mars_seg.c -- host side of the instance masks (include/mars_hip.h, "Instance masks"): argument checks, where the plan left the coefficient
 * and prototype tensors' bytes, the result block hung on the model, stream ordering, and the launches of csrc/hip/seg.hip behind the DFL
 * tail of csrc/hip/yolo_tail.hip (which records the origin of every kept detection for it).  The reference has no segmentation head.  There
 * is no CPU path: without the device every entry point fails.
 */
#include <math.h>
#include <stdint.h>
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

mars_error_t mars_hip_detect_seg_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_seg_opts_t *s) {
    if (!model || !s) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mars_error_t e = mars_stage_guard(m);
    if (e != MARS_OK) return e;
    seg_call_t c;
    memset(&c, 0, sizeof(c));
    mhip_seg_t *p = &c.seg;
    if (s->max_per_frame < 0 || s->max_per_frame > MARS_SEG_MAX_PER_FRAME || !isfinite(s->logit_min) || !isfinite(s->min_conf)) return MARS_ERR_INVALID_TENSOR;
    e = mars_dfl_resolve(m, heads, &c.dfl);
    if (e != MARS_OK) return e;
    int ic, bufs[5], nbuf = 0;
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
    for (int k = 0; k < c.dfl.n; k++) {
        e = mars_side_tensor(m, s->coef_tensors[k], nm, c.dfl.h[k], c.dfl.w[k], &t);
        if (e != MARS_OK) return e;
        if (t.ch_step <= 0) return MARS_ERR_INVALID_TENSOR;
        p->coef[k] = t.base; p->coef_frame_stride[k] = t.stride; p->coef_pix_step[k] = t.pix_step; p->coef_ch_step[k] = t.ch_step;
        bufs[nbuf++] = t.buf;
        const float cs = s->coef_scales[k] != 0 ? s->coef_scales[k] : model->tensors[s->coef_tensors[k]].desc.scale;
        if (!mars_scale_ok(cs)) return MARS_ERR_INVALID_TENSOR;
        p->scale[k] = cs * ps; /* one float32 product (-ffp-contract=off) */
        p->cells[k] = t.h * t.w;
    }
    p->nheads = c.dfl.n;
    p->nm = nm;
    p->frames = m->batch;
    p->det_cap = MARS_YOLO_MAX_DET;
    p->logit_min = s->logit_min;
    p->min_conf = s->min_conf;
    p->max_per_frame = s->max_per_frame ? s->max_per_frame : 16;
    e = mars_own_det_buffers(m);
    if (e == MARS_OK) e = mars_dfl_prepare(m, &c.dfl);
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
    /* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
    for (int k = 0; k < c.dfl.n; k++) m->mt[c.dfl.box_buf[k]].tail_read = m->mt[c.dfl.cls_buf[k]].tail_read = 1;
    for (int i = 0; i < nbuf; i++) m->mt[bufs[i]].tail_read = 1;
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
