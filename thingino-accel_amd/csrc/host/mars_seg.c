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
    void *ev[2];
} seg_call_t;

void mars_seg_release(mars_model_ext_t *m) {
    if (m->seg_dev) mhip_free(m->seg_dev);
    m->seg_dev = NULL;
    m->seg_bytes = 0;
    m->seg_frames = m->seg_max = m->seg_ph = m->seg_pw = 0;
    for (int i = 0; i < 2; i++) {
        if (m->ev_seg[i]) mhip_event_destroy(m->ev_seg[i]);
        m->ev_seg[i] = NULL;
    }
}

/* an int8 activation tensor of `want_c` channels (0: any, 1 .. MARS_SEG_MAX_NM) whose bytes the plan keeps: where they are, and that every byte
 * the kernel may touch lies inside the frame's stride */
static mars_error_t seg_tensor(const mars_model_ext_t *m, int T, int want_c, int want_h, int want_w, int *c, int *h, int *w, int *buf,
                               const int8_t **base, size_t *stride, int *pix_step, int *ch_step) {
    if (T < 0 || (uint32_t)T >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
    const mars_tensor_t *d = &m->pub.tensors[T].desc;
    int off;
    if (d->dtype != MARS_DTYPE_INT8 || m->mt[T].is_weight || mars_tensor_chw(d, c, h, w)) return MARS_ERR_INVALID_TENSOR;
    if (*c < 1 || *c > MARS_SEG_MAX_NM || (want_c && *c != want_c) || (want_h && (*h != want_h || *w != want_w))) return MARS_ERR_INVALID_TENSOR;
    if (mars_locate_i8(m, T, *c, *h, *w, 0, buf, &off, pix_step, ch_step)) return MARS_ERR_INVALID_TENSOR;
    const mtensor_t *tb = &m->mt[*buf];
    if (!tb->dev || *pix_step <= 0 || *ch_step <= 0) return MARS_ERR_INVALID_TENSOR;
    const size_t last = (size_t)off + ((size_t)*h * *w - 1) * (size_t)*pix_step + (size_t)(*c - 1) * (size_t)*ch_step;
    if (last >= tb->stride) return MARS_ERR_INVALID_TENSOR;
    *base = (const int8_t *)tb->dev + off;
    *stride = tb->stride;
    return MARS_OK;
}

static int scale_ok(float s) { return s > 0 && isfinite(s); }

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
    if (!m->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe) return MARS_ERR_INVALID_TENSOR; /* a pipe's slots own their buffers */
    seg_call_t c;
    memset(&c, 0, sizeof(c));
    mhip_seg_t *p = &c.seg;
    if (s->max_per_frame < 0 || s->max_per_frame > MARS_SEG_MAX_PER_FRAME || !isfinite(s->logit_min) || !isfinite(s->min_conf)) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_dfl_resolve(m, heads, &c.dfl);
    if (e != MARS_OK) return e;
    int ic, bufs[5], nbuf = 0, pc, nm;
    if (m->batch > 65535 || model->header.num_inputs < 1 || model->header.input_tensor_ids[0] >= model->header.num_tensors ||
        mars_tensor_chw(&model->tensors[model->header.input_tensor_ids[0]].desc, &ic, &p->in_h, &p->in_w))
        return MARS_ERR_INVALID_TENSOR;
    e = seg_tensor(m, s->proto_tensor, 0, 0, 0, &nm, &p->ph, &p->pw, &bufs[nbuf], &p->proto, &p->proto_frame_stride, &p->proto_pix_step, &p->proto_ch_step);
    if (e != MARS_OK) return e;
    nbuf++;
    if ((long long)p->ph * ((p->pw + 31) / 32) > (1LL << 24)) return MARS_ERR_INVALID_TENSOR;
    const float ps = s->proto_scale != 0 ? s->proto_scale : model->tensors[s->proto_tensor].desc.scale;
    if (!scale_ok(ps)) return MARS_ERR_INVALID_TENSOR;
    for (int k = 0; k < c.dfl.n; k++) {
        int hh, ww;
        e = seg_tensor(m, s->coef_tensors[k], nm, c.dfl.h[k], c.dfl.w[k], &pc, &hh, &ww, &bufs[nbuf], &p->coef[k], &p->coef_frame_stride[k],
                       &p->coef_pix_step[k], &p->coef_ch_step[k]);
        if (e != MARS_OK) return e;
        nbuf++;
        const float cs = s->coef_scales[k] != 0 ? s->coef_scales[k] : model->tensors[s->coef_tensors[k]].desc.scale;
        if (!scale_ok(cs)) return MARS_ERR_INVALID_TENSOR;
        p->scale[k] = cs * ps; /* one float32 product (-ffp-contract=off) */
        p->cells[k] = hh * ww;
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
    const size_t kept_off = ALIGN_UP(B * MARS_YOLO_MAX_DET * sizeof(int), 256), pre_off = 2 * kept_off;
    const size_t rec_off = pre_off + ALIGN_UP(B * MARS_YOLO_MAX_DET * sizeof(mars_det_t), 256);
    const size_t word_off = rec_off + ALIGN_UP(B * p->max_per_frame * sizeof(mars_mask_t), 256);
    const size_t total = word_off + ALIGN_UP(B * p->max_per_frame * units * sizeof(uint32_t), 256);
    if (!m->seg_dev || m->seg_bytes < total) {
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: an earlier tail may still use the old block */
        if (m->seg_dev) mhip_free(m->seg_dev);
        m->seg_frames = 0; m->seg_bytes = 0;
        m->seg_dev = mhip_malloc(total);
        if (!m->seg_dev) return MARS_ERR_ALLOC_FAILED;
        m->seg_bytes = total;
    }
    for (int i = 0; i < 2; i++) {
        if (!m->ev_seg[i]) m->ev_seg[i] = mhip_event_create();
        if (!m->ev_seg[i]) return MARS_ERR_ALLOC_FAILED;
        c.ev[i] = m->ev_seg[i];
    }
    uint8_t *blk = (uint8_t *)m->seg_dev;
    c.dfl.cand_pred = (int *)blk;
    c.dfl.kept_pred = (int *)(blk + kept_off);
    c.dfl.premap = blk + pre_off;
    p->pred = c.dfl.kept_pred;
    p->recs = blk + rec_off;
    p->words = (uint32_t *)(blk + word_off);
    /* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
    for (int k = 0; k < c.dfl.n; k++) m->mt[c.dfl.box_buf[k]].tail_read = m->mt[c.dfl.cls_buf[k]].tail_read = 1;
    for (int i = 0; i < nbuf; i++) m->mt[bufs[i]].tail_read = 1;
    m->seg_frames = 0;
    e = mars_tail_on_aux(m, seg_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = c.dfl.map;
    m->seg_rec_off = rec_off; m->seg_word_off = word_off;
    m->seg_frames = m->batch; m->seg_max = p->max_per_frame; m->seg_ph = p->ph; m->seg_pw = p->pw;
    return MARS_OK;
}

mars_error_t mars_hip_mask_results(mars_model_t *model, mars_mask_t *recs, uint32_t *words, int *ph, int *pw, int *pitch_words) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->seg_dev || m->seg_frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no seg call yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    m->tail_pending = 0;
    const int pitch = (m->seg_pw + 31) / 32;
    const size_t slots = (size_t)m->seg_frames * m->seg_max;
    if ((recs && mhip_d2h_async(recs, (uint8_t *)m->seg_dev + m->seg_rec_off, slots * sizeof(mars_mask_t))) ||
        (words && mhip_d2h_async(words, (uint8_t *)m->seg_dev + m->seg_word_off, slots * m->seg_ph * pitch * sizeof(uint32_t))) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
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

float mars_hip_mask_ms(mars_model_t *model) {
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m || !m->seg_dev || m->seg_frames <= 0 || !m->ev_seg[0] || !m->ev_seg[1]) return -1.0f;
    return mhip_event_elapsed_ms(m->ev_seg[0], m->ev_seg[1]);
}

int mars_yolo_masks(const int8_t *coefs, int n, int nm, const int8_t *proto, int ph, int pw, const mars_det_t *boxes, int in_w, int in_h, float s,
                    float logit_min, mars_mask_t *recs, uint32_t *words) {
    if (n < 0 || n > MARS_SEG_MAX_PER_FRAME || nm < 1 || nm > MARS_SEG_MAX_NM || ph <= 0 || pw <= 0 || in_w <= 0 || in_h <= 0 || !scale_ok(s) ||
        !isfinite(logit_min) || (long long)ph * ((pw + 31) / 32) > (1LL << 24))
        return -1;
    if (n == 0) return 0;
    if (!coefs || !proto || !boxes || !recs || !words) return -1;
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) return -1;
    const size_t units = (size_t)ph * ((pw + 31) / 32);
    const size_t coef_b = (size_t)n * nm, proto_b = (size_t)nm * ph * pw, box_b = (size_t)n * sizeof(mars_det_t), rec_b = (size_t)n * sizeof(mars_mask_t);
    const size_t word_b = (size_t)n * units * sizeof(uint32_t);
    const size_t o_proto = ALIGN_UP(coef_b, 256), o_box = o_proto + ALIGN_UP(proto_b, 256), o_cnt = o_box + ALIGN_UP(box_b, 256);
    const size_t o_pred = o_cnt + 256, o_rec = o_pred + ALIGN_UP((size_t)n * sizeof(int), 256), o_word = o_rec + ALIGN_UP(rec_b, 256);
    uint8_t *d = (uint8_t *)mhip_malloc(o_word + word_b);
    if (!d) return -1;
    int pred[MARS_SEG_MAX_PER_FRAME];
    for (int i = 0; i < n; i++) pred[i] = i; /* box i's row is "cell" i of one head of n cells */
    mhip_seg_t p;
    memset(&p, 0, sizeof(p));
    p.coef[0] = (const int8_t *)d; p.coef_pix_step[0] = nm; p.coef_ch_step[0] = 1; p.cells[0] = n; p.scale[0] = s; p.nheads = 1;
    p.proto = (const int8_t *)(d + o_proto); p.proto_pix_step = 1; p.proto_ch_step = ph * pw;
    p.nm = nm; p.ph = ph; p.pw = pw; p.in_w = in_w; p.in_h = in_h;
    p.frames = 1;
    p.boxes = d + o_box; p.counts = (const int *)(d + o_cnt); p.pred = (const int *)(d + o_pred); p.det_cap = n;
    p.logit_min = logit_min; p.select_all = 1; p.max_per_frame = n;
    p.recs = d + o_rec; p.words = (uint32_t *)(d + o_word);
    int rc = mhip_h2d_async(d, coefs, coef_b);
    if (!rc) rc = mhip_h2d_async(d + o_proto, proto, proto_b);
    if (!rc) rc = mhip_h2d_async(d + o_box, boxes, box_b);
    if (!rc) rc = mhip_h2d_async(d + o_cnt, &n, sizeof(int));
    if (!rc) rc = mhip_h2d_async(d + o_pred, pred, (size_t)n * sizeof(int));
    if (!rc) rc = mhip_seg(&p);
    if (!rc) rc = mhip_d2h_async(recs, p.recs, rec_b);
    if (!rc) rc = mhip_d2h_async(words, p.words, word_b);
    if (mhip_sync()) rc = -1; /* (`n` and `pred` are on this stack frame) */
    mhip_free(d);
    return rc ? -1 : 0;
}
