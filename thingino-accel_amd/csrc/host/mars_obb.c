/*
 * mars_obb.c -- host side of the oriented boxes (include/mars_hip.h, "Oriented boxes"): argument checks, where the plan left the angle
 * tensors' bytes, the angle tables (the host's expf, cosf, sinf), the result block hung on the model, stream ordering, and the launches of
 * csrc/hip/obb.hip in the DFL tail's place.  The reference has no oriented head.  There is no CPU path: without the device every entry point
 * but mars_yolo_obb_corners fails.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"
#include "nna.h"

#define OBB_TAB (4 * 768 * sizeof(float)) /* per head ang, cs, sn: 256 floats each */

typedef struct {
    mars_dfl_cfg_t dfl;
    mhip_obb_t obb;
    void *ev[2];
} obb_call_t;

void mars_obb_release(mars_model_ext_t *m) {
    if (m->obb_dev) mhip_free(m->obb_dev);
    m->obb_dev = NULL;
    m->obb_bytes = 0;
    m->obb_frames = m->obb_lut_n = 0;
    for (int i = 0; i < 2; i++) {
        if (m->ev_obb[i]) mhip_event_destroy(m->ev_obb[i]);
        m->ev_obb[i] = NULL;
    }
}

/* an int8 activation tensor of exactly 1 channel on a want_h x want_w grid whose bytes the plan keeps: where they are, and that every byte
 * the kernel may touch lies inside the frame's stride */
static mars_error_t angle_tensor(const mars_model_ext_t *m, int T, int want_h, int want_w, int *buf, const int8_t **base, size_t *stride, int *pix_step) {
    if (T < 0 || (uint32_t)T >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
    const mars_tensor_t *d = &m->pub.tensors[T].desc;
    int c, h, w, off, ch_step;
    if (d->dtype != MARS_DTYPE_INT8 || m->mt[T].is_weight || mars_tensor_chw(d, &c, &h, &w)) return MARS_ERR_INVALID_TENSOR;
    if (c != 1 || h != want_h || w != want_w) return MARS_ERR_INVALID_TENSOR;
    if (mars_locate_i8(m, T, c, h, w, 0, buf, &off, pix_step, &ch_step)) return MARS_ERR_INVALID_TENSOR;
    const mtensor_t *tb = &m->mt[*buf];
    if (!tb->dev || *pix_step <= 0) return MARS_ERR_INVALID_TENSOR;
    const size_t last = (size_t)off + ((size_t)h * w - 1) * (size_t)*pix_step;
    if (last >= tb->stride) return MARS_ERR_INVALID_TENSOR;
    *base = (const int8_t *)tb->dev + off;
    *stride = tb->stride;
    return MARS_OK;
}

static int scale_ok(float s) { return s > 0 && isfinite(s); }

/* ang, cs, sn of every byte under scale s: the sigmoid is the DFL class confidence's expression (mars_yolo.c) */
static void angle_table(float s, float *tab) {
    for (int q = -128; q < 128; q++) {
        const float sg = 1.0f / (1.0f + expf((-(float)q) * s));
        const float ang = (sg - 0.25f) * 3.14159265f;
        tab[q + 128] = ang;
        tab[256 + q + 128] = cosf(ang);
        tab[512 + q + 128] = sinf(ang);
    }
}

static float e_of(float T) { return (float)(1.0 - (1.0 - (double)T) * (1.0 - (double)T)); }

static int obb_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    const obb_call_t *c = (const obb_call_t *)cfg;
    mhip_obb_t p = c->obb;
    for (int k = 0; k < c->dfl.n; k++) {
        const mtensor_t *tb = &m->mt[c->dfl.box_buf[k]], *tc = &m->mt[c->dfl.cls_buf[k]];
        if (!tb->dev || !tc->dev) return -1;
        p.box[k] = (const int8_t *)tb->dev + c->dfl.box_off[k];
        p.cls[k] = (const int8_t *)tc->dev + c->dfl.cls_off[k];
        p.box_frame_stride[k] = tb->stride; p.cls_frame_stride[k] = tc->stride;
    }
    p.tab = m->dfl_lut_dev;
    p.dets = dets_dev;
    p.counts = counts_dev;
    p.raw_counts = counts_dev + m->batch;
    int rc = mhip_event_record(c->ev[0]);
    if (!rc) rc = mhip_obb(&p);
    if (!rc) rc = mhip_event_record(c->ev[1]);
    return rc;
}

mars_error_t mars_hip_detect_obb_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_obb_opts_t *s) {
    if (!model || !s) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe) return MARS_ERR_INVALID_TENSOR; /* a pipe's slots own their buffers */
    if ((s->flags & ~MARS_OBB_AGNOSTIC) || m->batch > 65535) return MARS_ERR_INVALID_TENSOR;
    obb_call_t c;
    memset(&c, 0, sizeof(c));
    mhip_obb_t *p = &c.obb;
    mars_error_t e = mars_dfl_resolve(m, heads, &c.dfl);
    if (e != MARS_OK) return e;
    int bufs[4];
    float scales[4] = {0, 0, 0, 0};
    for (int k = 0; k < c.dfl.n; k++) {
        e = angle_tensor(m, s->angle_tensors[k], c.dfl.h[k], c.dfl.w[k], &bufs[k], &p->ang[k], &p->ang_frame_stride[k], &p->ang_pix_step[k]);
        if (e != MARS_OK) return e;
        scales[k] = s->angle_scales[k] != 0 ? s->angle_scales[k] : model->tensors[s->angle_tensors[k]].desc.scale;
        if (!scale_ok(scales[k])) return MARS_ERR_INVALID_TENSOR;
        p->h[k] = c.dfl.h[k]; p->w[k] = c.dfl.w[k]; p->nc[k] = c.dfl.nc[k];
        p->box_pix_step[k] = c.dfl.box_pix_step[k]; p->box_ch_step[k] = c.dfl.box_ch_step[k];
        p->cls_pix_step[k] = c.dfl.cls_pix_step[k]; p->cls_ch_step[k] = c.dfl.cls_ch_step[k];
        p->stride[k] = c.dfl.stride[k];
    }
    p->reg_max = c.dfl.reg_max;
    p->nheads = c.dfl.n;
    p->frames = m->batch;
    p->conf = c.dfl.conf;
    p->e_thresh = e_of(c.dfl.nms);
    p->agnostic = (s->flags & MARS_OBB_AGNOSTIC) != 0;
    p->map = c.dfl.map; p->px = c.dfl.px; p->py = c.dfl.py; p->rx = c.dfl.rx; p->ry = c.dfl.ry;
    e = mars_own_det_buffers(m);
    if (e == MARS_OK) e = mars_dfl_prepare(m, &c.dfl);
    if (e != MARS_OK) return e;
    /* the block: angle tables (at its start: their place does not move with the batch), the kept counts, candidate records, their (cos, sin)
     * pairs, kept records, the kept records' (cos, sin) pairs */
    const size_t B = (size_t)m->batch, rec_b = ALIGN_UP(B * MARS_YOLO_MAX_DET * sizeof(mars_obb_t), 256);
    const size_t cnt_off = OBB_TAB, cand_off = cnt_off + ALIGN_UP(2 * B * sizeof(int), 256), csn_off = cand_off + rec_b;
    const size_t csn_b = ALIGN_UP(B * MARS_YOLO_MAX_DET * 2 * sizeof(float), 256);
    const size_t out_off = csn_off + csn_b, kcsn_off = out_off + rec_b, total = kcsn_off + csn_b; /* ... and the kept boxes' (cos, sin) pairs */
    if (!m->obb_dev || m->obb_bytes < total) {
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: an earlier tail may still use the old block */
        if (m->obb_dev) mhip_free(m->obb_dev);
        m->obb_frames = 0; m->obb_bytes = 0; m->obb_lut_n = 0;
        m->obb_dev = mhip_malloc(total);
        if (!m->obb_dev) return MARS_ERR_ALLOC_FAILED;
        m->obb_bytes = total;
    }
    for (int i = 0; i < 2; i++) {
        if (!m->ev_obb[i]) m->ev_obb[i] = mhip_event_create();
        if (!m->ev_obb[i]) return MARS_ERR_ALLOC_FAILED;
        c.ev[i] = m->ev_obb[i];
    }
    uint8_t *blk = (uint8_t *)m->obb_dev;
    /* the tables depend only on the effective scales: built and uploaded once; synchronises when they change (mars_dfl_prepare's way) */
    int stale = m->obb_lut_n != c.dfl.n;
    for (int k = 0; k < c.dfl.n; k++)
        if (memcmp(&m->obb_lut_scale[k], &scales[k], sizeof(float)) != 0) stale = 1;
    if (stale) {
        float tab[4 * 768];
        for (int k = 0; k < c.dfl.n; k++) angle_table(scales[k], tab + k * 768);
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED;
        m->obb_lut_n = 0; /* (until the new tables are up) */
        m->obb_frames = 0;
        if (mhip_h2d_async(blk, tab, (size_t)c.dfl.n * 768 * sizeof(float)) || mhip_sync()) return MARS_ERR_LAYER_FAILED; /* `tab` is on this stack frame */
        memcpy(m->obb_lut_scale, scales, sizeof(scales));
        m->obb_lut_n = c.dfl.n;
    }
    p->atab = (const float *)blk;
    p->out_counts = (int *)(blk + cnt_off);
    p->cand_counts = p->out_counts + B;
    p->cand = blk + cand_off;
    p->csn = (float *)(blk + csn_off);
    p->out = blk + out_off;
    p->csn_out = (float *)(blk + kcsn_off);
    /* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
    for (int k = 0; k < c.dfl.n; k++) m->mt[c.dfl.box_buf[k]].tail_read = m->mt[c.dfl.cls_buf[k]].tail_read = m->mt[bufs[k]].tail_read = 1;
    m->obb_frames = 0;
    e = mars_tail_on_aux(m, obb_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = c.dfl.map;
    m->obb_cnt_off = cnt_off; m->obb_out_off = out_off; m->obb_csn_off = kcsn_off;
    m->obb_frames = m->batch;
    return MARS_OK;
}

mars_error_t mars_hip_obb_results(mars_model_t *model, mars_obb_t *boxes, int *counts) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->obb_dev || m->obb_frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no obb call yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    m->tail_pending = 0;
    const size_t F = (size_t)m->obb_frames;
    if ((boxes && mhip_d2h_async(boxes, (uint8_t *)m->obb_dev + m->obb_out_off, F * MARS_YOLO_MAX_DET * sizeof(mars_obb_t))) ||
        (counts && mhip_d2h_async(counts, (uint8_t *)m->obb_dev + m->obb_cnt_off, F * sizeof(int))) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

mars_error_t mars_hip_detect_obb(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_obb_opts_t *s, mars_det_t *dets, int *counts,
                                 mars_obb_t *boxes) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_obb_device(model, heads, s);
    if (e == MARS_OK) e = mars_hip_detect_results(model, dets, counts);
    return e != MARS_OK ? e : mars_hip_obb_results(model, boxes, NULL);
}

float mars_hip_obb_ms(mars_model_t *model) {
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m || !m->obb_dev || m->obb_frames <= 0 || !m->ev_obb[0] || !m->ev_obb[1]) return -1.0f;
    return mhip_event_elapsed_ms(m->ev_obb[0], m->ev_obb[1]);
}

int mars_yolo_obb_nms(mars_obb_t *boxes, int n, float thresh, unsigned flags) {
    if (n < 0 || n > MARS_YOLO_MAX_DET || (flags & ~MARS_OBB_AGNOSTIC) || !(thresh >= 0) || !isfinite(thresh)) return -1;
    if (n == 0) return 0;
    if (!boxes) return -1;
    for (int i = 0; i < n; i++)
        if (!(boxes[i].conf >= 0) || signbit(boxes[i].conf)) return -1; /* NaN or negative (-0 too): the bit pattern would not order it */
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) return -1;
    const size_t rec_b = ALIGN_UP((size_t)n * sizeof(mars_obb_t), 256), csn_b = ALIGN_UP((size_t)n * 2 * sizeof(float), 256);
    const size_t o_csn = rec_b, o_out = o_csn + csn_b, o_cnt = o_out + rec_b;
    uint8_t *d = (uint8_t *)mhip_malloc(o_cnt + 256);
    if (!d) return -1;
    float csn[2 * MARS_YOLO_MAX_DET];
    for (int i = 0; i < n; i++) {
        csn[2 * i] = cosf(boxes[i].angle);
        csn[2 * i + 1] = sinf(boxes[i].angle);
    }
    mhip_obb_t p;
    memset(&p, 0, sizeof(p));
    p.frames = 1;
    p.e_thresh = e_of(thresh != 0 ? thresh : 0.45f);
    p.agnostic = (flags & MARS_OBB_AGNOSTIC) != 0;
    p.cand = d; p.csn = (float *)(d + o_csn); p.out = d + o_out;
    p.out_counts = (int *)(d + o_cnt); p.cand_counts = p.out_counts + 1;
    int kept = -1;
    int rc = mhip_h2d_async(p.cand, boxes, (size_t)n * sizeof(mars_obb_t));
    if (!rc) rc = mhip_h2d_async(p.csn, csn, (size_t)n * 2 * sizeof(float));
    if (!rc) rc = mhip_h2d_async(p.cand_counts, &n, sizeof(int));
    if (!rc) rc = mhip_obb_nms(&p);
    if (!rc) rc = mhip_d2h_async(&kept, p.out_counts, sizeof(int));
    if (mhip_sync()) rc = -1; /* (`n` and `csn` are on this stack frame) */
    if (!rc && (kept < 0 || kept > n)) rc = -1;
    if (!rc && kept > 0 && (mhip_d2h_async(boxes, p.out, (size_t)kept * sizeof(mars_obb_t)) || mhip_sync())) rc = -1;
    mhip_free(d);
    return rc ? -1 : kept;
}

void mars_yolo_obb_corners(const mars_obb_t *b, float xy[8]) {
    const float cs = cosf(b->angle), sn = sinf(b->angle);
    const float hw = b->w * 0.5f, hh = b->h * 0.5f;
    const float ux = hw * cs, uy = hw * sn, vx = hh * sn, vy = hh * cs;
    xy[0] = (b->x - ux) + vx; xy[1] = (b->y - uy) - vy;
    xy[2] = (b->x + ux) + vx; xy[3] = (b->y + uy) - vy;
    xy[4] = (b->x + ux) - vx; xy[5] = (b->y + uy) + vy;
    xy[6] = (b->x - ux) - vx; xy[7] = (b->y - uy) + vy;
}
