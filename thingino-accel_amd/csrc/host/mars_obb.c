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
    void *const *ev; /* the block's two timing events */
} obb_call_t;

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
    mars_error_t e = mars_stage_guard(m);
    if (e != MARS_OK) return e;
    if ((s->flags & ~MARS_OBB_AGNOSTIC) || m->batch > 65535) return MARS_ERR_INVALID_TENSOR;
    obb_call_t c;
    memset(&c, 0, sizeof(c));
    mhip_obb_t *p = &c.obb;
    e = mars_dfl_resolve(m, heads, &c.dfl);
    if (e != MARS_OK) return e;
    int bufs[4];
    float scales[4][2] = {{0}};
    for (int k = 0; k < c.dfl.n; k++) {
        mars_side_tensor_t t; /* exactly 1 channel: no channel step is taken */
        e = mars_side_tensor(m, s->angle_tensors[k], 1, c.dfl.h[k], c.dfl.w[k], &t);
        if (e != MARS_OK) return e;
        bufs[k] = t.buf;
        p->ang[k] = t.base; p->ang_frame_stride[k] = t.stride; p->ang_pix_step[k] = t.pix_step;
        scales[k][0] = s->angle_scales[k] != 0 ? s->angle_scales[k] : model->tensors[s->angle_tensors[k]].desc.scale;
        if (!mars_scale_ok(scales[k][0])) return MARS_ERR_INVALID_TENSOR;
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
    /* the block: angle tables (at its start: their place does not move with the batch), the kept and candidate counts, candidate records,
     * their (cos, sin) pairs, kept records, the kept records' (cos, sin) pairs */
    const size_t B = (size_t)m->batch, rec_b = B * MARS_YOLO_MAX_DET * sizeof(mars_obb_t), csn_b = B * MARS_YOLO_MAX_DET * 2 * sizeof(float);
    const size_t sz[6] = {OBB_TAB, 2 * B * sizeof(int), rec_b, csn_b, rec_b, csn_b};
    size_t off[6];
    int fresh;
    e = mars_block_reserve(&m->obb, mars_block_layout(sz, 6, off), 1, &fresh);
    if (fresh) m->obb_lut.n = 0;
    if (e != MARS_OK) return e;
    c.ev = m->obb.ev;
    uint8_t *blk = (uint8_t *)m->obb.dev;
    /* the tables depend only on the effective scales: built and uploaded once; synchronises when they change (mars_dfl_prepare's way) */
    if (mars_lut_stale(&m->obb_lut, c.dfl.n, scales)) {
        float tab[4 * 768];
        for (int k = 0; k < c.dfl.n; k++) angle_table(scales[k][0], tab + k * 768);
        m->obb.frames = 0;
        e = mars_lut_refresh(&m->obb_lut, blk, c.dfl.n, scales, tab, 768); /* `tab` is on this stack frame */
        if (e != MARS_OK) return e;
    }
    p->atab = (const float *)blk;
    p->out_counts = (int *)(blk + off[1]);
    p->cand_counts = p->out_counts + B;
    p->cand = blk + off[2];
    p->csn = (float *)(blk + off[3]);
    p->out = blk + off[4];
    p->csn_out = (float *)(blk + off[5]);
    /* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
    for (int k = 0; k < c.dfl.n; k++) m->mt[c.dfl.box_buf[k]].tail_read = m->mt[c.dfl.cls_buf[k]].tail_read = m->mt[bufs[k]].tail_read = 1;
    m->obb.frames = 0;
    e = mars_tail_on_aux(m, obb_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = c.dfl.map;
    m->obb_cnt_off = off[1]; m->obb_out_off = off[4]; m->obb_csn_off = off[5];
    m->obb.frames = m->batch;
    return MARS_OK;
}

mars_error_t mars_hip_obb_results(mars_model_t *model, mars_obb_t *boxes, int *counts) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    const size_t F = (size_t)m->obb.frames;
    const mars_block_part_t parts[2] = {{boxes, m->obb_out_off, F * MARS_YOLO_MAX_DET * sizeof(mars_obb_t)}, {counts, m->obb_cnt_off, F * sizeof(int)}};
    return mars_block_fetch(&m->obb, parts, 2, &m->tail_pending);
}

mars_error_t mars_hip_detect_obb(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_obb_opts_t *s, mars_det_t *dets, int *counts,
                                 mars_obb_t *boxes) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_obb_device(model, heads, s);
    if (e == MARS_OK) e = mars_hip_detect_results(model, dets, counts);
    return e != MARS_OK ? e : mars_hip_obb_results(model, boxes, NULL);
}

float mars_hip_obb_ms(mars_model_t *model) { return model ? mars_block_ms(&((mars_model_ext_t *)model)->obb) : -1.0f; }

int mars_yolo_obb_nms(mars_obb_t *boxes, int n, float thresh, unsigned flags) {
    if (n < 0 || n > MARS_YOLO_MAX_DET || (flags & ~MARS_OBB_AGNOSTIC) || !(thresh >= 0) || !isfinite(thresh)) return -1;
    if (n == 0) return 0;
    if (!boxes) return -1;
    for (int i = 0; i < n; i++)
        if (!(boxes[i].conf >= 0) || signbit(boxes[i].conf)) return -1; /* NaN or negative (-0 too): the bit pattern would not order it */
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) return -1;
    /* one scratch block: [candidates][their (cos, sin) pairs][kept][kept count, candidate count] */
    const size_t sz[4] = {(size_t)n * sizeof(mars_obb_t), (size_t)n * 2 * sizeof(float), (size_t)n * sizeof(mars_obb_t), 2 * sizeof(int)};
    size_t off[4];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 4, off));
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
    p.cand = d; p.csn = (float *)(d + off[1]); p.out = d + off[2];
    p.out_counts = (int *)(d + off[3]); p.cand_counts = p.out_counts + 1;
    int kept = -1;
    int rc = mhip_h2d_async(p.cand, boxes, sz[0]);
    if (!rc) rc = mhip_h2d_async(p.csn, csn, sz[1]);
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
