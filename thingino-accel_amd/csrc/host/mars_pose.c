/*
 * mars_pose.c -- host side of the pose keypoints (include/mars_hip.h, "Pose keypoints"): argument checks, where the plan left the keypoint
 * tensors' bytes, the visibility tables, the result block hung on the model, stream ordering, and the launches of csrc/hip/pose.hip behind
 * the DFL tail of csrc/hip/yolo_tail.hip (which records the origin of every kept detection for it).  The reference has no pose head.  There
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
    mhip_pose_t pose;
    void *const *ev; /* the block's two timing events */
} pose_call_t;

/* the visibility of every byte under scale s: the DFL class confidence's expression (mars_yolo.c), the host's expf */
static void vis_table(float s, float *tab) {
    for (int q = -128; q < 128; q++) tab[q + 128] = 1.0f / (1.0f + expf((-(float)q) * s));
}

static int pose_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    const pose_call_t *c = (const pose_call_t *)cfg;
    int rc = mars_dfl_launch(m, &c->dfl, dets_dev, counts_dev);
    if (rc) return rc;
    mhip_pose_t p = c->pose;
    p.dets = dets_dev; /* only the confidences are read: the mapping leaves them alone */
    p.counts = counts_dev;
    rc = mhip_event_record(c->ev[0]);
    if (!rc) rc = mhip_pose(&p);
    if (!rc) rc = mhip_event_record(c->ev[1]);
    return rc;
}

mars_error_t mars_hip_detect_pose_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_pose_opts_t *s) {
    if (!model || !s) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mars_error_t e = mars_stage_guard(m);
    if (e != MARS_OK) return e;
    pose_call_t c;
    memset(&c, 0, sizeof(c));
    mhip_pose_t *p = &c.pose;
    const int K = s->num_kpt, D = s->kpt_dim ? s->kpt_dim : 3;
    if (s->max_per_frame < 0 || s->max_per_frame > MARS_POSE_MAX_PER_FRAME || !isfinite(s->min_conf) || K < 1 || K > MARS_POSE_MAX_KPT ||
        (D != 2 && D != 3) || m->batch > 65535)
        return MARS_ERR_INVALID_TENSOR;
    e = mars_dfl_resolve(m, heads, &c.dfl);
    if (e != MARS_OK) return e;
    int bufs[4];
    float scales[4][2] = {{0}};
    for (int k = 0; k < c.dfl.n; k++) {
        mars_side_tensor_t t;
        e = mars_side_tensor(m, s->kpt_tensors[k], K * D, c.dfl.h[k], c.dfl.w[k], &t);
        if (e != MARS_OK) return e;
        bufs[k] = t.buf;
        p->kpt[k] = t.base; p->kpt_frame_stride[k] = t.stride; p->kpt_pix_step[k] = t.pix_step; p->kpt_ch_step[k] = t.ch_step;
        scales[k][0] = s->kpt_scales[k] != 0 ? s->kpt_scales[k] : model->tensors[s->kpt_tensors[k]].desc.scale;
        if (!mars_scale_ok(scales[k][0])) return MARS_ERR_INVALID_TENSOR;
        p->scale[k] = scales[k][0];
        p->cells[k] = c.dfl.h[k] * c.dfl.w[k];
        p->w[k] = c.dfl.w[k];
        p->stride[k] = c.dfl.stride[k];
    }
    p->nheads = c.dfl.n;
    p->num_kpt = K;
    p->dim = D;
    p->frames = m->batch;
    p->det_cap = MARS_YOLO_MAX_DET;
    p->min_conf = s->min_conf;
    p->max_per_frame = s->max_per_frame ? s->max_per_frame : 32;
    p->map = c.dfl.map; p->px = c.dfl.px; p->py = c.dfl.py; p->rx = c.dfl.rx; p->ry = c.dfl.ry;
    e = mars_own_det_buffers(m);
    if (e == MARS_OK) e = mars_dfl_prepare(m, &c.dfl);
    if (e != MARS_OK) return e;
    /* the block: visibility tables (at its start: their place does not move with the batch), candidate origins, kept origins, records,
     * keypoints */
    const size_t B = (size_t)m->batch;
    const size_t sz[5] = {4 * 256 * sizeof(float), B * MARS_YOLO_MAX_DET * sizeof(int), B * MARS_YOLO_MAX_DET * sizeof(int),
                          B * p->max_per_frame * sizeof(mars_pose_t), B * p->max_per_frame * K * sizeof(mars_kpt_t)};
    size_t off[5];
    int fresh;
    e = mars_block_reserve(&m->pose, mars_block_layout(sz, 5, off), 1, &fresh);
    if (fresh) m->pose_lut.n = 0;
    if (e != MARS_OK) return e;
    c.ev = m->pose.ev;
    uint8_t *blk = (uint8_t *)m->pose.dev;
    /* the tables depend only on the effective scales: built and uploaded once; synchronises when they change (mars_dfl_prepare's way) */
    if (mars_lut_stale(&m->pose_lut, c.dfl.n, scales)) {
        float tab[4 * 256];
        for (int k = 0; k < c.dfl.n; k++) vis_table(scales[k][0], tab + k * 256);
        m->pose.frames = 0;
        e = mars_lut_refresh(&m->pose_lut, blk, c.dfl.n, scales, tab, 256); /* `tab` is on this stack frame */
        if (e != MARS_OK) return e;
    }
    c.dfl.cand_pred = (int *)(blk + off[1]);
    c.dfl.kept_pred = (int *)(blk + off[2]);
    p->pred = c.dfl.kept_pred;
    p->vis = (const float *)blk;
    p->recs = blk + off[3];
    p->kpts = blk + off[4];
    /* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
    for (int k = 0; k < c.dfl.n; k++) m->mt[c.dfl.box_buf[k]].tail_read = m->mt[c.dfl.cls_buf[k]].tail_read = m->mt[bufs[k]].tail_read = 1;
    m->pose.frames = 0;
    e = mars_tail_on_aux(m, pose_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = c.dfl.map;
    m->pose_rec_off = off[3]; m->pose_kpt_off = off[4];
    m->pose.frames = m->batch; m->pose_max = p->max_per_frame; m->pose_k = K;
    return MARS_OK;
}

mars_error_t mars_hip_pose_results(mars_model_t *model, mars_pose_t *recs, mars_kpt_t *kpts, int *num_kpt) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    const size_t slots = (size_t)m->pose.frames * m->pose_max;
    const mars_block_part_t parts[2] = {{recs, m->pose_rec_off, slots * sizeof(mars_pose_t)}, {kpts, m->pose_kpt_off, slots * m->pose_k * sizeof(mars_kpt_t)}};
    const mars_error_t e = mars_block_fetch(&m->pose, parts, 2, &m->tail_pending);
    if (e == MARS_OK && num_kpt) *num_kpt = m->pose_k;
    return e;
}

mars_error_t mars_hip_detect_pose(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_pose_opts_t *s, mars_det_t *dets, int *counts,
                                  mars_pose_t *recs, mars_kpt_t *kpts) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_pose_device(model, heads, s);
    if (e == MARS_OK) e = mars_hip_detect_results(model, dets, counts);
    return e != MARS_OK ? e : mars_hip_pose_results(model, recs, kpts, NULL);
}

float mars_hip_pose_ms(mars_model_t *model) { return model ? mars_block_ms(&((mars_model_ext_t *)model)->pose) : -1.0f; }

int mars_yolo_keypoints(const int8_t *rows, int n, int K, int D, const int *gx, const int *gy, const int *stride, float s, mars_kpt_t *kpts) {
    if (n < 0 || n > MARS_POSE_MAX_PER_FRAME || K < 1 || K > MARS_POSE_MAX_KPT || (D != 2 && D != 3) || !mars_scale_ok(s)) return -1;
    if (n == 0) return 0;
    if (!rows || !gx || !gy || !stride || !kpts) return -1;
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) return -1;
    /* one scratch block: [rows][count][pred][grid][table][recs][kpts] */
    const size_t sz[7] = {(size_t)n * K * D, sizeof(int), (size_t)n * sizeof(int), (size_t)n * 3 * sizeof(int), 256 * sizeof(float),
                          (size_t)n * sizeof(mars_pose_t), (size_t)n * K * sizeof(mars_kpt_t)};
    size_t off[7];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 7, off));
    if (!d) return -1;
    int pred[MARS_POSE_MAX_PER_FRAME], grid[3 * MARS_POSE_MAX_PER_FRAME];
    float tab[256];
    for (int i = 0; i < n; i++) {
        pred[i] = i; /* row i is "cell" i of one head of n cells */
        grid[3 * i] = gx[i]; grid[3 * i + 1] = gy[i]; grid[3 * i + 2] = stride[i];
    }
    vis_table(s, tab);
    mhip_pose_t p;
    memset(&p, 0, sizeof(p));
    p.kpt[0] = (const int8_t *)d; p.kpt_pix_step[0] = K * D; p.kpt_ch_step[0] = 1; p.cells[0] = n; p.w[0] = n; p.stride[0] = 1; p.scale[0] = s;
    p.nheads = 1;
    p.vis = (const float *)(d + off[4]);
    p.num_kpt = K; p.dim = D;
    p.frames = 1;
    p.counts = (const int *)(d + off[1]); p.pred = (const int *)(d + off[2]); p.grid = (const int *)(d + off[3]); p.det_cap = n;
    p.select_all = 1; p.max_per_frame = n;
    p.recs = d + off[5]; p.kpts = d + off[6];
    int rc = mhip_h2d_async(d, rows, sz[0]);
    if (!rc) rc = mhip_h2d_async(d + off[1], &n, sizeof(int));
    if (!rc) rc = mhip_h2d_async(d + off[2], pred, sz[2]);
    if (!rc) rc = mhip_h2d_async(d + off[3], grid, sz[3]);
    if (!rc) rc = mhip_h2d_async(d + off[4], tab, sizeof(tab));
    if (!rc) rc = mhip_pose(&p);
    if (!rc) rc = mhip_d2h_async(kpts, p.kpts, sz[6]);
    if (mhip_sync()) rc = -1; /* (`n`, `pred`, `grid` and `tab` are on this stack frame) */
    mhip_free(d);
    return rc ? -1 : 0;
}
