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
    void *ev[2];
} pose_call_t;

void mars_pose_release(mars_model_ext_t *m) {
    if (m->pose_dev) mhip_free(m->pose_dev);
    m->pose_dev = NULL;
    m->pose_bytes = 0;
    m->pose_frames = m->pose_max = m->pose_k = m->pose_lut_n = 0;
    for (int i = 0; i < 2; i++) {
        if (m->ev_pose[i]) mhip_event_destroy(m->ev_pose[i]);
        m->ev_pose[i] = NULL;
    }
}

/* an int8 activation tensor of `want_c` channels on a want_h x want_w grid whose bytes the plan keeps: where they are, and that every byte
 * the kernel may touch lies inside the frame's stride */
static mars_error_t kpt_tensor(const mars_model_ext_t *m, int T, int want_c, int want_h, int want_w, int *buf, const int8_t **base, size_t *stride,
                               int *pix_step, int *ch_step) {
    if (T < 0 || (uint32_t)T >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
    const mars_tensor_t *d = &m->pub.tensors[T].desc;
    int c, h, w, off;
    if (d->dtype != MARS_DTYPE_INT8 || m->mt[T].is_weight || mars_tensor_chw(d, &c, &h, &w)) return MARS_ERR_INVALID_TENSOR;
    if (c != want_c || h != want_h || w != want_w) return MARS_ERR_INVALID_TENSOR;
    if (mars_locate_i8(m, T, c, h, w, 0, buf, &off, pix_step, ch_step)) return MARS_ERR_INVALID_TENSOR;
    const mtensor_t *tb = &m->mt[*buf];
    if (!tb->dev || *pix_step <= 0 || *ch_step <= 0) return MARS_ERR_INVALID_TENSOR;
    const size_t last = (size_t)off + ((size_t)h * w - 1) * (size_t)*pix_step + (size_t)(c - 1) * (size_t)*ch_step;
    if (last >= tb->stride) return MARS_ERR_INVALID_TENSOR;
    *base = (const int8_t *)tb->dev + off;
    *stride = tb->stride;
    return MARS_OK;
}

static int scale_ok(float s) { return s > 0 && isfinite(s); }

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
    if (!m->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe) return MARS_ERR_INVALID_TENSOR; /* a pipe's slots own their buffers */
    pose_call_t c;
    memset(&c, 0, sizeof(c));
    mhip_pose_t *p = &c.pose;
    const int K = s->num_kpt, D = s->kpt_dim ? s->kpt_dim : 3;
    if (s->max_per_frame < 0 || s->max_per_frame > MARS_POSE_MAX_PER_FRAME || !isfinite(s->min_conf) || K < 1 || K > MARS_POSE_MAX_KPT ||
        (D != 2 && D != 3) || m->batch > 65535)
        return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_dfl_resolve(m, heads, &c.dfl);
    if (e != MARS_OK) return e;
    int bufs[4];
    float scales[4] = {0, 0, 0, 0};
    for (int k = 0; k < c.dfl.n; k++) {
        e = kpt_tensor(m, s->kpt_tensors[k], K * D, c.dfl.h[k], c.dfl.w[k], &bufs[k], &p->kpt[k], &p->kpt_frame_stride[k], &p->kpt_pix_step[k],
                       &p->kpt_ch_step[k]);
        if (e != MARS_OK) return e;
        scales[k] = s->kpt_scales[k] != 0 ? s->kpt_scales[k] : model->tensors[s->kpt_tensors[k]].desc.scale;
        if (!scale_ok(scales[k])) return MARS_ERR_INVALID_TENSOR;
        p->scale[k] = scales[k];
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
    const size_t tab_off = 0, cand_off = 4 * 256 * sizeof(float), kept_off = cand_off + ALIGN_UP(B * MARS_YOLO_MAX_DET * sizeof(int), 256);
    const size_t rec_off = kept_off + ALIGN_UP(B * MARS_YOLO_MAX_DET * sizeof(int), 256);
    const size_t kpt_off = rec_off + ALIGN_UP(B * p->max_per_frame * sizeof(mars_pose_t), 256);
    const size_t total = kpt_off + ALIGN_UP(B * p->max_per_frame * K * sizeof(mars_kpt_t), 256);
    if (!m->pose_dev || m->pose_bytes < total) {
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: an earlier tail may still use the old block */
        if (m->pose_dev) mhip_free(m->pose_dev);
        m->pose_frames = 0; m->pose_bytes = 0; m->pose_lut_n = 0;
        m->pose_dev = mhip_malloc(total);
        if (!m->pose_dev) return MARS_ERR_ALLOC_FAILED;
        m->pose_bytes = total;
    }
    for (int i = 0; i < 2; i++) {
        if (!m->ev_pose[i]) m->ev_pose[i] = mhip_event_create();
        if (!m->ev_pose[i]) return MARS_ERR_ALLOC_FAILED;
        c.ev[i] = m->ev_pose[i];
    }
    uint8_t *blk = (uint8_t *)m->pose_dev;
    /* the tables depend only on the effective scales: built and uploaded once; synchronises when they change (mars_dfl_prepare's way) */
    int stale = m->pose_lut_n != c.dfl.n;
    for (int k = 0; k < c.dfl.n; k++)
        if (memcmp(&m->pose_lut_scale[k], &scales[k], sizeof(float)) != 0) stale = 1;
    if (stale) {
        float tab[4 * 256];
        for (int k = 0; k < c.dfl.n; k++) vis_table(scales[k], tab + k * 256);
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED;
        m->pose_lut_n = 0; /* (until the new tables are up) */
        m->pose_frames = 0;
        if (mhip_h2d_async(blk + tab_off, tab, (size_t)c.dfl.n * 256 * sizeof(float)) || mhip_sync())
            return MARS_ERR_LAYER_FAILED; /* `tab` is on this stack frame */
        memcpy(m->pose_lut_scale, scales, sizeof(scales));
        m->pose_lut_n = c.dfl.n;
    }
    c.dfl.cand_pred = (int *)(blk + cand_off);
    c.dfl.kept_pred = (int *)(blk + kept_off);
    p->pred = c.dfl.kept_pred;
    p->vis = (const float *)(blk + tab_off);
    p->recs = blk + rec_off;
    p->kpts = blk + kpt_off;
    /* behind the graph's event on the auxiliary stream; the next run's layers that write one of these buffers wait for it (tail_read) */
    for (int k = 0; k < c.dfl.n; k++) m->mt[c.dfl.box_buf[k]].tail_read = m->mt[c.dfl.cls_buf[k]].tail_read = m->mt[bufs[k]].tail_read = 1;
    m->pose_frames = 0;
    e = mars_tail_on_aux(m, pose_launch_cb, &c);
    if (e != MARS_OK) return e;
    m->det_mapped = c.dfl.map;
    m->pose_rec_off = rec_off; m->pose_kpt_off = kpt_off;
    m->pose_frames = m->batch; m->pose_max = p->max_per_frame; m->pose_k = K;
    return MARS_OK;
}

mars_error_t mars_hip_pose_results(mars_model_t *model, mars_pose_t *recs, mars_kpt_t *kpts, int *num_kpt) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->pose_dev || m->pose_frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no pose call yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    m->tail_pending = 0;
    const size_t slots = (size_t)m->pose_frames * m->pose_max;
    if ((recs && mhip_d2h_async(recs, (uint8_t *)m->pose_dev + m->pose_rec_off, slots * sizeof(mars_pose_t))) ||
        (kpts && mhip_d2h_async(kpts, (uint8_t *)m->pose_dev + m->pose_kpt_off, slots * m->pose_k * sizeof(mars_kpt_t))) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    if (num_kpt) *num_kpt = m->pose_k;
    return MARS_OK;
}

mars_error_t mars_hip_detect_pose(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, const mars_hip_pose_opts_t *s, mars_det_t *dets, int *counts,
                                  mars_pose_t *recs, mars_kpt_t *kpts) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_pose_device(model, heads, s);
    if (e == MARS_OK) e = mars_hip_detect_results(model, dets, counts);
    return e != MARS_OK ? e : mars_hip_pose_results(model, recs, kpts, NULL);
}

float mars_hip_pose_ms(mars_model_t *model) {
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m || !m->pose_dev || m->pose_frames <= 0 || !m->ev_pose[0] || !m->ev_pose[1]) return -1.0f;
    return mhip_event_elapsed_ms(m->ev_pose[0], m->ev_pose[1]);
}

int mars_yolo_keypoints(const int8_t *rows, int n, int K, int D, const int *gx, const int *gy, const int *stride, float s, mars_kpt_t *kpts) {
    if (n < 0 || n > MARS_POSE_MAX_PER_FRAME || K < 1 || K > MARS_POSE_MAX_KPT || (D != 2 && D != 3) || !scale_ok(s)) return -1;
    if (n == 0) return 0;
    if (!rows || !gx || !gy || !stride || !kpts) return -1;
    if (!nna_is_ready() && nna_init() != NNA_SUCCESS) return -1;
    const size_t row_b = (size_t)n * K * D, idx_b = (size_t)n * sizeof(int), grid_b = 3 * idx_b, kpt_b = (size_t)n * K * sizeof(mars_kpt_t);
    const size_t o_cnt = ALIGN_UP(row_b, 256), o_pred = o_cnt + 256, o_grid = o_pred + ALIGN_UP(idx_b, 256), o_tab = o_grid + ALIGN_UP(grid_b, 256);
    const size_t o_rec = o_tab + 256 * sizeof(float), o_kpt = o_rec + ALIGN_UP((size_t)n * sizeof(mars_pose_t), 256);
    uint8_t *d = (uint8_t *)mhip_malloc(o_kpt + kpt_b);
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
    p.vis = (const float *)(d + o_tab);
    p.num_kpt = K; p.dim = D;
    p.frames = 1;
    p.counts = (const int *)(d + o_cnt); p.pred = (const int *)(d + o_pred); p.grid = (const int *)(d + o_grid); p.det_cap = n;
    p.select_all = 1; p.max_per_frame = n;
    p.recs = d + o_rec; p.kpts = d + o_kpt;
    int rc = mhip_h2d_async(d, rows, row_b);
    if (!rc) rc = mhip_h2d_async(d + o_cnt, &n, sizeof(int));
    if (!rc) rc = mhip_h2d_async(d + o_pred, pred, idx_b);
    if (!rc) rc = mhip_h2d_async(d + o_grid, grid, grid_b);
    if (!rc) rc = mhip_h2d_async(d + o_tab, tab, sizeof(tab));
    if (!rc) rc = mhip_pose(&p);
    if (!rc) rc = mhip_d2h_async(kpts, p.kpts, kpt_b);
    if (mhip_sync()) rc = -1; /* (`n`, `pred`, `grid` and `tab` are on this stack frame) */
    mhip_free(d);
    return rc ? -1 : 0;
}
