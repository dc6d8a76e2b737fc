/*
 * mars_classify.c -- host side of the second-stage labels (include/mars_hip.h, "Second-stage labels"): argument checks, where the plan left
 * the feature tensor's bytes, the result block hung on the classifier, the label array hung on the detector, stream ordering, and the
 * launches of csrc/hip/classify.hip.  The reference's graph fails on GLOBAL_AVGPOOL and FC (src/mars/mars_runtime.c) and so does this
 * one: the classifier head is a tail call outside the graph, like the Detect heads.  There is no CPU path: without the device every entry
 * point fails.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

/* the checks that need no device and no model, and the defaults resolved: *top_k, *softmax; the scale stays as given (0 = the tensor's) */
static mars_error_t cls_opts(const mars_hip_cls_opts_t *o, int *top_k, int *softmax) {
    if (!o || o->top_k < 0 || o->top_k > MARS_CLS_MAX_TOPK || (o->flags & ~MARS_CLS_SOFTMAX)) return MARS_ERR_INVALID_FILE;
    if (!isfinite(o->scale) || o->scale < 0) return MARS_ERR_INVALID_FILE;
    *top_k = o->top_k ? o->top_k : 1;
    *softmax = (o->flags & MARS_CLS_SOFTMAX) != 0;
    return MARS_OK;
}

static size_t cls_block(const mhip_classify_t *p, size_t *sums_off, size_t *top_off) {
    *sums_off = ALIGN_UP((size_t)p->frames * p->nsplit * p->c * sizeof(int), 256);
    *top_off = *sums_off + ALIGN_UP((size_t)p->frames * p->c * sizeof(int), 256);
    return *top_off + ALIGN_UP((size_t)p->frames * p->top_k * sizeof(mars_cls_t), 256);
}

mars_error_t mars_yolo_classify_maps(const signed char *maps, int n, int c, int h, int w, int nhwc, float scale, const mars_hip_cls_opts_t *opts,
                                     mars_cls_t *top, int *sums) {
    mhip_classify_t p;
    memset(&p, 0, sizeof(p));
    const mars_error_t e = cls_opts(opts, &p.top_k, &p.softmax);
    if (e != MARS_OK) return e;
    if (!maps || !top || n <= 0 || c <= 0 || h <= 0 || w <= 0) return MARS_ERR_INVALID_FILE;
    if (c > MHIP_CLS_MAX_C || (long long)h * w > (1LL << 24) || n > 65535) return MARS_ERR_INVALID_TENSOR;
    p.scale = opts->scale != 0 ? opts->scale : scale;
    if (!(p.scale > 0) || !isfinite(p.scale)) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    p.frames = n; p.c = c; p.hw = h * w;
    p.frame_stride = (size_t)c * p.hw;
    if (nhwc) { p.pix_step = c; p.ch_step = 1; p.row_room = c; }
    else { p.pix_step = 1; p.ch_step = p.hw; p.row_room = p.hw == 1 ? c : 0; }
    const size_t in_b = p.frame_stride * (size_t)n;
    int8_t *d_in = (int8_t *)mhip_malloc(in_b);
    if (!d_in) return MARS_ERR_ALLOC_FAILED;
    p.base = d_in;
    p.nsplit = mhip_classify_split(&p);
    size_t so, to;
    const size_t total = cls_block(&p, &so, &to);
    uint8_t *d = p.nsplit > 0 ? (uint8_t *)mhip_malloc(total) : NULL;
    if (!d) {
        mhip_free(d_in);
        return p.nsplit > 0 ? MARS_ERR_ALLOC_FAILED : MARS_ERR_INVALID_TENSOR;
    }
    p.partial = (int *)d; p.sums = (int *)(d + so); p.top = d + to;
    int rc = mhip_h2d_async(d_in, maps, in_b);
    if (!rc) rc = mhip_classify(&p);
    if (!rc) rc = mhip_d2h_async(top, p.top, (size_t)n * p.top_k * sizeof(mars_cls_t));
    if (!rc && sums) rc = mhip_d2h_async(sums, p.sums, (size_t)n * c * sizeof(int));
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    mhip_free(d_in);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

void mars_cls_release(mars_model_ext_t *m) {
    if (m->cls_dev) mhip_free(m->cls_dev);
    if (m->label_dev) mhip_free(m->label_dev);
    m->cls_dev = m->label_dev = NULL;
    m->cls_bytes = 0;
    m->cls_frames = m->cls_c = m->cls_top_k = m->label_cap = m->label_frames = m->label_pending = 0;
    mars_match_release(m);
}

static int cls_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    (void)m; (void)dets_dev; (void)counts_dev;
    return mhip_classify((const mhip_classify_t *)cfg);
}

mars_error_t mars_hip_classify_device(mars_model_t *model, const mars_hip_cls_opts_t *opts) {
    mhip_classify_t p;
    memset(&p, 0, sizeof(p));
    if (!model) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = cls_opts(opts, &p.top_k, &p.softmax);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe) return MARS_ERR_INVALID_TENSOR; /* a pipe's slots own their buffers */
    int T;
    if (opts->tensor > 0) T = opts->tensor;
    else if (opts->output_index < 0 || (uint32_t)opts->output_index >= model->header.num_outputs) return MARS_ERR_INVALID_TENSOR;
    else T = (int)model->header.output_tensor_ids[opts->output_index];
    if (T < 0 || (uint32_t)T >= model->header.num_tensors) return MARS_ERR_INVALID_TENSOR;
    const mars_tensor_t *d = &model->tensors[T].desc;
    int c, h, w, buf, off;
    /* a graph input is refused too: uploads and crops overwrite it on the main stream without looking at a tail's event */
    if (d->dtype != MARS_DTYPE_INT8 || m->mt[T].is_weight || m->mt[T].io_in || mars_tensor_chw(d, &c, &h, &w)) return MARS_ERR_INVALID_TENSOR;
    if (c > MHIP_CLS_MAX_C || (long long)h * w > (1LL << 24) || m->batch > 65535) return MARS_ERR_INVALID_TENSOR;
    if (mars_locate_i8(m, T, c, h, w, 1, &buf, &off, &p.pix_step, &p.ch_step)) return MARS_ERR_INVALID_TENSOR;
    p.scale = opts->scale != 0 ? opts->scale : d->scale;
    if (!(p.scale > 0) || !isfinite(p.scale)) return MARS_ERR_INVALID_TENSOR;
    const mtensor_t *tb = &m->mt[buf];
    p.frames = m->batch; p.c = c; p.hw = h * w;
    p.base = (const int8_t *)tb->dev + off;
    p.frame_stride = tb->stride;
    if (!tb->dev) return MARS_ERR_INVALID_TENSOR;
    /* every byte the kernels touch lies inside the frame's stride.  Pixel rows: a load may run past channel c - 1 up to the end of the
     * row (pad channels, a concat's other slice), where the last pixel's row is inside the stride as well */
    if (p.ch_step != 1) {
        if ((size_t)c * p.hw > tb->stride) return MARS_ERR_INVALID_TENSOR;
    } else {
        const size_t last = (size_t)(p.hw - 1) * p.pix_step + off;
        p.row_room = p.hw == 1 && p.pix_step < c ? c : p.pix_step - off; /* ([C][1][1] planes are one pixel's row) */
        if (p.row_room < c || last + c > tb->stride) return MARS_ERR_INVALID_TENSOR;
        if (last + p.row_room > tb->stride) p.row_room = c;
    }
    p.nsplit = mhip_classify_split(&p);
    if (p.nsplit <= 0) return MARS_ERR_INVALID_TENSOR;
    size_t so, to;
    const size_t total = cls_block(&p, &so, &to);
    if (!m->cls_dev || m->cls_bytes < total) {
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: an earlier tail or scatter may still use the old block */
        if (m->cls_dev) mhip_free(m->cls_dev);
        m->cls_frames = 0; m->cls_bytes = 0;
        m->cls_dev = mhip_malloc(total);
        if (!m->cls_dev) return MARS_ERR_ALLOC_FAILED;
        m->cls_bytes = total;
    }
    p.partial = (int *)m->cls_dev;
    p.sums = (int *)((uint8_t *)m->cls_dev + so);
    p.top = (uint8_t *)m->cls_dev + to;
    /* behind the graph's event on the auxiliary stream; the next run's layers that write the tensor's buffer wait for it (tail_read), the
     * rest of that run overlaps it.  An earlier label scatter reads the block from the same stream: it is in front */
    m->mt[buf].tail_read = 1;
    m->cls_frames = 0;
    const mars_error_t e2 = mars_tail_on_aux(m, cls_launch_cb, &p);
    if (e2 != MARS_OK) return e2;
    m->cls_sums_off = so; m->cls_top_off = to;
    m->cls_frames = p.frames; m->cls_c = c; m->cls_top_k = p.top_k;
    return MARS_OK;
}

mars_error_t mars_hip_classify_results(mars_model_t *model, mars_cls_t *top, int *sums, int *channels) {
    if (!model || !top) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->cls_dev || m->cls_frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no classify call yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    m->tail_pending = 0;
    if (mhip_d2h_async(top, (uint8_t *)m->cls_dev + m->cls_top_off, (size_t)m->cls_frames * m->cls_top_k * sizeof(mars_cls_t)) ||
        (sums && mhip_d2h_async(sums, (uint8_t *)m->cls_dev + m->cls_sums_off, (size_t)m->cls_frames * m->cls_c * sizeof(int))) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    if (channels) *channels = m->cls_c;
    return MARS_OK;
}

mars_error_t mars_hip_classify(mars_model_t *model, const mars_hip_cls_opts_t *opts, mars_cls_t *top, int *sums) {
    if (!model || !opts || !top) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_classify_device(model, opts);
    return e != MARS_OK ? e : mars_hip_classify_results(model, top, sums, NULL);
}

mars_error_t mars_hip_label_detections_device(mars_model_t *det_model, mars_model_t *cls_model) {
    if (!det_model || !cls_model) return MARS_ERR_INVALID_FILE;
    if (det_model == cls_model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model, *m = (mars_model_ext_t *)cls_model;
    if (!m->act_dev || !det->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe || det->pipe) return MARS_ERR_INVALID_TENSOR;
    if (!m->roi_dev || m->roi_slots <= 0 || m->roi_from != det) return MARS_ERR_INVALID_TENSOR;            /* no crop call out of det_model */
    if (!m->cls_dev || m->cls_frames <= 0 || m->cls_frames < m->roi_slots) return MARS_ERR_INVALID_TENSOR; /* no classify results */
    if (!det->det_dev || !det->det_counts_dev || det->det_cap < det->batch) return MARS_ERR_INVALID_TENSOR; /* no detections in HBM */
    if (!det->label_dev || det->label_cap < det->batch) {
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: nothing may be in flight (own_det_buffers) */
        if (det->label_dev) mhip_free(det->label_dev);
        det->label_cap = det->label_frames = 0;
        det->label_dev = mhip_malloc((size_t)det->batch * MARS_YOLO_MAX_DET * sizeof(mars_cls_t));
        if (!det->label_dev) return MARS_ERR_ALLOC_FAILED;
        det->label_cap = det->batch;
    }
    if (!m->ev_graph_done) m->ev_graph_done = mhip_event_create_sync();
    if (!m->ev_label_done) m->ev_label_done = mhip_event_create_sync();
    if (!m->ev_graph_done || !m->ev_label_done) return MARS_ERR_ALLOC_FAILED;
    /* The auxiliary stream.  It carries every detection tail and every classify tail, so the scatter comes behind both models' tails and
     * ahead of det_model's next detect call and cls_model's next classify call.  The ROI table is written on the main stream: the scatter
     * waits for what that stream has been given so far, and the next crop call into cls_model waits for the scatter (ev_label_done) */
    mhip_select_stream(0);
    if (mhip_event_record(m->ev_graph_done)) return MARS_ERR_LAYER_FAILED;
    mhip_select_aux(1);
    int rc = mhip_stream_wait(1, m->ev_graph_done);
    if (!rc)
        rc = mhip_label_scatter((uint8_t *)m->roi_dev + 16, (const int *)m->roi_dev, m->roi_slots, (uint8_t *)m->cls_dev + m->cls_top_off, m->cls_top_k,
                                det->label_dev, det->batch, MARS_YOLO_MAX_DET);
    if (!rc) rc = mhip_event_record(m->ev_label_done);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->label_pending = 1;
    det->label_frames = det->batch;
    return MARS_OK;
}

mars_error_t mars_hip_label_results(mars_model_t *det_model, mars_cls_t *labels) {
    if (!det_model || !labels) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model;
    if (!det->label_dev || det->label_frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no scatter yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    if (mhip_d2h_async(labels, det->label_dev, (size_t)det->label_frames * MARS_YOLO_MAX_DET * sizeof(mars_cls_t)) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}
