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

/* the block of a classify call: [frames][nsplit][C] partial sums, [frames][C] sums, [frames][top_k] entries -> bytes */
static size_t cls_block(const mhip_classify_t *p, size_t off[3]) {
    const size_t sz[3] = {(size_t)p->frames * p->nsplit * p->c * sizeof(int), (size_t)p->frames * p->c * sizeof(int), (size_t)p->frames * p->top_k * sizeof(mars_cls_t)};
    return mars_block_layout(sz, 3, off);
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
    if (!mars_scale_ok(p.scale)) return MARS_ERR_INVALID_TENSOR;
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
    size_t off[3];
    const size_t total = cls_block(&p, off);
    uint8_t *d = p.nsplit > 0 ? (uint8_t *)mhip_malloc(total) : NULL;
    if (!d) {
        mhip_free(d_in);
        return p.nsplit > 0 ? MARS_ERR_ALLOC_FAILED : MARS_ERR_INVALID_TENSOR;
    }
    p.partial = (int *)d; p.sums = (int *)(d + off[1]); p.top = d + off[2];
    int rc = mhip_h2d_async(d_in, maps, in_b);
    if (!rc) rc = mhip_classify(&p);
    if (!rc) rc = mhip_d2h_async(top, p.top, (size_t)n * p.top_k * sizeof(mars_cls_t));
    if (!rc && sums) rc = mhip_d2h_async(sums, p.sums, (size_t)n * c * sizeof(int));
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    mhip_free(d_in);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

static int cls_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    (void)m; (void)dets_dev; (void)counts_dev;
    return mhip_classify((const mhip_classify_t *)cfg);
}

mars_error_t mars_hip_classify_device(mars_model_t *model, const mars_hip_cls_opts_t *opts) {
    mhip_classify_t p;
    memset(&p, 0, sizeof(p));
    if (!model) return MARS_ERR_INVALID_FILE;
    mars_error_t e = cls_opts(opts, &p.top_k, &p.softmax);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if ((e = mars_stage_guard(m)) != MARS_OK) return e;
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
    if (!mars_scale_ok(p.scale)) return MARS_ERR_INVALID_TENSOR;
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
    size_t boff[3];
    if ((e = mars_block_reserve(&m->cls, cls_block(&p, boff), 0, NULL)) != MARS_OK) return e;
    p.partial = (int *)m->cls.dev;
    p.sums = (int *)((uint8_t *)m->cls.dev + boff[1]);
    p.top = (uint8_t *)m->cls.dev + boff[2];
    /* behind the graph's event on the auxiliary stream; the next run's layers that write the tensor's buffer wait for it (tail_read), the
     * rest of that run overlaps it.  An earlier label scatter reads the block from the same stream: it is in front */
    m->mt[buf].tail_read = 1;
    m->cls.frames = 0;
    if ((e = mars_tail_on_aux(m, cls_launch_cb, &p)) != MARS_OK) return e;
    m->cls_sums_off = boff[1]; m->cls_top_off = boff[2];
    m->cls.frames = p.frames; m->cls_c = c; m->cls_top_k = p.top_k;
    return MARS_OK;
}

mars_error_t mars_hip_classify_results(mars_model_t *model, mars_cls_t *top, int *sums, int *channels) {
    if (!model || !top) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    const size_t F = (size_t)m->cls.frames;
    const mars_block_part_t parts[2] = {{top, m->cls_top_off, F * m->cls_top_k * sizeof(mars_cls_t)}, {sums, m->cls_sums_off, F * m->cls_c * sizeof(int)}};
    const mars_error_t e = mars_block_fetch(&m->cls, parts, 2, &m->tail_pending);
    if (e == MARS_OK && channels) *channels = m->cls_c;
    return e;
}

mars_error_t mars_hip_classify(mars_model_t *model, const mars_hip_cls_opts_t *opts, mars_cls_t *top, int *sums) {
    if (!model || !opts || !top) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_classify_device(model, opts);
    return e != MARS_OK ? e : mars_hip_classify_results(model, top, sums, NULL);
}

mars_error_t mars_hip_label_detections_device(mars_model_t *det_model, mars_model_t *cls_model) {
    if (!det_model || !cls_model) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model, *m = (mars_model_ext_t *)cls_model;
    return mars_scatter_on_aux(det, m, &m->cls, m->cls_top_off, m->cls_top_k, &det->label);
}

mars_error_t mars_hip_label_results(mars_model_t *det_model, mars_cls_t *labels) {
    if (!det_model || !labels) return MARS_ERR_INVALID_FILE;
    return mars_side_fetch(&((mars_model_ext_t *)det_model)->label, labels, sizeof(mars_cls_t));
}
