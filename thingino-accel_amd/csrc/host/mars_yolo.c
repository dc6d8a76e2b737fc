/*
 * mars_yolo.c -- host side of the detection tail (decode + NMS on the GPU).
 *
 * The reference keeps this in a demo program: src/mars/mars_yolo_test.c:80-104
 * (parse_output) and :107-130 (nms).  Here the host only tabulates the three
 * float functions of an int8 value the decode needs -- with the host libm, in
 * the reference's exact expression order -- and launches yolo_tail.hip.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mars_internal.h"
#include "nna.h"

/* lut[0..255] = (float)q*scale ; lut[256..511] = obj(q) ; lut[512..767] = 1 + expf(-val(q)) */
static void build_decode_lut(float scale, float *lut) {
    for (int q = -128; q < 128; q++) {
        float val = (float)q * scale;
        lut[q + 128] = val;
        lut[256 + q + 128] = 1.0f / (1.0f + expf((-(float)q) * scale)); /* :84 */
        lut[512 + q + 128] = 1.0f + expf(-val);                         /* :92 */
    }
}

/* value[q] strictly increasing over the whole table: the decode kernel may then take the class argmax on the int8 bytes
 * (first maximum of q == first maximum of value[q]); any NaN, a zero / negative / underflowing scale says no */
static int lut_increasing(const float *lut) {
    for (int i = 1; i < 256; i++)
        if (!(lut[i] > lut[i - 1])) return 0;
    return 1;
}

static int ensure_det_buffers(mars_model_ext_t *m, int frames) {
    if (m->det_cap >= frames && m->det_dev) return 0;
    if (m->det_dev) mhip_free(m->det_dev);
    if (m->det_counts_dev) mhip_free(m->det_counts_dev);
    m->det_dev = mhip_malloc((size_t)frames * MARS_YOLO_MAX_DET * sizeof(mars_det_t));
    m->det_counts_dev = (int *)mhip_malloc((size_t)frames * 2 * sizeof(int));
    if (!m->det_lut_dev) m->det_lut_dev = (float *)mhip_malloc(4 * 768 * sizeof(float));
    if (!m->det_dev || !m->det_counts_dev || !m->det_lut_dev) return -1;
    m->det_cap = frames;
    return 0;
}

/* decode tables of the listed outputs (they depend only on the output scales): built and uploaded once.  Synchronises. */
mars_error_t mars_detect_prepare(mars_model_ext_t *m, const int *output_indices, int n_outputs) {
    mars_model_t *model = &m->pub;
    if (!output_indices || n_outputs <= 0 || n_outputs > 4) return MARS_ERR_INVALID_TENSOR;
    if (!m->det_lut_dev) m->det_lut_dev = (float *)mhip_malloc(4 * 768 * sizeof(float));
    if (!m->det_lut_dev) return MARS_ERR_ALLOC_FAILED;
    float key[4][2] = {{0}};
    for (int s = 0; s < n_outputs; s++) {
        mars_runtime_tensor_t *t = mars_get_output(model, output_indices[s]);
        if (!t || t->desc.dtype != MARS_DTYPE_INT8) return MARS_ERR_INVALID_TENSOR;
        key[s][0] = t->desc.scale;
    }
    if (!mars_lut_stale(&m->det_lut, n_outputs, key)) return MARS_OK;
    float lut[4 * 768];
    for (int s = 0; s < n_outputs; s++) {
        build_decode_lut(key[s][0], lut + s * 768);
        m->det_lut_mono[s] = lut_increasing(lut + s * 768);
    }
    return mars_lut_refresh(&m->det_lut, m->det_lut_dev, n_outputs, key, lut, 768); /* `lut` is on this stack frame */
}

/* decode + NMS of the current batch on the CURRENT stream, from the output tensors' current device buffers into
 * dets_dev [batch][1000] / counts_dev [2 * batch].  Tables must be prepared.  0 or a launch error. */
int mars_detect_launch(mars_model_ext_t *m, const int *output_indices, int n_outputs, float nms_thresh, void *dets_dev,
                       int *counts_dev) {
    mars_model_t *model = &m->pub;
    mhip_detect_t p;
    memset(&p, 0, sizeof(p));
    for (int s = 0; s < n_outputs; s++) {
        if (output_indices[s] < 0 || (uint32_t)output_indices[s] >= model->header.num_outputs) return -1;
        uint32_t ti = model->header.output_tensor_ids[output_indices[s]];
        if (ti >= model->header.num_tensors || !m->mt[ti].dev) return -1;
        p.pred[s] = (const int8_t *)m->mt[ti].dev;
        p.stride[s] = m->mt[ti].stride;
        p.pix_c[s] = m->mt[ti].pix_c; p.pix_stride[s] = m->mt[ti].pix_stride;
        p.npred[s] = (int)(m->mt[ti].bytes / 85); /* rows of 85 int8: x,y,w,h,obj,80 classes */
        p.lut[s] = m->det_lut_dev + s * 768;
        p.mono[s] = m->det_lut_mono[s];
    }
    p.nseg = n_outputs;
    p.frames = m->batch;
    p.nms_thresh = nms_thresh;
    p.dets = dets_dev;
    p.counts = counts_dev;
    p.raw_counts = counts_dev + m->batch;
    p.do_nms = 1;
    return mhip_detect(&p);
}

typedef struct { const int *output_indices; int n_outputs; float nms_thresh; } detect_cfg_t;
static int detect_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    const detect_cfg_t *c = (const detect_cfg_t *)cfg;
    return mars_detect_launch(m, c->output_indices, c->n_outputs, c->nms_thresh, dets_dev, counts_dev);
}

mars_error_t mars_hip_detect_device(mars_model_t *model, const int *output_indices, int n_outputs, float nms_thresh) {
    if (!model || !output_indices || n_outputs <= 0 || n_outputs > 4) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mars_error_t e = mars_own_det_buffers(m);
    if (e != MARS_OK) return e;
    for (int s = 0; s < n_outputs; s++) {
        if (!mars_get_output(model, output_indices[s])) return MARS_ERR_INVALID_TENSOR;
        uint32_t ti = model->header.output_tensor_ids[output_indices[s]];
        if (!m->mt[ti].dev) return MARS_ERR_INVALID_TENSOR;
    }
    if ((e = mars_detect_prepare(m, output_indices, n_outputs)) != MARS_OK) return e;
    /* The tail runs on the auxiliary stream: it starts when the graph launches enqueued so far
     * have finished, and the NEXT run's output-writing layers wait for it (mars_hip_run_device_async),
     * so decode/sort/NMS of batch k overlap the convolutions of batch k+1. */
    const detect_cfg_t c = {output_indices, n_outputs, nms_thresh};
    if ((e = mars_tail_on_aux(m, detect_launch_cb, &c)) == MARS_OK) m->det_mapped = 0;
    return e;
}

mars_error_t mars_hip_detect(mars_model_t *model, const int *output_indices, int n_outputs, float nms_thresh,
                             mars_det_t *dets, int *counts) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_device(model, output_indices, n_outputs, nms_thresh);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams: the tail ran on the auxiliary one */
    m->tail_pending = 0; /* ... and is complete: the next run needs no hand-off (and may replay its captured graph) */
    if (mhip_d2h_async(dets, m->det_dev, (size_t)m->batch * MARS_YOLO_MAX_DET * sizeof(mars_det_t)) ||
        mhip_d2h_async(counts, m->det_counts_dev, (size_t)m->batch * sizeof(int)) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

/* ---- host-pointer, single-frame forms with the reference's signatures */
static int need_device(const char *who) {
    if (nna_is_ready() || nna_init() == NNA_SUCCESS) return 0;
    fprintf(stderr, "%s: no MI355X device available\n", who);
    return -1;
}

int mars_yolo_parse_output(const int8_t *data, int npred, float scale, mars_det_t *dets, int maxd) {
    if (!data || !dets || npred <= 0 || maxd <= 0) return 0;
    if (maxd > MARS_YOLO_MAX_DET) maxd = MARS_YOLO_MAX_DET;
    if (need_device("mars_yolo_parse_output")) return -1;
    const size_t pb = (size_t)npred * 85;
    uint8_t *d = (uint8_t *)mhip_malloc(pb + 256 + 768 * 4 + MARS_YOLO_MAX_DET * sizeof(mars_det_t) + 64);
    if (!d) return -1;
    float lut[768];
    build_decode_lut(scale, lut);
    uint8_t *dl = d + ((pb + 255) & ~(size_t)255);
    uint8_t *dd = dl + 768 * 4;
    int *dc = (int *)(dd + MARS_YOLO_MAX_DET * sizeof(mars_det_t));
    mhip_detect_t p;
    memset(&p, 0, sizeof(p));
    p.pred[0] = (const int8_t *)d; p.stride[0] = 0; p.npred[0] = npred; p.lut[0] = (const float *)dl;
    p.mono[0] = lut_increasing(lut);
    p.nseg = 1; p.frames = 1; p.dets = dd; p.counts = dc; p.raw_counts = NULL; p.do_nms = 0;
    int n = -1;
    if (!mhip_h2d_async(d, data, pb) && !mhip_h2d_async(dl, lut, sizeof(lut)) && !mhip_detect(&p) &&
        !mhip_d2h_async(&n, dc, sizeof(int)) && !mhip_sync()) {
        if (n > maxd) n = maxd; /* the first maxd candidates in scan order */
        if (n > 0 && (mhip_d2h_async(dets, dd, (size_t)n * sizeof(mars_det_t)) || mhip_sync())) n = -1;
    } else {
        mhip_sync();
        n = -1;
    }
    mhip_free(d);
    return n;
}

int mars_yolo_nms(mars_det_t *dets, int n, float thresh) {
    if (!dets || n <= 0) return 0;
    if (n > MARS_YOLO_MAX_DET) return -1;
    if (need_device("mars_yolo_nms")) return -1;
    uint8_t *d = (uint8_t *)mhip_malloc(MARS_YOLO_MAX_DET * sizeof(mars_det_t) + 64);
    if (!d) return -1;
    int *dc = (int *)(d + MARS_YOLO_MAX_DET * sizeof(mars_det_t));
    int kept = -1;
    if (!mhip_h2d_async(d, dets, (size_t)n * sizeof(mars_det_t)) && !mhip_h2d_async(dc, &n, sizeof(int)) &&
        !mhip_nms_only(d, dc, n, thresh) && !mhip_d2h_async(&kept, dc, sizeof(int)) && !mhip_sync()) {
        if (kept > 0 && (mhip_d2h_async(dets, d, (size_t)kept * sizeof(mars_det_t)) || mhip_sync())) kept = -1;
    } else {
        mhip_sync();
        kept = -1;
    }
    mhip_free(d);
    return kept;
}

/* ---- raw anchor-based YOLOv5 Detect heads (include/mars_hip.h: mars_hip_detect_heads) */
static int tensor_by_id(const mars_model_ext_t *m, uint32_t id) {
    if (id == NO_TENSOR) return -1;
    for (uint32_t i = 0; i < m->pub.header.num_tensors; i++)
        if (m->pub.tensors[i].desc.id == id) return (int)i;
    return -1;
}

/* channels and grid of a 4-D [1, C, H, W] / [1, H, W, C] (NHWC tag) tensor; -1 if it is not one */
int mars_tensor_chw(const mars_tensor_t *d, int *c, int *h, int *w) {
    if (d->ndims != 4 || d->shape[0] != 1) return -1;
    if (d->format == MARS_FORMAT_NHWC) { *h = d->shape[1]; *w = d->shape[2]; *c = d->shape[3]; }
    else { *c = d->shape[1]; *h = d->shape[2]; *w = d->shape[3]; }
    return *c > 0 && *h > 0 && *w > 0 ? 0 : -1;
}

/* graph input 0's grid (what the strides divide) */
static int input_hw(const mars_model_ext_t *m, int *h, int *w) {
    int c;
    if (m->pub.header.num_inputs < 1 || m->pub.header.input_tensor_ids[0] >= m->pub.header.num_tensors) return -1;
    return mars_tensor_chw(&m->pub.tensors[m->pub.header.input_tensor_ids[0]].desc, &c, h, w);
}

int mars_find_heads(const mars_model_ext_t *m, int *tensor_ids, int *strides, int *num_classes, int cap) {
    const uint32_t nl = m->pub.header.num_layers;
    int ih, iw, n = 0, ti[4], st[4], nc[4];
    if (input_hw(m, &ih, &iw)) return 0;
    for (uint32_t li = 0; li < nl; li++) {
        const mars_layer_t *L = &m->pub.layers[li].desc;
        if (L->type != MARS_LAYER_CONV2D || L->num_outputs < 1 || m->layer_noop[li]) continue;
        const int T = tensor_by_id(m, L->output_tensor_ids[0]);
        if (T < 0 || m->mt[T].is_weight) continue;
        const mars_tensor_t *d = &m->pub.tensors[T].desc;
        int c, h, w;
        if (d->dtype != MARS_DTYPE_INT8 || mars_tensor_chw(d, &c, &h, &w) || c % 3 || c / 3 - 5 < 1) continue;
        if (ih % h || iw % w || ih / h != iw / w) continue;
        int read = 0; /* by a layer that does something */
        for (uint32_t lj = 0; lj < nl && !read && !m->mt[T].io_out; lj++) {
            const mars_layer_t *R = &m->pub.layers[lj].desc;
            for (uint32_t k = 0; k < R->num_inputs && k < 4; k++)
                if (R->input_tensor_ids[k] == d->id && !m->layer_noop[lj]) read = 1;
        }
        if (read) continue;
        if (n < 4) { ti[n] = T; st[n] = ih / h; nc[n] = c / 3 - 5; }
        n++;
    }
    const int kept = n < 4 ? n : 4;
    for (int i = 1; i < kept; i++) /* by stride, stable */
        for (int j = i; j > 0 && st[j - 1] > st[j]; j--) {
            int t;
            t = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = t;
            t = st[j]; st[j] = st[j - 1]; st[j - 1] = t;
            t = nc[j]; nc[j] = nc[j - 1]; nc[j - 1] = t;
        }
    for (int i = 0; i < kept && i < cap; i++) {
        if (tensor_ids) tensor_ids[i] = ti[i];
        if (strides) strides[i] = st[i];
        if (num_classes) num_classes[i] = nc[i];
    }
    return n;
}

/* the letterbox of mars_preproc.c (the reference's load_image, mars_yolo_test.c:47-49) of w x hs frames for a tw x th graph input, as
 * the mapping of the kept boxes back into the frame */
static mars_error_t letterbox_of(int w, int hs, int tw, int th, int *map, int *px, int *py, float *rx, float *ry, int *nw_out, int *nh_out) {
    if (w <= 0 || hs <= 0) return MARS_ERR_INVALID_TENSOR;
    const float scale = fminf((float)tw / w, (float)th / hs);
    const int nw = (int)(w * scale), nh = (int)(hs * scale);
    if (nw <= 0 || nh <= 0) return MARS_ERR_INVALID_TENSOR;
    *map = 1;
    *px = (tw - nw) / 2;
    *py = (th - nh) / 2;
    *rx = (float)w / (float)nw;
    *ry = (float)hs / (float)nh;
    if (nw_out) *nw_out = nw;
    if (nh_out) *nh_out = nh;
    return MARS_OK;
}

static const float k_default_anchors[3][3][2] = {{{10, 13}, {16, 30}, {33, 23}}, {{30, 61}, {62, 45}, {59, 119}}, {{116, 90}, {156, 198}, {373, 326}}};

mars_error_t mars_heads_resolve(mars_model_ext_t *m, const mars_yolo_heads_t *h, mars_heads_cfg_t *c) {
    mars_yolo_heads_t zero;
    memset(&zero, 0, sizeof(zero));
    if (!h) h = &zero;
    memset(c, 0, sizeof(*c));
    int ih, iw;
    if (h->n_heads < 0 || h->n_heads > 4 || input_hw(m, &ih, &iw)) return MARS_ERR_INVALID_TENSOR;
    int n = h->n_heads;
    if (n == 0) {
        n = mars_find_heads(m, c->ti, NULL, NULL, 4);
        if (n <= 0 || n > 4) return MARS_ERR_INVALID_TENSOR;
    } else {
        memcpy(c->ti, h->head_tensors, sizeof(c->ti));
    }
    c->n = n;
    for (int k = 0; k < n; k++) {
        const int T = c->ti[k];
        if (T < 0 || (uint32_t)T >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
        const mtensor_t *t = &m->mt[T];
        const mars_tensor_t *d = &m->pub.tensors[T].desc;
        int ch, hh, ww;
        if (t->is_weight || t->partial || !t->dev || d->dtype != MARS_DTYPE_INT8 || !(d->scale > 0) || mars_tensor_chw(d, &ch, &hh, &ww) ||
            ch % 3 || ch / 3 - 5 < 1)
            return MARS_ERR_INVALID_TENSOR;
        /* the device layout is what the writing convolution stores: planes [C][H][W], or pixel rows at its pitch (NHWC tensors, the
         * padded rows of graph outputs, NCHW-tagged tensors held pixels x channels) */
        const mars_op_t *wr = NULL;
        for (int i = 0; i < m->n_ops && !wr; i++)
            if (m->ops[i].kind == OP_CONV_I8 && m->ops[i].t_out == T) wr = &m->ops[i];
        if (!wr || wr->out_ch_off || wr->out_byte_off || wr->out_c != ch || wr->out_h != hh || wr->out_w != ww) return MARS_ERR_INVALID_TENSOR;
        if (wr->out_nchw) { c->pix_step[k] = 1; c->ch_step[k] = hh * ww; }
        else { c->pix_step[k] = wr->out_pix_stride ? wr->out_pix_stride : ch; c->ch_step[k] = 1; }
        c->h[k] = hh; c->w[k] = ww; c->nc[k] = ch / 3 - 5;
        c->stride[k] = h->strides[k] > 0 ? h->strides[k] : ih / hh;
        if (h->strides[k] < 0 || c->stride[k] <= 0) return MARS_ERR_INVALID_TENSOR;
        if (!t->io_out) c->internal = 1;
    }
    int any = 0;
    for (int k = 0; k < 4; k++)
        for (int a = 0; a < 3; a++) any |= h->anchors[k][a][0] != 0 || h->anchors[k][a][1] != 0;
    if (any) memcpy(c->anchors, h->anchors, sizeof(c->anchors));
    else if (n <= 3) memcpy(c->anchors, k_default_anchors, (size_t)n * sizeof(k_default_anchors[0]));
    else return MARS_ERR_INVALID_TENSOR; /* no default anchors for a fourth head */
    c->conf = h->conf_thresh != 0 ? h->conf_thresh : 0.25f;
    c->nms = h->nms_thresh != 0 ? h->nms_thresh : 0.45f;
    if (h->src_w || h->src_h) return letterbox_of(h->src_w, h->src_h, iw, ih, &c->map, &c->px, &c->py, &c->rx, &c->ry, NULL, NULL);
    return MARS_OK;
}

/* sigmoid tables of the heads (they depend only on the heads' scales): built and uploaded once.  Synchronises when they change. */
mars_error_t mars_heads_prepare(mars_model_ext_t *m, const mars_heads_cfg_t *c) {
    if (!m->heads_lut_dev) m->heads_lut_dev = (float *)mhip_malloc(4 * 256 * sizeof(float));
    if (!m->heads_lut_dev) return MARS_ERR_ALLOC_FAILED;
    float key[4][2] = {{0}};
    for (int k = 0; k < c->n; k++) key[k][0] = m->pub.tensors[c->ti[k]].desc.scale;
    if (!mars_lut_stale(&m->heads_lut, c->n, key)) return MARS_OK;
    float lut[4 * 256], tab[768];
    for (int k = 0; k < c->n; k++) {
        build_decode_lut(key[k][0], tab); /* its obj(q) = 1 / (1 + expf(-q * scale)): the sigmoid of every head byte */
        memcpy(lut + k * 256, tab + 256, 256 * sizeof(float));
    }
    return mars_lut_refresh(&m->heads_lut, m->heads_lut_dev, c->n, key, lut, 256); /* `lut` is on this stack frame */
}

int mars_heads_launch(mars_model_ext_t *m, const mars_heads_cfg_t *c, void *dets_dev, int *counts_dev) {
    mhip_heads_t p;
    memset(&p, 0, sizeof(p));
    for (int k = 0; k < c->n; k++) {
        const mtensor_t *t = &m->mt[c->ti[k]];
        if (!t->dev) return -1;
        p.base[k] = (const int8_t *)t->dev;
        p.frame_stride[k] = t->stride;
        p.h[k] = c->h[k]; p.w[k] = c->w[k]; p.nc[k] = c->nc[k];
        p.pix_step[k] = c->pix_step[k]; p.ch_step[k] = c->ch_step[k];
        p.stride[k] = c->stride[k];
    }
    memcpy(p.anchors, c->anchors, sizeof(p.anchors));
    p.sig = m->heads_lut_dev;
    p.nheads = c->n;
    p.frames = m->batch;
    p.conf = c->conf;
    p.nms_thresh = c->nms;
    p.dets = dets_dev;
    p.counts = counts_dev;
    p.raw_counts = counts_dev + m->batch;
    p.map = c->map; p.px = c->px; p.py = c->py; p.rx = c->rx; p.ry = c->ry;
    return mhip_detect_heads(&p);
}

/* the model's own detection buffers, large enough for the current batch */
mars_error_t mars_own_det_buffers(mars_model_ext_t *m) {
    if (m->det_cap >= m->batch && m->det_dev) return MARS_OK;
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: nothing may be in flight */
    if (ensure_det_buffers(m, m->batch)) return MARS_ERR_ALLOC_FAILED;
    m->det_lut.n = 0;
    return MARS_OK;
}

/* a tail (launch(m, cfg, dets, counts) on the current stream: the decode of graph outputs, of raw heads, a later stage's) runs on the
 * auxiliary stream behind whatever the SELECTED stream has been given (no stream is selected here: the caller's stays), and the next
 * run's layers that write a tensor it reads wait for it (graph outputs; tail_read, set by the caller, where the heads are internal tensors) */
mars_error_t mars_tail_on_aux(mars_model_ext_t *m, int (*launch)(mars_model_ext_t *, const void *, void *, int *), const void *cfg) {
    if (!m->ev_tail_done && !(m->ev_tail_done = mhip_event_create_sync())) return MARS_ERR_ALLOC_FAILED;
    const mars_error_t e = mars_aux_behind_current(&m->ev_graph_done);
    if (e != MARS_OK) return e;
    int rc = launch(m, cfg, m->det_dev, m->det_counts_dev);
    if (!rc) rc = mhip_event_record(m->ev_tail_done);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->tail_pending = 1;
    return MARS_OK;
}

static int heads_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    return mars_heads_launch(m, (const mars_heads_cfg_t *)cfg, dets_dev, counts_dev);
}

mars_error_t mars_hip_detect_heads_device(mars_model_t *model, const mars_yolo_heads_t *heads) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mars_heads_cfg_t c;
    mars_error_t e = mars_heads_resolve(m, heads, &c);
    if (e == MARS_OK) e = mars_own_det_buffers(m);
    if (e == MARS_OK) e = mars_heads_prepare(m, &c);
    if (e != MARS_OK) return e;
    for (int k = 0; k < c.n; k++) m->mt[c.ti[k]].tail_read = 1;
    e = mars_tail_on_aux(m, heads_launch_cb, &c);
    if (e == MARS_OK) m->det_mapped = c.map;
    return e;
}

mars_error_t mars_hip_detect_results(mars_model_t *model, mars_det_t *dets, int *counts) {
    if (!model || !dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if (!m->det_dev || m->det_cap < m->batch) return MARS_ERR_INVALID_TENSOR;
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    m->tail_pending = 0;
    if (mhip_d2h_async(dets, m->det_dev, (size_t)m->batch * MARS_YOLO_MAX_DET * sizeof(mars_det_t)) ||
        mhip_d2h_async(counts, m->det_counts_dev, (size_t)m->batch * sizeof(int)) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

mars_error_t mars_hip_detect_heads(mars_model_t *model, const mars_yolo_heads_t *heads, mars_det_t *dets, int *counts) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_heads_device(model, heads);
    return e != MARS_OK ? e : mars_hip_detect_results(model, dets, counts);
}

/* ---- raw anchor-free DFL heads (include/mars_hip.h: mars_hip_detect_dfl) */
/* index of the CONV2D layer that does something and writes tensor T, or -1 */
static int conv_layer_of(const mars_model_ext_t *m, int T) {
    const uint32_t id = m->pub.tensors[T].desc.id;
    for (uint32_t li = 0; li < m->pub.header.num_layers; li++) {
        const mars_layer_t *L = &m->pub.layers[li].desc;
        if (L->type == MARS_LAYER_CONV2D && L->num_outputs >= 1 && !m->layer_noop[li] && L->output_tensor_ids[0] == id) return (int)li;
    }
    return -1;
}

/* layers that do something and read tensor T, `except` not counted */
static int real_readers(const mars_model_ext_t *m, int T, uint32_t except) {
    const uint32_t id = m->pub.tensors[T].desc.id;
    int n = 0;
    for (uint32_t lj = 0; lj < m->pub.header.num_layers; lj++) {
        const mars_layer_t *R = &m->pub.layers[lj].desc;
        if (lj == except || m->layer_noop[lj]) continue;
        for (uint32_t k = 0; k < R->num_inputs && k < 4; k++)
            if (R->input_tensor_ids[k] == id) { n++; break; }
    }
    return n;
}

int mars_find_dfl_heads(const mars_model_ext_t *m, int *box_ids, int *cls_ids, int *strides, int *num_classes, int *reg_max, int cap) {
    const uint32_t nl = m->pub.header.num_layers;
    int ih, iw, n = 0, bt[4], ct[4], st[4], nc[4], rm[4];
    if (input_hw(m, &ih, &iw)) return 0;
    for (uint32_t li = 0; li < nl; li++) {
        const mars_layer_t *L = &m->pub.layers[li].desc;
        if (L->type != MARS_LAYER_CONCAT || L->num_inputs != 2 || L->num_outputs < 1 || m->layer_noop[li]) continue;
        const int A = tensor_by_id(m, L->input_tensor_ids[0]), B = tensor_by_id(m, L->input_tensor_ids[1]), O = tensor_by_id(m, L->output_tensor_ids[0]);
        if (A < 0 || B < 0 || O < 0 || A == B) continue;
        int ca, ha, wa, cb, hb, wb, ok = 1;
        for (int q = 0; q < 2 && ok; q++) { /* int8 activations out of convolutions, read by this CONCAT alone */
            const int T = q ? B : A;
            ok = !m->mt[T].is_weight && m->pub.tensors[T].desc.dtype == MARS_DTYPE_INT8 && conv_layer_of(m, T) >= 0 && !real_readers(m, T, li);
        }
        if (!ok || mars_tensor_chw(&m->pub.tensors[A].desc, &ca, &ha, &wa) || mars_tensor_chw(&m->pub.tensors[B].desc, &cb, &hb, &wb)) continue;
        if (ha != hb || wa != wb || ih % ha || iw % wa || ih / ha != iw / wa) continue;
        if (ca % 4 || ca / 4 < 2 || ca / 4 > 32) continue;
        if (!m->mt[O].io_out && real_readers(m, O, nl)) continue;
        if (n < 4) { bt[n] = A; ct[n] = B; st[n] = ih / ha; nc[n] = cb; rm[n] = ca / 4; }
        n++;
    }
    const int kept = n < 4 ? n : 4;
    for (int i = 1; i < kept; i++) /* by stride, stable */
        for (int j = i; j > 0 && st[j - 1] > st[j]; j--) {
            int t;
#define SWAP(a) t = a[j]; a[j] = a[j - 1]; a[j - 1] = t
            SWAP(bt); SWAP(ct); SWAP(st); SWAP(nc); SWAP(rm);
#undef SWAP
        }
    for (int i = 0; i < kept && i < cap; i++) {
        if (box_ids) box_ids[i] = bt[i];
        if (cls_ids) cls_ids[i] = ct[i];
        if (strides) strides[i] = st[i];
        if (num_classes) num_classes[i] = nc[i];
        if (reg_max) reg_max[i] = rm[i];
    }
    return n;
}

/* Where the plan left the int8 bytes of activation tensor T ([ch] channels on an hh x ww grid): its own buffer -- planes [C][H][W], or pixel
 * rows at the writing convolution's pitch (NHWC tensors, NCHW-tagged ones held pixels x channels, the padded rows of graph outputs) -- or,
 * where the zero-copy concat redirected that convolution, a channel slice of the concat output's pixel rows.  any_writer = 0: only what a
 * convolution wrote (the Detect heads); != 0: a tensor some other launch writes (a LUT map, an Add, a pool), or a graph input, too, laid
 * out as mars_hip_read_tensor finds it.  0, or -1 if there are no such bytes. */
int mars_locate_i8(const mars_model_ext_t *m, int T, int ch, int hh, int ww, int any_writer, int *buf, int *off, int *pix_step, int *ch_step) {
    const mtensor_t *t = &m->mt[T];
    const mars_op_t *wr = NULL;
    if (t->is_weight || t->partial) return -1;
    for (int i = 0; i < m->n_ops && !wr; i++)
        if (m->ops[i].kind == OP_CONV_I8 && m->ops[i].t_out == T) wr = &m->ops[i];
    if (wr) {
        if (!t->dev || wr->out_ch_off || wr->out_byte_off || wr->out_c != ch || wr->out_h != hh || wr->out_w != ww) return -1;
        *buf = T;
        *off = 0;
        if (wr->out_nchw) { *pix_step = 1; *ch_step = hh * ww; }
        else { *pix_step = wr->out_pix_stride ? wr->out_pix_stride : ch; *ch_step = 1; }
        return 0;
    }
    const int li = conv_layer_of(m, T);
    for (int i = 0; i < m->n_ops && li >= 0; i++) {
        const mars_op_t *o = &m->ops[i];
        if (o->kind != OP_CONV_I8 || o->layer != li) continue;
        /* a plain convolution (no folded table or Add: the slice then holds T's bytes) writing rows of a wider tensor */
        if (o->t_out < 0 || o->t_out == T || o->out_nchw || o->out_byte_off || o->lut_off != NO_OFF || o->add_t || o->out_pix_stride <= 0 ||
            o->out_ch_off < 0 || o->out_ch_off + ch > o->out_pix_stride || o->out_c != ch || o->out_h != hh || o->out_w != ww ||
            !m->mt[o->t_out].dev || m->mt[o->t_out].partial)
            return -1;
        *buf = o->t_out;
        *off = o->out_ch_off;
        *pix_step = o->out_pix_stride;
        *ch_step = 1;
        return 0;
    }
    if (!any_writer || !t->dev || t->rec_c) return -1;
    const size_t hw = (size_t)hh * ww;
    *buf = T;
    *off = 0;
    *ch_step = 1;
    if (t->nhwc_c) { /* pixels x channels (nhwc_internal) */
        if (t->nhwc_c != ch || (size_t)t->nhwc_hw != hw) return -1;
        *pix_step = t->nhwc_pitch ? t->nhwc_pitch : ch;
    } else if (t->pix_stride) { /* padded pixel rows (pad_output_rows) */
        if (t->pix_c != ch || t->bytes != hw * (size_t)ch) return -1;
        *pix_step = t->pix_stride;
    } else if (t->bytes != hw * (size_t)ch) {
        return -1;
    } else if (m->pub.tensors[T].desc.format == MARS_FORMAT_NHWC) {
        *pix_step = ch;
    } else {
        *pix_step = 1;
        *ch_step = hh * ww;
    }
    return 0;
}

mars_error_t mars_dfl_resolve(mars_model_ext_t *m, const mars_yolo_dfl_heads_t *h, mars_dfl_cfg_t *c) {
    mars_yolo_dfl_heads_t zero;
    memset(&zero, 0, sizeof(zero));
    if (!h) h = &zero;
    memset(c, 0, sizeof(*c));
    int ih, iw;
    if (h->n_heads < 0 || h->n_heads > 4 || h->reg_max < 0 || input_hw(m, &ih, &iw)) return MARS_ERR_INVALID_TENSOR;
    int n = h->n_heads;
    if (n == 0) {
        n = mars_find_dfl_heads(m, c->box_t, c->cls_t, NULL, NULL, NULL, 4);
        if (n <= 0 || n > 4) return MARS_ERR_INVALID_TENSOR;
    } else {
        memcpy(c->box_t, h->box_tensors, sizeof(c->box_t));
        memcpy(c->cls_t, h->cls_tensors, sizeof(c->cls_t));
    }
    c->n = n;
    for (int k = 0; k < n; k++) {
        const int A = c->box_t[k], B = c->cls_t[k];
        if (A < 0 || B < 0 || (uint32_t)A >= m->pub.header.num_tensors || (uint32_t)B >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
        const mars_tensor_t *da = &m->pub.tensors[A].desc, *db = &m->pub.tensors[B].desc;
        int ca, ha, wa, cb, hb, wb;
        if (da->dtype != MARS_DTYPE_INT8 || db->dtype != MARS_DTYPE_INT8 || mars_tensor_chw(da, &ca, &ha, &wa) || mars_tensor_chw(db, &cb, &hb, &wb) ||
            ha != hb || wa != wb)
            return MARS_ERR_INVALID_TENSOR;
        const int R = h->reg_max ? h->reg_max : ca / 4;
        if (ca != 4 * R || R < 2 || R > 32 || (k && R != c->reg_max)) return MARS_ERR_INVALID_TENSOR;
        c->reg_max = R;
        if (mars_locate_i8(m, A, ca, ha, wa, 0, &c->box_buf[k], &c->box_off[k], &c->box_pix_step[k], &c->box_ch_step[k]) ||
            mars_locate_i8(m, B, cb, hb, wb, 0, &c->cls_buf[k], &c->cls_off[k], &c->cls_pix_step[k], &c->cls_ch_step[k]))
            return MARS_ERR_INVALID_TENSOR;
        c->box_scale[k] = h->box_scales[k] != 0 ? h->box_scales[k] : da->scale;
        c->cls_scale[k] = h->cls_scales[k] != 0 ? h->cls_scales[k] : db->scale;
        if (!(c->box_scale[k] > 0) || !(c->cls_scale[k] > 0)) return MARS_ERR_INVALID_TENSOR;
        c->h[k] = ha; c->w[k] = wa; c->nc[k] = cb;
        c->stride[k] = h->strides[k] > 0 ? h->strides[k] : ih / ha;
        if (h->strides[k] < 0 || c->stride[k] <= 0) return MARS_ERR_INVALID_TENSOR;
        if (!m->mt[c->box_buf[k]].io_out || !m->mt[c->cls_buf[k]].io_out) c->internal = 1;
    }
    c->conf = h->conf_thresh != 0 ? h->conf_thresh : 0.25f;
    c->nms = h->nms_thresh != 0 ? h->nms_thresh : 0.45f;
    if (h->src_w || h->src_h) return letterbox_of(h->src_w, h->src_h, iw, ih, &c->map, &c->px, &c->py, &c->rx, &c->ry, &c->nw, &c->nh);
    return MARS_OK;
}

/* per head E[d] = expf(-(d * box scale)), d = 0 .. 255, and the class sigmoid (the anchor path's table, by the same expression); they depend
 * only on the effective scales: built and uploaded once.  Synchronises when they change. */
mars_error_t mars_dfl_prepare(mars_model_ext_t *m, const mars_dfl_cfg_t *c) {
    if (!m->dfl_lut_dev) m->dfl_lut_dev = (float *)mhip_malloc(4 * 512 * sizeof(float));
    if (!m->dfl_lut_dev) return MARS_ERR_ALLOC_FAILED;
    float key[4][2] = {{0}};
    for (int k = 0; k < c->n; k++) { key[k][0] = c->box_scale[k]; key[k][1] = c->cls_scale[k]; }
    if (!mars_lut_stale(&m->dfl_lut, c->n, key)) return MARS_OK;
    float lut[4 * 512], tab[768];
    for (int k = 0; k < c->n; k++) {
        for (int d = 0; d < 256; d++) lut[k * 512 + d] = expf(-((float)d * c->box_scale[k]));
        build_decode_lut(c->cls_scale[k], tab);
        memcpy(lut + k * 512 + 256, tab + 256, 256 * sizeof(float));
    }
    return mars_lut_refresh(&m->dfl_lut, m->dfl_lut_dev, c->n, key, lut, 512); /* `lut` is on this stack frame */
}

int mars_dfl_launch(mars_model_ext_t *m, const mars_dfl_cfg_t *c, void *dets_dev, int *counts_dev) {
    mhip_dfl_heads_t p;
    memset(&p, 0, sizeof(p));
    for (int k = 0; k < c->n; k++) {
        const mtensor_t *tb = &m->mt[c->box_buf[k]], *tc = &m->mt[c->cls_buf[k]];
        if (!tb->dev || !tc->dev) return -1;
        p.box[k] = (const int8_t *)tb->dev + c->box_off[k];
        p.cls[k] = (const int8_t *)tc->dev + c->cls_off[k];
        p.box_frame_stride[k] = tb->stride; p.cls_frame_stride[k] = tc->stride;
        p.h[k] = c->h[k]; p.w[k] = c->w[k]; p.nc[k] = c->nc[k];
        p.box_pix_step[k] = c->box_pix_step[k]; p.box_ch_step[k] = c->box_ch_step[k];
        p.cls_pix_step[k] = c->cls_pix_step[k]; p.cls_ch_step[k] = c->cls_ch_step[k];
        p.stride[k] = c->stride[k];
    }
    p.reg_max = c->reg_max;
    p.tab = m->dfl_lut_dev;
    p.nheads = c->n;
    p.frames = m->batch;
    p.conf = c->conf;
    p.nms_thresh = c->nms;
    p.dets = dets_dev;
    p.counts = counts_dev;
    p.raw_counts = counts_dev + m->batch;
    p.map = c->map; p.px = c->px; p.py = c->py; p.rx = c->rx; p.ry = c->ry;
    p.cand_pred = c->cand_pred; p.kept_pred = c->kept_pred; p.premap = c->premap;
    return mhip_detect_dfl(&p);
}

static int dfl_launch_cb(mars_model_ext_t *m, const void *cfg, void *dets_dev, int *counts_dev) {
    return mars_dfl_launch(m, (const mars_dfl_cfg_t *)cfg, dets_dev, counts_dev);
}

mars_error_t mars_hip_detect_dfl_device(mars_model_t *model, const mars_yolo_dfl_heads_t *heads) {
    if (!model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    mars_dfl_cfg_t c;
    mars_error_t e = mars_dfl_resolve(m, heads, &c);
    if (e == MARS_OK) e = mars_own_det_buffers(m);
    if (e == MARS_OK) e = mars_dfl_prepare(m, &c);
    if (e != MARS_OK) return e;
    for (int k = 0; k < c.n; k++) m->mt[c.box_buf[k]].tail_read = m->mt[c.cls_buf[k]].tail_read = 1;
    e = mars_tail_on_aux(m, dfl_launch_cb, &c);
    if (e == MARS_OK) m->det_mapped = c.map;
    return e;
}

mars_error_t mars_hip_detect_dfl(mars_model_t *model, const mars_yolo_dfl_heads_t *heads, mars_det_t *dets, int *counts) {
    if (!dets || !counts) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_hip_detect_dfl_device(model, heads);
    return e != MARS_OK ? e : mars_hip_detect_results(model, dets, counts);
}
