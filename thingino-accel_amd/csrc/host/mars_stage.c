/*
 * mars_stage.c -- what the stages behind the detection tail share on the host (mars_internal.h, "tail stages"): the result block hung on a
 * model, the per-detection side arrays hung on a detector and the scatter that fills two of them, where the plan left an int8 side tensor,
 * the scale-keyed tables, the graph input that takes int8 pixels, and the hand-off from the selected stream to the auxiliary one.  No launch
 * of its own but the scatter's; the stage files (mars_seg.c, mars_pose.c, mars_obb.c, mars_tile.c, mars_redact.c, mars_overlay.c, mars_motion.c, mars_events.c, mars_shots.c, mars_roi.c,
 * mars_classify.c, mars_gallery.c, mars_track.c), the front-end's target (mars_preproc.c) and the tails and table functions of mars_yolo.c
 * are written on top of it.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

/* ---- result blocks */
size_t mars_block_layout(const size_t *sz, int n, size_t *off) {
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        off[i] = total;
        total += ALIGN_UP(sz[i], 256);
    }
    return total;
}

mars_error_t mars_block_reserve(mars_block_t *b, size_t total, int with_events, int *fresh) {
    if (fresh) *fresh = 0;
    if (!b->dev || b->bytes < total) {
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: an earlier tail, match or scatter may still use the old block */
        if (b->dev) mhip_free(b->dev);
        b->frames = 0; b->bytes = 0;
        if (fresh) *fresh = 1; /* (whatever the caller kept inside the old block is gone, also where the allocation fails) */
        b->dev = mhip_malloc(total);
        if (!b->dev) return MARS_ERR_ALLOC_FAILED;
        b->bytes = total;
    }
    for (int i = 0; with_events && i < 2; i++) {
        if (!b->ev[i]) b->ev[i] = mhip_event_create();
        if (!b->ev[i]) return MARS_ERR_ALLOC_FAILED;
    }
    return MARS_OK;
}

void mars_block_release(mars_block_t *b) {
    if (b->dev) mhip_free(b->dev);
    for (int i = 0; i < 2; i++)
        if (b->ev[i]) mhip_event_destroy(b->ev[i]);
    memset(b, 0, sizeof(*b));
}

float mars_block_ms(const mars_block_t *b) {
    if (!b->dev || b->frames <= 0 || !b->ev[0] || !b->ev[1]) return -1.0f;
    return mhip_event_elapsed_ms(b->ev[0], b->ev[1]);
}

mars_error_t mars_block_fetch(const mars_block_t *b, const mars_block_part_t *parts, int n, int *tail_pending) {
    if (!b->dev || b->frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no call of the stage yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    if (tail_pending) *tail_pending = 0;
    for (int i = 0; i < n; i++)
        if (parts[i].dst && mhip_d2h_async(parts[i].dst, (const uint8_t *)b->dev + parts[i].off, parts[i].bytes)) return MARS_ERR_LAYER_FAILED;
    return mhip_sync() ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

/* ---- per-detection side arrays */
mars_error_t mars_side_reserve(mars_det_side_t *s, int frames, size_t rec) {
    if (s->dev && s->cap >= frames) return MARS_OK;
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* re-allocation: nothing may be in flight (own_det_buffers) */
    if (s->dev) mhip_free(s->dev);
    s->cap = s->frames = 0;
    s->dev = mhip_malloc((size_t)frames * MARS_YOLO_MAX_DET * rec);
    if (!s->dev) return MARS_ERR_ALLOC_FAILED;
    s->cap = frames;
    return MARS_OK;
}

void mars_side_release(mars_det_side_t *s) {
    if (s->dev) mhip_free(s->dev);
    memset(s, 0, sizeof(*s));
}

mars_error_t mars_side_fetch(const mars_det_side_t *s, void *dst, size_t rec) {
    if (!s->dev || s->frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no scatter / track call yet */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* both streams */
    if (mhip_d2h_async(dst, s->dev, (size_t)s->frames * MARS_YOLO_MAX_DET * rec) || mhip_sync()) return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

mars_error_t mars_scatter_on_aux(mars_model_ext_t *det, mars_model_ext_t *m, const mars_block_t *src, size_t top_off, int top_k,
                                 mars_det_side_t *side) {
    if (det == m) return MARS_ERR_INVALID_TENSOR;
    if (!m->act_dev || !det->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe || det->pipe) return MARS_ERR_INVALID_TENSOR;
    if (!m->roi_dev || m->roi_slots <= 0 || m->roi_from != det) return MARS_ERR_INVALID_TENSOR;             /* no crop call out of det_model */
    if (!src->dev || src->frames <= 0 || src->frames < m->roi_slots) return MARS_ERR_INVALID_TENSOR;        /* no classify / match results */
    if (!mars_has_dets(det)) return MARS_ERR_INVALID_TENSOR; /* no detections in HBM */
    mars_error_t e = mars_side_reserve(side, det->batch, sizeof(mars_cls_t));
    if (e != MARS_OK) return e;
    if (!m->ev_label_done && !(m->ev_label_done = mhip_event_create_sync())) return MARS_ERR_ALLOC_FAILED;
    /* The auxiliary stream.  It carries every detection tail, every classify tail and every match, so the scatter comes behind both models'
     * tails and ahead of det_model's next detect call and cls_model's next classify call.  The ROI table is written on the main stream: the
     * scatter waits for what that stream has been given so far, and the next crop call into cls_model waits for the scatter (ev_label_done,
     * recorded again by every scatter of either kind) */
    mhip_select_stream(0);
    if ((e = mars_aux_behind_current(&m->ev_graph_done)) != MARS_OK) return e;
    int rc = mhip_label_scatter((uint8_t *)m->roi_dev + 16, (const int *)m->roi_dev, m->roi_slots, (const uint8_t *)src->dev + top_off, top_k, side->dev,
                                det->batch, MARS_YOLO_MAX_DET);
    if (!rc) rc = mhip_event_record(m->ev_label_done);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->label_pending = 1;
    side->frames = det->batch;
    return MARS_OK;
}

/* ---- int8 side tensors */
mars_error_t mars_side_tensor(const mars_model_ext_t *m, int T, int want_c, int want_h, int want_w, mars_side_tensor_t *o) {
    if (T < 0 || (uint32_t)T >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
    const mars_tensor_t *d = &m->pub.tensors[T].desc;
    int off;
    if (d->dtype != MARS_DTYPE_INT8 || m->mt[T].is_weight || mars_tensor_chw(d, &o->c, &o->h, &o->w)) return MARS_ERR_INVALID_TENSOR;
    if ((want_c && o->c != want_c) || (want_h && o->h != want_h) || (want_w && o->w != want_w)) return MARS_ERR_INVALID_TENSOR;
    if (mars_locate_i8(m, T, o->c, o->h, o->w, 0, &o->buf, &off, &o->pix_step, &o->ch_step)) return MARS_ERR_INVALID_TENSOR;
    const mtensor_t *tb = &m->mt[o->buf];
    /* ch_step is tested only where a channel is stepped.  mars_locate_i8 gives planes a ch_step of h * w, an int product that a map of 2^31
     * cells or more wraps to zero or below: the oriented stage (one channel, no step taken) has always taken such a tensor as far as the bound
     * below, the mask stage has always refused it and keeps that refusal with its caller */
    if (!tb->dev || o->pix_step <= 0 || (o->c > 1 && o->ch_step <= 0)) return MARS_ERR_INVALID_TENSOR;
    const size_t last = (size_t)off + ((size_t)o->h * o->w - 1) * (size_t)o->pix_step + (size_t)(o->c - 1) * (size_t)o->ch_step;
    if (last >= tb->stride) return MARS_ERR_INVALID_TENSOR;
    o->base = (const int8_t *)tb->dev + off;
    o->stride = tb->stride;
    return MARS_OK;
}

/* ---- the graph input that takes int8 pixels (the front-end, the crops, the tiles) */
_Static_assert(MARS_HIP_CAMERA_RGB == 0 && MARS_HIP_CAMERA_NV12 == 1 && (MARS_NV12_FULL_RANGE | MARS_NV12_VU) == 3u, "mhip_frame_format_ok of csrc/mhip.h");
mars_error_t mars_pixel_input(const mars_model_ext_t *m, int input_index, int geometry_only, mars_pixel_input_t *o) {
    if (input_index < 0 || (uint32_t)input_index >= m->pub.header.num_inputs) return MARS_ERR_INVALID_TENSOR;
    const uint32_t tid = m->pub.header.input_tensor_ids[input_index]; /* an index, as in mars_get_input() */
    if (tid >= m->pub.header.num_tensors) return MARS_ERR_INVALID_TENSOR;
    const mars_tensor_t *t = &m->pub.tensors[tid].desc;
    o->tid = (int)tid;
    o->nhwc = t->format == MARS_FORMAT_NHWC;
    o->th = o->nhwc ? t->shape[1] : t->shape[2]; o->tw = o->nhwc ? t->shape[2] : t->shape[3];
    const int ch = o->nhwc ? t->shape[3] : t->shape[1];
    if (ch != 3 || t->dtype != MARS_DTYPE_INT8 || o->tw <= 0 || o->th <= 0) return MARS_ERR_INVALID_TENSOR;
    if (geometry_only) return MARS_OK;
    if (!m->mt[tid].dev || m->mt[tid].stride < (size_t)o->tw * o->th * 3) return MARS_ERR_INVALID_TENSOR;
    o->dev = (int8_t *)m->mt[tid].dev; o->stride = m->mt[tid].stride;
    return MARS_OK;
}

/* ---- the hand-off to the auxiliary stream */
mars_error_t mars_aux_behind_current(void **ev) {
    if (!*ev && !(*ev = mhip_event_create_sync())) return MARS_ERR_ALLOC_FAILED;
    if (mhip_event_record(*ev)) return MARS_ERR_LAYER_FAILED;
    mhip_select_aux(1);
    if (!mhip_stream_wait(1, *ev)) return MARS_OK;
    mhip_select_aux(0);
    return MARS_ERR_LAYER_FAILED;
}

/* ---- scale-keyed tables */
int mars_lut_stale(const mars_lut_cache_t *c, int n, const float key[4][2]) {
    return c->n != n || memcmp(c->key, key, (size_t)n * sizeof(c->key[0])) != 0; /* bit for bit: -0.0 is not 0.0 */
}

mars_error_t mars_lut_refresh(mars_lut_cache_t *c, void *dst, int n, const float key[4][2], const float *tab, size_t floats_per_head) {
    if (!mars_lut_stale(c, n, key)) return MARS_OK;
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED; /* a tail enqueued earlier may still read the old tables */
    c->n = 0; /* (until the new tables are up) */
    if (mhip_h2d_async(dst, tab, (size_t)n * floats_per_head * sizeof(float)) || mhip_sync()) return MARS_ERR_LAYER_FAILED; /* `tab` is on the caller's stack frame */
    memcpy(c->key, key, (size_t)n * sizeof(c->key[0]));
    c->n = n;
    return MARS_OK;
}

/* ---- everything a model holds for these stages, when its device state goes away */
void mars_stages_release(mars_model_ext_t *m) {
    mars_roi_release(m);
    mars_block_t *blocks[] = {&m->cls, &m->match, &m->seg, &m->segn, &m->pose, &m->obb, &m->tile_roi, &m->tile, &m->track_app, &m->redact,
                            &m->overlay, &m->shot};
    mars_det_side_t *sides[] = {&m->label, &m->ident, &m->track, &m->motion, &m->event};
    for (size_t i = 0; i < sizeof(blocks) / sizeof(blocks[0]); i++) mars_block_release(blocks[i]);
    for (size_t i = 0; i < sizeof(sides) / sizeof(sides[0]); i++) mars_side_release(sides[i]);
    m->cls_c = m->cls_top_k = m->match_top_k = m->label_pending = m->shot_pending = 0;
    m->seg_max = m->seg_ph = m->seg_pw = m->pose_max = m->pose_k = 0;
    m->segn_max = m->segn_oh = m->segn_ow = 0;
    memset(m->segn_key, 0, sizeof(m->segn_key)); /* (those tables lived inside the block) */
    m->pose_lut.n = m->obb_lut.n = 0; /* (those tables lived inside the blocks) */
    if (m->ev_redact_done) mhip_event_destroy(m->ev_redact_done);
    m->ev_redact_done = NULL;
    free(m->overlay_img); /* (the palette and names it mirrors lived inside the block) */
    m->overlay_img = NULL;
    m->overlay_img_bytes = 0;
}
