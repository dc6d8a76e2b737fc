/*
 * mars_shots.c -- host side of the best shots (include/mars_hip.h, "Best shots"): the option checks, the shots object (per stream the slot
 * table, the pixel plane, the step counter and the counters in HBM; the band partials of the last call), the frame -> stream map, the
 * record array hung on the second model beside its ROI table, stream ordering, the launches of csrc/hip/shots.hip, and the hand-over of a
 * finished track's picture as uint8 [th][tw][3].  The reference has nothing of the kind.  There is no CPU path: without the device every
 * entry point fails once its arguments have passed the checks.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

struct mars_hip_shots {
    int streams, slots, tw, th, nhwc;
    size_t crop_bytes, plane_stride; /* tw * th * 3, and that rounded up to 16 */
    void *table;                     /* device: [streams][slots] x mars_shot_slot_t; all zero: a FREE slot */
    mhip_shots_hdr_t *hdr;           /* device: [streams] */
    int8_t *plane;                   /* device: [streams][slots] crops at plane_stride */
    int *last;                       /* device: [streams][slots], the walk's note for the copy */
    mars_block_t res;                /* the last call's band partials [crops][bands][2] x int64 and candidate ids [crops] x int */
};
_Static_assert(sizeof(mars_shot_t) == 24 && sizeof(mars_shot_slot_t) == 72 && sizeof(mars_hip_shot_opts_t) == 32, "the records shots.hip reads and writes");
_Static_assert(sizeof(mhip_shots_hdr_t) == 8 + 8 * MHIP_SHOTS_COUNTERS, "step, pad, then the counters in the order mars_hip_shots_read copies them");
_Static_assert(MARS_TRACK_SLOTS == MHIP_TRACK_SLOTS, "the walk's thread per slot");

#define SHOT_FLAGS (MARS_SHOT_STREAM_MAJOR | MARS_SHOT_KEEP_ASPECT | MARS_SHOT_INSIDE)

/* ---- the parts that need no device */
mars_error_t mars_shots_opts(const mars_hip_shot_opts_t *o, mhip_shots_t *p) {
    if (!o || (o->flags & ~SHOT_FLAGS) || o->max_gap < 0 || o->min_hits < 0 || o->min_sharp < 0 || o->src_w < 0 || o->src_h < 0) return MARS_ERR_INVALID_FILE;
    if (o->min_mean < 0 || o->max_mean > 255 || o->min_mean > o->max_mean) return MARS_ERR_INVALID_FILE;
    if ((o->flags & MARS_SHOT_INSIDE) && (o->src_w <= 0 || o->src_h <= 0)) return MARS_ERR_INVALID_FILE;
    p->max_gap = o->max_gap ? o->max_gap : 30;
    p->min_hits = o->min_hits ? o->min_hits : 1;
    p->min_mean = o->min_mean; p->max_mean = o->max_mean; p->min_sharp = o->min_sharp;
    p->src_w = o->src_w; p->src_h = o->src_h;
    p->stream_major = (o->flags & MARS_SHOT_STREAM_MAJOR) != 0;
    p->keep_aspect = (o->flags & MARS_SHOT_KEEP_ASPECT) != 0;
    p->inside = (o->flags & MARS_SHOT_INSIDE) != 0;
    return MARS_OK;
}

mars_error_t mars_shots_map(int streams, int frames, int *steps) {
    if (streams <= 0 || frames <= 0) return MARS_ERR_INVALID_FILE;
    if (frames % streams) return MARS_ERR_INVALID_TENSOR;
    *steps = frames / streams;
    return MARS_OK;
}

int mars_shots_frame(int streams, int steps, int stream_major, int stream, int step) {
    return stream_major ? stream * steps + step : step * streams + stream;
}

void mars_shots_relayout(const int8_t *src, int tw, int th, int nhwc, unsigned char *rgb) {
    const size_t n = (size_t)tw * th;
    if (nhwc) {
        for (size_t i = 0; i < n * 3; i++) rgb[i] = (unsigned char)(src[i] + 128);
    } else {
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < 3; c++) rgb[i * 3 + c] = (unsigned char)(src[(size_t)c * n + i] + 128);
    }
}

/* ---- the object */
static int shots_up(const mars_hip_shots_t *sh) { return sh->table && sh->hdr && sh->plane && sh->last && mhip_ready(); }
static size_t table_bytes(const mars_hip_shots_t *sh) { return (size_t)sh->slots * sizeof(mars_shot_slot_t); }

mars_error_t mars_hip_shots_create(int streams, int slots, int tw, int th, int nhwc, mars_hip_shots_t **out) {
    if (!out || streams <= 0 || slots <= 0 || tw <= 0 || th <= 0) return MARS_ERR_INVALID_FILE;
    if (streams > 65535 || slots > MARS_TRACK_SLOTS || tw > 1280 || th > 1280) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_hip_shots_t *sh = (mars_hip_shots_t *)calloc(1, sizeof(*sh));
    if (!sh) return MARS_ERR_ALLOC_FAILED;
    sh->streams = streams; sh->slots = slots; sh->tw = tw; sh->th = th; sh->nhwc = nhwc != 0;
    sh->crop_bytes = (size_t)tw * th * 3;
    sh->plane_stride = ALIGN_UP(sh->crop_bytes, 16);
    const size_t all = (size_t)streams * slots;
    sh->table = mhip_malloc(all * sizeof(mars_shot_slot_t));
    sh->hdr = (mhip_shots_hdr_t *)mhip_malloc((size_t)streams * sizeof(mhip_shots_hdr_t));
    sh->plane = (int8_t *)mhip_malloc(all * sh->plane_stride);
    sh->last = (int *)mhip_malloc(all * sizeof(int));
    if (!sh->table || !sh->hdr || !sh->plane || !sh->last || mars_hip_shots_reset(sh, -1) != MARS_OK) {
        mars_hip_shots_free(sh);
        return MARS_ERR_ALLOC_FAILED;
    }
    *out = sh;
    return MARS_OK;
}

void mars_hip_shots_free(mars_hip_shots_t *sh) {
    if (!sh) return;
    if (mhip_ready()) mhip_sync(); /* a shots call may still use the tables */
    if (sh->table) mhip_free(sh->table);
    if (sh->hdr) mhip_free(sh->hdr);
    if (sh->plane) mhip_free(sh->plane);
    if (sh->last) mhip_free(sh->last);
    mars_block_release(&sh->res);
    free(sh);
}

static mars_error_t stream_arg(const mars_hip_shots_t *sh, int stream, int lowest) {
    if (!sh) return MARS_ERR_INVALID_FILE;
    if (stream < lowest || stream >= sh->streams) return MARS_ERR_INVALID_TENSOR;
    return shots_up(sh) ? MARS_OK : MARS_ERR_NNA_INIT_FAILED;
}

mars_error_t mars_hip_shots_reset(mars_hip_shots_t *sh, int stream) {
    const mars_error_t e = stream_arg(sh, stream, -1);
    if (e != MARS_OK) return e;
    const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? (size_t)sh->streams : 1;
    /* behind every shots call enqueued so far, on either stream.  All zero: every slot FREE, step 0, counters 0; the plane's bytes are
     * reachable through a LIVE or DONE slot only */
    if (mhip_sync() || mhip_memset_async((uint8_t *)sh->table + first * table_bytes(sh), 0, n * table_bytes(sh)) ||
        mhip_memset_async(sh->hdr + first, 0, n * sizeof(mhip_shots_hdr_t)) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

/* one stream's table and header to the host (hdr may be NULL); waits */
static mars_error_t fetch_stream(mars_hip_shots_t *sh, int stream, mars_shot_slot_t *tab, mhip_shots_hdr_t *h) {
    if (mhip_sync() || mhip_d2h_async(tab, (uint8_t *)sh->table + (size_t)stream * table_bytes(sh), table_bytes(sh)) ||
        (h && mhip_d2h_async(h, sh->hdr + stream, sizeof(*h))) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    for (int s = 0; s < sh->slots; s++)
        if (tab[s].state == MARS_SHOT_FREE) memset(&tab[s], 0, sizeof(tab[s]));
    return MARS_OK;
}

static mars_error_t store_stream(mars_hip_shots_t *sh, int stream, const mars_shot_slot_t *tab, const mhip_shots_hdr_t *h) {
    if (mhip_h2d_async((uint8_t *)sh->table + (size_t)stream * table_bytes(sh), tab, table_bytes(sh)) ||
        (h && mhip_h2d_async(sh->hdr + stream, h, sizeof(*h))))
        return MARS_ERR_LAYER_FAILED;
    return mhip_sync() ? MARS_ERR_LAYER_FAILED : MARS_OK; /* (the host copies are read until here) */
}

mars_error_t mars_hip_shots_flush(mars_hip_shots_t *sh, int stream) {
    mars_error_t e = stream_arg(sh, stream, -1);
    if (e != MARS_OK) return e;
    mars_shot_slot_t *tab = (mars_shot_slot_t *)malloc(table_bytes(sh));
    if (!tab) return MARS_ERR_ALLOC_FAILED;
    for (int b = stream < 0 ? 0 : stream; e == MARS_OK && b < (stream < 0 ? sh->streams : stream + 1); b++) {
        mhip_shots_hdr_t h;
        if ((e = fetch_stream(sh, b, tab, &h)) != MARS_OK) break;
        int n = 0;
        for (int s = 0; s < sh->slots; s++)
            if (tab[s].state == MARS_SHOT_LIVE) { tab[s].state = MARS_SHOT_DONE; n++; }
        h.cnt[0] += n;
        if (n) e = store_stream(sh, b, tab, &h);
    }
    free(tab);
    return e;
}

mars_error_t mars_hip_shots_read(mars_hip_shots_t *sh, int stream, long long counters[6], int *n_live, int *n_done, int *step) {
    mars_error_t e = stream_arg(sh, stream, 0);
    if (e != MARS_OK) return e;
    mars_shot_slot_t *tab = (mars_shot_slot_t *)malloc(table_bytes(sh));
    if (!tab) return MARS_ERR_ALLOC_FAILED;
    mhip_shots_hdr_t h;
    e = fetch_stream(sh, stream, tab, &h);
    int live = 0, done = 0;
    for (int s = 0; e == MARS_OK && s < sh->slots; s++) { live += tab[s].state == MARS_SHOT_LIVE; done += tab[s].state == MARS_SHOT_DONE; }
    free(tab);
    if (e != MARS_OK) return e;
    if (counters) memcpy(counters, h.cnt, sizeof(h.cnt));
    if (n_live) *n_live = live;
    if (n_done) *n_done = done;
    if (step) *step = h.step;
    return MARS_OK;
}

mars_error_t mars_hip_shots_read_slots(mars_hip_shots_t *sh, int stream, mars_shot_slot_t *slots) {
    if (!slots) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = stream_arg(sh, stream, 0);
    return e != MARS_OK ? e : fetch_stream(sh, stream, slots, NULL);
}

/* the stored crop of one slot -> uint8 [th][tw][3] at rgb, through `tmp` of crop_bytes; the device is idle */
static mars_error_t fetch_pixels(mars_hip_shots_t *sh, int stream, int slot, int8_t *tmp, unsigned char *rgb) {
    if (mhip_d2h_async(tmp, sh->plane + ((size_t)stream * sh->slots + slot) * sh->plane_stride, sh->crop_bytes) || mhip_sync()) return MARS_ERR_LAYER_FAILED;
    mars_shots_relayout(tmp, sh->tw, sh->th, sh->nhwc, rgb);
    return MARS_OK;
}

mars_error_t mars_hip_shots_read_pixels(mars_hip_shots_t *sh, int stream, int slot, unsigned char *rgb) {
    if (!rgb) return MARS_ERR_INVALID_FILE;
    mars_error_t e = stream_arg(sh, stream, 0);
    if (e != MARS_OK) return e;
    if (slot < 0 || slot >= sh->slots) return MARS_ERR_INVALID_TENSOR;
    mars_shot_slot_t *tab = (mars_shot_slot_t *)malloc(table_bytes(sh));
    int8_t *tmp = (int8_t *)malloc(sh->crop_bytes);
    if (!tab || !tmp) e = MARS_ERR_ALLOC_FAILED;
    if (e == MARS_OK) e = fetch_stream(sh, stream, tab, NULL);
    if (e == MARS_OK && tab[slot].state == MARS_SHOT_FREE) e = MARS_ERR_INVALID_TENSOR;
    if (e == MARS_OK) e = fetch_pixels(sh, stream, slot, tmp, rgb);
    free(tab);
    free(tmp);
    return e;
}

mars_error_t mars_hip_shots_collect(mars_hip_shots_t *sh, int stream, mars_shot_slot_t *slots_out, unsigned char *rgb_out, int cap, int *n) {
    if (cap < 0 || (cap > 0 && (!slots_out || !rgb_out))) return MARS_ERR_INVALID_FILE;
    mars_error_t e = stream_arg(sh, stream, 0);
    if (e != MARS_OK) return e;
    mars_shot_slot_t *tab = (mars_shot_slot_t *)malloc(table_bytes(sh));
    int8_t *tmp = (int8_t *)malloc(sh->crop_bytes);
    if (!tab || !tmp) e = MARS_ERR_ALLOC_FAILED;
    if (e == MARS_OK) e = fetch_stream(sh, stream, tab, NULL);
    int done = 0, copied = 0;
    for (int s = 0; e == MARS_OK && s < sh->slots; s++) {
        if (tab[s].state != MARS_SHOT_DONE) continue;
        done++;
        if (copied >= cap) continue;
        if ((e = fetch_pixels(sh, stream, s, tmp, rgb_out + (size_t)copied * sh->crop_bytes)) != MARS_OK) break;
        slots_out[copied++] = tab[s];
        memset(&tab[s], 0, sizeof(tab[s])); /* FREE */
    }
    if (e == MARS_OK && copied) e = store_stream(sh, stream, tab, NULL);
    free(tab);
    free(tmp);
    if (e == MARS_OK && n) *n = done;
    return e;
}

/* ---- the calls */
/* the object's part of the launch record, and room for the band partials and candidate ids of n_crops crops */
static mars_error_t shots_prepare(mhip_shots_t *p, mars_hip_shots_t *sh, int n_crops, int frames) {
    if (n_crops > 65535) return MARS_ERR_INVALID_TENSOR;
    mars_error_t e = mars_shots_map(sh->streams, frames, &p->steps);
    if (e != MARS_OK) return e;
    if (!shots_up(sh)) return MARS_ERR_NNA_INIT_FAILED;
    p->streams = sh->streams; p->slots = sh->slots; p->n_crops = n_crops;
    p->tw = sh->tw; p->th = sh->th; p->nhwc = sh->nhwc;
    p->band_rows = mhip_shots_band_rows(sh->tw);
    p->bands = (sh->th + p->band_rows - 1) / p->band_rows;
    const size_t sz[2] = {(size_t)n_crops * p->bands * 2 * sizeof(long long), (size_t)n_crops * sizeof(int)};
    size_t off[2];
    const size_t total = mars_block_layout(sz, 2, off);
    if ((e = mars_block_reserve(&sh->res, total, 1, NULL)) != MARS_OK) return e;
    sh->res.frames = 0;
    p->partials = (long long *)sh->res.dev;
    p->cand = (int *)((uint8_t *)sh->res.dev + off[1]);
    p->table = sh->table; p->hdr = sh->hdr; p->plane = sh->plane; p->plane_stride = sh->plane_stride; p->last = sh->last;
    return MARS_OK;
}

/* the kernels between the timing events, on the selected stream */
static int shots_launch(mars_hip_shots_t *sh, const mhip_shots_t *p) {
    int rc = mhip_event_record(sh->res.ev[0]);
    if (!rc) rc = mhip_shots(p);
    if (!rc) rc = mhip_event_record(sh->res.ev[1]);
    return rc;
}

mars_error_t mars_yolo_shot_lists(mars_hip_shots_t *sh, const signed char *crops, const mars_roi_t *rois, const float *confs, const int *cls,
                                  const mars_track_t *tracks, int n_crops, int frames, const mars_hip_shot_opts_t *opts, mars_shot_t *records) {
    mhip_shots_t p;
    memset(&p, 0, sizeof(p));
    mars_error_t e = mars_shots_opts(opts, &p);
    if (e != MARS_OK) return e;
    if (!sh || !crops || !rois || !confs || !cls || !tracks || !records || n_crops <= 0 || frames <= 0) return MARS_ERR_INVALID_FILE;
    if ((e = shots_prepare(&p, sh, n_crops, frames)) != MARS_OK) return e;
    const size_t n = (size_t)n_crops;
    /* one scratch block: [crops][rois][confs][cls][tracks][records] */
    const size_t sz[6] = {n * sh->crop_bytes, n * sizeof(mars_roi_t), n * sizeof(float), n * sizeof(int), n * sizeof(mars_track_t), n * sizeof(mars_shot_t)};
    size_t off[6];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 6, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.crops = (const int8_t *)d; p.crop_stride = sh->crop_bytes;
    p.rois = d + off[1]; p.confs = (const float *)(d + off[2]); p.cls = (const int *)(d + off[3]); p.tracks = d + off[4]; p.records = d + off[5];
    /* on the main stream: behind whatever the auxiliary stream still does to these tables, hence the wait first */
    int rc = mhip_sync();
    mhip_select_stream(0);
    if (!rc) rc = mhip_h2d_async(d, crops, sz[0]) || mhip_h2d_async(d + off[1], rois, sz[1]) || mhip_h2d_async(d + off[2], confs, sz[2]) ||
                  mhip_h2d_async(d + off[3], cls, sz[3]) || mhip_h2d_async(d + off[4], tracks, sz[4]);
    if (!rc) rc = shots_launch(sh, &p);
    if (!rc) rc = mhip_d2h_async(records, p.records, sz[5]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    if (rc) return MARS_ERR_LAYER_FAILED;
    sh->res.frames = frames;
    return MARS_OK;
}

mars_error_t mars_hip_shots_device(mars_model_t *det_model, mars_model_t *src_model, int input_index, mars_hip_shots_t *sh,
                                   const mars_hip_shot_opts_t *opts) {
    mhip_shots_t p;
    memset(&p, 0, sizeof(p));
    if (!det_model || !src_model || !sh) return MARS_ERR_INVALID_FILE;
    mars_error_t e = mars_shots_opts(opts, &p);
    if (e != MARS_OK) return e;
    if (det_model == src_model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model, *m = (mars_model_ext_t *)src_model;
    if (!m->act_dev || !det->act_dev || !shots_up(sh)) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe || det->pipe) return MARS_ERR_INVALID_TENSOR;
    mars_pixel_input_t in;
    if (mars_pixel_input(m, input_index, 0, &in) != MARS_OK) return MARS_ERR_INVALID_TENSOR;
    if (in.tw != sh->tw || in.th != sh->th || in.nhwc != sh->nhwc || m->mt[in.tid].pix_stride) return MARS_ERR_INVALID_TENSOR; /* not the object's crops */
    if (!m->roi_dev || m->roi_slots <= 0 || m->roi_slots > m->batch || m->roi_from != det) return MARS_ERR_INVALID_TENSOR; /* no crop call out of det_model */
    if (!mars_has_dets(det)) return MARS_ERR_INVALID_TENSOR;                                                               /* no detections in HBM */
    if (!det->track.dev || det->track.frames <= 0 || det->track.frames != det->batch) return MARS_ERR_INVALID_TENSOR;      /* no track results */
    if (det->batch % sh->streams) return MARS_ERR_INVALID_TENSOR; /* (ahead of the reservations: a refused call leaves everything as it was) */
    if ((e = mars_block_reserve(&m->shot, (size_t)m->roi_slots * sizeof(mars_shot_t), 0, NULL)) != MARS_OK) return e;
    m->shot.frames = 0;
    if ((e = shots_prepare(&p, sh, m->roi_slots, det->batch)) != MARS_OK) return e;
    if (!m->ev_shot_done && !(m->ev_shot_done = mhip_event_create_sync())) return MARS_ERR_ALLOC_FAILED;
    p.crops = in.dev; p.crop_stride = in.stride;
    p.rois = (const uint8_t *)m->roi_dev + 16; p.kept = (const int *)m->roi_dev;
    p.det_cap = MARS_YOLO_MAX_DET; p.dets = det->det_dev; p.tracks = det->track.dev;
    p.records = m->shot.dev;
    /* The auxiliary stream, as the label scatter: it carries every detection tail and every track call, so this comes behind the tracker that
     * wrote the ids and ahead of det_model's next detect call.  The crops and the ROI table are written on the main stream: the kernels wait
     * for what that stream has been given so far, and the next crop call into src_model waits for them (ev_shot_done) */
    mhip_select_stream(0);
    if ((e = mars_aux_behind_current(&m->ev_graph_done)) != MARS_OK) return e;
    int rc = shots_launch(sh, &p);
    if (!rc) rc = mhip_event_record(m->ev_shot_done);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->shot_pending = 1;
    m->shot.frames = m->roi_slots;
    sh->res.frames = det->batch;
    return MARS_OK;
}

mars_error_t mars_hip_shots_results(mars_model_t *src_model, mars_hip_shots_t *sh, mars_shot_t *records) {
    if (!src_model || !sh) return MARS_ERR_INVALID_FILE;
    const mars_block_t *blk = &((mars_model_ext_t *)src_model)->shot;
    if (!blk->dev || blk->frames <= 0 || sh->res.frames <= 0) return MARS_ERR_INVALID_TENSOR; /* nothing pending (on this pair) */
    const mars_block_part_t part = {records, 0, (size_t)blk->frames * sizeof(mars_shot_t)};
    return mars_block_fetch(blk, &part, 1, NULL);
}

mars_error_t mars_hip_shots(mars_model_t *det_model, mars_model_t *src_model, int input_index, mars_hip_shots_t *sh,
                            const mars_hip_shot_opts_t *opts, mars_shot_t *records) {
    if (!det_model || !src_model || !sh || !opts) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_shots_device(det_model, src_model, input_index, sh, opts);
    return e != MARS_OK ? e : mars_hip_shots_results(src_model, sh, records);
}

float mars_hip_shots_ms(mars_hip_shots_t *sh) { return sh ? mars_block_ms(&sh->res) : -1.0f; }
