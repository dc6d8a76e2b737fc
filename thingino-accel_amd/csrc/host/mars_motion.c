/*
 * mars_motion.c -- host side of the motion maps (include/mars_hip.h, "Motion"): the detector object and its device image (the background
 * grids, the initialised flags, the raw scratch, the result block of the last call), option checks and the zones' cell ranges, the frame ->
 * stream map, the stream ordering of the device forms, the per-detection array hung on a model beside its tracks, and the host-pointer
 * forms.  The kernels are csrc/hip/motion.hip.  The reference has nothing of the kind.  There is no CPU pixel path: without the device
 * every entry point but mars_hip_motion_grid fails once its arguments have passed the checks.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

struct mars_hip_motion {
    int streams, w, h, fmt, cell_log2, gw, gh, pitch;
    size_t frame_bytes;
    uint16_t *bg;        /* device: [streams][gh][gw] */
    int *init;           /* device: [streams] */
    uint8_t *raw;        /* device: [raw_frames][gh][32 * pitch], the scratch between the two launches; grown with the calls */
    int raw_frames;
    mars_block_t res;    /* the last call's [frames][gh][pitch] words, [frames] x mars_motion_stats_t, [frames][n_zones] x int */
    size_t off[3];
    int n_zones;         /* of the last call */
    void *ev_read_done;  /* a detection count (auxiliary stream) has read the maps: the next motion call waits before it rewrites them */
    int read_pending;
};
_Static_assert(sizeof(mars_motion_stats_t) == 24 && sizeof(mars_motion_det_t) == 8, "the records motion.hip writes");
_Static_assert(MARS_MOTION_MAX_ZONES == MHIP_MOTION_MAX_ZONES, "the launch record's zone table");

#define MOTION_FLAGS (MARS_MOTION_STREAM_MAJOR | MARS_MOTION_FRAME_DIFF)

/* cell -> log2, or -1 outside {4, 8, 16, 32, 64}; 0 means 16 */
static int cell_log2(int cell) {
    if (cell == 0) return 4;
    for (int lg = 2; lg <= 6; lg++)
        if (cell == (1 << lg)) return lg;
    return -1;
}

mars_error_t mars_hip_motion_grid(int w, int h, int cell, int *gw, int *gh, int *pitch) {
    const int lg = cell_log2(cell);
    if (w <= 0 || h <= 0 || lg < 0) return MARS_ERR_INVALID_FILE;
    if (w > MHIP_MOTION_MAX_DIM || h > MHIP_MOTION_MAX_DIM) return MARS_ERR_INVALID_TENSOR;
    const int g = ((w - 1) >> lg) + 1;
    if (gw) *gw = g;
    if (gh) *gh = ((h - 1) >> lg) + 1;
    if (pitch) *pitch = (g + 31) / 32;
    return MARS_OK;
}

mars_error_t mars_hip_motion_create(int streams, int w, int h, int format, int cell, mars_hip_motion_t **out) {
    if (!out || streams <= 0) return MARS_ERR_INVALID_FILE;
    if (!mhip_frame_format_ok(format, 0)) return MARS_ERR_INVALID_FILE; /* (nothing is converted: there are no NV12 flags to give) */
    int gw, gh, pitch;
    const mars_error_t e = mars_hip_motion_grid(w, h, cell, &gw, &gh, &pitch);
    if (e != MARS_OK) return e;
    if (!mhip_frame_bytes(w, h, format)) return MARS_ERR_INVALID_FILE; /* an odd NV12 size: the grid call has seen to the rest */
    if (streams > 65535) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_hip_motion_t *m = (mars_hip_motion_t *)calloc(1, sizeof(*m));
    if (!m) return MARS_ERR_ALLOC_FAILED;
    m->streams = streams; m->w = w; m->h = h; m->fmt = format == MARS_HIP_CAMERA_NV12;
    m->cell_log2 = cell_log2(cell); m->gw = gw; m->gh = gh; m->pitch = pitch;
    m->frame_bytes = mhip_frame_bytes(w, h, format);
    m->bg = (uint16_t *)mhip_malloc((size_t)streams * gh * gw * sizeof(uint16_t));
    m->init = (int *)mhip_malloc((size_t)streams * sizeof(int));
    m->ev_read_done = mhip_event_create_sync();
    if (!m->bg || !m->init || !m->ev_read_done || mars_hip_motion_reset(m, -1) != MARS_OK) {
        mars_hip_motion_free(m);
        return MARS_ERR_ALLOC_FAILED;
    }
    *out = m;
    return MARS_OK;
}

mars_error_t mars_hip_motion_reset(mars_hip_motion_t *m, int stream) {
    if (!m) return MARS_ERR_INVALID_FILE;
    if (stream < -1 || stream >= m->streams) return MARS_ERR_INVALID_TENSOR;
    if (!m->bg || !m->init || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t grid = (size_t)m->gh * m->gw, first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? (size_t)m->streams : 1;
    /* behind every motion call enqueued so far.  All zero: not initialised, and a background nobody reads before the first step writes it */
    if (mhip_sync() || mhip_memset_async(m->bg + first * grid, 0, n * grid * sizeof(uint16_t)) || mhip_memset_async(m->init + first, 0, n * sizeof(int)) ||
        mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

void mars_hip_motion_free(mars_hip_motion_t *m) {
    if (!m) return;
    if (mhip_ready()) mhip_sync(); /* a motion call or a detection count may still use the grids and the maps */
    if (m->bg) mhip_free(m->bg);
    if (m->init) mhip_free(m->init);
    if (m->raw) mhip_free(m->raw);
    if (m->ev_read_done) mhip_event_destroy(m->ev_read_done);
    mars_block_release(&m->res);
    free(m);
}

mars_error_t mars_hip_motion_read(mars_hip_motion_t *m, int stream, uint16_t *bg, int *initialised) {
    if (!m) return MARS_ERR_INVALID_FILE;
    if (stream < 0 || stream >= m->streams) return MARS_ERR_INVALID_TENSOR;
    if (!m->bg || !m->init || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t grid = (size_t)m->gh * m->gw;
    int rc = mhip_sync();
    if (!rc && bg) rc = mhip_d2h_async(bg, m->bg + (size_t)stream * grid, grid * sizeof(uint16_t));
    if (!rc && initialised) rc = mhip_d2h_async(initialised, m->init + stream, sizeof(int));
    if (!rc) rc = mhip_sync();
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

/* the checks that need no device, the defaults and the zones' cell ranges resolved into the launch record */
static mars_error_t motion_opts(const mars_hip_motion_t *m, const mars_hip_motion_opts_t *o, int n_frames, mhip_motion_t *p) {
    memset(p, 0, sizeof(*p));
    if (!m || !o || n_frames <= 0) return MARS_ERR_INVALID_FILE;
    if (o->flags & ~MOTION_FLAGS) return MARS_ERR_INVALID_FILE;
    if (o->threshold < 0 || o->threshold > 255 || o->learn < 0 || o->learn > 16 || o->learn_active < 0 || o->learn_active > 16 ||
        o->min_neighbors < 0 || o->min_neighbors > 8 || o->n_zones < 0 || o->n_zones > MARS_MOTION_MAX_ZONES || (o->n_zones > 0 && !o->zones))
        return MARS_ERR_INVALID_FILE;
    for (int z = 0; z < o->n_zones; z++) {
        const mars_tile_t *r = &o->zones[z];
        if (r->x0 < 0 || r->y0 < 0 || r->x1 <= r->x0 || r->y1 <= r->y0 || r->x1 > m->w || r->y1 > m->h) return MARS_ERR_INVALID_FILE;
        p->zones[z][0] = r->x0 >> m->cell_log2; p->zones[z][1] = r->y0 >> m->cell_log2;
        p->zones[z][2] = (r->x1 - 1) >> m->cell_log2; p->zones[z][3] = (r->y1 - 1) >> m->cell_log2;
    }
    if (n_frames % m->streams) return MARS_ERR_INVALID_TENSOR;
    p->n_frames = n_frames; p->streams = m->streams; p->steps = n_frames / m->streams;
    p->stream_major = (o->flags & MARS_MOTION_STREAM_MAJOR) != 0;
    p->frame_diff = (o->flags & MARS_MOTION_FRAME_DIFF) != 0;
    p->w = m->w; p->h = m->h; p->fmt = m->fmt; p->cell_log2 = m->cell_log2; p->gw = m->gw; p->gh = m->gh; p->pitch = m->pitch;
    p->frame_stride = m->frame_bytes;
    p->threshold = o->threshold ? o->threshold : 8;
    p->learn = o->learn ? o->learn : 4;
    p->learn_active = o->learn_active ? o->learn_active : 8;
    p->min_neighbors = o->min_neighbors;
    p->n_zones = o->n_zones;
    p->bg = m->bg; p->init = m->init;
    return MARS_OK;
}

mars_error_t mars_hip_motion_device(mars_hip_motion_t *m, const void *frames_dev, int n_frames, const mars_hip_motion_opts_t *opts) {
    mhip_motion_t p;
    mars_error_t e = motion_opts(m, opts, n_frames, &p);
    if (e != MARS_OK) return e;
    if (!frames_dev) return MARS_ERR_INVALID_FILE;
    if (!m->bg || !m->init || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t grid = (size_t)m->gh * m->pitch * 32;
    if (m->raw_frames < n_frames) { /* (re-allocation: an earlier call may still use the old scratch) */
        if (mhip_sync()) return MARS_ERR_LAYER_FAILED;
        if (m->raw) mhip_free(m->raw);
        m->raw_frames = 0;
        m->raw = (uint8_t *)mhip_malloc((size_t)n_frames * grid);
        if (!m->raw) return MARS_ERR_ALLOC_FAILED;
        m->raw_frames = n_frames;
    }
    const size_t sz[3] = {(size_t)n_frames * m->gh * m->pitch * sizeof(uint32_t), (size_t)n_frames * sizeof(mars_motion_stats_t),
                          (size_t)n_frames * p.n_zones * sizeof(int)};
    if ((e = mars_block_reserve(&m->res, mars_block_layout(sz, 3, m->off), 1, NULL)) != MARS_OK) return e;
    uint8_t *blk = (uint8_t *)m->res.dev;
    p.frames = (const uint8_t *)frames_dev;
    p.raw = m->raw;
    p.maps = (uint32_t *)blk; p.stats = (int *)(blk + m->off[1]); p.zone_counts = p.n_zones ? (int *)(blk + m->off[2]) : NULL;
    m->res.frames = 0;
    /* The main stream, like the front-end: behind whatever the library was given for these frames so far (a redaction enqueued earlier has
     * made this stream wait for it), ahead of what comes later (a redaction enqueued later first waits for this stream).  The maps of the last
     * call may still be read by a detection count on the auxiliary stream: that first */
    mhip_select_stream(0);
    int rc = m->read_pending ? mhip_stream_wait(0, m->ev_read_done) : 0;
    m->read_pending = 0;
    if (!rc) rc = mhip_event_record(m->res.ev[0]);
    if (!rc) rc = mhip_motion_cells(&p);
    if (!rc) rc = mhip_motion_map(&p);
    if (!rc) rc = mhip_event_record(m->res.ev[1]);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->res.frames = n_frames;
    m->n_zones = p.n_zones;
    return MARS_OK;
}

mars_error_t mars_hip_motion_results(mars_hip_motion_t *m, uint32_t *maps, mars_motion_stats_t *stats, int *zone_counts) {
    if (!m) return MARS_ERR_INVALID_FILE;
    const size_t F = (size_t)m->res.frames;
    const mars_block_part_t parts[3] = {{maps, 0, F * m->gh * m->pitch * sizeof(uint32_t)}, {stats, m->off[1], F * sizeof(mars_motion_stats_t)},
                                        {m->n_zones ? zone_counts : NULL, m->off[2], F * m->n_zones * sizeof(int)}};
    return mars_block_fetch(&m->res, parts, 3, NULL);
}

mars_error_t mars_yolo_motion_frames(mars_hip_motion_t *m, const unsigned char *frames, int n_frames, const mars_hip_motion_opts_t *opts,
                                     uint32_t *maps, mars_motion_stats_t *stats, int *zone_counts) {
    mhip_motion_t p;
    mars_error_t e = motion_opts(m, opts, n_frames, &p);
    if (e != MARS_OK) return e;
    if (!frames) return MARS_ERR_INVALID_FILE;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t in_b = m->frame_bytes * (size_t)n_frames;
    uint8_t *d = (uint8_t *)mhip_malloc(in_b);
    if (!d) return MARS_ERR_ALLOC_FAILED;
    mhip_select_stream(0);
    if (mhip_h2d_async(d, frames, in_b)) e = MARS_ERR_LAYER_FAILED;
    if (e == MARS_OK) e = mars_hip_motion_device(m, d, n_frames, opts);
    if (e == MARS_OK) e = mars_hip_motion_results(m, maps, stats, zone_counts); /* waits */
    else (void)mhip_sync(); /* the upload may still be running */
    mhip_free(d);
    return e;
}

float mars_hip_motion_ms(mars_hip_motion_t *m) { return m ? mars_block_ms(&m->res) : -1.0f; }

/* the maps of the last call, as the counting kernel takes them */
static void dets_record(const mars_hip_motion_t *m, float expand, mhip_motion_dets_t *q) {
    memset(q, 0, sizeof(*q));
    q->maps = (const uint32_t *)m->res.dev; q->n_frames = m->res.frames;
    q->gw = m->gw; q->gh = m->gh; q->pitch = m->pitch; q->cell_log2 = m->cell_log2; q->w = m->w; q->h = m->h;
    q->expand = expand != 0 ? expand : 1.0f;
}

mars_error_t mars_hip_motion_detections_device(mars_model_t *det_model, mars_hip_motion_t *m, float expand) {
    if (!det_model || !m || !isfinite(expand) || expand < 0) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model;
    mars_error_t e = mars_stage_guard(det);
    if (e != MARS_OK) return e;
    const int B = det->batch;
    if (!mars_has_dets(det)) return MARS_ERR_INVALID_TENSOR;                                     /* no detections in HBM */
    if (!m->res.dev || m->res.frames <= 0 || m->res.frames != B) return MARS_ERR_INVALID_TENSOR;    /* no motion call, or one over other frames */
    if ((e = mars_side_reserve(&det->motion, B, sizeof(mars_motion_det_t))) != MARS_OK) return e;
    mhip_motion_dets_t q;
    dets_record(m, expand, &q);
    q.dets = det->det_dev; q.counts = det->det_counts_dev; q.det_cap = MARS_YOLO_MAX_DET; q.n_entries = B * MARS_YOLO_MAX_DET;
    q.out = det->motion.dev;
    /* The auxiliary stream, with the label scatter's ordering: it carries the detection tail, so this comes behind the tail that wrote the
     * lists and ahead of det_model's next detect call.  The maps are written on the main stream: the count waits for what that stream has
     * been given so far, and the detector's next motion call waits for the count (ev_read_done) before it rewrites them */
    det->motion.frames = 0;
    mhip_select_stream(0);
    if ((e = mars_aux_behind_current(&det->ev_graph_done)) != MARS_OK) return e;
    int rc = mhip_motion_dets(&q);
    if (!rc) rc = mhip_event_record(m->ev_read_done);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->read_pending = 1;
    det->motion.frames = B;
    return MARS_OK;
}

mars_error_t mars_hip_motion_det_results(mars_model_t *det_model, mars_motion_det_t *out) {
    if (!det_model || !out) return MARS_ERR_INVALID_FILE;
    return mars_side_fetch(&((mars_model_ext_t *)det_model)->motion, out, sizeof(mars_motion_det_t));
}

mars_error_t mars_yolo_motion_boxes(mars_hip_motion_t *m, const mars_det_t *boxes, const int *frame_of_box, int n_boxes, float expand,
                                    mars_motion_det_t *out) {
    if (!m || n_boxes < 0 || (n_boxes > 0 && (!boxes || !frame_of_box || !out)) || !isfinite(expand) || expand < 0) return MARS_ERR_INVALID_FILE;
    if (!m->res.dev || m->res.frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no motion call yet */
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (n_boxes == 0) return MARS_OK;
    const size_t n = (size_t)n_boxes;
    const size_t sz[3] = {n * sizeof(mars_det_t), n * sizeof(int), n * sizeof(mars_motion_det_t)};
    size_t off[3];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 3, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    mhip_motion_dets_t q;
    dets_record(m, expand, &q);
    q.dets = d; q.frame_of = (const int *)(d + off[1]); q.n_entries = n_boxes; q.out = d + off[2];
    mhip_select_stream(0); /* the stream that wrote the maps */
    int rc = mhip_h2d_async(d, boxes, sz[0]);
    if (!rc) rc = mhip_h2d_async(d + off[1], frame_of_box, sz[1]);
    if (!rc) rc = mhip_motion_dets(&q);
    if (!rc) rc = mhip_d2h_async(out, q.out, sz[2]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}
