/*
 * mars_events.c -- host side of the events stage (include/mars_hip.h, "Events"): the rule checks and the rules' device image, the events
 * object (per stream the rules, the slot table, the step counter and the totals in HBM; the per-frame counts of the last call), the
 * frame -> stream map, the record array hung on the detector beside its tracks, stream ordering, and the launch of csrc/hip/events.hip.
 * The reference has nothing of the kind.  There is no CPU path: without the device every entry point fails once its arguments have passed
 * the checks.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

struct mars_hip_events {
    int streams;              /* first: tests/test_events_cpu.py writes it into the bytes it stands where an events object would be */
    void *slots;              /* device: [streams][MARS_TRACK_SLOTS] x mars_event_slot_t; id == 0: a free slot */
    mhip_events_hdr_t *hdr;   /* device: [streams] */
    mhip_event_rules_t *rules; /* device: [streams] */
    mars_block_t res;         /* the last call's [frames][MARS_EVENTS_MAX_LINES][2] and [frames][MARS_EVENTS_MAX_ZONES][4] ints */
    size_t off[2];
};
_Static_assert(sizeof(struct mars_hip_events) <= 256, "tests/test_events_cpu.py passes 256 bytes as an events object");
_Static_assert(sizeof(mars_event_t) == 24 && sizeof(mars_event_slot_t) == 152, "the records events.hip reads and writes");
_Static_assert(MARS_EVENTS_MAX_LINES == MHIP_EVENTS_LINES && MARS_EVENTS_MAX_ZONES == MHIP_EVENTS_ZONES && MARS_EVENTS_MAX_VERTS == MHIP_EVENTS_VERTS,
               "the kernel's rule table");
_Static_assert(sizeof(mhip_events_hdr_t) == 8 + 8 * MHIP_EVENTS_TOTALS, "step, pad, then the totals in the order mars_hip_events_read copies them");

#define EVENTS_FLAGS (MARS_EVENTS_STREAM_MAJOR | MARS_EVENTS_ANCHOR_BOTTOM)
#define LINE_INTS (MARS_EVENTS_MAX_LINES * 2)
#define ZONE_INTS (MARS_EVENTS_MAX_ZONES * 4)

static int bad_coord(int v) { return v < -32768 || v > 32768; }

/* the checks that need no device, and the defaults resolved into the launch record */
static mars_error_t events_opts(const mars_hip_events_opts_t *o, mhip_events_t *p) {
    if (!o || (o->flags & ~EVENTS_FLAGS) || o->max_gap < 0 || o->min_hits < 0) return MARS_ERR_INVALID_FILE;
    p->max_gap = o->max_gap ? o->max_gap : 30;
    p->min_hits = o->min_hits ? o->min_hits : 1;
    p->stream_major = (o->flags & MARS_EVENTS_STREAM_MAJOR) != 0;
    p->anchor_bottom = (o->flags & MARS_EVENTS_ANCHOR_BOTTOM) != 0;
    return MARS_OK;
}

/* the rules' checks, and (img != NULL) their device image: every coordinate times 16 */
static mars_error_t events_rules(const mars_hip_event_rules_t *r, mhip_event_rules_t *img) {
    if (!r || r->n_lines < 0 || r->n_lines > MARS_EVENTS_MAX_LINES || r->n_zones < 0 || r->n_zones > MARS_EVENTS_MAX_ZONES) return MARS_ERR_INVALID_FILE;
    for (int l = 0; l < r->n_lines; l++) {
        const mars_event_line_t *s = &r->lines[l];
        if (bad_coord(s->ax) || bad_coord(s->ay) || bad_coord(s->bx) || bad_coord(s->by) || (s->ax == s->bx && s->ay == s->by)) return MARS_ERR_INVALID_FILE;
    }
    for (int z = 0; z < r->n_zones; z++) {
        const mars_event_zone_t *s = &r->zones[z];
        if (s->n < 3 || s->n > MARS_EVENTS_MAX_VERTS || s->dwell < 0) return MARS_ERR_INVALID_FILE;
        for (int v = 0; v < s->n; v++)
            if (bad_coord(s->x[v]) || bad_coord(s->y[v])) return MARS_ERR_INVALID_FILE;
    }
    if (!img) return MARS_OK;
    memset(img, 0, sizeof(*img));
    img->n_lines = r->n_lines; img->n_zones = r->n_zones;
    for (int l = 0; l < r->n_lines; l++) {
        img->lines[l][0] = r->lines[l].ax * 16; img->lines[l][1] = r->lines[l].ay * 16;
        img->lines[l][2] = r->lines[l].bx * 16; img->lines[l][3] = r->lines[l].by * 16;
    }
    for (int z = 0; z < r->n_zones; z++) {
        img->zones[z].n = r->zones[z].n; img->zones[z].dwell = r->zones[z].dwell;
        for (int v = 0; v < r->zones[z].n; v++) { img->zones[z].x[v] = r->zones[z].x[v] * 16; img->zones[z].y[v] = r->zones[z].y[v] * 16; }
    }
    return MARS_OK;
}

static int events_up(const mars_hip_events_t *ev) { return ev->slots && ev->hdr && ev->rules && mhip_ready(); }

/* the tables and headers of streams [first, first + n) cleared, on the selected stream; the rules stay */
static int events_clear(mars_hip_events_t *ev, size_t first, size_t n) {
    return mhip_memset_async((uint8_t *)ev->slots + first * MARS_TRACK_SLOTS * sizeof(mars_event_slot_t), 0, n * MARS_TRACK_SLOTS * sizeof(mars_event_slot_t)) ||
           mhip_memset_async(ev->hdr + first, 0, n * sizeof(mhip_events_hdr_t));
}

mars_error_t mars_hip_events_create(int streams, mars_hip_events_t **out) {
    if (!out || streams <= 0) return MARS_ERR_INVALID_FILE;
    if (streams > 65535) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_hip_events_t *ev = (mars_hip_events_t *)calloc(1, sizeof(*ev));
    if (!ev) return MARS_ERR_ALLOC_FAILED;
    ev->streams = streams;
    ev->slots = mhip_malloc((size_t)streams * MARS_TRACK_SLOTS * sizeof(mars_event_slot_t));
    ev->hdr = (mhip_events_hdr_t *)mhip_malloc((size_t)streams * sizeof(mhip_events_hdr_t));
    ev->rules = (mhip_event_rules_t *)mhip_malloc((size_t)streams * sizeof(mhip_event_rules_t));
    /* no rules: no line and no zone on any stream */
    if (!ev->slots || !ev->hdr || !ev->rules || mhip_sync() || mhip_memset_async(ev->rules, 0, (size_t)streams * sizeof(mhip_event_rules_t)) ||
        mars_hip_events_reset(ev, -1) != MARS_OK) {
        mars_hip_events_free(ev);
        return MARS_ERR_ALLOC_FAILED;
    }
    *out = ev;
    return MARS_OK;
}

void mars_hip_events_free(mars_hip_events_t *ev) {
    if (!ev) return;
    if (mhip_ready()) mhip_sync(); /* an events call may still use the tables */
    if (ev->slots) mhip_free(ev->slots);
    if (ev->hdr) mhip_free(ev->hdr);
    if (ev->rules) mhip_free(ev->rules);
    mars_block_release(&ev->res);
    free(ev);
}

mars_error_t mars_hip_events_reset(mars_hip_events_t *ev, int stream) {
    if (!ev) return MARS_ERR_INVALID_FILE;
    if (stream < -1 || stream >= ev->streams) return MARS_ERR_INVALID_TENSOR;
    if (!events_up(ev)) return MARS_ERR_NNA_INIT_FAILED;
    /* behind every events call enqueued so far, on either stream.  All zero: every slot free (id == 0), step 0, totals 0 */
    if (mhip_sync() || events_clear(ev, stream < 0 ? 0 : (size_t)stream, stream < 0 ? (size_t)ev->streams : 1) || mhip_sync()) return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

mars_error_t mars_hip_events_set_rules(mars_hip_events_t *ev, int stream, const mars_hip_event_rules_t *rules) {
    mhip_event_rules_t *img = (mhip_event_rules_t *)malloc(sizeof(*img)); /* (2.8 KB: not on the stack of a camera thread) */
    if (!img) return MARS_ERR_ALLOC_FAILED;
    mars_error_t e = !ev ? MARS_ERR_INVALID_FILE : events_rules(rules, img);
    if (e == MARS_OK && (stream < -1 || stream >= ev->streams)) e = MARS_ERR_INVALID_TENSOR;
    if (e == MARS_OK && !events_up(ev)) e = MARS_ERR_NNA_INIT_FAILED;
    if (e == MARS_OK) {
        const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? (size_t)ev->streams : 1;
        int rc = mhip_sync();
        for (size_t s = first; !rc && s < first + n; s++) rc = mhip_h2d_async(ev->rules + s, img, sizeof(*img));
        if (!rc) rc = events_clear(ev, first, n);
        if (mhip_sync() || rc) e = MARS_ERR_LAYER_FAILED; /* (the image is read until here) */
    }
    free(img);
    return e;
}

/* the stream's table, canonical: a free slot all zero, since[z] zero for a zone the slot is not inside */
static mars_error_t events_fetch_slots(mars_hip_events_t *ev, int stream, mars_event_slot_t *all, mhip_events_hdr_t *h) {
    if (mhip_sync() || mhip_d2h_async(all, (uint8_t *)ev->slots + (size_t)stream * MARS_TRACK_SLOTS * sizeof(*all), MARS_TRACK_SLOTS * sizeof(*all)) ||
        (h && mhip_d2h_async(h, ev->hdr + stream, sizeof(*h))) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    for (int s = 0; s < MARS_TRACK_SLOTS; s++) {
        if (all[s].id == 0) memset(&all[s], 0, sizeof(all[s]));
        for (int z = 0; z < MARS_EVENTS_MAX_ZONES; z++)
            if (!((all[s].inside >> z) & 1u)) all[s].since[z] = 0;
    }
    return MARS_OK;
}

mars_error_t mars_hip_events_read(mars_hip_events_t *ev, int stream, long long line_totals[MARS_EVENTS_MAX_LINES][2],
                                  long long zone_totals[MARS_EVENTS_MAX_ZONES][4], long long counters[5], int *n_used, int *step) {
    if (!ev) return MARS_ERR_INVALID_FILE;
    if (stream < 0 || stream >= ev->streams) return MARS_ERR_INVALID_TENSOR;
    if (!events_up(ev)) return MARS_ERR_NNA_INIT_FAILED;
    mars_event_slot_t *all = (mars_event_slot_t *)malloc(MARS_TRACK_SLOTS * sizeof(*all));
    if (!all) return MARS_ERR_ALLOC_FAILED;
    mhip_events_hdr_t h;
    const mars_error_t e = events_fetch_slots(ev, stream, all, &h);
    int n = 0;
    for (int s = 0; e == MARS_OK && s < MARS_TRACK_SLOTS; s++) n += all[s].id != 0;
    free(all);
    if (e != MARS_OK) return e;
    if (line_totals) memcpy(line_totals, h.tot, LINE_INTS * sizeof(long long));
    if (zone_totals) memcpy(zone_totals, h.tot + LINE_INTS, ZONE_INTS * sizeof(long long));
    if (counters) memcpy(counters, h.tot + LINE_INTS + ZONE_INTS, 5 * sizeof(long long));
    if (n_used) *n_used = n;
    if (step) *step = h.step;
    return MARS_OK;
}

mars_error_t mars_hip_events_read_slots(mars_hip_events_t *ev, int stream, mars_event_slot_t *slots) {
    if (!ev || !slots) return MARS_ERR_INVALID_FILE;
    if (stream < 0 || stream >= ev->streams) return MARS_ERR_INVALID_TENSOR;
    if (!events_up(ev)) return MARS_ERR_NNA_INIT_FAILED;
    return events_fetch_slots(ev, stream, slots, NULL);
}

/* frames of a call over S streams -> the launch record's streams, steps and tables, and room for the per-frame counts */
static mars_error_t events_map(mhip_events_t *p, mars_hip_events_t *ev, int frames) {
    if (ev->streams <= 0 || frames % ev->streams) return MARS_ERR_INVALID_TENSOR;
    if (!events_up(ev)) return MARS_ERR_NNA_INIT_FAILED;
    const size_t sz[2] = {(size_t)frames * LINE_INTS * sizeof(int), (size_t)frames * ZONE_INTS * sizeof(int)};
    size_t off[2];
    const size_t total = mars_block_layout(sz, 2, off);
    const mars_error_t e = mars_block_reserve(&ev->res, total, 1, NULL);
    if (e != MARS_OK) return e;
    ev->res.frames = 0; /* (from here on the block's layout is this call's) */
    ev->off[0] = off[0]; ev->off[1] = off[1];
    p->streams = ev->streams;
    p->steps = frames / ev->streams;
    p->slots = ev->slots; p->hdr = ev->hdr; p->rules = ev->rules;
    p->line_counts = (int *)ev->res.dev;
    p->zone_counts = (int *)((uint8_t *)ev->res.dev + ev->off[1]);
    return MARS_OK;
}

/* the kernel between the timing events, on the selected stream */
static int events_launch(mars_hip_events_t *ev, const mhip_events_t *p) {
    int rc = mhip_event_record(ev->res.ev[0]);
    if (!rc) rc = mhip_events(p);
    if (!rc) rc = mhip_event_record(ev->res.ev[1]);
    return rc;
}

mars_error_t mars_yolo_event_lists(mars_hip_events_t *ev, const mars_det_t *dets, const mars_track_t *tracks, const int *counts, int frames, int max_det,
                                   const mars_hip_events_opts_t *opts, mars_event_t *records, int *line_counts, int *zone_counts) {
    mhip_events_t p;
    memset(&p, 0, sizeof(p));
    mars_error_t e = events_opts(opts, &p);
    if (e != MARS_OK) return e;
    if (!ev || !dets || !tracks || !counts || !records || frames <= 0 || max_det <= 0) return MARS_ERR_INVALID_FILE;
    if (max_det > MARS_YOLO_MAX_DET) return MARS_ERR_INVALID_TENSOR;
    if ((e = events_map(&p, ev, frames)) != MARS_OK) return e;
    const size_t n = (size_t)frames * max_det;
    /* one scratch block: [dets][tracks][counts][records] */
    const size_t sz[4] = {n * sizeof(mars_det_t), n * sizeof(mars_track_t), (size_t)frames * sizeof(int), n * sizeof(mars_event_t)};
    size_t off[4];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 4, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.max_det = max_det;
    p.dets = d; p.tracks = d + off[1]; p.counts = (const int *)(d + off[2]); p.records = d + off[3];
    /* on the main stream: behind whatever the auxiliary stream still does to these tables, hence the wait first */
    int rc = mhip_sync();
    mhip_select_stream(0);
    if (!rc) rc = mhip_h2d_async(d, dets, sz[0]) || mhip_h2d_async(d + off[1], tracks, sz[1]) || mhip_h2d_async(d + off[2], counts, sz[2]);
    if (!rc) rc = events_launch(ev, &p);
    if (!rc) rc = mhip_d2h_async(records, p.records, sz[3]);
    if (!rc && line_counts) rc = mhip_d2h_async(line_counts, p.line_counts, (size_t)frames * LINE_INTS * sizeof(int));
    if (!rc && zone_counts) rc = mhip_d2h_async(zone_counts, p.zone_counts, (size_t)frames * ZONE_INTS * sizeof(int));
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    if (rc) return MARS_ERR_LAYER_FAILED;
    ev->res.frames = frames;
    return MARS_OK;
}

mars_error_t mars_hip_events_device(mars_model_t *det_model, mars_hip_events_t *ev, const mars_hip_events_opts_t *opts) {
    mhip_events_t p;
    memset(&p, 0, sizeof(p));
    if (!det_model || !ev) return MARS_ERR_INVALID_FILE;
    mars_error_t e = events_opts(opts, &p);
    if (e != MARS_OK) return e;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model;
    if (!det->act_dev || !events_up(ev)) return MARS_ERR_NNA_INIT_FAILED;
    if (det->pipe) return MARS_ERR_INVALID_TENSOR;
    if (!mars_has_dets(det)) return MARS_ERR_INVALID_TENSOR;                                          /* no detections in HBM */
    if (!det->track.dev || det->track.frames <= 0 || det->track.frames != det->batch) return MARS_ERR_INVALID_TENSOR; /* no track results */
    if (det->batch % ev->streams) return MARS_ERR_INVALID_TENSOR; /* (ahead of the reservations: a refused call leaves everything as it was) */
    if ((e = mars_side_reserve(&det->event, det->batch, sizeof(mars_event_t))) != MARS_OK) return e;
    det->event.frames = 0;
    if ((e = events_map(&p, ev, det->batch)) != MARS_OK) return e;
    p.max_det = MARS_YOLO_MAX_DET;
    p.dets = det->det_dev; p.tracks = det->track.dev; p.counts = det->det_counts_dev; p.records = det->event.dev;
    /* The auxiliary stream, as the label scatter: it carries every detection tail and every track call, so this comes behind the tracker that
     * wrote the ids and ahead of det_model's next detect call.  Nothing on the main stream reads or writes what the kernel touches */
    mhip_select_aux(1);
    const int rc = events_launch(ev, &p);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    det->event.frames = det->batch;
    ev->res.frames = det->batch;
    return MARS_OK;
}

mars_error_t mars_hip_events_results(mars_model_t *det_model, mars_hip_events_t *ev, mars_event_t *records, int *line_counts, int *zone_counts) {
    if (!det_model || !ev) return MARS_ERR_INVALID_FILE;
    const mars_det_side_t *side = &((mars_model_ext_t *)det_model)->event;
    if (!side->dev || side->frames <= 0 || ev->res.frames != side->frames) return MARS_ERR_INVALID_TENSOR; /* nothing pending (on this pair) */
    const size_t F = (size_t)side->frames;
    const mars_block_part_t parts[2] = {{line_counts, 0, F * LINE_INTS * sizeof(int)}, {zone_counts, ev->off[1], F * ZONE_INTS * sizeof(int)}};
    const mars_error_t e = mars_block_fetch(&ev->res, parts, 2, NULL);
    if (e != MARS_OK || !records) return e;
    return mars_side_fetch(side, records, sizeof(mars_event_t));
}

mars_error_t mars_hip_events(mars_model_t *det_model, mars_hip_events_t *ev, const mars_hip_events_opts_t *opts, mars_event_t *records, int *line_counts,
                             int *zone_counts) {
    if (!det_model || !ev || !opts) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_events_device(det_model, ev, opts);
    return e != MARS_OK ? e : mars_hip_events_results(det_model, ev, records, line_counts, zone_counts);
}

float mars_hip_events_ms(mars_hip_events_t *ev) { return ev ? mars_block_ms(&ev->res) : -1.0f; }
