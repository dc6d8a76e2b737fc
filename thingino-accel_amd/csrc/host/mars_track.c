/*
 * mars_track.c -- host side of the tracking tail (include/mars_hip.h, "Tracking"): argument checks and the options' defaults, the tracker
 * object and its device image, the frame -> stream map, the result array hung on the detector beside its labels and identities, stream
 * ordering, and the launch of csrc/hip/track.hip.  The reference has nothing of the kind.  There is no CPU path: without the device every
 * entry point fails once its arguments have passed the checks.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

struct mars_hip_tracker {
    int streams;            /* first: tests/test_track_cpu.py writes it into the bytes it stands where a tracker would be */
    void *states;           /* device: [streams][MARS_TRACK_SLOTS] x mars_track_state_t; hits == 0: a free slot */
    mhip_track_hdr_t *hdr;  /* device: [streams] */
};
_Static_assert(sizeof(struct mars_hip_tracker) <= 256, "tests/test_track_cpu.py passes 256 bytes as a tracker");
_Static_assert(sizeof(mars_track_t) == 8 && sizeof(mars_track_state_t) == 48, "the records track.hip reads and writes");
_Static_assert(MARS_TRACK_SLOTS == MHIP_TRACK_SLOTS && MARS_TRACK_MAX_CAND == MHIP_TRACK_CAND, "the kernel's table and candidate sizes");

#define TRACK_FLAGS (MARS_TRACK_ANY_CLASS | MARS_TRACK_CARRY_IDENTITY | MARS_TRACK_STREAM_MAJOR)

static int bad_unit(float v) { return !isfinite(v) || v < 0 || v > 1; }

/* the checks that need no device, and the defaults resolved into the launch record */
static mars_error_t track_opts(const mars_hip_track_opts_t *o, mhip_track_t *p) {
    if (!o || (o->flags & ~TRACK_FLAGS)) return MARS_ERR_INVALID_FILE;
    if (bad_unit(o->min_conf) || bad_unit(o->low_conf) || bad_unit(o->iou_thresh) || bad_unit(o->iou_thresh_low)) return MARS_ERR_INVALID_FILE;
    if (o->max_miss < 0 || o->cls_first < 0 || o->cls_count < 0) return MARS_ERR_INVALID_FILE;
    p->min_conf = o->min_conf != 0 ? o->min_conf : 0.5f;
    p->low_conf = o->low_conf;
    if (p->low_conf >= p->min_conf) return MARS_ERR_INVALID_FILE;
    p->iou = o->iou_thresh != 0 ? o->iou_thresh : 0.3f;
    p->iou_low = o->iou_thresh_low != 0 ? o->iou_thresh_low : 0.5f;
    p->max_miss = o->max_miss ? o->max_miss : 30;
    p->cls_first = o->cls_first; p->cls_count = o->cls_count;
    p->any_class = (o->flags & MARS_TRACK_ANY_CLASS) != 0;
    p->stream_major = (o->flags & MARS_TRACK_STREAM_MAJOR) != 0;
    return MARS_OK;
}

mars_error_t mars_hip_tracker_create(int streams, mars_hip_tracker_t **out) {
    if (!out || streams <= 0) return MARS_ERR_INVALID_FILE;
    if (streams > 65535) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_hip_tracker_t *t = (mars_hip_tracker_t *)calloc(1, sizeof(*t));
    if (!t) return MARS_ERR_ALLOC_FAILED;
    t->streams = streams;
    t->states = mhip_malloc((size_t)streams * MARS_TRACK_SLOTS * sizeof(mars_track_state_t));
    t->hdr = (mhip_track_hdr_t *)mhip_malloc((size_t)streams * sizeof(mhip_track_hdr_t));
    if (!t->states || !t->hdr || mars_hip_tracker_reset(t) != MARS_OK) {
        mars_hip_tracker_free(t);
        return MARS_ERR_ALLOC_FAILED;
    }
    *out = t;
    return MARS_OK;
}

mars_error_t mars_hip_tracker_reset(mars_hip_tracker_t *t) {
    if (!t) return MARS_ERR_INVALID_FILE;
    if (!t->states || !t->hdr || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    /* behind every track call enqueued so far, on either stream.  All zero: every slot free (hits == 0), no id given yet, counters 0 */
    if (mhip_sync() || mhip_memset_async(t->states, 0, (size_t)t->streams * MARS_TRACK_SLOTS * sizeof(mars_track_state_t)) ||
        mhip_memset_async(t->hdr, 0, (size_t)t->streams * sizeof(mhip_track_hdr_t)) || mhip_sync())
        return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}

void mars_hip_tracker_free(mars_hip_tracker_t *t) {
    if (!t) return;
    if (mhip_ready()) mhip_sync(); /* a track call may still use the tables */
    if (t->states) mhip_free(t->states);
    if (t->hdr) mhip_free(t->hdr);
    free(t);
}

mars_error_t mars_hip_tracker_read(mars_hip_tracker_t *t, int stream, mars_track_state_t *states, int cap, int *n_live, long long counters[4]) {
    if (!t || cap < 0 || (cap > 0 && !states)) return MARS_ERR_INVALID_FILE;
    if (stream < 0 || stream >= t->streams) return MARS_ERR_INVALID_TENSOR;
    if (!t->states || !t->hdr || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_track_state_t *all = (mars_track_state_t *)malloc(MARS_TRACK_SLOTS * sizeof(*all));
    if (!all) return MARS_ERR_ALLOC_FAILED;
    mhip_track_hdr_t h;
    if (mhip_sync() || mhip_d2h_async(all, (uint8_t *)t->states + (size_t)stream * MARS_TRACK_SLOTS * sizeof(*all), MARS_TRACK_SLOTS * sizeof(*all)) ||
        mhip_d2h_async(&h, t->hdr + stream, sizeof(h)) || mhip_sync()) {
        free(all);
        return MARS_ERR_LAYER_FAILED;
    }
    int n = 0;
    for (int s = 0; s < MARS_TRACK_SLOTS; s++) {
        if (all[s].hits <= 0) continue;
        if (n < cap) states[n] = all[s];
        n++;
    }
    free(all);
    if (n_live) *n_live = n;
    if (counters) memcpy(counters, h.counters, sizeof(h.counters));
    return MARS_OK;
}

/* frames of a call over a tracker of S streams -> the launch record's streams and steps */
static mars_error_t track_map(mhip_track_t *p, const mars_hip_tracker_t *t, int frames) {
    if (t->streams <= 0 || frames % t->streams) return MARS_ERR_INVALID_TENSOR;
    p->streams = t->streams;
    p->steps = frames / t->streams;
    p->states = t->states;
    p->hdr = t->hdr;
    return MARS_OK;
}

mars_error_t mars_yolo_track_lists(mars_hip_tracker_t *t, const mars_det_t *dets, const int *counts, const mars_cls_t *idents, int frames,
                                   int max_det, const mars_hip_track_opts_t *opts, mars_track_t *out) {
    mhip_track_t p;
    memset(&p, 0, sizeof(p));
    mars_error_t e = track_opts(opts, &p);
    if (e != MARS_OK) return e;
    if (!t || !dets || !counts || !out || frames <= 0 || max_det <= 0) return MARS_ERR_INVALID_FILE;
    if ((opts->flags & MARS_TRACK_CARRY_IDENTITY) && !idents) return MARS_ERR_INVALID_FILE;
    if (max_det > MARS_YOLO_MAX_DET) return MARS_ERR_INVALID_TENSOR;
    if ((e = track_map(&p, t, frames)) != MARS_OK) return e;
    if (!t->states || !t->hdr || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t n = (size_t)frames * max_det;
    const int carry = (opts->flags & MARS_TRACK_CARRY_IDENTITY) != 0;
    /* one scratch block: [dets][counts][tracks][identities, where they are carried] */
    const size_t sz[4] = {n * sizeof(mars_det_t), (size_t)frames * sizeof(int), n * sizeof(mars_track_t), carry ? n * sizeof(mars_cls_t) : 0};
    size_t off[4];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 4, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.max_det = max_det;
    p.dets = d;
    p.counts = (const int *)(d + off[1]);
    p.out = d + off[2];
    p.idents = carry ? d + off[3] : NULL;
    /* on the main stream: behind whatever the auxiliary stream still does to this tracker's tables, hence the wait first */
    int rc = mhip_sync();
    if (!rc) rc = mhip_h2d_async(d, dets, sz[0]) || mhip_h2d_async(d + off[1], counts, sz[1]);
    if (!rc && carry) rc = mhip_h2d_async(d + off[3], idents, sz[3]);
    if (!rc) rc = mhip_track(&p);
    if (!rc) rc = mhip_d2h_async(out, p.out, sz[2]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_hip_track_device(mars_model_t *det_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts) {
    mhip_track_t p;
    memset(&p, 0, sizeof(p));
    if (!det_model || !t) return MARS_ERR_INVALID_FILE;
    mars_error_t e = track_opts(opts, &p);
    if (e != MARS_OK) return e;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model;
    if (!det->act_dev || !t->states || !t->hdr || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (det->pipe) return MARS_ERR_INVALID_TENSOR;
    if (!det->det_dev || !det->det_counts_dev || det->det_cap < det->batch) return MARS_ERR_INVALID_TENSOR; /* no detections in HBM */
    const int carry = (opts->flags & MARS_TRACK_CARRY_IDENTITY) != 0;
    if (carry && (!det->ident.dev || det->ident.frames < det->batch)) return MARS_ERR_INVALID_TENSOR;      /* no identity scatter */
    if ((e = track_map(&p, t, det->batch)) != MARS_OK) return e;
    if ((e = mars_side_reserve(&det->track, det->batch, sizeof(mars_track_t))) != MARS_OK) return e;
    p.max_det = MARS_YOLO_MAX_DET;
    p.dets = det->det_dev;
    p.counts = det->det_counts_dev;
    p.idents = carry ? det->ident.dev : NULL;
    p.out = det->track.dev;
    /* The auxiliary stream, as the label scatter: it carries every detection tail and every scatter, so this comes behind the tail that
     * wrote the lists and the scatter that wrote the identities, and ahead of det_model's next detect call.  Nothing on the main stream
     * reads or writes what the kernel touches, so nothing there waits for it */
    det->track.frames = 0;
    mhip_select_aux(1);
    const int rc = mhip_track(&p);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    det->track.frames = det->batch;
    return MARS_OK;
}

mars_error_t mars_hip_track_results(mars_model_t *det_model, mars_track_t *tracks) {
    if (!det_model || !tracks) return MARS_ERR_INVALID_FILE;
    return mars_side_fetch(&((mars_model_ext_t *)det_model)->track, tracks, sizeof(mars_track_t));
}

mars_error_t mars_hip_track(mars_model_t *det_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts, mars_track_t *tracks) {
    if (!det_model || !t || !opts || !tracks) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_track_device(det_model, t, opts);
    return e != MARS_OK ? e : mars_hip_track_results(det_model, tracks);
}
