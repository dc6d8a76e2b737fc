/*
 * mars_track.c -- host side of the tracking tail (include/mars_hip.h, "Tracking"): argument checks and the options' defaults, the tracker
 * object and its device image, the frame -> stream map, the result array hung on the detector beside its labels and identities, stream
 * ordering, and the launch of csrc/hip/track.hip; and of "Appearance in tracking": the embedding plane, the two host restatements, the
 * join of the classify sums with the ROI table, and the launches of csrc/hip/track_app.hip.  The reference has nothing of the kind.  There
 * is no CPU path: without the device every entry point but mars_yolo_track_cosine and mars_yolo_embed_blend fails once its arguments have
 * passed the checks.
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
    /* "Appearance in tracking": behind the fields above, all zero on a tracker without an embedding plane (mars_hip_tracker_create) */
    int channels, cp;       /* C, and C rounded up to a multiple of 64 */
    int8_t *plane;          /* device: [streams][MARS_TRACK_SLOTS][cp], pad channels and slots without an embedding zero */
    int *plane_ee;          /* device: [streams][MARS_TRACK_SLOTS]; 0: none */
    float *cosm;            /* device: the cosine scratch of one launch, from the first call that brings vectors on */
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

/* channels == 0: no embedding plane */
static mars_error_t tracker_new(int streams, int channels, mars_hip_tracker_t **out) {
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_hip_tracker_t *t = (mars_hip_tracker_t *)calloc(1, sizeof(*t));
    if (!t) return MARS_ERR_ALLOC_FAILED;
    t->streams = streams;
    t->states = mhip_malloc((size_t)streams * MARS_TRACK_SLOTS * sizeof(mars_track_state_t));
    t->hdr = (mhip_track_hdr_t *)mhip_malloc((size_t)streams * sizeof(mhip_track_hdr_t));
    int bad = !t->states || !t->hdr;
    if (!bad && channels) {
        t->channels = channels;
        t->cp = (channels + 63) & ~63;
        t->plane = (int8_t *)mhip_malloc((size_t)streams * MARS_TRACK_SLOTS * t->cp);
        t->plane_ee = (int *)mhip_malloc((size_t)streams * MARS_TRACK_SLOTS * sizeof(int));
        bad = !t->plane || !t->plane_ee;
    }
    if (bad || mars_hip_tracker_reset(t) != MARS_OK) {
        mars_hip_tracker_free(t);
        return MARS_ERR_ALLOC_FAILED;
    }
    *out = t;
    return MARS_OK;
}

mars_error_t mars_hip_tracker_create(int streams, mars_hip_tracker_t **out) {
    if (!out || streams <= 0) return MARS_ERR_INVALID_FILE;
    if (streams > 65535) return MARS_ERR_INVALID_TENSOR;
    return tracker_new(streams, 0, out);
}

mars_error_t mars_hip_tracker_create_app(int streams, int channels, mars_hip_tracker_t **out) {
    if (!out || streams <= 0 || channels <= 0) return MARS_ERR_INVALID_FILE;
    if (streams > 65535 || channels > MHIP_TRACK_APP_MAX_C) return MARS_ERR_INVALID_TENSOR;
    return tracker_new(streams, channels, out);
}

mars_error_t mars_hip_tracker_reset(mars_hip_tracker_t *t) {
    if (!t) return MARS_ERR_INVALID_FILE;
    if (!t->states || !t->hdr || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    /* behind every track call enqueued so far, on either stream.  All zero: every slot free (hits == 0), no id given yet, counters 0 */
    if (mhip_sync() || mhip_memset_async(t->states, 0, (size_t)t->streams * MARS_TRACK_SLOTS * sizeof(mars_track_state_t)) ||
        mhip_memset_async(t->hdr, 0, (size_t)t->streams * sizeof(mhip_track_hdr_t)))
        return MARS_ERR_LAYER_FAILED;
    /* ... and no slot holds an embedding */
    if (t->plane && (mhip_memset_async(t->plane, 0, (size_t)t->streams * MARS_TRACK_SLOTS * t->cp) ||
                     mhip_memset_async(t->plane_ee, 0, (size_t)t->streams * MARS_TRACK_SLOTS * sizeof(int))))
        return MARS_ERR_LAYER_FAILED;
    return mhip_sync() ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

void mars_hip_tracker_free(mars_hip_tracker_t *t) {
    if (!t) return;
    if (mhip_ready()) mhip_sync(); /* a track call may still use the tables */
    if (t->states) mhip_free(t->states);
    if (t->hdr) mhip_free(t->hdr);
    if (t->plane) mhip_free(t->plane);
    if (t->plane_ee) mhip_free(t->plane_ee);
    if (t->cosm) mhip_free(t->cosm);
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

/* ---- "Appearance in tracking" */
static mars_error_t track_app_opts(const mars_hip_track_app_opts_t *a, mhip_track_app_t *p) {
    if (!a || (a->flags & ~MARS_TRACK_APP_SMOOTH)) return MARS_ERR_INVALID_FILE;
    if (bad_unit(a->app_thresh) || bad_unit(a->app_min_iou)) return MARS_ERR_INVALID_FILE;
    p->app_thresh = a->app_thresh != 0 ? a->app_thresh : 0.75f;
    p->app_min_iou = a->app_min_iou != 0 ? a->app_min_iou : 0.1f;
    p->smooth = (a->flags & MARS_TRACK_APP_SMOOTH) != 0;
    return MARS_OK;
}

static void track_app_plane(mhip_track_app_t *a, const mars_hip_tracker_t *t) {
    a->c = t->channels; a->cp = t->cp;
    a->plane = t->plane; a->plane_ee = t->plane_ee;
}

/* the cosine scratch of one launch, allocated by the first call that brings vectors */
static mars_error_t track_app_scratch(mars_hip_tracker_t *t, mhip_track_app_t *a) {
    if (!t->cosm) {
        const size_t streams = t->streams < MHIP_TRACK_APP_CHUNK ? (size_t)t->streams : MHIP_TRACK_APP_CHUNK;
        t->cosm = (float *)mhip_malloc(streams * MHIP_TRACK_APP_COS_FLOATS * sizeof(float));
        if (!t->cosm) return MARS_ERR_ALLOC_FAILED;
    }
    a->cosm = t->cosm;
    return MARS_OK;
}

/* The plain rule on this tracker: track.hip's kernel where it has no plane, and where it has one the appearance kernel with no embedding
 * supplied, so that deaths clear their rows */
static int track_launch(const mars_hip_tracker_t *t, const mhip_track_t *p) {
    if (!t->plane) return mhip_track(p);
    mhip_track_app_t a;
    memset(&a, 0, sizeof(a));
    a.t = *p;
    track_app_plane(&a, t);
    a.app_thresh = 0.75f; a.app_min_iou = 0.1f; /* (never looked at: no pair has two embeddings) */
    return mhip_track_app(&a);
}

mars_error_t mars_yolo_track_cosine(const signed char *q, int qq, const signed char *e, int ee, int c, float *cos) {
    if (!q || !e || !cos || c <= 0) return MARS_ERR_INVALID_FILE;
    if (c > MHIP_TRACK_APP_MAX_C || qq <= 0 || ee <= 0) return MARS_ERR_INVALID_TENSOR;
    int dot = 0;
    for (int i = 0; i < c; i++) dot += (int)q[i] * (int)e[i];
    const float einv = 1.0f / sqrtf((float)ee), qinv = 1.0f / sqrtf((float)qq);
    const float key = (float)dot * einv; /* (this file is compiled with contraction off) */
    *cos = key * qinv;
    return MARS_OK;
}

mars_error_t mars_yolo_embed_blend(const signed char *e, int ee, const signed char *q, int qq, int c, signed char *out, int *out_ee) {
    if (!out || !out_ee || c <= 0 || ee < 0 || qq < 0 || (ee > 0 && !e) || (qq > 0 && !q)) return MARS_ERR_INVALID_FILE;
    if (c > MHIP_TRACK_APP_MAX_C) return MARS_ERR_INVALID_TENSOR;
    if (qq == 0 || ee == 0) { /* nothing to blend: the slot keeps what it has, or takes the detection's */
        const signed char *src = qq == 0 ? e : q;
        const int keep = qq == 0 ? ee : qq;
        if (keep) memmove(out, src, (size_t)c);
        else memset(out, 0, (size_t)c);
        *out_ee = keep;
        return MARS_OK;
    }
    int *v = (int *)malloc((size_t)c * sizeof(int));
    if (!v) return MARS_ERR_ALLOC_FAILED;
    for (int i = 0; i < c; i++) v[i] = 3 * (int)e[i] + (int)q[i];
    const mars_error_t rc = mars_yolo_embed_quantise(v, 1, c, out, out_ee);
    free(v);
    return rc;
}

mars_error_t mars_hip_tracker_read_embeddings(mars_hip_tracker_t *t, int stream, signed char *q, int *ee, int cap, int *n_live) {
    if (!t || cap < 0 || (cap > 0 && (!q || !ee))) return MARS_ERR_INVALID_FILE;
    if (stream < 0 || stream >= t->streams || !t->plane) return MARS_ERR_INVALID_TENSOR;
    if (!t->states || !t->hdr || !t->plane_ee || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t cp = (size_t)t->cp, c = (size_t)t->channels;
    mars_track_state_t *all = (mars_track_state_t *)malloc(MARS_TRACK_SLOTS * sizeof(*all));
    int8_t *rows = (int8_t *)malloc(MARS_TRACK_SLOTS * cp);
    int *sq = (int *)malloc(MARS_TRACK_SLOTS * sizeof(int));
    mars_error_t rc = all && rows && sq ? MARS_OK : MARS_ERR_ALLOC_FAILED;
    if (rc == MARS_OK &&
        (mhip_sync() || mhip_d2h_async(all, (uint8_t *)t->states + (size_t)stream * MARS_TRACK_SLOTS * sizeof(*all), MARS_TRACK_SLOTS * sizeof(*all)) ||
         mhip_d2h_async(rows, t->plane + (size_t)stream * MARS_TRACK_SLOTS * cp, MARS_TRACK_SLOTS * cp) ||
         mhip_d2h_async(sq, t->plane_ee + (size_t)stream * MARS_TRACK_SLOTS, MARS_TRACK_SLOTS * sizeof(int)) || mhip_sync()))
        rc = MARS_ERR_LAYER_FAILED;
    int n = 0;
    for (int s = 0; rc == MARS_OK && s < MARS_TRACK_SLOTS; s++) {
        if (all[s].hits <= 0) continue;
        if (n < cap) {
            memcpy(q + (size_t)n * c, rows + (size_t)s * cp, c);
            ee[n] = sq[s];
        }
        n++;
    }
    free(all); free(rows); free(sq);
    if (rc == MARS_OK && n_live) *n_live = n;
    return rc;
}

/* Both list forms: the checks in the order the error codes are pinned to, one scratch block, the uploads, the launch, the fetch.  app_form:
 * mars_yolo_track_lists_app, which needs a tracker with a plane and brings `app` and the vectors; the plain form passes none of them */
static mars_error_t track_lists(mars_hip_tracker_t *t, const mars_det_t *dets, const int *counts, const mars_cls_t *idents, const int *vectors,
                                int n_vectors, const int *emb_index, int frames, int max_det, const mars_hip_track_opts_t *opts, int app_form,
                                const mars_hip_track_app_opts_t *app, mars_track_t *out) {
    mhip_track_app_t a;
    memset(&a, 0, sizeof(a));
    mars_error_t e = track_opts(opts, &a.t);
    if (e != MARS_OK) return e;
    if (app_form && (e = track_app_opts(app, &a)) != MARS_OK) return e;
    if (!t || !dets || !counts || !out || frames <= 0 || max_det <= 0) return MARS_ERR_INVALID_FILE;
    if (n_vectors < 0 || (n_vectors > 0 && (!vectors || !emb_index))) return MARS_ERR_INVALID_FILE;
    if ((opts->flags & MARS_TRACK_CARRY_IDENTITY) && !idents) return MARS_ERR_INVALID_FILE;
    if (max_det > MARS_YOLO_MAX_DET || n_vectors > MHIP_MATCH_MAX_ROWS) return MARS_ERR_INVALID_TENSOR;
    if ((e = track_map(&a.t, t, frames)) != MARS_OK) return e;
    if (app_form && !t->plane) return MARS_ERR_INVALID_TENSOR; /* a tracker of mars_hip_tracker_create */
    if (!t->states || !t->hdr || (app_form && !t->plane_ee) || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (app_form) track_app_plane(&a, t);
    if (n_vectors > 0 && (e = track_app_scratch(t, &a)) != MARS_OK) return e;
    const size_t n = (size_t)frames * max_det, nv = (size_t)n_vectors;
    const int carry = (opts->flags & MARS_TRACK_CARRY_IDENTITY) != 0;
    /* one scratch block: [dets][counts][tracks][identities, where they are carried], and where vectors come
     * [vectors][their int8 rows][their qq][the row indices] */
    const size_t sz[8] = {n * sizeof(mars_det_t), (size_t)frames * sizeof(int), n * sizeof(mars_track_t), carry ? n * sizeof(mars_cls_t) : 0,
                          nv * t->channels * sizeof(int), nv * t->cp, nv * sizeof(int), nv ? n * sizeof(int) : 0};
    size_t off[8];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 8, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    a.t.max_det = max_det;
    a.t.dets = d;
    a.t.counts = (const int *)(d + off[1]);
    a.t.out = d + off[2];
    a.t.idents = carry ? d + off[3] : NULL;
    if (nv) {
        a.vec = (const int *)(d + off[4]);
        a.n_vec = n_vectors;
        a.q = (int8_t *)(d + off[5]);
        a.qq = (int *)(d + off[6]);
        a.emb_index = (const int *)(d + off[7]);
    }
    /* on the main stream: behind whatever the auxiliary stream still does to this tracker's tables, hence the wait first */
    int rc = mhip_sync();
    if (!rc) rc = mhip_h2d_async(d, dets, sz[0]) || mhip_h2d_async(d + off[1], counts, sz[1]);
    if (!rc && carry) rc = mhip_h2d_async(d + off[3], idents, sz[3]);
    if (!rc && nv) rc = mhip_h2d_async(d + off[4], vectors, sz[4]) || mhip_h2d_async(d + off[7], emb_index, sz[7]);
    if (!rc) rc = app_form ? mhip_track_app(&a) : track_launch(t, &a.t);
    if (!rc) rc = mhip_d2h_async(out, a.t.out, sz[2]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_yolo_track_lists_app(mars_hip_tracker_t *t, const mars_det_t *dets, const int *counts, const mars_cls_t *idents, const int *vectors,
                                       int n_vectors, const int *emb_index, int frames, int max_det, const mars_hip_track_opts_t *opts,
                                       const mars_hip_track_app_opts_t *app, mars_track_t *out) {
    return track_lists(t, dets, counts, idents, vectors, n_vectors, emb_index, frames, max_det, opts, 1, app, out);
}

mars_error_t mars_yolo_track_cosine_matrix(const signed char *track_q, const int *track_ee, const int *vectors, int nt, int nc, int c, float *out) {
    if (!track_q || !track_ee || !vectors || !out || nt <= 0 || nc <= 0 || c <= 0) return MARS_ERR_INVALID_FILE;
    if (nt > MARS_TRACK_SLOTS || nc > MARS_TRACK_MAX_CAND || c > MHIP_TRACK_APP_MAX_C) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t cp = ((size_t)c + 63) & ~(size_t)63;
    /* [plane][ee][vectors][their int8 rows][their qq][the two matrices][out][the flag] */
    const size_t sz[8] = {MARS_TRACK_SLOTS * cp, MARS_TRACK_SLOTS * sizeof(int), (size_t)nc * c * sizeof(int), (size_t)nc * cp, (size_t)nc * sizeof(int),
                          MHIP_TRACK_APP_COS_FLOATS * sizeof(float), (size_t)nt * nc * sizeof(float), sizeof(int)};
    size_t off[8];
    const size_t total = mars_block_layout(sz, 8, off);
    int8_t *plane = (int8_t *)calloc(MARS_TRACK_SLOTS, cp);
    int ee[MARS_TRACK_SLOTS] = {0}, bad = 0;
    uint8_t *d = plane ? (uint8_t *)mhip_malloc(total) : NULL;
    if (!d) {
        free(plane);
        return MARS_ERR_ALLOC_FAILED;
    }
    for (int s = 0; s < nt; s++) {
        ee[s] = track_ee[s] > 0 ? track_ee[s] : 0;
        if (ee[s]) memcpy(plane + (size_t)s * cp, track_q + (size_t)s * c, (size_t)c);
    }
    int rc = mhip_h2d_async(d, plane, sz[0]) || mhip_h2d_async(d + off[1], ee, sz[1]) || mhip_h2d_async(d + off[2], vectors, sz[2]) ||
             mhip_memset_async(d + off[7], 0, sz[7]);
    if (!rc)
        rc = mhip_track_app_matrix((const int8_t *)d, (const int *)(d + off[1]), (const int *)(d + off[2]), nt, nc, c, (int)cp, (int8_t *)(d + off[3]),
                                   (int *)(d + off[4]), (float *)(d + off[5]), (float *)(d + off[6]), (int *)(d + off[7]));
    if (!rc) rc = mhip_d2h_async(out, d + off[6], sz[6]) || mhip_d2h_async(&bad, d + off[7], sz[7]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    free(plane);
    return rc || bad ? MARS_ERR_LAYER_FAILED : MARS_OK; /* bad: the candidate-major copy of the matrix differs from the slot-major one */
}

mars_error_t mars_yolo_track_lists(mars_hip_tracker_t *t, const mars_det_t *dets, const int *counts, const mars_cls_t *idents, int frames,
                                   int max_det, const mars_hip_track_opts_t *opts, mars_track_t *out) {
    return track_lists(t, dets, counts, idents, NULL, 0, NULL, frames, max_det, opts, 0, NULL, out);
}

/* The detector's side of a device call, the same with and without a second model: its lists in HBM, the identities where they are carried,
 * the frame -> stream map, room for the results, and the mhip_track_t part of the launch record filled */
static mars_error_t track_from_detector(mars_model_ext_t *det, const mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts, mhip_track_t *p) {
    if (!mars_has_dets(det)) return MARS_ERR_INVALID_TENSOR;                                               /* no detections in HBM */
    const int carry = (opts->flags & MARS_TRACK_CARRY_IDENTITY) != 0;
    if (carry && (!det->ident.dev || det->ident.frames < det->batch)) return MARS_ERR_INVALID_TENSOR;      /* no identity scatter */
    mars_error_t e = track_map(p, t, det->batch);
    if (e != MARS_OK) return e;
    if ((e = mars_side_reserve(&det->track, det->batch, sizeof(mars_track_t))) != MARS_OK) return e;
    p->max_det = MARS_YOLO_MAX_DET;
    p->dets = det->det_dev;
    p->counts = det->det_counts_dev;
    p->idents = carry ? det->ident.dev : NULL;
    p->out = det->track.dev;
    return MARS_OK;
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
    if ((e = track_from_detector(det, t, opts, &p)) != MARS_OK) return e;
    /* The auxiliary stream, as the label scatter: it carries every detection tail and every scatter, so this comes behind the tail that
     * wrote the lists and the scatter that wrote the identities, and ahead of det_model's next detect call.  Nothing on the main stream
     * reads or writes what the kernel touches, so nothing there waits for it */
    det->track.frames = 0;
    mhip_select_aux(1);
    const int rc = track_launch(t, &p);
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

mars_error_t mars_hip_track_app_device(mars_model_t *det_model, mars_model_t *cls_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts,
                                       const mars_hip_track_app_opts_t *app) {
    mhip_track_app_t a;
    memset(&a, 0, sizeof(a));
    if (!det_model || !cls_model || !t) return MARS_ERR_INVALID_FILE;
    mars_error_t e = track_opts(opts, &a.t);
    if (e != MARS_OK) return e;
    if ((e = track_app_opts(app, &a)) != MARS_OK) return e;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model, *m = (mars_model_ext_t *)cls_model;
    if (det == m || !t->plane) return MARS_ERR_INVALID_TENSOR; /* (neither model has been looked into yet) */
    /* the identify join's conditions (mars_scatter_on_aux), with the classify results where it has the match results */
    if (!m->act_dev || !det->act_dev || !t->states || !t->hdr || !t->plane_ee || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe || det->pipe) return MARS_ERR_INVALID_TENSOR;
    if (!m->roi_dev || m->roi_slots <= 0 || m->roi_from != det) return MARS_ERR_INVALID_TENSOR;             /* no crop call out of det_model */
    if (!m->cls.dev || m->cls.frames <= 0 || m->cls.frames < m->roi_slots) return MARS_ERR_INVALID_TENSOR;  /* no classify results */
    if (m->cls_c != t->channels) return MARS_ERR_INVALID_TENSOR;
    if ((e = track_from_detector(det, t, opts, &a.t)) != MARS_OK) return e;
    const size_t nv = (size_t)m->roi_slots;
    const size_t sz[3] = {nv * t->cp, nv * sizeof(int), (size_t)det->batch * MARS_YOLO_MAX_DET * sizeof(int)};
    size_t off[3];
    if ((e = mars_block_reserve(&det->track_app, mars_block_layout(sz, 3, off), 0, NULL)) != MARS_OK) return e;
    track_app_plane(&a, t);
    if ((e = track_app_scratch(t, &a)) != MARS_OK) return e;
    if (!m->ev_label_done && !(m->ev_label_done = mhip_event_create_sync())) return MARS_ERR_ALLOC_FAILED;
    uint8_t *blk = (uint8_t *)det->track_app.dev;
    a.vec = (const int *)((uint8_t *)m->cls.dev + m->cls_sums_off);
    a.n_vec = m->roi_slots; /* every slot's row is quantised; the index below names those below `kept` only */
    a.q = (int8_t *)blk; a.qq = (int *)(blk + off[1]);
    a.emb_index = (const int *)(blk + off[2]);
    /* The auxiliary stream, with the identity scatter's ordering (mars_scatter_on_aux): behind both models' tails and the identity scatter,
     * ahead of det_model's next detect call and cls_model's next classify call.  The ROI table is written on the main stream: the index
     * scatter waits for what that stream has been given so far, and the next crop call into cls_model waits for this call (ev_label_done) */
    det->track.frames = 0;
    mhip_select_stream(0);
    if ((e = mars_aux_behind_current(&m->ev_graph_done)) != MARS_OK) return e;
    int rc = mhip_track_app_index((uint8_t *)m->roi_dev + 16, (const int *)m->roi_dev, m->roi_slots, (int *)(blk + off[2]), det->batch, MARS_YOLO_MAX_DET);
    if (!rc) rc = mhip_track_app(&a);
    if (!rc) rc = mhip_event_record(m->ev_label_done);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->label_pending = 1;
    det->track.frames = det->batch;
    return MARS_OK;
}

mars_error_t mars_hip_track_app(mars_model_t *det_model, mars_model_t *cls_model, mars_hip_tracker_t *t, const mars_hip_track_opts_t *opts,
                                const mars_hip_track_app_opts_t *app, mars_track_t *tracks) {
    if (!det_model || !cls_model || !t || !opts || !app || !tracks) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_track_app_device(det_model, cls_model, t, opts, app);
    return e != MARS_OK ? e : mars_hip_track_results(det_model, tracks);
}
