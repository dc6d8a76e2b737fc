/*
 * mars_gallery.c -- host side of the gallery match (include/mars_hip.h, "Gallery match"): the quantisation rule on the host, the gallery
 * object and its device image, argument checks, the result block hung on the second-stage model, the identity array hung on the detector,
 * stream ordering, and the launches of csrc/hip/gallery.hip.  The reference has nothing of the kind: it stops at the feature map.  There is
 * no CPU path for the match itself: without the device every entry point but mars_yolo_embed_quantise fails.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

struct mars_hip_gallery {
    int channels, cp, capacity, count;
    int8_t *rows;   /* device: [capacity rounded up to 64][cp], pad channels zero */
    float *ginv;    /* device: [capacity rounded up to 64] */
    int *ids;       /* device: [capacity rounded up to 64] */
};
/* tests/test_gallery_cpu.py stands 256 zero bytes where a gallery would be, to reach the refusals that come before any device work: all
 * zero must read as a gallery without capacity and without rows, and the object must not outgrow those bytes */
_Static_assert(sizeof(struct mars_hip_gallery) <= 256, "tests/test_gallery_cpu.py passes 256 zero bytes as a gallery");

/* one vector by the rule; q gets `pitch` bytes, those behind c zero.  Returns qq (0: a null vector) */
static int quantise_one(const int *v, int c, int8_t *q, int pitch) {
    uint64_t m = 0;
    for (int i = 0; i < c; i++) {
        const uint64_t a = v[i] < 0 ? (uint64_t)(-(int64_t)v[i]) : (uint64_t)v[i];
        if (a > m) m = a;
    }
    int qq = 0;
    for (int i = 0; i < c; i++) {
        int x = 0;
        if (m) {
            const uint64_t a = v[i] < 0 ? (uint64_t)(-(int64_t)v[i]) : (uint64_t)v[i];
            const int mag = (int)((a * 127u + m / 2) / m);
            x = v[i] < 0 ? -mag : mag;
        }
        q[i] = (int8_t)x;
        qq += x * x;
    }
    for (int i = c; i < pitch; i++) q[i] = 0;
    return qq;
}

mars_error_t mars_yolo_embed_quantise(const int *vectors, int n, int c, signed char *q, int *qq) {
    if (!vectors || !q || n <= 0 || c <= 0) return MARS_ERR_INVALID_FILE;
    if (c > MHIP_MATCH_MAX_C) return MARS_ERR_INVALID_TENSOR;
    for (int i = 0; i < n; i++) {
        const int s = quantise_one(vectors + (size_t)i * c, c, (int8_t *)q + (size_t)i * c, c);
        if (qq) qq[i] = s;
    }
    return MARS_OK;
}

/* the checks that need no device, and the defaults resolved */
static mars_error_t match_opts(const mars_hip_match_opts_t *o, int *top_k, float *min_score) {
    if (!o || o->top_k < 0 || o->top_k > MARS_CLS_MAX_TOPK || o->flags) return MARS_ERR_INVALID_FILE;
    if (!isfinite(o->min_score) || o->min_score < 0) return MARS_ERR_INVALID_FILE;
    *top_k = o->top_k ? o->top_k : 1;
    *min_score = o->min_score;
    return MARS_OK;
}

mars_error_t mars_hip_gallery_create(int channels, int capacity, mars_hip_gallery_t **out) {
    if (!out || channels <= 0 || capacity <= 0) return MARS_ERR_INVALID_FILE;
    if (channels > MHIP_MATCH_MAX_C || capacity > MHIP_MATCH_MAX_ROWS) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    mars_hip_gallery_t *g = (mars_hip_gallery_t *)calloc(1, sizeof(*g));
    if (!g) return MARS_ERR_ALLOC_FAILED;
    g->channels = channels;
    g->cp = (channels + 63) & ~63;
    g->capacity = capacity;
    const size_t rows = ALIGN_UP((size_t)capacity, 64); /* the match kernel reads whole 16-row subtiles */
    g->rows = (int8_t *)mhip_malloc(rows * g->cp);
    g->ginv = (float *)mhip_malloc(rows * sizeof(float));
    g->ids = (int *)mhip_malloc(rows * sizeof(int));
    int rc = !g->rows || !g->ginv || !g->ids;
    if (!rc) rc = mhip_memset_async(g->rows, 0, rows * g->cp) || mhip_memset_async(g->ginv, 0, rows * sizeof(float)) ||
                  mhip_memset_async(g->ids, 0, rows * sizeof(int)) || mhip_sync();
    if (rc) {
        mars_hip_gallery_free(g);
        return MARS_ERR_ALLOC_FAILED;
    }
    *out = g;
    return MARS_OK;
}

void mars_hip_gallery_free(mars_hip_gallery_t *g) {
    if (!g) return;
    if (mhip_ready()) mhip_sync(); /* a match may still read the rows */
    if (g->rows) mhip_free(g->rows);
    if (g->ginv) mhip_free(g->ginv);
    if (g->ids) mhip_free(g->ids);
    free(g);
}

int mars_hip_gallery_count(const mars_hip_gallery_t *g) { return g ? g->count : -1; }

mars_error_t mars_hip_gallery_clear(mars_hip_gallery_t *g) {
    if (!g) return MARS_ERR_INVALID_FILE;
    g->count = 0; /* (a match enqueued earlier took its row count with it) */
    return MARS_OK;
}

mars_error_t mars_hip_gallery_add(mars_hip_gallery_t *g, const int *vectors, const int *ids, int n) {
    if (!g || !vectors || !ids || n <= 0) return MARS_ERR_INVALID_FILE;
    if (n > g->capacity - g->count) return MARS_ERR_INVALID_TENSOR;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0) return MARS_ERR_INVALID_FILE;
    const size_t cp = (size_t)g->cp;
    int8_t *q = (int8_t *)malloc((size_t)n * cp);
    float *ginv = (float *)malloc((size_t)n * sizeof(float));
    if (!q || !ginv) {
        free(q); free(ginv);
        return MARS_ERR_ALLOC_FAILED;
    }
    mars_error_t e = MARS_OK;
    for (int i = 0; i < n && e == MARS_OK; i++) {
        const int gg = quantise_one(vectors + (size_t)i * g->channels, g->channels, q + (size_t)i * cp, g->cp);
        if (!gg) e = MARS_ERR_INVALID_TENSOR; /* a null vector has no direction */
        else ginv[i] = 1.0f / sqrtf((float)gg);
    }
    /* behind every match enqueued so far (they read rows below count only, but waiting is simplest and an enrolment is rare) */
    if (e == MARS_OK && (!mhip_ready() || mhip_sync())) e = MARS_ERR_LAYER_FAILED;
    if (e == MARS_OK && (mhip_h2d_async(g->rows + (size_t)g->count * cp, q, (size_t)n * cp) ||
                         mhip_h2d_async(g->ginv + g->count, ginv, (size_t)n * sizeof(float)) ||
                         mhip_h2d_async(g->ids + g->count, ids, (size_t)n * sizeof(int)) || mhip_sync()))
        e = MARS_ERR_LAYER_FAILED;
    free(q); free(ginv);
    if (e == MARS_OK) g->count += n;
    return e;
}

int mars_hip_match_chunk(int rows) { return mhip_match_chunk(rows); }

/* the device block of a match of n queries: fills the pointers of p from `base` (NULL: sizes only); -> bytes */
static size_t match_block(mhip_match_t *p, uint8_t *base, size_t *top_off, size_t *row_off) {
    const size_t n = (size_t)p->queries, chunks = ((size_t)p->n_rows + p->chunk - 1) / p->chunk;
    const size_t sz[6] = {ALIGN_UP(n, 64) * p->cp, n * sizeof(int), n * sizeof(float), n * chunks * MHIP_MATCH_KEEP * sizeof(unsigned long long),
                          n * p->top_k * sizeof(mars_cls_t), n * p->top_k * sizeof(int)};
    size_t o[6];
    const size_t total = mars_block_layout(sz, 6, o);
    if (base) {
        p->q = (int8_t *)(base + o[0]); p->qq = (int *)(base + o[1]); p->qinv = (float *)(base + o[2]);
        p->part = (unsigned long long *)(base + o[3]); p->top = base + o[4]; p->top_row = (int *)(base + o[5]);
    }
    *top_off = o[4]; *row_off = o[5];
    return total;
}

static void match_gallery(mhip_match_t *p, const mars_hip_gallery_t *g) {
    p->c = g->channels; p->cp = g->cp;
    p->rows = g->rows; p->ginv = g->ginv; p->ids = g->ids;
    p->n_rows = g->count;
    p->chunk = mhip_match_chunk(g->count);
}

mars_error_t mars_yolo_match_vectors(mars_hip_gallery_t *g, const int *vectors, int n, const mars_hip_match_opts_t *opts, mars_cls_t *top, int *rows) {
    mhip_match_t p;
    memset(&p, 0, sizeof(p));
    const mars_error_t e = match_opts(opts, &p.top_k, &p.min_score);
    if (e != MARS_OK) return e;
    if (!g || !vectors || !top || n <= 0) return MARS_ERR_INVALID_FILE;
    if (n > 65535 || g->count <= 0) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    p.queries = n;
    match_gallery(&p, g);
    size_t to, ro;
    const size_t vec_b = ALIGN_UP((size_t)n * g->channels * sizeof(int), 256), total = vec_b + match_block(&p, NULL, &to, &ro);
    uint8_t *d = (uint8_t *)mhip_malloc(total);
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.vec = (const int *)d;
    match_block(&p, d + vec_b, &to, &ro);
    int rc = mhip_h2d_async(d, vectors, (size_t)n * g->channels * sizeof(int));
    if (!rc) rc = mhip_match(&p);
    if (!rc) rc = mhip_d2h_async(top, p.top, (size_t)n * p.top_k * sizeof(mars_cls_t));
    if (!rc && rows) rc = mhip_d2h_async(rows, p.top_row, (size_t)n * p.top_k * sizeof(int));
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_hip_match_device(mars_model_t *cls_model, mars_hip_gallery_t *g, const mars_hip_match_opts_t *opts) {
    mhip_match_t p;
    memset(&p, 0, sizeof(p));
    if (!cls_model || !g) return MARS_ERR_INVALID_FILE;
    mars_error_t e = match_opts(opts, &p.top_k, &p.min_score);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)cls_model;
    if ((e = mars_stage_guard(m)) != MARS_OK) return e;
    if (!m->cls.dev || m->cls.frames <= 0) return MARS_ERR_INVALID_TENSOR; /* no classify results */
    if (g->channels != m->cls_c || g->count <= 0) return MARS_ERR_INVALID_TENSOR;
    p.queries = m->cls.frames;
    p.vec = (const int *)((uint8_t *)m->cls.dev + m->cls_sums_off);
    match_gallery(&p, g);
    size_t to, ro;
    if ((e = mars_block_reserve(&m->match, match_block(&p, NULL, &to, &ro), 0, NULL)) != MARS_OK) return e;
    match_block(&p, (uint8_t *)m->match.dev, &to, &ro);
    /* The auxiliary stream: behind the classify tail that writes the sums, behind an earlier identity scatter that reads this block, and
     * ahead of the next classify tail that overwrites the sums */
    m->match.frames = 0;
    mhip_select_aux(1);
    const int rc = mhip_match(&p);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    m->match_top_off = to; m->match_row_off = ro;
    m->match.frames = p.queries; m->match_top_k = p.top_k;
    return MARS_OK;
}

mars_error_t mars_hip_match_results(mars_model_t *cls_model, mars_cls_t *top, int *rows) {
    if (!cls_model || !top) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)cls_model;
    const size_t n = (size_t)m->match.frames * m->match_top_k;
    const mars_block_part_t parts[2] = {{top, m->match_top_off, n * sizeof(mars_cls_t)}, {rows, m->match_row_off, n * sizeof(int)}};
    return mars_block_fetch(&m->match, parts, 2, NULL);
}

mars_error_t mars_hip_match(mars_model_t *cls_model, mars_hip_gallery_t *g, const mars_hip_match_opts_t *opts, mars_cls_t *top, int *rows) {
    if (!cls_model || !g || !opts || !top) return MARS_ERR_INVALID_FILE;
    const mars_error_t e = mars_hip_match_device(cls_model, g, opts);
    return e != MARS_OK ? e : mars_hip_match_results(cls_model, top, rows);
}

mars_error_t mars_hip_identify_detections_device(mars_model_t *det_model, mars_model_t *cls_model) {
    if (!det_model || !cls_model) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model, *m = (mars_model_ext_t *)cls_model;
    return mars_scatter_on_aux(det, m, &m->match, m->match_top_off, m->match_top_k, &det->ident);
}

mars_error_t mars_hip_identity_results(mars_model_t *det_model, mars_cls_t *idents) {
    if (!det_model || !idents) return MARS_ERR_INVALID_FILE;
    return mars_side_fetch(&((mars_model_ext_t *)det_model)->ident, idents, sizeof(mars_cls_t));
}
