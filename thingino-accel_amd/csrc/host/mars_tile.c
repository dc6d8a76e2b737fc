/*
 * mars_tile.c -- host side of the tiled inference (include/mars_hip.h, "Tiled inference"): the grid rule, argument checks and the options'
 * defaults, the per-tile map factors (the host's float32 division), the ROI table and the merged arrays hung on the model, stream ordering,
 * and the launches of csrc/hip/tile.hip and of roi.hip's crop kernel.  The reference has no batch and no such step.  There is no CPU pixel or
 * merge path: without the device every entry point but mars_tile_grid fails once its arguments have passed the checks.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

_Static_assert(sizeof(mars_tile_t) == 16 && sizeof(mars_tile_src_t) == 8 && sizeof(mars_tile_stats_t) == 24, "the records tile.hip reads and writes");
_Static_assert(MARS_TILE_MAX_TILES == MHIP_TILE_MAX_TILES && MARS_TILE_MAX_CAND == MHIP_TILE_MAX_CAND, "the kernel's table and candidate sizes");

#define TILE_FLAGS (MARS_TILE_KEEP_ASPECT | MARS_TILE_MATCH_IOS | MARS_TILE_AGNOSTIC | MARS_TILE_AREA)

/* the number of starts of one axis: every k with k * step + tile < W, and the final one */
static long long axis_starts(int W, int tile, int overlap) {
    if (tile >= W) return 1;
    const long long step = tile - overlap;
    return ((long long)W - tile + step - 1) / step + 1;
}

int mars_tile_grid(int W, int H, int tile_w, int tile_h, int overlap_x, int overlap_y, mars_tile_t *tiles, int cap) {
    if (W <= 0 || H <= 0 || tile_w <= 0 || tile_h <= 0 || overlap_x < 0 || overlap_y < 0 || overlap_x >= tile_w || overlap_y >= tile_h) return -1;
    const long long nx = axis_starts(W, tile_w, overlap_x), ny = axis_starts(H, tile_h, overlap_y);
    if (nx * ny > 0x7fffffff) return -1;
    if (!tiles || cap <= 0) return (int)(nx * ny);
    const int tw = tile_w < W ? tile_w : W, th = tile_h < H ? tile_h : H;
    const int step_x = tile_w - overlap_x, step_y = tile_h - overlap_y;
    long long k = 0;
    for (long long iy = 0; iy < ny && k < cap; iy++) {
        const int y0 = iy + 1 < ny ? (int)(iy * step_y) : H - th;
        for (long long ix = 0; ix < nx && k < cap; ix++, k++) {
            const int x0 = ix + 1 < nx ? (int)(ix * step_x) : W - tw;
            tiles[k].x0 = x0; tiles[k].y0 = y0; tiles[k].x1 = x0 + tw; tiles[k].y1 = y0 + th;
        }
    }
    return (int)(nx * ny);
}

/* the checks that need no device and no model, and the launch record: table, geometry of a tw x th target, defaults resolved */
static mars_error_t tile_opts(const mars_hip_tile_opts_t *o, int tw, int th, mhip_tile_t *p) {
    memset(p, 0, sizeof(*p));
    if (!o || !o->tiles || o->src_w <= 0 || o->src_h <= 0 || tw <= 0 || th <= 0) return MARS_ERR_INVALID_FILE;
    if (o->n_tiles < 1 || o->n_tiles > MARS_TILE_MAX_TILES) return MARS_ERR_INVALID_FILE;
    if (!mhip_frame_format_ok(o->src_format, o->src_flags) || !mhip_frame_bytes(o->src_w, o->src_h, o->src_format)) return MARS_ERR_INVALID_FILE;
    if (o->flags & ~TILE_FLAGS) return MARS_ERR_INVALID_FILE;
    if (!isfinite(o->merge_thresh) || o->merge_thresh < 0 || o->merge_thresh > 1 || !isfinite(o->edge_margin) || o->edge_margin < 0)
        return MARS_ERR_INVALID_FILE;
    if (o->max_per_tile < 0 || (long long)o->n_tiles * o->max_per_tile > MARS_TILE_MAX_CAND) return MARS_ERR_INVALID_FILE;
    for (int t = 0; t < o->n_tiles; t++) {
        const mars_tile_t *r = &o->tiles[t];
        if (r->x0 < 0 || r->y0 < 0 || r->x1 <= r->x0 || r->y1 <= r->y0 || r->x1 > o->src_w || r->y1 > o->src_h) return MARS_ERR_INVALID_FILE;
        const int cw = r->x1 - r->x0, ch = r->y1 - r->y0;
        int nw = tw, nh = th; /* "ROI crops", target geometry */
        if (o->flags & MARS_TILE_KEEP_ASPECT) {
            if ((long long)cw * th >= (long long)ch * tw) {
                nh = (int)(((long long)ch * tw + cw / 2) / cw);
                if (nh < 1) nh = 1;
            } else {
                nw = (int)(((long long)cw * th + ch / 2) / ch);
                if (nw < 1) nw = 1;
            }
        }
        mhip_tile_geom_t *g = &p->tiles[t];
        g->x0 = r->x0; g->y0 = r->y0; g->x1 = r->x1; g->y1 = r->y1;
        g->px = (float)((tw - nw) / 2); g->py = (float)((th - nh) / 2);
        g->rx = (float)cw / (float)nw; g->ry = (float)ch / (float)nh;
    }
    p->n_tiles = o->n_tiles;
    p->src_w = o->src_w; p->src_h = o->src_h;
    const int q = MARS_TILE_MAX_CAND / o->n_tiles;
    p->quota = o->max_per_tile ? o->max_per_tile : (q < MARS_YOLO_MAX_DET ? q : MARS_YOLO_MAX_DET);
    p->ios = (o->flags & MARS_TILE_MATCH_IOS) != 0;
    p->agnostic = (o->flags & MARS_TILE_AGNOSTIC) != 0;
    p->thresh = o->merge_thresh != 0 ? o->merge_thresh : 0.5f;
    p->edge_margin = o->edge_margin;
    return MARS_OK;
}

/* the crop launch record of a tile call: the ROI rules that look at boxes are not used, their fields only have to pass the launcher's checks */
static mars_error_t tile_roi(const mars_hip_tile_opts_t *o, int tw, int th, mhip_roi_t *r) {
    memset(r, 0, sizeof(*r));
    if (!mhip_roi_fits(o->src_w, tw, o->src_format)) return MARS_ERR_INVALID_FILE;
    if ((o->flags & MARS_TILE_AREA) && !mhip_roi_area_fits(o->src_w, tw, o->src_format)) return MARS_ERR_INVALID_FILE;
    r->w = o->src_w; r->h = o->src_h; r->fmt = o->src_format; r->nv12_flags = o->src_flags;
    r->frame_stride = mhip_frame_bytes(r->w, r->h, r->fmt);
    r->expand = 1.0f; r->min_size = 1;
    r->keep_aspect = (o->flags & MARS_TILE_KEEP_ASPECT) != 0;
    r->area = (o->flags & MARS_TILE_AREA) != 0;
    r->tw = tw; r->th = th;
    return MARS_OK;
}

mars_error_t mars_yolo_tile_frames(const unsigned char *frames, int n_frames, const mars_hip_tile_opts_t *opts, int tw, int th, int nhwc,
                                   signed char *out) {
    mhip_tile_t p;
    mhip_roi_t r;
    mars_error_t e = tile_opts(opts, tw, th, &p);
    if (e == MARS_OK) e = tile_roi(opts, tw, th, &r);
    if (e != MARS_OK) return e;
    if (!frames || !out || n_frames <= 0 || (long long)n_frames * p.n_tiles > 65535) return MARS_ERR_INVALID_FILE;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const int slots = n_frames * p.n_tiles;
    const size_t in_b = r.frame_stride * (size_t)n_frames, out_b = (size_t)tw * th * 3;
    /* one device block: [frames][counters][rois][out] */
    const size_t sz[4] = {in_b, 256, (size_t)slots * sizeof(mars_roi_t), out_b * (size_t)slots};
    size_t off[4];
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 4, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.cams = n_frames;
    p.n_out = (int *)(d + off[1]); p.rois = d + off[2];
    r.frames = d; r.n_frames = n_frames;
    r.n_out = p.n_out; r.rois = p.rois;
    r.out = (int8_t *)(d + off[3]); r.out_stride = out_b; r.slots = slots; r.nhwc = nhwc != 0;
    int rc = mhip_h2d_async(d, frames, in_b);
    if (!rc) rc = mhip_tile_rois(&p);
    if (!rc) rc = mhip_roi_crop(&r);
    if (!rc) rc = mhip_d2h_async(out, r.out, out_b * (size_t)slots);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_hip_preprocess_tiles_device(mars_model_t *model, int input_index, const void *frames_dev, const mars_hip_tile_opts_t *opts) {
    if (!model || !frames_dev || !opts) return MARS_ERR_INVALID_FILE;
    mhip_tile_t p;
    mhip_roi_t r;
    mars_error_t e = tile_opts(opts, 1, 1, &p); /* what can be said without looking at the model */
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if ((e = mars_stage_guard(m)) != MARS_OK) return e;
    mars_pixel_input_t in;
    if ((e = mars_pixel_input(m, input_index, 0, &in)) != MARS_OK) return e;
    if (m->batch % opts->n_tiles || m->batch > 65535) return MARS_ERR_INVALID_TENSOR;
    e = tile_opts(opts, in.tw, in.th, &p);
    if (e == MARS_OK) e = tile_roi(opts, in.tw, in.th, &r);
    if (e != MARS_OK) return e;
    /* (a re-allocation synchronises: a crop queued earlier may still read the old table) */
    if ((e = mars_block_reserve(&m->tile_roi, 256 + (size_t)m->batch * sizeof(mars_roi_t), 0, NULL)) != MARS_OK) return e;
    p.cams = m->batch / p.n_tiles;
    p.n_out = (int *)m->tile_roi.dev; p.rois = (uint8_t *)m->tile_roi.dev + 256;
    r.frames = (const uint8_t *)frames_dev; r.n_frames = p.cams;
    r.n_out = p.n_out; r.rois = p.rois;
    r.out = in.dev; r.out_stride = in.stride; r.slots = m->batch; r.nhwc = in.nhwc;
    /* the current stream, as mars_hip_preprocess_device: the table first, then the crops that read it */
    return mhip_tile_rois(&p) || mhip_roi_crop(&r) ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_hip_preprocess_tiles(mars_model_t *model, int input_index, const unsigned char *frames, const mars_hip_tile_opts_t *opts) {
    if (!model || !frames || !opts) return MARS_ERR_INVALID_FILE;
    mhip_tile_t p;
    mars_error_t e = tile_opts(opts, 1, 1, &p);
    if (e != MARS_OK) return e;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const int B = mars_hip_get_batch(model);
    if (B <= 0 || B % opts->n_tiles) return MARS_ERR_INVALID_TENSOR;
    const size_t in_b = mhip_frame_bytes(opts->src_w, opts->src_h, opts->src_format) * (size_t)(B / opts->n_tiles);
    uint8_t *d = (uint8_t *)mhip_malloc(in_b);
    if (!d) return MARS_ERR_ALLOC_FAILED;
    if (mhip_h2d_async(d, frames, in_b)) e = MARS_ERR_LAYER_FAILED;
    if (e == MARS_OK) e = mars_hip_preprocess_tiles_device(model, input_index, d, opts);
    if (mhip_sync() && e == MARS_OK) e = MARS_ERR_LAYER_FAILED;
    mhip_free(d);
    return e;
}

mars_error_t mars_yolo_merge_tiles(const mars_det_t *dets, const int *counts, int n_frames, int max_det, const mars_hip_tile_opts_t *opts,
                                   int tw, int th, mars_det_t *out, int *out_counts, mars_tile_src_t *origins, mars_tile_stats_t *stats) {
    mhip_tile_t p;
    const mars_error_t e = tile_opts(opts, tw, th, &p);
    if (e != MARS_OK) return e;
    if (!dets || !counts || !out || !out_counts || n_frames <= 0 || max_det < 1 || max_det > MARS_YOLO_MAX_DET) return MARS_ERR_INVALID_FILE;
    if ((long long)n_frames * p.n_tiles > 65535) return MARS_ERR_INVALID_FILE;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t lists = (size_t)n_frames * p.n_tiles, C = (size_t)n_frames;
    /* one device block: [dets][counts][out][out_counts][origins][stats] */
    size_t off[6];
    const size_t sz[6] = {lists * max_det * sizeof(mars_det_t), lists * sizeof(int), C * MARS_YOLO_MAX_DET * sizeof(mars_det_t), C * sizeof(int),
                          C * MARS_YOLO_MAX_DET * sizeof(mars_tile_src_t), C * sizeof(mars_tile_stats_t)};
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 6, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.cams = n_frames; p.max_det = max_det;
    p.dets = d; p.counts = (const int *)(d + off[1]);
    p.out = d + off[2]; p.out_counts = (int *)(d + off[3]); p.origins = d + off[4]; p.stats = d + off[5];
    int rc = mhip_h2d_async(d, dets, sz[0]);
    if (!rc) rc = mhip_h2d_async(d + off[1], counts, sz[1]);
    if (!rc) rc = mhip_tile_merge(&p);
    if (!rc) rc = mhip_d2h_async(out, p.out, sz[2]);
    if (!rc) rc = mhip_d2h_async(out_counts, p.out_counts, sz[3]);
    if (!rc && origins) rc = mhip_d2h_async(origins, p.origins, sz[4]);
    if (!rc && stats) rc = mhip_d2h_async(stats, p.stats, sz[5]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

/* the merged arrays of C camera frames, one block: [dets][origins][counts][stats] */
static void tile_parts(size_t C, size_t sz[4]) {
    sz[0] = C * MARS_YOLO_MAX_DET * sizeof(mars_det_t); sz[1] = C * MARS_YOLO_MAX_DET * sizeof(mars_tile_src_t);
    sz[2] = C * sizeof(int); sz[3] = C * sizeof(mars_tile_stats_t);
}

mars_error_t mars_hip_merge_tiles_device(mars_model_t *model, const mars_hip_tile_opts_t *opts) {
    if (!model || !opts) return MARS_ERR_INVALID_FILE;
    mhip_tile_t p;
    mars_error_t e = tile_opts(opts, 1, 1, &p);
    if (e != MARS_OK) return e;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    if ((e = mars_stage_guard(m)) != MARS_OK) return e;
    if (m->batch % opts->n_tiles) return MARS_ERR_INVALID_TENSOR;
    if (!mars_has_dets(m)) return MARS_ERR_INVALID_TENSOR; /* no detections in HBM */
    if (m->det_mapped) return MARS_ERR_INVALID_TENSOR;   /* the lists are in source-frame pixels already */
    mars_pixel_input_t in; /* the geometry the tiles were cut for: input 0's */
    if ((e = mars_pixel_input(m, 0, 1, &in)) != MARS_OK) return e;
    if ((e = tile_opts(opts, in.tw, in.th, &p)) != MARS_OK) return e;
    const int C = m->batch / p.n_tiles;
    size_t sz[4], off[4];
    tile_parts((size_t)C, sz);
    if ((e = mars_block_reserve(&m->tile, mars_block_layout(sz, 4, off), 1, NULL)) != MARS_OK) return e;
    uint8_t *blk = (uint8_t *)m->tile.dev;
    p.cams = C; p.max_det = MARS_YOLO_MAX_DET;
    p.dets = m->det_dev; p.counts = m->det_counts_dev;
    p.out = blk + off[0]; p.origins = blk + off[1]; p.out_counts = (int *)(blk + off[2]); p.stats = blk + off[3];
    /* The auxiliary stream, as mars_hip_track_device: it carries every detection tail, so this comes behind the tail that wrote the lists and
     * ahead of the model's next detect call.  Nothing on the main stream reads or writes what the kernel touches */
    m->tile.frames = 0;
    mhip_select_aux(1);
    int rc = mhip_event_record(m->tile.ev[0]);
    if (!rc) rc = mhip_tile_merge(&p);
    if (!rc) rc = mhip_event_record(m->tile.ev[1]);
    mhip_select_aux(0);
    if (rc) return MARS_ERR_LAYER_FAILED;
    memcpy(m->tile_off, off, sizeof(off));
    m->tile.frames = C;
    return MARS_OK;
}

mars_error_t mars_hip_tile_results(mars_model_t *model, mars_det_t *dets, int *counts, mars_tile_src_t *origins, mars_tile_stats_t *stats) {
    if (!model) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    size_t sz[4];
    tile_parts((size_t)m->tile.frames, sz);
    const mars_block_part_t parts[4] = {{dets, m->tile_off[0], sz[0]}, {origins, m->tile_off[1], sz[1]}, {counts, m->tile_off[2], sz[2]},
                                        {stats, m->tile_off[3], sz[3]}};
    return mars_block_fetch(&m->tile, parts, 4, NULL);
}

int mars_hip_tile_frames(mars_model_t *model) {
    const mars_model_ext_t *m = (const mars_model_ext_t *)model;
    return m && m->tile.dev && m->tile.frames > 0 ? m->tile.frames : 0;
}

mars_error_t mars_hip_merge_tiles(mars_model_t *model, const mars_hip_tile_opts_t *opts, mars_det_t *dets, int *counts, mars_tile_src_t *origins,
                                  mars_tile_stats_t *stats) {
    const mars_error_t e = mars_hip_merge_tiles_device(model, opts);
    return e != MARS_OK ? e : mars_hip_tile_results(model, dets, counts, origins, stats);
}

float mars_hip_tile_ms(mars_model_t *model) { return model ? mars_block_ms(&((mars_model_ext_t *)model)->tile) : -1.0f; }
