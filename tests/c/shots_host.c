/*
 * shots_host.c -- the parts of csrc/host/mars_shots.c that need no device, on the CPU, built with ASan + UBSan by
 * tests/test_shot_host_cpu.py: the option checks, the frame -> stream map, and the uint8 relayout behind mars_hip_shots_read_pixels and
 * mars_hip_shots_collect.  The device layer is stood in for as in stage_block.c (memory is host malloc, copies are memcpy, the launch does
 * nothing), so the object's host paths -- create, reset, flush, read, collect, free -- run over tables and a plane this program fills
 * itself.  Exit status 0 and "shots_host: ok" when every check holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mars_internal.h"

static int g_live_allocs, g_live_events;

/* ---- the device layer mars_shots.c and mars_stage.c call */
int mhip_ready(void) { return 1; }
int mhip_sync(void) { return 0; }
void *mhip_malloc(size_t bytes) { g_live_allocs++; return malloc(bytes ? bytes : 1); }
void mhip_free(void *p) { g_live_allocs--; free(p); }
int mhip_memset_async(void *dst, int value, size_t bytes) { memset(dst, value, bytes); return 0; }
int mhip_h2d_async(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
int mhip_d2h_async(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
void *mhip_event_create(void) { g_live_events++; return malloc(1); }
void *mhip_event_create_sync(void) { return mhip_event_create(); }
void mhip_event_destroy(void *ev) { g_live_events--; free(ev); }
int mhip_event_record(void *ev) { (void)ev; return 0; }
float mhip_event_elapsed_ms(void *a, void *b) { (void)a; (void)b; return 0.25f; }
void mhip_select_aux(int on) { (void)on; }
void mhip_select_stream(int which) { (void)which; }
int mhip_stream_wait(int which, void *ev) { (void)which; (void)ev; return 0; }
int mhip_label_scatter(const void *rois, const int *n_out, int slots, const void *top, int top_k, void *labels, int det_frames, int det_cap) {
    (void)rois; (void)n_out; (void)slots; (void)top; (void)top_k; (void)labels; (void)det_frames; (void)det_cap;
    return 0;
}
static mhip_shots_t g_launch; /* the last launch record */
static int g_launches;
int mhip_shots(const mhip_shots_t *p) { g_launch = *p; g_launches++; return 0; }
/* ... and the rest of the library they name (not exercised here) */
int mars_tensor_chw(const mars_tensor_t *d, int *c, int *h, int *w) { (void)d; (void)c; (void)h; (void)w; return -1; }
int mars_locate_i8(const mars_model_ext_t *m, int T, int ch, int hh, int ww, int any_writer, int *buf, int *off, int *pix_step, int *ch_step) {
    (void)m; (void)T; (void)ch; (void)hh; (void)ww; (void)any_writer; (void)buf; (void)off; (void)pix_step; (void)ch_step;
    return -1;
}
void mars_roi_release(mars_model_ext_t *m) { (void)m; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "shots_host: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int test_opts(void) {
    mhip_shots_t p;
    mars_hip_shot_opts_t o;
    memset(&p, 0, sizeof(p));
    memset(&o, 0, sizeof(o));
    CHECK(mars_shots_opts(NULL, &p) == MARS_ERR_INVALID_FILE);
    CHECK(mars_shots_opts(&o, &p) == MARS_OK && p.max_gap == 30 && p.min_hits == 1 && !p.stream_major && !p.keep_aspect && !p.inside);
    o.max_gap = 3; o.min_hits = 2; o.min_mean = 10; o.max_mean = 255; o.min_sharp = 7; o.src_w = 320; o.src_h = 240;
    o.flags = MARS_SHOT_STREAM_MAJOR | MARS_SHOT_KEEP_ASPECT | MARS_SHOT_INSIDE;
    CHECK(mars_shots_opts(&o, &p) == MARS_OK && p.max_gap == 3 && p.min_hits == 2 && p.min_mean == 10 && p.max_mean == 255 && p.min_sharp == 7);
    CHECK(p.stream_major == 1 && p.keep_aspect == 1 && p.inside == 1 && p.src_w == 320 && p.src_h == 240);
    const mars_hip_shot_opts_t good = o;
    o.flags = 8u; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.flags = 0x80000000u; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.max_gap = -1; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.min_hits = -1; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.min_sharp = -1; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.min_mean = -1; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.max_mean = 256; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.min_mean = 200; o.max_mean = 100; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.src_w = 0; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;       /* MARS_SHOT_INSIDE needs the frame size */
    o.src_h = -5; CHECK(mars_shots_opts(&o, &p) == MARS_ERR_INVALID_FILE); o = good;
    o.flags = 0; o.src_w = o.src_h = 0; CHECK(mars_shots_opts(&o, &p) == MARS_OK);
    o.max_gap = 0x7fffffff; o.min_hits = 0x7fffffff; o.min_sharp = 0x7fffffff; CHECK(mars_shots_opts(&o, &p) == MARS_OK && p.max_gap == 0x7fffffff);
    return 0;
}

static int test_map(void) {
    int steps = -1;
    CHECK(mars_shots_map(0, 4, &steps) == MARS_ERR_INVALID_FILE && mars_shots_map(4, 0, &steps) == MARS_ERR_INVALID_FILE);
    CHECK(mars_shots_map(3, 4, &steps) == MARS_ERR_INVALID_TENSOR && steps == -1);
    CHECK(mars_shots_map(3, 12, &steps) == MARS_OK && steps == 4);
    CHECK(mars_shots_map(65535, 65535, &steps) == MARS_OK && steps == 1);
    CHECK(mars_shots_map(1, 0x7fffffff, &steps) == MARS_OK && steps == 0x7fffffff);
    /* both orders are bijections of [0, S * T) */
    for (int major = 0; major < 2; major++) {
        unsigned char seen[12] = {0};
        for (int b = 0; b < 3; b++)
            for (int t = 0; t < 4; t++) {
                const int f = mars_shots_frame(3, 4, major, b, t);
                CHECK(f >= 0 && f < 12 && !seen[f]);
                seen[f] = 1;
                CHECK(major ? (f / 4 == b && f % 4 == t) : (f % 3 == b && f / 3 == t));
            }
    }
    CHECK(mars_shots_frame(65535, 32768, 1, 65534, 32767) == 65534 * 32768 + 32767);
    return 0;
}

static int test_relayout(void) {
    /* 1 x 1, a row, a column, 5 x 3: exact-size buffers, so a byte too far is the sanitizer's */
    static const int sizes[4][2] = {{1, 1}, {7, 1}, {1, 6}, {5, 3}};
    for (int k = 0; k < 4; k++)
        for (int nhwc = 0; nhwc < 2; nhwc++) {
            const int tw = sizes[k][0], th = sizes[k][1], n = tw * th;
            int8_t *src = (int8_t *)malloc((size_t)n * 3);
            unsigned char *rgb = (unsigned char *)malloc((size_t)n * 3);
            CHECK(src && rgb);
            for (int i = 0; i < n * 3; i++) src[i] = (int8_t)(i * 37 - 128);
            src[0] = -128; src[n * 3 - 1] = 127;
            mars_shots_relayout(src, tw, th, nhwc, rgb);
            for (int y = 0; y < th; y++)
                for (int x = 0; x < tw; x++)
                    for (int c = 0; c < 3; c++) {
                        const int8_t v = nhwc ? src[(y * tw + x) * 3 + c] : src[(c * th + y) * tw + x];
                        CHECK(rgb[(y * tw + x) * 3 + c] == (unsigned char)(v + 128));
                    }
            CHECK(rgb[0] == 0 && (nhwc ? rgb[n * 3 - 1] : rgb[n * 3 - 1]) == 255);
            free(src);
            free(rgb);
        }
    return 0;
}

/* the object over host memory: the table and the plane are filled through the launch record the stand-in kept */
static int test_object(void) {
    mars_hip_shots_t *sh = NULL;
    CHECK(mars_hip_shots_create(0, 4, 5, 3, 1, &sh) == MARS_ERR_INVALID_FILE && mars_hip_shots_create(2, 4, 5, 3, 1, NULL) == MARS_ERR_INVALID_FILE);
    CHECK(mars_hip_shots_create(65536, 4, 5, 3, 1, &sh) == MARS_ERR_INVALID_TENSOR && mars_hip_shots_create(2, 257, 5, 3, 1, &sh) == MARS_ERR_INVALID_TENSOR);
    CHECK(mars_hip_shots_create(2, 4, 1281, 3, 1, &sh) == MARS_ERR_INVALID_TENSOR && mars_hip_shots_create(2, 4, 5, 1281, 1, &sh) == MARS_ERR_INVALID_TENSOR);
    for (int nhwc = 0; nhwc < 2; nhwc++) {
        const int tw = 5, th = 3, S = 2, slots = 4, nb = tw * th * 3;
        CHECK(mars_hip_shots_create(S, slots, tw, th, nhwc, &sh) == MARS_OK && sh);
        /* one call, so that the launch record names the object's tables */
        int8_t crops[2][45];
        mars_roi_t rois[2] = {{0, -1, 1, 1, 9, 9}, {1, -1, 1, 1, 9, 9}};
        float confs[2] = {0.5f, 0.5f};
        int cls[2] = {0, 0};
        mars_track_t tracks[2] = {{1, 1}, {2, 1}};
        mars_shot_t rec[2];
        mars_hip_shot_opts_t o;
        memset(&o, 0, sizeof(o));
        memset(crops, 0, sizeof(crops));
        memset(rec, 0, sizeof(rec)); /* (the stand-in launch writes nothing: the download copies an uninitialised scratch otherwise) */
        CHECK(mars_yolo_shot_lists(sh, &crops[0][0], rois, confs, cls, tracks, 2, 3, &o, rec) == MARS_ERR_INVALID_TENSOR && g_launches == nhwc);
        CHECK(mars_yolo_shot_lists(sh, &crops[0][0], rois, confs, cls, tracks, 0, 2, &o, rec) == MARS_ERR_INVALID_FILE);
        CHECK(mars_yolo_shot_lists(sh, NULL, rois, confs, cls, tracks, 2, 2, &o, rec) == MARS_ERR_INVALID_FILE);
        CHECK(mars_yolo_shot_lists(sh, &crops[0][0], rois, confs, cls, tracks, 70000, 2, &o, rec) == MARS_ERR_INVALID_TENSOR);
        CHECK(mars_yolo_shot_lists(sh, &crops[0][0], rois, confs, cls, tracks, 2, 2, &o, rec) == MARS_OK && g_launches == nhwc + 1);
        CHECK(g_launch.streams == S && g_launch.steps == 1 && g_launch.slots == slots && g_launch.n_crops == 2 && g_launch.tw == tw && g_launch.th == th);
        CHECK(g_launch.band_rows == 16 && g_launch.bands == 1 && g_launch.plane_stride == 48 && g_launch.crop_stride == 45 && g_launch.max_gap == 30);
        CHECK(mars_hip_shots_ms(sh) == 0.25f);
        mars_shot_slot_t *tab = (mars_shot_slot_t *)g_launch.table;
        int8_t *plane = g_launch.plane;
        /* stream 1: slot 0 LIVE, slot 2 DONE, slot 3 DONE; the planes hold a ramp */
        for (int s = 0; s < slots; s++)
            for (int i = 0; i < nb; i++) plane[((size_t)slots + s) * 48 + i] = (int8_t)(s * 50 + i - 128);
        tab[slots + 0].id = 11; tab[slots + 0].state = MARS_SHOT_LIVE;
        tab[slots + 2].id = 12; tab[slots + 2].state = MARS_SHOT_DONE; tab[slots + 2].score = 99;
        tab[slots + 3].id = 13; tab[slots + 3].state = MARS_SHOT_DONE;
        tab[slots + 1].id = 77; /* FREE with a stale field: reads back all zero */
        long long cnt[6];
        int live, done, step;
        CHECK(mars_hip_shots_read(sh, 1, cnt, &live, &done, &step) == MARS_OK && live == 1 && done == 2 && step == 0 && cnt[0] == 0);
        CHECK(mars_hip_shots_read(sh, 2, cnt, &live, &done, &step) == MARS_ERR_INVALID_TENSOR && mars_hip_shots_read(sh, 0, NULL, NULL, NULL, NULL) == MARS_OK);
        mars_shot_slot_t got[4];
        CHECK(mars_hip_shots_read_slots(sh, 1, got) == MARS_OK && got[1].id == 0 && got[0].id == 11 && got[2].score == 99);
        unsigned char *rgb = (unsigned char *)malloc((size_t)nb * 2);
        CHECK(rgb);
        CHECK(mars_hip_shots_read_pixels(sh, 1, 1, rgb) == MARS_ERR_INVALID_TENSOR && mars_hip_shots_read_pixels(sh, 1, 4, rgb) == MARS_ERR_INVALID_TENSOR);
        CHECK(mars_hip_shots_read_pixels(sh, 1, 2, rgb) == MARS_OK);
        for (int y = 0; y < th; y++)
            for (int x = 0; x < tw; x++)
                for (int c = 0; c < 3; c++) {
                    const int i = nhwc ? (y * tw + x) * 3 + c : (c * th + y) * tw + x;
                    CHECK(rgb[(y * tw + x) * 3 + c] == (unsigned char)(2 * 50 + i));
                }
        /* collect with cap 1: slot 2 handed over and freed, slot 3 stays; then flush and the rest */
        int n = -1;
        mars_shot_slot_t out[2];
        CHECK(mars_hip_shots_collect(sh, 1, out, rgb, -1, &n) == MARS_ERR_INVALID_FILE && mars_hip_shots_collect(sh, 1, NULL, NULL, 1, &n) == MARS_ERR_INVALID_FILE);
        CHECK(mars_hip_shots_collect(sh, 1, NULL, NULL, 0, &n) == MARS_OK && n == 2);
        CHECK(mars_hip_shots_collect(sh, 1, out, rgb, 1, &n) == MARS_OK && n == 2 && out[0].id == 12 && rgb[0] == (unsigned char)(2 * 50));
        CHECK(tab[slots + 2].state == MARS_SHOT_FREE && tab[slots + 2].id == 0 && tab[slots + 3].state == MARS_SHOT_DONE);
        CHECK(mars_hip_shots_flush(sh, 5) == MARS_ERR_INVALID_TENSOR && mars_hip_shots_flush(sh, -1) == MARS_OK);
        CHECK(mars_hip_shots_read(sh, 1, cnt, &live, &done, &step) == MARS_OK && live == 0 && done == 2 && cnt[0] == 1);
        CHECK(mars_hip_shots_collect(sh, 1, out, rgb, 2, &n) == MARS_OK && n == 2 && out[0].id == 11 && out[1].id == 13);
        CHECK(rgb[nb] == (unsigned char)(3 * 50) && rgb[nb * 2 - 1] == (unsigned char)(3 * 50 + (nhwc ? nb - 1 : nb - 1)));
        CHECK(mars_hip_shots_read(sh, 1, cnt, &live, &done, &step) == MARS_OK && live == 0 && done == 0 && cnt[0] == 1);
        CHECK(mars_hip_shots_reset(sh, 1) == MARS_OK && mars_hip_shots_read(sh, 1, cnt, NULL, NULL, NULL) == MARS_OK && cnt[0] == 0);
        CHECK(mars_hip_shots_reset(sh, 2) == MARS_ERR_INVALID_TENSOR);
        free(rgb);
        mars_hip_shots_free(sh);
        sh = NULL;
    }
    mars_hip_shots_free(NULL);
    CHECK(mars_hip_shots_ms(NULL) == -1.0f);
    CHECK(g_live_allocs == 0 && g_live_events == 0);
    return 0;
}

int main(void) {
    if (test_opts() || test_map() || test_relayout() || test_object()) return 1;
    printf("shots_host: ok\n");
    return 0;
}
