/*
 * stage_block.c -- the tail stages' shared host helpers (csrc/host/mars_stage.c) on the CPU, built with ASan + UBSan by
 * tests/test_stage_cpu.py.  The device layer is stood in for: memory is host malloc, events are counters, every call is logged as one
 * letter (S sync, M malloc, F free, U upload, D download, E event created, X event destroyed), and a knob makes the N-th allocation,
 * upload or synchronise fail.  Exit status 0 and "stage_block: ok" when every check holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mars_internal.h"

static char g_log[256];
static int g_nlog, g_live_allocs, g_live_events;
static int g_fail_malloc, g_fail_upload, g_fail_sync; /* N > 0: the N-th call from now fails */

static void note(char c) {
    if (g_nlog < (int)sizeof(g_log) - 1) g_log[g_nlog++] = c;
    g_log[g_nlog] = 0;
}
static void log_reset(void) { g_nlog = 0; g_log[0] = 0; }
static int countdown(int *n) { return *n > 0 && --*n == 0; }

/* ---- the device layer mars_stage.c calls */
int mhip_ready(void) { return 1; }
int mhip_sync(void) { note('S'); return countdown(&g_fail_sync) ? -1 : 0; }
void *mhip_malloc(size_t bytes) {
    note('M');
    if (countdown(&g_fail_malloc)) return NULL;
    g_live_allocs++;
    return malloc(bytes ? bytes : 1);
}
void mhip_free(void *p) { note('F'); g_live_allocs--; free(p); }
int mhip_h2d_async(void *dst, const void *src, size_t bytes) {
    note('U');
    if (countdown(&g_fail_upload)) return -1;
    memcpy(dst, src, bytes);
    return 0;
}
int mhip_d2h_async(void *dst, const void *src, size_t bytes) { note('D'); memcpy(dst, src, bytes); return 0; }
void *mhip_event_create(void) { note('E'); g_live_events++; return malloc(1); }
void *mhip_event_create_sync(void) { return mhip_event_create(); }
void mhip_event_destroy(void *ev) { note('X'); g_live_events--; free(ev); }
int mhip_event_record(void *ev) { (void)ev; return 0; }
float mhip_event_elapsed_ms(void *a, void *b) { (void)a; (void)b; return 0.25f; }
void mhip_select_aux(int on) { (void)on; }
void mhip_select_stream(int which) { (void)which; }
int mhip_stream_wait(int which, void *ev) { (void)which; (void)ev; return 0; }
int mhip_label_scatter(const void *rois, const int *n_out, int slots, const void *top, int top_k, void *labels, int det_frames, int det_cap) {
    (void)rois; (void)n_out; (void)slots; (void)top; (void)top_k; (void)labels; (void)det_frames; (void)det_cap;
    return 0;
}
/* ... and the rest of the library it names (not exercised here) */
int mars_tensor_chw(const mars_tensor_t *d, int *c, int *h, int *w) { (void)d; (void)c; (void)h; (void)w; return -1; }
int mars_locate_i8(const mars_model_ext_t *m, int T, int ch, int hh, int ww, int any_writer, int *buf, int *off, int *pix_step, int *ch_step) {
    (void)m; (void)T; (void)ch; (void)hh; (void)ww; (void)any_writer; (void)buf; (void)off; (void)pix_step; (void)ch_step;
    return -1;
}
void mars_roi_release(mars_model_ext_t *m) { (void)m; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "stage_block: line %d: %s (log \"%s\")\n", __LINE__, #cond, g_log); return 1; } } while (0)

static int test_layout(void) {
    /* 1 -> 256, 256 -> 256, 257 -> 512, 0 -> 0 (a part without bytes shares its successor's offset), 1000 -> 1024 */
    const size_t sz[5] = {1, 256, 257, 0, 1000};
    size_t off[5];
    CHECK(mars_block_layout(sz, 5, off) == 256 + 256 + 512 + 0 + 1024);
    CHECK(off[0] == 0 && off[1] == 256 && off[2] == 512 && off[3] == 1024 && off[4] == 1024);
    CHECK(mars_block_layout(sz, 0, off) == 0);
    return 0;
}

static int test_reserve_release_fetch(void) {
    mars_block_t b;
    memset(&b, 0, sizeof(b));
    int fresh = -1;
    log_reset();
    CHECK(mars_block_ms(&b) == -1.0f);
    CHECK(mars_block_fetch(&b, NULL, 0, NULL) == MARS_ERR_INVALID_TENSOR && g_nlog == 0); /* nothing to fetch, no device call */
    CHECK(mars_block_reserve(&b, 1024, 1, &fresh) == MARS_OK && fresh == 1);
    CHECK(!strcmp(g_log, "SMEE") && b.dev && b.bytes == 1024 && b.frames == 0 && b.ev[0] && b.ev[1]);
    CHECK(mars_block_ms(&b) == -1.0f); /* events, but no call yet */
    b.frames = 3;
    CHECK(mars_block_ms(&b) == 0.25f);
    /* large enough: no device call at all, the contents stay */
    void *was = b.dev;
    memset(b.dev, 0x5A, 1024);
    log_reset();
    CHECK(mars_block_reserve(&b, 1000, 1, &fresh) == MARS_OK && fresh == 0 && g_nlog == 0 && b.dev == was && b.frames == 3 && b.bytes == 1024);
    /* fetch: synchronise, one download per destination, synchronise; a NULL destination is skipped */
    unsigned char got[16];
    int pending = 1;
    const mars_block_part_t parts[3] = {{NULL, 0, 1024}, {got, 512, sizeof(got)}, {NULL, 0, 1 << 20}};
    CHECK(mars_block_fetch(&b, parts, 3, &pending) == MARS_OK && !strcmp(g_log, "SDS") && pending == 0 && got[0] == 0x5A && got[15] == 0x5A);
    log_reset();
    g_fail_sync = 1;
    pending = 1;
    CHECK(mars_block_fetch(&b, parts, 3, &pending) == MARS_ERR_LAYER_FAILED && !strcmp(g_log, "S") && pending == 1);
    /* growing: synchronise BEFORE the old block is freed; the frames of the last call are forgotten, the events are kept */
    log_reset();
    CHECK(mars_block_reserve(&b, 4096, 1, &fresh) == MARS_OK && fresh == 1 && !strcmp(g_log, "SFM") && b.bytes == 4096 && b.frames == 0);
    /* a synchronise that fails leaves the block alone */
    b.frames = 2;
    log_reset();
    g_fail_sync = 1;
    CHECK(mars_block_reserve(&b, 8192, 1, &fresh) == MARS_ERR_LAYER_FAILED && !strcmp(g_log, "S") && b.bytes == 4096 && b.frames == 2 && fresh == 0);
    /* an allocation that fails: the record reads as empty, and the next reserve succeeds */
    log_reset();
    g_fail_malloc = 1;
    CHECK(mars_block_reserve(&b, 8192, 1, &fresh) == MARS_ERR_ALLOC_FAILED && !strcmp(g_log, "SFM") && fresh == 1);
    CHECK(b.dev == NULL && b.bytes == 0 && b.frames == 0);
    CHECK(mars_block_fetch(&b, parts, 3, NULL) == MARS_ERR_INVALID_TENSOR && mars_block_ms(&b) == -1.0f);
    log_reset();
    CHECK(mars_block_reserve(&b, 8192, 1, &fresh) == MARS_OK && fresh == 1 && !strcmp(g_log, "SM") && b.dev && b.bytes == 8192);
    /* release twice */
    log_reset();
    mars_block_release(&b);
    CHECK(!strcmp(g_log, "FXX") && !b.dev && !b.bytes && !b.frames && !b.ev[0] && !b.ev[1]);
    mars_block_release(&b);
    CHECK(!strcmp(g_log, "FXX") && g_live_allocs == 0 && g_live_events == 0);
    /* a block without events never gets any */
    CHECK(mars_block_reserve(&b, 64, 0, NULL) == MARS_OK && !b.ev[0] && !b.ev[1]);
    b.frames = 1;
    CHECK(mars_block_ms(&b) == -1.0f);
    mars_block_release(&b);
    CHECK(g_live_allocs == 0 && g_live_events == 0);
    return 0;
}

static int test_side_arrays(void) {
    mars_det_side_t s;
    memset(&s, 0, sizeof(s));
    int rec[2] = {0, 0};
    log_reset();
    CHECK(mars_side_fetch(&s, rec, 8) == MARS_ERR_INVALID_TENSOR && g_nlog == 0);
    CHECK(mars_side_reserve(&s, 2, 8) == MARS_OK && !strcmp(g_log, "SM") && s.cap == 2 && s.frames == 0);
    s.frames = 2;
    log_reset();
    CHECK(mars_side_reserve(&s, 1, 8) == MARS_OK && g_nlog == 0 && s.frames == 2); /* only ever grown */
    CHECK(mars_side_reserve(&s, 3, 8) == MARS_OK && !strcmp(g_log, "SFM") && s.cap == 3 && s.frames == 0);
    g_fail_malloc = 1;
    CHECK(mars_side_reserve(&s, 4, 8) == MARS_ERR_ALLOC_FAILED && !s.dev && !s.cap && !s.frames);
    CHECK(mars_side_reserve(&s, 1, 8) == MARS_OK && s.cap == 1);
    memset(s.dev, 0, (size_t)MARS_YOLO_MAX_DET * 8);
    s.frames = 1;
    unsigned char *out = (unsigned char *)malloc((size_t)MARS_YOLO_MAX_DET * 8);
    CHECK(out != NULL);
    log_reset();
    CHECK(mars_side_fetch(&s, out, 8) == MARS_OK && !strcmp(g_log, "SDS"));
    free(out);
    mars_side_release(&s);
    mars_side_release(&s);
    CHECK(g_live_allocs == 0);
    return 0;
}

static int test_tables(void) {
    mars_lut_cache_t c;
    memset(&c, 0, sizeof(c));
    float dev[2 * 4], tab[2 * 4] = {1, 2, 3, 4, 5, 6, 7, 8};
    float key[4][2] = {{0.5f, 0.0f}, {0.25f, 2.0f}, {0, 0}, {0, 0}};
    memset(dev, 0, sizeof(dev));
    log_reset();
    CHECK(mars_lut_stale(&c, 2, key));
    /* the safe order: synchronise, nothing marked up, upload, synchronise, then the keys */
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_OK && !strcmp(g_log, "SUS") && c.n == 2 && !memcmp(dev, tab, sizeof(tab)));
    CHECK(!mars_lut_stale(&c, 2, key));
    log_reset();
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_OK && g_nlog == 0); /* same keys, bit for bit: nothing happens */
    /* -0.0 is another key than 0.0 */
    key[0][1] = -0.0f;
    CHECK(mars_lut_stale(&c, 2, key));
    /* a failed upload leaves no table marked up; the next call uploads again */
    tab[0] = 9;
    g_fail_upload = 1;
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_ERR_LAYER_FAILED && !strcmp(g_log, "SU") && c.n == 0);
    key[0][1] = 0.0f; /* even the keys that were up before are not taken for fresh now */
    CHECK(mars_lut_stale(&c, 2, key));
    log_reset();
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_OK && !strcmp(g_log, "SUS") && c.n == 2 && dev[0] == 9);
    /* a failed synchronise in front of the upload keeps what is up; one behind it does not */
    key[1][0] = 0.125f;
    log_reset();
    g_fail_sync = 1;
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_ERR_LAYER_FAILED && !strcmp(g_log, "S") && c.n == 2);
    log_reset();
    g_fail_sync = 2;
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_ERR_LAYER_FAILED && !strcmp(g_log, "SUS") && c.n == 0);
    /* another head count is stale whatever the keys */
    CHECK(mars_lut_refresh(&c, dev, 2, key, tab, 4) == MARS_OK && c.n == 2 && mars_lut_stale(&c, 1, key) && !mars_lut_stale(&c, 2, key));
    return 0;
}

int main(void) {
    if (test_layout() || test_reserve_release_fetch() || test_side_arrays() || test_tables()) return 1;
    printf("stage_block: ok\n");
    return 0;
}
