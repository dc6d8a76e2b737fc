/* conv_i8_policy.c -- which launch variant the int8 convolution family picks, over a fixed grid of layer descriptors.
 * Built by tests/test_conv_i8_policy_cpu.py against the in-tree libnna_mars.so; needs no device: every function called
 * here is host arithmetic over the descriptor (pointer fields are dummies, nothing dereferences them).
 *
 * One line per descriptor, one column per knob setting (see main):
 *   <mhip_conv_i8_variants list>|<seg pre post split both chain predicates>/<mhip_conv_i8_code>
 * -DNO_CODE leaves the /<code> out (a library from before mhip_conv_i8_code existed: that is how the expected
 * output tests/golden/conv_i8_policy.txt was recorded). */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mhip.h"

#ifdef NO_CODE
#define mhip_conv_i8_code(p) 0
#endif
#define PTR(n) ((void *)(uintptr_t)(0x10000 + 0x1000 * (n)))

static const int IN_C[] = {16, 32, 64, 128, 256, 512}, OUT_C[] = {16, 32, 64, 128, 255, 256}, MAPS[] = {20, 40, 80, 160},
                 FRAMES[] = {1, 8, 256};

/* k x k convolution onto a map x map output; table: 0 none, 1 lut, 2 lut + lut2 */
static mhip_conv_i8_t layer(int in_c, int out_c, int k, int stride, int map, int frames, int table) {
    mhip_conv_i8_t p;
    memset(&p, 0, sizeof p);
    p.in = PTR(1); p.out = PTR(2); p.w = PTR(3); p.bias = PTR(4); p.w_rows = PTR(5);
    p.lut = table >= 1 ? PTR(6) : NULL;
    p.lut2 = table >= 2 ? PTR(7) : NULL;
    p.frames = frames;
    p.in_h = p.in_w = map * stride; p.in_c = in_c;
    p.out_h = p.out_w = map; p.out_c = out_c;
    p.kh = p.kw = k; p.stride_h = p.stride_w = stride; p.pad_top = p.pad_left = k / 2;
    mhip_conv_i8_pack_geom(in_c, k, out_c, &p.row_pad, &p.oc_pad, NULL);
    p.in_stride = (size_t)p.in_h * p.in_w * in_c;
    p.out_stride = (size_t)map * map * out_c;
    p.cs = 0.001f; p.safe = 1;
    for (int i = 0; i < 4; i++) p.seg_c0[i] = 0x7fffffff;
    return p;
}
static void two_segments(mhip_conv_i8_t *p) { /* the input as a never-materialised concat of two halves */
    p->nseg = 2;
    for (int i = 0; i < 2; i++) {
        p->seg_in[i] = PTR(8 + i); p->seg_c[i] = p->in_c / 2; p->seg_c0[i] = i * (p->in_c / 2);
        p->seg_stride[i] = (size_t)p->in_h * p->in_w * (p->in_c / 2);
    }
}

/* what one knob setting answers for one descriptor: "<variants list>|<seg pre post split both chain>", and mhip_conv_i8_code */
#define MAXDESC 400
#define NKNOBS 9
static char g_label[MAXDESC][64], g_rec[NKNOBS][MAXDESC][96];
static int g_code[NKNOBS][MAXDESC], g_knob, g_ndesc;

/* b = a's partner of a cv1 + cv2 pair (NULL: a copy of a with its own output), d = the 1x1 chained to side 1 (NULL: 64 -> 64 on a's output) */
static void emit(const char *kind, const mhip_conv_i8_t *a, const mhip_conv_i8_t *b, const mhip_conv_i8_t *d) {
    mhip_conv_i8_t b0 = *a, d0 = layer(64, 64, 1, 1, a->out_h, a->frames, 2);
    b0.out = PTR(12);
    d0.in = a->out; d0.in_stride = a->out_stride; d0.out = PTR(13);
    if (!b) b = &b0;
    if (!d) d = &d0;
    const int i = g_ndesc++;
    if (i >= MAXDESC) return;
    int codes[32];
    const int n = mhip_conv_i8_variants(a, codes, 32);
    snprintf(g_label[i], sizeof g_label[i], "%s c%d o%d k%d s%d m%d f%d t%d a%d n%d", kind, a->in_c, a->out_c, a->kh, a->stride_h, a->out_h,
             a->frames, a->lut2 ? 2 : (a->lut ? 1 : 0), a->add != NULL, a->nseg > 1 ? a->nseg : 1);
    char *r = g_rec[g_knob][i];
    int len = 0;
    for (int j = 0; j < n; j++) len += snprintf(r + len, 96 - len, "%s%d", j ? "," : "", codes[j]);
    snprintf(r + len, 96 - len, "|%d%d%d%d%d%d", mhip_conv_i8_seg_ok(a), mhip_conv_i8_pre_ok(a), mhip_conv_i8_post_ok(a), mhip_conv_i8_split_ok(a),
             mhip_conv_i8_both_ok(a, b), mhip_conv_i8_both_chain_ok(a, b, d, 1));
    g_code[g_knob][i] = mhip_conv_i8_code(a);
}

#define N(a) ((int)(sizeof(a) / sizeof((a)[0])))
/* the grids are pruned to every STEP-th point (STEP prime to the grid's dimensions: every value of every axis stays) */
#define EVERY(step) if (count++ % (step) != 0) continue

static void grid(void) {
    int count = 0;
    /* plain layers, with the residual Add where it is legal */
    for (int ic = 0; ic < N(IN_C); ic++)
        for (int oc = 0; oc < N(OUT_C); oc++)
            for (int k = 1; k <= 3; k += 2)
                for (int s = 1; s <= 2; s++)
                    for (int m = 0; m < N(MAPS); m++)
                        for (int f = 0; f < N(FRAMES); f++)
                            for (int t = 0; t <= 2; t++)
                                for (int add = 0; add <= 1; add++) {
                                    if (add && OUT_C[oc] % 16) continue;
                                    EVERY(113);
                                    mhip_conv_i8_t p = layer(IN_C[ic], OUT_C[oc], k, s, MAPS[m], FRAMES[f], t);
                                    if (add) { p.add = PTR(10); p.add_s_conv = p.add_s_other = 0.5f; p.add_inv = 1.0f; }
                                    emit("plain", &p, NULL, NULL);
                                }
    /* the deep 3x3 stride-1 layers the whole-row form competes for, all of them */
    for (int ic = 3; ic < N(IN_C); ic++)
        for (int m = 0; m < 2; m++)
            for (int f = 0; f < N(FRAMES); f++) {
                mhip_conv_i8_t p = layer(IN_C[ic], IN_C[ic], 3, 1, MAPS[m], FRAMES[f], 2);
                emit("deep", &p, NULL, NULL);
            }
    /* 1x1 over a never-materialised concat */
    count = 0;
    for (int ic = 2; ic < N(IN_C); ic++)
        for (int oc = 0; oc < N(OUT_C); oc++)
            for (int m = 0; m < N(MAPS); m++)
                for (int f = 0; f < N(FRAMES); f++)
                    for (int t = 0; t <= 2; t++) {
                        EVERY(29);
                        mhip_conv_i8_t p = layer(IN_C[ic], OUT_C[oc], 1, 1, MAPS[m], FRAMES[f], t);
                        two_segments(&p);
                        emit("seg", &p, NULL, NULL);
                    }
    /* fused bottleneck: a 1x1 (in_c -> in_c) ahead of the 3x3 */
    count = 0;
    for (int ic = 1; ic <= 2; ic++)
        for (int oc = 1; oc <= 2; oc++)
            for (int m = 0; m < N(MAPS); m++)
                for (int f = 0; f < N(FRAMES); f++)
                    for (int add = 0; add <= 1; add++) {
                        EVERY(5);
                        mhip_conv_i8_t p = layer(IN_C[ic], OUT_C[oc], 3, 1, MAPS[m], FRAMES[f], 2);
                        p.pre_w = PTR(14); p.pre_bias = PTR(15); p.pre_lut2 = PTR(16); p.pre_cs = 0.002f;
                        if (add) { p.add = PTR(10); p.add_s_conv = p.add_s_other = 0.5f; p.add_inv = 1.0f; }
                        emit("pre", &p, NULL, NULL);
                    }
    /* fused cv3: a 1x1 (2c -> 2c) behind the 3x3 of c channels */
    count = 0;
    for (int ic = 1; ic <= 2; ic++)
        for (int oc = 1; oc <= 2; oc++)
            for (int m = 0; m < N(MAPS); m++)
                for (int f = 0; f < N(FRAMES); f++)
                    for (int add = 0; add <= 1; add++) {
                        EVERY(5);
                        mhip_conv_i8_t p = layer(IN_C[ic], OUT_C[oc], 3, 1, MAPS[m], FRAMES[f], 2);
                        p.post_w = PTR(17); p.post_lut2 = PTR(18); p.post_cs = 0.002f; p.post_in = PTR(19);
                        p.post_in_stride = p.out_stride; p.post_out = PTR(20); p.post_out_stride = 2 * p.out_stride;
                        if (add) { p.add = PTR(10); p.add_s_conv = p.add_s_other = 0.5f; p.add_inv = 1.0f; }
                        emit("post", &p, NULL, NULL);
                    }
    /* fused cv1 + cv2 pair behind a 3x3 of 64 channels, with and without the 1x1 chained to side 1 */
    count = 0;
    for (int ic = 0; ic <= 3; ic++)
        for (int s = 1; s <= 2; s++)
            for (int m = 0; m < N(MAPS); m++)
                for (int f = 0; f < N(FRAMES); f++)
                    for (int chain = 0; chain <= 1; chain++) {
                        EVERY(7);
                        mhip_conv_i8_t p = layer(IN_C[ic], 64, 3, s, MAPS[m], FRAMES[f], 2);
                        p.split_w = PTR(21);
                        for (int i = 0; i < 2; i++) {
                            p.split_lut2[i] = PTR(22 + i); p.split_cs[i] = 0.002f; p.split_out[i] = PTR(24 + i);
                            p.split_out_stride[i] = (size_t)MAPS[m] * MAPS[m] * 32;
                        }
                        if (chain) {
                            p.chain_side = 1; p.chain_w = PTR(26); p.chain_lut2 = PTR(27); p.chain_cs = 0.002f; p.chain_out = PTR(28);
                            p.chain_out_stride = (size_t)MAPS[m] * MAPS[m] * 32;
                        }
                        emit(chain ? "chain" : "split", &p, NULL, NULL);
                    }
    /* the one-tile pair form: two 1x1s of 64 (128: the wide form) channels over one input, and the 64 -> 64 1x1 behind side 1 */
    count = 0;
    for (int ic = 2; ic <= 4; ic++)
        for (int oc = 2; oc <= 3; oc++)
            for (int seg = 0; seg <= 1; seg++)
                for (int m = 0; m < N(MAPS); m++)
                    for (int f = 0; f < N(FRAMES); f++) {
                        EVERY(7);
                        mhip_conv_i8_t a = layer(IN_C[ic], OUT_C[oc], 1, 1, MAPS[m], FRAMES[f], 2);
                        if (seg) two_segments(&a);
                        mhip_conv_i8_t b = a, d = layer(OUT_C[oc], OUT_C[oc], 1, 1, MAPS[m], FRAMES[f], 2);
                        b.out = PTR(29); b.w = PTR(30);
                        d.in = a.out; d.in_stride = a.out_stride; d.out = PTR(31);
                        emit("pair", &a, &b, &d);
                    }
}

/* One line per descriptor: the descriptor, then one column per knob setting in the order of the first line, "=" where the
 * setting answers what the default knobs answer; with mhip_conv_i8_code behind a "/" in every column */
int main(void) {
    static const struct { const char *key; int value; } KNOBS[NKNOBS] = {{NULL, 0}, {"persist", 0}, {"bpx", 256}, {"stages", 3}, {"wres", 0},
                                                                         {"small_batch", 0}, {"rows", 0}, {"variant", 14}, {"both_wide", 1}};
    printf("# knobs: default");
    for (int i = 1; i < NKNOBS; i++) printf(" %s=%d", KNOBS[i].key, KNOBS[i].value);
    printf("\n");
    for (g_knob = 0; g_knob < NKNOBS; g_knob++) {
        const char *key = KNOBS[g_knob].key;
        int before = 0;
        if (key && (mhip_conv_i8_tune_get(key, &before) || mhip_conv_i8_tune(key, KNOBS[g_knob].value))) return 2;
        g_ndesc = 0;
        grid();
        if (g_ndesc > MAXDESC) return 3;
        if (key && mhip_conv_i8_tune(key, before)) return 2;
    }
    for (int i = 0; i < g_ndesc; i++) {
        printf("%s", g_label[i]);
        for (int k = 0; k < NKNOBS; k++) {
            printf(" %s", k && !strcmp(g_rec[k][i], g_rec[0][i]) ? "=" : g_rec[k][i]);
#ifndef NO_CODE
            printf("/%d", g_code[k][i]);
#endif
        }
        printf("\n");
    }
    return 0;
}
