/*
 * align_fit.h -- "Aligned crops" (include/mars_hip.h): the least-squares similarity that carries the template onto a keypoint set -> the
 * skip decision, the Q16 sample frame, the mask of the keypoints that carried the fit and the enclosing rectangle.  ONE text for both
 * sides: csrc/host/mars_roi.c (gcc, mars_yolo_align_fit) and csrc/hip/roi.hip (hipcc, the select and rectangle kernels) compile this
 * file, so the host entry and the device tables cannot drift apart (tests/test_align_cpu.py holds the host side to its numpy
 * restatement, tests/test_gpu_align.py the device side to the host entry).  The enclosing rectangle of a rotated box lives here too: the
 * fit ends in it, and "Rotated crops" takes it from here.
 * Build with -ffp-contract=off: float32, every operation below is rounded on its own and in the order written -- sums in ascending j, `/`
 * the correctly rounded division and sqrtf the correctly rounded square root (both compilers' default), rintf round-to-nearest-even.
 */
#ifndef ALIGN_FIT_H
#define ALIGN_FIT_H
#include <math.h>

#include "mhip.h"

#ifdef __HIPCC__
#define ALIGN_FIT_FN __host__ __device__ static __forceinline__
#else
#define ALIGN_FIT_FN static inline
#endif

typedef struct { float x, y, v; } align_kpt_t;                                      /* mars_kpt_t */
typedef struct { int X0, Y0, Ux, Uy, Vx, Vy; unsigned used; int n_used; } align_t; /* mars_align_t */

ALIGN_FIT_FN int rot_q16(const float v) { return (int)rintf(v * 65536.0f); }

/* r = {x0, y0, x1, y1}: the integer rectangle around a box of sides we, he about (cx, cy) whose axis has |cos|, |sin| = ac, as, clipped to the frame */
ALIGN_FIT_FN void rot_enclose(const float cx, const float cy, const float we, const float he, const float ac, const float as, const int W, const int H,
                              int r[4]) {
    const float ex = ((we * ac) + (he * as)) * 0.5f, ey = ((we * as) + (he * ac)) * 0.5f;
    r[0] = (int)floorf(fmaxf(cx - ex, 0.0f)); r[2] = (int)ceilf(fminf(cx + ex, (float)W));
    r[1] = (int)floorf(fmaxf(cy - ey, 0.0f)); r[3] = (int)ceilf(fminf(cy + ey, (float)H));
}

/* 0 = skipped: `a` and the rectangle are then all zeros */
ALIGN_FIT_FN int align_fit(const align_kpt_t *kp, const mhip_roi_t *p, align_t *a, int r[4]) {
    const align_t none = {0, 0, 0, 0, 0, 0, 0u, 0};
    *a = none;
    r[0] = r[1] = r[2] = r[3] = 0;
    unsigned used = 0u;
    int cnt = 0;
    float sqx = 0.0f, sqy = 0.0f, spx = 0.0f, spy = 0.0f;
    for (int j = 0; j < p->num_kpt; j++) {
        if (!((p->use >> j) & 1u)) continue;
        const align_kpt_t k = kp[j];
        if (!(k.v >= p->min_vis)) continue; /* (a NaN visibility does not take part) */
        if (!(isfinite(k.x) && isfinite(k.y) && isfinite(k.v))) return 0;
        used |= 1u << j;
        cnt++;
        sqx = sqx + p->tmpl[j][0]; sqy = sqy + p->tmpl[j][1];
        spx = spx + k.x; spy = spy + k.y;
    }
    if (cnt < 2) return 0;
    const float n = (float)cnt;
    const float qmx = sqx / n, qmy = sqy / n, pmx = spx / n, pmy = spy / n;
    float A = 0.0f, B = 0.0f, D = 0.0f;
    for (int j = 0; j < p->num_kpt; j++) {
        if (!((used >> j) & 1u)) continue;
        const align_kpt_t k = kp[j];
        const float dqx = p->tmpl[j][0] - qmx, dqy = p->tmpl[j][1] - qmy, dpx = k.x - pmx, dpy = k.y - pmy;
        A = A + ((dqx * dpx) + (dqy * dpy));
        B = B + ((dqx * dpy) - (dqy * dpx));
        D = D + ((dqx * dqx) + (dqy * dqy));
    }
    if (!(D > 0.0f)) return 0;
    const float fa = A / D, fb = B / D;
    if (!(isfinite(fa) && isfinite(fb))) return 0;
    const float ux = ((float)p->tw * 0.5f) - qmx, uy = ((float)p->th * 0.5f) - qmy;
    const float cx = pmx + ((fa * ux) - (fb * uy)), cy = pmy + ((fb * ux) + (fa * uy));
    const float ae = fa * p->expand, be = fb * p->expand;
    const float s = sqrtf((ae * ae) + (be * be));
    const float we = s * (float)p->tw, he = s * (float)p->th;
    if (!(we >= (float)p->min_size && he >= (float)p->min_size && we <= 32768.0f && he <= 32768.0f)) return 0; /* (a NaN side is skipped) */
    if (!(cx >= 0.0f && cx <= (float)p->w && cy >= 0.0f && cy <= (float)p->h)) return 0;                       /* (a NaN centre is outside) */
    const float ha = ae * 0.5f, hb = be * 0.5f;
    a->Ux = rot_q16(ha); a->Uy = rot_q16(hb); a->Vx = rot_q16(-hb); a->Vy = rot_q16(ha);
    a->X0 = rot_q16(cx - 0.5f); a->Y0 = rot_q16(cy - 0.5f);
    a->used = used; a->n_used = cnt;
    rot_enclose(cx, cy, we, he, fabsf(ae) / s, fabsf(be) / s, p->w, p->h, r);
    return 1;
}
#endif
