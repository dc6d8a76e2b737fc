// seg_native.hip -- instance masks in frame pixels on gfx950: the masks of seg.hip on an out_w x out_h grid, every output pixel's centre
// carried through the letterbox into prototype coordinates, the int32 coefficient . prototype dots of its four neighbours blended with
// integer weights of 1/256, one float32 product and one compare, cut to the detection's rectangle in output pixels.
//
// include/mars_hip.h ("Instance masks in frame pixels") states the arithmetic.  Two launches:
//   seg_select_kernel   of seg.hip, unchanged: with the output grid where it takes the prototype size and the base grid where it takes the
//                       graph input, its rectangle rule is the one of this stage.
//   seg_native_kernel   grid (span, slot, frame), four wavefronts.  A span = 64 rows of one slot's mask.  Its rows above and below the
//                       slot's rectangle (all of them for an unused slot) are zero-filled as contiguous runs of words; the rows inside
//                       are walked in bands of 16 rows x tiles of 8 words (256 pixels), and a tile left or right of the rectangle is
//                       zero-filled too: the arithmetic is proportional to the boxes' area, not the frame's.  (One workgroup per tile
//                       and one per band of 16 rows were measured first: the empty workgroups' short fills, each behind a load of the
//                       record, were the bound.  DESIGN.md has the figures.)  A span that meets the rectangle gathers the slot's
//                       coefficient row once (64 bytes, zero from nm on, through the prediction index the tail kept); then every tile
//                       that meets it
//                         1. reads the prototype footprint of (tile ^ rectangle) from the host's tap tables (no 64-bit division on the
//                            device); up-scaling makes the taps move by at most one per output pixel, so the footprint is at most the
//                            tile's size + 1 per axis;
//                         2. computes the footprint's int32 dots once into LDS: v_dot4_i32_i8 over 16-byte channel groups;
//                         3. gives every wavefront a 64-pixel column strip: a lane keeps its column's two taps and weight (asked for
//                            before the dots are made) and walks the tile's rows, whose taps wait in LDS beside the dots: four dots per pixel, the horizontal blend in int32 (|.| <= 2^28), the vertical one in
//                            int64 (|S| <= 2^36), (float)S * s16 > logit_min;
//                         4. a ballot turns the 64 lanes into two words; lanes 0 and 1 store one each and count its bits.
//                       The span's count goes into the record's area with ONE integer atomicAdd: the order of the adds cannot show.
//                       Every word of every slot is written exactly once, padding bits zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "seg_common.hpp"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define SGN_THREADS 256
#define SGN_SPAN 64                    // rows of a workgroup
#define SGN_ROWS 16                    // rows of a tile
#define SGN_WORDS 8                    // words of a tile's row: two per wavefront
#define SGN_FP_H (SGN_ROWS + 2)        // the footprint the LDS holds (one more than up-scaling can ask for)
#define SGN_FP_W (SGN_WORDS * 32 + 2)

// sg_load16 for a lane's own pixel inside a loop: the channel pointer is stepped, so the planes' layout costs one uniform step and not
// sixteen uniform offsets (which, hoisted out of the footprint loop, spilled scalar registers)
__device__ __forceinline__ sg_v4i sgn_load16(const int8_t *q, const int kb, const int nm, const int ch_step) {
    sg_v4i v = {0, 0, 0, 0};
    if (ch_step == 1 && kb + 16 <= nm) {
        __builtin_memcpy(&v, q + kb, 16); // any alignment is served
        return v;
    }
    const int8_t *qq = q + (size_t)kb * ch_step;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int b = kb + j < nm ? (int)*qq & 255 : 0;
        v[j >> 2] |= b << (8 * (j & 3));
        if (kb + j + 1 < nm) qq += ch_step; // (never beyond the last channel's plane)
    }
    return v;
}

__global__ __launch_bounds__(SGN_THREADS) void seg_native_kernel(const mhip_seg_native_t p) {
    __shared__ int dots[SGN_FP_H * SGN_FP_W];
    __shared__ __attribute__((aligned(16))) int8_t a_s[64];
    __shared__ int ytap[3][SGN_ROWS]; // of the band's rows: the two dot rows' offsets in `dots` and the weight
    __shared__ int area_s;
    const mhip_seg_t &g = p.seg;
    const int f = blockIdx.z, slot = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ow = p.out_w, oh = p.out_h, pitch = (ow + 31) >> 5, tiles_x = (pitch + SGN_WORDS - 1) / SGN_WORDS;
    const int R0 = blockIdx.x * SGN_SPAN, R1 = min(R0 + SGN_SPAN, oh); // the workgroup's rows
    mask_t *rec = (mask_t *)g.recs + (size_t)f * g.max_per_frame + slot;
    uint32_t *words = g.words + ((size_t)f * g.max_per_frame + slot) * ((size_t)oh * pitch);
    const int det = rec->det;
    const bool sel = det >= 0 && det < g.det_cap;
    const int x0 = rec->x0, y0 = rec->y0, x1 = min(rec->x1, ow), y1 = min(rec->y1, oh);
    const bool hit = sel && x0 < x1 && max(R0, y0) < min(R1, y1);
    const int sy0 = hit ? max(R0, y0) : R1, sy1 = hit ? min(R1, y1) : R1; // the span's rows inside the rectangle
    // the rows above and below them: whole rows, two contiguous runs of words (an unused slot, a span off the rectangle: everything)
    for (int i = R0 * pitch + tid; i < sy0 * pitch; i += SGN_THREADS) words[i] = 0u;
    for (int i = sy1 * pitch + tid; i < R1 * pitch; i += SGN_THREADS) words[i] = 0u;
    if (!hit) return;
    // one base and five offsets: [ia][ib][w1] of the columns, then of the rows
    const int *T = p.taps;
    const int oxb = ow, oxw = 2 * ow, oya = 3 * ow, oyb = oya + oh, oyw = oyb + oh;
    // the slot's origin (uniform) and its coefficient row
    int head = -1, cell = 0;
    {
        int pr = g.pred[(size_t)f * g.det_cap + det];
        if (pr >= 0) {
            int k = 0;
            while (k < g.nheads && pr >= g.cells[k]) pr -= g.cells[k++];
            if (k < g.nheads) { head = k; cell = pr; }
        }
    }
    if (tid < 4) {
        sg_v4i v = {0, 0, 0, 0};
        if (head >= 0) v = sg_load16(g.coef[head] + (size_t)f * g.coef_frame_stride[head] + (size_t)cell * g.coef_pix_step[head], tid * 16, g.nm, g.coef_ch_step[head]);
        *(sg_v4i *)&a_s[tid * 16] = v;
    }
    if (tid == 0) area_s = 0;
    __syncthreads();
    const float s16 = head >= 0 ? g.scale[head] : 0.0f;
    const int8_t *pf = g.proto + (size_t)f * g.proto_frame_stride;
    int area = 0;
    for (int Y0 = sy0; Y0 < sy1; Y0 += SGN_ROWS) // bands of 16 rows, every one of them inside the rectangle
    for (int tx = 0; tx < tiles_x; tx++) {
        const int Y1 = min(Y0 + SGN_ROWS, sy1);
        // the footprint's rows: prototype rows fy0 .. fy0 + FH - 1.  With the host's up-scaling tables FH <= 17 and FW <= 257, so the caps at
        // SGN_FP_H / SGN_FP_W (and the clamps of every tap into the footprint) never act: they only keep every address inside the prototype
        // tensor and the LDS whatever a table says.  Under any other table the bits would be wrong without an error: mhip_seg_native's
        // callers pass tables of mars_yolo_mask_taps and nothing else.
        const int fy0 = min(max(T[oya + Y0], 0), g.ph - 1), FH = min(min(max(T[oyb + Y1 - 1], fy0), g.ph - 1) - fy0 + 1, SGN_FP_H);
        const int W0 = tx * SGN_WORDS, W1 = min(W0 + SGN_WORDS, pitch);
        const int cx0 = max(W0 * 32, x0), cx1 = min(W1 * 32, x1); // the tile's columns inside the rectangle
        if (cx0 >= cx1) { // uniform
            const int nw = W1 - W0;
            for (int i = tid, n = (Y1 - Y0) * nw; i < n; i += SGN_THREADS) {
                const int r = i / nw;
                words[(size_t)(Y0 + r) * pitch + W0 + (i - r * nw)] = 0u;
            }
            continue;
        }
        const int fx0 = min(max(T[cx0], 0), g.pw - 1), FW = min(min(max(T[oxb + cx1 - 1], fx0), g.pw - 1) - fx0 + 1, SGN_FP_W);
        // the lane's column and the band's rows: their taps are on the way while the dots are made
        const int X = W0 * 32 + wv * 64 + lane, wi = W0 + wv * 2 + lane; // lanes 0 and 1: the word they store
        const bool xin = X >= x0 && X < x1, store = lane < 2 && wi < W1;
        int ca = 0, cb = 0, wx1 = 0;
        if (xin) {
            ca = min(max(T[X] - fx0, 0), FW - 1);
            cb = min(max(T[oxb + X] - fx0, 0), FW - 1);
            wx1 = T[oxw + X];
        }
        const int wx0 = 256 - wx1;
        if (tid < Y1 - Y0) {
            ytap[0][tid] = min(max(T[oya + Y0 + tid] - fy0, 0), FH - 1) * FW;
            ytap[1][tid] = min(max(T[oyb + Y0 + tid] - fy0, 0), FH - 1) * FW;
            ytap[2][tid] = T[oyw + Y0 + tid];
        }
        for (int i = tid; i < FH * FW; i += SGN_THREADS) {
            const int r = i / FW, c = i - r * FW;
            const int8_t *q = pf + ((size_t)(fy0 + r) * g.pw + (fx0 + c)) * g.proto_pix_step;
            int acc = 0;
#pragma unroll 1 // (unrolled, the planes' 64 channel offsets are 128 scalar registers: they spilled)
            for (int kb = 0; kb < g.nm; kb += 16) {
                const sg_v4i a = *(const sg_v4i *)&a_s[kb]; // a broadcast read
                const sg_v4i b = sgn_load16(q, kb, g.nm, g.proto_ch_step);
#pragma unroll
                for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_sdot4(a[j], b[j], acc, false);
            }
            dots[i] = acc;
        }
        __syncthreads();
        for (int Y = Y0; Y < Y1; Y++) {
            const int ra = ytap[0][Y - Y0], rb = ytap[1][Y - Y0], wy1 = ytap[2][Y - Y0], wy0 = 256 - wy1;
            const int h0 = wx0 * dots[ra + ca] + wx1 * dots[ra + cb], h1 = wx0 * dots[rb + ca] + wx1 * dots[rb + cb];
            const long long S = (long long)wy0 * h0 + (long long)wy1 * h1;
            const unsigned long long m = __ballot(xin && __fmul_rn((float)S, s16) > g.logit_min);
            const uint32_t w = lane == 0 ? (uint32_t)m : (uint32_t)(m >> 32);
            if (store) {
                words[(size_t)Y * pitch + wi] = w;
                area += __popc(w);
            }
        }
        __syncthreads(); // the next tile's dots go where these are read
    }
    if (area) atomicAdd(&area_s, area);
    __syncthreads();
    if (tid == 0 && area_s) atomicAdd(&rec->area, area_s);
}

extern "C" int mhip_seg_native(const mhip_seg_native_t *p) {
    if (!p) return -1;
    const mhip_seg_t *g = &p->seg;
    if (g->nheads <= 0 || g->nheads > 4 || g->frames <= 0 || g->frames > 65535 || !g->proto || !g->boxes || !g->counts || !g->pred || !g->recs ||
        !g->words || !p->taps || g->det_cap <= 0 || g->nm < 1 || g->nm > MHIP_SEG_MAX_NM || g->ph <= 0 || g->pw <= 0 || g->in_w <= 0 || g->in_h <= 0 ||
        g->max_per_frame < 1 || g->max_per_frame > MHIP_SEG_MAX_PER_FRAME || g->proto_pix_step <= 0 || g->proto_ch_step <= 0 || p->out_w < 1 ||
        p->out_w > MHIP_SEGN_MAX_OUT || p->out_h < 1 || p->out_h > MHIP_SEGN_MAX_OUT || (long long)p->out_h * ((p->out_w + 31) / 32) > (1LL << 24))
        return -1;
    for (int k = 0; k < g->nheads; k++)
        if (!g->coef[k] || g->cells[k] <= 0 || g->coef_pix_step[k] <= 0 || g->coef_ch_step[k] <= 0) return -1;
    mhip_seg_t q = *g; // the selection's view: rectangles on the output grid, from boxes on the base grid
    q.pw = p->out_w;
    q.ph = p->out_h;
    int rc = mhip_seg_select(&q);
    if (rc) return rc;
    hipLaunchKernelGGL(seg_native_kernel, dim3((p->out_h + SGN_SPAN - 1) / SGN_SPAN, g->max_per_frame, g->frames), dim3(SGN_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "masks in frame pixels");
}
