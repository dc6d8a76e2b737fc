// seg.hip -- instance masks of YOLOv8-seg style heads on gfx950: for every selected detection of a frame, bit (y, x) of its mask is
// ((float)(coefficient row . prototype pixel) * scale > logit_min) inside the detection's rectangle, at the prototype tensor's size.
//
// include/mars_hip.h ("Instance masks") states the arithmetic.  Two launches:
//   seg_select_kernel   one wavefront per frame walks the kept list 64 records at a time; a ballot prefix numbers the records with
//                       conf >= min_conf in list order until max_per_frame are taken (a function of the list alone: no atomics).  Each
//                       taken record gets its rectangle (float32, every operation rounded on its own) and its record {det, x0, y0, x1,
//                       y1, area = 0}; the slots left over get {-1, 0, 0, 0, 0, 0}.
//   seg_mask_kernel     grid (pixel tiles, frames), four wavefronts.  A workgroup reads the frame's records, finds each one's (head, cell)
//                       from the prediction index the detection tail kept, and gathers those cells' coefficient rows into LDS as the A
//                       operand: 64 rows x 64 bytes, rows beyond the selection and channels beyond nm zero.  A wavefront then walks 16
//                       consecutive WORD UNITS -- 32 pixels of one prototype row, one uint32 of every mask -- and per unit loads the 32
//                       pixels' channel bytes ONCE as two B operands (operand maps as in conv_i8_common.hpp: lane l holds bytes
//                       16 * (l >> 4) .. + 15 of row l & 15; result register e of lane l is A-row 4 * (l >> 4) + e against B-row l & 15)
//                       and issues one v_mfma_i32_16x16x64_i8 per operand and 16-detection tile that holds a selected detection.
//                       The bit rule and the rectangle test run on the accumulators in registers; a ballot per result register turns 64
//                       lanes' bits into the 16-pixel runs of four detections, and lanes 0 .. 15 put two runs together into detection
//                       (tile * 16 + lane)'s word, store it, and count its bits.  A wavefront's 16 words of one mask are one 64-byte
//                       line.  Areas are summed per wavefront in registers and added to the record with one integer atomic per
//                       detection: the order of integer adds does not show.  Slots beyond the last computed tile are zero-filled with
//                       coalesced stores; a frame without a selection does nothing else.
// K is nm zero-padded to 64: one 16x16x64 instruction covers every nm <= 64 (the 16x16x32 form would take two for nm > 32 and saves
// nothing at nm = 32: the stage is bound by the prototype bytes it reads and the words it writes, not by the matrix unit).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../mhip.h"
#include "seg_common.hpp"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define SEG_SEL_THREADS 64
#define SEG_THREADS 256
#define SEG_WAVE_UNITS 16                                 // word units a wavefront walks
#define SEG_WG_UNITS (SEG_WAVE_UNITS * SEG_THREADS / 64)  // ... and a workgroup covers

__global__ __launch_bounds__(SEG_SEL_THREADS) void seg_select_kernel(const mhip_seg_t p) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int M = p.max_per_frame;
    const det_t *dets = (const det_t *)p.boxes + (size_t)f * p.det_cap;
    mask_t *recs = (mask_t *)p.recs + (size_t)f * M;
    int n = p.counts[f];
    n = n < 0 ? 0 : n > p.det_cap ? p.det_cap : n;
    const float fx = __fdiv_rn((float)p.pw, (float)p.in_w), fy = __fdiv_rn((float)p.ph, (float)p.in_h);
    int taken = 0;
    for (int base = 0; base < n && taken < M; base += SEG_SEL_THREADS) {
        const int i = base + lane;
        det_t d = {0, 0, 0, 0, 0, 0};
        if (i < n) d = dets[i];
        const bool ok = i < n && (p.select_all || d.conf >= p.min_conf);
        const unsigned long long m = __ballot(ok);
        const int slot = taken + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && slot < M) {
            const float hw = __fmul_rn(d.w, 0.5f), hh = __fmul_rn(d.h, 0.5f);
            mask_t r;
            r.det = i;
            r.x0 = sg_edge(__fmul_rn(__fsub_rn(d.x, hw), fx), p.pw, false);
            r.x1 = sg_edge(__fmul_rn(__fadd_rn(d.x, hw), fx), p.pw, true);
            r.y0 = sg_edge(__fmul_rn(__fsub_rn(d.y, hh), fy), p.ph, false);
            r.y1 = sg_edge(__fmul_rn(__fadd_rn(d.y, hh), fy), p.ph, true);
            r.area = 0;
            recs[slot] = r;
        }
        taken += __popcll(m);
    }
    if (taken > M) taken = M;
    for (int slot = taken + lane; slot < M; slot += SEG_SEL_THREADS) recs[slot] = mask_t{-1, 0, 0, 0, 0, 0};
}

__global__ __launch_bounds__(SEG_THREADS) void seg_mask_kernel(const mhip_seg_t p) {
    __shared__ __attribute__((aligned(16))) int8_t a_s[MHIP_SEG_MAX_PER_FRAME][64];
    __shared__ int rx0[64], ry0[64], rx1[64], ry1[64], shead[64], scell[64];
    __shared__ float rs[64];
    __shared__ int nsel_s;
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int M = p.max_per_frame, pitch = (p.pw + 31) >> 5, units = p.ph * pitch;
    mask_t *recs = (mask_t *)p.recs + (size_t)f * M;
    uint32_t *words = p.words + (size_t)f * M * units;
    if (tid < 64) {
        int det = -1, head = -1, cell = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (tid < M) det = recs[tid].det;
        const bool sel = det >= 0 && det < p.det_cap;
        if (sel) {
            x0 = recs[tid].x0; y0 = recs[tid].y0; x1 = recs[tid].x1; y1 = recs[tid].y1;
            int pr = p.pred[(size_t)f * p.det_cap + det];
            if (pr >= 0) {
                int k = 0;
                while (k < p.nheads && pr >= p.cells[k]) pr -= p.cells[k++];
                if (k < p.nheads) { head = k; cell = pr; }
            }
        }
        rx0[tid] = x0; ry0[tid] = y0; rx1[tid] = x1; ry1[tid] = y1; // an unselected slot: the empty rectangle, every bit 0
        shead[tid] = head; scell[tid] = cell;
        rs[tid] = head >= 0 ? p.scale[head] : 0.0f;
        const unsigned long long m = __ballot(sel);
        if (tid == 0) nsel_s = m ? 64 - __clzll(m) : 0; // the selection fills slots 0 .. nsel - 1
    }
    __syncthreads();
    const int nsel = nsel_s, mtiles = (nsel + 15) >> 4;
    const int wg_u0 = blockIdx.x * SEG_WG_UNITS, wg_u1 = min(wg_u0 + SEG_WG_UNITS, units);
    // slots no computed tile covers: all-zero words
    for (int s = mtiles * 16 + wv; s < M; s += SEG_THREADS / 64)
        for (int u = wg_u0 + lane; u < wg_u1; u += 64) words[(size_t)s * units + u] = 0u;
    if (!mtiles) return;
    { // the A operand: thread t brings bytes 16 * (t & 3) .. + 15 of row t >> 2
        const int row = tid >> 2, kb = (tid & 3) * 16, head = shead[row];
        sg_v4i v = {0, 0, 0, 0};
        if (row < nsel && head >= 0)
            v = sg_load16(p.coef[head] + (size_t)f * p.coef_frame_stride[head] + (size_t)scell[row] * p.coef_pix_step[head], kb, p.nm, p.coef_ch_step[head]);
        *(sg_v4i *)&a_s[row][kb] = v;
    }
    __syncthreads();
    const int col = lane & 15, kb = (lane >> 4) * 16;
    sg_v4i a[4];
#pragma unroll
    for (int mt = 0; mt < 4; mt++) a[mt] = mt < mtiles ? *(const sg_v4i *)&a_s[mt * 16 + col][kb] : (sg_v4i){0, 0, 0, 0};
    int area[4] = {0, 0, 0, 0};
    const int8_t *pf = p.proto + (size_t)f * p.proto_frame_stride;
    const int u0 = wg_u0 + wv * SEG_WAVE_UNITS;
    for (int uu = 0; uu < SEG_WAVE_UNITS; uu++) {
        const int u = u0 + uu;
        if (u >= units) break; // wave-uniform
        const int y = u / pitch, wc = u - y * pitch;
        const int xa = wc * 32 + col, xb = xa + 16;
        sg_v4i b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
        if (xa < p.pw) b0 = sg_load16(pf + ((size_t)y * p.pw + xa) * p.proto_pix_step, kb, p.nm, p.proto_ch_step);
        if (xb < p.pw) b1 = sg_load16(pf + ((size_t)y * p.pw + xb) * p.proto_pix_step, kb, p.nm, p.proto_ch_step);
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            if (mt >= mtiles) break; // uniform
            const sg_v4i z = {0, 0, 0, 0};
            const sg_v4i c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mt], b0, z, 0, 0, 0);
            const sg_v4i c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mt], b1, z, 0, 0, 0);
            unsigned long long bal0[4], bal1[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int slot = mt * 16 + (lane >> 4) * 4 + e;
                const float s = rs[slot];
                const int x0 = rx0[slot], x1 = rx1[slot];
                const bool iny = y >= ry0[slot] && y < ry1[slot];
                const bool bit0 = iny && xa >= x0 && xa < x1 && __fmul_rn((float)c0[e], s) > p.logit_min;
                const bool bit1 = iny && xb >= x0 && xb < x1 && __fmul_rn((float)c1[e], s) > p.logit_min;
                bal0[e] = __ballot(bit0);
                bal1[e] = __ballot(bit1);
            }
            // bits 16 g .. 16 g + 15 of ballot e: pixels xa (xb) of detection 4 g + e of this tile
            const int g = col >> 2, e = col & 3;
            const unsigned long long s0 = e == 0 ? bal0[0] : e == 1 ? bal0[1] : e == 2 ? bal0[2] : bal0[3];
            const unsigned long long s1 = e == 0 ? bal1[0] : e == 1 ? bal1[1] : e == 2 ? bal1[2] : bal1[3];
            const uint32_t word = (uint32_t)((s0 >> (16 * g)) & 0xffffull) | ((uint32_t)((s1 >> (16 * g)) & 0xffffull) << 16);
            const int slot = mt * 16 + col;
            if (lane < 16 && slot < M) {
                words[(size_t)slot * units + u] = word;
                area[mt] += __popc(word);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        const int slot = mt * 16 + col;
        if (mt < mtiles && lane < 16 && slot < M && area[mt]) atomicAdd(&recs[slot].area, area[mt]);
    }
}

// the selection alone, for a caller that has checked p (mhip_seg below; seg_native.hip, with the output grid in pw / ph and the base grid in in_w / in_h)
extern "C" int mhip_seg_select(const mhip_seg_t *p) {
    hipLaunchKernelGGL(seg_select_kernel, dim3(p->frames), dim3(SEG_SEL_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "mask selection");
}

extern "C" int mhip_seg(const mhip_seg_t *p) {
    if (!p || p->nheads <= 0 || p->nheads > 4 || p->frames <= 0 || p->frames > 65535 || !p->proto || !p->boxes || !p->counts || !p->pred ||
        !p->recs || !p->words || p->det_cap <= 0 || p->nm < 1 || p->nm > MHIP_SEG_MAX_NM || p->ph <= 0 || p->pw <= 0 || p->in_w <= 0 ||
        p->in_h <= 0 || p->max_per_frame < 1 || p->max_per_frame > MHIP_SEG_MAX_PER_FRAME || p->proto_pix_step <= 0 || p->proto_ch_step <= 0 ||
        (long long)p->ph * ((p->pw + 31) / 32) > (1LL << 24))
        return -1;
    for (int k = 0; k < p->nheads; k++)
        if (!p->coef[k] || p->cells[k] <= 0 || p->coef_pix_step[k] <= 0 || p->coef_ch_step[k] <= 0) return -1;
    int rc = mhip_seg_select(p);
    if (rc) return rc;
    const int units = p->ph * ((p->pw + 31) / 32);
    hipLaunchKernelGGL(seg_mask_kernel, dim3((units + SEG_WG_UNITS - 1) / SEG_WG_UNITS, p->frames), dim3(SEG_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "masks");
}
