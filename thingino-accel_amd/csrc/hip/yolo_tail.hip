// yolo_tail.hip -- detection tail on gfx950: ordered decode of [npred][85]
// int8 predictions and the reference's exchange-sort + greedy class-wise IoU
// suppression, one workgroup per frame, wavefront-wide scans instead of the
// reference's serial loops.
//
// Replaces reference src/mars/mars_yolo_test.c:80-104 (parse_output) and
// :107-130 (nms).  Bit-exactness notes:
//  * every expf() the reference evaluates has an int8-derived argument, so the
//    host tabulates val[q] = (float)q*scale, obj[q] = 1/(1+expf(-(float)q*scale))
//    and den[q] = 1+expf(-val[q]) with ITS libm; the GPU only divides
//    (correctly rounded) and compares;
//  * candidates keep ascending prediction order and stop at 1000;
//  * the exchange sort `for i: for j>i: if d[j].conf > d[i].conf swap` is NOT
//    stable; pass i moves the suffix maximum to slot i and shifts the chain of
//    strict left-to-right records one record-slot down.  Each pass is done here
//    as one wave-wide (max, first-holder) scan over register-resident slots,
//    reproducing the permutation exactly, ties included;
//  * suppression: the pair relation is evaluated in parallel, 64 rows at a time, into an LDS bit
//    matrix with the reference's float expression order, then applied greedily.
// Beside it (end of file): the decode of raw anchor-based YOLOv5 Detect heads into real boxes
// (heads_decode_kernel) and of anchor-free DFL heads (dfl_decode_kernel), which feed the same sort + suppression.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../mhip.h"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define ROW 85
#define NCLS 80
#define CONF_MIN 0.25f

// ------------------------------------------------------------------ decode
__global__ __launch_bounds__(256) void decode_kernel(const mhip_detect_t p) {
    __shared__ int wave_cnt[4];
    __shared__ int run_total;
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    det_t *dets = (det_t *)p.dets + (size_t)f * MAXD;
    if (tid == 0) run_total = 0;
    __syncthreads();
    int total = 0;
    for (int sgi = 0; sgi < p.nseg && total < MAXD; sgi++) {
        const int8_t *pred = p.pred[sgi] + (size_t)f * p.stride[sgi];
        const float *val = p.lut[sgi], *obj = val + 256, *den = val + 512;
        const int np = p.npred[sgi];
        const int pc = p.pix_c[sgi], ps = p.pix_stride[sgi], apx = (ps && pc % ROW == 0) ? pc / ROW : 0;
        for (int base = 0; base < np && total < MAXD; base += 256) {
            const int r = base + tid;
            bool cand = false;
            det_t d;
            if (r < np) {
                // padded pixel rows (the model wrote its 255-channel rows at a 256-byte pitch): prediction r is anchor
                // r % apx of pixel r / apx; a channel count that is no multiple of 85 takes the per-byte mapping
                const int8_t *rowp = pred + (size_t)r * ROW;
                if (ps && apx) rowp = pred + (size_t)(r / apx) * ps + (r % apx) * ROW;
                const bool bytewise = ps && !apx;
                auto at = [&](int k) -> int {
                    if (!bytewise) return rowp[k];
                    const size_t o = (size_t)r * ROW + k;
                    return pred[(o / pc) * ps + (o % pc)];
                };
                float o = obj[at(4) + 128];
                if (!(o < CONF_MIN)) {
                    int arg = 0, argq = -1000;
                    float top = -1e9f;
                    if (p.mono[sgi] && !bytewise) {
                        // value[q] strictly increasing (the host checked the table): the first maximum of value[q] is the
                        // first maximum of q.  The 80 class bytes come as five 16-byte loads (any alignment is served) and
                        // are compared as integers; one table read at the end restores `top`.
                        v4i w[5];
#pragma unroll
                        for (int k = 0; k < 5; k++) __builtin_memcpy(&w[k], rowp + 5 + 16 * k, 16);
                        int best = -129;
#pragma unroll
                        for (int k = 0; k < 20; k++) {
                            const int d = w[k >> 2][k & 3];
#pragma unroll
                            for (int b = 0; b < 4; b++) {
                                const int q = (d << (24 - 8 * b)) >> 24;
                                const bool gt = q > best;
                                best = gt ? q : best;
                                arg = gt ? 4 * k + b : arg;
                            }
                        }
                        const float s = val[best + 128];
                        if (s > top) { top = s; argq = best; } else arg = 0; // nothing above -1e9: as if no class had been seen
                    } else {
                        for (int c = 0; c < NCLS; c++) {
                            int q = at(5 + c);
                            float s = val[q + 128];
                            if (s > top) { top = s; arg = c; argq = q; }
                        }
                    }
                    // 1 + expf(-top); with no class above -1e9 the reference divides by +inf
                    float dn = argq == -1000 ? INFINITY : den[argq + 128];
                    float conf = o / dn;
                    if (!(conf < CONF_MIN)) {
                        cand = true;
                        d.x = val[at(0) + 128];
                        d.y = val[at(1) + 128];
                        d.w = val[at(2) + 128];
                        d.h = val[at(3) + 128];
                        d.conf = conf;
                        d.cls = arg;
                    }
                }
            }
            int step;
            const int slot = total + block_rank<4>(cand, wave_cnt, step);
            if (cand && slot < MAXD) dets[slot] = d;
            total += step;
            __syncthreads(); // wave_cnt is rewritten by the next step
        }
    }
    if (total > MAXD) total = MAXD;
    if (tid == 0) {
        if (p.raw_counts) p.raw_counts[f] = total;
        p.counts[f] = total;
    }
}

// ------------------------------------------------------------------- sort
// The reference orders the candidates with an exchange sort, `for i: for j > i: if d[j].conf > d[i].conf swap`
// (mars_yolo_test.c:108-110): not stable, and the permutation it leaves among equal confidences is part of the
// contract.  Rounds 1-2 replayed its n passes (wave-wide scans, then a systolic array: 0.5-0.7 ms per batch beside the
// convolutions, the longest kernel of the tail).  Round 3 computes the same permutation in closed form:
//   * the result is non-increasing in confidence, so an element's slot is (number of strictly greater elements) + its
//     place inside its tie group;
//   * for a tie group G of value v, let H = the elements > v.  While any of H is left, each pass takes away exactly the
//     first slot of H in the remaining array -- that element is a strict left-to-right record, so it moves on or is the
//     maximum and leaves -- and if members of G stand before it, the first of them (a record too) jumps into that slot,
//     behind the members it passes.  Whatever the values inside H are, G therefore behaves as a QUEUE walked along the
//     original array: a member of G is appended, an element of H moves the queue's front to its back.  Once H is gone
//     the passes pick the group's members left to right without moving the others, so the queue IS the group's order.
// So: one bitonic sort by (confidence descending, original index ascending) -- 55 compare-exchange rounds for 1024 --
// and, only for tie groups, a replay of that queue by the group's first thread: members arrive in index order, between
// two arrivals the queue turns by (the H elements passed) mod (its length); a circular linked list in LDS makes a turn
// one pointer step and an arrival O(1).  Steps per group <= min(|H|, sum of lengths).  Checked against the oracle's
// literal double loop on tie-heavy inputs (tests/test_gpu_kernels.py, tools/fuzz_tail.py).
// A NaN confidence (a NaN scale gives one, and `conf < 0.25` lets it through) is not ordered by `>`: a frame that
// holds one is sorted by the literal double loop on one thread -- slow, exact, and never taken by a real model.

// --------------------------------------------------------------- suppress
// One 256-thread workgroup per frame, 32 KB of LDS, so that it shares a CU with the convolution workgroups of
// the NEXT batch (the tail runs on the auxiliary stream; a 1024-thread / 148 KB version of this kernel evicted
// every convolution workgroup from the chip while it ran).  The pairwise "same class and IoU > t" relation is
// evaluated 64 rows at a time, inside class buckets, into an 8 KB bit matrix; wave 0 then walks those rows
// greedily OR-ing them into the removed set (suppressed boxes suppress nothing) -- exactly the reference's
// double loop.  The float expression order of the IoU is the reference's.
// cand_pred / kept_pred (both or neither; NULL = nothing is written): the origin of every record.  cand_pred[f][r] is the prediction index
// of candidate r as the decode wrote it; the compaction writes kept_pred[f][slot] = cand_pred[f][sperm[j]] for survivor j of the sorted
// order -- sperm[] is final on every path of the sort (bitonic, tie-queue replay, the NaN loop) and nothing overwrites it afterwards.
__global__ __launch_bounds__(NMS_THREADS) void sort_nms_kernel(det_t *all, int *counts, float thresh, const int *cand_pred, int *kept_pred) {
    __shared__ float bx[1024], by[1024], bw[1024], bh[1024], bconf[1024];
    __shared__ int bc[1024];
    __shared__ unsigned short blist[1024];              // box indices grouped by class bucket
    __shared__ int bstart[NMS_BUCKETS + 1], bfill[NMS_BUCKETS];
    __shared__ __attribute__((aligned(16))) unsigned int mask[NMS_CHUNK][32]; // 64 rows x 1024 bits
    __shared__ unsigned long long removed_s[16];
    __shared__ int wave_cnt[NMS_THREADS / 64];
    __shared__ unsigned short sperm[1024];              // sorted slot -> original index
    __shared__ int flags[2];                            // [0] a NaN confidence in this frame, [1] a tie in this frame

    const int f = blockIdx.x, tid = threadIdx.x;
    det_t *dets = all + (size_t)f * MAXD;
    int n = counts[f];
    if (n > MAXD) n = MAXD;
    if (n <= 0) return;
    // ---- sort (see "sort" above).  Scratch that the suppression only needs later: keys = the bit matrix (8 KB),
    // queue links = blist, passed-H counts = the class array.
    {
        unsigned long long *keys = (unsigned long long *)&mask[0][0];
        unsigned short *nxt = blist, *gtb = (unsigned short *)bc;
        int P = 2;
        while (P < n) P <<= 1;
        if (tid < 2) flags[tid] = 0;
        __syncthreads();
        bool nan = false;
        for (int r = tid; r < P; r += NMS_THREADS) {
            unsigned long long k = 0; // padding: below every real key (confidences are >= 0.25)
            if (r < n) {
                const float c = dets[r].conf;
                nan |= c != c;
                k = ((unsigned long long)__float_as_uint(c) << 10) | (unsigned)(1023 - r);
            }
            keys[r] = k;
        }
        if (nan) flags[0] = 1;
        __syncthreads();
        if (flags[0]) {
            // the literal double loop on (confidence, index) pairs; float compares, so NaN behaves as in the reference
            if (tid == 0) {
                for (int i = 0; i + 1 < n; i++) {
                    unsigned long long ki = keys[i];
                    for (int j = i + 1; j < n; j++) {
                        const unsigned long long kj = keys[j];
                        if (__uint_as_float((unsigned)(kj >> 10)) > __uint_as_float((unsigned)(ki >> 10))) { keys[i] = kj; keys[j] = ki; ki = kj; }
                    }
                }
            }
            __syncthreads();
            for (int r = tid; r < n; r += NMS_THREADS) sperm[r] = (unsigned short)(1023 - (int)(keys[r] & 1023));
        } else {
            bitonic_sort_desc(keys, P);
            // slots of untied elements are final; tie groups are replayed below
            bool member[2] = {false, false};
            for (int q = 0, r = tid; r < n; r += NMS_THREADS, q++) {
                const unsigned cb = (unsigned)(keys[r] >> 10);
                const bool tl = r > 0 && (unsigned)(keys[r - 1] >> 10) == cb, tr = r + 1 < n && (unsigned)(keys[r + 1] >> 10) == cb;
                member[q] = tl || tr;
                sperm[r] = (unsigned short)(1023 - (int)(keys[r] & 1023));
            }
            if (member[0] || member[1]) flags[1] = 1;
            __syncthreads();
            if (flags[1]) { // uniform
                // every member: how many greater elements stand before it in the original order
                for (int q = 0, r = tid; r < n; r += NMS_THREADS, q++) {
                    if (!member[q]) continue;
                    const unsigned cb = (unsigned)(keys[r] >> 10);
                    int g0 = r;
                    while (g0 > 0 && (unsigned)(keys[g0 - 1] >> 10) == cb) g0--;
                    const int pos = sperm[r];
                    int cnt = 0;
                    for (int s2 = 0; s2 < g0; s2++) cnt += sperm[s2] < pos;
                    gtb[r] = (unsigned short)cnt;
                }
                __syncthreads();
                unsigned short first[2] = {0, 0};
                int glen[2] = {0, 0};
                for (int q = 0, r = tid; r < n; r += NMS_THREADS, q++) {
                    if (!member[q]) continue;
                    const unsigned cb = (unsigned)(keys[r] >> 10);
                    if (r > 0 && (unsigned)(keys[r - 1] >> 10) == cb) continue; // not the group's first thread
                    // members r .. r+m-1 arrive in original-index order (the sort's second key)
                    int back = r, len = 1;
                    nxt[r] = (unsigned short)r;
                    int prev = gtb[r];
                    int x = r + 1;
                    for (; x < n && (unsigned)(keys[x] >> 10) == cb; x++) {
                        const int g = gtb[x];
                        for (int turn = (g - prev) % len; turn > 0; turn--) back = nxt[back];
                        prev = g;
                        nxt[x] = nxt[back];
                        nxt[back] = (unsigned short)x;
                        back = x;
                        len++;
                    }
                    for (int turn = (r - prev) % len; turn > 0; turn--) back = nxt[back]; // r = the count of greater elements
                    first[q] = nxt[back];
                    glen[q] = len;
                }
                __syncthreads(); // sperm is read (as the members' original indices) before it is rewritten
                for (int q = 0, r = tid; r < n; r += NMS_THREADS, q++) {
                    if (!glen[q]) continue;
                    // walk the queue front to back; the original indices are still in keys
                    int e = first[q];
                    for (int k2 = 0; k2 < glen[q]; k2++) {
                        sperm[r + k2] = (unsigned short)(1023 - (int)(keys[e] & 1023));
                        e = nxt[e];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (tid < NMS_BUCKETS) bfill[tid] = 0;
    for (int j = tid; j < n; j += NMS_THREADS) { // in the sorted order
        det_t d = dets[sperm[j]];
        bx[j] = d.x; by[j] = d.y; bw[j] = d.w; bh[j] = d.h; bc[j] = d.cls; bconf[j] = d.conf;
    }
    __syncthreads();
    // Only boxes of the same class can suppress each other (reference :118), so the pair relation is evaluated
    // inside class buckets (the exact class is still compared): ~n^2/160 IoUs instead of n^2/2 compares.
    const auto bucket_of = [&](const int j) { return class_bucket(bc[j]); };
    class_buckets(n, bstart, bfill, blist, bucket_of);
    struct row_t { box_edges_t box; int cls; };
    greedy_suppress<16>(
        n, &mask[0][0], bstart, blist, removed_s, bucket_of,
        [&](const int i) { return row_t{box_edges(bx[i], by[i], bw[i], bh[i]), bc[i]}; },
        [&](const row_t &a, const int j) { return bc[j] == a.cls && box_iou(a.box, bx[j], by[j], bw[j], bh[j]) > thresh; });
    // compact the survivors in order (a record only ever moves to a lower slot)
    const int total = compact_survivors(n, removed_s, wave_cnt, [&](const int idx, const int slot) {
        det_t k;
        k.x = bx[idx]; k.y = by[idx]; k.w = bw[idx]; k.h = bh[idx]; k.conf = bconf[idx]; k.cls = bc[idx];
        dets[slot] = k;
        if (kept_pred) kept_pred[(size_t)f * MAXD + slot] = cand_pred[(size_t)f * MAXD + sperm[idx]];
    });
    if (tid == 0) counts[f] = total;
}

extern "C" void mhip_tail_release(void) {} // (the systolic sort's permutation buffer lived here until round 3)
static int launch_sort_nms(det_t *dets, int *counts, int frames, float thresh, const int *cand_pred = nullptr, int *kept_pred = nullptr) {
    if (!cand_pred || !kept_pred) cand_pred = nullptr, kept_pred = nullptr;
    hipLaunchKernelGGL(sort_nms_kernel, dim3(frames), dim3(NMS_THREADS), 0, mhip_stream_native(), dets, counts, thresh, cand_pred, kept_pred);
    return mhip_check(hipGetLastError(), "sort + nms");
}

extern "C" int mhip_detect(const mhip_detect_t *p) {
    if (!p || p->nseg <= 0 || p->nseg > 4 || p->frames <= 0 || !p->dets || !p->counts) return -1;
    for (int s = 0; s < p->nseg; s++)
        if (!p->pred[s] || !p->lut[s] || p->npred[s] < 0 || (p->pix_stride[s] && (p->pix_c[s] <= 0 || p->pix_stride[s] < p->pix_c[s]))) return -1;
    hipLaunchKernelGGL(decode_kernel, dim3(p->frames), dim3(256), 0, mhip_stream_native(), *p);
    int rc = mhip_check(hipGetLastError(), "decode");
    if (rc || !p->do_nms) return rc;
    return launch_sort_nms((det_t *)p->dets, p->counts, p->frames, p->nms_thresh);
}

extern "C" int mhip_nms_only(void *dets_dev, int *count_dev, int n, float thresh) {
    if (!dets_dev || !count_dev || n < 0 || n > MAXD) return -1;
    return launch_sort_nms((det_t *)dets_dev, count_dev, 1, thresh);
}

// ------------------------------------------------------------ anchor heads
// The raw Detect-head convolutions of an anchor-based YOLOv5 graph decoded as the exported model's Detect layer would
// (mars_hip_detect_heads): prediction (head k, anchor a, cell gy, gx) reads channels a * (5 + nc) + 0 .. 4 + nc of the cell;
// with sig[q] = 1 / (1 + expf(-q * scale)) tabulated on the host per head (libm, the decode's own expression):
//   obj = sig[q4] (dropped below conf), best = first class of largest q (the table is strictly increasing for scale > 0, so
//   q decides), c = obj * sig[q_best] (dropped below conf), cx = ((2 sig[q0] - 0.5) + gx) * stride, w = (2 sig[q2])^2 * anchor_w.
// Every float operation is rounded on its own (explicit _rn intrinsics: no FMA contraction whatever the flags).  The first
// 1000 candidates in prediction order are kept -- t377's row order of the shipped file -- and sort_nms_kernel takes over.
// One 256-thread workgroup per frame walks the predictions 2048 at a time, each thread 8 consecutive cells: their objectness
// bytes are loaded first (8 loads in flight per thread), the class bytes only for the cells that pass, and one block-wide
// scan gives every candidate its slot.
#define HEADS_THREADS 256
#define HEADS_CELLS 8 // consecutive cells per thread and step

__global__ __launch_bounds__(HEADS_THREADS) void heads_decode_kernel(const mhip_heads_t p) {
    __shared__ float sig_s[4][256];
    __shared__ int wave_sum[HEADS_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < p.nheads * 256; i += HEADS_THREADS) sig_s[i >> 8][i & 255] = p.sig[i];
    __syncthreads();
    det_t *dets = (det_t *)p.dets + (size_t)f * MAXD;
    const float conf = p.conf;
    int total = 0;
    for (int hd = 0; hd < p.nheads && total < MAXD; hd++) {
        const int8_t *hb = p.base[hd] + (size_t)f * p.frame_stride[hd];
        const int W = p.w[hd], npix = p.h[hd] * W, nc = p.nc[hd], R = 5 + nc, ps = p.pix_step[hd], cs = p.ch_step[hd];
        const float *sg = sig_s[hd];
        const float fstride = (float)p.stride[hd];
        const bool fast80 = nc == 80 && cs == 1;
        for (int a = 0; a < 3 && total < MAXD; a++) {
            const int8_t *ab = hb + (size_t)a * R * cs; // channel a * R of cell 0
            const float aw = p.anchors[hd][a][0], ah = p.anchors[hd][a][1];
            for (int base = 0; base < npix && total < MAXD; base += HEADS_THREADS * HEADS_CELLS) {
                const int c0 = base + tid * HEADS_CELLS;
                int qo[HEADS_CELLS];
#pragma unroll
                for (int k = 0; k < HEADS_CELLS; k++) qo[k] = c0 + k < npix ? ab[(size_t)(c0 + k) * ps + 4 * cs] : 0;
                unsigned cand = 0;
                int best[HEADS_CELLS];
                float cf[HEADS_CELLS];
#pragma unroll
                for (int k = 0; k < HEADS_CELLS; k++) {
                    best[k] = 0;
                    cf[k] = 0.f;
                    if (c0 + k >= npix) continue;
                    const float obj = sg[qo[k] + 128];
                    if (obj < conf) continue;
                    const int8_t *row = ab + (size_t)(c0 + k) * ps;
                    int arg = 0, bq = -129;
                    if (fast80) {
                        // the 80 class bytes as five 16-byte loads (any alignment is served), compared as integers
                        v4i w[5];
#pragma unroll
                        for (int j = 0; j < 5; j++) __builtin_memcpy(&w[j], row + 5 + 16 * j, 16);
#pragma unroll
                        for (int j = 0; j < 20; j++) {
                            const int d = w[j >> 2][j & 3];
#pragma unroll
                            for (int b = 0; b < 4; b++) {
                                const int q = (d << (24 - 8 * b)) >> 24;
                                const bool gt = q > bq;
                                bq = gt ? q : bq;
                                arg = gt ? 4 * j + b : arg;
                            }
                        }
                    } else {
                        for (int c = 0; c < nc; c++) {
                            const int q = row[(size_t)(5 + c) * cs];
                            if (q > bq) { bq = q; arg = c; }
                        }
                    }
                    const float c = __fmul_rn(obj, sg[bq + 128]);
                    if (c < conf) continue;
                    cand |= 1u << k;
                    best[k] = arg;
                    cf[k] = c;
                }
                // slots: block-wide exclusive scan of the per-thread candidate counts (thread order = prediction order)
                const int n_t = __popc(cand);
                int incl = n_t;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o);
                    if (lane >= o) incl += v;
                }
                if (lane == 63) wave_sum[wv] = incl;
                __syncthreads();
                int slot = total, step = 0;
#pragma unroll
                for (int w = 0; w < HEADS_THREADS / 64; w++) {
                    if (w < wv) slot += wave_sum[w];
                    step += wave_sum[w];
                }
                slot += incl - n_t;
#pragma unroll
                for (int k = 0; k < HEADS_CELLS; k++) {
                    if (!((cand >> k) & 1u)) continue;
                    if (slot < MAXD) {
                        const int cell = c0 + k, gy = cell / W, gx = cell - gy * W;
                        const int8_t *row = ab + (size_t)cell * ps;
                        const float s0 = sg[row[0] + 128], s1 = sg[row[cs] + 128];
                        const float s2 = __fmul_rn(sg[row[2 * cs] + 128], 2.0f), s3 = __fmul_rn(sg[row[3 * cs] + 128], 2.0f);
                        det_t d;
                        d.x = __fmul_rn(__fadd_rn(__fsub_rn(__fmul_rn(s0, 2.0f), 0.5f), (float)gx), fstride);
                        d.y = __fmul_rn(__fadd_rn(__fsub_rn(__fmul_rn(s1, 2.0f), 0.5f), (float)gy), fstride);
                        d.w = __fmul_rn(__fmul_rn(s2, s2), aw);
                        d.h = __fmul_rn(__fmul_rn(s3, s3), ah);
                        d.conf = cf[k];
                        d.cls = best[k];
                        dets[slot] = d;
                    }
                    slot++;
                }
                total += step;
                __syncthreads(); // wave_sum is rewritten by the next step
            }
        }
    }
    if (total > MAXD) total = MAXD;
    if (tid == 0) {
        if (p.raw_counts) p.raw_counts[f] = total;
        p.counts[f] = total;
    }
}

// the kept boxes back through the letterbox of the image front-end (after NMS: suppression sees the network's coordinates)
// pre != NULL: the records as they were before the mapping (graph-input pixels) are kept in pre[frame][i] (the mask stage cuts by them)
__global__ __launch_bounds__(256) void heads_map_kernel(det_t *all, const int *counts, float px, float py, float rx, float ry, det_t *pre) {
    det_t *d = all + (size_t)blockIdx.x * MAXD;
    int n = counts[blockIdx.x];
    if (n > MAXD) n = MAXD;
    for (int i = threadIdx.x; i < n; i += 256) {
        det_t r = d[i];
        if (pre) pre[(size_t)blockIdx.x * MAXD + i] = r;
        r.x = __fmul_rn(__fsub_rn(r.x, px), rx);
        r.y = __fmul_rn(__fsub_rn(r.y, py), ry);
        r.w = __fmul_rn(r.w, rx);
        r.h = __fmul_rn(r.h, ry);
        d[i] = r;
    }
}

// ---------------------------------------------------------------- DFL heads
// The anchor-free head of the Ultralytics "u" / YOLOv8 models (mars_hip_detect_dfl): per scale a box convolution of 4 * R channels
// (R = reg_max bins for each of left, top, right, bottom) and a class convolution of nc channels on the same grid, one prediction per
// cell in the order (head, gy, gx).  With the host's tables per head, sg[q] = 1 / (1 + expf(-q * class scale)) and
// E[d] = expf(-(d * box scale)), d = 0 .. 255:
//   best = first class of largest byte, conf = sg[q_best], kept iff conf >= the threshold (no objectness);
//   side k: m = largest of its R bytes, e_i = E[m - q_i], dist_k = (sum of i * e_i) / (sum of e_i), both sums left to right;
//   x1 = (gx + 0.5) - dist_l, x2 = (gx + 0.5) + dist_r, cx = ((x1 + x2) * 0.5) * stride, w = (x2 - x1) * stride (y, h alike).
// Every float operation is rounded on its own (_rn intrinsics).  There is no objectness byte to filter on, so EVERY class byte of every
// cell is read: one 256-thread workgroup per frame walks the cells 1024 at a time, thread t the cells t, 256 + t, 512 + t, 768 + t of
// the step -- consecutive lanes take consecutive cells, so plane reads coalesce -- and issues the loads of its four cells before the
// first compare; pixel rows (ch_step 1) come as 16-byte loads and are compared as integers.  Box bytes are read only for the cells
// that pass.  Slots come from one ordered block-wide count per step, and the walk ends once 1000 candidates are reached.
// With cand_pred / kept_pred set the decode also writes each candidate's prediction index (cells of the heads before it + its cell) and
// the sort carries it to the kept list (mhip_dfl_heads_t); the records and counts are the same bytes either way.
#define DFL_THREADS 256
#define DFL_CELLS 4

// ... reg_max 16 in a pixel row: the side is one 16-byte load
__device__ __forceinline__ float dfl_side16(const int8_t *q, const float *E) {
    v4i w;
    __builtin_memcpy(&w, q, 16);
    int b[16], m = -128;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        b[i] = (w[i >> 2] << (24 - 8 * (i & 3))) >> 24;
        m = max(m, b[i]);
    }
    float den = E[m - b[0]], num = 0.0f;
#pragma unroll
    for (int i = 1; i < 16; i++) {
        const float e = E[m - b[i]];
        den = __fadd_rn(den, e);
        num = __fadd_rn(num, __fmul_rn((float)i, e));
    }
    return __fdiv_rn(num, den);
}

__global__ __launch_bounds__(DFL_THREADS) void dfl_decode_kernel(const mhip_dfl_heads_t p) {
    __shared__ float tab_s[4][512];
    __shared__ int wave_cnt[DFL_CELLS][DFL_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < p.nheads * 512; i += DFL_THREADS) tab_s[i >> 9][i & 511] = p.tab[i];
    __syncthreads();
    det_t *dets = (det_t *)p.dets + (size_t)f * MAXD;
    const float conf = p.conf;
    const int R = p.reg_max;
    int total = 0, pred0 = 0; // pred0: the prediction index of this head's cell 0
    for (int hd = 0; hd < p.nheads && total < MAXD; pred0 += p.h[hd] * p.w[hd], hd++) {
        const int8_t *cb = p.cls[hd] + (size_t)f * p.cls_frame_stride[hd];
        const int8_t *bb = p.box[hd] + (size_t)f * p.box_frame_stride[hd];
        const int W = p.w[hd], npix = p.h[hd] * W, nc = p.nc[hd];
        const int cps = p.cls_pix_step[hd], ccs = p.cls_ch_step[hd], bps = p.box_pix_step[hd], bcs = p.box_ch_step[hd];
        const float *E = tab_s[hd], *sg = E + 256;
        const float fstride = (float)p.stride[hd];
        for (int base = 0; base < npix && total < MAXD; base += DFL_THREADS * DFL_CELLS) {
            int bq[DFL_CELLS], arg[DFL_CELLS];
            const int8_t *row[DFL_CELLS]; // a cell past the end reads the last cell's bytes and is dropped below
#pragma unroll
            for (int k = 0; k < DFL_CELLS; k++) row[k] = cb + (size_t)min(base + k * DFL_THREADS + tid, npix - 1) * cps;
            dfl_class_walk<DFL_CELLS, true>(row, nc, ccs, bq, arg);
            // slots: candidates are numbered in cell order = (k, thread)
            bool cand[DFL_CELLS];
            float cf[DFL_CELLS];
            int rank[DFL_CELLS], step;
#pragma unroll
            for (int k = 0; k < DFL_CELLS; k++) {
                cf[k] = sg[bq[k] + 128];
                cand[k] = base + k * DFL_THREADS + tid < npix && cf[k] >= conf;
            }
            block_rank<DFL_THREADS / 64, DFL_CELLS>(cand, wave_cnt, rank, step);
#pragma unroll
            for (int k = 0; k < DFL_CELLS; k++) {
                const int slot = total + rank[k];
                if (!cand[k] || slot >= MAXD) continue;
                const int cell = base + k * DFL_THREADS + tid, gy = cell / W, gx = cell - gy * W;
                const int8_t *q = bb + (size_t)cell * bps;
                float dist[4];
                if (R == 16 && bcs == 1) {
#pragma unroll
                    for (int s = 0; s < 4; s++) dist[s] = dfl_side16(q + 16 * s, E);
                } else {
                    for (int s = 0; s < 4; s++) dist[s] = dfl_side(q + (size_t)s * R * bcs, R, bcs, E);
                }
                const float ax = __fadd_rn((float)gx, 0.5f), ay = __fadd_rn((float)gy, 0.5f);
                const float x1 = __fsub_rn(ax, dist[0]), y1 = __fsub_rn(ay, dist[1]), x2 = __fadd_rn(ax, dist[2]), y2 = __fadd_rn(ay, dist[3]);
                det_t d;
                d.x = __fmul_rn(__fmul_rn(__fadd_rn(x1, x2), 0.5f), fstride);
                d.y = __fmul_rn(__fmul_rn(__fadd_rn(y1, y2), 0.5f), fstride);
                d.w = __fmul_rn(__fsub_rn(x2, x1), fstride);
                d.h = __fmul_rn(__fsub_rn(y2, y1), fstride);
                d.conf = cf[k];
                d.cls = arg[k];
                dets[slot] = d;
                if (p.cand_pred) p.cand_pred[(size_t)f * MAXD + slot] = pred0 + cell;
            }
            total += step;
            __syncthreads(); // wave_cnt is rewritten by the next step
        }
    }
    if (total > MAXD) total = MAXD;
    if (tid == 0) {
        if (p.raw_counts) p.raw_counts[f] = total;
        p.counts[f] = total;
    }
}

extern "C" int mhip_detect_heads(const mhip_heads_t *p) {
    if (!p || p->nheads <= 0 || p->nheads > 4 || p->frames <= 0 || !p->dets || !p->counts || !p->sig) return -1;
    for (int k = 0; k < p->nheads; k++)
        if (!p->base[k] || p->h[k] <= 0 || p->w[k] <= 0 || p->nc[k] < 1 || p->pix_step[k] <= 0 || p->ch_step[k] <= 0) return -1;
    hipLaunchKernelGGL(heads_decode_kernel, dim3(p->frames), dim3(HEADS_THREADS), 0, mhip_stream_native(), *p);
    int rc = mhip_check(hipGetLastError(), "decode heads");
    if (!rc) rc = launch_sort_nms((det_t *)p->dets, p->counts, p->frames, p->nms_thresh);
    if (rc || !p->map) return rc;
    hipLaunchKernelGGL(heads_map_kernel, dim3(p->frames), dim3(256), 0, mhip_stream_native(), (det_t *)p->dets, p->counts, (float)p->px,
                       (float)p->py, p->rx, p->ry, (det_t *)nullptr);
    return mhip_check(hipGetLastError(), "letterbox mapping");
}

extern "C" int mhip_detect_dfl(const mhip_dfl_heads_t *p) {
    if (!p || p->nheads <= 0 || p->nheads > 4 || p->frames <= 0 || !p->dets || !p->counts || !p->tab || p->reg_max < 2 || p->reg_max > 32) return -1;
    for (int k = 0; k < p->nheads; k++)
        if (!p->box[k] || !p->cls[k] || p->h[k] <= 0 || p->w[k] <= 0 || p->nc[k] < 1 || p->box_pix_step[k] <= 0 || p->box_ch_step[k] <= 0 ||
            p->cls_pix_step[k] <= 0 || p->cls_ch_step[k] <= 0)
            return -1;
    mhip_dfl_heads_t q = *p;
    if (!q.cand_pred || !q.kept_pred) q.cand_pred = q.kept_pred = nullptr; // both or neither
    hipLaunchKernelGGL(dfl_decode_kernel, dim3(p->frames), dim3(DFL_THREADS), 0, mhip_stream_native(), q);
    int rc = mhip_check(hipGetLastError(), "decode DFL heads");
    if (!rc) rc = launch_sort_nms((det_t *)p->dets, p->counts, p->frames, p->nms_thresh, p->cand_pred, p->kept_pred);
    if (rc || !p->map) return rc;
    hipLaunchKernelGGL(heads_map_kernel, dim3(p->frames), dim3(256), 0, mhip_stream_native(), (det_t *)p->dets, p->counts, (float)p->px,
                       (float)p->py, p->rx, p->ry, (det_t *)p->premap);
    return mhip_check(hipGetLastError(), "letterbox mapping");
}
