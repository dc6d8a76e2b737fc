// track.hip -- tracking across frames on gfx950: the detection lists a detection tail left in HBM (or a caller's lists) -> a stable track
// id per detection, the track tables of S camera streams held in HBM between calls.
//
// include/mars_hip.h ("Tracking") states the arithmetic.  One launch, one workgroup of 512 threads per stream.  The workgroup loads its
// stream's table of 256 slots into LDS, walks the stream's frames of the call in order and writes the table back once.  Per frame:
//   candidates   the valid detections of the high (then the low) confidence set are compacted into LDS in index order by a ballot prefix
//                scan over the workgroup: position = rank, no atomics;
//   association  greedy matching by (iou descending, slot ascending, detection ascending) is a strict total order, so it equals rounds of
//                "every free track picks its best free eligible candidate, every free candidate its best free track, mutual picks are
//                taken": the best free pair overall is always mutual, and a mutual pair is one no earlier pair of the order can still
//                touch.  Threads 0 .. 255 own a track each, threads 256 .. 511 a candidate each; both halves scan the other side's boxes
//                in LDS (every lane reads the same address: a broadcast) and RECOMPUTE the IoU -- a 256 x 256 matrix is 256 KB and does not
//                fit.  A side that finds nothing eligible leaves the game: free sets only shrink.  The staircase case resolves one pair
//                per round, 256 rounds;
//   update       a thread per slot: matched, coasting or dead;
//   births       two prefix scans: free slots by ascending slot, unmatched high-set candidates by ascending index; birth b takes free
//                slot b and id next_id + b.  Slots and ids are a function of the lists alone.
// LDS: about 25 KB (the sort + NMS kernel's comment in yolo_tail.hip records what a 148 KB tail did to the next batch's convolutions).
// The records, the table, the scans, the compaction and the rounds are track_core.hpp's, shared with track_app.hip; the per-step body
// below is this kernel's own (track_core.hpp says why), and with it the kernel has none of the appearance term's code or LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "track_core.hpp"

#pragma clang fp contract(off)

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

// grid: streams
__global__ __launch_bounds__(TK_THREADS) void track_kernel(const mhip_track_t p) {
    __shared__ tk_lds_t<false> s;
    const int tid = threadIdx.x, b = blockIdx.x;
    tk_state_t *table = (tk_state_t *)p.states + (size_t)b * TK_SLOTS;
    if (tid < TK_SLOTS) {
        const tk_state_t v = table[tid];
        s.id[tid] = v.id; s.cls[tid] = v.cls; s.hits[tid] = v.hits; s.miss[tid] = v.miss;
        s.x[tid] = v.x; s.y[tid] = v.y; s.w[tid] = v.w; s.h[tid] = v.h; s.vx[tid] = v.vx; s.vy[tid] = v.vy;
        s.icls[tid] = v.ident.cls; s.iscore[tid] = v.ident.score;
    }
    if (tid < 4) s.counters[tid] = p.hdr[b].counters[tid];
    if (tid == 0) s.next_id = p.hdr[b].next_id;
    __syncthreads();
    for (int t = 0; t < p.steps; t++) {
        const size_t f = p.stream_major ? (size_t)b * p.steps + t : (size_t)t * p.streams + b;
        const det_t *d = (const det_t *)p.dets + f * p.max_det;
        const cls_t *idn = p.idents ? (const cls_t *)p.idents + f * p.max_det : nullptr;
        tk_out_t *o = (tk_out_t *)p.out + f * p.max_det;
        int n = p.counts[f];
        n = n < 0 ? 0 : n > p.max_det ? p.max_det : n;
        for (int i = tid; i < p.max_det; i += TK_THREADS) o[i] = tk_out_t{-1, 0};
        const bool live = tid < TK_SLOTS && s.hits[tid] > 0;
        if (tid < TK_SLOTS) {
            s.px[tid] = s.x[tid] + s.vx[tid];
            s.py[tid] = s.y[tid] + s.vy[tid];
            s.det[tid] = -1;
            s.tfree[tid] = live;
        }
        // pass 1: every live track against H
        const int nh = tk_candidates<false>(s, p, d, nullptr, n, false);
        tk_associate<false>(s, nh, p.iou, p.any_class != 0, 0.0f, 0.0f, nullptr, nullptr);
        if (tid < TK_CAND) {
            s.hidx[tid] = s.cidx[tid];
            s.hfree[tid] = tid < nh && s.cslot[tid] < 0;
        }
        __syncthreads();
        // pass 2: the tracks it left against L
        if (p.low_conf > 0.0f) {
            if (tid < TK_SLOTS) s.tfree[tid] = live && s.det[tid] < 0;
            const int nl = tk_candidates<false>(s, p, d, nullptr, n, true);
            tk_associate<false>(s, nl, p.iou_low, p.any_class != 0, 0.0f, 0.0f, nullptr, nullptr);
        }
        // update
        bool died = false;
        if (live) {
            const int i = s.det[tid];
            if (i >= 0) {
                const det_t v = d[i];
                const float dx = v.x - s.x[tid], dy = v.y - s.y[tid];
                if (s.hits[tid] == 1) { s.vx[tid] = dx; s.vy[tid] = dy; }
                else { s.vx[tid] = (s.vx[tid] + dx) * 0.5f; s.vy[tid] = (s.vy[tid] + dy) * 0.5f; }
                s.x[tid] = v.x; s.y[tid] = v.y; s.w[tid] = v.w; s.h[tid] = v.h; s.cls[tid] = v.cls;
                s.hits[tid] += 1;
                s.miss[tid] = 0;
                if (idn) {
                    const cls_t e = idn[i];
                    if (e.cls >= 0 && (s.icls[tid] < 0 || e.score >= s.iscore[tid])) { s.icls[tid] = e.cls; s.iscore[tid] = e.score; }
                }
                o[i] = tk_out_t{s.id[tid], s.hits[tid]}; // (behind the {-1, 0} of the loop above: the scans' barriers lie between)
            } else {
                s.x[tid] = s.px[tid]; s.y[tid] = s.py[tid];
                s.miss[tid] += 1;
                if (s.miss[tid] > p.max_miss) { s.hits[tid] = 0; died = true; }
            }
        }
        int deaths, nfree, nborn;
        tk_scan(died, s.wsum, deaths);
        // births: free slot r and unmatched H member r meet
        const bool is_free = tid < TK_SLOTS && s.hits[tid] == 0;
        const int r = tk_scan(is_free, s.wsum, nfree);
        if (is_free) s.freelist[r] = (short)tid;
        const bool wants = tid < TK_CAND && s.hfree[tid];
        const int bi = tk_scan(wants, s.wsum, nborn); // (its barriers publish the free list)
        const int fits = nborn < nfree ? nborn : nfree;
        if (wants && bi < fits) {
            const int slot = s.freelist[bi], i = s.hidx[tid];
            const det_t v = d[i];
            const int id = (int)((unsigned)s.next_id + 1u + (unsigned)bi);
            s.id[slot] = id; s.cls[slot] = v.cls; s.hits[slot] = 1; s.miss[slot] = 0;
            s.x[slot] = v.x; s.y[slot] = v.y; s.w[slot] = v.w; s.h[slot] = v.h; s.vx[slot] = 0.0f; s.vy[slot] = 0.0f;
            cls_t e = cls_t{-1, 0.0f};
            if (idn) e = idn[i];
            s.icls[slot] = e.cls; s.iscore[slot] = e.score;
            o[i] = tk_out_t{id, 1};
        }
        __syncthreads();
        if (tid == 0) {
            s.next_id = (int)((unsigned)s.next_id + (unsigned)fits);
            s.counters[0] += fits;
            s.counters[1] += deaths;
            s.counters[3] += nborn - fits;
        }
        __syncthreads();
    }
    if (tid < TK_SLOTS) {
        tk_state_t v;
        v.id = s.id[tid]; v.cls = s.cls[tid]; v.hits = s.hits[tid]; v.miss = s.miss[tid];
        v.x = s.x[tid]; v.y = s.y[tid]; v.w = s.w[tid]; v.h = s.h[tid]; v.vx = s.vx[tid]; v.vy = s.vy[tid];
        v.ident.cls = s.icls[tid]; v.ident.score = s.iscore[tid];
        table[tid] = v;
    }
    if (tid < 4) p.hdr[b].counters[tid] = s.counters[tid];
    if (tid == 0) p.hdr[b].next_id = s.next_id;
}

// ---- launcher
extern "C" int mhip_track(const mhip_track_t *p) {
    if (!p || !tk_args_ok(p)) return -1;
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)p->streams), dim3(TK_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "track");
}
