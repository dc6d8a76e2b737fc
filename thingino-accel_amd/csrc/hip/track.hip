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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "tail_core.hpp"

#pragma clang fp contract(off)

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define TK_SLOTS MHIP_TRACK_SLOTS
#define TK_CAND MHIP_TRACK_CAND
#define TK_THREADS 512
#define TK_WAVES (TK_THREADS / 64)

struct tk_out_t { int id, hits; };                                                        // mars_track_t
struct tk_state_t { int id, cls, hits, miss; float x, y, w, h, vx, vy; cls_t ident; };    // mars_track_state_t
static_assert(sizeof(tk_out_t) == 8 && sizeof(tk_state_t) == 48, "record sizes of include/mars_hip.h");

__device__ __forceinline__ bool tk_finite(const float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct tk_lds_t {
    // the table, one array per field
    int id[TK_SLOTS], cls[TK_SLOTS], hits[TK_SLOTS], miss[TK_SLOTS];
    float x[TK_SLOTS], y[TK_SLOTS], w[TK_SLOTS], h[TK_SLOTS], vx[TK_SLOTS], vy[TK_SLOTS];
    int icls[TK_SLOTS];
    float iscore[TK_SLOTS];
    float px[TK_SLOTS], py[TK_SLOTS]; // the prediction of this step
    int det[TK_SLOTS];                // the detection index this step's passes gave the slot, or -1
    // the candidates of the running pass
    float cx[TK_CAND], cy[TK_CAND], cw[TK_CAND], ch[TK_CAND];
    int ccls[TK_CAND];
    short cidx[TK_CAND], cslot[TK_CAND]; // index in the frame's list; the slot that took it, or -1
    short tpick[TK_SLOTS], cpick[TK_CAND];
    unsigned char tfree[TK_SLOTS], cfree[TK_CAND]; // still in the game
    // the high set after pass 1, for the births
    short hidx[TK_CAND];
    unsigned char hfree[TK_CAND];
    short freelist[TK_SLOTS];
    int wsum[TK_WAVES];
    long long counters[4];
    int next_id;
};

// rank of this thread among the threads with `flag`, in thread order, and their number.  Every thread of the workgroup calls it.
__device__ __forceinline__ int tk_scan(const bool flag, int *wsum, int &total) {
    __syncthreads(); // (the previous call's readers of wsum are through; what the caller wrote before is visible after)
    return block_rank<TK_WAVES>(flag, wsum, total);
}

// the first TK_CAND members of a set into the candidate arrays, in index order; -> their number.  low: the set L, otherwise H
__device__ int tk_candidates(tk_lds_t &s, const mhip_track_t &p, const det_t *d, const int n, const bool low) {
    const int tid = threadIdx.x;
    if (tid < TK_CAND) s.cfree[tid] = 0;
    int running = 0;
    for (int c0 = 0; c0 < n; c0 += TK_THREADS) { // (n is the same in every thread)
        const int i = c0 + tid;
        bool in = false;
        det_t v;
        if (i < n) {
            v = d[i];
            const bool gate = p.cls_count == 0 || (v.cls >= p.cls_first && (long long)v.cls < (long long)p.cls_first + p.cls_count);
            const bool valid = tk_finite(v.x) && tk_finite(v.y) && tk_finite(v.w) && tk_finite(v.h) && tk_finite(v.conf) && v.w > 0.0f && v.h > 0.0f && gate;
            in = valid && (low ? (v.conf >= p.low_conf && v.conf < p.min_conf) : v.conf >= p.min_conf);
        }
        int total;
        const int pos = running + tk_scan(in, s.wsum, total);
        if (in && pos < TK_CAND) {
            s.cx[pos] = v.x; s.cy[pos] = v.y; s.cw[pos] = v.w; s.ch[pos] = v.h;
            s.ccls[pos] = v.cls;
            s.cidx[pos] = (short)i;
            s.cslot[pos] = -1;
            s.cfree[pos] = 1;
        }
        running += total;
    }
    const int nc = running < TK_CAND ? running : TK_CAND;
    if (tid == 0) s.counters[2] += running - nc;
    __syncthreads();
    return nc;
}

// one pass: the tracks with tfree set against the nc candidates.  Leaves det[slot] and cslot[candidate] of the pairs taken
__device__ void tk_associate(tk_lds_t &s, const int nc, const float thresh, const bool any_class) {
    const int tid = threadIdx.x;
    const bool track_side = tid < TK_SLOTS;
    const int me = track_side ? tid : tid - TK_SLOTS;
    for (;;) {
        if (track_side) {
            int pick = -1;
            if (s.tfree[me]) {
                const box_edges_t a = box_edges(s.px[me], s.py[me], s.w[me], s.h[me]); // the track at its prediction
                const int acls = s.cls[me];
                float best = 0.0f;
                for (int j = 0; j < nc; j++) {
                    if (!s.cfree[j] || !(any_class || s.ccls[j] == acls)) continue;
                    const float iou = box_iou(a, s.cx[j], s.cy[j], s.cw[j], s.ch[j]);
                    if (iou >= thresh && (pick < 0 || iou > best)) { best = iou; pick = j; } // ties: the lower index stays
                }
            }
            s.tpick[me] = (short)pick;
        } else {
            int pick = -1;
            if (me < nc && s.cfree[me]) {
                const float bx = s.cx[me], by = s.cy[me], bw = s.cw[me], bh = s.ch[me];
                const int bcls = s.ccls[me];
                float best = 0.0f;
                for (int t = 0; t < TK_SLOTS; t++) {
                    if (!s.tfree[t] || !(any_class || s.cls[t] == bcls)) continue;
                    const float iou = box_iou(box_edges(s.px[t], s.py[t], s.w[t], s.h[t]), bx, by, bw, bh);
                    if (iou >= thresh && (pick < 0 || iou > best)) { best = iou; pick = t; } // ties: the lower slot stays
                }
            }
            s.cpick[me] = (short)pick;
        }
        __syncthreads();
        int took = 0;
        if (track_side) {
            if (s.tfree[me]) {
                const int j = s.tpick[me];
                if (j < 0) s.tfree[me] = 0; // nothing eligible is left for it, and nothing will be
                else if (s.cpick[j] == me) {
                    s.det[me] = s.cidx[j];
                    s.tfree[me] = 0;
                    took = 1;
                }
            }
        } else if (me < nc && s.cfree[me]) {
            const int t = s.cpick[me];
            if (t < 0) s.cfree[me] = 0;
            else if (s.tpick[t] == me) {
                s.cslot[me] = (short)t;
                s.cfree[me] = 0;
            }
        }
        if (!__syncthreads_or(took)) break; // every round with a free eligible pair takes the best of them: at most 256 rounds and one
    }
}

// grid: streams
__global__ __launch_bounds__(TK_THREADS) void track_kernel(const mhip_track_t p) {
    __shared__ tk_lds_t s;
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
        const int nh = tk_candidates(s, p, d, n, false);
        tk_associate(s, nh, p.iou, p.any_class != 0);
        if (tid < TK_CAND) {
            s.hidx[tid] = s.cidx[tid];
            s.hfree[tid] = tid < nh && s.cslot[tid] < 0;
        }
        __syncthreads();
        // pass 2: the tracks it left against L
        if (p.low_conf > 0.0f) {
            if (tid < TK_SLOTS) s.tfree[tid] = live && s.det[tid] < 0;
            const int nl = tk_candidates(s, p, d, n, true);
            tk_associate(s, nl, p.iou_low, p.any_class != 0);
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
    if (!p || !p->dets || !p->counts || !p->out || !p->states || !p->hdr) return -1;
    if (p->streams < 1 || p->streams > 65535 || p->steps < 1 || p->max_det < 1 || p->max_det > 1000) return -1;
    if (!(p->min_conf > 0.0f) || !(p->low_conf >= 0.0f) || !(p->iou > 0.0f) || !(p->iou_low > 0.0f) || p->max_miss < 1 || p->cls_count < 0) return -1;
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)p->streams), dim3(TK_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "track");
}
