// track_core.hpp -- what track.hip and track_app.hip share of the tracking walk, written once, device-only and inlined: the records, the
// LDS table, the scans, the candidates' compaction (tk_candidates) and the mutual-best-pick rounds (tk_associate), and the launchers' checks
// of the mhip_track_t part.  track.hip's header states the design.  The helpers are templated on APP, whether the tracker holds an embedding
// plane; the plain instantiations carry nothing of it, neither instructions nor LDS.  The per-step body around them (predict, update,
// births, counters, the table's load and store) is NOT here: each kernel has its own.  Moved into a function shared by both kernels --
// even the table's load and store alone -- it compiles, in track_kernel, to the same loops behind a different prologue, and the plain call
// measured 3 .. 4 % slower for it (profiles/HISTORY.md, "One walk"); with its own body track_kernel is, instruction for instruction and
// byte offset for byte offset, what it was before the helpers were shared.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "tail_core.hpp"

#define TK_SLOTS MHIP_TRACK_SLOTS
#define TK_CAND MHIP_TRACK_CAND
#define TK_THREADS 512
#define TK_WAVES (TK_THREADS / 64)
#define TK_TAKE_NONE (-1)
#define TK_CLEAR (-2)

struct tk_out_t { int id, hits; };                                                        // mars_track_t
struct tk_state_t { int id, cls, hits, miss; float x, y, w, h, vx, vy; cls_t ident; };    // mars_track_state_t
static_assert(sizeof(tk_out_t) == 8 && sizeof(tk_state_t) == 48, "record sizes of include/mars_hip.h");

__device__ __forceinline__ bool tk_finite(const float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct tk_table_t {
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
struct tk_plane_t {
    int ee[TK_SLOTS];                 // the slot's embedding: its sum of squares, 0 = none (the bytes live in HBM)
    int take[TK_SLOTS];               // this step's embedding action: the row of q to take, TK_TAKE_NONE or TK_CLEAR
    int crow[TK_CAND], cqq[TK_CAND];  // pass 1: the candidate's row of q and its qq; -1 and 0: it has no embedding
    unsigned char blend[TK_SLOTS];    // the row taken is blended 3:1 into what the slot holds
};
// The plain kernel's LDS is the table and nothing else; the appearance kernel's has the plane's arrays IN FRONT of it: behind it the kernel
// came out at 126 VGPRs, in front at the 125 it had with the arrays interleaved (the offsets decide which LDS accesses pair up)
template <bool APP> struct tk_lds_t : tk_table_t {};
template <> struct tk_lds_t<true> : tk_plane_t, tk_table_t {};
static_assert(sizeof(tk_lds_t<false>) == sizeof(tk_table_t) && sizeof(tk_lds_t<true>) == sizeof(tk_table_t) + 4 * 1024 + 256,
              "the plain table carries nothing of the plane's; the plane adds four int arrays and a byte array");

// the launch record of either kernel, and its mhip_track_t
template <bool APP> struct tk_params { typedef mhip_track_t type; };
template <> struct tk_params<true> { typedef mhip_track_app_t type; };
__device__ __forceinline__ const mhip_track_t &tk_of(const mhip_track_t &p) { return p; }
__device__ __forceinline__ const mhip_track_t &tk_of(const mhip_track_app_t &pa) { return pa.t; }

// A candidate's embedding row.  track_app.hip, which includes this header, defines it (__forceinline__); the only call sits in a branch
// that tk_candidates<false> discards, so track.hip never needs the definition.  The one place where this header looks back at a file above it.
__device__ int ta_row_of(const mhip_track_app_t &p, const int *idx, const int i, int &qq);

// rank of this thread among the threads with `flag`, in thread order, and their number.  Every thread of the workgroup calls it.
__device__ __forceinline__ int tk_scan(const bool flag, int *wsum, int &total) {
    __syncthreads(); // (the previous call's readers of wsum are through; what the caller wrote before is visible after)
    return block_rank<TK_WAVES>(flag, wsum, total);
}

// the first TK_CAND members of a set into the candidate arrays, in index order; -> their number.  low: the set L, otherwise H (APP: with
// each member's embedding row, idx being the frame's row indices or null)
template <bool APP>
__device__ int tk_candidates(tk_lds_t<APP> &s, const typename tk_params<APP>::type &pp, const det_t *d, const int *idx, const int n, const bool low) {
    const mhip_track_t &p = tk_of(pp);
    const int tid = threadIdx.x;
    if (tid < TK_CAND) {
        s.cfree[tid] = 0;
        if constexpr (APP) { s.crow[tid] = -1; s.cqq[tid] = 0; }
    }
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
        const int pos = running + tk_scan(in, s.wsum, total); // (its barriers lie behind the clearing above)
        if (in && pos < TK_CAND) {
            s.cx[pos] = v.x; s.cy[pos] = v.y; s.cw[pos] = v.w; s.ch[pos] = v.h;
            s.ccls[pos] = v.cls;
            s.cidx[pos] = (short)i;
            s.cslot[pos] = -1;
            s.cfree[pos] = 1;
            if constexpr (APP) {
                if (!low) {
                    int qq;
                    s.crow[pos] = ta_row_of(pp, idx, i, qq);
                    s.cqq[pos] = qq;
                }
            }
        }
        running += total;
    }
    const int nc = running < TK_CAND ? running : TK_CAND;
    if (tid == 0) s.counters[2] += running - nc;
    __syncthreads();
    return nc;
}

// one pass: the tracks with tfree set against the nc candidates.  Leaves det[slot] and cslot[candidate] of the pairs taken.  COS (APP
// only): pass 1 with the cosines of ta_matrix (sm, cm)
template <bool COS, bool APP>
__device__ void tk_associate(tk_lds_t<APP> &s, const int nc, const float thresh, const bool any_class, const float app_thresh, const float app_min_iou,
                             const float *sm, const float *cm) {
    static_assert(APP || !COS, "cosines need the embedding plane");
    const int tid = threadIdx.x;
    const bool track_side = tid < TK_SLOTS;
    const int me = track_side ? tid : tid - TK_SLOTS;
    for (;;) {
        if (track_side) {
            int pick = -1;
            if (s.tfree[me]) {
                const box_edges_t a = box_edges(s.px[me], s.py[me], s.w[me], s.h[me]); // the track at its prediction
                const int acls = s.cls[me];
                bool mine = false;
                if constexpr (COS) mine = s.ee[me] > 0;
                float best = 0.0f;
                for (int j = 0; j < nc; j++) {
                    if (!s.cfree[j] || !(any_class || s.ccls[j] == acls)) continue;
                    const float iou = box_iou(a, s.cx[j], s.cy[j], s.cw[j], s.ch[j]);
                    if constexpr (COS) {
                        float key = iou;
                        bool ok = iou >= thresh;
                        if (mine && s.cqq[j] > 0) {
                            const float cs = cm[(size_t)j * TK_SLOTS + me];
                            if (cs >= app_thresh && iou >= app_min_iou) { key = fmaxf(iou, cs); ok = true; }
                        }
                        if (ok && (pick < 0 || key > best)) { best = key; pick = j; } // ties: the lower index stays
                    } else { // the IoU alone, written out: through key and ok the scan came out with two instructions moved, 0.3 % of the staircase
                        if (iou >= thresh && (pick < 0 || iou > best)) { best = iou; pick = j; }
                    }
                }
            }
            s.tpick[me] = (short)pick;
        } else {
            int pick = -1;
            if (me < nc && s.cfree[me]) {
                const float bx = s.cx[me], by = s.cy[me], bw = s.cw[me], bh = s.ch[me];
                const int bcls = s.ccls[me];
                bool mine = false;
                if constexpr (COS) mine = s.cqq[me] > 0;
                float best = 0.0f;
                for (int t = 0; t < TK_SLOTS; t++) {
                    if (!s.tfree[t] || !(any_class || s.cls[t] == bcls)) continue;
                    const float iou = box_iou(box_edges(s.px[t], s.py[t], s.w[t], s.h[t]), bx, by, bw, bh);
                    if constexpr (COS) {
                        float key = iou;
                        bool ok = iou >= thresh;
                        if (mine && s.ee[t] > 0) {
                            const float cs = sm[(size_t)t * TK_CAND + me];
                            if (cs >= app_thresh && iou >= app_min_iou) { key = fmaxf(iou, cs); ok = true; }
                        }
                        if (ok && (pick < 0 || key > best)) { best = key; pick = t; } // ties: the lower slot stays
                    } else { // (as above)
                        if (iou >= thresh && (pick < 0 || iou > best)) { best = iou; pick = t; }
                    }
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

// what mhip_track and mhip_track_app both ask of the mhip_track_t part
static inline bool tk_args_ok(const mhip_track_t *p) {
    if (!p->dets || !p->counts || !p->out || !p->states || !p->hdr) return false;
    if (p->streams < 1 || p->streams > 65535 || p->steps < 1 || p->max_det < 1 || p->max_det > 1000) return false;
    return p->min_conf > 0.0f && p->low_conf >= 0.0f && p->iou > 0.0f && p->iou_low > 0.0f && p->max_miss >= 1 && p->cls_count >= 0;
}
