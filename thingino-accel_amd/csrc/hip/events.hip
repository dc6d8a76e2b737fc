// events.hip -- events from tracks on gfx950: the detection lists and the track ids a tracking call left in HBM (or a caller's lists) ->
// line crossings, zone entry, exit and dwell per detection, per frame and per stream, the tables of S camera streams held in HBM between
// calls.
//
// include/mars_hip.h ("Events") states the arithmetic.  One launch, one workgroup of 512 threads per stream, which walks the stream's frames
// of the call in order, as track.hip does.  Thread s < 256 owns slot s and keeps {id, last_step, q, inside, dwelled} in registers from the
// first step of the call to the last; since[] stays in HBM, touched by the owner alone and only for a zone that is entered or whose dwell
// can fire.  Thread k < 197 also keeps one of the stream's int64 totals in a register.  Per step:
//   expiry        a thread per slot;
//   participants  every entry's id (0: it is no candidate) goes into LDS, each candidate looks for its id at a lower index (every lane reads
//                 the same address: a broadcast), and the ones left are compacted in index order by track_core.hpp's ballot prefix scan,
//                 their anchors quantised on the way: position = rank, no atomics;
//   lookup        a used slot scans the participants' ids for its own; two more scans give "free slots by ascending slot, new ids by
//                 ascending index", as the tracker's births;
//   geometry      the slot's owner judges its participant.  The loops over the lines and the zones are uniform across the workgroup and
//                 the rules come through a const __restrict__ kernel argument, so the compiler keeps vertices and counts in scalar registers;
//                 all products are int64.  The per-frame counts are ballot popcounts inside those loops, one LDS add per wave: integer
//                 sums, so the order does not matter.
// LDS: about 12 KB (the sort + NMS kernel's comment in yolo_tail.hip records what a large tail does to the next batch's convolutions).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "track_core.hpp"

#pragma clang fp contract(off)

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

struct ev_slot_t { int id, last_step, qx, qy; unsigned inside, dwelled; int since[MHIP_EVENTS_ZONES]; }; // mars_event_slot_t
struct ev_rec_t { unsigned zones, entered, exited, dwelled, lines_in, lines_out; };                      // mars_event_t
static_assert(sizeof(ev_slot_t) == 152 && sizeof(ev_rec_t) == 24, "record sizes of include/mars_hip.h");

// the accumulators of one step: the frame's line and zone counts as they are stored, then what only the totals take
#define EV_ACC_LINES 0
#define EV_ACC_ZONES (2 * MHIP_EVENTS_LINES)
#define EV_ACC_LOST (EV_ACC_ZONES + 4 * MHIP_EVENTS_ZONES)
#define EV_ACC_FIRST (EV_ACC_LOST + MHIP_EVENTS_ZONES)
#define EV_ACC_EXPIRED (EV_ACC_FIRST + 1)
#define EV_ACC_OVERFLOW (EV_ACC_FIRST + 2)
#define EV_ACC_DROPPED (EV_ACC_FIRST + 3)
#define EV_ACC_DUPLICATES (EV_ACC_FIRST + 4)
#define EV_ACC (EV_ACC_FIRST + 5)

struct ev_lds_t {
    int cid[MAXD];                        // the id an entry brings, 0: it is no candidate
    int pid[TK_CAND], pqx[TK_CAND], pqy[TK_CAND]; // the participants: id and quantised anchor
    short pidx[TK_CAND], pslot[TK_CAND];  // index in the frame's list; the slot that holds the id, or -1
    short take[TK_SLOTS], freelist[TK_SLOTS]; // the participant a free slot is given, or -1
    int acc[EV_ACC];
    int wsum[TK_WAVES];
};

// which accumulator total k of mhip_events_hdr_t takes
__device__ __forceinline__ int ev_total_src(const int k) {
    if (k < EV_ACC_ZONES) return k;                                        // [line][in, out]
    if (k >= EV_ACC_LOST) return EV_ACC_FIRST + (k - EV_ACC_LOST);         // the five counters
    const int z = (k - EV_ACC_ZONES) >> 2, j = (k - EV_ACC_ZONES) & 3;     // [zone][entered, exited, dwelled, lost]
    return j == 3 ? EV_ACC_LOST + z : EV_ACC_ZONES + 4 * z + j + 1;
}

// the number of threads of the wave with `flag` is added to *acc.  Called under wave-uniform control flow
__device__ __forceinline__ void ev_count(int *acc, const bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(acc, __popcll(m));
}

__device__ __forceinline__ long long ev_cross(const int ux, const int uy, const int vx, const int vy) {
    return (long long)ux * vy - (long long)uy * vx;
}

__device__ __forceinline__ int ev_quantise(const float a) {
    const float c = fminf(fmaxf(a, -32768.0f), 32768.0f);
    return (int)floorf(c * 16.0f);
}

// grid: streams
__global__ __launch_bounds__(TK_THREADS) void events_kernel(const mhip_events_t p, const mhip_event_rules_t *__restrict__ rules) {
    __shared__ ev_lds_t s;
    const int tid = threadIdx.x, b = blockIdx.x;
    const mhip_event_rules_t &R = rules[b];
    const int nl = R.n_lines, nz = R.n_zones;
    const bool owner = tid < TK_SLOTS; // (uniform in a wave)
    ev_slot_t *slot = (ev_slot_t *)p.slots + (size_t)b * TK_SLOTS + (owner ? tid : 0);
    int id = 0, last = 0, qx = 0, qy = 0;
    unsigned inside = 0, dwelled = 0;
    if (owner) { id = slot->id; last = slot->last_step; qx = slot->qx; qy = slot->qy; inside = slot->inside; dwelled = slot->dwelled; }
    long long total = 0;
    const int src = ev_total_src(tid < MHIP_EVENTS_TOTALS ? tid : 0);
    if (tid < MHIP_EVENTS_TOTALS) total = p.hdr[b].tot[tid];
    int step = p.hdr[b].step;
    for (int t = 0; t < p.steps; t++, step++) {
        const size_t f = p.stream_major ? (size_t)b * p.steps + t : (size_t)t * p.streams + b;
        const det_t *d = (const det_t *)p.dets + f * p.max_det;
        const tk_out_t *tr = (const tk_out_t *)p.tracks + f * p.max_det;
        ev_rec_t *o = (ev_rec_t *)p.records + f * p.max_det;
        int n = p.counts[f];
        n = n < 0 ? 0 : n > p.max_det ? p.max_det : n;
        for (int i = tid; i < p.max_det; i += TK_THREADS) o[i] = ev_rec_t{0, 0, 0, 0, 0, 0};
        if (tid < EV_ACC) s.acc[tid] = 0;
        // expiry
        unsigned lost = 0;
        bool expired = false;
        if (owner && id != 0 && step - last > p.max_gap) { lost = inside; id = 0; expired = true; }
        if (owner) s.take[tid] = -1;
        // the candidates' ids
        for (int i = tid; i < n; i += TK_THREADS) {
            const tk_out_t k = tr[i];
            const det_t v = d[i];
            const bool cand = k.id >= 1 && k.hits >= p.min_hits && tk_finite(v.x) && tk_finite(v.y) && tk_finite(v.w) && tk_finite(v.h);
            s.cid[i] = cand ? k.id : 0;
        }
        __syncthreads();
        if (owner) {
            ev_count(&s.acc[EV_ACC_EXPIRED], expired);
            for (int z = 0; z < nz; z++) ev_count(&s.acc[EV_ACC_LOST + z], (lost >> z) & 1u);
        }
        // participants: a candidate whose id no lower index brings, the first TK_CAND of them
        int running = 0;
        for (int c0 = 0; c0 < n; c0 += TK_THREADS) { // (n is the same in every thread)
            const int i = c0 + tid;
            const int myid = i < n ? s.cid[i] : 0;
            bool part = myid != 0;
            if (part) {
                for (int j = 0; j < i; j++)
                    if (s.cid[j] == myid) { part = false; break; }
                if (!part) atomicAdd(&s.acc[EV_ACC_DUPLICATES], 1);
            }
            int cnt;
            const int pos = running + tk_scan(part, s.wsum, cnt);
            if (part && pos < TK_CAND) {
                const det_t v = d[i];
                float ay = v.y;
                if (p.anchor_bottom) {
                    const float half = v.h * 0.5f;
                    ay = v.y + half;
                }
                s.pid[pos] = myid; s.pqx[pos] = ev_quantise(v.x); s.pqy[pos] = ev_quantise(ay);
                s.pidx[pos] = (short)i;
                s.pslot[pos] = -1;
            }
            running += cnt;
        }
        const int np = running < TK_CAND ? running : TK_CAND;
        __syncthreads();
        // lookup: the slot that holds a participant's id
        int m = -1;
        if (owner && id != 0) {
            for (int j = 0; j < np; j++)
                if (s.pid[j] == id) { m = j; break; }
            if (m >= 0) s.pslot[m] = (short)tid;
        }
        // ... and for the others free slot r and new id r meet
        const bool is_free = owner && id == 0;
        int nfree, nnew;
        const int r = tk_scan(is_free, s.wsum, nfree); // (its barriers publish pslot)
        if (is_free) s.freelist[r] = (short)tid;
        const bool wants = tid < np && s.pslot[tid] < 0;
        const int bi = tk_scan(wants, s.wsum, nnew); // (its barriers publish the free list)
        const int fits = nnew < nfree ? nnew : nfree;
        if (wants && bi < fits) s.take[s.freelist[bi]] = (short)tid;
        if (tid == 0) { s.acc[EV_ACC_OVERFLOW] = running - np; s.acc[EV_ACC_DROPPED] = nnew - fits; }
        __syncthreads();
        bool first = false;
        if (is_free) {
            m = s.take[tid];
            first = m >= 0;
        }
        // geometry: the slot's owner judges its participant
        if (owner) {
            const bool has = m >= 0, again = has && !first;
            int Qx = 0, Qy = 0;
            if (has) { Qx = s.pqx[m]; Qy = s.pqy[m]; }
            ev_rec_t rec = ev_rec_t{0, 0, 0, 0, 0, 0};
            for (int l = 0; l < nl; l++) {
                const int ax = R.lines[l][0], ay = R.lines[l][1], bx = R.lines[l][2], by = R.lines[l][3];
                bool in = false, out = false;
                if (again) {
                    const bool sp = ev_cross(bx - ax, by - ay, qx - ax, qy - ay) >= 0, sq = ev_cross(bx - ax, by - ay, Qx - ax, Qy - ay) >= 0;
                    if (sp != sq) {
                        const bool da = ev_cross(Qx - qx, Qy - qy, ax - qx, ay - qy) >= 0, db = ev_cross(Qx - qx, Qy - qy, bx - qx, by - qy) >= 0;
                        if (da != db) { in = sq; out = !sq; }
                    }
                }
                if (in) rec.lines_in |= 1u << l;
                if (out) rec.lines_out |= 1u << l;
                ev_count(&s.acc[EV_ACC_LINES + 2 * l], in);
                ev_count(&s.acc[EV_ACC_LINES + 2 * l + 1], out);
            }
            for (int z = 0; z < nz; z++) {
                const int nv = R.zones[z].n, dwell = R.zones[z].dwell;
                const unsigned bit = 1u << z;
                bool now = false, entered = false, exited = false, fired = false;
                if (has) {
                    int vx = R.zones[z].x[0], vy = R.zones[z].y[0];
                    for (int e = 0; e < nv; e++) { // edge (V, W), closing back to the first vertex
                        const int w = e + 1 < nv ? e + 1 : 0;
                        const int wx = R.zones[z].x[w], wy = R.zones[z].y[w];
                        if ((vy > Qy) != (wy > Qy)) {
                            const int dy = wy - vy;
                            const long long lhs = (long long)(Qx - vx) * dy, rhs = (long long)(wx - vx) * (Qy - vy);
                            if (dy > 0 ? lhs < rhs : lhs > rhs) now = !now;
                        }
                        vx = wx; vy = wy;
                    }
                    if (first) {
                        if (now) slot->since[z] = step;
                    } else {
                        const bool was = (inside & bit) != 0;
                        entered = now && !was;
                        exited = was && !now;
                        if (entered) slot->since[z] = step;
                        if (entered || exited) dwelled &= ~bit;
                        if (now && was && dwell > 0 && !(dwelled & bit) && step - slot->since[z] >= dwell) { fired = true; dwelled |= bit; }
                    }
                }
                if (now) rec.zones |= bit;
                if (entered) rec.entered |= bit;
                if (exited) rec.exited |= bit;
                if (fired) rec.dwelled |= bit;
                ev_count(&s.acc[EV_ACC_ZONES + 4 * z], now);
                ev_count(&s.acc[EV_ACC_ZONES + 4 * z + 1], entered);
                ev_count(&s.acc[EV_ACC_ZONES + 4 * z + 2], exited);
                ev_count(&s.acc[EV_ACC_ZONES + 4 * z + 3], fired);
            }
            ev_count(&s.acc[EV_ACC_FIRST], first);
            if (has) {
                if (first) { id = s.pid[m]; dwelled = 0; }
                inside = rec.zones; qx = Qx; qy = Qy; last = step;
                o[s.pidx[m]] = rec; // (behind the zeros of the loop above: the scans' barriers lie between)
            }
        }
        __syncthreads();
        if (tid < MHIP_EVENTS_TOTALS) total += s.acc[src];
        if (tid < EV_ACC_ZONES) p.line_counts[f * EV_ACC_ZONES + tid] = s.acc[tid];
        else if (tid < EV_ACC_LOST) p.zone_counts[f * (4 * MHIP_EVENTS_ZONES) + (tid - EV_ACC_ZONES)] = s.acc[tid];
        __syncthreads(); // (the next step clears the accumulators)
    }
    if (owner) { slot->id = id; slot->last_step = last; slot->qx = qx; slot->qy = qy; slot->inside = inside; slot->dwelled = dwelled; }
    if (tid < MHIP_EVENTS_TOTALS) p.hdr[b].tot[tid] = total;
    if (tid == 0) p.hdr[b].step = step;
}

// ---- launcher
extern "C" int mhip_events(const mhip_events_t *p) {
    if (!p || !p->dets || !p->tracks || !p->counts || !p->records || !p->line_counts || !p->zone_counts || !p->slots || !p->hdr || !p->rules) return -1;
    if (p->streams < 1 || p->streams > 65535 || p->steps < 1 || p->max_det < 1 || p->max_det > MAXD) return -1;
    if (p->max_gap < 1 || p->min_hits < 1) return -1;
    hipLaunchKernelGGL(events_kernel, dim3((unsigned)p->streams), dim3(TK_THREADS), 0, mhip_stream_native(), *p, p->rules);
    return mhip_check(hipGetLastError(), "events");
}
