// shots.hip -- best shots on gfx950: the crops in a second model's input, their ROI table and the track ids a tracking call left in HBM (or
// a caller's lists) -> a quality measure per crop and, per camera stream, a table that keeps the best crop of every live track with its
// pixels until the track has ended.
//
// include/mars_hip.h ("Best shots") states the arithmetic.  Three launches, no atomic decides anything: which crop wins is a function of
// the lists alone.
//   shot_metrics_kernel<NHWC>  the hot path: every byte of every kept crop is read once.  A workgroup of 256 threads owns a band of
//                 mhip_shots_band_rows rows of one crop (16 at the second model's 160 x 160: 10 bands a crop, 640 workgroups at 64 crops
//                 for 256 CUs, and one halo row in 16 read twice).  It needs the band's content rows plus one row above and below
//                 (three plane rows each under NCHW).  Where they start on 16-byte boundaries -- the second model's input -- a lane
//                 loads 16 pixels with three 16-byte loads and forms their luma in registers; otherwise the rows are staged in LDS, 16
//                 bytes per lane where a whole aligned chunk lies inside them, byte by byte at the two ragged ends -- the LDS image
//                 keeps the global address modulo 16, so both sides of a copy are aligned whatever the crop's base is.  Luma is formed
//                 once per pixel into an LDS array, the Laplacian reads that array alone (4 pixels from 5 dwords where the width is a
//                 multiple of 4), the two sums go through a cross-lane reduction per wave and an LDS cell per wave, and the band's pair
//                 of int64 goes to HBM.  The walk adds the bands in ascending order: integer sums, exact whatever the cut.
//   shot_walk_kernel  one workgroup of 512 threads per stream walks the stream's steps in order, as events.hip does; thread s owns slot s
//                 and keeps it in registers for the whole call.  Per step: expiry; the metrics of the step's crops finished from the band
//                 partials and their scores; the candidates' ids into a scratch array in HBM (a crop belongs to one step of one stream,
//                 so nobody else writes its cell; read back past the vector cache); per chunk of 512 crops the candidates' ids compacted
//                 into LDS in index order and duplicates dropped by a scan of the ids in front (and, for a batch beyond 512 crops, of
//                 the earlier chunks' cells in HBM); the rest compacted by track_core.hpp's ballot prefix scan; lookup; free slots then finished slots handed
//                 out by two more scans; the owner judges its participant and notes the crop it stored.
//   shot_copy_kernel  a workgroup per table slot: the slot's final winner of this call, and only that one, goes into the plane, 16 bytes
//                 per lane where the source is aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "track_core.hpp"

#pragma clang fp contract(off)

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

struct sh_roi_t { int frame, det, x0, y0, x1, y1; };                                   // mars_roi_t
struct sh_rec_t { long long score; int sharp, mean, slot, taken; };                    // mars_shot_t
struct sh_slot_t { int id, state, first_step, last_step, best_step, seen, taken, cls; float conf; int x0, y0, x1, y1, sharp, mean, pad; long long score; }; // mars_shot_slot_t
static_assert(sizeof(sh_roi_t) == 24 && sizeof(sh_rec_t) == 24 && sizeof(sh_slot_t) == 72, "record sizes of include/mars_hip.h");
struct sh_geom_t { int nw, nh, px, py; };

#define SH_FREE 0
#define SH_LIVE 1
#define SH_DONE 2
#define SH_THREADS 256 // of the metrics and the copy kernel
#define SH_WAVES (SH_THREADS / 64)
// the counters of mhip_shots_hdr_t
#define SH_FINISHED 0
#define SH_LOST 1
#define SH_DROPPED 2
#define SH_OVERFLOW 3
#define SH_DUPLICATES 4
#define SH_TAKEN 5

// the content rectangle of a crop inside its tw x th target; false: the crop has no content
__device__ __forceinline__ bool sh_content(const mhip_shots_t &p, const sh_roi_t r, sh_geom_t &g) {
    if (r.x1 <= r.x0 || r.y1 <= r.y0 || r.frame < 0 || r.frame >= p.streams * p.steps) return false;
    g = sh_geom_t{p.tw, p.th, 0, 0};
    if (p.keep_aspect) {
        const long long cw = (long long)r.x1 - r.x0, ch = (long long)r.y1 - r.y0;
        if (cw * p.th >= ch * p.tw) {
            const long long v = (ch * p.tw + cw / 2) / cw;
            g.nh = (int)(v < 1 ? 1 : v > p.th ? p.th : v);
        } else {
            const long long v = (cw * p.th + ch / 2) / ch;
            g.nw = (int)(v < 1 ? 1 : v > p.tw ? p.tw : v);
        }
        g.px = (p.tw - g.nw) / 2;
        g.py = (p.th - g.nh) / 2;
    }
    return true;
}

__device__ __forceinline__ int sh_kept(const mhip_shots_t &p) {
    const int n = p.kept ? *p.kept : p.n_crops;
    return n < 0 ? 0 : n > p.n_crops ? p.n_crops : n;
}

// ---- the metrics.  grid: (n_crops, bands).  Dynamic LDS: the staged spans (one of rows x tw x 3 bytes, or three of rows x tw), each with
// room for the 15 bytes in front of an unaligned start, then rows x tw bytes of luma
template <bool NHWC>
__global__ __launch_bounds__(SH_THREADS) void shot_metrics_kernel(const mhip_shots_t p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sh_lds[];
    __shared__ long long red[2][SH_WAVES];
    const int k = blockIdx.x, band = blockIdx.y, tid = threadIdx.x;
    if (band == 0 && tid == 0) ((sh_rec_t *)p.records)[k] = sh_rec_t{0, 0, 0, -1, 0}; // (the walk overwrites it where the crop has content)
    if (k >= sh_kept(p)) return;
    sh_geom_t g;
    if (!sh_content(p, ((const sh_roi_t *)p.rois)[k], g)) return;
    long long *out = p.partials + ((size_t)k * p.bands + band) * 2;
    const int r0 = band * p.band_rows, r1 = r0 + p.band_rows < p.th ? r0 + p.band_rows : p.th;
    const int c0 = r0 > g.py ? r0 : g.py, c1 = r1 < g.py + g.nh ? r1 : g.py + g.nh; // the band's content rows
    if (c0 >= c1) {
        if (tid == 0) { out[0] = 0; out[1] = 0; }
        return;
    }
    const int rlo = c0 - 1 > g.py ? c0 - 1 : g.py, rhi = c1 + 1 < g.py + g.nh ? c1 + 1 : g.py + g.nh; // ... and a halo row of content either side
    const int rows = rhi - rlo, tw = p.tw;
    constexpr int SPANS = NHWC ? 1 : 3;
    const int len = rows * tw * (NHWC ? 3 : 1);
    const int cap = ((len + 15) & ~15) + 32;
    const int8_t *crop = p.crops + (size_t)k * p.crop_stride;
    const int npix = rows * tw;
    uint8_t *Y = sh_lds + SPANS * cap; // (16-byte aligned: cap is a multiple of 16)
    int shift[SPANS];
    bool aligned = true;
#pragma unroll
    for (int sp = 0; sp < SPANS; sp++) {
        const int8_t *src = crop + (NHWC ? (size_t)rlo * tw * 3 : ((size_t)sp * p.th + rlo) * tw);
        shift[sp] = (int)((uintptr_t)src & 15);
        aligned = aligned && shift[sp] == 0;
    }
    if (aligned) {
        // every span starts on a 16-byte boundary (the second model's input does): no staging.  A lane loads 16 pixels -- three 16-byte
        // loads, consecutive bytes under NHWC, one per plane under NCHW --, forms their luma in registers and stores 16 bytes of Y
        const int groups = npix >> 4;
        for (int gi = tid; gi < groups; gi += SH_THREADS) {
            unsigned w[12];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint4 v = NHWC ? ((const uint4 *)(crop + (size_t)rlo * tw * 3))[3 * gi + q] : ((const uint4 *)(crop + ((size_t)q * p.th + rlo) * tw))[gi];
                w[4 * q] = v.x ^ 0x80808080u; w[4 * q + 1] = v.y ^ 0x80808080u; w[4 * q + 2] = v.z ^ 0x80808080u; w[4 * q + 3] = v.w ^ 0x80808080u;
            }
            unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int nr = NHWC ? 3 * j : j, ng = NHWC ? 3 * j + 1 : 16 + j, nb = NHWC ? 3 * j + 2 : 32 + j; // byte numbers in w
                const unsigned R = (w[nr >> 2] >> ((nr & 3) * 8)) & 255u, G = (w[ng >> 2] >> ((ng & 3) * 8)) & 255u, B = (w[nb >> 2] >> ((nb & 3) * 8)) & 255u;
                o[j >> 2] |= ((77u * R + 150u * G + 29u * B + 128u) >> 8) << ((j & 3) * 8);
            }
            ((uint4 *)Y)[gi] = uint4{o[0], o[1], o[2], o[3]};
        }
        for (int i = (groups << 4) + tid; i < npix; i += SH_THREADS) { // the last pixels, fewer than 16
            int R, G, B;
            if constexpr (NHWC) {
                const int8_t *q = crop + (size_t)rlo * tw * 3 + 3 * i;
                R = q[0] + 128; G = q[1] + 128; B = q[2] + 128;
            } else {
                const int8_t *q = crop + (size_t)rlo * tw + i;
                R = q[0] + 128; G = q[(size_t)p.th * tw] + 128; B = q[2 * (size_t)p.th * tw] + 128;
            }
            Y[i] = (uint8_t)((77 * R + 150 * G + 29 * B + 128) >> 8);
        }
    }
#pragma unroll
    for (int sp = 0; sp < SPANS && !aligned; sp++) {
        const int8_t *src = crop + (NHWC ? (size_t)rlo * tw * 3 : ((size_t)sp * p.th + rlo) * tw);
        const int8_t *a0 = src - shift[sp]; // (only chunks that lie inside [src, src + len) are read whole)
        uint8_t *dst = sh_lds + sp * cap;
        const int chunks = (shift[sp] + len + 15) >> 4;
        for (int c = tid; c < chunks; c += SH_THREADS) {
            const int b0 = c << 4;
            if (b0 >= shift[sp] && b0 + 16 <= shift[sp] + len) {
                *(uint4 *)(dst + b0) = *(const uint4 *)(a0 + b0);
            } else {
                const int lo = b0 > shift[sp] ? b0 : shift[sp], hi = b0 + 16 < shift[sp] + len ? b0 + 16 : shift[sp] + len;
                for (int i = lo; i < hi; i++) dst[i] = (uint8_t)a0[i];
            }
        }
    }
    if (!aligned) __syncthreads(); // (uniform in the workgroup)
    for (int i = tid; i < npix && !aligned; i += SH_THREADS) { // luma, once per staged pixel; byte + 128 == byte ^ 0x80
        int R, G, B;
        if constexpr (NHWC) {
            const uint8_t *q = sh_lds + shift[0] + 3 * i;
            R = q[0] ^ 0x80; G = q[1] ^ 0x80; B = q[2] ^ 0x80;
        } else {
            R = sh_lds[shift[0] + i] ^ 0x80; G = sh_lds[cap + shift[SPANS > 1 ? 1 : 0] + i] ^ 0x80; B = sh_lds[2 * cap + shift[SPANS > 2 ? 2 : 0] + i] ^ 0x80;
        }
        Y[i] = (uint8_t)((77 * R + 150 * G + 29 * B + 128) >> 8);
    }
    __syncthreads();
    int sum_y = 0;
    unsigned long long sum_l = 0;
    const int nw = g.nw, x_last = g.nw - 1, y_first = g.py + 1, y_last = g.py + g.nh - 1;
    if ((tw & 3) == 0) {
        // rows of Y start on a 4-byte boundary: a lane takes 4 pixels from 5 dwords (itself, left, right, above, below)
        const int gpr = tw >> 2;
        for (int gi = tid; gi < (c1 - c0) * gpr; gi += SH_THREADS) {
            const int yy = gi / gpr, x4 = (gi - yy * gpr) << 2, y = c0 + yy;
            if (x4 + 3 < g.px || x4 >= g.px + nw) continue;
            const unsigned *row = (const unsigned *)(Y + (y - rlo) * tw) + (x4 >> 2);
            const bool yin = y >= y_first && y < y_last; // (then the rows above and below are staged)
            const unsigned C = row[0];
            unsigned Lw = 0, Rw = 0, U = 0, D = 0;
            if (yin) {
                if (x4 > 0) Lw = row[-1];
                if (x4 + 4 < tw) Rw = row[1];
                U = row[-gpr]; D = row[gpr];
            }
            const int h[6] = {(int)(Lw >> 24), (int)(C & 255u), (int)((C >> 8) & 255u), (int)((C >> 16) & 255u), (int)(C >> 24), (int)(Rw & 255u)};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int xx = x4 + j - g.px;
                if (xx < 0 || xx >= nw) continue;
                const int v = h[j + 1];
                sum_y += v;
                if (yin && xx >= 1 && xx < x_last) { // (a neighbour taken from a zero word lies outside the content: not reached)
                    const int L = 4 * v - h[j] - h[j + 2] - (int)((U >> (8 * j)) & 255u) - (int)((D >> (8 * j)) & 255u);
                    sum_l += (unsigned)(L * L);
                }
            }
        }
    }
    for (int i = tid; i < (c1 - c0) * nw && (tw & 3) != 0; i += SH_THREADS) {
        const int yy = i / nw, xx = i - yy * nw, y = c0 + yy;
        const uint8_t *q = Y + (y - rlo) * tw + g.px + xx;
        const int v = q[0];
        sum_y += v;
        if (xx >= 1 && xx < x_last && y >= y_first && y < y_last) { // four neighbours inside the content: all staged
            const int L = 4 * v - q[-1] - q[1] - q[-tw] - q[tw];
            sum_l += (unsigned)(L * L);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        sum_y += __shfl_xor(sum_y, d);
        sum_l += __shfl_xor(sum_l, d);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = sum_y; red[1][tid >> 6] = (long long)sum_l; }
    __syncthreads();
    if (tid == 0) {
        long long a = 0, b = 0;
        for (int w = 0; w < SH_WAVES; w++) { a += red[0][w]; b += red[1][w]; }
        out[0] = a; out[1] = b;
    }
}

// ---- the walk
struct sh_lds_t {
    int pid[TK_CAND], pidx[TK_CAND], psharp[TK_CAND], pmean[TK_CAND]; // the participants: id, crop index, metrics
    long long pscore[TK_CAND];
    short pslot[TK_CAND];                     // the LIVE slot that holds the id, or -1
    int cid[TK_THREADS];                      // the ids the candidates of a chunk of TK_THREADS crops bring, in index order
    short take[TK_SLOTS], freelist[TK_SLOTS]; // the participant a slot is given, or -1; the FREE slots, then the DONE ones, by ascending slot
    int acc[MHIP_SHOTS_COUNTERS];
    int wsum[TK_WAVES];
};

// the number of threads of the wave with `flag` is added to *acc.  Every thread of the workgroup calls it
__device__ __forceinline__ void sh_count(int *acc, const bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(acc, __popcll(m));
}

// what the lists say about crop k: confidence, class, track
__device__ __forceinline__ void sh_entry(const mhip_shots_t &p, const int k, const sh_roi_t r, float &conf, int &cls, tk_out_t &tr) {
    conf = 0.0f; cls = 0; tr = tk_out_t{-1, 0};
    if (p.det_cap == 0) {
        conf = p.confs[k]; cls = p.cls[k]; tr = ((const tk_out_t *)p.tracks)[k];
    } else if (r.det >= 0 && r.det < p.det_cap) { // (r.frame is inside the call's frames: the crop has content)
        const size_t i = (size_t)r.frame * p.det_cap + r.det;
        const det_t d = ((const det_t *)p.dets)[i];
        conf = d.conf; cls = d.cls; tr = ((const tk_out_t *)p.tracks)[i];
    }
}

// grid: streams
__global__ __launch_bounds__(TK_THREADS) void shot_walk_kernel(const mhip_shots_t p) {
    __shared__ sh_lds_t s;
    const int tid = threadIdx.x, b = blockIdx.x;
    const bool owner = tid < p.slots;
    sh_slot_t *slot = (sh_slot_t *)p.table + (size_t)b * p.slots + (owner ? tid : 0);
    const sh_roi_t *rois = (const sh_roi_t *)p.rois;
    sh_rec_t *recs = (sh_rec_t *)p.records;
    sh_slot_t sl = sh_slot_t{0, 0, 0, 0, 0, 0, 0, 0, 0.0f, 0, 0, 0, 0, 0, 0, 0, 0};
    if (owner) sl = *slot;
    int lastk = -1;
    long long total = tid < MHIP_SHOTS_COUNTERS ? p.hdr[b].cnt[tid] : 0;
    int step = p.hdr[b].step;
    const int kept = sh_kept(p);
    const long long T = (long long)p.tw * p.th;
    for (int t = 0; t < p.steps; t++, step++) {
        const int f = p.stream_major ? b * p.steps + t : t * p.streams + b;
        if (tid < MHIP_SHOTS_COUNTERS) s.acc[tid] = 0;
        // expiry
        const bool expired = owner && sl.state == SH_LIVE && step - sl.last_step > p.max_gap;
        if (expired) sl.state = SH_DONE;
        if (owner) s.take[tid] = -1;
        __syncthreads();
        sh_count(&s.acc[SH_FINISHED], expired);
        // the step's crops: metrics from the band partials, the score, the record, and the id each brings as a candidate
        for (int k = tid; k < kept; k += TK_THREADS) {
            const sh_roi_t r = rois[k];
            if (r.frame != f) continue;
            sh_geom_t g;
            int id = 0;
            if (sh_content(p, r, g)) {
                const long long *part = p.partials + (size_t)k * p.bands * 2;
                long long sy = 0, sq = 0;
                for (int bd = 0; bd < p.bands; bd++) { sy += part[2 * bd]; sq += part[2 * bd + 1]; }
                const int mean = (int)(sy / ((long long)g.nw * g.nh));
                const int sharp = g.nw < 3 || g.nh < 3 ? 0 : (int)(sq / ((long long)(g.nw - 2) * (g.nh - 2)));
                float conf; int cls; tk_out_t tr;
                sh_entry(p, k, r, conf, cls, tr);
                const long long cw = (long long)r.x1 - r.x0, ch = (long long)r.y1 - r.y0;
                const long long a = cw >= T || ch >= T ? T : cw * ch < T ? cw * ch : T;
                int c = 0;
                if (tk_finite(conf)) c = (int)floorf(fminf(fmaxf(conf, 0.0f), 1.0f) * 1024.0f);
                recs[k] = sh_rec_t{a * (sharp + 1) * c, sharp, mean, -1, 0};
                bool cand = tr.id >= 1 && tr.hits >= p.min_hits && sharp >= p.min_sharp;
                if (p.min_mean != 0 || p.max_mean != 0) cand = cand && mean >= p.min_mean && mean <= p.max_mean;
                if (p.inside) cand = cand && r.x0 > 0 && r.y0 > 0 && r.x1 < p.src_w && r.y1 < p.src_h;
                if (cand) id = tr.id;
            }
            __hip_atomic_store(&p.cand[k], id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads(); // (the stores above have left the wave: s_waitcnt in front of the barrier)
        // participants: a candidate whose id no lower index of the step brings, the first TK_CAND of them
        int running = 0;
        for (int c0 = 0; c0 < kept; c0 += TK_THREADS) { // (kept is the same in every thread)
            const int k = c0 + tid;
            int myid = 0;
            if (k < kept && rois[k].frame == f) myid = __hip_atomic_load(&p.cand[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool part = myid != 0;
            int cnt;
            const int before = tk_scan(part, s.wsum, cnt); // the chunk's candidates before this one
            if (part) s.cid[before] = myid;
            __syncthreads();
            if (part) {
                for (int q = 0; q < before; q++)
                    if (s.cid[q] == myid) { part = false; break; }
                for (int j = 0; part && j < c0; j++) // (batches beyond TK_THREADS crops only: the chunks in front, from HBM)
                    if (rois[j].frame == f && __hip_atomic_load(&p.cand[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == myid) part = false;
                if (!part) atomicAdd(&s.acc[SH_DUPLICATES], 1);
            }
            const int pos = running + tk_scan(part, s.wsum, cnt);
            if (part && pos < TK_CAND) { // (tk_scan's barrier lies behind the readers of cid)
                const sh_rec_t v = recs[k]; // (this thread's own store)
                s.pid[pos] = myid; s.pidx[pos] = k; s.psharp[pos] = v.sharp; s.pmean[pos] = v.mean; s.pscore[pos] = v.score;
                s.pslot[pos] = -1;
            }
            running += cnt;
        }
        const int np = running < TK_CAND ? running : TK_CAND;
        __syncthreads();
        // lookup: the LIVE slot that holds a participant's id
        int m = -1;
        if (owner && sl.state == SH_LIVE) {
            for (int j = 0; j < np; j++)
                if (s.pid[j] == sl.id) { m = j; break; }
            if (m >= 0) s.pslot[m] = (short)tid;
        }
        // ... and for the others: FREE slots by ascending slot, then DONE slots by ascending slot, meet the new ids by ascending index
        const bool is_free = owner && sl.state == SH_FREE, is_done = owner && sl.state == SH_DONE;
        int nfree, ndone, nnew;
        const int rf = tk_scan(is_free, s.wsum, nfree); // (its barriers publish pslot)
        if (is_free) s.freelist[rf] = (short)tid;
        const int rd = tk_scan(is_done, s.wsum, ndone);
        if (is_done) s.freelist[nfree + rd] = (short)tid;
        const bool wants = tid < np && s.pslot[tid] < 0;
        const int bi = tk_scan(wants, s.wsum, nnew); // (its barriers publish the free list)
        const int avail = nfree + ndone, fits = nnew < avail ? nnew : avail;
        if (wants && bi < fits) s.take[s.freelist[bi]] = (short)tid;
        if (tid == 0) {
            s.acc[SH_OVERFLOW] = running - np;
            s.acc[SH_DROPPED] = nnew - fits;
            s.acc[SH_LOST] = fits > nfree ? fits - nfree : 0;
        }
        __syncthreads();
        bool first = false;
        if (is_free || is_done) {
            m = s.take[tid];
            first = m >= 0;
        }
        // the slot's owner judges its participant
        bool stored = false;
        if (owner && m >= 0) {
            const int k = s.pidx[m];
            const long long score = s.pscore[m];
            if (first) {
                sl.id = s.pid[m]; sl.state = SH_LIVE; sl.first_step = step; sl.seen = 1; sl.taken = 1; sl.pad = 0;
                stored = true;
            } else {
                sl.seen += 1;
                if (score > sl.score) { stored = true; sl.taken += 1; }
            }
            if (stored) {
                const sh_roi_t r = rois[k];
                tk_out_t tr;
                sh_entry(p, k, r, sl.conf, sl.cls, tr);
                sl.x0 = r.x0; sl.y0 = r.y0; sl.x1 = r.x1; sl.y1 = r.y1;
                sl.sharp = s.psharp[m]; sl.mean = s.pmean[m]; sl.score = score; sl.best_step = step;
                lastk = k;
            }
            sl.last_step = step;
            recs[k] = sh_rec_t{score, s.psharp[m], s.pmean[m], tid, stored ? 1 : 0};
        }
        sh_count(&s.acc[SH_TAKEN], stored);
        __syncthreads();
        if (tid < MHIP_SHOTS_COUNTERS) total += s.acc[tid];
        __syncthreads(); // (the next step clears the accumulators)
    }
    if (owner) {
        *slot = sl;
        p.last[(size_t)b * p.slots + tid] = lastk;
    }
    if (tid < MHIP_SHOTS_COUNTERS) p.hdr[b].cnt[tid] = total;
    if (tid == 0) p.hdr[b].step = step;
}

// ---- the copy.  grid: streams * slots
__global__ __launch_bounds__(SH_THREADS) void shot_copy_kernel(const mhip_shots_t p) {
    const int k = p.last[blockIdx.x], tid = threadIdx.x;
    if (k < 0 || k >= p.n_crops) return;
    const int8_t *src = p.crops + (size_t)k * p.crop_stride;
    int8_t *dst = p.plane + (size_t)blockIdx.x * p.plane_stride; // (16-byte aligned: the plane's base and pitch are)
    const int n = p.tw * p.th * 3;
    int done = 0;
    if (((uintptr_t)src & 15) == 0) {
        const int n16 = n >> 4;
        for (int i = tid; i < n16; i += SH_THREADS) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
        done = n16 << 4;
    }
    for (int i = done + tid; i < n; i += SH_THREADS) dst[i] = src[i];
}

// ---- launcher
extern "C" int mhip_shots(const mhip_shots_t *p) {
    if (!p || !p->crops || !p->rois || !p->tracks || !p->partials || !p->cand || !p->records || !p->table || !p->hdr || !p->plane || !p->last) return -1;
    if (p->det_cap == 0 ? (!p->confs || !p->cls) : (!p->dets || p->det_cap < 0)) return -1;
    if (p->streams < 1 || p->streams > 65535 || p->steps < 1 || (long long)p->streams * p->steps > 0x7fffffffLL) return -1;
    if (p->slots < 1 || p->slots > TK_SLOTS || p->n_crops < 1 || p->n_crops > 65535) return -1;
    if (p->tw < 1 || p->tw > 1280 || p->th < 1 || p->th > 1280) return -1;
    if (p->band_rows != mhip_shots_band_rows(p->tw) || p->bands != (p->th + p->band_rows - 1) / p->band_rows || p->bands > 65535) return -1;
    if (p->crop_stride < (size_t)p->tw * p->th * 3 || p->plane_stride < (size_t)p->tw * p->th * 3 || (p->plane_stride & 15) || ((uintptr_t)p->plane & 15)) return -1;
    if (p->max_gap < 1 || p->min_hits < 1) return -1;
    const int rows = p->band_rows + 2, spans = p->nhwc ? 1 : 3;
    const size_t len = (size_t)rows * p->tw * (p->nhwc ? 3 : 1);
    const size_t lds = spans * (((len + 15) & ~(size_t)15) + 32) + (size_t)rows * p->tw;
    if (lds > MHIP_SHOTS_LDS + 256) return -1;
    hipStream_t st = mhip_stream_native();
    const dim3 grid((unsigned)p->n_crops, (unsigned)p->bands);
    if (p->nhwc) hipLaunchKernelGGL(shot_metrics_kernel<true>, grid, dim3(SH_THREADS), lds, st, *p);
    else hipLaunchKernelGGL(shot_metrics_kernel<false>, grid, dim3(SH_THREADS), lds, st, *p);
    if (mhip_check(hipGetLastError(), "shot_metrics")) return -1;
    hipLaunchKernelGGL(shot_walk_kernel, dim3((unsigned)p->streams), dim3(TK_THREADS), 0, st, *p);
    if (mhip_check(hipGetLastError(), "shot_walk")) return -1;
    hipLaunchKernelGGL(shot_copy_kernel, dim3((unsigned)(p->streams * p->slots)), dim3(SH_THREADS), 0, st, *p);
    return mhip_check(hipGetLastError(), "shot_copy");
}
