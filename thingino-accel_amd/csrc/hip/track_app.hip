// track_app.hip -- tracking with an appearance term on gfx950: the walk of track.hip on a tracker whose slots hold an int8 embedding each,
// the cosines of slots against candidates on v_mfma_i32_16x16x64_i8, and the embedding plane's update.
//
// include/mars_hip.h ("Appearance in tracking") states the arithmetic.  The records, the LDS table, the scans, the candidates' compaction
// and the rounds are track_core.hpp's, one source for this file and track.hip; the per-step body is this kernel's own, track.hip's with
// the plane's steps worked in (track_core.hpp says why the body is not shared).  What the plane adds, per stream and step:
//   candidates   the high set's compaction also notes each candidate's embedding row (emb_index -> q, qq), or none;
//   cosines      between the compaction and pass 1 the eight wavefronts compute slots x candidates: a wavefront takes two of the sixteen
//                16-slot tiles as the MFMA's A operand and walks the candidates' 16-tiles four at a time as B operands (gallery.hip's operand
//                maps: lane l holds bytes 16 * (l >> 4) .. + 15 of row l & 15 of a 64-channel step; result register e of lane l is A-row
//                4 * (l >> 4) + e against B-row l & 15), K over cp / 64.  The epilogue turns the int32 dots into cosines and writes them
//                TWICE into an HBM scratch of 512 KB per workgroup: slot-major for the candidate half of the workgroup (thread c reads
//                [t][c]: a wavefront reads 64 consecutive floats) and candidate-major for the slot half.  256 x 256 floats do not fit the
//                LDS; the scratch is written and read by one workgroup between two of its barriers and stays in L2.  A step in which no
//                live slot or no candidate has an embedding skips the products and runs pass 1 on the IoU alone;
//   association  pass 1 reads cos where both sides have an embedding and recomputes the IoU as before; a pair's key depends on the pair
//                alone, so the mutual-best-pick rounds stay a valid evaluation of the greedy order.  Pass 2 is the plain one;
//   embeddings   the update and the births leave one action per slot (take row r, blend with row r, clear, nothing); a wavefront per slot
//                row then writes the plane in HBM, the 3:1 blend re-quantised by the gallery's rule (tail_core.hpp's quantise_row, which
//                gallery.hip's and this file's quantise launches call too).
// The streams of a call run in chunks of MHIP_TRACK_APP_CHUNK over one scratch block, so the scratch is bounded by 256 MB whatever the
// number of streams.  LDS: about 28 KB (the plain table's 25 KB + four int arrays of 256).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "track_core.hpp"

#pragma clang fp contract(off)

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

static_assert(TK_SLOTS == 256 && TK_CAND == 256 && TK_WAVES == 8, "the tile walk below: sixteen 16-slot tiles over eight wavefronts");

// detection i of a frame -> its row of q, or -1: no index array, an index outside the rows, a null vector
__device__ __forceinline__ int ta_row_of(const mhip_track_app_t &p, const int *idx, const int i, int &qq) {
    qq = 0;
    if (!idx) return -1;
    const int r = idx[i];
    if (r < 0 || r >= p.n_vec) return -1;
    qq = p.qq[r];
    return qq > 0 ? r : -1;
}

// The cosines of the TK_SLOTS rows of `plane` (ee[t] == 0: none) against candidates 0 .. nc - 1 (crow[c] < 0: none): sm[t][c] and cm[c][t],
// pitch 256, for every t and every c below nc rounded up to 16; 0.0f where a side has no embedding.  Every thread of the workgroup calls
// it; no barrier inside: the caller has made ee, crow and cqq (LDS) and the rows (HBM) visible, and puts a barrier before the readers.
__device__ void ta_matrix(const int8_t *plane, const int *ee, const int8_t *q, const int *crow, const int *cqq, const int nc, const int cp,
                          float *sm, float *cm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, frow = lane & 15, fchunk = lane >> 4;
    const int ntile = (nc + 15) >> 4, ksteps = cp >> 6;
    for (int tt = w; tt < TK_SLOTS / 16; tt += TK_WAVES) {
        const int t0 = tt * 16, tb = t0 + 4 * fchunk; // this lane's four slots: tb .. tb + 3
        float einv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int v = ee[tb + e];
            einv[e] = v > 0 ? 1.0f / sqrtf((float)v) : 0.0f;
        }
        const bool any_t = __ballot(ee[t0 + frow] > 0) != 0ull; // (the same in every lane)
        const int8_t *ap = plane + (size_t)(t0 + frow) * cp + fchunk * 16;
        for (int g = 0; g < ntile; g += 4) {
            const int8_t *bp[4];
            float qinv[4];
            bool have = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int c = (g + u) * 16 + frow;
                const int row = c < nc ? crow[c] : -1;
                const int v = row >= 0 ? cqq[c] : 0;
                bp[u] = row >= 0 ? q + (size_t)row * cp + fchunk * 16 : nullptr;
                qinv[u] = v > 0 ? 1.0f / sqrtf((float)v) : 0.0f;
                have = have || row >= 0;
            }
            v4i acc[4];
#pragma unroll
            for (int u = 0; u < 4; u++) acc[u] = (v4i){0, 0, 0, 0};
            if (any_t && __ballot(have) != 0ull) {
                for (int ks = 0; ks < ksteps; ks++) {
                    const v4i a = *(const v4i *)(ap + ks * 64);
                    v4i b[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) b[u] = bp[u] ? *(const v4i *)(bp[u] + ks * 64) : (v4i){0, 0, 0, 0};
#pragma unroll
                    for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[u], acc[u], 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (g + u >= ntile) continue;
                const int c = (g + u) * 16 + frow; // < 256
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float k = (float)acc[u][e] * einv[e]; // two roundings, then a third: no contraction in this file
                    v[e] = (einv[e] != 0.0f && qinv[u] != 0.0f) ? k * qinv[u] : 0.0f;
                    sm[(size_t)(tb + e) * TK_CAND + c] = v[e];
                }
                *(float4 *)(cm + (size_t)c * TK_SLOTS + tb) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

// One slot's row of the plane by its action, a wavefront per row; -> the row's new ee (the same in every lane)
__device__ int ta_row_update(int8_t *row, const int ee, const int8_t *src, const int src_qq, const bool clear, const bool blend, const int cp) {
    const int lane = threadIdx.x & 63;
    if (clear) {
        for (int c = lane; c < cp; c += 64) row[c] = 0;
        return 0;
    }
    if (!blend || ee <= 0) {
        for (int c = lane; c < cp; c += 64) row[c] = src[c]; // (the pad channels of q are zero)
        return src_qq;
    }
    // v = 3 e + q over all cp channels (the pads of both rows are zero, and stay so); a lane's own bytes, read before it writes them
    return quantise_row(row, cp, cp, [row, src](const int c) { return 3 * (int)row[c] + (int)src[c]; });
}

// grid: the streams of one chunk; b0: the first of them
__global__ __launch_bounds__(TK_THREADS) void track_app_kernel(const mhip_track_app_t pa, const int b0) {
    __shared__ tk_lds_t<true> s;
    const mhip_track_t &p = pa.t;
    const int tid = threadIdx.x, b = b0 + blockIdx.x;
    tk_state_t *table = (tk_state_t *)p.states + (size_t)b * TK_SLOTS;
    int8_t *plane = pa.plane + (size_t)b * TK_SLOTS * pa.cp;
    int *plane_ee = pa.plane_ee + (size_t)b * TK_SLOTS;
    float *sm = pa.cosm ? pa.cosm + (size_t)blockIdx.x * MHIP_TRACK_APP_COS_FLOATS : nullptr, *cm = sm ? sm + TK_SLOTS * TK_CAND : nullptr;
    const bool with_vectors = pa.emb_index && pa.n_vec > 0 && sm;
    if (tid < TK_SLOTS) {
        const tk_state_t v = table[tid];
        s.id[tid] = v.id; s.cls[tid] = v.cls; s.hits[tid] = v.hits; s.miss[tid] = v.miss;
        s.x[tid] = v.x; s.y[tid] = v.y; s.w[tid] = v.w; s.h[tid] = v.h; s.vx[tid] = v.vx; s.vy[tid] = v.vy;
        s.icls[tid] = v.ident.cls; s.iscore[tid] = v.ident.score;
        s.ee[tid] = plane_ee[tid];
    }
    if (tid < 4) s.counters[tid] = p.hdr[b].counters[tid];
    if (tid == 0) s.next_id = p.hdr[b].next_id;
    __syncthreads();
    for (int t = 0; t < p.steps; t++) {
        const size_t f = p.stream_major ? (size_t)b * p.steps + t : (size_t)t * p.streams + b;
        const det_t *d = (const det_t *)p.dets + f * p.max_det;
        const cls_t *idn = p.idents ? (const cls_t *)p.idents + f * p.max_det : nullptr;
        const int *idx = with_vectors ? pa.emb_index + f * p.max_det : nullptr;
        tk_out_t *o = (tk_out_t *)p.out + f * p.max_det;
        int n = p.counts[f];
        n = n < 0 ? 0 : n > p.max_det ? p.max_det : n;
        for (int i = tid; i < p.max_det; i += TK_THREADS) o[i] = tk_out_t{-1, 0};
        const bool live = tid < TK_SLOTS && s.hits[tid] > 0;
        if (tid < TK_SLOTS) {
            s.px[tid] = s.x[tid] + s.vx[tid];
            s.py[tid] = s.y[tid] + s.vy[tid];
            s.det[tid] = -1;
            s.take[tid] = TK_TAKE_NONE;
            s.blend[tid] = 0;
            s.tfree[tid] = live;
        }
        // pass 1: every live track against H, with the cosines where both sides of some pair have an embedding
        const int nh = tk_candidates<true>(s, pa, d, idx, n, false);
        const int some_c = __syncthreads_or(tid < nh && s.cqq[tid < TK_CAND ? tid : 0] > 0);
        const int some_t = __syncthreads_or(live && s.ee[tid < TK_SLOTS ? tid : 0] > 0);
        if (idx && some_c && some_t) {
            ta_matrix(plane, s.ee, pa.q, s.crow, s.cqq, nh, pa.cp, sm, cm);
            __syncthreads(); // the matrix in HBM, written and read by this workgroup alone
            tk_associate<true>(s, nh, p.iou, p.any_class != 0, pa.app_thresh, pa.app_min_iou, sm, cm);
        } else {
            tk_associate<false>(s, nh, p.iou, p.any_class != 0, 0.0f, 0.0f, nullptr, nullptr);
        }
        if (tid < TK_CAND) {
            s.hidx[tid] = s.cidx[tid];
            s.hfree[tid] = tid < nh && s.cslot[tid] < 0;
        }
        __syncthreads();
        // pass 2: the tracks it left against L, on the IoU alone
        if (p.low_conf > 0.0f) {
            if (tid < TK_SLOTS) s.tfree[tid] = live && s.det[tid] < 0;
            const int nl = tk_candidates<true>(s, pa, d, idx, n, true);
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
                int qq;
                const int r = ta_row_of(pa, idx, i, qq);
                if (r >= 0) { s.take[tid] = r; s.blend[tid] = pa.smooth && s.ee[tid] > 0; }
                o[i] = tk_out_t{s.id[tid], s.hits[tid]}; // (behind the {-1, 0} of the loop above: the scans' barriers lie between)
            } else {
                s.x[tid] = s.px[tid]; s.y[tid] = s.py[tid];
                s.miss[tid] += 1;
                if (s.miss[tid] > p.max_miss) { s.hits[tid] = 0; died = true; s.take[tid] = TK_CLEAR; }
            }
        }
        int deaths, nfree, nborn;
        tk_scan(died, s.wsum, deaths);
        // births: free slot r and unmatched H member r meet
        const bool is_free = tid < TK_SLOTS && s.hits[tid] == 0;
        const int r = tk_scan(is_free, s.wsum, nfree);
        if (is_free) s.freelist[r] = (short)tid;
        const bool wants = tid < TK_CAND && s.hfree[tid];
        const int bi = tk_scan(wants, s.wsum, nborn); // (its barriers publish the free list, and the actions of the update)
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
            int qq;
            const int row = ta_row_of(pa, idx, i, qq);
            if (row >= 0) s.take[slot] = row; // the detection's, never the previous occupant's: a slot freed in this step stays at TK_CLEAR
            o[i] = tk_out_t{id, 1};           // otherwise, one free for longer holds zeros already
        }
        __syncthreads();
        if (tid == 0) {
            s.next_id = (int)((unsigned)s.next_id + (unsigned)fits);
            s.counters[0] += fits;
            s.counters[1] += deaths;
            s.counters[3] += nborn - fits;
        }
        // embeddings: a wavefront per slot row
        for (int slot = tid >> 6; slot < TK_SLOTS; slot += TK_WAVES) {
            const int a = s.take[slot]; // (the same in every lane)
            if (a == TK_TAKE_NONE) continue;
            const int ee = ta_row_update(plane + (size_t)slot * pa.cp, s.ee[slot], a >= 0 ? pa.q + (size_t)a * pa.cp : nullptr, a >= 0 ? pa.qq[a] : 0,
                                         a == TK_CLEAR, s.blend[slot] != 0, pa.cp);
            if ((tid & 63) == 0) s.ee[slot] = ee;
        }
        __syncthreads(); // the next step's products read the rows and ee
    }
    if (tid < TK_SLOTS) {
        tk_state_t v;
        v.id = s.id[tid]; v.cls = s.cls[tid]; v.hits = s.hits[tid]; v.miss = s.miss[tid];
        v.x = s.x[tid]; v.y = s.y[tid]; v.w = s.w[tid]; v.h = s.h[tid]; v.vx = s.vx[tid]; v.vy = s.vy[tid];
        v.ident.cls = s.icls[tid]; v.ident.score = s.iscore[tid];
        table[tid] = v;
        plane_ee[tid] = s.ee[tid];
    }
    if (tid < 4) p.hdr[b].counters[tid] = s.counters[tid];
    if (tid == 0) p.hdr[b].next_id = s.next_id;
}

// grid: rows, one wavefront each: gallery.hip's quantise launch without its qinv
__global__ __launch_bounds__(64) void ta_quantise_kernel(const int *vec, const int c, const int cp, int8_t *q, int *qq_out) {
    const int n = blockIdx.x;
    const int *v = vec + (size_t)n * c;
    const int qq = quantise_row(q + (size_t)n * cp, c, cp, [v](const int k) { return v[k]; });
    if (threadIdx.x == 0) qq_out[n] = qq;
}

__global__ __launch_bounds__(256) void ta_index_fill_kernel(int *idx, const size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) idx[i] = -1;
}

__global__ __launch_bounds__(256) void ta_index_scatter_kernel(const roi_t *rois, const int *n_out, const int slots, int *idx, const int det_frames,
                                                               const int det_cap) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= slots || k >= n_out[0]) return;
    const roi_t r = rois[k];
    if (r.frame < 0 || r.frame >= det_frames || r.det < 0 || r.det >= det_cap) return; // (a caller's box: det = -1)
    idx[(size_t)r.frame * det_cap + r.det] = k;
}

// the test hook: one workgroup runs ta_matrix as the tracking kernel does, every candidate j using row j
__global__ __launch_bounds__(TK_THREADS) void ta_matrix_hook_kernel(const int8_t *plane, const int *plane_ee, const int8_t *q, const int *qq, const int nt,
                                                                    const int nc, const int cp, float *cosm, float *out, int *bad) {
    __shared__ int ee[TK_SLOTS], crow[TK_CAND], cqq[TK_CAND];
    const int tid = threadIdx.x;
    if (tid < TK_SLOTS) {
        ee[tid] = plane_ee[tid];
        const int v = tid < nc ? qq[tid] : 0;
        crow[tid] = v > 0 ? tid : -1;
        cqq[tid] = v > 0 ? v : 0;
    }
    __syncthreads();
    float *sm = cosm, *cm = cosm + TK_SLOTS * TK_CAND;
    ta_matrix(plane, ee, q, crow, cqq, nc, cp, sm, cm);
    __syncthreads();
    int differs = 0;
    for (int i = tid; i < nt * nc; i += TK_THREADS) {
        const int t = i / nc, c = i % nc;
        const float v = sm[(size_t)t * TK_CAND + c];
        out[i] = v;
        differs |= __float_as_uint(v) != __float_as_uint(cm[(size_t)c * TK_SLOTS + t]);
    }
    if (differs) *bad = 1;
}

// ---- launchers
static bool ta_rows_ok(const int c, const int cp) { return c >= 1 && c <= MHIP_TRACK_APP_MAX_C && cp == ((c + 63) & ~63); }

extern "C" int mhip_track_app(const mhip_track_app_t *pa) {
    if (!pa || !tk_args_ok(&pa->t) || !pa->plane || !pa->plane_ee) return -1;
    const mhip_track_t *p = &pa->t;
    if (!ta_rows_ok(pa->c, pa->cp) || pa->n_vec < 0) return -1;
    if (pa->n_vec > 0 && (!pa->vec || !pa->q || !pa->qq || !pa->emb_index || !pa->cosm)) return -1;
    if (!(pa->app_thresh > 0.0f) || !(pa->app_thresh <= 1.0f) || !(pa->app_min_iou > 0.0f) || !(pa->app_min_iou <= 1.0f)) return -1;
    hipStream_t st = mhip_stream_native();
    if (pa->n_vec > 0) hipLaunchKernelGGL(ta_quantise_kernel, dim3((unsigned)pa->n_vec), dim3(64), 0, st, pa->vec, pa->c, pa->cp, pa->q, pa->qq);
    for (int b0 = 0; b0 < p->streams; b0 += MHIP_TRACK_APP_CHUNK) { // stream order keeps one chunk's scratch from the next
        const int nb = p->streams - b0 < MHIP_TRACK_APP_CHUNK ? p->streams - b0 : MHIP_TRACK_APP_CHUNK;
        hipLaunchKernelGGL(track_app_kernel, dim3((unsigned)nb), dim3(TK_THREADS), 0, st, *pa, b0);
    }
    return mhip_check(hipGetLastError(), "track with appearance");
}

extern "C" int mhip_track_app_index(const void *rois, const int *n_out, int slots, int *emb_index, int det_frames, int det_cap) {
    if (!rois || !n_out || !emb_index || slots < 1 || det_frames < 1 || det_cap < 1) return -1;
    const size_t n = (size_t)det_frames * det_cap;
    const unsigned fill = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipStream_t st = mhip_stream_native();
    hipLaunchKernelGGL(ta_index_fill_kernel, dim3(fill), dim3(256), 0, st, emb_index, n);
    hipLaunchKernelGGL(ta_index_scatter_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, (const roi_t *)rois, n_out, slots, emb_index,
                       det_frames, det_cap);
    return mhip_check(hipGetLastError(), "track index scatter");
}

extern "C" int mhip_track_app_matrix(const int8_t *plane, const int *plane_ee, const int *vec, int nt, int nc, int c, int cp, int8_t *q, int *qq,
                                     float *cosm, float *out, int *bad) {
    if (!plane || !plane_ee || !vec || !q || !qq || !cosm || !out || !bad) return -1;
    if (nt < 1 || nt > TK_SLOTS || nc < 1 || nc > TK_CAND || !ta_rows_ok(c, cp)) return -1;
    hipStream_t st = mhip_stream_native();
    hipLaunchKernelGGL(ta_quantise_kernel, dim3((unsigned)nc), dim3(64), 0, st, vec, c, cp, q, qq);
    hipLaunchKernelGGL(ta_matrix_hook_kernel, dim3(1), dim3(TK_THREADS), 0, st, plane, plane_ee, (const int8_t *)q, (const int *)qq, nt, nc, cp, cosm, out, bad);
    return mhip_check(hipGetLastError(), "track cosine matrix");
}
