// tile.hip -- tiled inference on gfx950: the tile table -> the ROI table the crop kernel of roi.hip reads, and T per-tile detection lists ->
// one list per camera frame in camera pixels.
//
// include/mars_hip.h ("Tiled inference") states the arithmetic.  The reference has no batch and no such step; nothing here restates it.
//   tile_rois_kernel   slot c * T + t of the ROI table = tile t's rectangle in camera frame c.  The front-end is then roi_crop_kernel itself:
//                      the bytes of a tile are the bytes of a crop of that rectangle, by construction.
//   tile_merge_kernel  one workgroup per camera frame, sort_nms_kernel (yolo_tail.hip) in shape; sort, buckets, walk and compaction are
//                      tail_core.hpp's:
//                      gather  the first `quota` entries of every tile's list, validity, map and edge rule applied, into LDS by an ordered
//                              block-wide count (block_rank), so that slot k is candidate k of the header's numbering;
//                      sort    bitonic over a 64-bit key (confidence in its order-preserving integer form, 2047 - k): confidence descending,
//                              k ascending, a strict total order -- no tie replay as in the tail, the exchange-sort permutation is not part of
//                              this contract;
//                      pairs   "different tiles, same class (or agnostic), m > t" inside class buckets into a 64 x 2048 bit matrix
//                              (greedy_suppress<32>: 32 lanes hold the removed set);
//                      output  survivors compacted in sorted order, the first 1000 written, the slots behind them zeroed, the counters.
// LDS: 2048 x {x, y, w, h, conf, class: 24 bytes, list index: 2, tile: 1, sorted slot -> k: 2, bucket list: 2} = 62 KB, the bit matrix (the
// sort's keys before it is needed) 16 KB, bucket and scan words 1.5 KB: 81464 bytes, under 80 KB so that two workgroups share a CU and the
// kernel leaves room for the next batch's convolution workgroups (the comment above sort_nms_kernel records what a 148 KB tail did).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define TM_THREADS NMS_THREADS
#define TM_WAVES NMS_WAVES
#define TM_CAND MHIP_TILE_MAX_CAND
#define TM_CHUNK NMS_CHUNK
#define TM_BUCKETS NMS_BUCKETS
#define TM_WORDS (TM_CAND / 32)         // 32-bit words of a matrix row

// byte offsets of the kernel's LDS arrays
#define TM_OFF_X 0
#define TM_OFF_Y (TM_OFF_X + TM_CAND * 4)
#define TM_OFF_W (TM_OFF_Y + TM_CAND * 4)
#define TM_OFF_H (TM_OFF_W + TM_CAND * 4)
#define TM_OFF_CONF (TM_OFF_H + TM_CAND * 4)
#define TM_OFF_CLS (TM_OFF_CONF + TM_CAND * 4)
#define TM_OFF_MASK (TM_OFF_CLS + TM_CAND * 4)                    // 64 rows x 2048 bits; the sort's 2048 keys of 8 bytes
#define TM_OFF_REMOVED (TM_OFF_MASK + TM_CHUNK * TM_WORDS * 4)    // 32 x 8 bytes
#define TM_OFF_DET (TM_OFF_REMOVED + 32 * 8)
#define TM_OFF_PERM (TM_OFF_DET + TM_CAND * 2)
#define TM_OFF_BLIST (TM_OFF_PERM + TM_CAND * 2)
#define TM_OFF_TILE (TM_OFF_BLIST + TM_CAND * 2)
#define TM_OFF_BSTART (TM_OFF_TILE + TM_CAND)                     // 129 ints
#define TM_OFF_BFILL (TM_OFF_BSTART + (TM_BUCKETS + 1) * 4)
#define TM_OFF_TSTART (TM_OFF_BFILL + TM_BUCKETS * 4)             // 65 ints: first gather slot of every tile
#define TM_OFF_WAVE (TM_OFF_TSTART + (MHIP_TILE_MAX_TILES + 1) * 4)
#define TM_OFF_STAT (TM_OFF_WAVE + TM_WAVES * 4)                  // overflow, invalid, edge, -
#define TM_LDS (TM_OFF_STAT + 4 * 4)
static_assert(TM_LDS <= 80 * 1024, "two workgroups of the merge share a CU's 160 KB");
static_assert(TM_OFF_REMOVED % 8 == 0 && TM_OFF_MASK % 16 == 0 && TM_OFF_BSTART % 4 == 0, "alignment of the 8-byte and 4-byte arrays");

// finite floats -> unsigned integers in the same order (-0 below +0)
__device__ __forceinline__ unsigned tile_ord(const float c) {
    const unsigned u = __float_as_uint(c);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void tile_rois_kernel(const mhip_tile_t p) {
    const int i = blockIdx.x * 256 + threadIdx.x, slots = p.cams * p.n_tiles;
    if (i == 0) {
        p.n_out[0] = slots;
        p.n_out[1] = 0;
    }
    if (i >= slots) return;
    const int c = i / p.n_tiles, t = i - c * p.n_tiles;
    roi_t r;
    r.frame = c; r.det = t;
    r.x0 = p.tiles[t].x0; r.y0 = p.tiles[t].y0; r.x1 = p.tiles[t].x1; r.y1 = p.tiles[t].y1;
    ((roi_t *)p.rois)[i] = r;
}

__global__ __launch_bounds__(TM_THREADS) void tile_merge_kernel(const mhip_tile_t p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    float *bx = (float *)(sm + TM_OFF_X), *by = (float *)(sm + TM_OFF_Y), *bw = (float *)(sm + TM_OFF_W), *bh = (float *)(sm + TM_OFF_H);
    float *bconf = (float *)(sm + TM_OFF_CONF);
    int *bc = (int *)(sm + TM_OFF_CLS);
    unsigned int *mask = (unsigned int *)(sm + TM_OFF_MASK);             // [TM_CHUNK][TM_WORDS]
    unsigned long long *keys = (unsigned long long *)(sm + TM_OFF_MASK); // the sort's, before the matrix is needed
    unsigned long long *removed_s = (unsigned long long *)(sm + TM_OFF_REMOVED);
    unsigned short *bdet = (unsigned short *)(sm + TM_OFF_DET), *perm = (unsigned short *)(sm + TM_OFF_PERM), *blist = (unsigned short *)(sm + TM_OFF_BLIST);
    unsigned char *btile = sm + TM_OFF_TILE;
    int *bstart = (int *)(sm + TM_OFF_BSTART), *bfill = (int *)(sm + TM_OFF_BFILL), *tstart = (int *)(sm + TM_OFF_TSTART);
    int *wave_cnt = (int *)(sm + TM_OFF_WAVE), *stat = (int *)(sm + TM_OFF_STAT);

    const int cam = blockIdx.x, tid = threadIdx.x;
    const int T = p.n_tiles;
    const det_t *lists = (const det_t *)p.dets + (size_t)cam * T * p.max_det;
    det_t *out = (det_t *)p.out + (size_t)cam * MAXD;
    tile_src_t *org = (tile_src_t *)p.origins + (size_t)cam * MAXD;

    // ---- quota: the gather slots [tstart[t], tstart[t + 1]) are the first entries of tile t's list
    if (tid == 0) {
        int acc = 0, over = 0;
        for (int t = 0; t < T; t++) {
            const int n = min(max(p.counts[cam * T + t], 0), p.max_det), q = min(n, p.quota);
            tstart[t] = acc;
            acc += q;
            over += n - q;
        }
        tstart[T] = acc;
        stat[0] = over; stat[1] = 0; stat[2] = 0; stat[3] = 0;
    }
    __syncthreads();
    // ---- gather: thread order = (tile, list index) order, so the ordered count numbers the candidates as the header does
    const int M = tstart[T]; // <= T * quota <= TM_CAND
    int n = 0;
    for (int base = 0; base < M; base += TM_THREADS) {
        const int s = base + tid;
        bool keep = false;
        float X = 0, Y = 0, Wd = 0, Hd = 0, conf = 0;
        int cls = 0, t = 0, i = 0;
        if (s < M) {
            while (tstart[t + 1] <= s) t++; // (empty tiles are stepped over; t < T because s < tstart[T])
            i = s - tstart[t];
            const det_t d = lists[(size_t)t * p.max_det + i];
            const mhip_tile_geom_t g = p.tiles[t];
            if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.w) && isfinite(d.h) && isfinite(d.conf)) || !(d.w > 0.0f) || !(d.h > 0.0f)) {
                atomicAdd(&stat[1], 1);
            } else {
                X = (d.x - g.px) * g.rx + (float)g.x0;
                Y = (d.y - g.py) * g.ry + (float)g.y0;
                Wd = d.w * g.rx;
                Hd = d.h * g.ry;
                conf = d.conf; cls = d.cls;
                keep = true;
                if (p.edge_margin > 0.0f) {
                    const float l = X - Wd * 0.5f, r = X + Wd * 0.5f, tp = Y - Hd * 0.5f, bt = Y + Hd * 0.5f;
                    const bool cut = (g.x0 > 0 && l - (float)g.x0 < p.edge_margin) || (g.x1 < p.src_w && (float)g.x1 - r < p.edge_margin) ||
                                     (g.y0 > 0 && tp - (float)g.y0 < p.edge_margin) || (g.y1 < p.src_h && (float)g.y1 - bt < p.edge_margin);
                    if (cut) {
                        atomicAdd(&stat[2], 1);
                        keep = false;
                    }
                }
            }
        }
        int step;
        const int k = n + block_rank<TM_WAVES>(keep, wave_cnt, step);
        if (keep) { // k < TM_CAND: at most M entries are kept
            bx[k] = X; by[k] = Y; bw[k] = Wd; bh[k] = Hd; bconf[k] = conf; bc[k] = cls;
            bdet[k] = (unsigned short)i; btile[k] = (unsigned char)t;
        }
        n += step;
        __syncthreads(); // wave_cnt is rewritten by the next step
    }
    if (n == 0) { // uniform
        const det_t zd = {0, 0, 0, 0, 0, 0};
        const tile_src_t zs = {0, 0};
        for (int j = tid; j < MAXD; j += TM_THREADS) { out[j] = zd; org[j] = zs; }
        if (tid == 0) {
            const tile_stats_t st = {0, stat[0], stat[1], stat[2], 0, 0};
            ((tile_stats_t *)p.stats)[cam] = st;
            p.out_counts[cam] = 0;
        }
        return;
    }
    // ---- sort: confidence descending, then k ascending.  Padding keys are 0, below every real key (tile_ord of a finite float is >= 0x00800000)
    {
        int P = 2;
        while (P < n) P <<= 1;
        for (int r = tid; r < P; r += TM_THREADS)
            keys[r] = r < n ? ((unsigned long long)tile_ord(bconf[r]) << 11) | (unsigned)(TM_CAND - 1 - r) : 0ull;
        __syncthreads();
        bitonic_sort_desc(keys, P);
        for (int r = tid; r < n; r += TM_THREADS) perm[r] = (unsigned short)(TM_CAND - 1 - (int)(keys[r] & (TM_CAND - 1)));
    }
    if (tid < TM_BUCKETS) bfill[tid] = 0;
    __syncthreads();
    // ---- class buckets over the sorted slots (the exact class is still compared); one bucket when every pair counts
    const auto bucket_of = [&](const int j) { return p.agnostic ? 0 : class_bucket(bc[perm[j]]); };
    class_buckets(n, bstart, bfill, blist, bucket_of);
    // ---- pairs: different tiles, same class (or agnostic), IoU or IoS above the threshold
    struct row_t { box_edges_t box; int cls, tile; };
    greedy_suppress<TM_CAND / 64>(
        n, mask, bstart, blist, removed_s, bucket_of,
        [&](const int i) {
            const int a = perm[i];
            return row_t{box_edges(bx[a], by[a], bw[a], bh[a]), bc[a], btile[a]};
        },
        [&](const row_t &a, const int j) {
            const int q = perm[j];
            if (btile[q] == a.tile || (!p.agnostic && bc[q] != a.cls)) return false;
            float inter, barea, den;
            box_iou_terms(a.box, bx[q], by[q], bw[q], bh[q], inter, barea);
            if (p.ios) den = fminf(a.box.area, barea);
            else {
                den = a.box.area + barea;
                den = den - inter;
            }
            den = den + 1e-6f;
            return inter / den > p.thresh;
        });
    // ---- the survivors in sorted order, the first 1000 of them (the count goes on: the stats need it)
    const int total = compact_survivors(n, removed_s, wave_cnt, [&](const int idx, const int slot) {
        if (slot >= MAXD) return;
        const int a = perm[idx];
        det_t d;
        d.x = bx[a]; d.y = by[a]; d.w = bw[a]; d.h = bh[a]; d.conf = bconf[a]; d.cls = bc[a];
        out[slot] = d;
        tile_src_t o;
        o.tile = btile[a]; o.det = bdet[a];
        org[slot] = o;
    });
    const int kept = min(total, MAXD);
    {
        const det_t zd = {0, 0, 0, 0, 0, 0};
        const tile_src_t zs = {0, 0};
        for (int j = kept + tid; j < MAXD; j += TM_THREADS) { out[j] = zd; org[j] = zs; }
    }
    if (tid == 0) {
        const tile_stats_t st = {n, stat[0], stat[1], stat[2], n - total, total - kept};
        ((tile_stats_t *)p.stats)[cam] = st;
        p.out_counts[cam] = kept;
    }
}

static bool tile_table_ok(const mhip_tile_t *p) {
    if (!p || p->n_tiles < 1 || p->n_tiles > MHIP_TILE_MAX_TILES || p->cams < 1 || p->src_w <= 0 || p->src_h <= 0) return false;
    for (int t = 0; t < p->n_tiles; t++) {
        const mhip_tile_geom_t *g = &p->tiles[t];
        if (g->x0 < 0 || g->y0 < 0 || g->x1 <= g->x0 || g->y1 <= g->y0 || g->x1 > p->src_w || g->y1 > p->src_h) return false;
    }
    return true;
}

extern "C" int mhip_tile_rois(const mhip_tile_t *p) {
    if (!tile_table_ok(p) || !p->rois || !p->n_out || (long long)p->cams * p->n_tiles > 65535) return -1;
    hipLaunchKernelGGL(tile_rois_kernel, dim3((unsigned)((p->cams * p->n_tiles + 255) / 256)), dim3(256), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "tile rois");
}

extern "C" int mhip_tile_merge(const mhip_tile_t *p) {
    if (!tile_table_ok(p) || !p->dets || !p->counts || !p->out || !p->out_counts || !p->origins || !p->stats) return -1;
    if (p->max_det < 1 || p->max_det > MAXD || p->quota < 1 || (long long)p->n_tiles * p->quota > TM_CAND) return -1;
    if (!(p->thresh >= 0.0f) || !(p->edge_margin >= 0.0f)) return -1;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void *)tile_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TM_LDS) != hipSuccess)
            return mhip_check(hipErrorUnknown, "tile merge attribute");
        attr = true;
    }
    hipLaunchKernelGGL(tile_merge_kernel, dim3((unsigned)p->cams), dim3(TM_THREADS), TM_LDS, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "tile merge");
}
