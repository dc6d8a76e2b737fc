// tile.hip -- tiled inference on gfx950: the tile table -> the ROI table the crop kernel of roi.hip reads, and T per-tile detection lists ->
// one list per camera frame in camera pixels.
//
// include/mars_hip.h ("Tiled inference") states the arithmetic.  The reference has no batch and no such step; nothing here restates it.
//   tile_rois_kernel   slot c * T + t of the ROI table = tile t's rectangle in camera frame c.  The front-end is then roi_crop_kernel itself:
//                      the bytes of a tile are the bytes of a crop of that rectangle, by construction.
//   tile_merge_kernel  one workgroup per camera frame, sort_nms_kernel (yolo_tail.hip) in shape:
//                      gather  the first `quota` entries of every tile's list, validity, map and edge rule applied, into LDS by an ordered
//                              block-wide count (wave ballots + a scan over the waves), so that slot k is candidate k of the header's numbering;
//                      sort    bitonic over a 64-bit key (confidence in its order-preserving integer form, 2047 - k): confidence descending,
//                              k ascending, a strict total order -- no tie replay as in the tail, the exchange-sort permutation is not part of
//                              this contract;
//                      pairs   "different tiles, same class (or agnostic), m > t" 64 rows at a time inside class buckets into a 64 x 2048 bit
//                              matrix; wave 0 walks the rows greedily (a removed candidate removes nothing), 32 lanes holding the removed set;
//                      output  survivors compacted in sorted order, the first 1000 written, the slots behind them zeroed, the counters.
// LDS: 2048 x {x, y, w, h, conf, class: 24 bytes, list index: 2, tile: 1, sorted slot -> k: 2, bucket list: 2} = 62 KB, the bit matrix (the
// sort's keys before it is needed) 16 KB, bucket and scan words 1.5 KB: 81464 bytes, under 80 KB so that two workgroups share a CU and the
// kernel leaves room for the next batch's convolution workgroups (the comment above sort_nms_kernel records what a 148 KB tail did).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

struct tile_det_t { float x, y, w, h, conf; int cls; };   // mars_det_t
struct tile_src_t { int tile, det; };                     // mars_tile_src_t
struct tile_roi_t { int frame, det, x0, y0, x1, y1; };    // mars_roi_t
struct tile_stats_t { int candidates, overflow, invalid, edge, suppressed, truncated; }; // mars_tile_stats_t

#define TM_THREADS 512
#define TM_WAVES (TM_THREADS / 64)
#define TM_CAND MHIP_TILE_MAX_CAND
#define TM_CHUNK 64
#define TM_SUBS (TM_THREADS / TM_CHUNK) // threads that share a row's bucket
#define TM_BUCKETS 128
#define TM_MAXD 1000
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
    tile_roi_t r;
    r.frame = c; r.det = t;
    r.x0 = p.tiles[t].x0; r.y0 = p.tiles[t].y0; r.x1 = p.tiles[t].x1; r.y1 = p.tiles[t].y1;
    ((tile_roi_t *)p.rois)[i] = r;
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

    const int cam = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = p.n_tiles;
    const tile_det_t *lists = (const tile_det_t *)p.dets + (size_t)cam * T * p.max_det;
    tile_det_t *out = (tile_det_t *)p.out + (size_t)cam * TM_MAXD;
    tile_src_t *org = (tile_src_t *)p.origins + (size_t)cam * TM_MAXD;

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
            const tile_det_t d = lists[(size_t)t * p.max_det + i];
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
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = n;
        for (int w = 0; w < wv; w++) off += wave_cnt[w];
        const int k = off + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) { // k < TM_CAND: at most M entries are kept
            bx[k] = X; by[k] = Y; bw[k] = Wd; bh[k] = Hd; bconf[k] = conf; bc[k] = cls;
            bdet[k] = (unsigned short)i; btile[k] = (unsigned char)t;
        }
        for (int w = 0; w < TM_WAVES; w++) n += wave_cnt[w];
        __syncthreads();
    }
    if (n == 0) { // uniform
        const tile_det_t zd = {0, 0, 0, 0, 0, 0};
        const tile_src_t zs = {0, 0};
        for (int j = tid; j < TM_MAXD; j += TM_THREADS) { out[j] = zd; org[j] = zs; }
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
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += TM_THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const unsigned long long a = keys[lo], b = keys[hi];
                    const bool desc = (lo & k) == 0;
                    if (desc ? a < b : a > b) { keys[lo] = b; keys[hi] = a; }
                }
                __syncthreads();
            }
        for (int r = tid; r < n; r += TM_THREADS) perm[r] = (unsigned short)(TM_CAND - 1 - (int)(keys[r] & (TM_CAND - 1)));
    }
    if (tid < TM_BUCKETS) bfill[tid] = 0;
    __syncthreads();
    // ---- class buckets over the sorted slots (class & 127, the exact class is still compared); one bucket when every pair counts
    for (int j = tid; j < n; j += TM_THREADS) atomicAdd(&bfill[p.agnostic ? 0 : (unsigned)bc[perm[j]] & (TM_BUCKETS - 1)], 1);
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int b = 0; b < TM_BUCKETS; b++) { bstart[b] = acc; acc += bfill[b]; bfill[b] = 0; }
        bstart[TM_BUCKETS] = acc;
    }
    __syncthreads();
    for (int j = tid; j < n; j += TM_THREADS) {
        const int b = p.agnostic ? 0 : (unsigned)bc[perm[j]] & (TM_BUCKETS - 1);
        blist[bstart[b] + atomicAdd(&bfill[b], 1)] = (unsigned short)j;
    }
    __syncthreads();
    const int nw = (n + 63) >> 6;
    unsigned long long removed = 0; // wave 0: lane w (< 32) holds word w of the removed set
    for (int i0 = 0; i0 < n; i0 += TM_CHUNK) {
        const int rows = n - i0 < TM_CHUNK ? n - i0 : TM_CHUNK;
        for (int k = tid; k < TM_CHUNK * TM_WORDS; k += TM_THREADS) mask[k] = 0;
        __syncthreads();
        {
            const int r = tid / TM_SUBS, sub = tid % TM_SUBS, i = i0 + r;
            if (r < rows) {
                const int a = perm[i];
                const float xi = bx[a], yi = by[a], wi = bw[a], hi = bh[a];
                const int ci = bc[a], ti = btile[a];
                const float ax1 = xi - wi / 2, ay1 = yi - hi / 2, ax2 = xi + wi / 2, ay2 = yi + hi / 2;
                const float aarea = wi * hi;
                const int b = p.agnostic ? 0 : (unsigned)ci & (TM_BUCKETS - 1);
                for (int e = bstart[b] + sub; e < bstart[b + 1]; e += TM_SUBS) {
                    const int j = blist[e];
                    if (j <= i) continue;
                    const int q = perm[j];
                    if (btile[q] == ti || (!p.agnostic && bc[q] != ci)) continue;
                    const float xj = bx[q], yj = by[q], wj = bw[q], hj = bh[q];
                    float x1 = fmaxf(ax1, xj - wj / 2);
                    float y1 = fmaxf(ay1, yj - hj / 2);
                    float x2 = fminf(ax2, xj + wj / 2);
                    float y2 = fminf(ay2, yj + hj / 2);
                    float iw = fmaxf(0.0f, x2 - x1), ih = fmaxf(0.0f, y2 - y1);
                    float inter = iw * ih;
                    float barea = wj * hj;
                    float den;
                    if (p.ios) den = fminf(aarea, barea);
                    else {
                        den = aarea + barea;
                        den = den - inter;
                    }
                    den = den + 1e-6f;
                    if (inter / den > p.thresh) atomicOr(&mask[r * TM_WORDS + (j >> 5)], 1u << (j & 31));
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            // the greedy walk: a dependent chain of `rows` steps whose matrix rows do not depend on it, so they are fetched 16 at a time ahead of
            // the steps that use them, and a removed row is skipped by a select, not a branch (sort_nms_kernel's walk, 32 words wide)
            const int wl = tid < 32 ? tid : 31, c = i0 >> 6; // rows i0.. live in word c of the removed set
            for (int r0 = 0; r0 < rows; r0 += 16) {
                unsigned long long mrow[16];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int r = r0 + k < TM_CHUNK ? r0 + k : TM_CHUNK - 1;
                    mrow[k] = *(const unsigned long long *)&mask[r * TM_WORDS + 2 * wl];
                }
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int r = r0 + k;
                    const unsigned half = r < 32 ? __builtin_amdgcn_readlane((unsigned)removed, c) : __builtin_amdgcn_readlane((unsigned)(removed >> 32), c);
                    const bool dead = (half >> (r & 31)) & 1u; // a removed candidate removes nothing
                    removed |= (dead || tid >= nw || r >= rows) ? 0ull : mrow[k];
                }
            }
        }
        __syncthreads(); // the next chunk overwrites the bit matrix
    }
    if (tid < 32) removed_s[tid] = tid < nw ? removed : ~0ull;
    __syncthreads();
    // ---- the survivors in sorted order, the first 1000 of them
    int total = 0;
    for (int base = 0; base < n; base += TM_THREADS) {
        const int idx = base + tid;
        const bool keep = idx < n && !((removed_s[idx >> 6] >> (idx & 63)) & 1ull);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wv; w++) off += wave_cnt[w];
        const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && slot < TM_MAXD) {
            const int a = perm[idx];
            tile_det_t d;
            d.x = bx[a]; d.y = by[a]; d.w = bw[a]; d.h = bh[a]; d.conf = bconf[a]; d.cls = bc[a];
            out[slot] = d;
            tile_src_t o;
            o.tile = btile[a]; o.det = bdet[a];
            org[slot] = o;
        }
        for (int w = 0; w < TM_WAVES; w++) total += wave_cnt[w];
        __syncthreads();
    }
    const int kept = min(total, TM_MAXD);
    {
        const tile_det_t zd = {0, 0, 0, 0, 0, 0};
        const tile_src_t zs = {0, 0};
        for (int j = kept + tid; j < TM_MAXD; j += TM_THREADS) { out[j] = zd; org[j] = zs; }
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
    if (p->max_det < 1 || p->max_det > TM_MAXD || p->quota < 1 || (long long)p->n_tiles * p->quota > TM_CAND) return -1;
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
