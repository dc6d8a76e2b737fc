// tail_core.hpp -- what the detection-tail kernels share, device-only and inlined: the mirrors of the public records, the ordered
// block-wide rank, and the sort / class buckets / greedy suppression / compaction core of the three NMS kernels (sort_nms_kernel of
// yolo_tail.hip, obb_sort_nms_kernel of obb.hip, tile_merge_kernel of tile.hip), the reference's upright IoU, the box -> source rectangle rule of the
// crops and the redaction (roi.hip, redact.hip), the int8 quantisation of an embedding row (gallery.hip's queries, track_app.hip's vectors and its blend) and the DFL head helpers.
// No kernels and no launchers here.  Every helper that contains a barrier says so; all of those are called by EVERY thread of the
// workgroup under uniform control flow (a kernel's early returns stay ahead of them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------- records
// include/mars_hip.h's records as the kernels read and write them (csrc/mhip.h stays free of the public header)
struct det_t { float x, y, w, h, conf; int cls; };                                        // mars_det_t
struct roi_t { int frame, det, x0, y0, x1, y1; };                                         // mars_roi_t
struct cls_t { int cls; float score; };                                                   // mars_cls_t
struct obb_t { float x, y, w, h, conf; int cls; float angle; int pred; };                 // mars_obb_t
struct tile_src_t { int tile, det; };                                                     // mars_tile_src_t
struct tile_stats_t { int candidates, overflow, invalid, edge, suppressed, truncated; };  // mars_tile_stats_t
struct mask_t { int det, x0, y0, x1, y1, area; };                                         // mars_mask_t
struct pose_t { int det, head, cell; };                                                   // mars_pose_t
struct kpt_t { float x, y, v; };                                                          // mars_kpt_t
static_assert(sizeof(det_t) == 24 && sizeof(roi_t) == 24 && sizeof(cls_t) == 8 && sizeof(obb_t) == 32 && sizeof(tile_src_t) == 8 &&
                  sizeof(tile_stats_t) == 24 && sizeof(mask_t) == 24 && sizeof(pose_t) == 12 && sizeof(kpt_t) == 12,
              "record sizes of include/mars_hip.h");
#define MAXD 1000 // records per frame in every detection list

typedef int v4i __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------ ordered rank
// For each of CELLS flags per thread: rank[k] = the number of set flags in front of (k, this thread) in (k, thread) order; total = the number
// of set flags.  wave_cnt is the caller's int[CELLS][WAVES] in LDS.  Contains ONE barrier, between writing wave_cnt and reading it: what the
// caller wrote before the call is visible after it.  The caller puts a barrier between two calls on the same wave_cnt (the readers of the
// first must be through before the second writes).
template <int WAVES, int CELLS>
__device__ __forceinline__ void block_rank(const bool (&flag)[CELLS], int (*wave_cnt)[WAVES], int (&rank)[CELLS], int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CELLS; k++) {
        const unsigned long long m = __ballot(flag[k]);
        rank[k] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[k][wv] = __popcll(m);
    }
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int k = 0; k < CELLS; k++) {
        rank[k] += t;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const int c = wave_cnt[k][w];
            rank[k] += w < wv ? c : 0;
            t += c;
        }
    }
    total = t;
}
// one flag per thread: -> its rank.  wave_cnt is an int[WAVES]
template <int WAVES>
__device__ __forceinline__ int block_rank(const bool flag, int *wave_cnt, int &total) {
    const bool f[1] = {flag};
    int r[1];
    block_rank<WAVES, 1>(f, (int(*)[WAVES])wave_cnt, r, total);
    return r[0];
}

// ---------------------------------------------------------- upright boxes
// The reference's IoU (mars_yolo_test.c:119-128), operations in its order, unfused (the build passes -ffp-contract=off); `w / 2` is a division.
struct box_edges_t { float x1, y1, x2, y2, area; };
__device__ __forceinline__ box_edges_t box_edges(const float x, const float y, const float w, const float h) {
    box_edges_t a;
    a.x1 = x - w / 2; a.y1 = y - h / 2; a.x2 = x + w / 2; a.y2 = y + h / 2;
    a.area = w * h;
    return a;
}
// the intersection of a with box b and b's area (a's is a.area)
__device__ __forceinline__ void box_iou_terms(const box_edges_t &a, const float bx, const float by, const float bw, const float bh, float &inter,
                                              float &barea) {
    const float x1 = fmaxf(a.x1, bx - bw / 2);
    const float y1 = fmaxf(a.y1, by - bh / 2);
    const float x2 = fminf(a.x2, bx + bw / 2);
    const float y2 = fminf(a.y2, by + bh / 2);
    const float iw = fmaxf(0.0f, x2 - x1), ih = fmaxf(0.0f, y2 - y1);
    inter = iw * ih;
    barea = bw * bh;
}
__device__ __forceinline__ float box_iou(const box_edges_t &a, const float bx, const float by, const float bw, const float bh) {
    float inter, barea;
    box_iou_terms(a, bx, by, bw, bh, inter, barea);
    float uni = a.area + barea;
    uni = uni - inter;
    uni = uni + 1e-6f;
    return inter / uni;
}

// ------------------------------------------------ box -> source rectangle
// "ROI crops" of include/mars_hip.h, shared by the crop selection (roi.hip) and the regions of "Redaction" (redact.hip).
// box -> source rectangle q = {x0, y0, x1, y1}; false = skipped (the rectangle is then all zeros).  float32, every operation rounded on its own
// (-ffp-contract=off).  The two clamps in front of the conversions keep far-away boxes inside the int range and change no decision:
// x0f > W + 1 means x0 > x1 anyway
__device__ __forceinline__ bool roi_rect(const det_t d, const float expand, const int min_size, const int W, const int H, int q[4]) {
    q[0] = q[1] = q[2] = q[3] = 0;
    if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.w) && isfinite(d.h) && isfinite(d.conf))) return false;
    if (!(d.w > 0.0f) || !(d.h > 0.0f)) return false;
    const float hw = (d.w * expand) * 0.5f, hh = (d.h * expand) * 0.5f;
    float x0f = fmaxf(d.x - hw, 0.0f), x1f = fminf(d.x + hw, (float)W);
    float y0f = fmaxf(d.y - hh, 0.0f), y1f = fminf(d.y + hh, (float)H);
    x0f = fminf(x0f, (float)(W + 1)); x1f = fmaxf(x1f, -1.0f);
    y0f = fminf(y0f, (float)(H + 1)); y1f = fmaxf(y1f, -1.0f);
    const int ax0 = (int)floorf(x0f), ax1 = (int)ceilf(x1f), ay0 = (int)floorf(y0f), ay1 = (int)ceilf(y1f);
    if (ax1 - ax0 < min_size || ay1 - ay0 < min_size) return false;
    q[0] = ax0; q[1] = ay0; q[2] = ax1; q[3] = ay1;
    return true;
}

// -------------------------------------------------------- int8 embedding rows
__device__ __forceinline__ unsigned abs_u32(const int v) { return v < 0 ? 0u - (unsigned)v : (unsigned)v; } // (|INT32_MIN| = 2^31 fits)

// The gallery's quantisation rule (include/mars_hip.h, "Gallery match") on one row, by one wavefront, every lane calling: m = max |v| by
// shuffles, out[k] = sign * ((|v| * 127 + m / 2) / m) in 64-bit integers for k < c, zero for the pad channels c .. cp - 1 and where m is 0;
// -> qq = sum out^2 (the same in every lane).  value(k), k < c, is channel k's integer; a lane reads value(k) before it writes out[k] and
// touches no other lane's channels, so value may read the row it writes.
template <class Value>
__device__ __forceinline__ int quantise_row(int8_t *out, const int c, const int cp, const Value value) {
    const int lane = threadIdx.x & 63;
    unsigned m = 0;
    for (int k = lane; k < c; k += 64) m = max(m, abs_u32(value(k)));
    for (int s = 32; s > 0; s >>= 1) m = max(m, (unsigned)__shfl_xor(m, s, 64));
    int qq = 0;
    for (int k = lane; k < cp; k += 64) {
        int o = 0;
        if (k < c && m) {
            const int x = value(k);
            const int mag = (int)(((unsigned long long)abs_u32(x) * 127u + (m >> 1)) / m);
            o = x < 0 ? -mag : mag;
        }
        out[k] = (int8_t)o;
        qq += o * o;
    }
    for (int s = 32; s > 0; s >>= 1) qq += __shfl_xor(qq, s, 64);
    return qq;
}

// ------------------------------------------- sort, buckets, suppress, compact
// The geometry the three NMS kernels share: one workgroup of NMS_THREADS per list, the pair relation NMS_CHUNK rows at a time, NMS_SUBS
// threads on a row, class & (NMS_BUCKETS - 1) as the bucket of a class.  Each kernel declares its own LDS and passes pointers.
#define NMS_THREADS 512
#define NMS_WAVES (NMS_THREADS / 64)
#define NMS_CHUNK 64
#define NMS_SUBS (NMS_THREADS / NMS_CHUNK) // threads that share a row's bucket
#define NMS_BUCKETS 128
__device__ __forceinline__ int class_bucket(const int cls) { return (unsigned)cls & (NMS_BUCKETS - 1); }

// keys[0 .. P), P a power of two >= 2, into descending order: the bitonic network, P/2 compare-exchanges per round.  The caller has written
// the keys (padding included) and made them visible; one barrier behind every round, so the sorted keys are visible on return.
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long *keys, const int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += NMS_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = keys[lo], b = keys[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? a < b : a > b) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
}

// The sorted slots 0 .. n - 1 grouped by bucket_of(slot) (0 .. NMS_BUCKETS - 1; constant 0 when every pair counts): bucket b's slots are
// blist[bstart[b] .. bstart[b + 1]), in no particular order (the bits they produce are OR-ed).  The caller has zeroed bfill[NMS_BUCKETS] and
// made it, and whatever bucket_of reads, visible.  Three barriers: behind the count, the prefix and the scatter.
template <class BucketOf>
__device__ __forceinline__ void class_buckets(const int n, int *bstart, int *bfill, unsigned short *blist, const BucketOf bucket_of) {
    const int tid = threadIdx.x;
    for (int j = tid; j < n; j += NMS_THREADS) atomicAdd(&bfill[bucket_of(j)], 1);
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int b = 0; b < NMS_BUCKETS; b++) { bstart[b] = acc; acc += bfill[b]; bfill[b] = 0; }
        bstart[NMS_BUCKETS] = acc;
    }
    __syncthreads();
    for (int j = tid; j < n; j += NMS_THREADS) {
        const int b = bucket_of(j);
        blist[bstart[b] + atomicAdd(&bfill[b], 1)] = (unsigned short)j;
    }
    __syncthreads();
}

// Greedy suppression over the sorted slots 0 .. n - 1, n <= 64 * WORDS: slot i, unless an earlier slot removed it, removes every later slot j
// of its bucket with pair(row, j), row = load_row(i) read once per row -- the reference's double loop (mars_yolo_test.c:112-130).  The pair
// relation is evaluated NMS_CHUNK rows at a time, NMS_SUBS threads per row, into the bit matrix mask[NMS_CHUNK][2 * WORDS] (32-bit words);
// wave 0 then applies those rows in order, lane w holding 64-bit word w of the removed set.  Leaves removed_s[WORDS]: bit i of the set, ones
// behind slot n's word.  Three barriers per chunk and one behind removed_s; the caller has made the buckets and the operands visible.
template <int WORDS, class BucketOf, class LoadRow, class Pair>
__device__ __forceinline__ void greedy_suppress(const int n, unsigned int *mask, const int *bstart, const unsigned short *blist,
                                                unsigned long long *removed_s, const BucketOf bucket_of, const LoadRow load_row, const Pair pair) {
    const int tid = threadIdx.x;
    const int nw = (n + 63) >> 6;
    unsigned long long removed = 0; // wave 0: lane w (< WORDS) holds word w of the removed set
    for (int i0 = 0; i0 < n; i0 += NMS_CHUNK) {
        const int rows = n - i0 < NMS_CHUNK ? n - i0 : NMS_CHUNK;
        for (int k = tid; k < NMS_CHUNK * 2 * WORDS; k += NMS_THREADS) mask[k] = 0;
        __syncthreads();
        {
            const int r = tid / NMS_SUBS, sub = tid % NMS_SUBS, i = i0 + r;
            if (r < rows) {
                const auto row = load_row(i);
                const int b = bucket_of(i);
                for (int e = bstart[b] + sub; e < bstart[b + 1]; e += NMS_SUBS) {
                    const int j = blist[e];
                    if (j <= i) continue;
                    if (pair(row, j)) atomicOr(&mask[r * 2 * WORDS + (j >> 5)], 1u << (j & 31));
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            // the greedy walk is a dependent chain of `rows` steps; its matrix rows do not depend on it, so they are fetched 16 at a time
            // ahead of the steps that use them (one LDS latency per 16 rows instead of one per row) and a suppressed row is skipped by a
            // select, not a branch
            const int wl = tid < WORDS ? tid : WORDS - 1, c = i0 >> 6; // rows i0.. live in word c of the removed set
            for (int r0 = 0; r0 < rows; r0 += 16) {
                unsigned long long mrow[16];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int r = r0 + k < NMS_CHUNK ? r0 + k : NMS_CHUNK - 1;
                    mrow[k] = *(const unsigned long long *)&mask[r * 2 * WORDS + 2 * wl];
                }
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int r = r0 + k; // bit r of word c: rows >= `rows` hold an all-zero matrix row
                    const unsigned half = r < 32 ? __builtin_amdgcn_readlane((unsigned)removed, c) : __builtin_amdgcn_readlane((unsigned)(removed >> 32), c);
                    const bool dead = (half >> (r & 31)) & 1u; // suppressed boxes suppress nothing
                    removed |= (dead || tid >= nw || r >= rows) ? 0ull : mrow[k];
                }
            }
        }
        __syncthreads(); // the next chunk overwrites the bit matrix
    }
    if (tid < WORDS) removed_s[tid] = tid < nw ? removed : ~0ull;
    __syncthreads();
}

// The survivors of greedy_suppress in sorted order: write(idx, slot) for sorted slot idx, the slot-th survivor; -> their number.  Two
// barriers per NMS_THREADS slots: one between writing wave_cnt (an int[NMS_WAVES]) and reading it, one behind the step (the next rewrites
// it).  This is block_rank's count written out with the step's total read BEHIND the survivors' stores: in the form that calls block_rank
// the tile merge measured 0.181 ms against 0.171 ms (tools/tile_rate.py, profiles/tail_core_ab.json), in this one 0.170 ms.
template <class Write>
__device__ __forceinline__ int compact_survivors(const int n, const unsigned long long *removed_s, int *wave_cnt, const Write write) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int total = 0;
    for (int base = 0; base < n; base += NMS_THREADS) {
        const int idx = base + threadIdx.x;
        const bool keep = idx < n && !((removed_s[idx >> 6] >> (idx & 63)) & 1ull);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wv; w++) off += wave_cnt[w];
        const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) write(idx, slot);
        for (int w = 0; w < NMS_WAVES; w++) total += wave_cnt[w];
        __syncthreads();
    }
    return total;
}

// --------------------------------------------------------------- DFL heads
// the first maximum of 16 int8 bytes (classes c0 .. c0 + 15) folded into (bq, arg)
__device__ __forceinline__ void argmax16(const v4i w, const int c0, int &bq, int &arg) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int d = w[j];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int q = (d << (24 - 8 * b)) >> 24;
            const bool gt = q > bq;
            bq = gt ? q : bq;
            arg = gt ? c0 + 4 * j + b : arg;
        }
    }
}

// one box side from its R bytes at q[i * cs]
__device__ __forceinline__ float dfl_side(const int8_t *q, const int R, const int cs, const float *E) {
    int m = -128;
    for (int i = 0; i < R; i++) m = max(m, (int)q[(size_t)i * cs]);
    float den = E[m - q[0]], num = 0.0f; // 0 * e_0 adds nothing to 0.0f
    for (int i = 1; i < R; i++) {
        const float e = E[m - q[(size_t)i * cs]];
        den = __fadd_rn(den, e);
        num = __fadd_rn(num, __fmul_rn((float)i, e));
    }
    return __fdiv_rn(num, den);
}

// The first class of largest byte of CELLS cells at once (row[k]: the cell's class bytes, nc of them ccs apart) -> bq[k], arg[k].  Pixel rows
// (ccs 1) come as 16-byte loads (any alignment is served) and are compared as integers; UNROLL80 adds the fully unrolled walk of 80-class
// rows, every load in flight before the first compare -- a compile-time choice, a decoder that passes false carries none of it.
template <int CELLS, bool UNROLL80>
__device__ __forceinline__ void dfl_class_walk(const int8_t *const (&row)[CELLS], const int nc, const int ccs, int (&bq)[CELLS], int (&arg)[CELLS]) {
#pragma unroll
    for (int k = 0; k < CELLS; k++) {
        bq[k] = -129;
        arg[k] = 0;
    }
    if (UNROLL80 && ccs == 1 && nc == 80) {
        v4i w[CELLS][5]; // 20 loads of 16 bytes in flight
#pragma unroll
        for (int k = 0; k < CELLS; k++)
#pragma unroll
            for (int j = 0; j < 5; j++) __builtin_memcpy(&w[k][j], row[k] + 16 * j, 16);
#pragma unroll
        for (int k = 0; k < CELLS; k++)
#pragma unroll
            for (int j = 0; j < 5; j++) argmax16(w[k][j], 16 * j, bq[k], arg[k]);
    } else if (ccs == 1) {
        const int n16 = nc >> 4; // whole 16-byte runs inside the row, then its last bytes one by one
        for (int j = 0; j < n16; j++) {
            v4i w[CELLS];
#pragma unroll
            for (int k = 0; k < CELLS; k++) __builtin_memcpy(&w[k], row[k] + 16 * j, 16);
#pragma unroll
            for (int k = 0; k < CELLS; k++) argmax16(w[k], 16 * j, bq[k], arg[k]);
        }
        for (int c = n16 << 4; c < nc; c++) {
            int q[CELLS];
#pragma unroll
            for (int k = 0; k < CELLS; k++) q[k] = row[k][c];
#pragma unroll
            for (int k = 0; k < CELLS; k++)
                if (q[k] > bq[k]) { bq[k] = q[k]; arg[k] = c; }
        }
    } else {
#pragma unroll 4
        for (int c = 0; c < nc; c++) { // planes: a wave reads 64 consecutive bytes of plane c per load
            int q[CELLS];
#pragma unroll
            for (int k = 0; k < CELLS; k++) q[k] = row[k][(size_t)c * ccs];
#pragma unroll
            for (int k = 0; k < CELLS; k++)
                if (q[k] > bq[k]) { bq[k] = q[k]; arg[k] = c; }
        }
    }
}
