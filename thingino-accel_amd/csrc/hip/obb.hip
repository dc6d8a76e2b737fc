// obb.hip -- oriented boxes of YOLOv8-obb style heads on gfx950: the DFL decode with one angle byte per cell, a stable sort by
// (confidence descending, index ascending) and greedy suppression of rotated rectangles by ProbIoU.
//
// include/mars_hip.h ("Oriented boxes") states the arithmetic; every float operation below is one rounding (_rn intrinsics, the build
// passes -ffp-contract=off), division and square root are the correctly rounded ones (`/` and sqrtf under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt; NOT __fsqrt_rn, which is the native approximation in this toolchain), and the one
// exponential of the pair relation is csrc/expf_exact.h, the host libm's expf bit for bit.  Two launches, one workgroup per frame each:
//   obb_decode_kernel    the walk of dfl_decode_kernel (csrc/hip/yolo_tail.hip: 1024 cells per step, thread t the cells t, 256 + t, ...,
//                        every class byte read, box bytes only for the cells that pass, slots from one ordered ballot count per step:
//                        a function of the bytes alone, no atomics) with the angle byte of a passing cell read at
//                        base + cell * pix_step, its angle, cosine and sine taken from the host's per-head tables, and the rotated
//                        centre.  Writes 32-byte records, the (cos, sin) pair of every record beside them, and the count.
//   obb_sort_nms_kernel  512 threads, 35 KB of LDS -- at most sort_nms_kernel's, so that the tail still shares a CU with the next batch's
//                        convolutions.  Bitonic sort of (confidence bits << 10 | 1023 - index) keys: confidences are >= 0 and never
//                        NaN here, so the bit pattern orders them, and the order is plain and stable -- no tie replay, the reference
//                        has no such head.  The records are then permuted in place in HBM (every load before a barrier, every store
//                        after it) and x, y, a, b, c and the class of every sorted box go to LDS; d = max(a b - c c, 0) of the row's
//                        box is computed once per row and of the other box from its a, b, c per pair (three operations, the same
//                        bits) -- a fourth 4 KB array would lift the kernel above sort_nms_kernel's LDS.  The pair relation is
//                        evaluated 64 rows at a time inside class buckets (class & 127, the exact class still compared; one bucket
//                        under MARS_OBB_AGNOSTIC) into an 8 KB bit matrix; wave 0 applies the rows greedily (suppressed boxes suppress
//                        nothing) exactly as sort_nms_kernel does; the survivors are compacted in order by ballot prefix, mapped
//                        through the letterbox, and written twice: the 32-byte record and the enclosing upright rectangle as a
//                        24-byte detection, index-aligned; where the caller asks (csn_out), the kept box's (cos, sin) pair too, for the
//                        rotated crops of roi.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../expf_exact.h"
#include "../mhip.h"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define MAXD 1000

typedef int v4i __attribute__((ext_vector_type(4)));

struct obb_rec {
    float x, y, w, h, conf;
    int cls;
    float angle;
    int pred;
};
struct obb_det {
    float x, y, w, h, conf;
    int cls;
};

// ------------------------------------------------------------------ decode
#define OBB_DEC_THREADS 256
#define OBB_DEC_CELLS 4

// the first maximum of 16 int8 bytes (classes c0 .. c0 + 15) folded into (bq, arg)
__device__ __forceinline__ void obb_argmax16(const v4i w, const int c0, int &bq, int &arg) {
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

// one box side from its R bytes at q[i * cs]: the DFL tail's expression
__device__ __forceinline__ float obb_side(const int8_t *q, const int R, const int cs, const float *E) {
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

__global__ __launch_bounds__(OBB_DEC_THREADS) void obb_decode_kernel(const mhip_obb_t p) {
    __shared__ float tab_s[4][512];
    __shared__ int wave_cnt[OBB_DEC_CELLS][OBB_DEC_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < p.nheads * 512; i += OBB_DEC_THREADS) tab_s[i >> 9][i & 511] = p.tab[i];
    __syncthreads();
    obb_rec *recs = (obb_rec *)p.cand + (size_t)f * MAXD;
    float *csn = p.csn + (size_t)f * MAXD * 2;
    const float conf = p.conf;
    const int R = p.reg_max;
    int total = 0, pred0 = 0; // pred0: the prediction index of this head's cell 0
    for (int hd = 0; hd < p.nheads && total < MAXD; pred0 += p.h[hd] * p.w[hd], hd++) {
        const int8_t *cb = p.cls[hd] + (size_t)f * p.cls_frame_stride[hd];
        const int8_t *bb = p.box[hd] + (size_t)f * p.box_frame_stride[hd];
        const int8_t *ab = p.ang[hd] + (size_t)f * p.ang_frame_stride[hd];
        const int W = p.w[hd], npix = p.h[hd] * W, nc = p.nc[hd];
        const int cps = p.cls_pix_step[hd], ccs = p.cls_ch_step[hd], bps = p.box_pix_step[hd], bcs = p.box_ch_step[hd], aps = p.ang_pix_step[hd];
        const float *E = tab_s[hd], *sg = E + 256;
        const float *at = p.atab + hd * 768;
        const float fstride = (float)p.stride[hd];
        for (int base = 0; base < npix && total < MAXD; base += OBB_DEC_THREADS * OBB_DEC_CELLS) {
            int bq[OBB_DEC_CELLS], arg[OBB_DEC_CELLS];
            const int8_t *row[OBB_DEC_CELLS]; // a cell past the end reads the last cell's bytes and is dropped below
#pragma unroll
            for (int k = 0; k < OBB_DEC_CELLS; k++) {
                bq[k] = -129;
                arg[k] = 0;
                row[k] = cb + (size_t)min(base + k * OBB_DEC_THREADS + tid, npix - 1) * cps;
            }
            if (ccs == 1) {
                const int n16 = nc >> 4; // whole 16-byte runs inside the row (any alignment is served), then its last bytes one by one
                for (int j = 0; j < n16; j++) {
                    v4i w[OBB_DEC_CELLS];
#pragma unroll
                    for (int k = 0; k < OBB_DEC_CELLS; k++) __builtin_memcpy(&w[k], row[k] + 16 * j, 16);
#pragma unroll
                    for (int k = 0; k < OBB_DEC_CELLS; k++) obb_argmax16(w[k], 16 * j, bq[k], arg[k]);
                }
                for (int c = n16 << 4; c < nc; c++) {
                    int q[OBB_DEC_CELLS];
#pragma unroll
                    for (int k = 0; k < OBB_DEC_CELLS; k++) q[k] = row[k][c];
#pragma unroll
                    for (int k = 0; k < OBB_DEC_CELLS; k++)
                        if (q[k] > bq[k]) { bq[k] = q[k]; arg[k] = c; }
                }
            } else {
#pragma unroll 4
                for (int c = 0; c < nc; c++) { // planes: a wave reads 64 consecutive bytes of plane c per load
                    int q[OBB_DEC_CELLS];
#pragma unroll
                    for (int k = 0; k < OBB_DEC_CELLS; k++) q[k] = row[k][(size_t)c * ccs];
#pragma unroll
                    for (int k = 0; k < OBB_DEC_CELLS; k++)
                        if (q[k] > bq[k]) { bq[k] = q[k]; arg[k] = c; }
                }
            }
            // slots: candidates are numbered in cell order = (k, thread); one count per (k, wave)
            bool cand[OBB_DEC_CELLS];
            float cf[OBB_DEC_CELLS];
            int before[OBB_DEC_CELLS];
#pragma unroll
            for (int k = 0; k < OBB_DEC_CELLS; k++) {
                cf[k] = sg[bq[k] + 128];
                cand[k] = base + k * OBB_DEC_THREADS + tid < npix && cf[k] >= conf;
                const unsigned long long m = __ballot(cand[k]);
                before[k] = __popcll(m & ((1ull << lane) - 1ull));
                if (lane == 0) wave_cnt[k][wv] = __popcll(m);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < OBB_DEC_CELLS; k++) {
                int slot = total + before[k];
#pragma unroll
                for (int w = 0; w < OBB_DEC_THREADS / 64; w++) {
                    const int c = wave_cnt[k][w];
                    if (w < wv) slot += c;
                    total += c;
                }
                if (!cand[k] || slot >= MAXD) continue;
                const int cell = base + k * OBB_DEC_THREADS + tid, gy = cell / W, gx = cell - gy * W;
                const int8_t *q = bb + (size_t)cell * bps;
                float dist[4]; // left, top, right, bottom
                for (int s = 0; s < 4; s++) dist[s] = obb_side(q + (size_t)s * R * bcs, R, bcs, E);
                const int qa = (int)ab[(size_t)cell * aps] + 128;
                const float ang = at[qa], cs = at[256 + qa], sn = at[512 + qa];
                const float xf = __fmul_rn(__fsub_rn(dist[2], dist[0]), 0.5f), yf = __fmul_rn(__fsub_rn(dist[3], dist[1]), 0.5f);
                const float ax = __fadd_rn((float)gx, 0.5f), ay = __fadd_rn((float)gy, 0.5f);
                obb_rec d;
                d.x = __fmul_rn(__fadd_rn(__fsub_rn(__fmul_rn(xf, cs), __fmul_rn(yf, sn)), ax), fstride);
                d.y = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(xf, sn), __fmul_rn(yf, cs)), ay), fstride);
                d.w = __fmul_rn(__fadd_rn(dist[0], dist[2]), fstride);
                d.h = __fmul_rn(__fadd_rn(dist[1], dist[3]), fstride);
                d.conf = cf[k];
                d.cls = arg[k];
                d.angle = ang;
                d.pred = pred0 + cell;
                recs[slot] = d;
                csn[2 * slot] = cs;
                csn[2 * slot + 1] = sn;
            }
            __syncthreads(); // wave_cnt is rewritten by the next step
        }
    }
    if (total > MAXD) total = MAXD;
    if (tid == 0) {
        if (p.raw_counts) p.raw_counts[f] = total;
        p.cand_counts[f] = total;
    }
}

// -------------------------------------------------------- sort + suppress
#define OBB_NMS_THREADS 512
#define OBB_NMS_CHUNK 64
#define OBB_NMS_SUBS (OBB_NMS_THREADS / OBB_NMS_CHUNK) // threads that share a row's bucket
#define OBB_NMS_BUCKETS 128

// d = max(a b - c c, 0); a NaN gives 0
__device__ __forceinline__ float obb_det2(const float a, const float b, const float c) {
    const float v = __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, c));
    return v > 0.0f ? v : 0.0f;
}

__global__ __launch_bounds__(OBB_NMS_THREADS) void obb_sort_nms_kernel(const mhip_obb_t p) {
    __shared__ float sx[1024], sy[1024], sa[1024], sb[1024], sc[1024];
    __shared__ int scl[1024];
    __shared__ unsigned short blist[1024]; // box indices grouped by class bucket
    __shared__ int bstart[OBB_NMS_BUCKETS + 1], bfill[OBB_NMS_BUCKETS];
    __shared__ __attribute__((aligned(16))) unsigned int mask[OBB_NMS_CHUNK][32]; // 64 rows x 1024 bits; the sort's keys before that
    __shared__ unsigned long long removed_s[16];
    __shared__ int wave_cnt[OBB_NMS_THREADS / 64];

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    obb_rec *cand = (obb_rec *)p.cand + (size_t)f * MAXD;
    float2 *csn = (float2 *)p.csn + (size_t)f * MAXD;
    int n = p.cand_counts[f];
    n = n < 0 ? 0 : n > MAXD ? MAXD : n;
    if (n == 0) { // uniform
        if (tid == 0) {
            p.out_counts[f] = 0;
            if (p.counts) p.counts[f] = 0;
        }
        return;
    }
    // ---- sort: (confidence bits, 1023 - index) descending = confidence descending, index ascending
    unsigned long long *keys = (unsigned long long *)&mask[0][0];
    int P = 2;
    while (P < n) P <<= 1;
    for (int r = tid; r < P; r += OBB_NMS_THREADS) {
        unsigned long long k = 0; // padding: below every real key (index 1023 does not exist)
        if (r < n) k = ((unsigned long long)__float_as_uint(cand[r].conf) << 10) | (unsigned)(1023 - r);
        keys[r] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += OBB_NMS_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = keys[lo], b = keys[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? a < b : a > b) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    // ---- the records into sorted order, in place: every load before the barrier, every store after it
    {
        obb_rec r[2];
        float2 t[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int j = tid + q * OBB_NMS_THREADS;
            if (j < n) {
                const int src = 1023 - (int)(keys[j] & 1023);
                r[q] = cand[src];
                t[q] = csn[src];
            }
        }
        if (tid < OBB_NMS_BUCKETS) bfill[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int j = tid + q * OBB_NMS_THREADS;
            if (j < n) {
                cand[j] = r[q];
                csn[j] = t[q];
                const float cs = t[q].x, sn = t[q].y;
                const float A = __fdiv_rn(__fmul_rn(r[q].w, r[q].w), 12.0f), B = __fdiv_rn(__fmul_rn(r[q].h, r[q].h), 12.0f);
                const float cc = __fmul_rn(cs, cs), ss = __fmul_rn(sn, sn);
                sx[j] = r[q].x;
                sy[j] = r[q].y;
                sa[j] = __fadd_rn(__fmul_rn(A, cc), __fmul_rn(B, ss));
                sb[j] = __fadd_rn(__fmul_rn(A, ss), __fmul_rn(B, cc));
                sc[j] = __fmul_rn(__fsub_rn(A, B), __fmul_rn(cs, sn));
                scl[j] = r[q].cls;
            }
        }
    }
    __syncthreads(); // the keys are dead: the bit matrix takes their place
    // ---- class buckets (one bucket when every pair counts)
    const bool agn = p.agnostic != 0;
    for (int j = tid; j < n; j += OBB_NMS_THREADS) atomicAdd(&bfill[agn ? 0 : (unsigned)scl[j] & (OBB_NMS_BUCKETS - 1)], 1);
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int b = 0; b < OBB_NMS_BUCKETS; b++) { bstart[b] = acc; acc += bfill[b]; bfill[b] = 0; }
        bstart[OBB_NMS_BUCKETS] = acc;
    }
    __syncthreads();
    for (int j = tid; j < n; j += OBB_NMS_THREADS) {
        const int b = agn ? 0 : (unsigned)scl[j] & (OBB_NMS_BUCKETS - 1);
        blist[bstart[b] + atomicAdd(&bfill[b], 1)] = (unsigned short)j; // (the order inside a bucket does not matter: bits are OR-ed)
    }
    __syncthreads();
    const float E = p.e_thresh;
    const int nw = (n + 63) >> 6;
    unsigned long long removed = 0; // wave 0: lane w (< 16) holds word w of the removed set
    for (int i0 = 0; i0 < n; i0 += OBB_NMS_CHUNK) {
        const int rows = n - i0 < OBB_NMS_CHUNK ? n - i0 : OBB_NMS_CHUNK;
        for (int k = tid; k < OBB_NMS_CHUNK * 32; k += OBB_NMS_THREADS) ((unsigned int *)mask)[k] = 0;
        __syncthreads();
        {
            const int r = tid / OBB_NMS_SUBS, sub = tid % OBB_NMS_SUBS, i = i0 + r;
            if (r < rows) {
                const float xi = sx[i], yi = sy[i], ai = sa[i], bi = sb[i], ci = sc[i];
                const float di = obb_det2(ai, bi, ci);
                const int cli = scl[i];
                const int b = agn ? 0 : (unsigned)cli & (OBB_NMS_BUCKETS - 1);
                for (int e = bstart[b] + sub; e < bstart[b + 1]; e += OBB_NMS_SUBS) {
                    const int j = blist[e];
                    if (j <= i || (!agn && scl[j] != cli)) continue;
                    const float aj = sa[j], bj = sb[j], cj = sc[j];
                    const float dj = obb_det2(aj, bj, cj);
                    const float ua = __fadd_rn(ai, aj), ub = __fadd_rn(bi, bj), uc = __fadd_rn(ci, cj);
                    const float dx = __fsub_rn(xi, sx[j]), dy = __fsub_rn(yi, sy[j]);
                    const float den = __fsub_rn(__fmul_rn(ua, ub), __fmul_rn(uc, uc));
                    const float t1 = __fmul_rn(__fdiv_rn(__fadd_rn(__fmul_rn(ua, __fmul_rn(dy, dy)), __fmul_rn(ub, __fmul_rn(dx, dx))), den), 0.25f);
                    const float t2 = __fmul_rn(__fdiv_rn(__fmul_rn(__fmul_rn(uc, -dx), dy), den), 0.5f);
                    const float X = __fdiv_rn(den, __fmul_rn(4.0f, sqrtf(__fmul_rn(di, dj))));
                    const float lhs = expf_exact(-__fadd_rn(t1, t2), expf_exact_tab);
                    if (lhs > __fmul_rn(E, sqrtf(X))) atomicOr(&mask[r][j >> 5], 1u << (j & 31)); // a NaN on either side: false
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            // the greedy walk of sort_nms_kernel: a dependent chain of `rows` steps whose matrix rows are fetched 16 at a time ahead of the
            // steps that use them; a suppressed row is skipped by a select, not a branch
            const int wl = tid < 16 ? tid : 15, c = i0 >> 6; // lane w holds word w of the removed set; rows i0.. live in word c
            for (int r0 = 0; r0 < rows; r0 += 16) {
                unsigned long long mrow[16];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int r = r0 + k < OBB_NMS_CHUNK ? r0 + k : OBB_NMS_CHUNK - 1;
                    mrow[k] = *(const unsigned long long *)&mask[r][2 * wl];
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
    if (tid < 16) removed_s[tid] = tid < nw ? removed : ~0ull;
    __syncthreads();
    // ---- compact the survivors in order; the mapping and the enclosing rectangle on the way out
    obb_rec *out = (obb_rec *)p.out + (size_t)f * MAXD;
    obb_det *dets = p.dets ? (obb_det *)p.dets + (size_t)f * MAXD : nullptr;
    int total = 0;
    for (int base = 0; base < n; base += OBB_NMS_THREADS) {
        const int idx = base + tid;
        const bool keep = idx < n && !((removed_s[idx >> 6] >> (idx & 63)) & 1ull);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wv; w++) off += wave_cnt[w];
        const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) {
            obb_rec k = cand[idx]; // sorted order since the permutation above
            const float2 t = csn[idx];
            if (p.map) {
                k.x = __fmul_rn(__fsub_rn(k.x, (float)p.px), p.rx);
                k.y = __fmul_rn(__fsub_rn(k.y, (float)p.py), p.ry);
                k.w = __fmul_rn(k.w, p.rx);
                k.h = __fmul_rn(k.h, p.rx); // both sides by rx: they lie along the box's own axes
            }
            out[slot] = k;
            if (p.csn_out) ((float2 *)p.csn_out + (size_t)f * MAXD)[slot] = t;
            if (dets) {
                const float ac = fabsf(t.x), as = fabsf(t.y);
                obb_det e;
                e.x = k.x; e.y = k.y; e.conf = k.conf; e.cls = k.cls;
                e.w = __fadd_rn(__fmul_rn(k.w, ac), __fmul_rn(k.h, as));
                e.h = __fadd_rn(__fmul_rn(k.w, as), __fmul_rn(k.h, ac));
                dets[slot] = e;
            }
        }
        for (int w = 0; w < OBB_NMS_THREADS / 64; w++) total += wave_cnt[w];
        __syncthreads();
    }
    if (tid == 0) {
        p.out_counts[f] = total;
        if (p.counts) p.counts[f] = total;
    }
}

static int obb_nms_args_ok(const mhip_obb_t *p) {
    return p && p->frames > 0 && p->frames <= 65535 && p->cand && p->csn && p->cand_counts && p->out && p->out_counts && p->out != p->cand &&
           (!p->counts == !p->dets);
}

extern "C" int mhip_obb_nms(const mhip_obb_t *p) {
    if (!obb_nms_args_ok(p)) return -1;
    hipLaunchKernelGGL(obb_sort_nms_kernel, dim3(p->frames), dim3(OBB_NMS_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "oriented sort + nms");
}

extern "C" int mhip_obb(const mhip_obb_t *p) {
    if (!obb_nms_args_ok(p) || p->nheads <= 0 || p->nheads > 4 || !p->tab || !p->atab || p->reg_max < 2 || p->reg_max > 32) return -1;
    for (int k = 0; k < p->nheads; k++)
        if (!p->box[k] || !p->cls[k] || !p->ang[k] || p->h[k] <= 0 || p->w[k] <= 0 || p->nc[k] < 1 || p->box_pix_step[k] <= 0 || p->box_ch_step[k] <= 0 ||
            p->cls_pix_step[k] <= 0 || p->cls_ch_step[k] <= 0 || p->ang_pix_step[k] <= 0)
            return -1;
    hipLaunchKernelGGL(obb_decode_kernel, dim3(p->frames), dim3(OBB_DEC_THREADS), 0, mhip_stream_native(), *p);
    const int rc = mhip_check(hipGetLastError(), "decode oriented heads");
    return rc ? rc : mhip_obb_nms(p);
}
