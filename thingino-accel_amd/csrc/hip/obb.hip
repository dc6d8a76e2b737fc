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
//                        bits) -- a fourth 4 KB array would lift the kernel above sort_nms_kernel's LDS.  Sort, class buckets (one
//                        bucket under MARS_OBB_AGNOSTIC), the chunked greedy walk and the compaction are tail_core.hpp's, shared
//                        with sort_nms_kernel; the ProbIoU pair predicate is this kernel's.  The survivors are mapped
//                        through the letterbox, and written twice: the 32-byte record and the enclosing upright rectangle as a
//                        24-byte detection, index-aligned; where the caller asks (csn_out), the kept box's (cos, sin) pair too, for the
//                        rotated crops of roi.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../expf_exact.h"
#include "../mhip.h"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

// ------------------------------------------------------------------ decode
#define OBB_DEC_THREADS 256
#define OBB_DEC_CELLS 4

__global__ __launch_bounds__(OBB_DEC_THREADS) void obb_decode_kernel(const mhip_obb_t p) {
    __shared__ float tab_s[4][512];
    __shared__ int wave_cnt[OBB_DEC_CELLS][OBB_DEC_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < p.nheads * 512; i += OBB_DEC_THREADS) tab_s[i >> 9][i & 511] = p.tab[i];
    __syncthreads();
    obb_t *recs = (obb_t *)p.cand + (size_t)f * MAXD;
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
            for (int k = 0; k < OBB_DEC_CELLS; k++) row[k] = cb + (size_t)min(base + k * OBB_DEC_THREADS + tid, npix - 1) * cps;
            dfl_class_walk<OBB_DEC_CELLS, false>(row, nc, ccs, bq, arg);
            // slots: candidates are numbered in cell order = (k, thread)
            bool cand[OBB_DEC_CELLS];
            float cf[OBB_DEC_CELLS];
            int rank[OBB_DEC_CELLS], step;
#pragma unroll
            for (int k = 0; k < OBB_DEC_CELLS; k++) {
                cf[k] = sg[bq[k] + 128];
                cand[k] = base + k * OBB_DEC_THREADS + tid < npix && cf[k] >= conf;
            }
            block_rank<OBB_DEC_THREADS / 64, OBB_DEC_CELLS>(cand, wave_cnt, rank, step);
#pragma unroll
            for (int k = 0; k < OBB_DEC_CELLS; k++) {
                const int slot = total + rank[k];
                if (!cand[k] || slot >= MAXD) continue;
                const int cell = base + k * OBB_DEC_THREADS + tid, gy = cell / W, gx = cell - gy * W;
                const int8_t *q = bb + (size_t)cell * bps;
                float dist[4]; // left, top, right, bottom
                for (int s = 0; s < 4; s++) dist[s] = dfl_side(q + (size_t)s * R * bcs, R, bcs, E);
                const int qa = (int)ab[(size_t)cell * aps] + 128;
                const float ang = at[qa], cs = at[256 + qa], sn = at[512 + qa];
                const float xf = __fmul_rn(__fsub_rn(dist[2], dist[0]), 0.5f), yf = __fmul_rn(__fsub_rn(dist[3], dist[1]), 0.5f);
                const float ax = __fadd_rn((float)gx, 0.5f), ay = __fadd_rn((float)gy, 0.5f);
                obb_t d;
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
            total += step;
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
#define OBB_NMS_THREADS NMS_THREADS

// d = max(a b - c c, 0); a NaN gives 0
__device__ __forceinline__ float obb_det2(const float a, const float b, const float c) {
    const float v = __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, c));
    return v > 0.0f ? v : 0.0f;
}

__global__ __launch_bounds__(OBB_NMS_THREADS) void obb_sort_nms_kernel(const mhip_obb_t p) {
    __shared__ float sx[1024], sy[1024], sa[1024], sb[1024], sc[1024];
    __shared__ int scl[1024];
    __shared__ unsigned short blist[1024]; // box indices grouped by class bucket
    __shared__ int bstart[NMS_BUCKETS + 1], bfill[NMS_BUCKETS];
    __shared__ __attribute__((aligned(16))) unsigned int mask[NMS_CHUNK][32]; // 64 rows x 1024 bits; the sort's keys before that
    __shared__ unsigned long long removed_s[16];
    __shared__ int wave_cnt[OBB_NMS_THREADS / 64];

    const int f = blockIdx.x, tid = threadIdx.x;
    obb_t *cand = (obb_t *)p.cand + (size_t)f * MAXD;
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
    bitonic_sort_desc(keys, P);
    // ---- the records into sorted order, in place: every load before the barrier, every store after it
    {
        obb_t r[2];
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
        if (tid < NMS_BUCKETS) bfill[tid] = 0;
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
    const auto bucket_of = [&](const int j) { return agn ? 0 : class_bucket(scl[j]); };
    class_buckets(n, bstart, bfill, blist, bucket_of);
    // ---- pairs: same class (or agnostic) and ProbIoU above the threshold, in the form exp(-(t1 + t2)) > e_thresh * sqrt(X)
    const float E = p.e_thresh;
    struct row_t { float x, y, a, b, c, d; int cls; };
    greedy_suppress<16>(
        n, &mask[0][0], bstart, blist, removed_s, bucket_of,
        [&](const int i) { return row_t{sx[i], sy[i], sa[i], sb[i], sc[i], obb_det2(sa[i], sb[i], sc[i]), scl[i]}; },
        [&](const row_t &r, const int j) {
            if (!agn && scl[j] != r.cls) return false;
            const float aj = sa[j], bj = sb[j], cj = sc[j];
            const float dj = obb_det2(aj, bj, cj);
            const float ua = __fadd_rn(r.a, aj), ub = __fadd_rn(r.b, bj), uc = __fadd_rn(r.c, cj);
            const float dx = __fsub_rn(r.x, sx[j]), dy = __fsub_rn(r.y, sy[j]);
            const float den = __fsub_rn(__fmul_rn(ua, ub), __fmul_rn(uc, uc));
            const float t1 = __fmul_rn(__fdiv_rn(__fadd_rn(__fmul_rn(ua, __fmul_rn(dy, dy)), __fmul_rn(ub, __fmul_rn(dx, dx))), den), 0.25f);
            const float t2 = __fmul_rn(__fdiv_rn(__fmul_rn(__fmul_rn(uc, -dx), dy), den), 0.5f);
            const float X = __fdiv_rn(den, __fmul_rn(4.0f, sqrtf(__fmul_rn(r.d, dj))));
            const float lhs = expf_exact(-__fadd_rn(t1, t2), expf_exact_tab);
            return lhs > __fmul_rn(E, sqrtf(X)); // a NaN on either side: false
        });
    // ---- compact the survivors in order; the mapping and the enclosing rectangle on the way out
    obb_t *out = (obb_t *)p.out + (size_t)f * MAXD;
    det_t *dets = p.dets ? (det_t *)p.dets + (size_t)f * MAXD : nullptr;
    const int total = compact_survivors(n, removed_s, wave_cnt, [&](const int idx, const int slot) {
        obb_t k = cand[idx]; // sorted order since the permutation above
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
            det_t e;
            e.x = k.x; e.y = k.y; e.conf = k.conf; e.cls = k.cls;
            e.w = __fadd_rn(__fmul_rn(k.w, ac), __fmul_rn(k.h, as));
            e.h = __fadd_rn(__fmul_rn(k.w, as), __fmul_rn(k.h, ac));
            dets[slot] = e;
        }
    });
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
