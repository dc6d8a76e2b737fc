// gallery.hip -- gallery match on gfx950: the int32 embeddings a second stage leaves in HBM (the classify tail's pooled sums, or a caller's
// vectors) -> int8 rows -> dot products against every row of a gallery on v_mfma_i32_16x16x64_i8 -> the best top_k identities per query.
//
// include/mars_hip.h ("Gallery match") states the arithmetic.  Three launches:
//   gm_quantise_kernel   one wavefront per query: max |v| by wave shuffles, q = sign * ((|v| * 127 + m / 2) / m) in 64-bit integers, the
//                        int8 row written zero-padded to the 64-channel multiple (pad rows up to a multiple of 64 queries too, so that
//                        the match kernel loads without a mask), qq = sum q^2 and qinv = 1 / sqrtf(qq);
//   gm_match_kernel      grid (gallery chunks, tiles of 64 queries), four wavefronts.  A wavefront walks every fourth 16-row subtile of
//                        its chunk: the rows are the MFMA's A operand, the 64 queries four B operands (operand maps as in
//                        conv_i8_common.hpp: lane l holds bytes 16 * (l >> 4) .. + 15 of row l & 15; result register e of lane l is
//                        A-row 4 * (l >> 4) + e against B-row l & 15), so a lane sees four gallery rows for each of four queries per
//                        step.  key = (float)dot * ginv; a key that does not reach the lane's eighth-best for that query -- nearly all
//                        of them -- costs a convert, a multiply and a compare.  The others enter a sorted list of eight RANK WORDS in
//                        registers.  A rank word is 64 bits: the key's float bits mapped to an unsigned number of the same order, above
//                        0x7fffffff - row.  Descending words = descending keys, ties to the lower row: one total order, so merging
//                        lists -- across the lanes that share a query (shuffles), across the wavefronts (LDS), across the chunks (the
//                        merge launch) -- gives the same eight words however the gallery was cut.  No atomics, no arrival order;
//   gm_merge_kernel      one wavefront per query: top_k passes of a wave-wide maximum over the chunks' lists, then score = key * qinv,
//                        the threshold and the id lookup.
// With C = 64 the queries' operands stay in registers and a gallery row is read once per query tile; wider embeddings read both
// operands per 64-channel step (L1 / L2 serve the repeats).  The identity scatter is classify.hip's label scatter, called with the match
// results.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

typedef unsigned long long gm_word_t;

#define GM_QT 64        // queries per workgroup
#define GM_KEEP MHIP_MATCH_KEEP
#define GM_MIN_CHUNK 1024
#define GM_MAX_CHUNKS 256

// (key, row) -> rank word; 0 = an empty slot, below every real entry (keys are finite)
__device__ __forceinline__ gm_word_t gm_ord(const float key, const int row) {
    unsigned u = __float_as_uint(key);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
    return ((gm_word_t)u << 32) | (unsigned)(0x7fffffff - row);
}
__device__ __forceinline__ float gm_key(const gm_word_t o) {
    unsigned u = (unsigned)(o >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(u);
}
__device__ __forceinline__ int gm_row(const gm_word_t o) { return 0x7fffffff - (int)(unsigned)o; }

// the sorted list takes o if it beats the last entry
__device__ __forceinline__ void gm_insert(gm_word_t (&l)[GM_KEEP], const gm_word_t o) {
    if (o > l[GM_KEEP - 1]) {
        l[GM_KEEP - 1] = o;
#pragma unroll
        for (int i = GM_KEEP - 1; i > 0; i--) {
            const gm_word_t a = l[i - 1], b = l[i];
            const bool up = b > a;
            l[i - 1] = up ? b : a;
            l[i] = up ? a : b;
        }
    }
}

__device__ __forceinline__ gm_word_t gm_shfl_xor(const gm_word_t v, const int mask) {
    const unsigned lo = __shfl_xor((unsigned)v, mask, 64), hi = __shfl_xor((unsigned)(v >> 32), mask, 64);
    return ((gm_word_t)hi << 32) | lo;
}

// grid: queries rounded up to GM_QT, one wavefront each: tail_core.hpp's quantise_row, its qinv, and the pad rows
__global__ __launch_bounds__(64) void gm_quantise_kernel(const mhip_match_t p) {
    const int n = blockIdx.x, lane = threadIdx.x;
    int8_t *out = p.q + (size_t)n * p.cp;
    if (n >= p.queries) {
        for (int c = lane; c < p.cp; c += 64) out[c] = 0;
        return;
    }
    const int *v = p.vec + (size_t)n * p.c;
    const int qq = quantise_row(out, p.c, p.cp, [v](const int c) { return v[c]; });
    if (lane == 0) {
        p.qq[n] = qq;
        p.qinv[n] = qq ? 1.0f / sqrtf((float)qq) : 0.0f;
    }
}

// grid: (chunks, query tiles).  ONE: cp == 64, the queries' operands stay in registers
template <bool ONE>
__global__ __launch_bounds__(256) void gm_match_kernel(const mhip_match_t p, const int chunks) {
    __shared__ gm_word_t meet[4][GM_QT][GM_KEEP]; // 16 KB
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, frow = lane & 15, fchunk = lane >> 4;
    const int chunk = blockIdx.x, q0 = blockIdx.y * GM_QT;
    const int r0 = chunk * p.chunk, r1 = min(r0 + p.chunk, p.n_rows), nsub = (r1 - r0 + 15) >> 4;
    const size_t cp = (size_t)p.cp;
    const int ksteps = p.cp >> 6;
    const int8_t *qp = p.q + (size_t)(q0 + frow) * cp + fchunk * 16; // query subtile u: + u * 16 rows
    gm_word_t list[4][GM_KEEP];
    float thr[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        thr[u] = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < GM_KEEP; i++) list[u][i] = 0;
    }
    v4i b[4];
    if (ONE) {
#pragma unroll
        for (int u = 0; u < 4; u++) b[u] = *(const v4i *)(qp + (size_t)u * 16 * cp);
    }
    const int8_t *ap = p.rows + (size_t)(r0 + frow) * cp + fchunk * 16;
    v4i a_next = (v4i){0, 0, 0, 0};
    if (ONE && w < nsub) a_next = *(const v4i *)(ap + (size_t)w * 16 * cp);
    for (int s = w; s < nsub; s += 4) {
        const int row0 = r0 + s * 16;
        v4i acc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) acc[u] = (v4i){0, 0, 0, 0};
        if (ONE) {
            const v4i a = a_next;
            if (s + 4 < nsub) a_next = *(const v4i *)(ap + (size_t)(s + 4) * 16 * cp); // the next subtile's rows, under this one's arithmetic
#pragma unroll
            for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[u], acc[u], 0, 0, 0);
        } else {
            const int8_t *as = ap + (size_t)s * 16 * cp;
            for (int ks = 0; ks < ksteps; ks++) {
                const v4i a = *(const v4i *)(as + ks * 64);
#pragma unroll
                for (int u = 0; u < 4; u++) b[u] = *(const v4i *)(qp + (size_t)u * 16 * cp + ks * 64);
#pragma unroll
                for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[u], acc[u], 0, 0, 0);
            }
        }
        const int rb = row0 + fchunk * 4; // this lane's four gallery rows
        const float4 gi = *(const float4 *)(p.ginv + rb);
        const float g[4] = {gi.x, gi.y, gi.z, gi.w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float key = (float)acc[u][e] * g[e]; // two roundings (-ffp-contract=off)
                if (key >= thr[u] && rb + e < r1) {
                    gm_insert(list[u], gm_ord(key, rb + e));
                    if (list[u][GM_KEEP - 1]) thr[u] = gm_key(list[u][GM_KEEP - 1]);
                }
            }
        }
    }
    // the four lanes that share a query column (lane ^ 16, lane ^ 32): afterwards each of them holds the merged list
#pragma unroll
    for (int u = 0; u < 4; u++) {
#pragma unroll
        for (int step = 16; step <= 32; step <<= 1) {
            gm_word_t other[GM_KEEP];
#pragma unroll
            for (int i = 0; i < GM_KEEP; i++) other[i] = gm_shfl_xor(list[u][i], step);
#pragma unroll
            for (int i = 0; i < GM_KEEP; i++) gm_insert(list[u], other[i]);
        }
        if (fchunk == 0) {
#pragma unroll
            for (int i = 0; i < GM_KEEP; i++) meet[w][u * 16 + frow][i] = list[u][i];
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < GM_QT && q0 + t < p.queries) { // the four wavefronts' lists of query q0 + t
        gm_word_t l[GM_KEEP];
#pragma unroll
        for (int i = 0; i < GM_KEEP; i++) l[i] = meet[0][t][i];
        for (int ww = 1; ww < 4; ww++) {
#pragma unroll
            for (int i = 0; i < GM_KEEP; i++) gm_insert(l, meet[ww][t][i]);
        }
        gm_word_t *dst = p.part + ((size_t)(q0 + t) * chunks + chunk) * GM_KEEP;
#pragma unroll
        for (int i = 0; i < GM_KEEP; i++) dst[i] = l[i];
    }
}

// One wavefront per query.  Pass k: the largest word below pass k - 1's (rows are distinct, so are the words of real entries).
__global__ __launch_bounds__(64) void gm_merge_kernel(const mhip_match_t p, const int chunks) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const gm_word_t *src = p.part + (size_t)n * chunks * GM_KEEP;
    const int cand = chunks * GM_KEEP;
    gm_word_t mine = 0, prev = ~(gm_word_t)0;
    for (int k = 0; k < p.top_k; k++) {
        gm_word_t best = 0;
        for (int i = lane; i < cand; i += 64) {
            const gm_word_t o = src[i];
            if (o < prev && o > best) best = o;
        }
        for (int s = 32; s > 0; s >>= 1) {
            const gm_word_t o = gm_shfl_xor(best, s);
            best = o > best ? o : best;
        }
        if (lane == k) mine = best;
        if (best) prev = best; // (best == 0: nothing is left, and nothing will be)
        else prev = 0;
    }
    if (lane < p.top_k) {
        cls_t r;
        r.cls = -1;
        r.score = 0.0f;
        int row = -1;
        if (mine && p.qq[n]) {
            const float score = gm_key(mine) * p.qinv[n];
            if (!(p.min_score != 0.0f && score < p.min_score)) {
                row = gm_row(mine);
                r.cls = p.ids[row];
                r.score = score;
            }
        }
        ((cls_t *)p.top)[(size_t)n * p.top_k + lane] = r;
        p.top_row[(size_t)n * p.top_k + lane] = row;
    }
}

// ---- launchers
extern "C" int mhip_match_chunk(int n_rows) {
    if (n_rows < 1 || n_rows > MHIP_MATCH_MAX_ROWS) return 0;
    // at most GM_MAX_CHUNKS lists per query for the merge to read; at least GM_MIN_CHUNK rows, so that the meeting of a workgroup's lists
    // stays small beside its rows
    const int c = (((n_rows + GM_MAX_CHUNKS - 1) / GM_MAX_CHUNKS) + 63) & ~63;
    return c < GM_MIN_CHUNK ? GM_MIN_CHUNK : c;
}

extern "C" int mhip_match(const mhip_match_t *p) {
    if (!p || !p->vec || !p->q || !p->qq || !p->qinv || !p->rows || !p->ginv || !p->ids || !p->part || !p->top || !p->top_row) return -1;
    if (p->queries < 1 || p->queries > 65535 || p->c < 1 || p->c > MHIP_MATCH_MAX_C || p->cp != ((p->c + 63) & ~63)) return -1;
    if (p->top_k < 1 || p->top_k > GM_KEEP || !(p->min_score >= 0.0f)) return -1;
    if (p->chunk < 64 || p->chunk != mhip_match_chunk(p->n_rows)) return -1;
    const int chunks = (p->n_rows + p->chunk - 1) / p->chunk;
    const int tiles = (p->queries + GM_QT - 1) / GM_QT;
    hipStream_t st = mhip_stream_native();
    hipLaunchKernelGGL(gm_quantise_kernel, dim3((unsigned)(tiles * GM_QT)), dim3(64), 0, st, *p);
    if (p->cp == 64) hipLaunchKernelGGL(gm_match_kernel<true>, dim3((unsigned)chunks, (unsigned)tiles), dim3(256), 0, st, *p, chunks);
    else hipLaunchKernelGGL(gm_match_kernel<false>, dim3((unsigned)chunks, (unsigned)tiles), dim3(256), 0, st, *p, chunks);
    hipLaunchKernelGGL(gm_merge_kernel, dim3((unsigned)p->queries), dim3(64), 0, st, *p, chunks);
    return mhip_check(hipGetLastError(), "gallery match");
}
