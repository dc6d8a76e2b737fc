// classify.hip -- second-stage labels on gfx950: the int8 feature map a classifier / embedder leaves in HBM -> per-channel int32 sums (the
// global average pool's numerator) -> ranked top-K entries per frame, and the scatter of every crop's top-1 back onto the detection it came from.
//
// include/mars_hip.h ("Second-stage labels") states the arithmetic.  The reference stops one step earlier: its graph fails on GLOBAL_AVGPOOL
// and FC (src/mars/mars_runtime.c) and a deployment would read the whole map back.  Here the map never leaves HBM:
//   cls_pool_planes_kernel    [C][H][W] tensors: a wavefront owns one part of one channel's plane, a contiguous run of bytes, reads it 16 bytes
//                             per lane (single bytes up to the first and behind the last 16-byte boundary) and sums four bytes per
//                             v_dot4_i32_i8 against ones;
//   cls_pool_rows_kernel<V>   pixel rows (NHWC tensors, NCHW-tagged ones held pixels x channels, padded graph outputs, a channel slice of a
//                             wider row): a lane owns V adjacent channels and walks down the pixels, V = 16 / 4 / 1 bytes per load as the
//                             alignment allows; a byte is taken out of its dword by a dot product with a one-hot selector; the lanes that share
//                             channels meet in LDS;
//   cls_finish_kernel         one wavefront per frame: sums the parts (integers: any order gives the same bits, which is why the parts are
//                             combined by a second launch and neither by atomics nor in floating point), ranks, scores, and adds the softmax
//                             denominator left to right on one lane;
//   cls_label_fill / _scatter the label array of the detector: every entry {-1, 0}, then crop k's top-1 at (roi.frame, roi.det).
// Every byte is read once.  The pooling launch is bound by HBM reads; everything else is noise beside it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../expf_exact.h"
#include "../mhip.h"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define CLS_ONES 0x01010101

__device__ __forceinline__ int cls_wave_sum(int v) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// grid: (channel quads x parts, frames); wave w of a workgroup: channel 4 * quad + w, part `part` of its plane
__global__ __launch_bounds__(256) void cls_pool_planes_kernel(const mhip_classify_t p, const int quads, const int seg) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int quad = blockIdx.x % quads, part = blockIdx.x / quads, f = blockIdx.y;
    const int ch = quad * 4 + w;
    if (ch >= p.c) return;
    const long long lo = (long long)part * seg;
    const int n = (int)max(0LL, min((long long)p.hw - lo, (long long)seg));
    const int8_t *a = p.base + (size_t)f * p.frame_stride + (size_t)ch * (size_t)p.ch_step + (size_t)lo;
    const int head = min(n, (int)((16u - (unsigned)((uintptr_t)a & 15)) & 15u)), nv = (n - head) >> 4;
    int acc = 0;
    if (lane < head) acc += a[lane];
    const uint4 *v = (const uint4 *)(a + head);
    int i = lane;
    for (; i + 192 < nv; i += 256) { // four independent loads in flight per lane
        const uint4 x0 = v[i], x1 = v[i + 64], x2 = v[i + 128], x3 = v[i + 192];
#define CLS_ADD4(q)                                                   \
    acc = __builtin_amdgcn_sdot4((int)q.x, CLS_ONES, acc, false);     \
    acc = __builtin_amdgcn_sdot4((int)q.y, CLS_ONES, acc, false);     \
    acc = __builtin_amdgcn_sdot4((int)q.z, CLS_ONES, acc, false);     \
    acc = __builtin_amdgcn_sdot4((int)q.w, CLS_ONES, acc, false)
        CLS_ADD4(x0); CLS_ADD4(x1); CLS_ADD4(x2); CLS_ADD4(x3);
    }
    for (; i < nv; i += 64) {
        const uint4 x0 = v[i];
        CLS_ADD4(x0);
    }
#undef CLS_ADD4
    const int done = head + (nv << 4);
    if (done + lane < n) acc += a[done + lane]; // fewer than 16 bytes are left
    acc = cls_wave_sum(acc);
    if (lane == 0) p.partial[((size_t)f * p.nsplit + part) * p.c + ch] = acc;
}

template <int V> struct cls_vec_t;
template <> struct cls_vec_t<16> { typedef uint4 type; };
template <> struct cls_vec_t<4> { typedef unsigned type; };
template <> struct cls_vec_t<1> { typedef int8_t type; };

template <int V> __device__ __forceinline__ void cls_acc(int *acc, const typename cls_vec_t<V>::type x);
template <> __device__ __forceinline__ void cls_acc<1>(int *acc, const int8_t x) { acc[0] += x; }
template <> __device__ __forceinline__ void cls_acc<4>(int *acc, const unsigned x) {
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = __builtin_amdgcn_sdot4((int)x, 1 << (8 * k), acc[k], false); // byte k of x, sign-extended
}
template <> __device__ __forceinline__ void cls_acc<16>(int *acc, const uint4 x) {
    cls_acc<4>(acc, x.x); cls_acc<4>(acc + 4, x.y); cls_acc<4>(acc + 8, x.z); cls_acc<4>(acc + 12, x.w);
}

// grid: (column tiles x parts, frames).  A workgroup covers tpr groups of V channels; thread t: group t % tpr, pixels part_lo + t / tpr + k * rpi
template <int V>
__global__ __launch_bounds__(256) void cls_pool_rows_kernel(const mhip_classify_t p, const int groups, const int tpr, const int tiles, const int pps) {
    typedef typename cls_vec_t<V>::type vec_t;
    __shared__ int red[256 * V];
    const int t = threadIdx.x, rpi = 256 / tpr;
    const int tile = blockIdx.x % tiles, part = blockIdx.x / tiles, f = blockIdx.y;
    const int r = t / tpr, gl = t - r * tpr, g = tile * tpr + gl;
    const int p0 = (int)min((long long)part * pps, (long long)p.hw), p1 = (int)min((long long)p0 + pps, (long long)p.hw);
    int acc[V];
#pragma unroll
    for (int k = 0; k < V; k++) acc[k] = 0;
    if (r < rpi && g < groups) {
        const int8_t *a = p.base + (size_t)f * p.frame_stride + (size_t)g * V;
        const size_t pitch = (size_t)p.pix_step;
        int px = p0 + r;
        for (; px + 3 * rpi < p1; px += 4 * rpi) { // four independent loads in flight per lane
            const vec_t x0 = *(const vec_t *)(a + (size_t)px * pitch), x1 = *(const vec_t *)(a + (size_t)(px + rpi) * pitch);
            const vec_t x2 = *(const vec_t *)(a + (size_t)(px + 2 * rpi) * pitch), x3 = *(const vec_t *)(a + (size_t)(px + 3 * rpi) * pitch);
            cls_acc<V>(acc, x0); cls_acc<V>(acc, x1); cls_acc<V>(acc, x2); cls_acc<V>(acc, x3);
        }
        for (; px < p1; px += rpi) cls_acc<V>(acc, *(const vec_t *)(a + (size_t)px * pitch));
    }
#pragma unroll
    for (int k = 0; k < V; k++) red[t * V + k] = acc[k];
    __syncthreads();
    // thread o: channel o of the tile = group o / V, byte o % V: the rpi threads that walked that group
    for (int o = t; o < tpr * V; o += 256) {
        const int og = o / V, k = o - og * V, ch = (tile * tpr + og) * V + k;
        if (ch >= p.c) continue;
        int s = 0;
        for (int rr = 0; rr < rpi; rr++) s += red[(rr * tpr + og) * V + k];
        p.partial[((size_t)f * p.nsplit + part) * p.c + ch] = s;
    }
}

// One wavefront per frame.  key(c) = sum[c] * 4096 + (4095 - c): descending keys = descending sums, ties to the lower channel.
__global__ __launch_bounds__(64) void cls_finish_kernel(const mhip_classify_t p) {
    __shared__ int s[MHIP_CLS_MAX_C];
    __shared__ float e[MHIP_CLS_MAX_C];
    const int f = blockIdx.x, lane = threadIdx.x, C = p.c;
    for (int c = lane; c < C; c += 64) {
        const int *q = p.partial + (size_t)f * p.nsplit * C + c;
        int v = 0;
        for (int k = 0; k < p.nsplit; k++) v += q[(size_t)k * C];
        s[c] = v;
        p.sums[(size_t)f * C + c] = v;
    }
    __syncthreads();
    int cls[MHIP_CLS_MAX_TOPK];
    long long prev = 0x7fffffffffffffffLL;
#pragma unroll
    for (int k = 0; k < MHIP_CLS_MAX_TOPK; k++) {
        long long best = -0x7fffffffffffffffLL - 1;
        if (k < p.top_k) {
            for (int c = lane; c < C; c += 64) {
                const long long key = (long long)s[c] * 4096 + (4095 - c);
                if (key < prev && key > best) best = key;
            }
            for (int sh = 32; sh > 0; sh >>= 1) {
                const long long o = __shfl_xor(best, sh, 64);
                best = o > best ? o : best;
            }
        }
        const bool found = best != -0x7fffffffffffffffLL - 1;
        cls[k] = found ? 4095 - (int)(best & 4095) : -1;
        if (found) prev = best;
    }
    // float32, every operation rounded on its own (-ffp-contract=off): logit = ((float)sum / (float)hw) * scale
    const float fhw = (float)p.hw;
    float den = 1.0f;
    if (p.softmax) {
        const float lb = ((float)s[cls[0]] / fhw) * p.scale;
        for (int c = lane; c < C; c += 64) e[c] = expf_exact(((float)s[c] / fhw) * p.scale - lb, expf_exact_tab);
        __syncthreads();
        den = e[0];
        for (int c = 1; c < C; c++) den += e[c]; // left to right; every lane the same
    }
    if (lane < p.top_k) {
        int my = -1;
#pragma unroll
        for (int k = 0; k < MHIP_CLS_MAX_TOPK; k++) my = lane == k ? cls[k] : my;
        cls_t r;
        r.cls = my;
        r.score = 0.0f;
        if (my >= 0) r.score = p.softmax ? e[my] / den : ((float)s[my] / fhw) * p.scale;
        ((cls_t *)p.top)[(size_t)f * p.top_k + lane] = r;
    }
}

__global__ __launch_bounds__(256) void cls_label_fill_kernel(cls_t *labels, const size_t n) {
    cls_t none;
    none.cls = -1;
    none.score = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) labels[i] = none;
}

__global__ __launch_bounds__(256) void cls_label_scatter_kernel(const roi_t *rois, const int *n_out, const int slots, const cls_t *top, const int top_k,
                                                                cls_t *labels, const int det_frames, const int det_cap) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= slots || k >= n_out[0]) return;
    const roi_t r = rois[k];
    if (r.frame < 0 || r.frame >= det_frames || r.det < 0 || r.det >= det_cap) return; // (a caller's box: det = -1)
    labels[(size_t)r.frame * det_cap + r.det] = top[(size_t)k * top_k];
}

// ---- launchers
struct cls_plan_t { int planes, vec, groups, tpr, tiles; };

// the form that reads such a tensor; false = a layout these kernels do not read
static bool cls_plan(const mhip_classify_t *p, cls_plan_t *q) {
    if (!p || p->c < 1 || p->c > MHIP_CLS_MAX_C || p->hw < 1 || p->hw > (1 << 24) || p->frames < 1 || p->frames > 65535) return false;
    q->planes = 0; q->vec = 1; q->groups = p->c; q->tpr = q->tiles = 1;
    if (p->ch_step == 1 && (p->hw == 1 || p->pix_step >= p->c)) {
        if (p->row_room < p->c) return false;
        // V bytes per load: every load aligned, and the last group's load inside the bytes that belong to the row
        const uintptr_t al = (uintptr_t)p->base | (uintptr_t)p->frame_stride | (uintptr_t)(p->hw == 1 ? 0 : p->pix_step);
        for (int v = 16; v > 1; v >>= 2)
            if ((al & (uintptr_t)(v - 1)) == 0 && ((p->c + v - 1) / v) * v <= p->row_room) { q->vec = v; break; }
        q->groups = (p->c + q->vec - 1) / q->vec;
        q->tpr = q->groups < 256 ? q->groups : 256;
        q->tiles = (q->groups + q->tpr - 1) / q->tpr;
        return true;
    }
    if (p->pix_step == 1 && p->ch_step == p->hw) {
        q->planes = 1;
        return true;
    }
    return false;
}

#define CLS_WANT_WGS 2048 // 8 workgroups of 4 waves per CU

extern "C" int mhip_classify_split(const mhip_classify_t *p) {
    cls_plan_t q;
    if (!cls_plan(p, &q)) return 0;
    long long wgs, most;
    if (q.planes) {
        wgs = (long long)p->frames * ((p->c + 3) / 4);
        most = p->hw / 4096; // a part of a plane: 4 KB at least
    } else {
        wgs = (long long)p->frames * q.tiles;
        most = p->hw / ((256 / q.tpr) * 8); // a part of the pixels: 8 steps of the workgroup at least
    }
    long long n = (CLS_WANT_WGS + wgs - 1) / wgs;
    n = n < most ? n : most;
    return (int)(n < 1 ? 1 : n > 256 ? 256 : n);
}

extern "C" int mhip_classify(const mhip_classify_t *p) {
    cls_plan_t q;
    if (!cls_plan(p, &q) || !p->base || !p->partial || !p->sums || !p->top || p->top_k < 1 || p->top_k > MHIP_CLS_MAX_TOPK || p->nsplit < 1 ||
        p->nsplit > 256 || !(p->scale > 0.0f))
        return -1;
    hipStream_t st = mhip_stream_native();
    if (q.planes) {
        const int quads = (p->c + 3) / 4;
        const int seg = (((p->hw + p->nsplit - 1) / p->nsplit) + 15) & ~15;
        hipLaunchKernelGGL(cls_pool_planes_kernel, dim3((unsigned)(quads * p->nsplit), (unsigned)p->frames), dim3(256), 0, st, *p, quads, seg);
    } else {
        const int pps = (p->hw + p->nsplit - 1) / p->nsplit;
        const dim3 g((unsigned)(q.tiles * p->nsplit), (unsigned)p->frames);
        if (q.vec == 16) hipLaunchKernelGGL(cls_pool_rows_kernel<16>, g, dim3(256), 0, st, *p, q.groups, q.tpr, q.tiles, pps);
        else if (q.vec == 4) hipLaunchKernelGGL(cls_pool_rows_kernel<4>, g, dim3(256), 0, st, *p, q.groups, q.tpr, q.tiles, pps);
        else hipLaunchKernelGGL(cls_pool_rows_kernel<1>, g, dim3(256), 0, st, *p, q.groups, q.tpr, q.tiles, pps);
    }
    hipLaunchKernelGGL(cls_finish_kernel, dim3((unsigned)p->frames), dim3(64), 0, st, *p);
    return mhip_check(hipGetLastError(), "classify");
}

extern "C" int mhip_label_scatter(const void *rois, const int *n_out, int slots, const void *top, int top_k, void *labels, int det_frames, int det_cap) {
    if (!rois || !n_out || !top || !labels || slots < 1 || top_k < 1 || top_k > MHIP_CLS_MAX_TOPK || det_frames < 1 || det_cap < 1) return -1;
    const size_t n = (size_t)det_frames * det_cap;
    const unsigned fill = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipStream_t st = mhip_stream_native();
    hipLaunchKernelGGL(cls_label_fill_kernel, dim3(fill), dim3(256), 0, st, (cls_t *)labels, n);
    hipLaunchKernelGGL(cls_label_scatter_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, (const roi_t *)rois, n_out, slots,
                       (const cls_t *)top, top_k, (cls_t *)labels, det_frames, det_cap);
    return mhip_check(hipGetLastError(), "label scatter");
}
