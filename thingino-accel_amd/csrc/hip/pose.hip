// pose.hip -- pose keypoints of YOLOv8-pose style heads on gfx950: for every selected detection of a frame, the K keypoints {x, y, v} its
// origin cell of the head's keypoint tensor holds, x = (((float)q_x * s) * 2 + gx) * stride (y alike), v = the host's sigmoid table at q_v.
//
// include/mars_hip.h ("Pose keypoints") states the arithmetic.  Two launches:
//   pose_select_kernel  one wavefront per frame walks the kept list 64 records at a time; a ballot prefix numbers the records with
//                       conf >= min_conf in list order until max_per_frame are taken (a function of the list alone: no atomics).  Each
//                       taken record's prediction index, as the detection tail kept it, is turned into (head, cell) with the heads'
//                       cell counts and stored as {det, head, cell}; the slots left over get {-1, -1, -1}.
//   pose_kpt_kernel     grid (slots x keypoints in blocks of 256, frames), one thread per (slot, keypoint).  A thread reads its slot's
//                       record, the D bytes of its keypoint at base + cell * pix_step + c * ch_step (pixel rows, planes and a channel slice
//                       of a concat are the same three numbers), decodes them with one rounding per operation, maps them through the
//                       letterbox if the boxes are mapped, and stores one 12-byte record: thread t of a frame writes record t, so a
//                       wavefront's stores are 768 contiguous bytes.  A thread of an unused slot stores zeros and reads nothing else.
// The stage moves little data (at most 256 frames x 256 slots x 32 keypoints); it is here because the origins are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define POSE_SEL_THREADS 64
#define POSE_THREADS 256

__global__ __launch_bounds__(POSE_SEL_THREADS) void pose_select_kernel(const mhip_pose_t p) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int M = p.max_per_frame;
    const det_t *dets = (const det_t *)p.dets + (size_t)f * p.det_cap;
    const int *pred = p.pred + (size_t)f * p.det_cap;
    pose_t *recs = (pose_t *)p.recs + (size_t)f * M;
    int n = p.counts[f];
    n = n < 0 ? 0 : n > p.det_cap ? p.det_cap : n;
    int taken = 0;
    for (int base = 0; base < n && taken < M; base += POSE_SEL_THREADS) {
        const int i = base + lane;
        float conf = 0.0f;
        if (i < n && !p.select_all) conf = dets[i].conf; // (select_all: dets may be NULL)
        const bool ok = i < n && (p.select_all || conf >= p.min_conf);
        const unsigned long long m = __ballot(ok);
        const int slot = taken + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && slot < M) {
            pose_t r = {i, -1, -1};
            int pr = pred[i]; // (never read beyond the count)
#pragma unroll
            for (int k = 0; k < 4; k++) // constant indices into the kernel arguments
                if (k < p.nheads && r.head < 0 && pr >= 0) {
                    if (pr < p.cells[k]) { r.head = k; r.cell = pr; }
                    else pr -= p.cells[k];
                }
            recs[slot] = r; // an index no head holds (the tail writes none): {det, -1, -1}, all-zero keypoints
        }
        taken += __popcll(m);
    }
    if (taken > M) taken = M;
    for (int slot = taken + lane; slot < M; slot += POSE_SEL_THREADS) recs[slot] = pose_t{-1, -1, -1};
}

__global__ __launch_bounds__(POSE_THREADS) void pose_kpt_kernel(const mhip_pose_t p) {
    const int f = blockIdx.y, t = blockIdx.x * POSE_THREADS + threadIdx.x;
    const int K = p.num_kpt, D = p.dim, M = p.max_per_frame;
    if (t >= M * K) return;
    const int slot = t / K, j = t - slot * K;
    const pose_t r = ((const pose_t *)p.recs)[(size_t)f * M + slot];
    kpt_t o = {0.0f, 0.0f, 0.0f};
    if (r.det >= 0 && r.head >= 0) {
        const int8_t *b = nullptr;
        size_t fs = 0;
        int pstep = 0, cstep = 0, W = 1, st = 0;
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (r.head == k) {
                b = p.kpt[k]; fs = p.kpt_frame_stride[k]; pstep = p.kpt_pix_step[k]; cstep = p.kpt_ch_step[k];
                W = p.w[k]; st = p.stride[k]; s = p.scale[k];
            }
        int gx, gy;
        if (p.grid) {
            const int *g = p.grid + ((size_t)f * p.det_cap + r.det) * 3;
            gx = g[0]; gy = g[1]; st = g[2];
        } else {
            gy = r.cell / W;
            gx = r.cell - gy * W;
        }
        const int8_t *q = b + (size_t)f * fs + (size_t)r.cell * pstep + (size_t)(D * j) * cstep;
        const int qx = q[0], qy = q[cstep];
        const float fst = (float)st;
        o.x = __fmul_rn(__fadd_rn(__fmul_rn(__fmul_rn((float)qx, s), 2.0f), (float)gx), fst);
        o.y = __fmul_rn(__fadd_rn(__fmul_rn(__fmul_rn((float)qy, s), 2.0f), (float)gy), fst);
        o.v = D == 3 ? p.vis[r.head * 256 + (int)q[2 * (size_t)cstep] + 128] : 1.0f;
        if (p.map) {
            o.x = __fmul_rn(__fsub_rn(o.x, (float)p.px), p.rx);
            o.y = __fmul_rn(__fsub_rn(o.y, (float)p.py), p.ry);
        }
    }
    ((kpt_t *)p.kpts)[(size_t)f * M * K + t] = o;
}

extern "C" int mhip_pose(const mhip_pose_t *p) {
    if (!p || p->nheads <= 0 || p->nheads > 4 || p->frames <= 0 || p->frames > 65535 || (!p->dets && !p->select_all) || !p->counts || !p->pred || !p->recs ||
        !p->kpts || p->det_cap <= 0 || p->num_kpt < 1 || p->num_kpt > MHIP_POSE_MAX_KPT || (p->dim != 2 && p->dim != 3) ||
        (p->dim == 3 && !p->vis) || p->max_per_frame < 1 || p->max_per_frame > MHIP_POSE_MAX_PER_FRAME)
        return -1;
    for (int k = 0; k < p->nheads; k++)
        if (!p->kpt[k] || p->cells[k] <= 0 || p->w[k] <= 0 || p->kpt_pix_step[k] <= 0 || p->kpt_ch_step[k] <= 0) return -1;
    hipLaunchKernelGGL(pose_select_kernel, dim3(p->frames), dim3(POSE_SEL_THREADS), 0, mhip_stream_native(), *p);
    int rc = mhip_check(hipGetLastError(), "keypoint selection");
    if (rc) return rc;
    const int work = p->max_per_frame * p->num_kpt;
    hipLaunchKernelGGL(pose_kpt_kernel, dim3((work + POSE_THREADS - 1) / POSE_THREADS, p->frames), dim3(POSE_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "keypoints");
}
