// nv12.hpp -- the integer BT.601 conversion of NV12 camera frames (include/mars_hip.h, "NV12 camera frames"), shared by the letterbox front-end
// (preproc.hip) and the ROI crops (roi.hip): one statement of the arithmetic, so that both write the same bytes.
#pragma once
#include <hip/hip_runtime.h>

struct nv12_coef_t {
    int cy, yoff, crv, cgu, cgv, cbu, vu;
};
__device__ __forceinline__ nv12_coef_t nv12_coef(const unsigned flags) {
    nv12_coef_t k;
    const bool full = flags & 1u; // MARS_NV12_FULL_RANGE
    k.cy = full ? 256 : 298; k.yoff = full ? 0 : 16;
    k.crv = full ? 359 : 409; k.cgu = full ? -88 : -100; k.cgv = full ? -183 : -208; k.cbu = full ? 454 : 516;
    k.vu = (flags >> 1) & 1u;     // MARS_NV12_VU
    return k;
}
// four pixels: yv = their Y bytes, cv = the two chroma pairs (bytes 0, 1: pixels 0, 1; bytes 2, 3: pixels 2, 3) -> rgb[pixel][channel], 0 .. 255
__device__ __forceinline__ void nv12_quad(const nv12_coef_t k, const unsigned yv, const unsigned cv, int rgb[4][3]) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int c0 = (int)((cv >> (16 * q)) & 255u), c1 = (int)((cv >> (16 * q + 8)) & 255u);
        const int d = (k.vu ? c1 : c0) - 128, e = (k.vu ? c0 : c1) - 128;
        const int rr = k.crv * e + 128, gg = k.cgu * d + k.cgv * e + 128, bb = k.cbu * d + 128;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int c = k.cy * ((int)((yv >> (8 * (2 * q + t))) & 255u) - k.yoff);
            rgb[2 * q + t][0] = min(max((c + rr) >> 8, 0), 255); // (>> of a negative int: arithmetic, i.e. floor)
            rgb[2 * q + t][1] = min(max((c + gg) >> 8, 0), 255);
            rgb[2 * q + t][2] = min(max((c + bb) >> 8, 0), 255);
        }
    }
}
