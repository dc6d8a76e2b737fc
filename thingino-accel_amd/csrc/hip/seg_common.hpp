// seg_common.hpp -- what the mask kernels of seg.hip and seg_native.hip share: the edge rule of the selection's rectangles and the 16-byte channel load.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef int sg_v4i __attribute__((ext_vector_type(4)));

// floorf / ceilf of v clamped to 0 .. hi BEFORE the conversion (the same integers as clamp((int)..., 0, hi) wherever that is defined; a
// value beyond the int range lands on the bound, a NaN on 0)
__device__ __forceinline__ int sg_edge(float v, int hi, bool up) {
    v = up ? ceilf(v) : floorf(v);
    return (int)fminf(fmaxf(v, 0.0f), (float)hi);
}

// the 16 bytes of channels kb .. kb + 15 (zero from nm on) of the pixel / cell whose channel 0 is at q
__device__ __forceinline__ sg_v4i sg_load16(const int8_t *q, const int kb, const int nm, const int ch_step) {
    sg_v4i v = {0, 0, 0, 0};
    if (kb >= nm) return v;
    if (ch_step == 1 && kb + 16 <= nm) {
        __builtin_memcpy(&v, q + kb, 16); // any alignment is served
        return v;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int c = kb + j;
        const int b = c < nm ? (int)q[(size_t)c * ch_step] & 255 : 0;
        v[j >> 2] |= b << (8 * (j & 3));
    }
    return v;
}
