// conv_f32_common.hpp -- what the float convolution translation units share (conv_f32.hip, conv_f32_split.hip, conv_f32_patch.hip,
// conv_f32_stem.hip, conv_f32_vcat.hip): the SiLU forms, exact division, the bf16 piece rules of both sides (host packers, device
// splits), the record format's pairing, the three piece products, barriers, the weight stage and the diagnostic stamp.  Every rule
// has its one definition and its one explanation here; the kernel files say what they do with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../expf_exact.h"
#include "../mhip.h"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// ---- diagnostic builds (tools/stamps_build.sh splitstamps | fpatch; read with tools/split_stamps.py / tools/fpatch_stamps.py): where a K
// step goes.  STAMP(i) adds the cycles since the previous stamp to the kernel's st_acc[i]; the shipped library compiles none of it.
#if defined(SPLIT_STAMPS) || defined(FPATCH_STAMPS)
#define STAMP(i)                                                                  \
    do {                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                        \
        const unsigned long long t_ = __builtin_readcyclecounter();              \
        st_acc[i] += t_ - st_last;                                                \
        st_last = t_;                                                             \
        __builtin_amdgcn_sched_barrier(0);                                        \
    } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// ---- SiLU
// fused SiLU as the exporter writes it (conv -> SIGMOID -> MUL, reference mars_runtime.c:742-749 and :807-816 float forms):
// s = 1.0f / (1.0f + expf(-v)); out = v * s -- every step rounded as the reference rounds it, expf as this image's libm
// (expf_exact.h), so folding the two element-wise layers into the convolution's epilogue changes no bit.  The exact-order and
// f32-MFMA kernels and the six-product mode of conv_f32_split use it.
__device__ __forceinline__ float silu_exact(float v) {
    const float s = 1.0f / (1.0f + expf_exact(-v, expf_exact_tab));
    return v * s;
}
// three piece products (relative error per product up to 2^-16) do not need libm's last bit: v_exp_f32 and v_rcp_f32, 1 ulp each --
// the exact form above is double-precision arithmetic and a table, a fifth of the kernel's time on every layer
// v / (1 + e) as (v / 2) * rcp((1 + e) / 2): v_rcp_f32 returns 0 where its result would be a denormal, i.e. for 1 + e > 2^126 (v <
// -87.34, a true value of up to 1.0e-36 came out as -0); halved, the operand stays below 2^127 until v = -88.03, where the true value
// is 5.2e-37.  No larger factor: v / 2 is exact down to |v| = 2^-125 and the product never exceeds |v|, so nothing changes at tiny or
// huge v (a factor 2^-32 made v 2^-32 a denormal below |v| = 2^-94 and lost its bits).  The fma rounds once, like the addition it replaces.
__device__ __forceinline__ float silu_fast(float v) {
    const float e = __builtin_amdgcn_exp2f(v * -1.44269504088896341f); // exp(-v)
    return (v * 0.5f) * __builtin_amdgcn_rcpf(__builtin_fmaf(e, 0.5f, 0.5f));
}

// ---- exact unsigned division by a run-time constant (magic number, one multiply-high): kernel index arithmetic, and the same
// arithmetic on the host for the geometry code that emulates it
struct fdiv_t {
    unsigned m, s1, s2;
};
__host__ __device__ __forceinline__ unsigned fdiv(unsigned n, const fdiv_t d) {
#ifdef __HIP_DEVICE_COMPILE__
    const unsigned q = __umulhi(d.m, n);
#else
    const unsigned q = (unsigned)(((unsigned long long)d.m * n) >> 32);
#endif
    return (q + ((n - q) >> d.s1)) >> d.s2;
}
static inline fdiv_t make_fdiv(unsigned d) {
    fdiv_t r;
    unsigned l = 0;
    while ((1ull << l) < d) l++;
    r.m = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    r.s1 = l < 1 ? l : 1;
    r.s2 = l > 0 ? l - 1 : 0;
    return r;
}

// ---- bf16 pieces, scalar: round to nearest even (a NaN stays one) and the value back.  The host packers cut weights with these
// (hi = bf16(x); mid = bf16(x - hi) where hi is finite, exact), conv_f32_vcat_head cuts its few results, and mars_hip_write_tensor
// (host/mars_run.c, C: its own copy of this rule) cuts records.
__host__ __device__ __forceinline__ uint16_t bf16_rn(float x) {
    const uint32_t b = __builtin_bit_cast(uint32_t, x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((b >> 16) | 0x40u);
    return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}
__host__ __device__ __forceinline__ float bf16_val(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

// ---- bf16 pieces, in the kernels: N floats -> N bf16 in each plane (N / 2 dwords each; v_cvt_pk_bf16_f32 converts and packs two at a
// time, element 2i in the low half), round-to-nearest split: hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid.  Every subtraction is
// exact (x - hi has at most 16 significant bits, x - hi - mid at most 8, a bf16 value), so x == hi + mid + lo exactly; with two planes
// |x - hi - mid| <= 2^-17 |x|, errors of either sign.
// A value bf16 would round to +-inf (x = +-inf, or |x| >= 2^128 - 2^119) keeps a FINITE hi and the LAST plane carries the infinity: the
// last plane of the input meets only the weights' hi plane (mid * hi, lo * hi), so the sum sees inf * w.hi once and gives sign(w) * inf
// as the reference does.  With the infinity in the hi plane it also met w.mid and w.lo -- inf * 0, or inf times a residual of the other
// sign -- and inf - inf as its own residual: NaN.  FLT_MAX still comes out as inf (hi + mid = 2^128).  A NaN ends as a NaN piece.
// Two forms of that rule, and who uses which:
//   split2<N>       two planes; hi saturates at the largest bf16 by one v_med3_f32 per element, the residual is then +-inf by itself.
//                   The staging phases that split once per tile (conv_f32_patch, conv_f32_stem) and conv_f32_stem's record output.
//   splitn<N, NPL>  conv_f32_split, whose split sits in the K loop.  Two planes: hi saturates by two packed 16-bit minima per PAIR of
//                   elements (cheaper there than two med3).  Three planes (not the benchmark's mode): hi = mid = 0 and lo = bf16(x).
// On every finite or infinite input the two two-plane forms give the same pieces (clamping before the rounding or the rounded bits
// after it: the same hi); they are two instruction sequences, not two rules.
template <int N>
__device__ __forceinline__ void split2(const float (&x)[N], int (&hi)[N / 2], int (&mid)[N / 2]) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
        const f32x2 v = {x[2 * i], x[2 * i + 1]};
        const f32x2 vh = {__builtin_amdgcn_fmed3f(v[0], -0x1.fep+127f, 0x1.fep+127f), __builtin_amdgcn_fmed3f(v[1], -0x1.fep+127f, 0x1.fep+127f)};
        const int h = __builtin_bit_cast(int, __builtin_convertvector(vh, bf16x2));
        const float h0 = __int_as_float(h << 16), h1 = __int_as_float(h & (int)0xffff0000);
        f32x2 r; // two plain subtractions (left to itself the compiler packs them into a v_pk_add_f32 behind two register moves)
        asm("v_sub_f32 %0, %1, %2" : "=v"(r[0]) : "v"(v[0]), "v"(h0));
        asm("v_sub_f32 %0, %1, %2" : "=v"(r[1]) : "v"(v[1]), "v"(h1));
        hi[i] = h;
        mid[i] = __builtin_bit_cast(int, __builtin_convertvector(r, bf16x2));
    }
}
#define NONFINITE_BF16 0x1.ffp+127f // 2^128 - 2^119: from here on bf16 rounding gives inf
template <int N, int NPL>
__device__ __forceinline__ void splitn(const float (&x)[N], int (&hi)[N / 2], int (&mid)[N / 2], int (&lo)[N / 2]) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) { // (element 2i, element 2i + 1) -> one dword per plane, element 2i in the low half
        const f32x2 v = {x[2 * i], x[2 * i + 1]};
        const bool f0 = __builtin_fabsf(v[0]) < NONFINITE_BF16, f1 = __builtin_fabsf(v[1]) < NONFINITE_BF16; // (false for a NaN; NPL == 3 only)
        const f32x2 vh = {NPL == 3 && !f0 ? 0.0f : v[0], NPL == 3 && !f1 ? 0.0f : v[1]};
        int h = __builtin_bit_cast(int, __builtin_convertvector(vh, bf16x2));
        if (NPL == 2) { // saturate both halves at once: +inf / +NaN (0x7f80 ..) -> 0x7f7f as signed, -inf / -NaN (0xff80 ..) -> 0xff7f as unsigned
            h = __builtin_bit_cast(int, __builtin_elementwise_min(__builtin_bit_cast(s16x2, h), (s16x2){0x7f7f, 0x7f7f}));
            h = __builtin_bit_cast(int, __builtin_elementwise_min(__builtin_bit_cast(u16x2, h), (u16x2){0xff7f, 0xff7f}));
        }
        const f32x2 hf = {__int_as_float(h << 16), __int_as_float(h & (int)0xffff0000)};
        const f32x2 r = v - hf; // (+-inf: itself)
        hi[i] = h;
        if (NPL == 3) {
            const f32x2 rm = {f0 ? r[0] : 0.0f, f1 ? r[1] : 0.0f};
            const int m = __builtin_bit_cast(int, __builtin_convertvector(rm, bf16x2));
            const f32x2 mf = {__int_as_float(m << 16), __int_as_float(m & (int)0xffff0000)};
            mid[i] = m;
            lo[i] = __builtin_bit_cast(int, __builtin_convertvector(r - mf, bf16x2)); // exact
        } else {
            mid[i] = __builtin_bit_cast(int, __builtin_convertvector(r, bf16x2));
            lo[i] = 0;
        }
    }
}

// ---- the three piece products of a two-piece product on v_mfma_f32_16x16x32_bf16, smallest terms first: mid * hi, hi * mid, hi * hi
// (relative error per product <= 2^-16).  WA false: the PIXELS are the MFMA's A operand (D = X W^T), a lane ends with 4 consecutive
// pixels of one channel row -- one 16-byte store into an NCHW map.  WA true: the weights are A (D = W X^T), a lane ends with 4
// consecutive CHANNELS of one pixel -- what a record holds (record_half).
template <bool WA>
__device__ __forceinline__ void mfma3_tile(v4f &acc, const bf16x8 xh, const bf16x8 xm, const bf16x8 wh, const bf16x8 wm) {
    if (WA) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wh, acc, 0, 0, 0); // mid * hi
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wm, acc, 0, 0, 0); // hi * mid
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh, acc, 0, 0, 0); // hi * hi
    }
}
// ... over a wave's MI x NI tiles: acc[a][c] += W tile a (wh, wm: MI channel tiles) x X tile c (xh, xm: NI pixel tiles)
template <int MI, int NI, bool WA = false>
__device__ __forceinline__ void mfma3(v4f (&acc)[MI][NI], const bf16x8 (&xh)[NI], const bf16x8 (&xm)[NI], const bf16x8 (&wh)[MI], const bf16x8 (&wm)[MI]) {
#pragma unroll
    for (int a = 0; a < MI; a++)
#pragma unroll
        for (int c = 0; c < NI; c++) mfma3_tile<WA>(acc[a][c], xh[c], xm[c], wh[a], wm[a]);
}

// ---- barriers between K-step phases.  barrier_lds: this wave's LDS operations done (loads in flight stay in flight), then the barrier.
// NOT __syncthreads(): that waits vmcnt(0) as well, i.e. for global loads issued a moment ago for a later step -- a full memory
// latency per K step.  barrier_raw: the barrier alone, fenced for the scheduler.
__device__ __forceinline__ void barrier_lds() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void barrier_raw() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- weight tile of a K step in LDS: rows of 64 bytes (32 bf16 taps), the row's four 16-byte chunks swizzled so that the fragment
// reads (16 rows x one chunk per lane group) spread over the banks -- the int8 kernels' A layout
__device__ __forceinline__ int a_lds_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 1) & 2)) << 4); }
// ... staged through registers: thread = AE (8 | 4 | 2) consecutive taps of one row of every plane, AE / 2 dwords.  wstage_fetch: both
// planes (hi, mid) of step ks by buffer loads -- a 32-bit per-lane offset `voff` (row, tap), the (plane, step) part in the scalar
// offset: no 64-bit row pointer and address arithmetic per load.  wstage_commit: NPL planes into the stage at `st` (planes APLANE bytes
// apart), row `arow`, taps akc .. + AE - 1.
template <int AE>
__device__ __forceinline__ void wstage_fetch(const __amdgpu_buffer_rsrc_t wrs, const unsigned voff, const unsigned wplane, const int ks, int (&areg)[2][AE / 2]) {
    constexpr int AD = AE / 2;
#pragma unroll
    for (int pl = 0; pl < 2; pl++) {
        const unsigned so = (unsigned)pl * wplane + (unsigned)ks * 64u;
        if (AE == 8) { const v4i t = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrs, voff, so, 0)); areg[pl][0] = t[0]; areg[pl][1 % AD] = t[1]; areg[pl][2 % AD] = t[2]; areg[pl][3 % AD] = t[3]; }
        else if (AE == 4) { const auto t = __builtin_amdgcn_raw_buffer_load_b64(wrs, voff, so, 0); areg[pl][0] = (int)t[0]; areg[pl][1 % AD] = (int)t[1]; }
        else areg[pl][0] = (int)__builtin_amdgcn_raw_buffer_load_b32(wrs, voff, so, 0);
    }
}
template <int AE, int APLANE, int NPL = 2>
__device__ __forceinline__ void wstage_commit(int8_t *st, const int arow, const int akc, const int (&areg)[NPL][AE / 2]) {
    constexpr int AD = AE / 2;
    const int aoff = a_lds_off(arow, akc >> 3) + (akc & 7) * 2; // AE bf16 = AE * 2 bytes inside the 16-byte chunk
#pragma unroll
    for (int pl = 0; pl < NPL; pl++) {
        if (AE == 8) *(v4i *)(st + pl * APLANE + aoff) = (v4i){areg[pl][0], areg[pl][1 % AD], areg[pl][2 % AD], areg[pl][3 % AD]};
        else if (AE == 4) *(int2 *)(st + pl * APLANE + aoff) = make_int2(areg[pl][0], areg[pl][1 % AD]);
        else *(int *)(st + pl * APLANE + aoff) = areg[pl][0];
    }
}

// ---- record format (mhip_conv_f32_t.out_rec / in_rec): [C / 8][H][W] x 32 bytes = [8 x bf16 hi | 8 x bf16 mid] of 8 consecutive
// channels of one pixel, written for the one k x k convolution that reads the tensor (conv_f32_prec / conv_f32_patch<RECIN>: its
// staging phase is then a plain copy).  record_half: a lane of a WA accumulator tile holds channels 4 fc .. + 3 (fc = lane / 16) of
// one pixel, x[] = those four results (after the SiLU); they are split into two hi and two mid dwords, then v_permlane16_swap
// between lane rows fc, fc ^ 1 (every lane takes part: call it before any branch): the even row ends with the mid pieces of all 8
// channels of the record, the odd row with the hi pieces -- the 16 bytes the lane stores at the record's offset (fc & 1) ? 0 : 16,
// 32 contiguous bytes per pixel.  MED3 picks the split (above): conv_f32_stem's is split2, conv_f32_split's splitn<4, 2> -- an
// infinite result leaves either with a finite hi and the infinity in mid.
template <bool MED3>
__device__ __forceinline__ v4i record_half(const float (&x)[4]) {
    int hi[2], mid[2], lo_[2];
    if (MED3) split2<4>(x, hi, mid);
    else splitn<4, 2>(x, hi, mid, lo_);
    const auto s0 = __builtin_amdgcn_permlane16_swap((unsigned)mid[0], (unsigned)hi[0], false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap((unsigned)mid[1], (unsigned)hi[1], false, false);
    return (v4i){(int)s0[0], (int)s1[0], (int)s0[1], (int)s1[1]};
}

// ---- host: a one-frame mhip_conv_f32_t from a shape (square stride, equal pads): what the packers' geometry code takes
static inline void conv_f32_shape(mhip_conv_f32_t *p, int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w) {
    memset(p, 0, sizeof(*p));
    p->out_c = out_c; p->in_c = in_c; p->kh = kh; p->kw = kw; p->stride_h = p->stride_w = stride; p->pad_top = p->pad_left = pad;
    p->in_h = in_h; p->in_w = in_w; p->out_h = out_h; p->out_w = out_w;
    p->in_stride = (size_t)in_c * in_h * in_w * 4; p->out_stride = (size_t)out_c * out_h * out_w * 4; p->frames = 1;
}
