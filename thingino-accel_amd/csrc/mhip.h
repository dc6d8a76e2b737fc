/*
 * mhip.h -- the thin C-ABI layer between the C host code (csrc/host) and the
 * HIP translation units (csrc/hip).  Plain pointers, sizes and small POD
 * structs only; no HIP types cross this boundary.  Every launcher enqueues on
 * the library's single stream and returns 0 or a negative hipError_t.
 *
 * Replaces, conceptually: ioctl/mmap device access (reference src/device.c),
 * NNDMA staging (reference src/nna_dma.c) and the MXUv3 kernels (reference
 * src/mars/mxu_conv.c, mxu_ops.c).
 */
#ifndef MHIP_H
#define MHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime */
int mhip_init(int device_hint);          /* 0 ok; <0: no device / wrong arch */
void mhip_shutdown(void);
int mhip_ready(void);
int mhip_device_info(int *cu_count, int *lds_bytes, int *gfx_version, size_t *hbm_bytes);
void *mhip_stream(void);
int mhip_sync(void);                    /* both streams */
void mhip_select_aux(int on);          /* launchers enqueue on the auxiliary stream while on */
void mhip_select_stream(int which);    /* ... or on: 0 main, 1 auxiliary, 2 upload, 3 download (pipelined I/O), 4 second compute */
int mhip_stream_wait(int which, void *ev); /* that stream waits for an event */
int mhip_event_sync(void *ev);         /* host waits for an event */
void *mhip_malloc(size_t bytes);         /* HBM */
void mhip_free(void *p);
void *mhip_host_alloc(size_t bytes);     /* pinned + device mapped */
void mhip_host_free(void *p);
int mhip_memset_async(void *dst, int value, size_t bytes);
int mhip_h2d_async(void *dst, const void *src, size_t bytes);
int mhip_d2h_async(void *dst, const void *src, size_t bytes);
int mhip_d2d_async(void *dst, const void *src, size_t bytes);
/* strided copies: `rows` rows of `row_bytes`, source/destination pitches */
int mhip_h2d_2d_async(void *dst, size_t dpitch, const void *src, size_t spitch, size_t row_bytes, size_t rows);
int mhip_d2h_2d_async(void *dst, size_t dpitch, const void *src, size_t spitch, size_t row_bytes, size_t rows);
/* event pairs for per-op timing */
void *mhip_event_create(void);
void *mhip_event_create_sync(void); /* ordering only (no timing): for stream -> stream hand-offs */
void mhip_event_destroy(void *ev);
int mhip_event_record(void *ev);
float mhip_event_elapsed_ms(void *start, void *stop); /* waits for stop */
const char *mhip_last_error(void);
/* capture the launches enqueued on the main stream between begin and end into an executable graph (NULL on failure) */
int mhip_graph_begin(void);
void *mhip_graph_end(int ok);
int mhip_graph_launch(void *exec);
void mhip_graph_destroy(void *exec);

/* ---- int8 convolution (conv_i8.hip) */
typedef struct {
    const int8_t *in;  size_t in_stride;   /* per-frame stride, bytes */
    int8_t *out;       size_t out_stride;
    const int8_t *w;   /* packed: [oc_pad][kh][row_pad], see mhip_conv_i8_pack_geom */
    const int32_t *bias; /* [oc_pad] or NULL */
    const uint8_t *lut;  /* 256-entry post-requant map (index q+128) or NULL */
    const uint8_t *lut2; /* optional 512-entry half-step form of `lut` (index trunc(2*acc*cs)+256, lower clamp folded in);
                            only valid when mhip_conv_i8_lut2_ok(cs): enables the 4-instruction requantisation */
    /* optional: a 1x1 stride-1 convolution with a fused SiLU table (in_c -> in_c channels) evaluated on the staged input
     * patch BEFORE this k x k convolution reads it (C3 bottleneck: cv2(cv1(x)), patch-staged kernel only):
     * packed weights [in_c][64], bias rows, half-step table, combined scale */
    const int8_t *pre_w;
    const int32_t *pre_bias;
    const uint8_t *pre_lut2;
    float pre_cs;
    const int8_t *w_rgb;        /* optional: the RGB stem's A operands in the layout conv_i8_rgb keeps in LDS
                                 * (mhip_conv_i8_rgb_pack); NULL = the kernel re-lays p.w itself, once per workgroup */
    const int8_t *w_rows;       /* optional: the weights as conv_i8_rows streams them (mhip_conv_i8_rows_pack): one 8 KB LDS
                                 * image per (channel tile, 64-channel chunk, tap); NULL = that launch variant is not offered */
    int frames;
    int in_h, in_w, in_c;       /* input as NHWC */
    int out_h, out_w, out_c;
    int kh, kw, stride_h, stride_w, pad_top, pad_left;
    int row_pad;                /* bytes per kernel row in the packed weights (multiple of 16) */
    int oc_pad;                 /* packed output channels (multiple of 16) */
    float cs;                   /* (in_scale*w_scale)/out_scale, evaluated on the host in f32 */
    int relu;                   /* clamp negative results to 0 (fused ReLU, byte semantics) */
    int out_nchw;               /* store [O][H][W] instead of [H][W][O] */
    int in_planar;              /* > 0 (small-channel stem only, in_c == 4): `in` is in_planar (<= 4) PLANES [c][in_h][in_w] per frame -- an NCHW-tagged graph's
                                   input as the reference holds it -- which conv_i8_smallc interleaves while it stages its patch (round 6: no relayout launch);
                                   mhip_conv_i8 returns -2 when that kernel does not take the shape (the caller relays the input and launches again) */
    int safe;                   /* host proved |acc*cs| < 2^31 and cs finite: skip the x86 overflow fix-up */
    int out_pix_stride;         /* NHWC only: bytes between consecutive output pixels (0 = out_c); with out_ch_off
                                   this writes straight into a channel slice of a wider tensor (zero-copy concat) */
    int out_ch_off;
    int variant;                /* 0 = default launch policy, else a code from mhip_conv_i8_variants() */
    /* virtual concatenation (1x1 convolutions): when nseg > 1 the input pixel's in_c channels are the
     * concatenation of nseg dense NHWC tensors; `in` is unused.  seg_c0 = first channel of a segment (unused
     * entries 0x7fffffff), every seg_c a multiple of 32.  See mhip_conv_i8_seg_ok(). */
    /* fused residual Add (ADD layer folded into this convolution's epilogue): `add` = the other operand, an int8
     * tensor with exactly the output's layout and frame stride (NULL = none); out = sat8(trunc((conv*add_s_conv +
     * other*add_s_other)*add_inv + 0.5f)).  Only the one-tile and patch-staged forms implement it. */
    const int8_t *add;
    float add_s_conv, add_s_other, add_inv;
    int nseg;
    const int8_t *seg_in[4];
    size_t seg_stride[4];
    int seg_c[4], seg_c0[4];
    int seg_up;                 /* bit k: segment k is read through a 2x2 nearest upsample (its tensor is out_h/2 x out_w/2) */
    /* optional: a 1x1 stride-1 convolution with a fused SiLU table evaluated on this convolution's RESULT tile while it is still
     * in registers (C3: cv3 over concat({this result, post_in}), patch-staged kernel only; out_c = c in {32, 64}, the 1x1 maps
     * 2c -> 2c channels).  The result of this convolution itself is NOT stored (`out` may be NULL; out_stride still is the frame
     * stride of `add`).  post_w = the image of mhip_conv_i8_post_pack (weights in the kernel's K and row order, then the bias rows);
     * post_in = the concat's second half, a dense NHWC tensor of c channels; post_out / post_out_* as out / out_* of the 1x1 */
    const int8_t *post_w;
    const uint8_t *post_lut2;
    float post_cs;
    const int8_t *post_in;  size_t post_in_stride;
    int8_t *post_out;       size_t post_out_stride;
    int post_out_pix_stride, post_out_ch_off;
    /* optional: TWO 1x1 stride-1 convolutions with fused SiLU tables (C3's cv1 and cv2, 64 -> 32 channels each) evaluated on this
     * convolution's RESULT tile while it is still in registers (patch-staged kernel only; out_c = oc_pad = 64, stride 1 or 2, no Add).
     * The result of this convolution itself is NOT stored (`out` may be NULL).  split_w = the image of mhip_conv_i8_split_pack (both
     * sides' weights in the kernel's row order, then the bias rows); side i has its own half-step table, combined scale and output:
     * a dense NHWC tensor of 32 channels */
    const int8_t *split_w;
    const uint8_t *split_lut2[2];
    float split_cs[2];
    int8_t *split_out[2];   size_t split_out_stride[2];
    /* optional, with split_w only: a THIRD 1x1 stride-1 convolution with a fused SiLU table (the bottleneck's m.cv1, 32 -> 32 channels) that
     * reads side chain_side - 1 (chain_side = 1 or 2, 0 = none), evaluated on that side's requantised tile row while it is still in
     * registers.  Both sides are stored as without it.  chain_w = the image of mhip_conv_i8_chain_pack; its own half-step table, combined
     * scale and output: a dense NHWC tensor of 32 channels */
    int chain_side;
    const int8_t *chain_w;
    const uint8_t *chain_lut2;
    float chain_cs;
    int8_t *chain_out;      size_t chain_out_stride;
} mhip_conv_i8_t;
/* can the convolution described by *p take the pair of 1x1s behind it (split_* fields) in its launch?  (geometry only, at some tile height) */
int mhip_conv_i8_split_ok(const mhip_conv_i8_t *p);
/* Bytes of, and (packed0, packed1, out != NULL) the content of, the pair's image: packed_i / bias_i = side i's packed weights
 * [oc_pad = 32][k64 = 64] and bias rows as every conv_i8 launch reads them (bias NULL = zeros).  64 rows x 64 bytes in the kernel's LDS
 * layout (chunk swizzle applied), K in natural order, then 64 bias rows; row side * 32 + s * 16 + g * 4 + r carries output channel
 * g * 8 + s * 4 + r of that side (mhip_conv_i8_split_row; tests) */
size_t mhip_conv_i8_split_pack(const int8_t *packed0, const int32_t *bias0, const int8_t *packed1, const int32_t *bias1, int8_t *out);
int mhip_conv_i8_split_row(int side, int oc);
/* Bytes of, and (packed, out != NULL) the content of, the chained 1x1's image (chain_* fields): packed / bias = its packed weights
 * [oc_pad = 32][k64 = 64] (input channels 0..31, then zeros) and bias rows as every conv_i8 launch reads them (bias NULL = zeros).
 * 32 rows x 64 bytes in the kernel's LDS layout (chunk swizzle applied), then 32 bias rows; row mhip_conv_i8_split_row(0, oc) carries
 * output channel oc; input channel c sits at K position (c >> 3) * 16 + (c & 7) -- a lane group's 8 bytes of one side, the upper 8 bytes
 * of its 16-byte chunk are zero (mhip_conv_i8_chain_k; tests) */
size_t mhip_conv_i8_chain_pack(const int8_t *packed, const int32_t *bias, int8_t *out);
int mhip_conv_i8_chain_k(int c);
/* can the convolution described by *p take a following 1x1 (post_* fields) in its launch?  (geometry only, at some tile height) */
int mhip_conv_i8_post_ok(const mhip_conv_i8_t *p);
/* Bytes of, and (packed, out != NULL) the content of, the 1x1's image for a fused launch of c = 32 / 64 channels: `packed` / `bias` = the
 * 1x1's packed weights [oc_pad = 2c][k64 = 2c] and bias rows as every conv_i8 launch reads them (bias NULL = zeros).  Weights: K steps of
 * 64 bytes x 2c rows x 64 bytes in the kernel's LDS layout (chunk swizzle applied); row s * 16 + g * 4 + r carries output channel
 * g * (2c / 4) + s * 4 + r; K order: c = 64 natural ({result, post_in}), c = 32 chunk g = [result 8g..8g+7 | post_in 8g..8g+7].
 * mhip_conv_i8_post_k / _row say where input channel k / output channel oc went (tests).  0 = not such a shape */
size_t mhip_conv_i8_post_pack(int c, const int8_t *packed, const int32_t *bias, int8_t *out);
int mhip_conv_i8_post_k(int c, int k);
int mhip_conv_i8_post_row(int c, int oc);
/* row of the packed weights / bias that holds output channel oc (channels are permuted so that a lane's
 * results are consecutive channels) */
int mhip_conv_i8_oc_row(int oc, int oc_pad);
/* Bytes of, and (out != NULL) the content of, conv_i8_rgb's LDS weight image for this geometry; 0 = not an RGB-stem shape
 * that kernel takes.  `packed` = the layer's packed weights [oc_pad][k64] (mars_pack_conv_i8, 4-byte taps). */
/* can the convolution described by *p take a preceding 1x1 (pre_* fields) in its launch?  (geometry only) */
int mhip_conv_i8_pre_ok(const mhip_conv_i8_t *p);
size_t mhip_conv_i8_rgb_pack(int in_c, int kh, int kw, int stride_h, int stride_w, int pad_left, int oc_pad, int k64,
                             const int8_t *packed, int8_t *out);
/* Bytes of, and (out != NULL) the content of, conv_i8_rows' weight image (deep 3x3 stride-1 layers); 0 = not a shape that
 * kernel takes (out_w = the map width, 0 = unknown / any) */
size_t mhip_conv_i8_rows_pack(int in_c, int kh, int kw, int stride_h, int stride_w, int oc_pad, int k64, int out_w,
                              const int8_t *packed, int8_t *out);
unsigned long mhip_conv_i8_rows_launches(void); /* launches of conv_i8_rows since load (diagnostic) */
/* is the float->int conversion of acc*cs provably in range for every int32 accumulator? */
int mhip_conv_i8_is_safe(float cs);
/* may the half-step LUT be used for this combined scale?  (no int32 accumulator may requantise to +-0x3EFFFFFF) */
int mhip_conv_i8_lut2_ok(float cs);
int mhip_conv_i8_tune(const char *key, int value); /* launch-policy knobs, see mars_hip_set_tuning */
int mhip_conv_i8_tune_get(const char *key, int *value);
/* launch variants that can run this layer (same bytes out, different speed), the default first; 0 if none */
int mhip_conv_i8_variants(const mhip_conv_i8_t *p, int *codes, int max);
/* the variant code mhip_conv_i8 runs *p with under p->variant, the "variant" knob and the default policy; 0 = the stem / generic
 * kernels serve the layer, -1 = no kernel takes it as described.  Pure host arithmetic: no device call, pointers may be dummies */
int mhip_conv_i8_code(const mhip_conv_i8_t *p);
/* can this (shape-only: pointers may be dummies) segmented convolution run?  frames/out_stride as they will be */
int mhip_conv_i8_seg_ok(const mhip_conv_i8_t *p);
/* two convolutions over the same input in one launch (the second's input reads hit L2); -2 = not eligible as a
 * pair (launch them separately), else the launch result */
int mhip_conv_i8_pair(const mhip_conv_i8_t *a, const mhip_conv_i8_t *b);
/* ... in ONE tile that carries both (conv_i8_persist<BOTH>): the input -- a never-materialised concat included -- is staged once
 * for both.  1x1, stride 1, both sides out_c = oc_pad = 64 with dense rows and a half-step table.  _both_ok: do shape and batch
 * allow it (pointers may be dummies; the sides' `out` must differ)?  _both: -2 = not eligible, else the launch result */
int mhip_conv_i8_both_ok(const mhip_conv_i8_t *a, const mhip_conv_i8_t *b);
int mhip_conv_i8_both(const mhip_conv_i8_t *a, const mhip_conv_i8_t *b);
/* ... and a 1x1 `d` from 64 to 64 channels (half-step table, dense rows, the layer's own packed weights and bias rows) that reads side
 * `side` - 1 (1 | 2) evaluated in that side's waves on the bytes they have just packed (conv_i8_persist<CHAIN>): d's launch and its read
 * of the side go.  elide: the side itself is not stored (its `out` is not touched and may be NULL) */
int mhip_conv_i8_both_chain_ok(const mhip_conv_i8_t *a, const mhip_conv_i8_t *b, const mhip_conv_i8_t *d, int side);
int mhip_conv_i8_both_chain(const mhip_conv_i8_t *a, const mhip_conv_i8_t *b, const mhip_conv_i8_t *d, int side, int elide);
/* does a layer with in_c bytes per pixel take the small-channel packing (every pixel widened to 4 bytes, 32-byte kernel rows)? */
int mhip_conv_i8_small_c(int in_c, int kw, int out_c);
/* packing geometry shared by host packer and kernel */
/* c_eff: bytes per input pixel in the packed K layout (4 in small-channel mode, else in_c) */
void mhip_conv_i8_pack_geom(int in_c, int kw, int out_c, int *row_pad, int *oc_pad, int *c_eff);
int mhip_conv_i8(const mhip_conv_i8_t *p);

/* ---- float32 convolution (conv_f32.hip): NCHW / OIHW, reference summation order */
typedef struct {
    const float *in;  size_t in_stride;
    float *out;       size_t out_stride;
    const float *w;   const float *bias;
    const void *w_split; /* optional: the weights cut into bf16 planes (mhip_conv_f32_split_pack): conv_f32_split needs it */
    const void *w_patch; /* optional: unit table, schedule and the weights' two bf16 planes in conv_f32_patch's K order
                            (mhip_conv_f32_patch_pack): k x k layers take that kernel under use_mfma == 3 when it is there */
    int frames;
    int in_h, in_w, in_c, out_h, out_w, out_c;
    int kh, kw, stride_h, stride_w, pad_top, pad_left;
    int silu;     /* fused conv -> SIGMOID -> MUL chain (float forms): out = v * (1 / (1 + expf(-v))), libm-exact expf */
    const float *add; size_t add_stride; /* optional fused residual Add (reference mars_runtime.c:807-816, the float ADD): out = result + add[same index],
                                            one float add after the SiLU -- the same float the separate layer computes */
    int use_mfma; /* 0: reference summation order, bit-identical; 1: implicit GEMM on v_mfma_f32_16x16x4_f32 (fused
                     rounding per tap: inside the 1e-4 tolerance of the float32 models, not bit-equal); 2: implicit GEMM on
                     v_mfma_f32_16x16x32_bf16 with every operand split into three bf16 pieces, six piece products per
                     product (conv_f32_split.hip: errors of the size of an f32 rounding); 3: the same with two pieces
                     and three piece products ("bf16x3": relative error per product <= 2^-16, same tolerance class) */
    int k_limit;  /* use_mfma >= 2 (conv_f32_split): input channels >= k_limit are known to be exact zeros in every frame (the planner proves it:
                     mars_plan.c zero_tail_f32 -- the reference's byte-wise CONCAT writes a quarter of a float tensor's bytes): the K loop stops
                     there.  Adding +-0 to an f32 accumulator changes nothing but the sign of a zero sum.  0 = no such knowledge */
    int k_limit_required; /* the planes from k_limit on are NOT zeros but memory the launch must not sum (`in` is a shifted view of another
                     tensor: mars_plan.c virtual_concat_f32): only a kernel that honours k_limit may run it -- the launch fails otherwise */
    int in_rec, out_rec; /* use_mfma == 3 only: the input (1: read by conv_f32_prec, 2: by conv_f32_patch's record-input form; mhip_conv_f32_patch_rec_form) / the
                            output is in RECORD format instead of NCHW floats -- [c / 8][h][w] records of
                            32 bytes = [8 x bf16 hi | 8 x bf16 mid] of 8 consecutive channels of one pixel (hi = bf16(x), mid = bf16(x - hi):
                            the two pieces conv_f32_patch cuts every input into anyway).  Same bytes per element; a tensor written by one
                            convolution for ONE k x k convolution to read (the planner pairs them: mars_plan.c rec_pairs).  in_rec needs
                            w_patch packed by mhip_conv_f32_patch_pack2(rec = 1) (conv_f32_prec); out_rec: conv_f32_split / conv_f32_stem,
                            no fused Add, out_c a multiple of 8 */
} mhip_conv_f32_t;
int mhip_conv_f32(const mhip_conv_f32_t *p);
/* the first pixels of a 1 x 1 convolution over a never-materialised byte-wise CONCAT of float maps (conv_f32_vcat.hip): p->in = the concat's LAST
 * input, p->k_limit = planes to sum, w_t = the weights of those planes transposed to [plane][out_c] (mhip_conv_f32_vcat_pack: bytes, and with w and out
 * the content); first[n_first] = its other inputs in order, run_floats = floats per concat run (shape[3] / 4).  Overwrites pixels
 * [0, n_first * run_floats) of every output plane (or their records: out_rec) */
size_t mhip_conv_f32_vcat_pack(int out_c, int in_c, int planes, const float *w, float *out);
int mhip_conv_f32_vcat_head(const mhip_conv_f32_t *p, const float *w_t, const float *const *first, const size_t *first_strides, int n_first, int run_floats);
/* two float convolutions over the same input in one launch (use_mfma >= 2, conv_f32_split: same geometry and channel count, no residual Add, no
 * record operands -- C3's cv1 + cv2): the second one's input reads hit L2; -2 = not eligible as a pair (launch them separately) */
int mhip_conv_f32_pair(const mhip_conv_f32_t *a, const mhip_conv_f32_t *b);
unsigned long mhip_conv_f32_pair_launches(void); /* paired launches since load (diagnostic) */
/* Bytes of, and (out != NULL) the content of, the weight image conv_f32_split reads: `planes` (2: hi, mid; 3: hi, mid, lo) planes of bf16
 * [oc_pad][k_pad] -- oc_pad = roundup128(out_c), k_pad = roundup64(K') + 64, zero filled -- with w = hi + mid + lo exactly
 * (hi = bf16(w), mid = bf16(w - hi), round to nearest; use_mfma == 3 reads the first two planes).  K' = in_c * kh * kw, or in_c * kh * (kw + 1) for stride_w == 2 with an odd kw (one zero column
 * appended to every kernel row: taps come in pairs there). */
size_t mhip_conv_f32_split_pack(int out_c, int in_c, int kh, int kw, int stride_w, int planes, const float *w, void *out);
unsigned long mhip_conv_f32_split_launches(void); /* launches of conv_f32_split since load (diagnostic) */
/* which gather form conv_f32_split takes for this shape (1 / 2: 16-byte gathers at stride 1 / 2; 0: a dword per tap), or -1: it declines the
 * shape whatever the batch (a weight image alone does not make a layer one it runs: the planner asks before it plans record output) */
int mhip_conv_f32_split_takes(int out_c, int in_c, int kh, int kw, int stride_h, int stride_w, int pad_left, int in_w, int out_w);
/* conv_f32_patch (conv_f32_patch.hip: the input patch of a pixel tile staged and split once, k x k layers with >= 8 taps, stride
 * 1 / 2, in_c a multiple of 8 and >= 32, map widths multiples of 4).  Bytes of, and (w, out != NULL) the content of, its image:
 * [nsteps][4] unit offsets, [nsteps] chunk schedule, two bf16 planes [oc_pad][kp] in its K order; 0 = not such a shape */
size_t mhip_conv_f32_patch_pack(int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w,
                                const float *w, void *out);
/* rec != 0: the image for record-format input (conv_f32_prec: DMA issue schedule, a ring of up to four slots) */
size_t mhip_conv_f32_patch_pack2(int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w,
                                 int rec, const float *w, void *out);
int mhip_conv_f32_patch_geom2(int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w,
                              int rec, int *outv, int cap);
unsigned long mhip_conv_f32_prec_launches(void); /* launches of conv_f32_prec (record-format input) since load */
unsigned long mhip_conv_f32_recin_launches(void); /* ... of conv_f32_patch's record-input form (two slots, through registers) */
/* which kernel reads this layer's input when it arrives as records: 0 none, 1 conv_f32_prec (pack the image with rec = 1), 2 conv_f32_patch's
 * record-input form (the plain image) */
int mhip_conv_f32_patch_rec_form(int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w);
/* the layer geometry that kernel derives, as ints (tests, tools): see conv_f32_patch.hip; returns the count, 0 = not such a shape */
int mhip_conv_f32_patch_geom(int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w,
                             int *outv, int cap);
unsigned long mhip_conv_f32_patch_launches(void); /* launches of conv_f32_patch since load (diagnostic) */
/* conv_f32_stem (conv_f32_stem.hip: the float twins' first layer -- in_c <= 4, out_c <= 32, even kernel width, stride 2, output maps
 * multiples of 16 x 32): bytes of, and (w, out != NULL) the content of, the weight image it loads into registers (two bf16 planes
 * [32][20 units][8]); 0 = not such a shape.  The image travels in mhip_conv_f32_t.w_patch like conv_f32_patch's (a shape is taken by at
 * most one of the two kernels). */
size_t mhip_conv_f32_stem_pack(int out_c, int in_c, int kh, int kw, int stride, int pad, int in_h, int in_w, int out_h, int out_w,
                               const float *w, void *out);
unsigned long mhip_conv_f32_stem_launches(void);
/* policy knob: 0 never the matrix cores, 1 (default) wherever the host proves it safe, 2 everywhere, 3 / 4 everywhere on the
 * bf16 matrix cores with operands split in two / three (three / six piece products).  set < 0 only
 * reads; returns the mode in force (first call reads MARS_HIP_F32_MFMA) */
int mhip_conv_f32_mode(int set);

/* ---- element-wise (eltwise.hip).  n = elements per frame. */
int mhip_lut_i8(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride, int frames,
                size_t n, const uint8_t *lut_dev);
int mhip_relu_bytes(int8_t *buf, size_t stride, int frames, size_t n);
/* out_run > 0: the result is written as pixels of out_run channels into a wider tensor:
 * element i goes to (i / out_run) * out_pix_stride + out_ch_off + i % out_run (zero-copy concat) */
int mhip_binary_i8(int is_mul, const int8_t *a, size_t a_stride, const int8_t *b, size_t b_stride,
                   int8_t *out, size_t out_stride, int frames, size_t n, float sa, float sb, float inv_so,
                   int out_run, int out_pix_stride, int out_ch_off);
int mhip_sigmoid_f32(const float *in, size_t in_stride, float *out, size_t out_stride, int frames, size_t n);
int mhip_binary_f32(int op /*0 add,1 mul,2 sub*/, const float *a, size_t a_stride, const float *b,
                    size_t b_stride, float *out, size_t out_stride, int frames, size_t n);
int mhip_relu_f32(const float *in, size_t in_stride, float *out, size_t out_stride, int frames,
                  size_t n, float alpha);
int mhip_batchnorm_i8(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride, int frames,
                      int n, int c, int hw, const float *s, const float *b, float in_scale, float out_scale);
int mhip_batchnorm_f32(const float *in, size_t in_stride, float *out, size_t out_stride, int frames,
                       int n, int c, int hw, const float *s, const float *b);

/* ---- data movement (move.hip); all int8-byte semantics, NHWC index math */
/* out_pix_stride (0 = ch) / out_ch_off: as for the conv */
int mhip_maxpool_i8(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride, int frames,
                    int in_h, int in_w, int ch, int out_h, int out_w, int kh, int kw, int sh, int sw,
                    int out_pix_stride, int out_ch_off);
/* n <= 3 chained stride-1 max-pools (same window, output size = input size, ch % 16 == 0, h*w*64 <= 60 KB of LDS):
 * stage i reads stage i-1's result and writes outs[i] */
int mhip_pool_chain_i8(const int8_t *in, size_t in_stride, int8_t *const *outs, const size_t *out_strides, int n,
                       int frames, int h, int w, int ch, int kh, int kw);
int mhip_unpad_rows(const void *src, void *dst, size_t rows, int width, int pitch); /* device -> device */
int mhip_concat_slice(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride, int frames,
                      int out_h, int out_w, int in_c, int out_c, int ch_off);
/* the reference's CONCAT on [1, C, H, W]-tagged tensors of equal H, W (runs of W bytes, input n shifted n rows down, the last input wins), with
 * every operand held pixels x channels on the device; channel counts multiples of 16, n <= 4 (move.hip: concat_nchwq_kernel) */
int mhip_concat_nchwq(const int8_t *const *ins, const size_t *in_strides, const int *in_c, int n, int8_t *out, size_t out_stride,
                      int frames, int out_c, int H, int W, int rows_only /* > 0: only the first rows_only map rows of the output */);
/* ... and its UPSAMPLE (quirk dims qih x qiw x qch -> qoh x qow x qch, factors sh / sw) and stride-1, same-size MAXPOOL (window kh channels x kw
 * map rows) on such tensors: Ci / Co / C multiples of 16 */
int mhip_upsample_nchwq(const int8_t *in, size_t in_stride, int Ci, int Hi, int Wi, int8_t *out, size_t out_stride, int Co, int Ho, int Wo,
                        int frames, int qih, int qiw, int qch, int qoh, int qow, int sh, int sw);
int mhip_maxpool_nchwq(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride, int frames, int C, int H, int W, int kh, int kw);
int mhip_upsample_i8(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride, int frames,
                     int in_h, int in_w, int ch, int out_h, int out_w, int scale_h, int scale_w,
                     int out_pix_stride, int out_ch_off);
/* [C][HW] -> [HW][c_pad] with zero channel padding (feeds the NHWC conv kernel) */
int mhip_nchw_to_nhwc_pad(const int8_t *in, size_t in_stride, int8_t *out, size_t out_stride,
                          int frames, int c, int hw, int c_pad);

/* ---- detection tails (yolo_tail.hip) */
typedef struct {
    const int8_t *pred[4]; size_t stride[4]; int npred[4];
    int pix_c[4], pix_stride[4]; /* pix_stride != 0: every pix_c prediction bytes sit at the start of a pix_stride-byte pixel row */
    const float *lut[4];   /* per segment, device: 3 x 256 floats: value[q], obj[q], den[q] */
    int mono[4];           /* value[q] is strictly increasing in q (finite scale > 0): the class argmax may compare bytes */
    int nseg;
    int frames;
    float nms_thresh;
    void *dets;            /* device [frames][1000] records of 24 bytes */
    int *counts;           /* device [frames] kept */
    int *raw_counts;       /* device [frames] candidates before NMS (or NULL) */
    int do_nms;
} mhip_detect_t;
int mhip_detect(const mhip_detect_t *p);
int mhip_nms_only(void *dets_dev, int *count_dev, int n, float thresh);
/* raw anchor-based YOLOv5 Detect heads (yolo_tail.hip: heads_decode_kernel), decoded in prediction order (head, anchor, gy, gx),
 * then the same sort + NMS as mhip_detect, then (map) the letterbox mapping x' = (x - px) * rx, w' = w * rx (y, h alike) */
typedef struct {
    const int8_t *base[4]; size_t frame_stride[4]; /* head k of frame f starts at base[k] + f * frame_stride[k] */
    int h[4], w[4], nc[4];  /* grid and classes: 3 * (5 + nc) channels */
    int pix_step[4], ch_step[4]; /* byte of (pixel p = gy * w + gx, channel c) = p * pix_step + c * ch_step */
    int stride[4];
    float anchors[4][3][2]; /* pixels */
    const float *sig;       /* device [head][256]: 1 / (1 + expf(-q * scale)) at q + 128, the head's own scale */
    int nheads, frames;
    float conf, nms_thresh;
    void *dets;             /* device [frames][1000] records of 24 bytes */
    int *counts;            /* device [frames] kept */
    int *raw_counts;        /* device [frames] candidates before NMS (or NULL) */
    int map, px, py;        /* map != 0: boxes mapped back through a letterbox at (px, py) with factors rx, ry */
    float rx, ry;
} mhip_heads_t;
int mhip_detect_heads(const mhip_heads_t *p);
/* raw anchor-free DFL heads (yolo_tail.hip: dfl_decode_kernel): per head a box tensor of 4 * reg_max channels and a class tensor of nc
 * channels on the same grid, decoded in prediction order (head, gy, gx); then sort + NMS and the letterbox mapping as mhip_detect_heads */
typedef struct {
    const int8_t *box[4], *cls[4]; size_t box_frame_stride[4], cls_frame_stride[4]; /* tensor X of head k, frame f: X[k] + f * X_frame_stride[k] */
    int h[4], w[4], nc[4];
    int box_pix_step[4], box_ch_step[4], cls_pix_step[4], cls_ch_step[4]; /* byte of (pixel p, channel c) = p * pix_step + c * ch_step */
    int stride[4];
    int reg_max;            /* bins per box side, 2 .. 32 */
    const float *tab;       /* device [head][512]: E[d] = expf(-(d * box scale)) at d = 0 .. 255, then 1 / (1 + expf(-q * class scale)) at 256 + q + 128 */
    int nheads, frames;
    float conf, nms_thresh;
    void *dets;             /* device [frames][1000] records of 24 bytes */
    int *counts;            /* device [frames] kept */
    int *raw_counts;        /* device [frames] candidates before NMS (or NULL) */
    int map, px, py;
    float rx, ry;
    /* optional, both or neither (NULL: nothing is written, nothing else changes): the origin of every record as a prediction index --
     * cells of the heads before its head + its cell.  cand_pred [frames][1000]: of candidate r as the decode wrote it (scratch of the
     * sort); kept_pred [frames][1000]: of kept record `slot` */
    int *cand_pred, *kept_pred;
    void *premap;           /* optional, looked at only with map != 0: device [frames][1000] records, the kept boxes BEFORE the letterbox mapping */
} mhip_dfl_heads_t;
int mhip_detect_dfl(const mhip_dfl_heads_t *p);

/* ---- camera frames, as every stage that reads or writes them takes them (host checks and launchers alike): fmt 0 = RGB [h][w][3], fmt 1 =
 * NV12 (MARS_HIP_CAMERA_* of include/mars_hip.h; mars_stage.c asserts the values), flags = MARS_NV12_* (bits 0 and 1), legal with NV12 only */
static inline int mhip_frame_format_ok(int fmt, unsigned flags) { return fmt == 0 ? flags == 0 : fmt == 1 && !(flags & ~3u); }
/* bytes of one w x h frame; 0: a non-positive size, or an odd one of an NV12 frame */
static inline size_t mhip_frame_bytes(int w, int h, int fmt) {
    if (w <= 0 || h <= 0 || (fmt && ((w | h) & 1))) return 0;
    return fmt ? (size_t)w * (size_t)h / 2 * 3 : (size_t)w * (size_t)h * 3;
}

/* ---- image front-end (preproc.hip): letterbox resize + (px - 128); tables from csrc/host/mars_preproc.c */
typedef struct {
    const uint8_t *rgb; size_t rgb_stride;   /* [frames][h][w][3] uint8 on the device (mhip_letterbox_nv12: [frames] NV12 frames) */
    int8_t *out;        size_t out_stride;   /* [frames] x (tw*th*3) int8: [th][tw][3] (nhwc) or [3][th][tw] */
    int frames, w, h, tw, th, nhwc;
    int nw, nh, px, py;                      /* resized size and its offset inside the target */
    const int *xstart, *xsrc; const float *xw; /* gather lists of the horizontal / vertical pass (device) */
    const int *ystart, *ysrc; const float *yw;
    int max_cols, max_rows;                  /* largest source region (columns, rows) any 16 x 16 output tile touches; 0 = unknown */
    int n_xtaps;                             /* entries of the horizontal gather list (xstart[nw]); 0 = unknown: the strip form is not offered */
    int max_ytaps;                           /* longest vertical gather list of one output row (the strip form stages 8 of them in LDS); 0 = unknown */
    int form;                                /* 0: the launcher's choice (strips where they fit, else 16 x 16 tiles, else one thread per pixel); 1 / 2: tiles / per-pixel forced (tests) */
} mhip_letterbox_t;
int mhip_letterbox(const mhip_letterbox_t *p);
/* NV12 camera frames (Y plane [h][w], behind it the chroma plane [h/2][w/2][2]; w, h even; flags = MARS_NV12_* of include/mars_hip.h).
 * mhip_nv12_to_rgb: frames x NV12 -> frames x uint8 RGB [h][w][3] (strides in bytes between frames).
 * mhip_letterbox_nv12: mhip_letterbox with p->rgb / p->rgb_stride naming NV12 frames; the strip form converts while it stages a source row,
 * every other form converts into `scratch` (frames x w * h * 3 bytes on the device) first; mhip_letterbox_nv12_fused says which (1: no scratch needed) */
int mhip_nv12_to_rgb(const uint8_t *nv12, size_t nv12_stride, uint8_t *rgb, size_t rgb_stride, int frames, int w, int h, unsigned flags);
int mhip_letterbox_nv12_fused(const mhip_letterbox_t *p);
int mhip_letterbox_nv12(const mhip_letterbox_t *p, unsigned flags, uint8_t *scratch);

/* ---- ROI crops (roi.hip): boxes -> source rectangles -> bilinear crops into a second model's input; include/mars_hip.h "ROI crops" states
 * the arithmetic.  Every pointer is device memory.  Geometry travels through device memory: the select / rectangle kernels write `rois`
 * ([slots] records of 24 bytes: frame, det, x0, y0, x1, y1) and `n_out` ([0] kept, [1] dropped), the crop kernel reads them */
typedef struct {
    const uint8_t *frames; size_t frame_stride; /* [n_frames] RGB [h][w][3] (fmt 0) or NV12 (fmt 1) frames */
    int n_frames, w, h, fmt;
    unsigned nv12_flags;                        /* MARS_NV12_* */
    const void *dets; const int *counts; int det_cap; /* mhip_roi_select: [n_frames][det_cap] records of 24 bytes + [n_frames] list lengths */
    const void *boxes; const int *frame_of_box; int n_boxes; /* mhip_roi_rects: the caller's boxes, box i -> slot i */
    float expand, min_conf;                     /* resolved: expand > 0 */
    int min_size, cls_first, cls_count, max_per_frame; /* resolved: min_size >= 1 */
    int keep_aspect;
    int8_t *out; size_t out_stride;             /* [slots] x (tw * th * 3) int8: [th][tw][3] (nhwc) or [3][th][tw] */
    int slots, tw, th, nhwc;
    void *rois; int *n_out;
    int *frame_kept;                            /* mhip_roi_select: scratch, [n_frames] */
    const float *csn;                           /* the mhip_roi_rot_* calls only ("Rotated crops"): dets / boxes hold records of 32 bytes (mars_obb_t)
                                                 * and csn the (cos, sin) pair of every one of them, index-aligned */
    int area;                                   /* mhip_roi_crop only: box-filter the down-scaled axes ("Area averaging"); needs mhip_roi_area_fits */
    /* the mhip_roi_align_* calls only ("Aligned crops"); at the end: the other calls' fields keep their places */
    void *fits;                                 /* [slots] records of 32 bytes (mars_align_t): written by select / rects, read by the crop */
    const void *pose_recs, *pose_kpts;          /* mhip_roi_align_select: [n_frames][pose_max] records of 12 bytes and [n_frames][pose_max][num_kpt]
                                                 * keypoints of 12 bytes, as mhip_pose leaves them; mhip_roi_align_rects: `boxes` = [n_boxes][num_kpt] keypoints */
    int pose_max, num_kpt;                      /* num_kpt: 1 .. 32 */
    unsigned use;                               /* resolved: a non-empty mask below 1 << num_kpt */
    float min_vis;
    float tmpl[32][2];                          /* the template, target pixels */
} mhip_roi_t;
int mhip_roi_select(const mhip_roi_t *p); /* the selection rules over the detection lists, frame-major, list order; two launches */
int mhip_roi_rects(const mhip_roi_t *p);  /* the rectangle rule alone: slot i = box i (x1 == x0: skipped), n_out = {n_boxes, 0} */
int mhip_roi_crop(const mhip_roi_t *p);   /* slots >= n_out[0], skipped slots and pad bands are filled with -17 */
int mhip_roi_fits(int w, int tw, int fmt); /* 1: the crop kernel's LDS holds two source rows of such frames and a strip of such a target */
int mhip_roi_area_fits(int w, int tw, int fmt); /* 1: the area kernel takes such a target (<= 1280 wide) and its LDS holds one source row of such frames beside it */
/* the same three over oriented boxes: the skip rule of "Rotated crops" in the rectangle rule's place, x0 .. y1 = the enclosing rectangle (for the
 * caller only), and a crop kernel that reads box (frame, det) of dets -- box `slot` of boxes where det < 0 -- and samples along its axes */
int mhip_roi_rot_select(const mhip_roi_t *p);
int mhip_roi_rot_rects(const mhip_roi_t *p);
int mhip_roi_rot_crop(const mhip_roi_t *p);
int mhip_roi_rot_fits(int w, int h, int tw); /* 1: positions of such frames fit the Q16 integers and a strip of such a target fits the LDS */
/* the same three for "Aligned crops": the lists are pose slots (select: slot order, det == -1 ends a frame's list, the slot's detection
 * passes min_conf and the class window) or a caller's keypoint sets (rects); the least-squares fit of the template decides the skip and
 * gives the six Q16 integers, written beside the ROI entry into `fits` (skipped and empty slots: zeros); the crop kernel is the rotated
 * sampler reading its geometry from `fits`.  mhip_roi_rot_fits is the size check. */
int mhip_roi_align_select(const mhip_roi_t *p);
int mhip_roi_align_rects(const mhip_roi_t *p);
int mhip_roi_align_crop(const mhip_roi_t *p);

/* ---- second-stage labels (classify.hip): int8 feature maps -> per-channel int32 sums -> ranked top-K entries; include/mars_hip.h
 * "Second-stage labels" states the arithmetic.  Every pointer is device memory. */
#define MHIP_CLS_MAX_C 4096
#define MHIP_CLS_MAX_TOPK 8
typedef struct {
    const int8_t *base; size_t frame_stride; /* frame f starts at base + f * frame_stride */
    int frames, c, hw;
    int pix_step, ch_step;  /* byte of (pixel p, channel ch) = p * pix_step + ch * ch_step: planes (1, hw) or pixel rows (pitch, 1) */
    int row_room;           /* pixel rows: bytes from channel 0 to the end of its pixel row that belong to the buffer (>= c) */
    int nsplit;             /* parts a frame's pixels are cut into (mhip_classify_split) */
    int *partial;           /* [frames][nsplit][c]: written by the pooling launch, summed by the finishing one */
    int *sums;              /* [frames][c] */
    void *top;              /* [frames][top_k] records of 8 bytes {int cls, float score} */
    int top_k, softmax;
    float scale;
} mhip_classify_t;
int mhip_classify_split(const mhip_classify_t *p); /* the nsplit the launcher wants for such a tensor (>= 1; looks at the layout fields only); 0: not a layout it reads */
int mhip_classify(const mhip_classify_t *p); /* two launches: pool into `partial`, then sum, rank and score (one wavefront per frame) */
/* labels [det_frames][det_cap] records of 8 bytes: every entry {-1, 0}, then entry (roi.frame, roi.det) of crop k < min(n_out[0], slots) = top[k][0] */
int mhip_label_scatter(const void *rois, const int *n_out, int slots, const void *top, int top_k, void *labels, int det_frames, int det_cap);

/* ---- gallery match (gallery.hip): int32 embeddings -> int8 rows (the exact rule of include/mars_hip.h, "Gallery match") -> int8 MFMA dot
 * products against the gallery's rows -> ranked (key, row) lists -> {id, score} entries.  Every pointer is device memory. */
#define MHIP_MATCH_MAX_C 4096
#define MHIP_MATCH_KEEP 8           /* entries of a partial list: MHIP_CLS_MAX_TOPK, whatever top_k asks for */
#define MHIP_MATCH_MAX_ROWS (1 << 24)
typedef struct {
    const int *vec;         /* [queries][c] int32 embeddings */
    int queries, c, cp;     /* cp = c rounded up to a multiple of 64: the pitch of every int8 row */
    int8_t *q;              /* [queries rounded up to 64][cp]: the quantised queries, pad channels and pad rows zero */
    int *qq; float *qinv;   /* [queries]; qq == 0: a null query */
    const int8_t *rows; const float *ginv; const int *ids; /* the gallery: [rows][cp], [rows], [rows]; rows and ginv are READ up to n_rows
                                                            * rounded up to 16: the arrays are that long (mars_gallery.c allocates multiples of 64) */
    int n_rows, chunk;      /* chunk = mhip_match_chunk(n_rows) */
    unsigned long long *part; /* [queries][chunks][MHIP_MATCH_KEEP] rank words (gallery.hip: gm_ord), chunks = ceil(n_rows / chunk): written by
                               * the match launch, read by the merge */
    void *top; int *top_row; /* [queries][top_k] records of 8 bytes {int id, float score}, and the row index of each (-1: empty) */
    int top_k;
    float min_score;        /* 0: no threshold */
} mhip_match_t;
int mhip_match_chunk(int n_rows); /* gallery rows per workgroup the launcher wants for such a gallery (a multiple of 64; a function of n_rows alone); 0: n_rows out of range */
int mhip_match(const mhip_match_t *p); /* three launches: quantise, match (one partial list per query and chunk), merge */
/* (the identity scatter is mhip_label_scatter of classify.hip with another source and destination) */

/* ---- tracking (track.hip): detection lists of `frames` frames -> a track id per detection, by the exact rule of include/mars_hip.h
 * ("Tracking").  One workgroup per stream walks that stream's `steps` frames in order with the stream's table on chip.  Every pointer is
 * device memory. */
#define MHIP_TRACK_SLOTS 256
#define MHIP_TRACK_CAND 256
typedef struct { long long counters[4]; int next_id, pad; } mhip_track_hdr_t; /* births, deaths, overflow, dropped; the id the next birth gets - 1 */
typedef struct {
    int streams, steps;     /* frames = streams * steps */
    int max_det;            /* row length of dets, idents and out: 1 .. 1000 */
    int stream_major;       /* frame of (stream b, step t): b * steps + t; otherwise t * streams + b */
    const void *dets;       /* [frames][max_det] records of 24 bytes {float x, y, w, h, conf; int cls} */
    const int *counts;      /* [frames]; clamped to 0 .. max_det */
    const void *idents;     /* [frames][max_det] records of 8 bytes {int cls, float score}, or NULL: no identity is carried */
    void *out;              /* [frames][max_det] records of 8 bytes {int id, hits} */
    void *states;           /* [streams][MHIP_TRACK_SLOTS] records of 48 bytes (mars_track_state_t); hits == 0: a free slot */
    mhip_track_hdr_t *hdr;  /* [streams] */
    float min_conf, low_conf, iou, iou_low; /* resolved: low_conf == 0 means no second pass, the others are never 0 */
    int max_miss, cls_first, cls_count, any_class;
} mhip_track_t;
int mhip_track(const mhip_track_t *p); /* one launch */

/* ---- appearance in tracking (track_app.hip): the same walk on a tracker that holds an int8 embedding per slot, by the exact rule of
 * include/mars_hip.h ("Appearance in tracking").  Both kernels take records, table, scans, compaction and rounds from hip/track_core.hpp;
 * mhip_track's kernel has none of what the plane adds.  Per stream and step the cosines of the 256 slots against the high set's candidates
 * are computed on the int8 matrix unit into `cosm`, twice (slot-major and candidate-major: the two halves of the workgroup walk it along
 * different axes), and pass 1 reads them.  Every pointer is device memory. */
#define MHIP_TRACK_APP_MAX_C 4096
#define MHIP_TRACK_APP_COS_FLOATS (2 * MHIP_TRACK_SLOTS * MHIP_TRACK_CAND) /* per stream of a launch: 512 KB */
#define MHIP_TRACK_APP_CHUNK 512    /* streams per launch: the launcher walks the streams in chunks over ONE block of at most 256 MB */
typedef struct {
    mhip_track_t t;         /* the lists, the tables and the resolved options, as for mhip_track */
    int c, cp;              /* channels; cp = c rounded up to a multiple of 64: the pitch of every int8 row */
    int8_t *plane;          /* [streams][MHIP_TRACK_SLOTS][cp]: the slots' embeddings, pad channels zero, a slot without one all zero */
    int *plane_ee;          /* [streams][MHIP_TRACK_SLOTS]; 0: the slot has none */
    const int *vec;         /* [n_vec][c] int32 embeddings of this call's detections, or NULL with n_vec == 0 */
    int n_vec;
    int8_t *q; int *qq;     /* [n_vec][cp], [n_vec]: written by the quantise launch (the rule of gallery.hip); NULL with n_vec == 0 */
    const int *emb_index;   /* [frames][max_det]: detection (f, i) uses row emb_index[f][i]; outside 0 .. n_vec - 1: none.  NULL: none has one */
    float *cosm;            /* [min(streams, MHIP_TRACK_APP_CHUNK)][MHIP_TRACK_APP_COS_FLOATS]; NULL only where emb_index is NULL */
    float app_thresh, app_min_iou; /* resolved: never 0 */
    int smooth;
} mhip_track_app_t;
int mhip_track_app(const mhip_track_app_t *p); /* the quantise launch (n_vec > 0), then one launch per chunk of streams */
/* emb_index [det_frames][det_cap]: every entry -1, then entry (roi.frame, roi.det) of crop k < min(n_out[0], slots) = k */
int mhip_track_app_index(const void *rois, const int *n_out, int slots, int *emb_index, int det_frames, int det_cap);
/* test hook: plane [256][cp] / plane_ee [256] against the quantised vec [nc][c] -> out [nt][nc], the slot-major matrix of the kernel's own
 * routine; *bad (device) is raised where the candidate-major copy differs from it.  q, qq as above; cosm: MHIP_TRACK_APP_COS_FLOATS floats */
int mhip_track_app_matrix(const int8_t *plane, const int *plane_ee, const int *vec, int nt, int nc, int c, int cp, int8_t *q, int *qq, float *cosm,
                          float *out, int *bad);

/* ---- instance masks (seg.hip): kept detections + their prediction indices -> per frame up to max_per_frame records and bit masks at the
 * prototype tensor's size, by the exact rule of include/mars_hip.h ("Instance masks").  Every pointer is device memory.  Two launches: the
 * selection (records, rectangles), then the masks (int8 MFMA of the selected cells' coefficient rows against the prototype pixels). */
#define MHIP_SEG_MAX_PER_FRAME 64
#define MHIP_SEG_MAX_NM 64
typedef struct {
    const int8_t *coef[4]; size_t coef_frame_stride[4]; /* coefficient tensor of head k, frame f: coef[k] + f * coef_frame_stride[k] */
    int coef_pix_step[4], coef_ch_step[4];              /* byte of (cell p, channel c) = p * pix_step + c * ch_step */
    int cells[4];                                       /* h * w of head k: prediction index = cells of the heads before + cell */
    float scale[4];                                     /* coefficient scale of head k * prototype scale, one float32 product */
    int nheads;
    const int8_t *proto; size_t proto_frame_stride; int proto_pix_step, proto_ch_step;
    int nm, ph, pw, in_w, in_h;
    int frames;
    const void *boxes;      /* [frames][det_cap] records of 24 bytes, graph-input pixels */
    const int *counts;      /* [frames] list lengths (clamped to 0 .. det_cap) */
    const int *pred;        /* [frames][det_cap] prediction index of every listed record */
    int det_cap;
    float logit_min, min_conf;
    int select_all;         /* != 0: every listed record is taken whatever its confidence (the host-pointer form) */
    int max_per_frame;      /* 1 .. MHIP_SEG_MAX_PER_FRAME */
    void *recs;             /* [frames][max_per_frame] records of 24 bytes {det, x0, y0, x1, y1, area} */
    uint32_t *words;        /* [frames][max_per_frame][ph][(pw + 31) / 32] */
} mhip_seg_t;
int mhip_seg(const mhip_seg_t *p);
int mhip_seg_select(const mhip_seg_t *p); /* the selection launch alone; p is not checked */

/* ---- instance masks in frame pixels (seg_native.hip): the same lists, tensors and selection, the masks on an out_w x out_h grid by the
 * exact rule of include/mars_hip.h ("Instance masks in frame pixels").  Two launches: the selection of seg.hip with the output grid in the
 * prototype size's place, then one workgroup per (span of 64 rows, slot, frame), walked in tiles of 16 rows x 8 words. */
#define MHIP_SEGN_MAX_OUT 8192
typedef struct {
    mhip_seg_t seg;         /* as mhip_seg takes it, but: in_w / in_h = the BASE grid the boxes are in, scale[k] = the product scale * 2^-16,
                             * words = [frames][max_per_frame][out_h][(out_w + 31) / 32]; ph / pw stay the prototype tensor's */
    int out_w, out_h;       /* 1 .. MHIP_SEGN_MAX_OUT */
    const int *taps;        /* [ia][ib][w1] of out_w ints each, then the same of out_h for the rows (mars_yolo_mask_taps): up-scaling tables,
                             * ia <= ib <= ia + 1, non-decreasing, inside the prototype tensor */
} mhip_seg_native_t;
int mhip_seg_native(const mhip_seg_native_t *p);

/* ---- pose keypoints (pose.hip): kept detections + their prediction indices -> per frame up to max_per_frame records {det, head, cell} and K
 * keypoints {x, y, v} each, gathered from the origin cell of the heads' keypoint tensors by the exact rule of include/mars_hip.h ("Pose
 * keypoints").  Every pointer is device memory.  Two launches: the selection (records), then the gather + decode. */
#define MHIP_POSE_MAX_PER_FRAME 256
#define MHIP_POSE_MAX_KPT 32
typedef struct {
    const int8_t *kpt[4]; size_t kpt_frame_stride[4]; /* keypoint tensor of head k, frame f: kpt[k] + f * kpt_frame_stride[k] */
    int kpt_pix_step[4], kpt_ch_step[4];              /* byte of (cell p, channel c) = p * pix_step + c * ch_step */
    int cells[4], w[4], stride[4];                    /* h * w, grid width and stride of head k: prediction index = cells of the heads before + cell */
    float scale[4];                                   /* keypoint scale of head k */
    int nheads;
    const float *vis;       /* [nheads][256] visibility of byte q at [q + 128] (the host's 1 / (1 + expf(-q * scale))); looked at only with dim == 3 */
    int num_kpt, dim;       /* K: 1 .. MHIP_POSE_MAX_KPT; D: 2 or 3 */
    int frames;
    const void *dets;       /* [frames][det_cap] records of 24 bytes: only conf is read (select_all: may be NULL) */
    const int *counts;      /* [frames] list lengths (clamped to 0 .. det_cap) */
    const int *pred;        /* [frames][det_cap] prediction index of every listed record */
    const int *grid;        /* NULL, or [frames][det_cap][3] = (gx, gy, stride) of listed record i in place of its cell's (the host-pointer form) */
    int det_cap;
    float min_conf;
    int select_all;         /* != 0: every listed record is taken whatever its confidence (the host-pointer form) */
    int max_per_frame;      /* 1 .. MHIP_POSE_MAX_PER_FRAME */
    int map, px, py;        /* map != 0: x' = (x - px) * rx, y' = (y - py) * ry */
    float rx, ry;
    void *recs;             /* [frames][max_per_frame] records of 12 bytes {det, head, cell} */
    void *kpts;             /* [frames][max_per_frame][num_kpt] records of 12 bytes {x, y, v} */
} mhip_pose_t;
int mhip_pose(const mhip_pose_t *p);

/* ---- oriented boxes (obb.hip): the DFL heads plus a 1-channel angle tensor per head -> rotated candidates, then sort + ProbIoU suppression
 * by the exact rule of include/mars_hip.h ("Oriented boxes").  Every pointer is device memory.  Records are 32 bytes {x, y, w, h, conf, cls,
 * angle, pred}.  mhip_obb: the decode, then the sort + suppression.  mhip_obb_nms: the sort + suppression alone on cand / csn / cand_counts
 * as a caller filled them (ang, box, cls, tab are not looked at). */
typedef struct {
    const int8_t *box[4], *cls[4], *ang[4]; size_t box_frame_stride[4], cls_frame_stride[4], ang_frame_stride[4];
    int h[4], w[4], nc[4];
    int box_pix_step[4], box_ch_step[4], cls_pix_step[4], cls_ch_step[4], ang_pix_step[4]; /* byte of (pixel p, channel c) = p * pix_step + c * ch_step */
    int stride[4];
    int reg_max;            /* bins per box side, 2 .. 32 */
    const float *tab;       /* [head][512]: mhip_dfl_heads_t.tab */
    const float *atab;      /* [head][768]: ang[q], cs[q], sn[q] at q + 128, + 256, + 512 */
    int nheads, frames;
    float conf;
    float e_thresh;         /* E = (float)(1 - (1 - T)^2) */
    int agnostic;           /* != 0: every pair is evaluated, whatever the classes */
    void *cand;             /* [frames][1000] records: the candidates in prediction order; the sort leaves them in sorted order */
    float *csn;             /* [frames][1000][2]: cos, sin of every candidate's angle (permuted with the records) */
    int *cand_counts;       /* [frames] candidates (the decode writes it; clamped to 0 .. 1000) */
    void *out;              /* [frames][1000] records: the kept boxes, mapped */
    float *csn_out;         /* NULL, or [frames][1000][2]: cos, sin of every kept box, index-aligned with out (the rotated crops read them) */
    int *out_counts;        /* [frames] kept */
    void *dets;             /* NULL, or [frames][1000] records of 24 bytes: the enclosing upright rectangles, index-aligned with out */
    int *counts;            /* NULL, or [frames] kept (the detection list's) */
    int *raw_counts;        /* NULL, or [frames] candidates before NMS */
    int map, px, py;        /* map != 0: x' = (x - px) * rx, y' = (y - py) * ry, w' = w * rx, h' = h * rx */
    float rx, ry;
} mhip_obb_t;
int mhip_obb(const mhip_obb_t *p);
int mhip_obb_nms(const mhip_obb_t *p);

/* ---- tiled inference (tile.hip): the tile table -> the ROI table the crop kernel of roi.hip reads (tile t of camera frame c = slot c * T + t);
 * T per-tile detection lists -> one list per camera frame in camera pixels, by the exact rule of include/mars_hip.h ("Tiled inference").
 * The table travels by value in the launch record (at most 64 tiles); every pointer is device memory. */
#define MHIP_TILE_MAX_TILES 64
#define MHIP_TILE_MAX_CAND 2048
typedef struct { int x0, y0, x1, y1; float px, py, rx, ry; } mhip_tile_geom_t; /* the rectangle; (float)px, (float)py and the factors of the map */
typedef struct {
    mhip_tile_geom_t tiles[MHIP_TILE_MAX_TILES];
    int n_tiles, cams;      /* T, C: model frames = C * T */
    int src_w, src_h;
    int max_det;            /* row length of dets: 1 .. 1000 */
    int quota;              /* entries a tile contributes: n_tiles * quota <= MHIP_TILE_MAX_CAND */
    int ios, agnostic;
    float thresh, edge_margin; /* edge_margin == 0: no edge rule */
    const void *dets;       /* [C * T][max_det] records of 24 bytes {float x, y, w, h, conf; int cls} */
    const int *counts;      /* [C * T]; clamped to 0 .. max_det */
    void *out;              /* [C][1000] records of 24 bytes; slots behind the last survivor are zeroed */
    int *out_counts;        /* [C] */
    void *origins;          /* [C][1000] records of 8 bytes {int tile, det} */
    void *stats;            /* [C] records of 24 bytes {candidates, overflow, invalid, edge, suppressed, truncated} */
    void *rois; int *n_out; /* mhip_tile_rois: [C * T] records of 24 bytes (mhip_roi_t.rois) and {C * T, 0} (mhip_roi_t.n_out) */
} mhip_tile_t;
int mhip_tile_rois(const mhip_tile_t *p);  /* one launch: the ROI table of C camera frames */
int mhip_tile_merge(const mhip_tile_t *p); /* one launch, one workgroup per camera frame */

/* ---- redaction (redact.hip): detections -> per frame a table of regions {x0, y0, x1, y1, mask slot or -1} -> the frames with the union of
 * the regions mosaicked or filled, by the exact rule of include/mars_hip.h ("Redaction").  Every pointer is device memory.  Two launches:
 * mhip_redact_select (one workgroup per frame: the selection, the rectangle rule of "ROI crops", the table, the counts), then mhip_redact
 * (one workgroup per 64 x 64 pixel tile and frame; it adds the frame's `pixels`). */
#define MHIP_REDACT_MAX_DIM 8192
typedef struct {
    const uint8_t *frames; uint8_t *dst;        /* [n_frames] RGB [h][w][3] (fmt 0) or NV12 (fmt 1) frames; dst == frames: in place, else a second such buffer */
    size_t frame_stride;
    int n_frames, w, h, fmt;
    unsigned nv12_flags;                        /* MARS_NV12_* (only VU matters: the fill colour's order) */
    const void *dets; const int *counts;        /* frame f's list: counts[f] records of 24 bytes from record list_off[f] on (list_off == NULL: */
    const int *list_off; int det_cap;           /* f * det_cap, and counts[f] is clamped to 0 .. det_cap) */
    int select_all;                             /* != 0: every listed record is selected (the host-pointer form) */
    float expand, min_conf, ident_min;          /* resolved: expand > 0 */
    int cls_first, cls_count;
    const void *idents;                         /* NULL, or records of 8 bytes {cls, score} index-aligned with dets: cls >= 0 and score >= ident_min spares */
    const void *mask_recs; int mask_max;        /* NULL, or [n_frames][mask_max] records of 24 bytes whose det field names a list index: that
                                                 * detection's mask is slot f * mask_max + j; mask_max <= 64 */
    const int *mask_of;                         /* NULL, or a slot (or < 0: none) per record, index-aligned with dets (the host-pointer form) */
    const uint32_t *mask_words;                 /* [slot][h][(w + 31) / 32] */
    int mode, cell_log2;                        /* 0 mosaic, 1 fill; cell = 1 << cell_log2: 2 .. 64 */
    unsigned char fill[3];
    int *table;                                 /* 5 ints per record, at the place of the frame's list: the first table_n[f] of them are regions */
    int *table_n;                               /* [n_frames] */
    int *stats;                                 /* [n_frames][4]: regions, masked, skipped, pixels */
} mhip_redact_t;
int mhip_redact_select(const mhip_redact_t *p);
int mhip_redact(const mhip_redact_t *p);

/* ---- overlay (overlay.hip): detections, track ids, masks and keypoints -> the frames with boxes, labels, tints and markers painted in, by
 * the exact rule of include/mars_hip.h ("Overlay").  Every pointer is device memory.  Two launches: mhip_overlay_select (one workgroup per
 * frame: the selection, the rectangle rule, colours, label texts, mask and pose slots, the frame's element table and marker table, the
 * counts), then mhip_overlay (one workgroup per 64 x 64 pixel tile and frame; it adds the frame's `pixels`).
 * A colour is packed as c0 | c1 << 8 | c2 << 16 | white << 24: R, G, B, or Y and the chroma pair in its stored order -- the host converts,
 * the kernels are format-blind; white = the text on it is white, from the RGB colour. */
#define MHIP_OVERLAY_MAX_DIM 8192
#define MHIP_OVERLAY_MAX_KPT 32
#define MHIP_OVERLAY_REC_INTS 12 /* an element: x0, y0, x1, y1, mask slot or -1, colour | text length << 25, 24 text bytes */
#define MHIP_OVERLAY_MASKS 1u
#define MHIP_OVERLAY_BOXES 2u
#define MHIP_OVERLAY_KEYPOINTS 4u
#define MHIP_OVERLAY_LABELS 8u
typedef struct {
    const uint8_t *frames; uint8_t *dst;        /* as in mhip_redact_t */
    size_t frame_stride;
    int n_frames, w, h, fmt;
    const void *dets; const int *counts;        /* the lists, as in mhip_redact_t */
    const int *list_off; int det_cap;
    int select_all;                             /* != 0: every listed record is selected (the host-pointer form) */
    float min_conf;
    int cls_first, cls_count;
    const void *tracks;                         /* NULL, or records of 8 bytes {id, hits} index-aligned with dets */
    int tracked_only, min_hits;                 /* != 0: only records with id >= 0 and hits >= min_hits (resolved: >= 1) */
    int color_by;                               /* 0 class, 1 track id, 2 fixed */
    const int *keys;                            /* NULL, or the colour key of every record, index-aligned with dets: overrides color_by */
    unsigned text;                              /* MHIP_OVERLAY_TEXT_* of csrc/overlay_rule.h, resolved: not 0 */
    const char *texts;                          /* NULL, or [.][24] bytes index-aligned with dets: the label of a record, up to the first NUL */
    const char *names; int n_names;             /* NULL, or [n_names][16] */
    const void *mask_recs; int mask_max;        /* as in mhip_redact_t */
    const int *mask_of;
    const uint32_t *mask_words;
    const void *pose_recs; int pose_max;        /* NULL, or [n_frames][pose_max] records of 12 bytes whose det field names a list index: that
                                                 * detection's keypoints are row f * pose_max + j of kpts; pose_max <= 256 */
    int kpt_rows;                               /* != 0 (the host-pointer form): record i's keypoints are row i of kpts, index-aligned with dets */
    const void *kpts; int num_kpt;              /* [row][num_kpt] records of 12 bytes {x, y, v}; num_kpt 1 .. 32 */
    float kpt_min_v;                            /* resolved */
    unsigned layers;                            /* MHIP_OVERLAY_*, resolved: not 0 */
    int thick, radius, scale, alpha;            /* resolved: 1 .. 16, 1 .. 8, 1 .. 8, 1 .. 256 */
    const uint32_t *palette; int n_palette;     /* packed colours, 1 .. 256 of them */
    uint32_t no_key, text_col[2];               /* packed: the colour of a negative key; black and white */
    int *table;                                 /* MHIP_OVERLAY_REC_INTS per record, at the place of the frame's list: the first table_n[f] are elements */
    int *table_n;                               /* [n_frames] */
    int *marks;                                 /* 4 ints per marker {cx, cy, element * 32 + keypoint, 0}: frame f's from marker list_off[f] * */
    size_t mark_stride;                         /* num_kpt on (list_off != NULL), else from f * mark_stride on; in no order: the key orders them */
    int *marks_n;                               /* [n_frames] */
    int *stats;                                 /* [n_frames][6]: boxes, masked, labels, markers, skipped, pixels */
} mhip_overlay_t;
int mhip_overlay_select(const mhip_overlay_t *p);
int mhip_overlay(const mhip_overlay_t *p);

/* ---- motion maps (motion.hip): camera frames -> per frame a bit map of the grid cells whose mean luma left the stream's background, by the
 * exact rule of include/mars_hip.h ("Motion").  Every pointer is device memory.  Two launches per call: mhip_motion_cells (one workgroup
 * per 64 x 64 pixel tile and STREAM, which walks that stream's steps in order: cell means, the compare, the background update, one raw byte
 * per cell and the frames' `first`), then mhip_motion_map (one workgroup per frame: the neighbour filter, the packed words, the statistics,
 * the zone counts; it marks the frame's stream initialised).  mhip_motion_dets counts a box list's cells against the maps. */
#define MHIP_MOTION_MAX_DIM 8192
#define MHIP_MOTION_MAX_ZONES 64
typedef struct {
    const uint8_t *frames;                      /* [n_frames] RGB [h][w][3] (fmt 0) or NV12 (fmt 1: only the Y plane is read) */
    size_t frame_stride;
    int n_frames, streams, steps, stream_major; /* n_frames = streams * steps; frame of (stream s, step t) = stream_major ? s * steps + t : t * streams + s */
    int w, h, fmt, cell_log2, gw, gh, pitch;    /* cell = 1 << cell_log2: 4 .. 64; gw, gh = the grid; pitch = (gw + 31) / 32 words */
    int threshold, learn, learn_active;         /* resolved: 1 .. 255, 1 .. 16, 1 .. 16 */
    int min_neighbors, frame_diff;              /* 0 .. 8; != 0: bg = m after the comparison */
    uint16_t *bg;                               /* [streams][gh][gw] */
    int *init;                                  /* [streams]: != 0 once a step has run */
    uint8_t *raw;                               /* [n_frames][gh][32 * pitch]: scratch between the two launches, 16-byte aligned; cells >= gw are never written */
    uint32_t *maps;                             /* [n_frames][gh][pitch] */
    int *stats;                                 /* [n_frames][6]: active, x0, y0, x1, y1, first */
    int *zone_counts;                           /* [n_frames][n_zones]; may be NULL with n_zones == 0 */
    int n_zones;
    int zones[MHIP_MOTION_MAX_ZONES][4];        /* the zones' CELL ranges, inclusive: cx0, cy0, cx1, cy1, inside the grid */
} mhip_motion_t;
int mhip_motion_cells(const mhip_motion_t *p);
int mhip_motion_map(const mhip_motion_t *p);
typedef struct {
    const uint32_t *maps; int n_frames, gw, gh, pitch, cell_log2, w, h;
    const void *dets;       /* records of 24 bytes */
    const int *counts;      /* device form: [n_frames] list lengths, clamped to 0 .. det_cap; entry e is record e % det_cap of frame e / det_cap */
    int det_cap;
    const int *frame_of;    /* list form (counts == NULL): the frame of entry e; one that names no frame gives {0, 0} */
    int n_entries;          /* device form: n_frames * det_cap */
    float expand;           /* resolved: > 0 */
    void *out;              /* [n_entries] records of 8 bytes {active, cells} */
} mhip_motion_dets_t;
int mhip_motion_dets(const mhip_motion_dets_t *p);

/* ---- events (events.hip): detection lists and their track ids -> line crossings, zone entry, exit and dwell per detection, per frame and
 * per stream, by the exact rule of include/mars_hip.h ("Events").  One workgroup per stream walks that stream's `steps` frames in order;
 * thread s owns slot s of the stream's table.  Every pointer is device memory. */
#define MHIP_EVENTS_LINES 32
#define MHIP_EVENTS_ZONES 32
#define MHIP_EVENTS_VERTS 8
#define MHIP_EVENTS_TOTALS (2 * MHIP_EVENTS_LINES + 4 * MHIP_EVENTS_ZONES + 5)
/* a stream's rules as the kernel reads them: every coordinate already multiplied by 16 */
typedef struct {
    int n_lines, n_zones;
    int lines[MHIP_EVENTS_LINES][4];                                                    /* ax, ay, bx, by */
    struct { int n, dwell, x[MHIP_EVENTS_VERTS], y[MHIP_EVENTS_VERTS]; } zones[MHIP_EVENTS_ZONES];
} mhip_event_rules_t;
/* a stream's step counter and running totals: [line][in, out], [zone][entered, exited, dwelled, lost], first, expired, overflow, dropped,
 * duplicates */
typedef struct { int step, pad; long long tot[MHIP_EVENTS_TOTALS]; } mhip_events_hdr_t;
typedef struct {
    int streams, steps;     /* frames = streams * steps */
    int max_det;            /* row length of dets, tracks and records: 1 .. 1000 */
    int stream_major;       /* frame of (stream b, step t): b * steps + t; otherwise t * streams + b */
    const void *dets;       /* [frames][max_det] records of 24 bytes {float x, y, w, h, conf; int cls} */
    const void *tracks;     /* [frames][max_det] records of 8 bytes {int id, hits} */
    const int *counts;      /* [frames]; clamped to 0 .. max_det */
    void *records;          /* [frames][max_det] records of 24 bytes (mars_event_t) */
    int *line_counts;       /* [frames][MHIP_EVENTS_LINES][2] */
    int *zone_counts;       /* [frames][MHIP_EVENTS_ZONES][4] */
    void *slots;            /* [streams][MHIP_TRACK_SLOTS] records of 152 bytes (mars_event_slot_t); id == 0: a free slot */
    mhip_events_hdr_t *hdr; /* [streams] */
    const mhip_event_rules_t *rules; /* [streams] */
    int max_gap, min_hits;  /* resolved: >= 1 */
    int anchor_bottom;
} mhip_events_t;
int mhip_events(const mhip_events_t *p); /* one launch */

/* ---- best shots (shots.hip): the crops in a second model's input, their ROI table and the track ids -> a quality measure per crop and, per
 * stream, a table that keeps the best crop of every live track with its pixels, by the exact rule of include/mars_hip.h ("Best shots").
 * Three launches: the metrics of every crop (band partials), the walk (one workgroup per stream, its steps in order), the copy of each
 * slot's final winner into the plane.  Every pointer is device memory. */
#define MHIP_SHOTS_COUNTERS 6
#define MHIP_SHOTS_LDS 40960 /* bytes of staged rows and luma a metrics workgroup may hold: decides the band height */
/* a stream's step counter and counters: finished, lost, dropped, overflow, duplicates, taken */
typedef struct { int step, pad; long long cnt[MHIP_SHOTS_COUNTERS]; } mhip_shots_hdr_t;
typedef struct {
    int streams, steps;      /* frames = streams * steps */
    int slots;               /* table slots per stream: 1 .. MHIP_TRACK_SLOTS */
    int n_crops;             /* entries of crops, rois, partials, cand and records */
    int tw, th, nhwc;        /* a crop: tw * th * 3 int8, [th][tw][3] or [3][th][tw] */
    int band_rows, bands;    /* rows a metrics workgroup owns (mhip_shots_band_rows), and ceil(th / band_rows) */
    int stream_major, keep_aspect, inside, src_w, src_h;
    int max_gap, min_hits;   /* resolved: >= 1 */
    int min_mean, max_mean, min_sharp; /* min_mean == max_mean == 0: no window */
    const int8_t *crops;     /* crop k at crops + k * crop_stride */
    size_t crop_stride;
    const void *rois;        /* [n_crops] records of 24 bytes (mars_roi_t) */
    const int *kept;         /* the number of crops written, clamped to 0 .. n_crops; NULL: n_crops */
    /* det_cap == 0: one entry per crop.  det_cap > 0: lists of det_cap entries per frame, crop k's entry is [rois[k].frame][rois[k].det] */
    int det_cap;
    const float *confs;      /* det_cap == 0: [n_crops] */
    const int *cls;          /* det_cap == 0: [n_crops] */
    const void *dets;        /* det_cap > 0: [frames][det_cap] records of 24 bytes (mars_det_t) */
    const void *tracks;      /* [n_crops] or [frames][det_cap] records of 8 bytes {int id, hits} */
    long long *partials;     /* scratch: [n_crops][bands][2], the bands' sums of Y and of L * L */
    int *cand;               /* scratch: [n_crops], the id a crop brings as a candidate of its step, 0: none */
    void *records;           /* [n_crops] records of 24 bytes (mars_shot_t) */
    void *table;             /* [streams][slots] records of 72 bytes (mars_shot_slot_t) */
    mhip_shots_hdr_t *hdr;   /* [streams] */
    int8_t *plane;           /* [streams][slots] crops at a pitch of plane_stride bytes, in the crops' layout */
    size_t plane_stride;     /* a multiple of 16 */
    int *last;               /* [streams][slots]: the crop the walk stored last in that slot in this call, or -1 */
} mhip_shots_t;
static inline int mhip_shots_band_rows(int tw) { /* 16 rows, fewer where 4 bytes a pixel of band and halo rows would not fit */
    const int fit = MHIP_SHOTS_LDS / (tw * 4) - 2;
    return fit > 16 ? 16 : fit < 1 ? 1 : fit;
}
int mhip_shots(const mhip_shots_t *p); /* the three launches */

#ifdef __cplusplus
}
#endif
#endif
