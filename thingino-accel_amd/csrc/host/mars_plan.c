/*
 * mars_plan.c -- the launch planner of the .mars executor: one planner per layer kind (each cites the reference lines it
 * mirrors: src/mars/mars_runtime.c:511-1224), the host arithmetic they share, the parameter arena, and the fusion passes
 * (SiLU tables, residual Adds, virtual / zero-copy concats, paired launches, pool chains, the float32 policy).
 * Split out of mars_model.c in round 4; loader: mars_model.c, run paths: mars_run.c.
 * The passes ask who reads and writes a tensor through ONE layer of helpers (use-def helpers below), on the operand model stated at
 * mars_op_t (mars_internal.h) and checked by plan_check; the environment switches they obey are m->sw (plan_switches_t).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mars_internal.h"
#include "nna.h"

/* ------------------------------------------------------- host arithmetic */
int32_t mars_trunc_x86(float x) {
    /* x86 cvttss2si: out of range or NaN -> INT32_MIN */
    if (x >= -2147483648.0f && x < 2147483648.0f) return (int32_t)x;
    return INT32_MIN;
}
static int sat8(int32_t v) { return v > 127 ? 127 : (v < -128 ? -128 : v); }
static int q_half_up(float v) { return sat8(mars_trunc_x86(v + 0.5f)); }

size_t elem_size(uint32_t dtype) {
    switch (dtype) {
        case MARS_DTYPE_FLOAT32: case MARS_DTYPE_INT32: return 4;
        case MARS_DTYPE_INT16: return 2;
        default: return 1;
    }
}

size_t shape_numel(const mars_tensor_t *d) {
    size_t n = 1;
    for (uint32_t i = 0; i < d->ndims && i < MARS_MAX_DIMS; i++) {
        if (d->shape[i] <= 0) return 0;
        n *= (size_t)d->shape[i];
        if (n > MAX_DIM_PRODUCT) return 0;
    }
    return n;
}

/* Format-aware byte size of a tensor, reference mars_runtime.c:80-124 (`tensor_byte_size`): NDHWC32 rounds the
 * channel count (shape[1]) up to 32, NMHWSOIB2 counts 1024-byte blocks, UINT4 packs two elements per byte; every
 * other tag is numel * element size.  The reference evaluates the products in `int` and converts to size_t; the
 * same wrap-around is kept by computing in 32-bit unsigned arithmetic and sign-extending. */
size_t mars_hip_tensor_byte_size(const mars_tensor_t *t) {
    if (!t) return 0;
    size_t es;
    switch (t->dtype) {
        case MARS_DTYPE_FLOAT32: case MARS_DTYPE_INT32: es = 4; break;
        case MARS_DTYPE_INT16: es = 2; break;
        default: es = 1; break; /* INT8, UINT8, UINT4 (two per byte, handled below), unknown */
    }
    if (t->format == MARS_FORMAT_NDHWC32 && t->ndims >= 4) {
        const uint32_t n = (uint32_t)t->shape[0], h = (uint32_t)t->shape[2], w = (uint32_t)t->shape[3];
        const uint32_t d = (uint32_t)((int32_t)((uint32_t)t->shape[1] + 31u) / 32); /* the reference's int sum, wrapped without UB */
        return (size_t)(int32_t)(n * d * h * w * 32u) * es; /* int product, then * size_t (:101) */
    }
    if (t->format == MARS_FORMAT_NMHWSOIB2 && t->ndims >= 4) {
        const uint32_t no = (uint32_t)((int32_t)((uint32_t)t->shape[0] + 31u) / 32), mi = (uint32_t)((int32_t)((uint32_t)t->shape[1] + 31u) / 32);
        return (size_t)(int32_t)(no * mi * (uint32_t)t->shape[2] * (uint32_t)t->shape[3] * 1024u);
    }
    size_t numel = 1;
    for (uint32_t i = 0; i < t->ndims && i < MARS_MAX_DIMS; i++) numel *= (size_t)(int64_t)t->shape[i];
    if (t->dtype == MARS_DTYPE_UINT4) return (numel + 1) / 2;
    return numel * es;
}

/* What the reference reports as `alloc_size` of every activation tensor (mars_runtime.c:250-334): all of them share
 * working buffers of ONE size, the largest 64-byte-rounded tensor_byte_size of any activation -- or less when three,
 * then two such buffers do not fit behind the weights in its 8 MiB arena.  Callers fill / scan `alloc_size` bytes
 * through vaddr (mars_test.c:73-84, 117-127), so single-frame I/O tensors report the same number here and their
 * staging is at least that large.  Where the reference would refuse to load (weights > 8 MiB, < 64 KiB per buffer)
 * this build still loads and reports the unreduced size. */
size_t reference_buffer_size(const mars_model_ext_t *m) {
    size_t max_sz = 0;
    for (uint32_t i = 0; i < m->pub.header.num_tensors; i++) {
        const mars_tensor_t *d = &m->pub.tensors[i].desc;
        if (d->data_size != 0) continue;
        size_t sz = ALIGN_UP(mars_hip_tensor_byte_size(d), 64);
        if (sz > max_sz) max_sz = sz;
    }
    const size_t ddr = (size_t)8 << 20;
    if (m->pub.weights_size > ddr) return max_sz;
    const size_t remaining = ddr - m->pub.weights_size;
    if (max_sz * 3 <= remaining || max_sz * 2 <= remaining) return max_sz;
    const size_t reduced = (remaining / 2) & ~(size_t)63;
    return reduced >= 65536 ? reduced : max_sz;
}

/* --------------------------------------------------------- parameter arena */
size_t arena_reserve(mars_model_ext_t *m, size_t bytes) {
    /* any failure here fails the whole plan (build_plan returns plan_err): no op keeps an unset offset */
    if (bytes > ARENA_MAX || m->arena_size > ARENA_MAX) { m->plan_err = MARS_ERR_ALLOC_FAILED; return NO_OFF; }
    size_t off = ALIGN_UP(m->arena_size, 256);
    size_t end = off + ALIGN_UP(bytes ? bytes : 1, 256);
    if (end > ARENA_MAX) { m->plan_err = MARS_ERR_ALLOC_FAILED; return NO_OFF; }
    if (end > m->arena_cap) {
        size_t cap = m->arena_cap ? m->arena_cap : (1u << 20);
        while (cap < end) cap *= 2; /* end <= 2^40: cannot overflow */
        uint8_t *p = (uint8_t *)realloc(m->arena_host, cap);
        if (!p) { m->plan_err = MARS_ERR_ALLOC_FAILED; return NO_OFF; }
        memset(p + m->arena_cap, 0, cap - m->arena_cap);
        m->arena_host = p;
        m->arena_cap = cap;
    }
    m->arena_size = end;
    return off;
}

/* bytes [off, off+n) of the weight blob; beyond its end the blob reads as zeros */
void blob_read(const mars_model_ext_t *m, size_t off, size_t n, void *dst) {
    const uint8_t *blob = (const uint8_t *)m->pub.weights;
    size_t have = m->pub.weights_size;
    memset(dst, 0, n);
    if (!blob || off >= have) return;
    size_t c = have - off < n ? have - off : n;
    memcpy(dst, blob + off, c);
}

/* weights -> [oc_pad][k64] rows, each kernel row padded to row_pad bytes.
 * nchw: source is OIHW and the (transposed) input has c_pad channels. */
void mars_pack_conv_i8(const int8_t *w, size_t avail, int nchw, int out_c, int in_c, int kh, int kw,
                       int c_pad, int row_pad, int oc_pad, int8_t *dst) {
    const int k64 = (int)ALIGN_UP((size_t)kh * row_pad, 64);
    memset(dst, 0, (size_t)oc_pad * k64);
    for (int oc = 0; oc < out_c; oc++)
        for (int ky = 0; ky < kh; ky++)
            for (int kx = 0; kx < kw; kx++)
                for (int ic = 0; ic < in_c; ic++) {
                    size_t src = nchw ? (((size_t)oc * in_c + ic) * kh + ky) * kw + kx
                                      : (((size_t)oc * kh + ky) * kw + kx) * in_c + ic;
                    int8_t v = src < avail ? w[src] : 0;
                    dst[(size_t)mhip_conv_i8_oc_row(oc, oc_pad) * k64 + (size_t)ky * row_pad + (size_t)kx * c_pad + ic] = v;
                }
}

/* ------------------------------------------------------------------- ops */
static mars_op_t *new_op(mars_model_ext_t *m, int kind, int layer) {
    if (m->n_ops == m->cap_ops) {
        int cap = m->cap_ops ? m->cap_ops * 2 : 64;
        mars_op_t *p = (mars_op_t *)realloc(m->ops, (size_t)cap * sizeof(mars_op_t));
        if (!p) { m->plan_err = MARS_ERR_ALLOC_FAILED; return NULL; }
        m->ops = p;
        m->cap_ops = cap;
    }
    mars_op_t *op = &m->ops[m->n_ops++];
    memset(op, 0, sizeof(*op));
    op->kind = kind;
    op->layer = layer;
    op->t_in[0] = op->t_in[1] = op->t_in[2] = op->t_in[3] = op->t_out = -1;
    op->w_off = op->b_off = op->lut_off = op->lut2_off = op->s_off = op->w2_off = op->w3_off = NO_OFF;
    op->w_blob_off[0] = op->w_blob_off[1] = NO_OFF;
    op->prof_kind = 4;
    return op;
}

static void fail_op(mars_model_ext_t *m, int layer, int err) {
    mars_op_t *op = new_op(m, OP_FAIL, layer);
    if (op) op->err = err;
}

/* the executor searches tensors by desc.id, first match (mars_runtime.c:516-558, 713-721) */
static int find_tensor(const mars_model_ext_t *m, uint32_t id) {
    if (id == NO_TENSOR) return -1;
    for (uint32_t i = 0; i < m->pub.header.num_tensors; i++)
        if (m->pub.tensors[i].desc.id == id) return (int)i;
    return -1;
}

static void touch(mars_model_ext_t *m, int ti, size_t extent) {
    if (ti < 0) return;
    mtensor_t *t = &m->mt[ti];
    t->needed = 1;
    if (t->is_weight) {
        size_t end = (size_t)m->pub.tensors[ti].desc.data_offset + extent;
        if (end > m->blob_mirror_bytes) m->blob_mirror_bytes = end;
    } else if (extent > t->extent) {
        t->extent = extent;
    }
}

static size_t lut_i8(mars_model_ext_t *m, const int8_t table[256]) {
    size_t off = arena_reserve(m, 256);
    if (off != NO_OFF) memcpy(m->arena_host + off, table, 256);
    return off;
}

/* int8 sigmoid of one value, reference mars_runtime.c:758-768 */
static int sigmoid_q(int q, float in_scale, float out_scale) {
    float os = out_scale > 0 ? out_scale : 1.0f;
    float x = (float)q * in_scale;
    float y = 1.0f / (1.0f + expf(-x));
    return q_half_up(y / os);
}
/* int8 mul/add of one pair, reference mars_runtime.c:822-835 / :889-902 */
static int binary_q(int is_mul, int a, int b, float sa, float sb, float so) {
    float inv = 1.0f / (so > 0 ? so : 1.0f);
    float va = (float)a * sa, vb = (float)b * sb;
    float y = is_mul ? va * vb : va + vb;
    return q_half_up(y * inv);
}

/* ---- CONV2D: reference mars_runtime.c:511-710 */
static void plan_conv(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    const mars_conv_params_t *cp = &L->params.conv;
    int ti = find_tensor(m, L->input_tensor_ids[0]);
    int to = find_tensor(m, L->output_tensor_ids[0]);
    int tw = find_tensor(m, cp->weight_tensor_id);
    int tb = find_tensor(m, cp->bias_tensor_id);
    if (ti < 0 || to < 0 || tw < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    const mars_tensor_t *in = &m->pub.tensors[ti].desc, *out = &m->pub.tensors[to].desc;
    const mars_tensor_t *w = &m->pub.tensors[tw].desc;
    /* weights / bias must come from the blob, the result must be an activation, and a
     * parallel kernel cannot run a layer in place */
    if (!m->mt[tw].is_weight || (tb >= 0 && !m->mt[tb].is_weight) || m->mt[to].is_weight || ti == to) {
        fail_op(m, li, MARS_ERR_LAYER_FAILED);
        return;
    }
    const int in_nhwc = in->format == MARS_FORMAT_NHWC, out_nhwc = out->format == MARS_FORMAT_NHWC;
    int in_h, in_w, in_c, out_h, out_w, out_c;
    if (in_nhwc) { in_h = in->shape[1]; in_w = in->shape[2]; in_c = in->shape[3]; }
    else         { in_c = in->shape[1]; in_h = in->shape[2]; in_w = in->shape[3]; }
    if (out_nhwc) { out_h = out->shape[1]; out_w = out->shape[2]; out_c = out->shape[3]; }
    else          { out_c = out->shape[1]; out_h = out->shape[2]; out_w = out->shape[3]; }
    const int kh = (int)cp->kernel_h, kw = (int)cp->kernel_w, sh = (int)cp->stride_h, sw = (int)cp->stride_w;
    int pt = 0, pl = 0;
    if (cp->padding == MARS_PAD_SAME) { /* EXPLICIT / VALID run unpadded (:592-598) */
        int32_t ph = (int32_t)((uint32_t)(out_h - 1) * cp->stride_h + cp->kernel_h - (uint32_t)in_h);
        int32_t pw = (int32_t)((uint32_t)(out_w - 1) * cp->stride_w + cp->kernel_w - (uint32_t)in_w);
        pt = ph / 2;
        pl = pw / 2;
    }
    if (out_h <= 0 || out_w <= 0 || out_c <= 0) return; /* empty loops in the reference: nothing is written */
    /* channel counts are bounded so that every packed-weight product below (kw * c_pad, kh * row_pad, oc_pad * k64)
     * stays far inside int / size_t: a crafted in_c once wrapped kw * in_c and let the packer write past its slot */
    if (in_h <= 0 || in_w <= 0 || in_c <= 0 || kh <= 0 || kw <= 0 || sh < 0 || sw < 0 || kh > 64 || kw > 64 ||
        in_c > MAX_CHANNELS || out_c > MAX_CHANNELS ||
        (size_t)in_h * in_w * in_c > MAX_DIM_PRODUCT || (size_t)out_h * out_w * out_c > MAX_DIM_PRODUCT ||
        (size_t)out_c * in_c * kh * kw > ((size_t)1 << 31)) {
        fail_op(m, li, MARS_ERR_LAYER_FAILED); /* degenerate geometry this build does not launch */
        return;
    }
    const int is_f32 = in->dtype == MARS_DTYPE_FLOAT32;
    mars_op_t *op = new_op(m, is_f32 ? OP_CONV_F32 : OP_CONV_I8, li);
    if (!op) return;
    op->t_in[0] = ti; op->n_in = 1; op->t_out = to;
    op->in_h = in_h; op->in_w = in_w; op->in_c = in_c;
    op->out_h = out_h; op->out_w = out_w; op->out_c = out_c;
    op->kh = kh; op->kw = kw; op->sh = sh; op->sw = sw; op->pt = pt; op->pl = pl;
    op->is_f32 = is_f32;
    op->macs = (double)out_h * out_w * out_c * in_c * kh * kw;
    const size_t es = is_f32 ? 4 : 1;
    touch(m, ti, (size_t)in_h * in_w * in_c * es);
    touch(m, to, (size_t)out_h * out_w * out_c * es);
    m->mt[tw].needed = 1;
    op->bytes = (double)((size_t)in_h * in_w * in_c + (size_t)out_h * out_w * out_c) * es;
    const size_t wcount = (size_t)out_c * in_c * kh * kw;

    if (is_f32) {
        op->prof_kind = 1;
        op->w_off = arena_reserve(m, wcount * 4);
        if (op->w_off == NO_OFF) return;
        if (!m->deferred) blob_read(m, (size_t)w->data_offset, wcount * 4, m->arena_host + op->w_off);
        /* The bf16 images of the weights the split-operand matrix-core kernels read, for the f32_mfma mode in force AT LOAD (set it
         * before loading; a model switched to mode 3 / 4 later runs its convolutions on the f32 matrix cores instead): mode 3 =
         * conv_f32_patch's image where the shape is one it takes (k x k layers; unit table + two planes in its K order), else two
         * planes for conv_f32_split; mode 4 = three planes for conv_f32_split; modes 0 - 2 read neither (no dead planes in
         * the arena, its upload and its multi-GPU broadcast). */
        {
            const int mode = m->plan_f32_mode;
            size_t n3 = 0;
            int stem = 0;
            if (mode == 3 && sh == sw && pt == pl) {
                n3 = mhip_conv_f32_stem_pack(out_c, in_c, kh, kw, sw, pl, in_h, in_w, out_h, out_w, NULL, NULL);
                stem = n3 != 0;
                if (!n3) n3 = mhip_conv_f32_patch_pack(out_c, in_c, kh, kw, sw, pl, in_h, in_w, out_h, out_w, NULL, NULL);
            }
            if (n3) {
                op->w3_stem = stem;
                op->w3_off = arena_reserve(m, n3);
                if (op->w3_off == NO_OFF) return;
                if (!m->deferred) {
                    if (stem)
                        mhip_conv_f32_stem_pack(out_c, in_c, kh, kw, sw, pl, in_h, in_w, out_h, out_w, (const float *)(m->arena_host + op->w_off),
                                                m->arena_host + op->w3_off);
                    else
                        mhip_conv_f32_patch_pack(out_c, in_c, kh, kw, sw, pl, in_h, in_w, out_h, out_w, (const float *)(m->arena_host + op->w_off),
                                                 m->arena_host + op->w3_off);
                }
            } else if (mode >= 3) {
                const int planes = mode == 3 ? 2 : 3;
                const size_t n2 = mhip_conv_f32_split_pack(out_c, in_c, kh, kw, sw, planes, NULL, NULL);
                if (n2) {
                    op->w2_off = arena_reserve(m, n2);
                    if (op->w2_off == NO_OFF) return;
                    op->w2_planes = planes; /* what a later mode change may read (conv_f32_params) */
                    if (!m->deferred)
                        mhip_conv_f32_split_pack(out_c, in_c, kh, kw, sw, planes, (const float *)(m->arena_host + op->w_off), m->arena_host + op->w2_off);
                }
            }
        }
        if (tb >= 0) {
            op->b_off = arena_reserve(m, (size_t)out_c * 4);
            if (op->b_off != NO_OFF && !m->deferred)
                blob_read(m, (size_t)m->pub.tensors[tb].desc.data_offset, (size_t)out_c * 4, m->arena_host + op->b_off);
        }
        if (cp->activation == MARS_ACT_RELU) { /* byte-wise clamp over H*W*C BYTES of the f32 result (:700-707) */
            mars_op_t *r = new_op(m, OP_RELU_BYTES, li);
            if (r) { r->t_out = to; r->n = (size_t)out_h * out_w * out_c; r->prof_kind = 2; r->bytes = 2.0 * r->n; }
        }
        return;
    }

    op->prof_kind = 0;
    op->nchw = !in_nhwc; /* the kernel is chosen by the INPUT tag (:640-662) */
    op->out_nchw = op->nchw; /* ... and conv2d_int8_mxu writes [O][H][W] whatever the output's tag says */
    op->c_pad = op->nchw ? (int)ALIGN_UP((size_t)in_c, 16) : in_c;
    /* NCHW stem (round 6: the shipped files' first layer is 3 planes of 640 x 640): relaid to 4 bytes per pixel, the small-channel kernels'
     * own input layout (K = 6 rows x 32 bytes), instead of 16 (K = 6 x 96: 2.4 of yolov5n_int8.mars' 12.5 ms per batch went there) */
    if (op->nchw && in_c <= 4 && mhip_conv_i8_small_c(4, kw, out_c) && ((size_t)in_h * in_w) % 4 == 0) op->c_pad = 4;
    int c_eff = op->c_pad; /* bytes per pixel in the packed K layout (4 in small-channel mode) */
    mhip_conv_i8_pack_geom(op->c_pad, kw, out_c, &op->row_pad, &op->oc_pad, &c_eff);
    const size_t k64 = ALIGN_UP((size_t)kh * op->row_pad, 64);
    op->w_off = arena_reserve(m, (size_t)op->oc_pad * k64);
    if (op->w_off == NO_OFF) return;
    if (!m->deferred) {
        int8_t *tmp = (int8_t *)malloc(wcount ? wcount : 1);
        if (!tmp) { m->plan_err = MARS_ERR_ALLOC_FAILED; return; }
        blob_read(m, (size_t)w->data_offset, wcount, tmp);
        mars_pack_conv_i8(tmp, wcount, op->nchw, out_c, in_c, kh, kw, c_eff, op->row_pad, op->oc_pad,
                          (int8_t *)m->arena_host + op->w_off);
        free(tmp);
    }
    if (!op->nchw) { /* RGB stem: its matrix-core operands pre-laid for conv_i8_rgb (12 KB for 32 channels, 6 x 6) */
        const size_t n2 = mhip_conv_i8_rgb_pack(in_c, kh, kw, sh, sw, pl, op->oc_pad, (int)k64, NULL, NULL);
        if (n2) {
            op->w2_off = arena_reserve(m, n2);
            if (op->w2_off == NO_OFF) return;
            if (!m->deferred)
                mhip_conv_i8_rgb_pack(in_c, kh, kw, sh, sw, pl, op->oc_pad, (int)k64, (const int8_t *)m->arena_host + op->w_off,
                                      (int8_t *)m->arena_host + op->w2_off);
        }
    }
    if (!op->nchw && op->w2_off == NO_OFF) { /* deep 3x3 stride-1 layers: the weight image conv_i8_rows streams (same bytes, K-step blocks) */
        const size_t n3 = mhip_conv_i8_rows_pack(in_c, kh, kw, sh, sw, op->oc_pad, (int)k64, out_w, NULL, NULL);
        if (n3) {
            op->w2_off = arena_reserve(m, n3);
            if (op->w2_off == NO_OFF) return;
            op->w2_rows = 1;
            if (!m->deferred)
                mhip_conv_i8_rows_pack(in_c, kh, kw, sh, sw, op->oc_pad, (int)k64, out_w, (const int8_t *)m->arena_host + op->w_off,
                                       (int8_t *)m->arena_host + op->w2_off);
        }
    }
    if (tb >= 0) { /* raw bytes reinterpreted as int32, whatever the tensor says it is (:645,656) */
        op->b_off = arena_reserve(m, (size_t)op->oc_pad * 4);
        if (op->b_off != NO_OFF && !m->deferred) {
            int32_t *raw = (int32_t *)calloc((size_t)out_c, 4), *dstb = (int32_t *)(m->arena_host + op->b_off);
            if (!raw) { m->plan_err = MARS_ERR_ALLOC_FAILED; return; }
            blob_read(m, (size_t)m->pub.tensors[tb].desc.data_offset, (size_t)out_c * 4, raw);
            for (int oc = 0; oc < out_c; oc++) dstb[mhip_conv_i8_oc_row(oc, op->oc_pad)] = raw[oc]; /* same row order as the weights */
            free(raw);
        }
    }
    op->cs = (in->scale * w->scale) / out->scale; /* float32, this order (mxu_conv.c:639,722) */
    op->safe = mhip_conv_i8_is_safe(op->cs);
    op->relu = cp->activation == MARS_ACT_RELU;
    if (op->nchw) {
        size_t need = (size_t)in_h * in_w * op->c_pad;
        if (need > m->scratch_per_frame) m->scratch_per_frame = need;
        /* (op->bytes stays input + output: the relayout's traffic is this implementation's cost, not algorithmic work) */
    }
}

static size_t numel_of(const mars_model_ext_t *m, int ti) { return shape_numel(&m->pub.tensors[ti].desc); }

/* ---- SIGMOID / RELU family: unary maps (mars_runtime.c:724-771, 1047-1089) */
static void plan_unary(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    int ti = find_tensor(m, L->input_tensor_ids[0]), to = find_tensor(m, L->output_tensor_ids[0]);
    if (ti < 0 || to < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    if (m->mt[to].is_weight) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    const mars_tensor_t *in = &m->pub.tensors[ti].desc, *out = &m->pub.tensors[to].desc;
    const size_t n = numel_of(m, ti);
    if (n == 0) return;
    const int is_sig = L->type == MARS_LAYER_SIGMOID;
    const int leaky = L->type == MARS_LAYER_LEAKY_RELU;
    if (in->dtype == MARS_DTYPE_FLOAT32) {
        mars_op_t *op = new_op(m, is_sig ? OP_SIGMOID_F32 : OP_RELU_F32, li);
        if (!op) return;
        op->t_in[0] = ti; op->n_in = 1; op->t_out = to; op->n = n;
        op->f0 = leaky ? 0.01f : 0.0f; /* slope is a constant in the reference (:1064) */
        op->prof_kind = 2; op->bytes = 8.0 * n;
        touch(m, ti, n * 4); touch(m, to, n * 4);
        return;
    }
    int8_t tab[256];
    for (int q = -128; q < 128; q++) {
        int r;
        if (is_sig) r = sigmoid_q(q, in->scale, out->scale);
        else if (q > 0) r = q;
        else if (leaky) { int32_t v = mars_trunc_x86((float)q * 0.01f); r = (int8_t)(v < -128 ? -128 : v); }
        else r = 0; /* RELU and RELU6 alike: no upper clamp (:1179-1182) */
        tab[q + 128] = (int8_t)r;
    }
    mars_op_t *op = new_op(m, OP_LUT_I8, li);
    if (!op) return;
    op->t_in[0] = ti; op->n_in = 1; op->t_out = to; op->n = n;
    op->lut_off = lut_i8(m, tab);
    op->prof_kind = 2; op->bytes = 2.0 * n;
    touch(m, ti, n); touch(m, to, n);
}

/* ---- MUL / ADD (mars_runtime.c:774-905): extent from operand A only */
static void plan_binary(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    int ta = find_tensor(m, L->input_tensor_ids[0]), tb = find_tensor(m, L->input_tensor_ids[1]);
    int to = find_tensor(m, L->output_tensor_ids[0]);
    if (ta < 0 || tb < 0 || to < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    if (m->mt[to].is_weight) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    const mars_tensor_t *a = &m->pub.tensors[ta].desc, *b = &m->pub.tensors[tb].desc, *o = &m->pub.tensors[to].desc;
    const size_t n = numel_of(m, ta);
    if (n == 0) return;
    const int f32 = a->dtype == MARS_DTYPE_FLOAT32;
    mars_op_t *op = new_op(m, f32 ? OP_BINARY_F32 : OP_BINARY_I8, li);
    if (!op) return;
    op->t_in[0] = ta; op->t_in[1] = tb; op->n_in = 2; op->t_out = to; op->n = n;
    op->is_mul = L->type == MARS_LAYER_MUL;
    op->f0 = a->scale; op->f1 = b->scale;
    op->f2 = 1.0f / (o->scale > 0 ? o->scale : 1.0f);
    op->prof_kind = 2; op->bytes = 3.0 * n * (f32 ? 4 : 1);
    const size_t es = f32 ? 4 : 1;
    touch(m, ta, n * es); touch(m, tb, n * es); touch(m, to, n * es);
}

/* ---- MAXPOOL (mars_runtime.c:908-960) */
static void plan_maxpool(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    const mars_pool_params_t *pp = &L->params.pool;
    int ti = find_tensor(m, L->input_tensor_ids[0]), to = find_tensor(m, L->output_tensor_ids[0]);
    if (ti < 0 || to < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    if (m->mt[to].is_weight || ti == to) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    const mars_tensor_t *in = &m->pub.tensors[ti].desc, *out = &m->pub.tensors[to].desc;
    int in_h = in->shape[1], in_w = in->shape[2], ch = in->shape[3], out_h = out->shape[1], out_w = out->shape[2];
    if (out_h <= 0 || out_w <= 0 || ch <= 0) return;
    if (in_h < 0 || in_w < 0 || (int)pp->kernel_h < 0 || (int)pp->kernel_w < 0 || (int)pp->stride_h < 0 ||
        (int)pp->stride_w < 0 || pp->kernel_h > 4096 || pp->kernel_w > 4096) {
        fail_op(m, li, MARS_ERR_LAYER_FAILED);
        return;
    }
    mars_op_t *op = new_op(m, OP_MAXPOOL, li);
    if (!op) return;
    op->t_in[0] = ti; op->n_in = 1; op->t_out = to;
    op->in_h = in_h; op->in_w = in_w; op->in_c = ch; op->out_h = out_h; op->out_w = out_w;
    op->kh = (int)pp->kernel_h; op->kw = (int)pp->kernel_w; op->sh = (int)pp->stride_h; op->sw = (int)pp->stride_w;
    op->prof_kind = 3;
    op->bytes = (double)in_h * in_w * ch + (double)out_h * out_w * ch;
    /* reads stay inside in_h*in_w*ch by the window clip; writes cover out_h*out_w*ch */
    if (op->kh > 0 && op->kw > 0) touch(m, ti, (size_t)in_h * in_w * ch);
    else m->mt[ti].needed = 1;
    touch(m, to, (size_t)out_h * out_w * ch);
}

/* ---- CONCAT (mars_runtime.c:963-1000): one copy kernel per input, in order */
static void plan_concat(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    int to = find_tensor(m, L->output_tensor_ids[0]);
    if (to < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    if (m->mt[to].is_weight) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    const mars_tensor_t *out = &m->pub.tensors[to].desc;
    const int out_h = out->shape[1], out_w = out->shape[2], out_c = out->shape[3];
    if (L->num_inputs > 4) { fail_op(m, li, MARS_ERR_INVALID_LAYER); return; }
    int off = 0;
    for (uint32_t k = 0; k < L->num_inputs; k++) {
        int ti = find_tensor(m, L->input_tensor_ids[k]);
        if (ti < 0) continue; /* skipped without advancing the channel offset (:980) */
        const int in_c = m->pub.tensors[ti].desc.shape[3];
        if (out_h > 0 && out_w > 0 && in_c > 0) {
            /* pixel slots of one input may not overlap each other in a parallel copy */
            if (in_c > out_c || out_c <= 0 || ti == to) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
            mars_op_t *op = new_op(m, OP_CONCAT_SLICE, li);
            if (!op) return;
            op->t_in[0] = ti; op->n_in = 1; op->t_out = to;
            op->out_h = out_h; op->out_w = out_w; op->in_c = in_c; op->out_c = out_c; op->ch_off = off;
            op->prof_kind = 3;
            const size_t npix = (size_t)out_h * out_w;
            op->bytes = 2.0 * npix * in_c;
            touch(m, ti, npix * in_c);
            touch(m, to, (npix - 1) * out_c + off + in_c);
        }
        off += in_c;
    }
}

/* ---- UPSAMPLE (mars_runtime.c:1003-1044) */
static void plan_upsample(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    const mars_upsample_params_t *up = &L->params.upsample;
    int ti = find_tensor(m, L->input_tensor_ids[0]), to = find_tensor(m, L->output_tensor_ids[0]);
    if (ti < 0 || to < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    if (m->mt[to].is_weight || ti == to) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    const mars_tensor_t *in = &m->pub.tensors[ti].desc, *out = &m->pub.tensors[to].desc;
    int in_h = in->shape[1], in_w = in->shape[2], ch = in->shape[3], out_h = out->shape[1], out_w = out->shape[2];
    if ((up->scale_h == 0 && in_h == 0) || (up->scale_w == 0 && in_w == 0)) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    int sh = up->scale_h > 0 ? (int)up->scale_h : out_h / in_h;
    int sw = up->scale_w > 0 ? (int)up->scale_w : out_w / in_w;
    if (out_h <= 0 || out_w <= 0 || ch <= 0) return;
    if (sh <= 0 || sw <= 0 || in_h <= 0 || in_w <= 0) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    mars_op_t *op = new_op(m, OP_UPSAMPLE, li);
    if (!op) return;
    op->t_in[0] = ti; op->n_in = 1; op->t_out = to;
    op->in_h = in_h; op->in_w = in_w; op->in_c = ch; op->out_h = out_h; op->out_w = out_w;
    op->scale_h = sh; op->scale_w = sw;
    op->prof_kind = 3;
    op->bytes = (double)in_h * in_w * ch + (double)out_h * out_w * ch;
    touch(m, ti, (size_t)in_h * in_w * ch);
    touch(m, to, (size_t)out_h * out_w * ch);
}

/* ---- BATCHNORM (mars_runtime.c:1092-1158) */
static void plan_batchnorm(mars_model_ext_t *m, int li) {
    const mars_layer_t *L = &m->pub.layers[li].desc;
    int ti = find_tensor(m, L->input_tensor_ids[0]), to = find_tensor(m, L->output_tensor_ids[0]);
    int ts = find_tensor(m, L->input_tensor_ids[1]), tb = find_tensor(m, L->input_tensor_ids[2]);
    if (ti < 0 || to < 0) { fail_op(m, li, MARS_ERR_INVALID_TENSOR); return; }
    if (m->mt[to].is_weight || (ts >= 0 && !m->mt[ts].is_weight) || (tb >= 0 && !m->mt[tb].is_weight)) {
        fail_op(m, li, MARS_ERR_LAYER_FAILED);
        return;
    }
    const mars_tensor_t *in = &m->pub.tensors[ti].desc, *out = &m->pub.tensors[to].desc;
    int n = in->shape[0] > 0 ? in->shape[0] : 1, c = in->shape[1] > 0 ? in->shape[1] : 1;
    int h = in->shape[2] > 0 ? in->shape[2] : 1, w = in->shape[3] > 0 ? in->shape[3] : 1;
    if ((size_t)n * c * h * w > MAX_DIM_PRODUCT || c > MAX_CHANNELS) { fail_op(m, li, MARS_ERR_LAYER_FAILED); return; }
    const int f32 = in->dtype == MARS_DTYPE_FLOAT32;
    mars_op_t *op = new_op(m, OP_BN, li);
    if (!op) return;
    op->t_in[0] = ti; op->n_in = 1; op->t_out = to;
    op->bn_n = n; op->in_c = c; op->in_h = h; op->in_w = w; op->is_f32 = f32;
    op->f0 = in->scale > 0 ? in->scale : 1.0f;
    op->f1 = out->scale > 0 ? out->scale : 1.0f;
    if (ts >= 0) {
        op->s_off = arena_reserve(m, (size_t)c * 4);
        if (op->s_off != NO_OFF && !m->deferred)
            blob_read(m, (size_t)m->pub.tensors[ts].desc.data_offset, (size_t)c * 4, m->arena_host + op->s_off);
    }
    if (tb >= 0) {
        op->b_off = arena_reserve(m, (size_t)c * 4);
        if (op->b_off != NO_OFF && !m->deferred)
            blob_read(m, (size_t)m->pub.tensors[tb].desc.data_offset, (size_t)c * 4, m->arena_host + op->b_off);
    }
    const size_t total = (size_t)n * c * h * w * (f32 ? 4 : 1);
    op->prof_kind = 2; op->bytes = 2.0 * total;
    touch(m, ti, total); touch(m, to, total);
}

/* dispatcher, reference mars_runtime.c:1161-1224 */
void plan_layer(mars_model_ext_t *m, int li) {
    switch (m->pub.layers[li].desc.type) {
        case MARS_LAYER_CONV2D: plan_conv(m, li); break;
        case MARS_LAYER_SIGMOID:
        case MARS_LAYER_RELU:
        case MARS_LAYER_RELU6:
        case MARS_LAYER_LEAKY_RELU: plan_unary(m, li); break;
        case MARS_LAYER_MUL:
        case MARS_LAYER_ADD: plan_binary(m, li); break;
        case MARS_LAYER_MAXPOOL: plan_maxpool(m, li); break;
        case MARS_LAYER_CONCAT: plan_concat(m, li); break;
        case MARS_LAYER_UPSAMPLE: plan_upsample(m, li); break;
        case MARS_LAYER_BATCHNORM: plan_batchnorm(m, li); break;
        case MARS_LAYER_DEPTHWISE_CONV2D: /* accepted, not executed (:1168-1213) */
        case MARS_LAYER_AVGPOOL:
        case MARS_LAYER_SILU:
        case MARS_LAYER_RESHAPE:
        case MARS_LAYER_TRANSPOSE:
        case MARS_LAYER_SOFTMAX: break;
        default: fail_op(m, li, MARS_ERR_INVALID_LAYER); break; /* GLOBAL_AVGPOOL, FC, unknown (:1218-1220) */
    }
}

/* ---------------------------------------------------------- use-def helpers
 * The operand model (mars_op_t): a launch reads t_in[0 .. n_in) and writes t_out + chain_out[0 .. chain_n).  Two facts let every pass use
 * the same helpers, whatever arrays its hand-written loops used to scan:
 *  (1) seg_t / add_t / vc_t name entries of t_in once more (plan_check), so scanning them next to t_in finds nothing new;
 *  (2) chain_n == 0 in every op until fuse_pool_chains has run, so before it `o->t_out == t` and op_writes(o, t) agree. */
int op_reads(const mars_op_t *o, int t) {
    for (int k = 0; k < o->n_in; k++)
        if (o->t_in[k] == t) return 1;
    return 0;
}
int op_writes(const mars_op_t *o, int t) {
    if (o->t_out == t) return 1;
    for (int k = 0; k < o->chain_n; k++)
        if (o->chain_out[k] == t) return 1;
    return 0;
}

/* readers[t] = operand slots that read tensor t (an op that reads it twice counts twice), writers[t] = ops that write it; both for the caller to
 * free (one allocation: free(readers)).  A pass that rewrites ops keeps the counts it still needs current itself.  0 = out of memory. */
static int use_counts(const mars_model_ext_t *m, int **readers, int **writers) {
    const size_t nt = (size_t)m->pub.header.num_tensors + 1;
    int *c = (int *)calloc(2 * nt, sizeof(int));
    if (!c) return 0;
    for (int i = 0; i < m->n_ops; i++) {
        const mars_op_t *o = &m->ops[i];
        for (int k = 0; k < o->n_in; k++)
            if (o->t_in[k] >= 0) c[o->t_in[k]]++;
        if (o->t_out >= 0) c[nt + (size_t)o->t_out]++;
        for (int k = 0; k < o->chain_n; k++) /* (the chain's last stage is t_out: counted above) */
            if (o->chain_out[k] >= 0 && o->chain_out[k] != o->t_out) c[nt + (size_t)o->chain_out[k]]++;
    }
    *readers = c;
    *writers = c + nt;
    return 1;
}

/* the last op in front of op `before` whose t_out is t (THE writer where writers[t] == 1), or -1 */
static int writer_before(const mars_model_ext_t *m, int t, int before) {
    for (int k = before - 1; k >= 0; k--)
        if (m->ops[k].t_out == t) return k;
    return -1;
}

enum { USE_READ = 1, USE_WRITE = 2 };
/* does an op in [lo, hi) read / write tensor t?  (ops a pass has marked dead, kind -1, count like any other) */
static int touched_between(const mars_model_ext_t *m, int lo, int hi, int t, int how) {
    for (int k = lo < 0 ? 0 : lo; k < hi && k < m->n_ops; k++)
        if (((how & USE_READ) && op_reads(&m->ops[k], t)) || ((how & USE_WRITE) && op_writes(&m->ops[k], t))) return 1;
    return 0;
}
/* does an op outside [lo, hi] read or write tensor t? */
static int touched_by_other(const mars_model_ext_t *m, int t, int lo, int hi) {
    return touched_between(m, 0, lo, t, USE_READ | USE_WRITE) || touched_between(m, hi + 1, m->n_ops, t, USE_READ | USE_WRITE);
}

/* closes a pass that marked ops dead (kind = -1) */
static void drop_dead_ops(mars_model_ext_t *m) {
    int w = 0;
    for (int i = 0; i < m->n_ops; i++)
        if (m->ops[i].kind != -1) m->ops[w++] = m->ops[i];
    m->n_ops = w;
}

/* device bytes per frame a tensor will get (alloc_batch).  Every tensor a launch touches has extent > 0, so the 256 of an empty one only shows for
 * a graph input / output that no layer uses. */
size_t planned_stride(const mtensor_t *t) {
    size_t s = ALIGN_UP(t->extent > t->bytes ? t->extent : t->bytes, 256);
    return s ? s : 256;
}

/* the half-step form of a convolution's fused 256-entry table, where its scale allows it: index k = trunc(2 * acc * cs) in [-256, 255] determines
 * round-half-away(acc * cs) = (k >= 0 ? (k+1)>>1 : -((1-k)>>1)) exactly (conv_i8.hip, requant_pack FAST); the ReLU clamp folds in.
 * (tab may point into the arena: it is read before the arena can move) */
static void lut2_from_lut(mars_model_ext_t *m, mars_op_t *c, const int8_t *tab) {
    if (!mhip_conv_i8_lut2_ok(c->cs)) return;
    int8_t tab2[512];
    for (int k = -256; k < 256; k++) {
        int r = k >= 0 ? (k + 1) >> 1 : -((1 - k) >> 1);
        const int lo = c->relu ? 0 : -128;
        r = r < lo ? lo : (r > 127 ? 127 : r);
        tab2[k + 256] = tab[r + 128];
    }
    c->lut2_off = arena_reserve(m, 512);
    if (c->lut2_off != NO_OFF) memcpy(m->arena_host + c->lut2_off, tab2, 512);
}

/* the geometry half of a conv_i8 launch record (conv_i8_record adds addresses, strides and the epilogue's operands) */
static void conv_i8_geometry(const mars_op_t *op, int frames, mhip_conv_i8_t *p) {
    memset(p, 0, sizeof(*p));
    p->frames = frames;
    p->in_c = op->in_c; p->in_h = op->in_h; p->in_w = op->in_w;
    p->out_h = op->out_h; p->out_w = op->out_w; p->out_c = op->store_c ? op->store_c : op->out_c;
    p->kh = op->kh; p->kw = op->kw; p->stride_h = op->sh; p->stride_w = op->sw; p->pad_top = op->pt; p->pad_left = op->pl;
    p->row_pad = op->row_pad; p->oc_pad = op->oc_pad; p->safe = op->safe;
    p->out_pix_stride = op->out_pix_stride; p->out_ch_off = op->out_ch_off;
}
/* does the device code take convolution `op` with a 1 x 1 + SiLU folded in front of it (fuse_bottleneck), at this batch and these frame strides?
 * It decides on geometry: the operands only need to be non-null */
int conv_i8_pre_fits(const mars_op_t *op, int frames, size_t in_stride, size_t out_stride) {
    mhip_conv_i8_t p;
    conv_i8_geometry(op, frames, &p);
    p.in_stride = in_stride; p.out_stride = out_stride;
    p.pre_w = (const int8_t *)op; p.pre_bias = (const int32_t *)op; p.pre_lut2 = (const uint8_t *)op; p.lut2 = (const uint8_t *)op;
    p.lut = (const uint8_t *)op;
    return mhip_conv_i8_pre_ok(&p);
}

/* ---- the launch records of a group, built in ONE place for the question "does the device code take it at this batch?" (shape-only) and for the
 * launch itself (live), so that the record asked about is the record launched.  Shape-only: an operand's address is a stand-in -- non-null,
 * another one for another tensor (the queries compare outputs) -- and its stride the one alloc_batch will give. */
typedef struct { const mars_model_ext_t *m; int frames, live; } rec_ctx_t;
static uint8_t *rec_addr(const rec_ctx_t *c, int ti) {
    if (c->live) return tdev(c->m, ti);
    return ti >= 0 ? (uint8_t *)c->m->mt + ti : NULL;
}
static size_t rec_stride(const rec_ctx_t *c, int ti) { return c->live ? tstride(c->m, ti) : ti >= 0 ? planned_stride(&c->m->mt[ti]) : 0; }
/* an entry of the parameter arena; `image`: one of the fused forms' weight images, which a candidate has not reserved yet */
static const uint8_t *rec_param(const rec_ctx_t *c, size_t off, int image) {
    if (!c->live) return image || off != NO_OFF ? (const uint8_t *)c->m->mt : NULL;
    return off != NO_OFF ? c->m->arena_dev + off : NULL;
}
/* one member's own record; unwritten: its result never reaches memory (the head of a post / split launch), so its tensor has no buffer */
static void conv_i8_record(const rec_ctx_t *c, const mars_op_t *op, int unwritten, mhip_conv_i8_t *p) {
    conv_i8_geometry(op, c->frames, p);
    p->in = (const int8_t *)rec_addr(c, op->t_in[0]); p->in_stride = rec_stride(c, op->t_in[0]);
    p->out = (int8_t *)rec_addr(c, op->t_out); p->out_stride = rec_stride(c, op->t_out);
    if (c->live && p->in) p->in += op->in_byte_off;   /* (a row range of the tensors: virtual_concat_q) */
    if (c->live && p->out) p->out += op->out_byte_off;
    p->w = (const int8_t *)rec_param(c, op->w_off, 0);
    p->bias = (const int32_t *)rec_param(c, op->b_off, 0);
    p->lut = rec_param(c, op->lut_off, 0);
    p->lut2 = op->lut_off != NO_OFF ? rec_param(c, op->lut2_off, 0) : NULL;
    p->w_rgb = !op->w2_rows ? (const int8_t *)rec_param(c, op->w2_off, 0) : NULL;
    p->w_rows = op->w2_rows ? (const int8_t *)rec_param(c, op->w2_off, 0) : NULL;
    if (op->pre) {
        p->pre_w = (const int8_t *)rec_param(c, op->pre_w_off, 0);
        p->pre_bias = (const int32_t *)rec_param(c, op->pre_b_off, 0);
        p->pre_lut2 = rec_param(c, op->pre_lut2_off, 0);
        p->pre_cs = op->pre_cs;
    }
    p->cs = op->cs; p->relu = op->relu; p->out_nchw = op->out_nchw;
    p->variant = op->variant;
    if (unwritten && op->t_out >= 0) p->out_stride = planned_stride(&c->m->mt[op->t_out]); /* (never allocated: the Add's operand has its layout) */
    if (op->add_t && (!c->live || rec_stride(c, op->add_t - 1) == p->out_stride)) { /* (the planner guarantees equal strides: launch_op) */
        p->add = (const int8_t *)rec_addr(c, op->add_t - 1);
        p->add_s_conv = op->add_s_conv; p->add_s_other = op->add_s_other; p->add_inv = op->add_inv;
    }
    p->nseg = op->nseg;
    p->seg_up = op->seg_up;
    int c0 = 0;
    for (int k = 0; k < 4; k++) {
        p->seg_c0[k] = 0x7fffffff;
        if (k < op->nseg) {
            p->seg_in[k] = (const int8_t *)rec_addr(c, op->seg_t[k]);
            p->seg_stride[k] = rec_stride(c, op->seg_t[k]);
            p->seg_c[k] = op->seg_c[k];
            p->seg_c0[k] = c0;
            c0 += op->seg_c[k];
        }
    }
    if (op->nseg > 1) p->in = p->seg_in[0];
}
/* g[]: the members (candidates: their flags need not be set), side: the chained 1x1's (FORM_SPLIT_CHAIN).  The tile walkers' forms (pair, one
 * tile, + chain) get a record per member, p[k] for g[k]; the patch-staged ones (post, split, + chain) one record, p[0], that carries the mates */
void conv_i8_group_records(const mars_model_ext_t *m, int form, const mars_op_t *g[4], int side, int frames, int live, mhip_conv_i8_t *p) {
    const rec_ctx_t c = {m, frames, live};
    const int patch = form == FORM_POST || form == FORM_SPLIT || form == FORM_SPLIT_CHAIN;
    conv_i8_record(&c, g[0], patch, &p[0]);
    if (!patch) {
        for (int k = 1; k < form_span(form); k++) conv_i8_record(&c, g[k], 0, &p[k]);
        return;
    }
    if (form == FORM_POST) {
        const mars_op_t *cv3 = g[1];
        p->post_w = (const int8_t *)rec_param(&c, g[0]->post_w_off, 1);
        p->post_lut2 = rec_param(&c, cv3->lut2_off, 0);
        p->post_cs = cv3->cs;
        p->post_in = (const int8_t *)rec_addr(&c, cv3->seg_t[1]); p->post_in_stride = rec_stride(&c, cv3->seg_t[1]);
        p->post_out = (int8_t *)rec_addr(&c, cv3->t_out); p->post_out_stride = rec_stride(&c, cv3->t_out);
        if (live && p->post_out) p->post_out += cv3->out_byte_off;
        p->post_out_pix_stride = cv3->out_pix_stride; p->post_out_ch_off = cv3->out_ch_off;
        return;
    }
    p->split_w = (const int8_t *)rec_param(&c, g[0]->split_w_off, 1);
    for (int k = 0; k < 2; k++) {
        p->split_lut2[k] = rec_param(&c, g[1 + k]->lut2_off, 0);
        p->split_cs[k] = g[1 + k]->cs;
        p->split_out[k] = (int8_t *)rec_addr(&c, g[1 + k]->t_out); p->split_out_stride[k] = rec_stride(&c, g[1 + k]->t_out);
    }
    if (form == FORM_SPLIT_CHAIN) {
        p->chain_side = side;
        p->chain_w = (const int8_t *)rec_param(&c, g[0]->chain_w_off, 1);
        p->chain_lut2 = rec_param(&c, g[3]->lut2_off, 0);
        p->chain_cs = g[3]->cs;
        p->chain_out = (int8_t *)rec_addr(&c, g[3]->t_out); p->chain_out_stride = rec_stride(&c, g[3]->t_out);
    }
}
/* does the device code take the group in this form at this batch?  The passes ask for one frame before they set a flag, alloc_batch asks
 * again for its batch.  (The side-by-side pair has no query: its launch steps aside at run time.) */
int conv_i8_group_fits(const mars_model_ext_t *m, int form, const mars_op_t *g[4], int side, int frames) {
    mhip_conv_i8_t p[3];
    const int tile = form == FORM_BOTH || form == FORM_BOTH_CHAIN;
    for (int k = 0; k < form_span(form); k++)
        if (g[k]->t_out < 0 || (tile && g[k]->nchw)) return 0;
    if ((!tile && g[0]->t_in[0] < 0) || ((form == FORM_BOTH_CHAIN || form == FORM_SPLIT_CHAIN) && side != 1 && side != 2)) return 0;
    conv_i8_group_records(m, form, g, side, frames, 0, p);
    switch (form) {
        case FORM_POST: return mhip_conv_i8_post_ok(&p[0]);
        case FORM_SPLIT: case FORM_SPLIT_CHAIN: return mhip_conv_i8_split_ok(&p[0]);
        case FORM_BOTH: return mhip_conv_i8_both_ok(&p[0], &p[1]);
        case FORM_BOTH_CHAIN: return mhip_conv_i8_both_chain_ok(&p[0], &p[1], &p[2], side);
        default: return 0;
    }
}

/* ------------------------------------------------------------------ fusion
 * conv -> sigmoid -> mul (SiLU as exported to ONNX) collapses into the conv
 * epilogue: every value of the chain is a function of the conv's int8 result
 * q1 alone, so lut[q1] = mul(q1, sigmoid(q1)) computed on the host with the
 * reference's own float steps is bit-identical.
 * Only done when q1 and sigmoid(q1) have no other reader and are not outputs.
 * match_silu: ops i .. i + 2 are such a chain, int8 or float32 -> q = {q1, q2, q3}, fwd = the MUL's operand order. */
static int match_silu(const mars_model_ext_t *m, int i, int f32, const int *readers, const int *writers, int q[3], int *fwd) {
    const mars_op_t *c = &m->ops[i], *s = c + 1, *mu = c + 2;
    if (c->kind != (f32 ? OP_CONV_F32 : OP_CONV_I8) || s->kind != (f32 ? OP_SIGMOID_F32 : OP_LUT_I8) || mu->kind != (f32 ? OP_BINARY_F32 : OP_BINARY_I8) || !mu->is_mul)
        return 0;
    if (!f32 && m->pub.layers[s->layer].desc.type != MARS_LAYER_SIGMOID) return 0;
    const int q1 = q[0] = c->t_out, q2 = q[1] = s->t_out, q3 = q[2] = mu->t_out;
    if (s->t_in[0] != q1 || q1 == q2 || q2 == q3 || q1 == q3) return 0;
    *fwd = mu->t_in[0] == q1 && mu->t_in[1] == q2;
    if (!*fwd && !(mu->t_in[0] == q2 && mu->t_in[1] == q1)) return 0;
    /* redirecting the result onto one of the convolution's own inputs would make a parallel launch run in place */
    if (f32 ? q3 == c->t_in[0] || m->mt[q3].is_weight : op_reads(c, q3)) return 0;
    if (readers[q1] != 2 || readers[q2] != 1 || writers[q1] != 1 || writers[q2] != 1 || writers[q3] != 1) return 0;
    if (m->mt[q1].io_out || m->mt[q2].io_out || m->mt[q1].io_in || m->mt[q2].io_in) return 0;
    const size_t n1 = (size_t)c->out_h * c->out_w * c->out_c;
    return s->n == n1 && mu->n == n1; /* the chain must cover exactly the conv's result */
}

/* float32 form of the same chain: conv_f32 -> SIGMOID (float, :742-749) -> MUL (float, :807-816).  The epilogue evaluates
 * s = 1.0f / (1.0f + expf(-v)), out = v * s with the reference's roundings and this image's libm expf (expf_exact.h), so
 * the fused result is the same float bit for bit; the two intermediates are never written (5 of the 7 float passes over
 * the tensor disappear: the element-wise layers were 36 % of the float32 graph's time). */
void fold_silu(mars_model_ext_t *m, int f32) {
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 2 < m->n_ops; i++) {
        mars_op_t *c = &m->ops[i];
        int q[3], fwd;
        if (!match_silu(m, i, f32, readers, writers, q, &fwd)) continue;
        const size_t n1 = (size_t)c->out_h * c->out_w * c->out_c;
        if (f32) {
            c->silu_f32 = 1;
        } else {
            const mars_tensor_t *d1 = &m->pub.tensors[q[0]].desc, *d2 = &m->pub.tensors[q[1]].desc, *d3 = &m->pub.tensors[q[2]].desc;
            int8_t tab[256];
            for (int v = -128; v < 128; v++) {
                int sg = sigmoid_q(v, d1->scale, d2->scale);
                tab[v + 128] = (int8_t)(fwd ? binary_q(1, v, sg, d1->scale, d2->scale, d3->scale)
                                            : binary_q(1, sg, v, d2->scale, d1->scale, d3->scale));
            }
            c->lut_off = lut_i8(m, tab);
            lut2_from_lut(m, c, tab);
        }
        c->t_out = q[2]; /* same bytes written, to q3 instead of q1 */
        touch(m, q[2], n1 * (f32 ? 4 : 1));
        m->mt[q[0]].needed = 0;
        m->mt[q[1]].needed = 0;
        /* drop the two element-wise ops */
        memmove(&m->ops[i + 1], &m->ops[i + 3], (size_t)(m->n_ops - i - 3) * sizeof(mars_op_t));
        m->n_ops -= 2;
    }
    free(readers);
}

/* A single int8 activation layer behind a convolution (RELU / RELU6 / LEAKY_RELU / SIGMOID as their own layers: the shipped tiny_160_int8.mars,
 * any exporter that does not fold them): the layer is a 256-entry map of the convolution's int8 result (plan_unary builds it), which is what the
 * convolution's fused table applies in its epilogue -- the same bytes, one launch and two passes over the tensor less.
 * Conditions as for the SiLU chain: the convolution's result has no other reader and is no graph tensor. */
void fuse_lut(mars_model_ext_t *m) {
    if (m->sw.no_fuse_lut) return;
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 1 < m->n_ops; i++) {
        mars_op_t *c = &m->ops[i], *s = &m->ops[i + 1];
        if (c->kind != OP_CONV_I8 || s->kind != OP_LUT_I8 || c->lut_off != NO_OFF || s->lut_off == NO_OFF) continue;
        const int q1 = c->t_out, q2 = s->t_out;
        if (q1 < 0 || q2 < 0 || s->t_in[0] != q1 || q1 == q2) continue;
        if (op_reads(c, q2)) continue; /* redirecting the result onto one of the convolution's own inputs would make a parallel launch run in place */
        if (readers[q1] != 1 || writers[q1] != 1 || writers[q2] != 1 || m->mt[q1].io_out || m->mt[q1].io_in || m->mt[q1].is_weight || m->mt[q2].is_weight) continue;
        const size_t n1 = (size_t)c->out_h * c->out_w * c->out_c;
        if (s->n != n1 || m->mt[q2].bytes < n1) continue; /* the layer must cover exactly the convolution's result */
        if (m->pub.tensors[q1].desc.dtype != MARS_DTYPE_INT8 || m->pub.tensors[q2].desc.dtype != MARS_DTYPE_INT8) continue;
        c->lut_off = s->lut_off;
        lut2_from_lut(m, c, (const int8_t *)(m->arena_host + s->lut_off));
        c->t_out = q2;
        touch(m, q2, n1);
        m->mt[q1].needed = 0;
        memmove(&m->ops[i + 1], &m->ops[i + 2], (size_t)(m->n_ops - i - 2) * sizeof(mars_op_t));
        m->n_ops -= 1;
    }
    free(readers);
}

/* ------------------------------------------------------------- zero-copy concat
 * A concat input that (a) has exactly one producer launch of a kind that can write a channel slice
 * (int8 NHWC conv, int8 add/mul, max-pool, upsample), (b) is read by nothing but that concat, and
 * (c) has the concat's pixel grid, is produced directly inside the concat's output tensor: the
 * producer gets (pixel stride = concat channels, channel offset) and the copy launch disappears.
 * Same bytes end up in the concat output; the intermediate tensor is never materialised. */
void elide_concat(mars_model_ext_t *m) {
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i < m->n_ops; i++) {
        mars_op_t *cs = &m->ops[i];
        if (cs->kind != OP_CONCAT_SLICE) continue;
        const int ti = cs->t_in[0], to = cs->t_out;
        const mtensor_t *mt = &m->mt[ti];
        if (mt->is_weight || mt->io_in || mt->io_out || readers[ti] != 1 || writers[ti] != 1) continue;
        const int j = writer_before(m, ti, i);
        if (j < 0) continue;
        mars_op_t *pr = &m->ops[j];
        if (pr->out_pix_stride || pr->add_t) continue; /* a folded Add needs its other operand laid out like the output */
        const size_t npix = (size_t)cs->out_h * cs->out_w;
        int ok = 0;
        if (pr->kind == OP_CONV_I8 && !pr->nchw && !pr->out_nchw) ok = (size_t)pr->out_h * pr->out_w == npix && pr->out_c == cs->in_c;
        else if (pr->kind == OP_BINARY_I8) ok = pr->n == npix * (size_t)cs->in_c;
        else if (pr->kind == OP_MAXPOOL || pr->kind == OP_UPSAMPLE) ok = (size_t)pr->out_h * pr->out_w == npix && pr->in_c == cs->in_c;
        if (!ok || cs->ch_off + cs->in_c > cs->out_c) continue;
        /* nothing between producer and the copy may touch the concat output except its other slices (own loop: those are allowed writers,
         * and a slice copy already elided is skipped) */
        int clash = 0;
        for (int k = j; k < i && !clash; k++) {
            const mars_op_t *o = &m->ops[k];
            if (o->kind == -1) continue;
            if (op_reads(o, to) || (o->t_out == to && o->kind != OP_CONCAT_SLICE && !o->out_pix_stride)) clash = 1;
        }
        if (clash) continue;
        pr->t_out = to;
        pr->out_pix_stride = cs->out_c;
        pr->out_ch_off = cs->ch_off;
        if (pr->kind == OP_BINARY_I8) pr->in_c = cs->in_c; /* channel run of the slice */
        pr->bytes += 0;
        m->mt[ti].needed = 0;
        cs->kind = -1;
    }
    drop_dead_ops(m);
    free(readers);
}

/* Dead stores of a CONCAT.  The reference copies input k's "pixels" (runs of shape[3] BYTES, whatever the dtype) to byte
 * p * out_c + off_k of the output, one input after the other (mars_runtime.c:977-996).  When shape[3] of an input EQUALS the
 * output's (the NCHW-tagged float twins: every tensor's shape[3] is the map width), a slice is one contiguous run of
 * npix * out_c bytes starting at off_k, and the next input's run, starting out_c bytes later, overwrites all of it but its first
 * off_j - off_k bytes before anything can read them.  Such a slice copies only the pixels that hold surviving bytes (the partly
 * surviving last one whole: the later slice, launched after it on the same stream, rewrites the rest) -- the tensor's final bytes
 * are the reference's.  On the float yolov5 twins this halves the concat traffic (2.7 -> 1.4 ms per batch of 256). */
void trim_concat(mars_model_ext_t *m) {
    for (int i = 0; i < m->n_ops; i++) {
        mars_op_t *k = &m->ops[i];
        if (k->kind != OP_CONCAT_SLICE || k->in_c != k->out_c || k->out_c <= 0) continue;
        const size_t npix = (size_t)k->out_h * k->out_w;
        for (int q = i + 1; q < m->n_ops && m->ops[q].layer == k->layer; q++) {
            const mars_op_t *j = &m->ops[q];
            if (j->kind != OP_CONCAT_SLICE || j->t_out != k->t_out || j->in_c != j->out_c || j->out_c != k->out_c) continue;
            if ((size_t)j->out_h * j->out_w != npix || j->ch_off < k->ch_off) continue;
            const size_t live = (size_t)(j->ch_off - k->ch_off), live_pix = (live + (size_t)k->out_c - 1) / (size_t)k->out_c;
            if (live_pix < (size_t)k->out_h * k->out_w) {
                k->out_h = 1;
                k->out_w = (int)live_pix; /* 0: nothing of this slice survives (the launcher skips an empty copy) */
                k->bytes = 2.0 * (double)live_pix * k->in_c;
            }
        }
    }
}

/* NCHW-tagged int8 graphs (every shipped model: SURVEY a7, mxu_conv.c:630-670) on the NHWC kernels without a relayout per layer (round 6).
 * conv2d_int8_mxu reads [C][H][W] and writes [O][H][W]; the matrix-core kernels want pixels x channels, so every such convolution used to
 * relay its input into scratch (nchw_to_nhwc_kernel: 44 % of yolov5n_int8.mars' GPU time at batch 256) and stage its result through LDS
 * for the planar store -- and no fusion pass took them.  But a tensor that only convolutions and ELEMENT-WISE layers (LUT maps, Mul / Add:
 * functions of corresponding bytes, whatever the order) touch need not hold the reference's byte order at all: it is kept as
 * [H * W][C] on the device (mtensor_t.nhwc_c), the convolution reading it skips the relayout (op->nchw = 0), the one writing it stores
 * rows (op->out_nchw = 0), and the passes that follow (Add folding, paired launches) see plain NHWC convolutions.  Same values at the
 * same (channel, pixel): the reference's NCHW and NHWC kernels compute the same sums (mxu_conv.c:639-667 against :722-754).  Tensors a
 * byte-wise layer touches (MAXPOOL / CONCAT / UPSAMPLE index bytes by shape[1..3] whatever the tag: :919-1041), graph inputs and
 * outputs keep the reference's bytes.  mars_hip_read_tensor / write_tensor convert; fusion level 0 keeps every tensor as tagged. */
void nhwc_internal(mars_model_ext_t *m) {
    const int nt = (int)m->pub.header.num_tensors;
    for (int i = 0; i < nt; i++) m->mt[i].nhwc_c = m->mt[i].nhwc_hw = m->mt[i].nhwc_pitch = m->mt[i].partial = 0;
    if (m->sw.fusion < 1 || m->sw.no_nhwc_internal) return;
    unsigned char *el = (unsigned char *)calloc((size_t)nt + 1, 1);
    if (!el) return;
    for (int t = 0; t < nt; t++) { /* candidates: dense [1, C, H, W] int8 activations, C a multiple of 16 (16-byte pixel rows), not NHWC-tagged */
        const mars_tensor_t *d = &m->pub.tensors[t].desc;
        const mtensor_t *mt = &m->mt[t];
        if (mt->is_weight || mt->io_in || mt->io_out || !mt->needed || d->dtype != MARS_DTYPE_INT8 || d->format == MARS_FORMAT_NHWC || d->ndims != 4 ||
            d->shape[0] != 1 || d->shape[1] <= 0 || (d->shape[1] & 15) || d->shape[2] <= 0 || d->shape[3] <= 0)
            continue;
        if (mt->bytes != (size_t)d->shape[1] * d->shape[2] * d->shape[3]) continue; /* (what every op touches of it is checked per op below) */
        el[t] = 1;
    }
    /* CONCAT layers whose inputs and output all have the same H, W (every C3 concat of the shipped files): the reference's byte logic is
     * then a fixed function of flat indices (move.hip: concat_nchwq_kernel), computable on pixels x channels operands -- the layer's
     * slices become ONE launch (OP_CONCAT_Q) if its tensors all stay eligible, else they all keep the reference's bytes.  grp[i] = index of
     * the first slice op of op i's layer when that layer qualifies, else -1 */
    int *grp = (int *)malloc(sizeof(int) * (size_t)(m->n_ops + 1));
    if (!grp) { free(el); return; }
    for (int i = 0; i < m->n_ops; i++) grp[i] = -1;
    for (int i = 0; i < m->n_ops; i++) {
        const mars_op_t *o = &m->ops[i];
        if (o->kind != OP_CONCAT_SLICE || grp[i] != -1 || (i > 0 && m->ops[i - 1].kind == OP_CONCAT_SLICE && m->ops[i - 1].layer == o->layer)) continue;
        int n = 0, ok = 1;
        while (i + n < m->n_ops && m->ops[i + n].kind == OP_CONCAT_SLICE && m->ops[i + n].layer == o->layer) n++;
        const mars_layer_t *Ld = &m->pub.layers[o->layer].desc;
        const mars_tensor_t *od = o->t_out >= 0 ? &m->pub.tensors[o->t_out].desc : NULL;
        if (!od || n < 1 || n > 4 || (uint32_t)n != Ld->num_inputs || od->ndims != 4) ok = 0;
        for (int k = 0; k < n && ok; k++) {
            const mars_op_t *q = &m->ops[i + k];
            const mars_tensor_t *id = q->t_in[0] >= 0 ? &m->pub.tensors[q->t_in[0]].desc : NULL;
            /* slice k: runs of W bytes at offset k W, over C_out x H "pixels" (shape[1] x shape[2] of the output) */
            if (!id || id->ndims != 4 || q->t_out != o->t_out || q->t_in[0] == o->t_out || q->out_pix_stride || id->shape[2] != od->shape[2] ||
                id->shape[3] != od->shape[3] || q->in_c != od->shape[3] || q->out_c != od->shape[3] || q->ch_off != k * od->shape[3] ||
                q->out_h != od->shape[1] || q->out_w != od->shape[2] || (long)od->shape[1] * od->shape[2] * od->shape[3] > 0x7fffffffL)
                ok = 0;
            for (int k2 = 0; k2 < k && ok; k2++)
                if (m->ops[i + k2].t_in[0] == q->t_in[0]) ok = 0; /* (one tensor twice: keep it simple) */
        }
        if (ok)
            for (int k = 0; k < n; k++) grp[i + k] = i;
    }
#define DIMS_ARE(t, c, h, w) (m->pub.tensors[t].desc.shape[1] == (c) && m->pub.tensors[t].desc.shape[2] == (h) && m->pub.tensors[t].desc.shape[3] == (w))
    for (int pass = 0, changed = 1; changed && pass < nt + 2; pass++) {
        changed = 0;
        for (int i = 0; i < m->n_ops; i++) {
            const mars_op_t *o = &m->ops[i];
            if (o->kind == OP_CONCAT_SLICE && grp[i] >= 0) { /* a qualifying CONCAT layer: all of its tensors, or none */
                if (grp[i] != i) continue;
                int all = el[o->t_out];
                for (int k = i; k < m->n_ops && grp[k] == i; k++) all = all && el[m->ops[k].t_in[0]];
                if (!all) {
                    if (el[o->t_out]) { el[o->t_out] = 0; changed = 1; }
                    for (int k = i; k < m->n_ops && grp[k] == i; k++)
                        if (el[m->ops[k].t_in[0]]) { el[m->ops[k].t_in[0]] = 0; changed = 1; }
                }
                continue;
            }
            if ((o->kind == OP_UPSAMPLE || (o->kind == OP_MAXPOOL && !o->chain_n)) && o->t_in[0] >= 0 && o->t_out >= 0 && o->t_in[0] != o->t_out &&
                !o->out_pix_stride && !o->out_ch_off) {
                /* the byte-wise UPSAMPLE / stride-1 MAXPOOL as fixed functions of flat indices (move.hip *_nchwq_kernel): both tensors or neither */
                const mars_tensor_t *id = &m->pub.tensors[o->t_in[0]].desc, *od = &m->pub.tensors[o->t_out].desc;
                int fits = id->ndims == 4 && od->ndims == 4 && o->in_h == id->shape[1] && o->in_w == id->shape[2] && o->in_c == id->shape[3] &&
                           o->out_h == od->shape[1] && o->out_w == od->shape[2] && (long)o->out_h * o->out_w * o->in_c <= (long)od->shape[1] * od->shape[2] * od->shape[3];
                if (o->kind == OP_MAXPOOL)
                    fits = fits && o->sh == 1 && o->sw == 1 && o->kh >= 1 && o->kh <= 17 && o->kw >= 1 && od->shape[1] == id->shape[1] &&
                           od->shape[2] == id->shape[2] && od->shape[3] == id->shape[3];
                if (fits && el[o->t_in[0]] && el[o->t_out]) continue;
                /* (else: the generic path below takes both tensors out) */
            }
            int ts[8], n = 0, ok[8];
            for (int k = 0; k < o->n_in && k < 4; k++) { ts[n] = o->t_in[k]; ok[n++] = 0; }
            const int n_in = n;
            if (o->t_out >= 0) { ts[n] = o->t_out; ok[n++] = 0; }
            if (o->kind == OP_CONV_I8 && !o->nseg && !o->add_t && !o->pre && !o->out_pix_stride && !o->chain_n) {
                /* input side: the tagged-NCHW view of a tensor of exactly these dims; output side likewise */
                if (n_in == 1 && o->nchw && ts[0] >= 0 && el[ts[0]] && DIMS_ARE(ts[0], o->in_c, o->in_h, o->in_w) && o->c_pad == o->in_c) ok[0] = 1;
                if (o->t_out >= 0 && o->out_nchw && el[o->t_out] && DIMS_ARE(o->t_out, o->out_c, o->out_h, o->out_w) && ts[0] != o->t_out) ok[n - 1] = 1;
            } else if ((o->kind == OP_LUT_I8 || (o->kind == OP_BINARY_I8 && !o->out_pix_stride)) && o->t_out >= 0) {
                /* element-wise: every operand and the result in the same order, or none of them */
                int all = 1;
                for (int k = 0; k < n; k++)
                    if (ts[k] < 0 || !el[ts[k]] || o->n != m->mt[ts[k]].bytes || !DIMS_ARE(ts[k], m->pub.tensors[ts[0]].desc.shape[1], m->pub.tensors[ts[0]].desc.shape[2], m->pub.tensors[ts[0]].desc.shape[3]))
                        all = 0;
                for (int k = 0; k < n; k++) ok[k] = all;
            }
            for (int k = 0; k < n; k++)
                if (ts[k] >= 0 && el[ts[k]] && !ok[k]) { el[ts[k]] = 0; changed = 1; }
            for (int k = 0; k < o->chain_n && k < 3; k++)
                if (o->chain_out[k] >= 0 && el[o->chain_out[k]]) { el[o->chain_out[k]] = 0; changed = 1; }
            for (int k = 0; k < o->nseg && k < 4; k++)
                if (o->seg_t[k] >= 0 && el[o->seg_t[k]]) { el[o->seg_t[k]] = 0; changed = 1; }
        }
    }
#undef DIMS_ARE
    for (int i = 0; i < m->n_ops; i++) {
        mars_op_t *o = &m->ops[i];
        if (o->kind == OP_CONCAT_SLICE && grp[i] == i && el[o->t_out]) { /* the layer's slices -> one launch on pixels x channels operands */
            const mars_tensor_t *od = &m->pub.tensors[o->t_out].desc;
            int n = 0;
            double bytes = (double)m->mt[o->t_out].bytes;
            for (int k = i; k < m->n_ops && grp[k] == i; k++, n++) {
                o->t_in[n] = m->ops[k].t_in[0];
                bytes += (double)m->mt[m->ops[k].t_in[0]].bytes;
                if (k != i) m->ops[k].kind = -1;
            }
            o->kind = OP_CONCAT_Q;
            o->n_in = n;
            o->out_c = od->shape[1]; o->in_h = od->shape[2]; o->in_w = od->shape[3];
            o->out_h = od->shape[2]; o->out_w = od->shape[3];
            o->bytes = bytes;
            continue;
        }
        if ((o->kind == OP_UPSAMPLE || (o->kind == OP_MAXPOOL && !o->chain_n)) && o->t_in[0] >= 0 && o->t_out >= 0 && el[o->t_in[0]] && el[o->t_out]) {
            o->kind = o->kind == OP_UPSAMPLE ? OP_UPSAMPLE_Q : OP_MAXPOOL_Q; /* (the fixpoint left both tensors eligible only where the op fits) */
            continue;
        }
        if (o->kind != OP_CONV_I8) continue;
        if (o->n_in >= 1 && o->t_in[0] >= 0 && el[o->t_in[0]]) o->nchw = 0;
        if (o->t_out >= 0 && el[o->t_out]) o->out_nchw = 0;
    }
    drop_dead_ops(m);
    free(grp);
    for (int t = 0; t < nt; t++)
        if (el[t]) {
            m->mt[t].nhwc_c = m->pub.tensors[t].desc.shape[1];
            m->mt[t].nhwc_hw = m->pub.tensors[t].desc.shape[2] * m->pub.tensors[t].desc.shape[3];
            /* every layer left on it touches exactly its nominal bytes (checked above); what the replaced concat slices would have read
             * past them (their runs cover the OUTPUT's byte count) no longer counts -- with it a concat input had another frame stride than
             * its producer's other operand and the residual Add in front of a C3's concat was not folded */
            m->mt[t].extent = m->mt[t].bytes;
        }
    /* Write-only convolution results with a ragged channel count (the 255-channel Detect convolutions of the shipped files: their readers are
     * no-op layers): nothing in the graph reads them, so they too are kept pixels x channels, at a 16-byte-aligned pixel pitch (255 -> 256; the
     * pad channel has zero weights, its byte is never read) -- the convolution then takes the aligned row epilogue and the tile walkers instead
     * of the planar store through LDS.  mars_hip_read_tensor un-pads and converts. */
    for (int i = 0; i < m->n_ops; i++) {
        mars_op_t *o = &m->ops[i];
        const int T = o->t_out;
        if (o->kind != OP_CONV_I8 || !o->out_nchw || T < 0 || el[T] || (o->out_c & 15) == 0 || (o->in_c & 15) || o->out_pix_stride || o->out_ch_off ||
            o->add_t || o->nseg || o->pre)
            continue;
        const mars_tensor_t *d = &m->pub.tensors[T].desc;
        const mtensor_t *mt = &m->mt[T];
        const int P = (o->out_c + 15) & ~15;
        if (mt->is_weight || mt->io_in || mt->io_out || d->dtype != MARS_DTYPE_INT8 || d->format == MARS_FORMAT_NHWC || d->ndims != 4 || d->shape[0] != 1 ||
            d->shape[1] != o->out_c || d->shape[2] != o->out_h || d->shape[3] != o->out_w || P > o->oc_pad ||
            mt->bytes != (size_t)o->out_c * o->out_h * o->out_w || mt->extent != mt->bytes)
            continue;
        if (touched_by_other(m, T, i, i)) continue; /* any other op that reads or writes it keeps it as tagged (op i itself: no convolution reads its own result) */
        o->out_nchw = 0;
        o->out_pix_stride = P;
        o->store_c = P;
        m->mt[T].nhwc_c = o->out_c;
        m->mt[T].nhwc_hw = o->out_h * o->out_w;
        m->mt[T].nhwc_pitch = P;
        touch(m, T, (size_t)o->out_h * o->out_w * P);
    }
    free(el);
}

/* The reference's CONCAT on NCHW-tagged maps of equal size is a shift of its LAST input by N - 1 map rows (move.hip: concat_nchwq_kernel):
 *   out(c, h, w) = in_last(c, h - (N - 1), w)  for h >= N - 1 and c < C_last,   0 for c >= C_last;   the first N - 1 rows are irregular.
 * When its only reader is a plain 1 x 1 convolution X (C3's cv3, SPPF's cv2 in the shipped files), X over rows h >= N - 1 is the SAME
 * convolution over in_last with its K loop cut to the C_last channels that are not zero, its output N - 1 rows further down:
 *   - the concat produces its first N - 1 rows only (rows_only; the tensor becomes `partial`),
 *   - X is split in two launches: rows 0 .. N - 2 from those rows (all channels, the original weights), rows N - 1 .. H - 1 straight from
 *     in_last (a second weight image: the first C_last input channels).
 * The concat's copy of the whole map and the zero half (or three quarters) of X's K loop go.  Same bytes out: every output row is the sum
 * the reference computes, over exactly the non-zero terms. */
void virtual_concat_q(mars_model_ext_t *m) {
    if (m->sw.fusion < 1 || m->sw.no_vconcat_q) return;
    for (int i = 0; i < m->n_ops; i++) {
        mars_op_t *cq = &m->ops[i];
        if (cq->kind != OP_CONCAT_Q || cq->n_in < 2 || cq->rows_only) continue;
        const int T = cq->t_out, N = cq->n_in, H = cq->in_h, W = cq->in_w, Cout = cq->out_c;
        const int TL = cq->t_in[N - 1];
        const int CL = m->mt[TL].nhwc_c;
        if (H < N + 1 || CL <= 0 || (CL & 15) || CL >= Cout || m->mt[TL].nhwc_pitch || m->mt[T].nhwc_pitch) continue;
        int r = -1, nr = 0, bad = 0;
        for (int j = 0; j < m->n_ops; j++) {
            const mars_op_t *o = &m->ops[j];
            for (int k = 0; k < o->n_in; k++)
                if (o->t_in[k] == T) { nr++; if (r < 0) r = j; }
            if (j != i && op_writes(o, T)) bad = 1;
        }
        if (bad || r <= i || nr < 1 || nr > 2) continue;
        /* one reader, or the two of a paired launch (a head C3's cv1 + cv2: both are split, both halves stay pairs) */
        int g[4];
        const int form = op_form(m, r, g), np = op_span(m, r);
        if ((form != FORM_PLAIN && form != FORM_PAIR && form != FORM_BOTH) || nr != np || op_is_mate(m, r) || (np == 2 && m->ops[r + 1].t_in[0] != T)) continue;
        int ok = 1;
        for (int q = 0; q < np && ok; q++) {
            const mars_op_t *cv = &m->ops[r + q];
            if (cv->kind != OP_CONV_I8 || cv->kh != 1 || cv->kw != 1 || cv->sh != 1 || cv->sw != 1 || cv->pt || cv->pl || cv->nchw || cv->out_nchw ||
                cv->nseg || cv->add_t || cv->pre || cv->out_pix_stride || cv->out_ch_off ||
                cv->n_in != 1 || cv->in_c != Cout || cv->in_h != H || cv->in_w != W || cv->out_h != H || cv->out_w != W || cv->in_byte_off ||
                cv->out_byte_off || cv->t_out == TL || cv->t_out == T || (cv->out_c & 15) || m->mt[cv->t_out].nhwc_pitch)
                ok = 0;
        }
        if (!ok) continue;
        if (touched_between(m, i + 1, r + np, TL, USE_WRITE)) continue; /* in_last must still hold at the readers what it held at the concat */
        /* the second weight images: input channels [0, C_last) of every output channel (1 x 1: OIHW and OHWI coincide) */
        size_t w_off2[2] = {NO_OFF, NO_OFF};
        int row_pad2 = 0;
        for (int q = 0; q < np && ok; q++) {
            const mars_op_t *cv = &m->ops[r + q];
            const mars_layer_t *L = &m->pub.layers[cv->layer].desc;
            const int tw = find_tensor(m, L->params.conv.weight_tensor_id);
            int oc_pad2, c_eff2;
            mhip_conv_i8_pack_geom(CL, 1, cv->out_c, &row_pad2, &oc_pad2, &c_eff2);
            if (tw < 0 || oc_pad2 != cv->oc_pad || c_eff2 != CL) { ok = 0; break; }
            const size_t k64 = ALIGN_UP((size_t)row_pad2, 64);
            w_off2[q] = arena_reserve(m, (size_t)oc_pad2 * k64);
            if (w_off2[q] == NO_OFF) return;
            cv = &m->ops[r + q];
            if (!m->deferred) {
                const size_t full = (size_t)cv->out_c * Cout, cut = (size_t)cv->out_c * CL;
                int8_t *tmp = (int8_t *)malloc(full ? full : 1), *sel = (int8_t *)malloc(cut ? cut : 1);
                if (!tmp || !sel) { free(tmp); free(sel); m->plan_err = MARS_ERR_ALLOC_FAILED; return; }
                blob_read(m, (size_t)m->pub.tensors[tw].desc.data_offset, full, tmp);
                for (int oc = 0; oc < cv->out_c; oc++) memcpy(sel + (size_t)oc * CL, tmp + (size_t)oc * Cout, (size_t)CL);
                mars_pack_conv_i8(sel, cut, 1, cv->out_c, CL, 1, 1, c_eff2, row_pad2, oc_pad2, (int8_t *)m->arena_host + w_off2[q]);
                free(tmp); free(sel);
            }
        }
        if (!ok) continue; /* (an image reserved for the first of a pair stays unused: a few KB of the arena) */
        /* ops: [concat: first N - 1 rows] ... [the readers over those rows] [the readers over in_last] */
        while (m->n_ops + np > m->cap_ops) {
            const int cap = m->cap_ops * 2;
            mars_op_t *npp = (mars_op_t *)realloc(m->ops, (size_t)cap * sizeof(mars_op_t));
            if (!npp) { m->plan_err = MARS_ERR_ALLOC_FAILED; return; }
            m->ops = npp; m->cap_ops = cap;
        }
        cq = &m->ops[i];
        memmove(&m->ops[r + 2 * np], &m->ops[r + np], sizeof(mars_op_t) * (size_t)(m->n_ops - r - np));
        m->n_ops += np;
        for (int q = np - 1; q >= 0; q--) m->ops[r + np + q] = m->ops[r + q]; /* (np == 2: [a b] -> [a b a b]) */
        for (int q = 0; q < np; q++) {
            mars_op_t *top = &m->ops[r + q], *mainop = &m->ops[r + np + q];
            top->in_h = top->out_h = N - 1;
            top->macs = top->macs * (N - 1) / H;
            top->bytes = (double)(N - 1) * W * (Cout + top->out_c);
            top->w2_off = NO_OFF; top->w2_rows = 0;
            mainop->t_in[0] = TL;
            mainop->in_c = CL; mainop->c_pad = CL; mainop->row_pad = row_pad2;
            mainop->in_h = mainop->out_h = H - (N - 1);
            mainop->w_off = w_off2[q];
            mainop->w2_off = NO_OFF; mainop->w2_rows = 0;
            mainop->out_byte_off = (size_t)(N - 1) * W * (size_t)mainop->out_c;
            mainop->macs = (double)(H - (N - 1)) * W * mainop->out_c * CL;
            mainop->bytes = (double)(H - (N - 1)) * W * (CL + mainop->out_c);
            mainop->variant = 0;
        }
        cq->rows_only = N - 1;
        cq->bytes = (double)(N - 1) * W * Cout * 2.0;
        m->mt[T].partial = 1;
    }
}

/* Residual Add folded into the convolution that produces one of its operands (the bottleneck shortcut of C3):
 * out = Add(conv_result, x) is evaluated in the convolution's epilogue with the reference's float steps
 * (mars_runtime.c ADD branch: (a*sa + b*sb) * (1/so) + 0.5f, truncated, saturated), reading x where the output
 * goes.  Saves writing the convolution result and reading it back.  Conditions: the convolution result has no
 * other reader, x and the Add output have the same dense layout and frame stride, nothing touches them in
 * between, and the scales keep the float -> int conversion in range (so no x86 fix-up is needed).
 * The float32 form: Add(conv_f32 result, x) (reference mars_runtime.c:807-816: out[i] = a[i] + b[i]) evaluated where the
 * convolution stores -- one float add behind the (fused) SiLU, the same float the separate layer computes from the same two
 * floats, so every kernel form stays what it was (the exact-order kernel bit-identical).  Saves a write and two reads of
 * the tensor per bottleneck (7 launches, 7 % of the float32 twin's step).  It needs none of the int8 form's layout conditions. */
void fold_add(mars_model_ext_t *m, int f32) {
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int j = 0; j < m->n_ops; j++) {
        mars_op_t *ad = &m->ops[j];
        if (ad->kind != (f32 ? OP_BINARY_F32 : OP_BINARY_I8) || ad->is_mul || ad->n_in != 2 || (!f32 && ad->out_pix_stride)) continue;
        for (int side = 0; side < 2; side++) {
            const int A = ad->t_in[side], X = ad->t_in[1 - side], O = ad->t_out;
            if (A < 0 || X < 0 || O < 0 || A == X || O == X || O == A) continue;
            if (readers[A] != 1 || writers[A] != 1 || m->mt[A].io_in || m->mt[A].io_out || m->mt[A].is_weight) continue;
            if (m->mt[X].is_weight || m->mt[O].is_weight || writers[O] != 1) continue;
            const int i = writer_before(m, A, j);
            if (i < 0) continue;
            mars_op_t *c = &m->ops[i];
            if (c->kind != (f32 ? OP_CONV_F32 : OP_CONV_I8) || c->add_t || c->n_in != 1) continue;
            if (!f32 && (c->out_nchw || !c->safe || c->out_pix_stride || (c->out_c & 15) || (c->in_c & 15) || c->nseg)) continue;
            if (ad->n != (size_t)c->out_h * c->out_w * c->out_c) continue;
            if (c->t_in[0] == O) continue; /* add(conv(X), Y) -> X: sequential in the reference, a race when fused */
            const float s_conv = side == 0 ? ad->f0 : ad->f1, s_other = side == 0 ? ad->f1 : ad->f0, inv = ad->f2;
            if (!f32) { /* the int8 epilogue reads x where the output goes, and converts float -> int without the x86 fix-up */
                if (planned_stride(&m->mt[X]) != planned_stride(&m->mt[O])) continue;
                const double bound = 128.0 * (fabs((double)s_conv) + fabs((double)s_other)) * fabs((double)inv) + 1.0;
                if (!(bound < 2147483000.0)) continue; /* also rejects NaN / inf */
            }
            /* x must be complete before the convolution runs, and nothing in between may touch the Add's output */
            if (touched_between(m, i, j + 1, X, USE_WRITE) || touched_between(m, i + 1, j, O, USE_READ | USE_WRITE)) continue;
            c->t_out = O;
            c->add_t = X + 1;
            if (!f32) { c->add_s_conv = s_conv; c->add_s_other = s_other; c->add_inv = inv; }
            c->t_in[c->n_in++] = X;
            c->bytes += (f32 ? 4.0 : 1.0) * (double)ad->n;
            m->mt[A].needed = 0;
            ad->kind = -1;
            readers[A] = 0;
            break;
        }
    }
    drop_dead_ops(m);
    free(readers);
}

/* Fused C3 bottleneck: conv1x1 + SiLU (A) whose only reader is the k x k convolution B right behind it (B usually
 * carries the folded residual Add of A's input) -> B evaluates A on its staged input patch (conv_i8_patch<PRE>); A's
 * output tensor is never written.  Same bytes: B sees, at every in-image pixel of its window, exactly the int8 value A
 * would have stored there, and zeros outside the image as its SAME padding prescribes.  Only where the device code can
 * take it (mhip_conv_i8_pre_ok: stride 1, 32 / 64 channels, patch fits); everything else keeps the two launches.
 * Fusion level 2 only: measured on the yolov5s twin it removes 4 launches (batch 1: 0.494 -> 0.485 ms) but returns
 * nothing at batch 256 -- these 32 / 64-channel layers are bound by the requantisation's vector instructions, not by
 * the bytes the fusion saves, and the halo makes the fused kernel requantise 1.3x the pixels. */
void fuse_bottleneck(mars_model_ext_t *m) {
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 1 < m->n_ops; i++) {
        mars_op_t *a = &m->ops[i], *b = &m->ops[i + 1];
        if (a->kind != OP_CONV_I8 || b->kind != OP_CONV_I8 || a->pre || b->pre) continue;
        const int T = a->t_out;
        if (T < 0 || b->t_in[0] != T || readers[T] != 1 || m->mt[T].io_in || m->mt[T].io_out || m->mt[T].is_weight) continue;
        if (a->kh != 1 || a->kw != 1 || a->sh != 1 || a->sw != 1 || a->nchw || b->nchw || a->out_nchw || b->out_nchw || !a->safe || !b->safe || a->nseg || b->nseg ||
            a->add_t || a->n_in != 1 || a->out_pix_stride || a->relu || a->lut2_off == NO_OFF || b->lut2_off == NO_OFF ||
            a->in_c != a->out_c || a->out_c != b->in_c || (a->in_c != 32 && a->in_c != 64) || b->sh != 1 || b->sw != 1 ||
            a->in_h != b->in_h || a->in_w != b->in_w || a->b_off == NO_OFF || !op_plain(m, i) || !op_plain(m, i + 1) || op_is_mate(m, i))
            continue;
        const int X = a->t_in[0];
        if (X < 0 || X == b->t_out || m->mt[X].is_weight) continue;
        if (!conv_i8_pre_fits(b, 1, 0, 0)) continue; /* one frame, no strides: alloc_batch asks again for its batch */
        b->pre = 1;
        b->pre_w_off = a->w_off; b->pre_b_off = a->b_off; b->pre_lut2_off = a->lut2_off; b->pre_cs = a->cs;
        b->t_in[0] = X;
        b->macs += a->macs;
        m->mt[T].needed = 0;
        readers[T] = 0;
        a->kind = -1;
    }
    drop_dead_ops(m);
    free(readers);
}

/* C3's cv3 inside the k x k convolution that feeds it: A = the last bottleneck's k x k convolution (with its folded residual Add where there is
 * one), whose result u only B reads, B = the 1 x 1 right behind it over the virtual concat {u, y2}.  A's launch (conv_i8_patch<POST>) holds a
 * tile row of u as the B operand of B's first K part the moment it is requantised, reads the same pixels of y2, and stores B's result: u is
 * never written nor read back, and one launch goes.  Same bytes: B sees exactly the int8 values A would have stored, no halo is involved.
 * Both ops stay in the plan (as a pair's do): A carries post_next and is launched, B is skipped.  Only where the device code takes it
 * (mhip_conv_i8_post_ok: 32 / 64 channels in one channel tile, mostly full tiles); a decision on shapes alone -- alloc_batch takes it back for
 * a batch whose output offsets leave 31 bits (m->no_post). */
void fuse_post(mars_model_ext_t *m) {
    if (m->sw.no_post || m->no_post) return;
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 1 < m->n_ops; i++) {
        mars_op_t *a = &m->ops[i], *b = &m->ops[i + 1];
        if (a->kind != OP_CONV_I8 || b->kind != OP_CONV_I8 || a->pre || b->pre || !op_plain(m, i) || !op_plain(m, i + 1) || op_is_mate(m, i)) continue;
        const int c = a->out_c, T = a->t_out, O = b->t_out;
        if ((c != 32 && c != 64) || a->oc_pad != c || a->kh * a->kw < 2 || a->sh != 1 || a->sw != 1 || !a->safe || a->nchw || a->out_nchw || a->nseg ||
            a->out_pix_stride || a->out_ch_off || a->store_c || a->chain_n || a->in_byte_off || a->out_byte_off || a->lut_off == NO_OFF ||
            a->lut2_off == NO_OFF || a->n_in >= 4)
            continue;
        if (b->kh != 1 || b->kw != 1 || b->sh != 1 || b->sw != 1 || b->pt || b->pl || !b->safe || b->nchw || b->out_nchw || b->add_t || b->chain_n ||
            b->store_c || b->in_byte_off || b->lut_off == NO_OFF || b->lut2_off == NO_OFF || b->nseg != 2 || b->seg_up || b->seg_t[0] != T ||
            b->seg_c[0] != c || b->seg_c[1] != c || b->in_c != 2 * c || b->out_c != 2 * c || b->oc_pad != 2 * c || b->row_pad != 2 * c ||
            b->in_h != a->out_h || b->in_w != a->out_w || b->out_h != a->out_h || b->out_w != a->out_w)
            continue;
        const int Y = b->seg_t[1];
        if (T < 0 || O < 0 || Y < 0 || Y == T || O == T || O == Y || readers[T] != 1 || writers[T] != 1 || m->mt[T].io_in || m->mt[T].io_out ||
            m->mt[T].is_weight || m->mt[T].tail_read || m->mt[Y].is_weight || m->mt[Y].pix_stride ||
            m->mt[Y].bytes != (size_t)a->out_h * a->out_w * c || op_reads(a, O) || op_reads(a, Y))
            continue;
        const mars_op_t *g[4] = {a, b};
        if (!conv_i8_group_fits(m, FORM_POST, g, 0, 1)) continue;
        const size_t bytes = mhip_conv_i8_post_pack(c, NULL, NULL, NULL);
        const size_t off = arena_reserve(m, bytes); /* (may move the arena: pointers are taken afterwards) */
        if (off == NO_OFF) break;
        mhip_conv_i8_post_pack(c, (const int8_t *)(m->arena_host + b->w_off), b->b_off != NO_OFF ? (const int32_t *)(m->arena_host + b->b_off) : NULL,
                               (int8_t *)(m->arena_host + off));
        a->post_next = 1;
        a->post_w_off = off;
        a->t_in[a->n_in++] = Y; /* (operand model: the launch reads y2) */
        m->mt[T].needed = 0;
        readers[T] = 0;
        readers[Y]++;
        i++; /* B is taken */
    }
    free(readers);
}

/* C3's cv1 + cv2 inside the k x k convolution that feeds them: A = a k x k convolution (stride 1 or 2) to 64 channels whose result T only the
 * two members B, C of the paired launch right behind it read (1 x 1, 64 -> 32 channels each).  A's launch (conv_i8_patch<SPLIT>) holds a tile
 * row of T as the B operand of both 1 x 1s' only K step the moment it is requantised and stores their results: T is never written nor read
 * back, and the pair launch goes.  Same bytes: B and C see exactly the int8 values A would have stored.  All three ops stay in the plan: A
 * carries split_next and is launched, B (which keeps pair_next) and C are skipped.  B and C write dense tensors: pair_convs forms no pair that
 * writes a channel slice, and one that has been given a byte offset or padded rows is declined here.  Only where the device code takes it
 * (mhip_conv_i8_split_ok); alloc_batch takes the decision back for a batch whose output offsets leave 31 bits (m->no_split). */
/* the mate every fused 1x1 form takes: a plain SiLU 1 x 1 from in_c to out_c channels over a's output map, dense on both sides, with a half-step
 * table.  Shape only: whether d is free (no head, no mate of another launch) and which tensor it reads is the caller's question */
static int free_1x1_ok(const mars_op_t *d, const mars_op_t *a, int in_c, int out_c) {
    return d->kind == OP_CONV_I8 && d->kh == 1 && d->kw == 1 && d->sh == 1 && d->sw == 1 && !d->pt && !d->pl && d->safe && !d->nchw && !d->out_nchw && !d->add_t &&
           !d->chain_n && !d->store_c && !d->in_byte_off && !d->out_byte_off && !d->out_pix_stride && !d->out_ch_off && d->lut_off != NO_OFF &&
           d->lut2_off != NO_OFF && !d->nseg && !d->pre && d->n_in == 1 && d->in_c == in_c && d->out_c == out_c && d->oc_pad == out_c && d->row_pad == in_c &&
           d->in_h == a->out_h && d->in_w == a->out_w && d->out_h == a->out_h && d->out_w == a->out_w;
}
void fuse_split(mars_model_ext_t *m) {
    if (m->sw.no_split || m->no_split) return;
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 2 < m->n_ops; i++) {
        mars_op_t *a = &m->ops[i], *b = &m->ops[i + 1], *c = &m->ops[i + 2];
        int gi[4];
        if (a->kind != OP_CONV_I8 || a->pre || !op_plain(m, i) || op_form(m, i + 1, gi) != FORM_PAIR || !op_plain(m, i + 2) || op_is_mate(m, i)) continue;
        const int T = a->t_out;
        if (a->out_c != 64 || a->oc_pad != 64 || a->kh * a->kw < 2 || (a->sh != 1 && a->sh != 2) || a->sw != a->sh || !a->safe || a->nchw || a->out_nchw ||
            a->nseg || a->out_pix_stride || a->out_ch_off || a->store_c || a->chain_n || a->in_byte_off || a->out_byte_off || a->add_t ||
            a->lut_off == NO_OFF || a->lut2_off == NO_OFF || a->n_in != 1)
            continue;
        if (T < 0 || !free_1x1_ok(b, a, 64, 32) || !free_1x1_ok(c, a, 64, 32) || b->t_in[0] != T || c->t_in[0] != T) continue;
        const int O0 = b->t_out, O1 = c->t_out;
        if (O0 < 0 || O1 < 0 || O0 == O1 || O0 == T || O1 == T || readers[T] != 2 || writers[T] != 1 || m->mt[T].io_in || m->mt[T].io_out ||
            m->mt[T].is_weight || m->mt[T].tail_read || m->mt[O0].pix_stride || m->mt[O1].pix_stride || op_reads(a, O0) || op_reads(a, O1))
            continue;
        const mars_op_t *g[4] = {a, b, c};
        if (!conv_i8_group_fits(m, FORM_SPLIT, g, 0, 1)) continue;
        const size_t bytes = mhip_conv_i8_split_pack(NULL, NULL, NULL, NULL, NULL);
        const size_t off = arena_reserve(m, bytes); /* (may move the arena: pointers are taken afterwards) */
        if (off == NO_OFF) break;
        mhip_conv_i8_split_pack((const int8_t *)(m->arena_host + b->w_off), b->b_off != NO_OFF ? (const int32_t *)(m->arena_host + b->b_off) : NULL,
                                (const int8_t *)(m->arena_host + c->w_off), c->b_off != NO_OFF ? (const int32_t *)(m->arena_host + c->b_off) : NULL,
                                (int8_t *)(m->arena_host + off));
        a->split_next = 1;
        a->split_w_off = off;
        m->mt[T].needed = 0;
        i += 2; /* B and C are taken */
    }
    free(readers);
}

/* op `from` moves up to position `to` (<= from); the ops in between move one down */
static void move_up(mars_model_ext_t *m, int to, int from) {
    const mars_op_t moved = m->ops[from];
    memmove(&m->ops[to + 1], &m->ops[to], sizeof(mars_op_t) * (size_t)(from - to));
    m->ops[to] = moved;
}

/* The search both chain passes share.  The launch at i has the members of `form` but the last; its two sides are the last two of them.  D = the
 * first free 1 x 1 from c to c channels, at most 48 ops behind i, that reads exactly one side, writes a plain tensor of its own that only it
 * writes, may move up behind the members under pair_up's rule (nothing in between touches its output or writes its input), and with which the
 * device code takes the form at one frame.  -> D's index and *side = the side it reads (1 | 2); -1 = there is none.  Nothing is changed: the
 * caller reserves what the form needs, then moves D up (move_up) and sets its flag */
static int find_chained_1x1(const mars_model_ext_t *m, int i, int form, int c, const int *writers, int *side_out) {
    const int n = form_span(form) - 1, O0 = m->ops[i + n - 2].t_out, O1 = m->ops[i + n - 1].t_out;
    const mars_op_t *a = &m->ops[i], *g[4] = {a, a + 1, a + 2, NULL};
    for (int j = i + n; j < m->n_ops && j <= i + 48; j++) {
        const mars_op_t *d = &m->ops[j];
        if (!free_1x1_ok(d, a, c, c) || !op_plain(m, j) || op_is_mate(m, j)) continue; /* (a head or a mate of another launch is not D) */
        const int side = d->t_in[0] == O0 ? 1 : (d->t_in[0] == O1 ? 2 : 0), O = d->t_out;
        if (!side || O < 0 || O == O0 || O == O1 || O == a->t_out || writers[O] != 1 || m->mt[O].io_in || m->mt[O].is_weight || m->mt[O].pix_stride || op_reads(d, O))
            continue;
        int reads = 0;
        for (int k = 0; k < n; k++) reads |= op_reads(&a[k], O);
        if (reads || touched_between(m, i + n, j, O, USE_READ | USE_WRITE) || touched_between(m, i + n, j, d->t_in[0], USE_WRITE)) continue;
        g[n] = d;
        if (!conv_i8_group_fits(m, form, g, side, 1)) continue;
        *side_out = side;
        return j;
    }
    return -1;
}

/* The bottleneck's m.cv1 inside the launch that already runs cv1 + cv2: A carries split_next with mates B and C; D = a 1 x 1 SiLU convolution from 32
 * to 32 channels that reads exactly B's or C's output over the same map.  A's launch (conv_i8_patch<CHAIN>) holds that side's requantised tile row
 * in registers the moment it stores it: it is the B operand of D's only K step.  D's input is still written (other ops read it: cv1's tensor is the
 * bottleneck's shortcut), only D's read of it and D's launch go.  Same bytes: D sees exactly the int8 values its input tensor holds.  All four ops
 * stay in the plan: A records the side (split_chain = 1 for B's, 2 for C's) and the image, D is skipped by the run loop like B and C.  D is moved up
 * behind C under pair_up's rule (nothing in between touches its output or writes its input); the first op that qualifies is taken.  Only where the
 * device code takes it (conv_i8_group_fits); alloc_batch takes the decision back for a batch whose output offsets leave 31 bits (m->no_chain). */
void fuse_split_chain(mars_model_ext_t *m) {
    if (m->sw.no_chain || m->no_chain || m->sw.no_split || m->no_split) return;
    int *readers, *writers, g[4];
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 3 < m->n_ops; i += op_span(m, i)) {
        mars_op_t *a = &m->ops[i];
        if (a->kind != OP_CONV_I8 || op_form(m, i, g) != FORM_SPLIT) continue;
        int side;
        const int j = find_chained_1x1(m, i, FORM_SPLIT_CHAIN, 32, writers, &side);
        if (j < 0) continue;
        const size_t bytes = mhip_conv_i8_chain_pack(NULL, NULL, NULL);
        const size_t off = arena_reserve(m, bytes); /* (may move the arena: pointers are taken afterwards) */
        if (off == NO_OFF) break;
        move_up(m, i + 3, j);
        const mars_op_t *d = &m->ops[i + 3];
        mhip_conv_i8_chain_pack((const int8_t *)(m->arena_host + d->w_off), d->b_off != NO_OFF ? (const int32_t *)(m->arena_host + d->b_off) : NULL,
                                (int8_t *)(m->arena_host + off));
        a->split_chain = side;
        a->chain_w_off = off;
    }
    free(readers);
}

/* The bottleneck's m.cv1 inside a one-tile pair: A carries pair_both with its mate B right behind it; D = a 1 x 1 SiLU convolution from 64 to 64
 * channels that reads exactly A's or B's output over the same map.  The side's waves (conv_i8_persist<CHAIN>) hold its requantised bytes in
 * registers the moment they store them: they are the B operand of D's only K step.  D's launch and its read of the side go.  Where D is the
 * side's ONLY reader and the side is no graph output (the neck's C3: no shortcut), the side is not stored either and its tensor is not
 * allocated (both_elide; as fuse_split's k x k result).  Same bytes: D sees exactly the int8 values its input tensor holds, or would hold.
 * All three ops stay in the plan: A records the side (both_chain = 1 for its own, 2 for B's), D is moved up behind B under pair_up's rule and
 * skipped by the run loop like B.  It reads D's own packed weights and bias rows: no second image.  Only where the device code takes it
 * (conv_i8_group_fits); alloc_batch takes the decision back for a batch whose output offsets leave 31 bits (m->no_both_chain). */
void fuse_both_chain(mars_model_ext_t *m) {
    if (m->sw.no_both_chain || m->no_both_chain || m->sw.no_both || m->no_both) return;
    int *readers, *writers, g[4];
    if (!use_counts(m, &readers, &writers)) return;
    for (int i = 0; i + 2 < m->n_ops; i += op_span(m, i)) {
        mars_op_t *a = &m->ops[i];
        if (a->kind != OP_CONV_I8 || op_form(m, i, g) != FORM_BOTH || a->in_byte_off || a[1].in_byte_off || a->out_byte_off || a[1].out_byte_off) continue;
        int side;
        const int j = find_chained_1x1(m, i, FORM_BOTH_CHAIN, 64, writers, &side);
        if (j < 0) continue;
        move_up(m, i + 2, j);
        a->both_chain = side;
        const int S = a[side - 1].t_out;
        if (readers[S] == 1 && writers[S] == 1 && !m->mt[S].io_in && !m->mt[S].io_out && !m->mt[S].is_weight && !m->mt[S].tail_read) {
            a->both_elide = 1;
            m->mt[S].needed = 0;
        }
    }
    free(readers);
}

/* Ragged pixel rows of graph outputs (the 255-channel YOLO heads) are kept at a 16-byte-aligned pitch on the device:
 * the producing convolution then takes the aligned epilogue (16-byte stores straight from registers, every launch
 * form) instead of the LDS-staged copy-out with 8+4+2+1-byte row tails.  Only tensors nothing in the graph reads:
 * their readers are the detection tail (told the pitch) and the download / read entry points (2-D copies), so hosts
 * still see the reference's dense [H][W][C] bytes.  The pad channels carry zero weights; their bytes are never read. */
void pad_output_rows(mars_model_ext_t *m) {
    for (uint32_t i = 0; i < m->pub.header.num_tensors; i++) m->mt[i].pix_c = m->mt[i].pix_stride = 0;
    if (m->sw.no_rowpad) return;
    for (int i = 0; i < m->n_ops; i++) {
        mars_op_t *o = &m->ops[i];
        if (o->kind != OP_CONV_I8 || o->out_nchw || o->out_pix_stride || o->out_ch_off || o->add_t || o->t_out < 0 ||
            (o->out_c & 15) == 0 || (o->in_c & 15) != 0)
            continue;
        mtensor_t *t = &m->mt[o->t_out];
        const int P = (o->out_c + 15) & ~15;
        const size_t px = (size_t)o->out_h * o->out_w;
        if (!t->io_out || t->io_in || P > o->oc_pad || t->bytes != px * (size_t)o->out_c || (px * P) % 256 != 0) continue;
        if (touched_by_other(m, o->t_out, i, i)) continue; /* any other op touching the tensor keeps it dense */
        o->out_pix_stride = P;
        o->store_c = P;
        t->pix_c = o->out_c;
        t->pix_stride = P;
        if (px * P > t->extent) t->extent = px * P;
    }
}

/* Virtual concat: when every reader of a Concat output is a plain 1x1 convolution, the concat tensor is never
 * written -- the convolution's K loop takes each run of channels straight from the tensor that owns it
 * (conv_i8_persist<SEG>).  The slice copies disappear and every producer keeps writing dense rows.  Same bytes
 * as the reference: the copy would have put pixel p, channels [off, off+in_c) of the concat tensor = pixel p of the
 * input, which is exactly what the segmented read fetches (checked: nothing rewrites an input between the copy's
 * position and the last reader). */
void virtual_concat(mars_model_ext_t *m) {
    const int nt = (int)m->pub.header.num_tensors;
    for (int T = 0; T < nt; T++) {
        const mtensor_t *mt = &m->mt[T];
        if (mt->is_weight || mt->io_in || mt->io_out) continue;
        int sl[4], ns = 0, bad = 0, first_reader = -1, last_reader = -1, last_slice = -1;
        for (int i = 0; i < m->n_ops && !bad; i++) {
            const mars_op_t *o = &m->ops[i];
            if (o->t_out == T) {
                if (o->kind != OP_CONCAT_SLICE || ns >= 4) bad = 1;
                else { sl[ns++] = i; last_slice = i; }
            }
            for (int k = 0; k < o->n_in; k++)
                if (o->t_in[k] == T) {
                    if (o->kind != OP_CONV_I8 || k != 0 || o->n_in != 1 || o->nchw || o->kh != 1 || o->kw != 1 || o->sh != 1 ||
                        o->sw != 1 || o->pt || o->pl || !o->safe || o->nseg || (o->out_c & 15) || o->in_h != o->out_h ||
                        o->in_w != o->out_w || (o->in_c & (o->in_c - 1)) != 0 || o->add_t) /* the tile walker: K position by
                                                                                            * shifts, no folded Add */
                        bad = 1;
                    if (first_reader < 0) first_reader = i;
                    last_reader = i;
                }
        }
        if (bad || ns < 2 || first_reader < 0 || last_slice > first_reader) continue;
        /* slices in channel order, tiling [0, out_c) in multiples of 32, all over the same pixels */
        for (int a = 0; a < ns; a++)
            for (int b = a + 1; b < ns; b++)
                if (m->ops[sl[b]].ch_off < m->ops[sl[a]].ch_off) { int t = sl[a]; sl[a] = sl[b]; sl[b] = t; }
        int c = 0;
        const mars_op_t *s0 = &m->ops[sl[0]];
        for (int a = 0; a < ns && !bad; a++) {
            const mars_op_t *o = &m->ops[sl[a]];
            if (o->ch_off != c || (o->in_c & 31) || o->out_h != s0->out_h || o->out_w != s0->out_w || o->out_c != s0->out_c ||
                o->t_in[0] == T || o->t_in[0] < 0)
                bad = 1;
            c += o->in_c;
            /* the input must still hold at the last reader what it held where the copy stood */
            if (!bad && touched_between(m, sl[a] + 1, last_reader + 1, o->t_in[0], USE_WRITE)) bad = 1;
        }
        if (bad || c != s0->out_c) continue;
        for (int i = 0; i < m->n_ops && !bad; i++) {
            const mars_op_t *o = &m->ops[i];
            if (o->kind == OP_CONV_I8 && o->n_in == 1 && o->t_in[0] == T &&
                (o->in_c != c || (size_t)o->in_h * o->in_w != (size_t)s0->out_h * s0->out_w))
                bad = 1;
        }
        if (bad) continue;
        for (int i = 0; i < m->n_ops; i++) {
            mars_op_t *o = &m->ops[i];
            if (o->kind != OP_CONV_I8 || o->n_in != 1 || o->t_in[0] != T) continue;
            o->nseg = ns;
            o->n_in = ns;
            for (int a = 0; a < ns; a++) {
                o->seg_t[a] = o->t_in[a] = m->ops[sl[a]].t_in[0];
                o->seg_c[a] = m->ops[sl[a]].in_c;
            }
        }
        for (int a = 0; a < ns; a++) m->ops[sl[a]].kind = -1;
        m->mt[T].needed = 0;
        /* a segment that is a 2x2 nearest upsample (reference :1003-1044) of a half-size tensor, read by nothing
         * else: the convolution reads the half-size tensor at pixel (y/2, x/2) and the upsample launch goes too */
        for (int a = 0; a < ns; a++) {
            const int S = m->ops[sl[a]].t_in[0];
            int up = -1, nread = 0, nwrite = 0, ok = 1;
            for (int i = 0; i < m->n_ops; i++) {
                const mars_op_t *o = &m->ops[i];
                if (o->kind == -1) continue;
                if (o->t_out == S) { nwrite++; up = i; }
                for (int k = 0; k < o->n_in; k++)
                    if (o->t_in[k] == S && !(o->kind == OP_CONV_I8 && o->nseg == ns && o->seg_t[a] == S)) nread++;
            }
            if (nwrite != 1 || nread != 0 || up < 0 || m->mt[S].io_out || m->mt[S].io_in || m->mt[S].is_weight) continue;
            const mars_op_t *u = &m->ops[up];
            if (u->kind != OP_UPSAMPLE || u->out_pix_stride || u->scale_h != 2 || u->scale_w != 2 || u->out_h != 2 * u->in_h ||
                u->out_w != 2 * u->in_w || u->in_c != m->ops[sl[a]].in_c || u->out_h != s0->out_h || u->out_w != s0->out_w)
                continue;
            const int U = u->t_in[0];
            if (U < 0 || U == S) continue;
            int last = -1;
            for (int i = 0; i < m->n_ops; i++)
                if (m->ops[i].kind == OP_CONV_I8 && m->ops[i].nseg == ns && m->ops[i].seg_t[a] == S) last = i;
            for (int i = up; i <= last && ok; i++)
                if (m->ops[i].kind != -1 && m->ops[i].t_out == U) ok = 0; /* the half-size tensor must stay as it was */
            if (!ok) continue;
            for (int i = 0; i < m->n_ops; i++) {
                mars_op_t *o = &m->ops[i];
                if (o->kind == OP_CONV_I8 && o->nseg == ns && o->seg_t[a] == S) {
                    o->seg_t[a] = o->t_in[a] = U;
                    o->seg_up |= 1 << a;
                }
            }
            m->ops[up].kind = -1;
            m->mt[S].needed = 0;
        }
    }
    drop_dead_ops(m);
}

/* Two convolutions that read the same input with the same geometry (C3's cv1 and cv2, which the exporter emits
 * a few layers apart) are launched as ONE grid (conv_i8_persist<PAIR>): the workgroups that need a pixel tile run
 * next to each other, so the input is read from HBM once.  The later one is moved up behind the earlier one when
 * nothing in between touches its operands or its output. */
static int same_conv_input(const mars_op_t *a, const mars_op_t *b) {
    if (a->n_in != b->n_in || a->nseg != b->nseg || a->seg_up != b->seg_up) return 0;
    for (int k = 0; k < a->n_in; k++)
        if (a->t_in[k] != b->t_in[k]) return 0;
    for (int k = 0; k < a->nseg; k++)
        if (a->seg_t[k] != b->seg_t[k] || a->seg_c[k] != b->seg_c[k]) return 0;
    return a->in_h == b->in_h && a->in_w == b->in_w && a->in_c == b->in_c && a->out_h == b->out_h && a->out_w == b->out_w &&
           a->kh == b->kh && a->kw == b->kw && a->sh == b->sh && a->sw == b->sw && a->pt == b->pt && a->pl == b->pl &&
           a->row_pad == b->row_pad && a->oc_pad == b->oc_pad;
}
static int pairable(const mars_op_t *o) {
    /* measured: side-by-side pairs with a plain input gain 10-20 %, those reading a virtual concat lose (their single launches are
     * tuned individually), so a pair over a concat is formed only where it takes the one-tile form (pair_convs) */
    return o->kind == OP_CONV_I8 && !o->nchw && !o->out_nchw && !o->add_t && o->safe && o->lut_off != NO_OFF &&
           (o->in_c & 15) == 0 && o->in_c > 4 && (o->out_c & 15) == 0 && !o->out_pix_stride;
}
/* the step both pairing passes share: op j becomes op i's mate (moved up right behind it) unless an op between them touches j's output or
 * writes one of j's inputs */
static int pair_up(mars_model_ext_t *m, int i, int j) {
    const mars_op_t *b = &m->ops[j];
    if (touched_between(m, i + 1, j, b->t_out, USE_READ | USE_WRITE)) return 0;
    for (int k = 0; k < b->n_in; k++)
        if (touched_between(m, i + 1, j, b->t_in[k], USE_WRITE)) return 0;
    move_up(m, i + 1, j);
    m->ops[i].pair_next = 1;
    return 1;
}
void pair_convs(mars_model_ext_t *m) {
    for (int i = 0; i + 1 < m->n_ops; i++) {
        mars_op_t *a = &m->ops[i];
        if (!pairable(a) || !op_plain(m, i) || op_is_mate(m, i)) continue;
        for (int j = i + 1; j < m->n_ops && j <= i + 48; j++) {
            mars_op_t *b = &m->ops[j];
            if (!pairable(b) || !op_plain(m, j) || !same_conv_input(a, b) || b->t_out == a->t_out) continue;
            if (op_reads(b, b->t_out) || op_reads(b, a->t_out)) continue;
            /* the one-tile form (sides of 64 channels: the input is staged once for both) where the device code takes it at one frame; alloc_batch
             * asks again for its batch (m->no_both).  MARS_HIP_NO_BOTH: the side-by-side form, and no pair over a concat */
            const mars_op_t *g[4] = {a, b};
            const int both = !m->sw.no_both && !m->no_both && conv_i8_group_fits(m, FORM_BOTH, g, 0, 1);
            if (a->nseg && !both) continue;
            if (pair_up(m, i, j)) {
                m->ops[i].pair_both = both;
                break;
            }
        }
    }
}

/* The float twins' C3: cv1 and cv2 are two 1 x 1 convolutions over the same tensor with the same shape.  As one grid (conv_f32_split's
 * pair form, mhip_conv_f32_pair) the second one's input reads hit L2: at float32 the input of these layers is 4 bytes per element and
 * they are bound by exactly those bytes.  Formed where both take conv_f32_split (a weight image packed under f32_mfma = 3 / 4 at load),
 * neither has a folded Add; the second is moved up next to the first when nothing in between touches its tensors (as pair_convs). */
static int pairable_f32(const mars_op_t *o) {
    return o->kind == OP_CONV_F32 && !o->add_t && o->n_in == 1 && o->w2_off != NO_OFF && o->w3_off == NO_OFF && !o->in_rec && !o->out_rec &&
           o->kh == 1 && o->kw == 1;
}
void pair_convs_f32(mars_model_ext_t *m) {
    if (m->sw.no_pair_f32) return;
    for (int i = 0; i + 1 < m->n_ops; i++) {
        mars_op_t *a = &m->ops[i];
        if (!pairable_f32(a) || !op_plain(m, i) || op_is_mate(m, i)) continue;
        for (int j = i + 1; j < m->n_ops && j <= i + 48; j++) {
            mars_op_t *b = &m->ops[j];
            if (!pairable_f32(b) || !op_plain(m, j) || b->t_in[0] != a->t_in[0] || b->t_out == a->t_out || b->t_out < 0 || a->t_out < 0) continue;
            if (a->in_h != b->in_h || a->in_w != b->in_w || a->in_c != b->in_c || a->out_h != b->out_h || a->out_w != b->out_w || a->out_c != b->out_c ||
                a->sh != b->sh || a->sw != b->sw || a->pt != b->pt || a->pl != b->pl || a->silu_f32 != b->silu_f32 || a->f32_exact != b->f32_exact)
                continue;
            if (planned_stride(&m->mt[a->t_out]) != planned_stride(&m->mt[b->t_out])) continue;
            if (a->w2_planes != b->w2_planes) continue;
            int ok = b->t_in[0] != b->t_out && b->t_in[0] != a->t_out;
            for (int q = i + 1; q < j && ok; q++)
                if (m->ops[q].pair_next) ok = 0; /* (this pass does not move an op past a pair; pair_convs does: kept as it was.  The flag, not op_span: only pairs stop it, no other group) */
            if (ok && pair_up(m, i, j)) break;
        }
    }
}

/* SPPF: MaxPool -> MaxPool -> MaxPool, stride 1, same window, each feeding the next: one launch that keeps the
 * frame in LDS (mhip_pool_chain_i8).  Every stage's tensor is still written (the concat / convolution reads them). */
void fuse_pool_chains(mars_model_ext_t *m) {
    for (int i = 0; i + 1 < m->n_ops; i++) {
        mars_op_t *a = &m->ops[i];
        if (a->kind != OP_MAXPOOL || a->chain_n || a->sh != 1 || a->sw != 1 || a->out_pix_stride || (a->in_c & 15) ||
            a->out_h != a->in_h || a->out_w != a->in_w || a->kh <= 0 || a->kw <= 0 || (size_t)a->in_h * a->in_w * 64 > 60 * 1024 ||
            a->t_out < 0 || m->mt[a->t_out].io_out)
            continue;
        int n = 1;
        a->chain_out[0] = a->t_out;
        while (n < 3 && i + n < m->n_ops) {
            const mars_op_t *b = &m->ops[i + n];
            if (b->kind != OP_MAXPOOL || b->t_in[0] != a->chain_out[n - 1] || b->sh != 1 || b->sw != 1 || b->out_pix_stride ||
                b->in_c != a->in_c || b->in_h != a->in_h || b->in_w != a->in_w || b->out_h != a->in_h || b->out_w != a->in_w ||
                b->kh != a->kh || b->kw != a->kw || b->t_out < 0 || m->mt[b->t_out].io_out || b->t_out == a->t_in[0])
                break;
            a->chain_out[n] = b->t_out;
            n++;
        }
        if (n < 2) continue;
        a->chain_n = n;
        for (int k = 1; k < n; k++) {
            a->bytes += m->ops[i + k].bytes - (double)a->in_h * a->in_w * a->in_c; /* later stages re-read nothing */
            m->ops[i + k].kind = -1;
        }
        a->t_out = a->chain_out[n - 1];
    }
    drop_dead_ops(m);
}

/* float32 graphs: which convolutions may take the f32 matrix cores (fused rounding per tap, inside the 1e-4 tolerance)?
 * The reference's MAXPOOL runs int8 byte logic on whatever bytes it is given (mars_runtime.c:919-957), and so does the
 * fused-ReLU clamp of a float convolution (:700-707): over float bytes both are DISCONTINUOUS functions of their input (a
 * last-bit change can flip which byte wins / whether a mantissa byte is zeroed: measured, 1 value in 16 384 left the
 * tolerance), so every convolution from which one of them can be reached keeps the reference's summation order (conv_f32_kernel, bit-identical); byte-copying
 * layers (concat, upsample) and the float element-wise layers only pass small differences on. */
/* Record-format tensors between float convolutions (f32_mfma = 3 at load, fusion >= 1).  conv_f32_patch cuts every input value into
 * two bf16 pieces and lays them out channels-last in LDS -- per K step ~130 vector instructions of its staging phase, which is what
 * bounds it (profiles/r05_experiments.md).  Where the tensor a k x k convolution X reads is written by another convolution P and read
 * by nothing else (a C3 bottleneck's 1 x 1 -> 3 x 3, the stem -> layer 3, a C3's last 1 x 1 -> the stride-2 convolution behind it), P
 * writes those pieces itself ([c / 8][h][w] records of 32 bytes, the same bytes per element: mhip_conv_f32_t.out_rec) and X fills its
 * patch ring by LDS-DMA (conv_f32_prec).  Same arithmetic: X multiplies exactly the pieces it would have cut itself.  The tensor's
 * bytes are then not the reference's floats: mars_hip_read_tensor / write_tensor convert (hi + mid, the value to 2^-16).  Depends on
 * shapes and the mode only (descriptor-only ranks decide alike). */
void rec_pairs(mars_model_ext_t *m) {
    const int nt = (int)m->pub.header.num_tensors;
    for (int i = 0; i < nt; i++) m->mt[i].rec_c = m->mt[i].rec_hw = 0;
    m->rec_skipped = 0;
    m->rec_max_frames = (size_t)-1;
    if (m->sw.fusion < 1 || m->sw.no_rec || m->plan_f32_mode != 3) return;
    const size_t frames = m->rec_frames > 0 ? (size_t)m->rec_frames : 1, lim = m->sw.rec_limit; /* 32-bit byte offsets over all frames of a tensor */
    int *readers, *writers;
    if (!use_counts(m, &readers, &writers)) return;
    for (int j = 0; j < m->n_ops; j++) {
        mars_op_t *x = &m->ops[j];
        if (x->kind != OP_CONV_F32 || x->w3_off == NO_OFF || x->w3_stem || x->n_in != (x->add_t ? 2 : 1) || x->in_rec) continue;
        const int T = x->t_in[0];
        if (T < 0 || readers[T] != 1 || writers[T] != 1 || m->mt[T].io_in || m->mt[T].io_out || m->mt[T].is_weight) continue;
        if (x->add_t && x->add_t - 1 == T) continue;
        const int i = writer_before(m, T, j);
        if (i < 0) continue;
        mars_op_t *pr = &m->ops[i];
        if (pr->kind != OP_CONV_F32 || pr->add_t || pr->out_rec || (pr->out_c & 7) || pr->kh > 32 || pr->kw > 32) continue;
        if (!op_plain(m, i) || op_is_mate(m, i)) continue; /* (a paired launch writes plain floats) */
        if (pr->out_c != x->in_c || pr->out_h != x->in_h || pr->out_w != x->in_w) continue;
        if (!(pr->w2_off != NO_OFF || (pr->w3_off != NO_OFF && pr->w3_stem))) continue; /* conv_f32_split or conv_f32_stem writes it */
        /* a weight image alone does not mean conv_f32_split takes the shape (stride 2 with an odd kernel width and pad > 1, maps
         * narrower than a gather ...): it would decline at launch, and nothing else writes records -- the run would fail */
        if (pr->w2_off != NO_OFF && mhip_conv_f32_split_takes(pr->out_c, pr->in_c, pr->kh, pr->kw, pr->sh, pr->sw, pr->pl, pr->in_w, pr->out_w) < 0) continue;
        /* ... and the reader declines a folded Add whose operand has another frame stride than its output (conv_f32_try_patch) */
        if (x->add_t && planned_stride(&m->mt[x->add_t - 1]) != planned_stride(&m->mt[x->t_out])) continue;
        if (m->mt[T].bytes != (size_t)x->in_c * x->in_h * x->in_w * 4) continue;
        const int form = mhip_conv_f32_patch_rec_form(x->out_c, x->in_c, x->kh, x->kw, x->sw, x->pl, x->in_h, x->in_w, x->out_h, x->out_w);
        if (!form) continue;
        if (form == 1) { /* conv_f32_prec: its image replaces the plain one in place (same size by construction) */
            const size_t n0 = mhip_conv_f32_patch_pack2(x->out_c, x->in_c, x->kh, x->kw, x->sw, x->pl, x->in_h, x->in_w, x->out_h, x->out_w, 0, NULL, NULL);
            const size_t n1 = mhip_conv_f32_patch_pack2(x->out_c, x->in_c, x->kh, x->kw, x->sw, x->pl, x->in_h, x->in_w, x->out_h, x->out_w, 1, NULL, NULL);
            if (!n1 || n1 != n0) continue;
        }
        { /* the three tensors the two launches address with 32-bit offsets: all frames of each must stay below 4 GiB */
            const int tt[3] = {pr->t_in[0], T, x->t_out};
            size_t worst = 0;
            for (int q = 0; q < 3; q++)
                if (tt[q] >= 0 && planned_stride(&m->mt[tt[q]]) > worst) worst = planned_stride(&m->mt[tt[q]]);
            if (worst && worst * frames > lim) {
                m->rec_skipped = 1;
                continue;
            }
            if (worst && lim / worst < m->rec_max_frames) m->rec_max_frames = lim / worst;
        }
        if (form == 1 && !m->deferred)
            mhip_conv_f32_patch_pack2(x->out_c, x->in_c, x->kh, x->kw, x->sw, x->pl, x->in_h, x->in_w, x->out_h, x->out_w, 1,
                                      (const float *)(m->arena_host + x->w_off), m->arena_host + x->w3_off);
        x->in_rec = form;
        pr->out_rec = 1;
        m->mt[T].rec_c = x->in_c;
        m->mt[T].rec_hw = x->in_h * x->in_w;
    }
    free(readers);
}

/* Exact zeros the reference's byte-wise CONCAT leaves in float tensors (round 6).  The concat copies runs of shape[3] BYTES whatever the dtype
 * (mars_runtime.c:971-999): on [1, C, H, W] float tensors it writes C H W bytes (+ the slices' offsets) of an output that holds 4 C H W -- in
 * the private zero-initialised buffers of the parity target everything behind that is zero in every frame, i.e. all but the
 * first C / 4 + 1 channels (measured on the twins: tests).  A 1 x 1 convolution that reads such a tensor (every C3's cv3, SPPF's cv2, the head
 * C3s' cv1 + cv2) multiplies zeros for three quarters of its K loop.  Under the split-bf16 modes (3 / 4: results inside the tolerance, not
 * bit-equal anyway) its K loop stops at the last channel that can be non-zero (mhip_conv_f32_t.k_limit): acc + (+-0 * w) == acc for finite w,
 * so the sums are the same floats (up to the sign of a zero); skipped weights are checked to be finite where the blob is at hand.  Modes 0 - 2
 * keep the full loop.  Depends on shapes only. */
void zero_tail_f32(mars_model_ext_t *m) {
    const int nt = (int)m->pub.header.num_tensors;
    for (int i = 0; i < nt; i++) m->mt[i].zero_from = 0;
    for (int i = 0; i < m->n_ops; i++) m->ops[i].k_limit = 0;
    if (m->sw.fusion < 1 || m->sw.no_zero_tail) return;
    for (int j = 0; j < m->n_ops; j++) {
        mars_op_t *x = &m->ops[j];
        if (x->kind != OP_CONV_F32 || x->kh != 1 || x->kw != 1 || x->sh != 1 || x->sw != 1 || x->pt || x->pl || x->in_rec || x->w2_off == NO_OFF) continue;
        const int T = x->t_in[0];
        if (T < 0 || m->mt[T].is_weight || m->mt[T].io_in || m->pub.tensors[T].desc.dtype != MARS_DTYPE_FLOAT32) continue;
        if (m->mt[T].bytes != (size_t)x->in_c * x->in_h * x->in_w * 4) continue;
        size_t written = 0; /* bytes [0, written) may be non-zero: the furthest byte any writer reaches */
        int ok = 1, nw = 0;
        for (int q = 0; q < m->n_ops && ok; q++) {
            const mars_op_t *o = &m->ops[q];
            if (!op_writes(o, T)) continue;
            if (o->kind != OP_CONCAT_SLICE || o->out_pix_stride) { ok = 0; break; } /* (a pool chain that writes it is no slice either) */
            nw++;
            const size_t npix = (size_t)o->out_h * o->out_w;
            if (npix && o->in_c > 0) {
                const size_t end = (npix - 1) * (size_t)o->out_c + (size_t)o->ch_off + (size_t)o->in_c;
                if (end > written) written = end;
            }
        }
        if (!ok || !nw || !written) continue;
        const size_t plane = (size_t)x->in_h * x->in_w * 4;
        const size_t kl = (written + plane - 1) / plane; /* channels that hold a written byte */
        if (kl >= (size_t)x->in_c) continue;
        if (!m->deferred) { /* 0 * w must be 0: every skipped weight finite */
            const float *w = (const float *)(m->arena_host + x->w_off);
            int finite = 1;
            for (int oc = 0; oc < x->out_c && finite; oc++)
                for (int ic = (int)kl; ic < x->in_c; ic++) {
                    const float v = w[(size_t)oc * x->in_c + ic];
                    if (!(v - v == 0.0f)) { finite = 0; break; }
                }
            if (!finite) continue;
        }
        x->k_limit = (int)kl;
        if (!m->mt[T].zero_from || written > m->mt[T].zero_from) m->mt[T].zero_from = written;
        /* the layer's algorithmic work is what is not provably zero */
        x->macs = (double)x->out_h * x->out_w * x->out_c * (double)kl;
        x->bytes = ((double)x->in_h * x->in_w * (double)kl + (double)x->out_h * x->out_w * x->out_c) * 4.0;
    }
}

/* A float CONCAT that no launch materialises (round 6; conv_f32_vcat.hip has the arithmetic).  On N float maps [1, C, H, W] of equal size the reference's
 * byte-wise CONCAT (trim_concat has already cut it to what survives) leaves, per frame: the first W BYTES of every input but the last, then the first
 * L = C_out H W bytes of the LAST input shifted by sB = (N - 1) W bytes, then zeros.  Its readers -- one 1 x 1 convolution, or a pair of them --
 * already stop their K loop behind the written bytes (zero_tail_f32: k_limit = L / plane + 1).  For every pixel from sB / 4 on, such a convolution over
 * the concat IS the convolution over the address (last input - sB) with L / plane input planes: it runs on that view (vc_shift, k_limit required),
 * and a second, tiny launch (OP_CONV_F32_VHEAD) recomputes the first sB / 4 pixels of every output plane from their true operands.  The copies
 * (two passes over a quarter of the concat tensor) and the tensor itself go.  Same tolerance class as the launch it replaces (split-bf16 modes only).
 * Batch-dependent like rec_pairs (32-bit offsets over all frames): shares its per-batch re-planning. */
void virtual_concat_f32(mars_model_ext_t *m) {
    if (m->sw.fusion < 1 || m->sw.no_vconcat_f32 || (m->plan_f32_mode != 3 && m->plan_f32_mode != 4)) return;
    const size_t frames = m->rec_frames > 0 ? (size_t)m->rec_frames : 1, lim = m->sw.rec_limit;
    for (int i = 0; i < m->n_ops; i++) {
        if (m->ops[i].kind != OP_CONCAT_SLICE) continue;
        const int T = m->ops[i].t_out, layer = m->ops[i].layer;
        int e = i;
        while (e + 1 < m->n_ops && m->ops[e + 1].kind == OP_CONCAT_SLICE && m->ops[e + 1].layer == layer && m->ops[e + 1].t_out == T) e++;
        const int N = e - i + 1, first_op = i;
        i = e; /* (whatever happens below, the scan goes on behind the group) */
        if (N < 2 || N > 4 || T < 0 || m->mt[T].io_in || m->mt[T].io_out || m->mt[T].is_weight || m->pub.tensors[T].desc.dtype != MARS_DTYPE_FLOAT32) continue;
        const mars_op_t *last = &m->ops[e];
        const int Wb = last->in_c; /* bytes per run */
        if (Wb <= 0 || (Wb & 3) || last->out_c != Wb || last->ch_off != (N - 1) * Wb || last->out_pix_stride || last->out_h <= 0 || last->out_w <= 0) continue;
        const int TL = last->t_in[0];
        const size_t Lb = (size_t)last->out_h * last->out_w * (size_t)Wb, sB = (size_t)(N - 1) * (size_t)Wb;
        if (TL < 0 || TL == T || m->mt[TL].is_weight || m->mt[TL].io_in || m->mt[TL].io_out /* (a pipeline hands every graph input and output over in a buffer of its own: nothing mapped in front) */ || m->mt[TL].rec_c || m->mt[TL].nhwc_c || m->mt[TL].pix_stride || m->mt[TL].bytes < Lb ||
            m->pub.tensors[TL].desc.dtype != MARS_DTYPE_FLOAT32 || sB > 256)
            continue;
        int ok = 1, firsts[3] = {-1, -1, -1};
        for (int k = 0; k < N - 1 && ok; k++) {
            const mars_op_t *sl = &m->ops[first_op + k];
            const int ti = sl->t_in[0];
            if (sl->in_c != Wb || sl->out_c != Wb || sl->ch_off != k * Wb || sl->out_h != 1 || sl->out_w != 1 || sl->out_pix_stride || ti < 0 || ti == T ||
                m->mt[ti].is_weight || m->mt[ti].rec_c || m->mt[ti].nhwc_c || m->mt[ti].bytes < (size_t)Wb)
                ok = 0;
            firsts[k] = ti;
        }
        if (!ok) continue;
        /* who touches the concat tensor: the group writes it, one convolution (or one pair) reads it, nothing else */
        int r1 = -1, nr = 0;
        for (int j = 0; j < m->n_ops && ok; j++) {
            const mars_op_t *o = &m->ops[j];
            if (j >= first_op && j <= e) continue;
            if (op_writes(o, T)) ok = 0;
            for (int k = 0; k < o->n_in; k++)
                if (o->t_in[k] == T) {
                    if (k != 0 || j <= e) ok = 0;
                    if (r1 < 0) r1 = j;
                    nr++;
                }
        }
        if (!ok || r1 < 0 || nr > 2) continue;
        int g[4];
        const int paired = op_form(m, r1, g) == FORM_PAIR_F32;
        if (nr != 1 + paired || op_is_mate(m, r1) || (paired && m->ops[r1 + 1].t_in[0] != T)) continue;
        const int rl = r1 + paired; /* the last reader */
        size_t km = 0, worst = 0;
        for (int j = r1; j <= rl && ok; j++) {
            const mars_op_t *x = &m->ops[j];
            if (x->kind != OP_CONV_F32 || x->k_limit <= 0 || x->n_in != 1 || x->add_t || x->in_rec || x->vc_shift || x->kh != 1 || x->kw != 1 || x->sh != 1 || x->sw != 1 ||
                x->pt || x->pl || x->w2_off == NO_OFF || x->in_h != x->out_h || x->in_w != x->out_w || x->t_out == TL || x->t_out == T || x->t_out < 0) { ok = 0; break; }
            const size_t hw = (size_t)x->in_h * x->in_w, Pb = hw * 4;
            if (m->mt[T].bytes != (size_t)x->in_c * Pb || Lb % Pb || sB / 4 >= hw) { ok = 0; break; }
            km = Lb / Pb;
            if (km < 1 || (size_t)x->k_limit != km + 1 || km + 1 > (size_t)x->in_c) { ok = 0; break; }
            if (x->out_rec && (x->out_c & 7)) { ok = 0; break; }
            for (int k = 0; k < N - 1; k++)
                if (x->t_out == firsts[k]) ok = 0;
            const size_t st = planned_stride(&m->mt[x->t_out]);
            if (st > worst) worst = st;
        }
        if (!ok) continue;
        ok = !touched_between(m, e + 1, rl + 1, TL, USE_WRITE); /* the operands must still hold at the readers what they held at the concat */
        for (int k = 0; k < N - 1 && ok; k++) ok = !touched_between(m, e + 1, rl + 1, firsts[k], USE_WRITE);
        if (!ok) continue;
        if (planned_stride(&m->mt[TL]) > worst) worst = planned_stride(&m->mt[TL]);
        /* (the main launch's buffer range is the CONCAT tensor's size over the last input's frame stride: at most 3 strides more than frames of it) */
        if (worst * (frames + 3) > lim) { /* conv_f32_split addresses all frames of a tensor with 32-bit offsets and nothing else honours k_limit: as rec_pairs */
            m->rec_skipped = 1;
            continue;
        }
        if (lim / worst - 3 < m->rec_max_frames) m->rec_max_frames = lim / worst - 3;
        if (!m->deferred) { /* plane km is skipped for the pixels where the concat holds zeros: 0 * w must be 0 there (as zero_tail_f32 checks the planes behind it) */
            for (int j = r1; j <= rl && ok; j++) {
                const mars_op_t *x = &m->ops[j];
                const float *w = (const float *)(m->arena_host + x->w_off);
                for (int oc = 0; oc < x->out_c; oc++) {
                    const float v = w[(size_t)oc * x->in_c + km];
                    if (!(v - v == 0.0f)) { ok = 0; break; }
                }
            }
            if (!ok) continue;
        }
        /* ops: [slices: gone] ... [readers on the view] [one head launch per reader] */
        const int heads = 1 + paired;
        size_t wt_off[2] = {NO_OFF, NO_OFF}; /* the head launches' weights: planes 0 .. km transposed (mhip_conv_f32_vcat_pack) */
        for (int q = 0; q < heads; q++) {
            const mars_op_t *x = &m->ops[r1 + q];
            wt_off[q] = arena_reserve(m, mhip_conv_f32_vcat_pack(x->out_c, x->in_c, (int)km + 1, NULL, NULL));
            if (wt_off[q] == NO_OFF) return;
            if (!m->deferred)
                mhip_conv_f32_vcat_pack(x->out_c, x->in_c, (int)km + 1, (const float *)(m->arena_host + x->w_off), (float *)(m->arena_host + wt_off[q]));
        }
        while (m->n_ops + heads > m->cap_ops) {
            const int cap = m->cap_ops * 2;
            mars_op_t *np = (mars_op_t *)realloc(m->ops, (size_t)cap * sizeof(mars_op_t));
            if (!np) { m->plan_err = MARS_ERR_ALLOC_FAILED; return; }
            m->ops = np; m->cap_ops = cap;
        }
        memmove(&m->ops[rl + 1 + heads], &m->ops[rl + 1], sizeof(mars_op_t) * (size_t)(m->n_ops - rl - 1));
        m->n_ops += heads;
        for (int q = 0; q < heads; q++) {
            mars_op_t *x = &m->ops[r1 + q], *h = &m->ops[rl + 1 + q];
            const double hw = (double)x->in_h * x->in_w;
            x->t_in[0] = TL;
            x->vc_shift = (int)sB;
            x->k_limit = (int)km;
            x->macs = hw * x->out_c * (double)km;
            x->bytes = (hw * (double)km + hw * x->out_c) * 4.0;
            *h = *x;
            h->kind = OP_CONV_F32_VHEAD;
            h->pair_next = 0; h->vc_shift = 0;
            h->k_limit = (int)km + 1;
            h->vc_n = N - 1; h->vc_run = Wb / 4;
            h->n_in = N;
            for (int k = 0; k < N - 1; k++) { h->vc_t[k] = firsts[k]; h->t_in[1 + k] = firsts[k]; }
            h->macs = (double)(sB / 4) * x->out_c * (double)(km + 1);
            h->bytes = ((double)(sB / 4) * (double)(km + 1) + (double)(sB / 4) * x->out_c) * 4.0;
            h->variant = 0;
            h->w3_off = wt_off[q]; h->w3_stem = 0;
            h->w2_off = NO_OFF; h->w2_planes = 0;
        }
        memmove(&m->ops[first_op], &m->ops[e + 1], sizeof(mars_op_t) * (size_t)(m->n_ops - e - 1));
        m->n_ops -= N;
        m->mt[T].needed = 0;
        m->mt[T].partial = 1;
        m->mt[T].zero_from = 0;
        i = first_op - 1; /* (the array moved down by N: go on at the op that now stands where the group stood) */
    }
}

void f32_policy(mars_model_ext_t *m) {
    const int nt = (int)m->pub.header.num_tensors;
    unsigned char *hot = (unsigned char *)calloc((size_t)nt + 1, 1);
    if (!hot) {
        for (int i = 0; i < m->n_ops; i++) m->ops[i].f32_exact = 1;
        return;
    }
    for (int i = m->n_ops - 1; i >= 0; i--) {
        mars_op_t *o = &m->ops[i];
        int reach = 0;
        if (o->kind == OP_MAXPOOL && o->t_in[0] >= 0 && m->pub.tensors[o->t_in[0]].desc.dtype == MARS_DTYPE_FLOAT32) reach = 1;
        if (o->kind == OP_RELU_BYTES && o->t_out >= 0) { /* the fused-ReLU byte clamp over float bytes (:700-707): in place */
            hot[o->t_out] = 1;
            continue;
        }
        if (o->t_out >= 0 && hot[o->t_out]) reach = 1;
        for (int k = 0; k < o->chain_n; k++)
            if (o->chain_out[k] >= 0 && hot[o->chain_out[k]]) reach = 1;
        if (!reach) continue;
        for (int k = 0; k < o->n_in; k++)
            if (o->t_in[k] >= 0) hot[o->t_in[k]] = 1;
        if (o->kind == OP_CONV_F32) o->f32_exact = 1;
    }
    free(hot);
}

/* The operand model every pass above relies on (mars_op_t), checked once per plan: a violation is a planner bug, fails the plan with
 * MARS_ERR_LAYER_FAILED and names the op under MARS_VERBOSE. */
void plan_check(mars_model_ext_t *m) {
    for (int i = 0; i < m->n_ops; i++) {
        const mars_op_t *o = &m->ops[i];
        const char *why = NULL;
        const mars_op_t *M[4];
        int g[4], gg[4];
        op_form(m, i, g);
        for (int k = 0; k < 4; k++) M[k] = g[k] >= 0 ? &m->ops[g[k]] : NULL;
        if (o->kind == -1) why = "a dead op is left";
        else if (o->n_in < 0 || o->n_in > 4 || o->nseg < 0 || o->nseg > 4 || o->chain_n < 0 || o->chain_n > 3 || o->vc_n < 0 || o->vc_n > 3) why = "an operand count is out of range";
        else if (o->add_t && !op_reads(o, o->add_t - 1)) why = "add_t is not among t_in";
        else if (o->chain_n && o->t_out != o->chain_out[o->chain_n - 1]) why = "t_out is not the chain's last stage";
        /* the launch group o heads (or, for cv1 of a split group, would head): M[k] = its k-th member, NULL where the plan ends before it.  The flags
         * themselves are read here and only here: this is where their coherence is checked */
        else if (o->pair_next && (!M[1] || M[1]->kind != o->kind)) why = "pair_next without a mate of its kind";
        else if (o->pair_both && (!o->pair_next || o->kind != OP_CONV_I8 || (o->out_c != 64 && o->out_c != 128) || M[1]->out_c != o->out_c)) why = "pair_both without a pair of 64- or 128-channel sides";
        else if (o->kind == OP_CONV_I8 && o->pair_next && o->nseg && !o->pair_both) why = "a side-by-side pair over a virtual concat";
        else if (o->post_next && (o->kind != OP_CONV_I8 || !M[1] || M[1]->kind != OP_CONV_I8 || M[1]->nseg != 2 || M[1]->seg_t[0] != o->t_out || !op_reads(o, M[1]->seg_t[1])))
            why = "post_next without its 1x1 behind it, or y2 is not among t_in";
        else if (o->split_next && (o->kind != OP_CONV_I8 || !M[2] || M[1]->kind != OP_CONV_I8 || M[2]->kind != OP_CONV_I8 || op_form(m, g[1], gg) != FORM_PAIR || !op_plain(m, g[2]) ||
                                   M[1]->n_in != 1 || M[2]->n_in != 1 || M[1]->t_in[0] != o->t_out || M[2]->t_in[0] != o->t_out || o->post_next || o->pair_next || o->pre || o->add_t))
            why = "split_next without its pair of 1x1s behind it";
        else if (o->split_chain && (!o->split_next || !M[3] || !free_1x1_ok(M[3], o, 32, 32) || !op_plain(m, g[3]) || (o->split_chain != 1 && o->split_chain != 2) ||
                                    M[3]->t_in[0] != M[o->split_chain]->t_out || M[3]->t_out < 0 || M[3]->t_out == M[1]->t_out || M[3]->t_out == M[2]->t_out ||
                                    M[3]->t_out == o->t_out || m->mt[M[3]->t_out].pix_stride || o->chain_w_off == NO_OFF))
            why = "split_chain without its 1x1 behind the pair";
        else if (o->both_chain && (!o->pair_both || !M[2] || !free_1x1_ok(M[2], o, 64, 64) || !op_plain(m, g[2]) || (o->both_chain != 1 && o->both_chain != 2) ||
                                   M[2]->t_in[0] != M[o->both_chain - 1]->t_out || M[2]->t_out < 0 || M[2]->t_out == o->t_out || M[2]->t_out == M[1]->t_out))
            why = "both_chain without its 1x1 behind the pair";
        else if (o->both_elide && (!o->both_chain || m->mt[M[o->both_chain - 1]->t_out].needed || m->mt[M[o->both_chain - 1]->t_out].io_out))
            why = "both_elide on a side that is kept";
        for (int k = 0; !why && k < o->nseg; k++)
            if (!op_reads(o, o->seg_t[k])) why = "a seg_t is not among t_in";
        for (int k = 0; !why && k < o->vc_n; k++)
            if (!op_reads(o, o->vc_t[k])) why = "a vc_t is not among t_in";
        if (!why) continue;
        VLOG("plan_check: op %d (layer %d, kind %d): %s\n", i, o->layer, o->kind, why);
        m->plan_err = MARS_ERR_LAYER_FAILED;
        return;
    }
}
