/*
 * mars_model.c -- .mars loader of the MI355X executor: file validation, tensor / device state, batch allocation, accessors.
 * (The launch planner lives in mars_plan.c, the run paths in mars_run.c: one 2 200-line file until round 4.)
 *
 * Public behaviour: reference include/mars_runtime.h:79-138, implemented in
 * the reference by src/mars/mars_runtime.c.  What changes underneath:
 *   - the 8 MiB round-robin "DDR" arena (mars_runtime.c:205-334) becomes one
 *     HBM buffer per activation tensor and frame, zero-initialised, sized from
 *     the byte extents the layers actually touch (no aliasing between live
 *     tensors; the reference's in-place hazards cannot occur);
 *   - the per-call dispatch switch (mars_runtime.c:1161-1224) becomes a launch
 *     plan built once at load: tensor ids resolved, weights re-packed for the
 *     MFMA kernel, float scales folded on the host exactly as the C code folds
 *     them, 256-entry LUTs for every int8 transcendental;
 *   - a frame batch dimension (the reference has none).
 * Layer semantics, including the quirks, follow the reference line by line;
 * each planner below cites the lines it mirrors.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>
#include <time.h>

#include "mars_internal.h"
#include "nna.h"


int mars_verbose(void) {
    static int v = -1;
    if (v < 0) v = getenv("MARS_VERBOSE") ? 1 : 0;
    return v;
}

/* every environment switch of the planner and of alloc_batch, with its default (plan_switches_t) */
void plan_switches_read(plan_switches_t *sw, int at_load) {
    const char *e;
    if (at_load) sw->fusion = (e = getenv("MARS_HIP_FUSION")) ? atoi(e) : 1;
    sw->no_fuse_lut = getenv("MARS_HIP_NO_FUSE_LUT") != NULL;
    sw->no_nhwc_internal = getenv("MARS_HIP_NO_NHWC_INTERNAL") != NULL;
    sw->no_vconcat_q = getenv("MARS_HIP_NO_VCONCAT_Q") != NULL;
    sw->no_pair_f32 = getenv("MARS_HIP_NO_PAIR_F32") != NULL;
    sw->no_rec = getenv("MARS_HIP_NO_REC") != NULL;
    sw->no_zero_tail = getenv("MARS_HIP_NO_ZERO_TAIL") != NULL;
    sw->no_vconcat_f32 = getenv("MARS_HIP_NO_VCONCAT_F32") != NULL;
    sw->no_rowpad = getenv("MARS_HIP_NO_ROWPAD") != NULL;
    sw->no_post = getenv("MARS_HIP_NO_POST") != NULL;
    sw->no_split = getenv("MARS_HIP_NO_SPLIT") != NULL;
    sw->no_chain = getenv("MARS_HIP_NO_CHAIN") != NULL;
    sw->no_both = getenv("MARS_HIP_NO_BOTH") != NULL;
    sw->no_both_chain = getenv("MARS_HIP_NO_BOTH_CHAIN") != NULL;
    /* (tests lower the limits to see the per-batch decisions with small tensors) */
    sw->rec_limit = (e = getenv("MARS_HIP_REC_LIMIT")) ? (size_t)strtoull(e, NULL, 0) : (size_t)0xfffffff0u;
    sw->vconcat_limit = (e = getenv("MARS_HIP_VCONCAT_LIMIT")) ? (size_t)strtoull(e, NULL, 0) : (size_t)0x7fffffffu;
    sw->bottleneck_limit = (e = getenv("MARS_HIP_BOTTLENECK_LIMIT")) ? (size_t)strtoull(e, NULL, 0) : 0;
}

void drop_graph(mars_model_ext_t *m) {
    if (m->graph_exec) {
        mhip_sync();
        mhip_graph_destroy(m->graph_exec);
    }
    m->graph_exec = NULL;
    m->ran_plain = 0;
}

/* ------------------------------------------------------------------ errors */
static const char *const k_err[] = {
    "OK", "Invalid magic number", "Version mismatch", "Memory allocation failed",
    "Invalid file format", "NNA initialization failed", "Layer execution failed",
    "Invalid tensor", "Invalid layer",
};

const char *mars_get_error_string(mars_error_t err) {
    int i = -(int)err;
    if (i >= 0 && i < (int)(sizeof(k_err) / sizeof(k_err[0]))) return k_err[i];
    return "Unknown error";
}

/* ------------------------------------------------------------------- load */
static void free_device_state(mars_model_ext_t *m) {
    drop_graph(m);
    if (m->act_dev) mhip_free(m->act_dev);
    if (m->scratch_dev) mhip_free(m->scratch_dev);
    m->act_dev = m->scratch_dev = NULL;
    for (uint32_t i = 0; m->mt && i < m->pub.header.num_tensors; i++) {
        if (m->mt[i].host) mhip_host_free(m->mt[i].host);
        m->mt[i].host = NULL;
        if (m->mt[i].dense_dev) mhip_free(m->mt[i].dense_dev);
        m->mt[i].dense_dev = NULL;
        if (!m->mt[i].is_weight) m->mt[i].dev = NULL;
    }
    if (m->det_dev) mhip_free(m->det_dev);
    if (m->det_counts_dev) mhip_free(m->det_counts_dev);
    m->det_dev = NULL;
    m->det_counts_dev = NULL;
    m->det_cap = 0;
    m->tail_pending = 0;
    mars_stages_release(m);
}

static void free_ops(mars_model_ext_t *m) {
    drop_graph(m);
    for (int i = 0; i < m->n_ops; i++) {
        if (m->ops[i].ev0) mhip_event_destroy(m->ops[i].ev0);
        if (m->ops[i].ev1) mhip_event_destroy(m->ops[i].ev1);
    }
    free(m->ops);
    m->ops = NULL;
    m->n_ops = m->cap_ops = 0;
}

/* every loaded model (single-threaded contract, like the reference's globals: SURVEY 8b "Threading") */
static mars_model_ext_t *g_live_models = NULL;
mars_model_ext_t *mars_live_models(void) { return g_live_models; }

void mars_free(mars_model_t *model) {
    if (!model) return;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    for (mars_model_ext_t **pp = &g_live_models; *pp; pp = &(*pp)->live_next)
        if (*pp == m) { *pp = m->live_next; break; }
    for (mars_model_ext_t *x = g_live_models; x; x = x->live_next)
        if (x->roi_from == m) x->roi_from = NULL;
    if (m->pipe) mars_hip_pipe_close(model);
    if (mhip_ready()) mhip_sync();
    free_device_state(m);
    free_ops(m);
    if (m->arena_dev) mhip_free(m->arena_dev);
    if (m->det_lut_dev) mhip_free(m->det_lut_dev);
    if (m->heads_lut_dev) mhip_free(m->heads_lut_dev);
    if (m->dfl_lut_dev) mhip_free(m->dfl_lut_dev);
    if (m->ev_graph_done) mhip_event_destroy(m->ev_graph_done);
    if (m->ev_tail_done) mhip_event_destroy(m->ev_tail_done);
    if (m->ev_label_done) mhip_event_destroy(m->ev_label_done);
    if (m->ev_shot_done) mhip_event_destroy(m->ev_shot_done);
    if (m->ev_fork) mhip_event_destroy(m->ev_fork);
    for (int k = 0; k < 3; k++)
        if (m->ev_join[k]) mhip_event_destroy(m->ev_join[k]);
    for (int k = 0; k < 2; k++)
        for (int c = 0; c < 8; c++)
            if (m->ev_chunk[k][c]) mhip_event_destroy(m->ev_chunk[k][c]);
    free(m->arena_host);
    free(m->layer_noop);
    free(m->mt);
    free(m->pub.weights);
    free(m->pub.layers);
    free(m->pub.tensors);
    free(m);
}

mars_error_t build_plan(mars_model_ext_t *m) {
    const uint32_t nt = m->pub.header.num_tensors, nl = m->pub.header.num_layers;
    plan_switches_read(&m->sw, 0);
    free_ops(m);
    m->arena_size = 0;
    if (m->arena_host) memset(m->arena_host, 0, m->arena_cap); /* re-plans must not see stale bytes */
    m->scratch_per_frame = 0;
    m->plan_err = MARS_OK;
    m->plan_f32_mode = mhip_conv_f32_mode(-1); /* (the passes read the stored value) */
    m->blob_mirror_bytes = m->pub.weights_size;
    for (uint32_t i = 0; i < nt; i++) {
        m->mt[i].extent = m->mt[i].bytes;
        m->mt[i].pix_c = m->mt[i].pix_stride = 0;
        m->mt[i].needed = (m->mt[i].io_in || m->mt[i].io_out) ? 1 : 0;
    }
    /* slot 0 of the arena: mirror of the raw blob (element-wise layers may read weight
     * tensors directly); sized after planning, so reserve generously now */
    for (uint32_t i = 0; i < nl && m->plan_err == MARS_OK; i++) {
        const int n0 = m->n_ops;
        plan_layer(m, (int)i);
        m->layer_noop[i] = m->n_ops == n0;
    }
    if (m->plan_err != MARS_OK) return (mars_error_t)m->plan_err;
    /* the passes, in order; why each stands where it stands is said here and nowhere else */
    if (m->sw.fusion >= 1) {
        fold_silu(m, 0);
        fuse_lut(m);      /* after the SiLU chains: a SIGMOID that feeds a MUL belongs to them, a lone activation layer is what is left */
        fold_silu(m, 1);
        nhwc_internal(m); /* after the SiLU fold: its intermediates are gone; before Add folding / pairing: they then see NHWC convolutions */
        fold_add(m, 0);
        fold_add(m, 1);
        if (!m->no_vconcat) virtual_concat(m);
        elide_concat(m);  /* after virtual_concat: only the concats that stay materialised get producers that write slices */
        trim_concat(m);
        fuse_pool_chains(m); /* the first pass that sets chain_out: from here on op_writes() is more than t_out */
        pair_convs(m);
        if (m->sw.fusion >= 2 && !m->no_bottleneck) fuse_bottleneck(m); /* opt-in (level 2); after pairing: a paired launch stays a pair */
        fuse_post(m);     /* after both: a paired launch stays a pair, an op carrying `pre` never takes `post` (level 2 keeps its plans) */
        fuse_split(m);    /* after pairing: it takes whole pairs; an op carrying `pre` or `post_next` is left alone */
        fuse_split_chain(m); /* after fuse_split: it extends its launches; after fuse_bottleneck: a 1x1 folded into a 3x3 as `pre` is no op any more */
        pad_output_rows(m);
        virtual_concat_q(m); /* last of the passes that form int8 launches: it splits a convolution in two launches over one output tensor */
        fuse_both_chain(m);  /* after every pass that marks mates or cuts a pair in row ranges: it takes whole one-tile pairs and free 1x1s only */
    } else {
        nhwc_internal(m); /* only resets what a plan at another level left in the tensors */
    }
    f32_policy(m);
    zero_tail_f32(m); /* before pairing: a pair shares its input, hence its limit; resets its flags at fusion level 0 */
    if (m->sw.fusion >= 1) pair_convs_f32(m); /* after f32_policy: a pair shares one kernel choice */
    rec_pairs(m);          /* fusion >= 1 only; resets the tensors' record flags in any case */
    virtual_concat_f32(m); /* last: it replaces launches; shares rec_pairs' per-batch decision */
    if (m->plan_err == MARS_OK) plan_check(m);
    return (mars_error_t)m->plan_err;
}

mars_error_t upload_params(mars_model_ext_t *m) {
    /* final arena = [planned entries][blob mirror]; mirror appended last so its size is known */
    size_t mirror_off = arena_reserve(m, m->blob_mirror_bytes + 64);
    if (mirror_off == NO_OFF) return MARS_ERR_ALLOC_FAILED;
    if (!m->deferred) blob_read(m, 0, m->blob_mirror_bytes, m->arena_host + mirror_off);
    if (m->arena_dev) mhip_free(m->arena_dev);
    m->arena_dev = (uint8_t *)mhip_malloc(m->arena_size);
    if (!m->arena_dev) return MARS_ERR_ALLOC_FAILED;
    if (mhip_h2d_async(m->arena_dev, m->arena_host, m->arena_size) || mhip_sync()) return MARS_ERR_NNA_INIT_FAILED;
    for (uint32_t i = 0; i < m->pub.header.num_tensors; i++) {
        if (!m->mt[i].is_weight) continue;
        m->mt[i].dev = m->arena_dev + mirror_off + (size_t)m->pub.tensors[i].desc.data_offset;
        m->mt[i].stride = 0;
        m->pub.tensors[i].paddr = m->mt[i].dev;
    }
    m->pub.ddr_paddr = m->arena_dev;
    m->pub.ddr_size = m->arena_size;
    return MARS_OK;
}

static mars_error_t replan(mars_model_ext_t *m) {
    const mars_error_t e = build_plan(m);
    return e == MARS_OK ? upload_params(m) : e;
}

/* The fusions alloc_batch takes back for a batch they do not fit, in the order it asks: {the model flag that switches the pass off, how to ask,
 * the form asked about, the chained form whose launches are asked as that form too}.  The order matters: a chained 1x1 is asked before the
 * launch it extends (without it the pair may still fit), and the one-tile rows stand behind fuse_split's (a re-plan without it frees pairs
 * for that form). */
enum { ASK_VCONCAT, ASK_PRE, ASK_GROUP };
typedef struct { size_t flag; int ask, form, chained; } take_back_t;
#define FLAG(f) offsetof(mars_model_ext_t, f)
static const take_back_t TAKE_BACK[] = {
    {FLAG(no_vconcat), ASK_VCONCAT, 0, 0},
    {FLAG(no_bottleneck), ASK_PRE, 0, 0}, /* (level 2) */
    {FLAG(no_post), ASK_GROUP, FORM_POST, FORM_POST},
    {FLAG(no_chain), ASK_GROUP, FORM_SPLIT_CHAIN, FORM_SPLIT_CHAIN},
    {FLAG(no_split), ASK_GROUP, FORM_SPLIT, FORM_SPLIT_CHAIN},
    {FLAG(no_both_chain), ASK_GROUP, FORM_BOTH_CHAIN, FORM_BOTH_CHAIN},
    {FLAG(no_both), ASK_GROUP, FORM_BOTH, FORM_BOTH_CHAIN},
};
#undef FLAG

mars_error_t alloc_batch(mars_model_ext_t *m, int n) {
    const uint32_t nt = m->pub.header.num_tensors;
    if (m->pipe) mars_hip_pipe_close(&m->pub); /* its slots were sized for the old batch */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED;
    plan_switches_read(&m->sw, 0);
    /* tests exercise the two fall-backs below with a small batch: their limits are the ones read just now (a re-plan below reads the record
     * again, these two stay) */
    const size_t vlim = m->sw.vconcat_limit, blim = m->sw.bottleneck_limit;
    /* the two batch-dependent fall-backs are decided afresh for every batch (they used to stick once a large
     * batch had switched them on): plan again with the fusions allowed, the checks below take them back if need be */
    /* (record-format pairs, rec_pairs: chosen per batch too -- plan again when a chosen pair would not fit this batch, or one left
     * alone at a larger batch may fit now) */
    const int rec_replan = (size_t)n > m->rec_max_frames || (m->rec_skipped && n < m->rec_frames);
    m->rec_frames = n;
    if (m->no_vconcat || m->no_bottleneck || m->no_post || m->no_split || m->no_chain || m->no_both || m->no_both_chain || rec_replan) {
        m->no_vconcat = m->no_bottleneck = m->no_post = m->no_split = m->no_chain = m->no_both = m->no_both_chain = 0;
        const mars_error_t e = replan(m);
        if (e != MARS_OK) return e;
    }
    /* Every fusion below was accepted on shapes alone (one frame), and its launch has no other form to fall back to: the mates are not launched
     * on their own, a folded 1x1 has left the plan.  The launchers' limits also depend on the batch (31- / 32-bit output offsets, tile counts):
     * ask every such launch again for THIS batch and plan again without the fusion if one does not fit.  Each row sees the plan the rows
     * before it left (deferred, descriptor-only ranks take the same decisions: they depend on shapes and batch only) */
    for (size_t r = 0; r < sizeof TAKE_BACK / sizeof *TAKE_BACK; r++) {
        const take_back_t *tb = &TAKE_BACK[r];
        int *off = (int *)((char *)m + tb->flag);
        if (*off || (tb->ask == ASK_PRE && m->sw.fusion < 2)) continue;
        for (int i = 0; i < m->n_ops; i++) {
            const mars_op_t *op = &m->ops[i], *mem[4] = {op, NULL, NULL, NULL};
            int g[4], fits = 1;
            if (op->kind != OP_CONV_I8) continue;
            if (tb->ask == ASK_VCONCAT) { /* segmented convolutions address their output with 32-bit buffer offsets */
                fits = op->nseg < 2 || op->t_out < 0 || planned_stride(&m->mt[op->t_out]) * (size_t)n <= vlim;
            } else if (tb->ask == ASK_PRE) {
                const size_t in_stride = op->t_in[0] >= 0 ? planned_stride(&m->mt[op->t_in[0]]) : 0;
                fits = !op->pre || op->t_out < 0 || (conv_i8_pre_fits(op, n, in_stride, planned_stride(&m->mt[op->t_out])) && !(blim && (size_t)n > blim));
            } else {
                const int form = op_form(m, i, g);
                if (form != tb->form && form != tb->chained) continue;
                for (int q = 1; q < form_span(tb->form); q++) mem[q] = &m->ops[g[q]];
                fits = conv_i8_group_fits(m, tb->form, mem, tb->form == FORM_SPLIT_CHAIN ? op->split_chain : op->both_chain, n);
            }
            if (fits) continue;
            *off = 1;
            const mars_error_t e = replan(m);
            if (e != MARS_OK) return e;
            break;
        }
    }
    free_device_state(m);
    size_t per_frame = 0;
    for (uint32_t i = 0; i < nt; i++) {
        mtensor_t *t = &m->mt[i];
        if (t->is_weight || !t->needed) continue;
        t->stride = planned_stride(t);
        per_frame += t->stride;
    }
    m->act_bytes = per_frame * (size_t)n;
    /* + 256: vector loads may read up to 15 bytes past the last element they use (the stem's unaligned 16-byte loads
     * of 12-byte pixel groups); the slack keeps that inside the allocation for the last tensor too */
    /* 256 in front: a convolution may read a tensor through a view that starts up to 256 bytes before it (virtual_concat_f32: those
     * results are overwritten, but the addresses must be mapped for the first tensor too) */
    m->act_dev = (uint8_t *)mhip_malloc(m->act_bytes + 512);
    if (!m->act_dev) return MARS_ERR_ALLOC_FAILED;
    if (mhip_memset_async(m->act_dev, 0, m->act_bytes + 256)) return MARS_ERR_ALLOC_FAILED;
    size_t off = 256;
    for (uint32_t i = 0; i < nt; i++) {
        mtensor_t *t = &m->mt[i];
        mars_runtime_tensor_t *rt = &m->pub.tensors[i];
        if (t->is_weight) continue;
        rt->vaddr = NULL; rt->paddr = NULL; rt->alloc_size = 0;
        if (!t->needed) continue;
        t->dev = m->act_dev + off;
        off += t->stride * (size_t)n;
        rt->paddr = t->dev;
        rt->alloc_size = t->stride * (size_t)n;
        if (t->io_in || t->io_out) {
            /* what a caller may fill / read through vaddr (mars_test.c:73-84): one frame = the reference's working
             * buffer size; a batch (extension) = n densely packed frames */
            const size_t hb = t->bytes * (size_t)n, ref = reference_buffer_size(m);
            size_t cap = hb > ref ? hb : ref;
            /* what the reference can ever report is bounded by its 8 MiB arena; anything larger comes from wrapped int
             * products of a hostile descriptor (NDHWC32 / NMHWSOIB2 shapes near INT_MAX) and is not honoured: a single-frame
             * load must not pin and clear gigabytes per I/O tensor */
            if (ref > ((size_t)8 << 20)) cap = hb;
            t->host = (uint8_t *)mhip_host_alloc(cap ? cap : 64);
            if (!t->host) return MARS_ERR_ALLOC_FAILED;
            memset(t->host, 0, cap);
            rt->vaddr = t->host;
            rt->alloc_size = n == 1 && cap >= ref ? ref : hb;
        }
        if (t->pix_stride) {
            t->dense_dev = (uint8_t *)mhip_malloc(t->bytes * (size_t)n);
            if (!t->dense_dev) return MARS_ERR_ALLOC_FAILED;
        }
    }
    if (m->scratch_per_frame) {
        m->scratch_dev = (uint8_t *)mhip_malloc(ALIGN_UP(m->scratch_per_frame, 256) * (size_t)n + 256); /* (+ 256: 16-byte loads at the last pixels) */
        if (!m->scratch_dev) return MARS_ERR_ALLOC_FAILED;
    }
    m->batch = n;
    m->frame0 = 0;
    m->run_frames = n;
    return mhip_sync() ? MARS_ERR_ALLOC_FAILED : MARS_OK;
}

/* the host-only part of a load: parse, validate, plan (weights packed into the host image of the parameter arena).  No device call. */
static mars_error_t load_host(const void *data, size_t size, unsigned flags, mars_model_ext_t **out_m) {
    if (!data || !out_m || size < sizeof(mars_header_t)) return MARS_ERR_INVALID_FILE;
    const uint8_t *p = (const uint8_t *)data;
    mars_header_t h;
    memcpy(&h, p, sizeof(h));
    if (h.magic != MARS_MAGIC) {
        VLOG("Invalid magic 0x%08x (expected 0x%08x)\n", h.magic, MARS_MAGIC);
        return MARS_ERR_INVALID_MAGIC;
    }
    if (h.version_major != MARS_VERSION_MAJOR) return MARS_ERR_VERSION_MISMATCH;
    /* superset of the reference: it trusts every count and offset (mars_runtime.c:172-200, 220) */
    if (h.num_tensors > 65536 || h.num_layers > 65536 || h.num_inputs > 4 || h.num_outputs > 4) return MARS_ERR_INVALID_FILE;
    const size_t tables = sizeof(h) + (size_t)h.num_tensors * sizeof(mars_tensor_t) + (size_t)h.num_layers * sizeof(mars_layer_t);
    if (tables > size) return MARS_ERR_INVALID_FILE;
    const int deferred = (flags & MARS_HIP_LOAD_DEFER_WEIGHTS) != 0;
    if (!deferred && h.weights_size > 0 && (h.weights_offset > size || h.weights_size > size - h.weights_offset))
        return MARS_ERR_INVALID_FILE;
    if (h.weights_size > ((uint64_t)1 << 36)) return MARS_ERR_INVALID_FILE;

    mars_model_ext_t *m = (mars_model_ext_t *)calloc(1, sizeof(*m));
    if (!m) return MARS_ERR_ALLOC_FAILED;
    m->pub.header = h;
    plan_switches_read(&m->sw, 1);
    m->deferred = deferred;
    m->pub.tensors = (mars_runtime_tensor_t *)calloc(h.num_tensors ? h.num_tensors : 1, sizeof(mars_runtime_tensor_t));
    m->pub.layers = (mars_runtime_layer_t *)calloc(h.num_layers ? h.num_layers : 1, sizeof(mars_runtime_layer_t));
    m->mt = (mtensor_t *)calloc(h.num_tensors ? h.num_tensors : 1, sizeof(mtensor_t));
    m->layer_noop = (unsigned char *)calloc(h.num_layers ? h.num_layers : 1, 1);
    if (!m->pub.tensors || !m->pub.layers || !m->mt || !m->layer_noop) { mars_free(&m->pub); return MARS_ERR_ALLOC_FAILED; }
    const uint8_t *q = p + sizeof(h);
    for (uint32_t i = 0; i < h.num_tensors; i++, q += sizeof(mars_tensor_t)) memcpy(&m->pub.tensors[i].desc, q, sizeof(mars_tensor_t));
    for (uint32_t i = 0; i < h.num_layers; i++, q += sizeof(mars_layer_t)) memcpy(&m->pub.layers[i].desc, q, sizeof(mars_layer_t));

    m->pub.weights_size = (size_t)h.weights_size;
    if (h.weights_size) {
        m->pub.weights = calloc(1, (size_t)h.weights_size);
        if (!m->pub.weights) { mars_free(&m->pub); return MARS_ERR_ALLOC_FAILED; }
        if (!deferred) memcpy(m->pub.weights, p + h.weights_offset, (size_t)h.weights_size);
    }
    m->pub.ddr_base = m->pub.weights;
    for (uint32_t i = 0; i < h.num_tensors; i++) {
        mars_runtime_tensor_t *rt = &m->pub.tensors[i];
        if (rt->desc.ndims > MARS_MAX_DIMS) { mars_free(&m->pub); return MARS_ERR_INVALID_FILE; }
        m->mt[i].bytes = shape_numel(&rt->desc) * elem_size(rt->desc.dtype);
        if (rt->desc.data_size > 0) {
            if (rt->desc.data_offset > h.weights_size) { mars_free(&m->pub); return MARS_ERR_INVALID_FILE; }
            m->mt[i].is_weight = 1;
            rt->vaddr = (uint8_t *)m->pub.weights + rt->desc.data_offset;
            rt->alloc_size = (size_t)rt->desc.data_size;
        }
    }
    for (uint32_t i = 0; i < h.num_inputs; i++) {
        uint32_t id = h.input_tensor_ids[i];
        if (id < h.num_tensors && !m->mt[id].is_weight) m->mt[id].io_in = (int)i + 1;
    }
    for (uint32_t i = 0; i < h.num_outputs; i++) {
        uint32_t id = h.output_tensor_ids[i];
        if (id < h.num_tensors && !m->mt[id].is_weight) m->mt[id].io_out = (int)i + 1;
    }

    mars_error_t err = build_plan(m);
    if (err != MARS_OK) { mars_free(&m->pub); return err; }
    VLOG("%u layers -> %d launches, parameter arena %zu bytes\n", h.num_layers, m->n_ops, m->arena_size);
    *out_m = m;
    return MARS_OK;
}

mars_error_t mars_hip_load_memory_ex(const void *data, size_t size, unsigned flags, mars_model_t **out_model) {
    if (!out_model) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = NULL;
    mars_error_t err = load_host(data, size, flags, &m);
    if (err != MARS_OK) return err;
    /* everything above is host-only; from here on a GPU is required.  No CPU fallback. */
    if (!nna_is_ready() || !mhip_ready()) {
        fprintf(stderr, "Mars: no initialised MI355X device (call nna_init first); refusing to load\n");
        mars_free(&m->pub);
        return MARS_ERR_NNA_INIT_FAILED;
    }
    err = upload_params(m);
    if (err == MARS_OK) err = alloc_batch(m, 1);
    if (err != MARS_OK) { mars_free(&m->pub); return err; }
    m->live_next = g_live_models;
    g_live_models = m;
    *out_model = &m->pub;
    return MARS_OK;
}

/* MARS_HIP_DESCRIBE_FULL: every scalar field of a launch that the run path reads, appended to its line at k (pointers, events and timings are not plan) */
static int describe_op_full(const mars_op_t *o, char *line, size_t cap, int k) {
#define ADD(...) k += snprintf(line + k, cap - (size_t)k, __VA_ARGS__)
    ADD(" | err %d in %dx%dx%d out %dx%dx%d k %dx%d s %dx%d p %d,%d", o->err, o->in_h, o->in_w, o->in_c, o->out_h, o->out_w, o->out_c, o->kh, o->kw, o->sh, o->sw, o->pt, o->pl);
    ADD(" nchw %d out_nchw %d relu %d is_mul %d is_f32 %d leaky %d safe %d silu %d f32_exact %d variant %d", o->nchw, o->out_nchw, o->relu, o->is_mul, o->is_f32, o->leaky,
        o->safe, o->silu_f32, o->f32_exact, o->variant);
    ADD(" row_pad %d oc_pad %d c_pad %d store_c %d ch_off %d out_ch_off %d out_pix_stride %d in_byte_off %zu out_byte_off %zu scale %dx%d bn_n %d n %zu", o->row_pad,
        o->oc_pad, o->c_pad, o->store_c, o->ch_off, o->out_ch_off, o->out_pix_stride, o->in_byte_off, o->out_byte_off, o->scale_h, o->scale_w, o->bn_n, o->n);
    ADD(" k_limit %d rows_only %d pair_next %d in_rec %d out_rec %d vc %d,%d,%d:", o->k_limit, o->rows_only, o->pair_next, o->in_rec, o->out_rec, o->vc_n, o->vc_run, o->vc_shift);
    for (int q = 0; q < o->vc_n && q < 3; q++) ADD(" %d", o->vc_t[q]);
    ADD(" add %d %a %a %a seg %d up %d:", o->add_t, (double)o->add_s_conv, (double)o->add_s_other, (double)o->add_inv, o->nseg, o->seg_up);
    for (int q = 0; q < o->nseg && q < 4; q++) ADD(" %d/%d", o->seg_t[q], o->seg_c[q]);
    ADD(" chain %d:", o->chain_n);
    for (int q = 0; q < o->chain_n && q < 3; q++) ADD(" %d", o->chain_out[q]);
    ADD(" cs %a f %a %a %a", (double)o->cs, (double)o->f0, (double)o->f1, (double)o->f2);
    ADD(" w_off %zd b_off %zd lut_off %zd lut2_off %zd s_off %zd w2_off %zd rows %d planes %d w3_off %zd stem %d blob %zd %zd", (ssize_t)o->w_off, (ssize_t)o->b_off,
        (ssize_t)o->lut_off, (ssize_t)o->lut2_off, (ssize_t)o->s_off, (ssize_t)o->w2_off, o->w2_rows, o->w2_planes, (ssize_t)o->w3_off, o->w3_stem, (ssize_t)o->w_blob_off[0],
        (ssize_t)o->w_blob_off[1]);
    ADD(" post_next %d", o->post_next);
    if (o->post_next) ADD(" %zd", (ssize_t)o->post_w_off);
    ADD(" split_next %d", o->split_next);
    if (o->split_next) ADD(" %zd", (ssize_t)o->split_w_off);
    ADD(" split_chain %d", o->split_chain);
    if (o->split_chain) ADD(" %zd", (ssize_t)o->chain_w_off);
    ADD(" pair_both %d both_chain %d both_elide %d", o->pair_both, o->both_chain, o->both_elide);
    ADD(" pre %d", o->pre);
    if (o->pre) ADD(" %zd %zd %zd %a", (ssize_t)o->pre_w_off, (ssize_t)o->pre_b_off, (ssize_t)o->pre_lut2_off, (double)o->pre_cs);
    ADD(" macs %a bytes %a prof_kind %d", o->macs, o->bytes, o->prof_kind);
#undef ADD
    return k;
}

/* The plan of a file as text, WITHOUT a device (tests of the planner on the CPU: which layers fuse, which tensors are kept pixels x channels,
 * which K loops are cut ...): one line per launch -- "op I layer L KIND in T.. out T" + the flags that are set -- and one per tensor that is not
 * held as tagged.  Returns the length needed (the text is cut at cap); 0 on a file the loader rejects.
 * MARS_HIP_DESCRIBE_FULL adds, and alters nothing: " | ..." behind those lines and whole lines that start with "+" (include/mars_hip.h). */
size_t mars_hip_describe_plan(const void *data, size_t size, unsigned flags, char *out, size_t cap) {
    static const char *const kinds[] = {"conv_i8", "conv_f32", "relu_bytes", "lut_i8", "binary_i8", "sigmoid_f32", "binary_f32", "relu_f32", "bn",
                                        "maxpool", "concat_slice", "upsample", "upsample_q", "maxpool_q", "concat_q", "conv_f32_vhead", "fail"};
    mars_model_ext_t *m = NULL;
    const int full = (flags & MARS_HIP_DESCRIBE_FULL) != 0;
    if (load_host(data, size, flags & ~MARS_HIP_DESCRIBE_FULL, &m) != MARS_OK) return 0;
    size_t n = 0;
    char line[4096];
#define EMIT() do { const size_t l = strlen(line); if (out && n < cap) memcpy(out + n, line, n + l <= cap ? l : cap - n); n += l; } while (0)
    for (int i = 0; i < m->n_ops; i++) {
        const mars_op_t *o = &m->ops[i];
        int k = snprintf(line, sizeof line, "op %d layer %d %s in", i, o->layer, o->kind >= 0 && o->kind <= OP_FAIL ? kinds[o->kind] : "?");
        for (int q = 0; q < o->n_in && q < 4; q++) k += snprintf(line + k, sizeof line - (size_t)k, " %d", o->t_in[q]);
        k += snprintf(line + k, sizeof line - (size_t)k, " out %d", o->t_out);
#define FLAG(cond, ...) if (cond) k += snprintf(line + k, sizeof line - (size_t)k, __VA_ARGS__)
        FLAG(o->kind == OP_CONV_I8 || o->kind == OP_CONV_F32 || o->kind == OP_CONV_F32_VHEAD, " k%dx%d s%d c%d->%d", o->kh, o->kw, o->sw, o->in_c, o->out_c);
        FLAG(o->nchw, " relayout"); FLAG(o->out_nchw, " planar_store"); FLAG(o->lut_off != NO_OFF, " lut"); FLAG(o->add_t, " add=%d", o->add_t - 1);
        FLAG(o->nseg, " seg=%d", o->nseg); FLAG(o->pair_next && !(o->pair_both && o->nseg), " pair_next"); /* (a pair over a concat exists in the one-tile form only: pair_both says it all) */ FLAG(o->pair_both, " pair_both"); FLAG(o->both_chain, " both_chain=%d", o->both_chain); FLAG(o->both_elide, " both_elide"); FLAG(o->post_next, " post_next"); FLAG(o->split_next, " split_next"); FLAG(o->pre, " pre"); FLAG(o->silu_f32, " silu");
        FLAG(o->k_limit, " k_limit=%d", o->k_limit); FLAG(o->in_rec, " in_rec=%d", o->in_rec); FLAG(o->out_rec, " out_rec");
        FLAG(o->vc_shift, " view=-%d", o->vc_shift); FLAG(o->vc_n, " vcat=%dx%d", o->vc_n, o->vc_run);
        FLAG(o->rows_only, " rows_only=%d", o->rows_only); FLAG(o->out_byte_off, " out_off=%zu", o->out_byte_off); FLAG(o->chain_n, " chain=%d", o->chain_n);
        FLAG(o->out_pix_stride, " pix_stride=%d", o->out_pix_stride); FLAG(o->kind == OP_FAIL, " err=%d", o->err);
#undef FLAG
        if (full) k = describe_op_full(o, line, sizeof line, k);
        snprintf(line + k, sizeof line - (size_t)k, "\n");
        EMIT();
    }
    for (uint32_t t = 0; t < m->pub.header.num_tensors; t++) {
        const mtensor_t *mt = &m->mt[t];
        const int listed = mt->nhwc_c || mt->partial || mt->zero_from || mt->rec_c || mt->pix_stride;
        if (!listed && !(full && mt->needed)) continue;
        int k = listed ? snprintf(line, sizeof line, "tensor %u nhwc_c %d pitch %d partial %d zero_from %zu rec_c %d pix_stride %d", t, mt->nhwc_c, mt->nhwc_pitch,
                                  mt->partial, mt->zero_from, mt->rec_c, mt->pix_stride)
                       : snprintf(line, sizeof line, "+tensor %u", t);
        if (full)
            k += snprintf(line + k, sizeof line - (size_t)k, " | bytes %zu extent %zu needed %d tail_read %d weight %d io %d,%d pix_c %d rec_hw %d nhwc_hw %d", mt->bytes,
                          mt->extent, mt->needed, mt->tail_read, mt->is_weight, mt->io_in, mt->io_out, mt->pix_c, mt->rec_hw, mt->nhwc_hw);
        snprintf(line + k, sizeof line - (size_t)k, "\n");
        EMIT();
    }
    if (full) {
        const plan_switches_t *w = &m->sw;
        snprintf(line, sizeof line, "+plan n_ops %d arena_size %zu scratch_per_frame %zu blob_mirror_bytes %zu rec_max_frames %zu rec_skipped %d f32_mode %d | fusion %d"
                 " no_fuse_lut %d no_nhwc_internal %d no_vconcat_q %d no_pair_f32 %d no_rec %d no_zero_tail %d no_vconcat_f32 %d no_rowpad %d no_post %d no_split %d no_chain %d no_both %d no_both_chain %d rec_limit %zu"
                 " vconcat_limit %zu bottleneck_limit %zu\n", m->n_ops, m->arena_size, m->scratch_per_frame, m->blob_mirror_bytes, m->rec_max_frames, m->rec_skipped,
                 m->plan_f32_mode, w->fusion, w->no_fuse_lut, w->no_nhwc_internal, w->no_vconcat_q, w->no_pair_f32, w->no_rec, w->no_zero_tail, w->no_vconcat_f32,
                 w->no_rowpad, w->no_post, w->no_split, w->no_chain, w->no_both, w->no_both_chain, w->rec_limit, w->vconcat_limit, w->bottleneck_limit);
        EMIT();
    }
#undef EMIT
    if (out && cap) out[n < cap ? n : cap - 1] = 0;
    mars_free(&m->pub);
    return n;
}

/* anchor-based YOLOv5 heads of a file, host only: the loader's parse and plan (which layers are no-ops), then mars_find_heads */
int mars_yolo_find_heads(const void *data, size_t size, int *tensor_ids, int *strides, int *num_classes, int cap) {
    mars_model_ext_t *m = NULL;
    if (load_host(data, size, 0, &m) != MARS_OK) return -1;
    const int n = mars_find_heads(m, tensor_ids, strides, num_classes, cap);
    mars_free(&m->pub);
    return n;
}

/* ... and its anchor-free DFL heads (mars_find_dfl_heads) */
int mars_yolo_find_dfl_heads(const void *data, size_t size, int *box_ids, int *cls_ids, int *strides, int *num_classes, int *reg_max, int cap) {
    mars_model_ext_t *m = NULL;
    if (load_host(data, size, 0, &m) != MARS_OK) return -1;
    const int n = mars_find_dfl_heads(m, box_ids, cls_ids, strides, num_classes, reg_max, cap);
    mars_free(&m->pub);
    return n;
}

mars_error_t mars_load_memory(const void *data, size_t size, mars_model_t **model) {
    return mars_hip_load_memory_ex(data, size, 0, model);
}

mars_error_t mars_load_file(const char *path, mars_model_t **model) {
    if (!path || !model) return MARS_ERR_INVALID_FILE;
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        fprintf(stderr, "Mars: Cannot open %s\n", path);
        return MARS_ERR_INVALID_FILE;
    }
    fseek(fp, 0, SEEK_END);
    long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (size <= 0) { fclose(fp); return MARS_ERR_INVALID_FILE; }
    void *buf = malloc((size_t)size);
    if (!buf) { fclose(fp); return MARS_ERR_ALLOC_FAILED; }
    if (fread(buf, 1, (size_t)size, fp) != (size_t)size) { free(buf); fclose(fp); return MARS_ERR_INVALID_FILE; }
    fclose(fp);
    mars_error_t err = mars_load_memory(buf, (size_t)size, model);
    free(buf); /* the model keeps its own copy (reference :384) */
    return err;
}

/* ---------------------------------------------------------------- accessors */
mars_runtime_tensor_t *mars_get_input(mars_model_t *model, int index) {
    if (!model || index < 0 || (uint32_t)index >= model->header.num_inputs) return NULL;
    uint32_t tid = model->header.input_tensor_ids[index];
    if (tid >= model->header.num_tensors) return NULL;
    return &model->tensors[tid];
}

mars_runtime_tensor_t *mars_get_output(mars_model_t *model, int index) {
    if (!model || index < 0 || (uint32_t)index >= model->header.num_outputs) return NULL;
    uint32_t tid = model->header.output_tensor_ids[index];
    if (tid >= model->header.num_tensors) return NULL;
    return &model->tensors[tid];
}

int mars_get_num_inputs(mars_model_t *model) { return model ? (int)model->header.num_inputs : 0; }
int mars_get_num_outputs(mars_model_t *model) { return model ? (int)model->header.num_outputs : 0; }

void mars_print_summary(mars_model_t *model) {
    if (!model) return;
    mars_model_ext_t *m = (mars_model_ext_t *)model;
    printf("\nMars model summary (MI355X)\n");
    printf("Layers: %u\n", model->header.num_layers);
    printf("Tensors: %u\n", model->header.num_tensors);
    printf("Inputs: %u\n", model->header.num_inputs);
    printf("Outputs: %u\n", model->header.num_outputs);
    printf("Weights: %zu bytes\n", model->weights_size);
    printf("Launches per run: %d, batch %d, activations %zu bytes, parameters %zu bytes\n\n", m->n_ops, m->batch,
           m->act_bytes, m->arena_size);
}

