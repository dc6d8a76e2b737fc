/*
 * mars_roi.c -- host side of the ROI crops (include/mars_hip.h, "ROI crops", "Rotated crops" and "Aligned crops"): argument checks, the ROI and fit
 * tables hung on the destination model, stream ordering, and the launches of csrc/hip/roi.hip.  The reference stops at the boxes (src/mars/mars_yolo_test.c:132-214);
 * a second stage there would cut crops on the host.  There is no CPU pixel path here: without the device every entry point fails.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../align_fit.h"
#include "../mhip.h"
#include "mars_hip.h"
#include "mars_internal.h"

/* the checks that need no device and no model, and the defaults resolved into the launch record */
static mars_error_t roi_opts(const mars_hip_roi_opts_t *o, int tw, int th, mhip_roi_t *p) {
    memset(p, 0, sizeof(*p));
    if (!o || o->src_w <= 0 || o->src_h <= 0 || tw <= 0 || th <= 0) return MARS_ERR_INVALID_FILE;
    if (!mhip_frame_format_ok(o->src_format, o->src_flags) || !mhip_frame_bytes(o->src_w, o->src_h, o->src_format)) return MARS_ERR_INVALID_FILE;
    if (o->flags & ~(MARS_ROI_KEEP_ASPECT | MARS_ROI_AREA)) return MARS_ERR_INVALID_FILE;
    if (!isfinite(o->expand) || o->expand < 0 || !isfinite(o->min_conf) || o->min_size < 0 || o->cls_count < 0 || o->max_per_frame < 0)
        return MARS_ERR_INVALID_FILE;
    if (!mhip_roi_fits(o->src_w, tw, o->src_format)) return MARS_ERR_INVALID_FILE;
    if ((o->flags & MARS_ROI_AREA) && !mhip_roi_area_fits(o->src_w, tw, o->src_format)) return MARS_ERR_INVALID_FILE;
    p->w = o->src_w; p->h = o->src_h; p->fmt = o->src_format; p->nv12_flags = o->src_flags;
    p->frame_stride = mhip_frame_bytes(p->w, p->h, p->fmt);
    p->expand = o->expand != 0 ? o->expand : 1.0f;
    p->min_conf = o->min_conf;
    p->min_size = o->min_size ? o->min_size : 2;
    p->cls_first = o->cls_first; p->cls_count = o->cls_count; p->max_per_frame = o->max_per_frame;
    p->keep_aspect = (o->flags & MARS_ROI_KEEP_ASPECT) != 0;
    p->area = (o->flags & MARS_ROI_AREA) != 0;
    p->tw = tw; p->th = th;
    return MARS_OK;
}

/* ... and what the rotated forms refuse on top */
static mars_error_t rot_opts(const mars_hip_roi_opts_t *o, int tw, int th, mhip_roi_t *p) {
    if (o && (o->flags & MARS_ROI_AREA)) return MARS_ERR_INVALID_FILE; /* an area filter along a rotated box is another kernel */
    const mars_error_t e = roi_opts(o, tw, th, p);
    if (e != MARS_OK) return e;
    return mhip_roi_rot_fits(o->src_w, o->src_h, tw) ? MARS_OK : MARS_ERR_INVALID_FILE;
}

/* ... and the aligned forms: the two geometry flags, and the template, which goes into the launch record with the resolved mask */
static mars_error_t align_opts(const mars_hip_roi_opts_t *o, const mars_hip_align_opts_t *a, int tw, int th, mhip_roi_t *p) {
    if (o && (o->flags & (MARS_ROI_KEEP_ASPECT | MARS_ROI_AREA))) return MARS_ERR_INVALID_FILE; /* the template fixes the geometry; the sampler has four taps */
    const mars_error_t e = rot_opts(o, tw, th, p);
    if (e != MARS_OK) return e;
    if (!a || a->num_kpt < 1 || a->num_kpt > MARS_POSE_MAX_KPT || !isfinite(a->min_vis)) return MARS_ERR_INVALID_FILE;
    const unsigned all = a->num_kpt == 32 ? ~0u : (1u << a->num_kpt) - 1u;
    if (a->use & ~all) return MARS_ERR_INVALID_FILE;
    for (int j = 0; j < a->num_kpt; j++)
        if (!isfinite(a->tmpl[j][0]) || !isfinite(a->tmpl[j][1])) return MARS_ERR_INVALID_FILE;
    p->num_kpt = a->num_kpt;
    p->use = a->use ? a->use : all;
    p->min_vis = a->min_vis;
    memcpy(p->tmpl, a->tmpl, (size_t)a->num_kpt * sizeof(a->tmpl[0]));
    return MARS_OK;
}

/* "Aligned crops" on the host: align_fit of csrc/align_fit.h, the text the device compiles too; 0 = skipped */
_Static_assert(sizeof(align_kpt_t) == sizeof(mars_kpt_t) && sizeof(align_t) == sizeof(mars_align_t), "align_fit.h restates mars_kpt_t and mars_align_t");
int mars_yolo_align_fit(const mars_kpt_t *kpts, const mars_hip_align_opts_t *align, const mars_hip_roi_opts_t *opts, int tw, int th, mars_align_t *fit,
                        mars_roi_t *roi) {
    mhip_roi_t p;
    if (!kpts || !fit || align_opts(opts, align, tw, th, &p) != MARS_OK) return -1;
    int r[4];
    const int kept = align_fit((const align_kpt_t *)kpts, &p, (align_t *)fit, r);
    if (roi) { roi->x0 = r[0]; roi->y0 = r[1]; roi->x1 = r[2]; roi->y1 = r[3]; }
    return kept;
}

int mars_yolo_align_template_face5(int tw, int th, float tmpl[][2]) {
    /* the five landmark positions of the public ArcFace alignment for a 112 x 112 crop: eyes, nose tip, mouth corners */
    static const float ref[5][2] = {{38.2946f, 51.6963f}, {73.5318f, 51.5014f}, {56.0252f, 71.7366f}, {41.5493f, 92.3655f}, {70.7299f, 92.2041f}};
    if (!tmpl || tw <= 0 || th <= 0) return -1;
    for (int j = 0; j < 5; j++) {
        tmpl[j][0] = ref[j][0] * ((float)tw / 112.0f);
        tmpl[j][1] = ref[j][1] * ((float)th / 112.0f);
    }
    return 5;
}

/* the host-pointer forms: boxes of box_b bytes each; csn != NULL: oriented boxes and their (cos, sin) pairs; fits != NULL: keypoint sets ("Aligned crops") */
static mars_error_t crop_host(const unsigned char *frames, int n_frames, const void *boxes, size_t box_b, const float *csn, const int *frame_of_box, int n_boxes,
                              mhip_roi_t p, int nhwc, signed char *out, mars_roi_t *rois, mars_align_t *fits) {
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const size_t in_b = p.frame_stride * (size_t)n_frames, out_b = (size_t)p.tw * p.th * 3;
    /* one device block: [frames][boxes][frame_of_box][counters][rois][out][(cos, sin) pairs][fit records] */
    size_t off[8];
    const size_t sz[8] = {in_b, (size_t)n_boxes * box_b, (size_t)n_boxes * sizeof(int), 16, (size_t)n_boxes * sizeof(mars_roi_t),
                          out_b * (size_t)n_boxes, csn ? (size_t)n_boxes * 2 * sizeof(float) : 0, fits ? (size_t)n_boxes * sizeof(mars_align_t) : 0};
    uint8_t *d = (uint8_t *)mhip_malloc(mars_block_layout(sz, 8, off));
    if (!d) return MARS_ERR_ALLOC_FAILED;
    p.frames = d; p.n_frames = n_frames;
    p.boxes = d + off[1]; p.frame_of_box = (const int *)(d + off[2]); p.n_boxes = n_boxes;
    p.n_out = (int *)(d + off[3]); p.rois = d + off[4];
    p.out = (int8_t *)(d + off[5]); p.out_stride = out_b; p.slots = n_boxes; p.nhwc = nhwc != 0;
    if (csn) p.csn = (const float *)(d + off[6]);
    if (fits) p.fits = d + off[7];
    int rc = mhip_h2d_async(d, frames, in_b);
    if (!rc) rc = mhip_h2d_async(d + off[1], boxes, sz[1]);
    if (!rc) rc = mhip_h2d_async(d + off[2], frame_of_box, sz[2]);
    if (!rc && csn) rc = mhip_h2d_async(d + off[6], csn, sz[6]);
    if (!rc) rc = fits ? mhip_roi_align_rects(&p) : csn ? mhip_roi_rot_rects(&p) : mhip_roi_rects(&p);
    if (!rc) rc = fits ? mhip_roi_align_crop(&p) : csn ? mhip_roi_rot_crop(&p) : mhip_roi_crop(&p);
    if (!rc) rc = mhip_d2h_async(out, p.out, sz[5]);
    if (!rc && rois) rc = mhip_d2h_async(rois, p.rois, sz[4]);
    if (!rc && fits) rc = mhip_d2h_async(fits, p.fits, sz[7]);
    if (mhip_sync()) rc = -1;
    mhip_free(d);
    return rc ? MARS_ERR_LAYER_FAILED : MARS_OK;
}

mars_error_t mars_yolo_crop_boxes(const unsigned char *frames, int n_frames, const mars_det_t *boxes, const int *frame_of_box, int n_boxes,
                                  const mars_hip_roi_opts_t *opts, int tw, int th, int nhwc, signed char *out, mars_roi_t *rois) {
    mhip_roi_t p;
    const mars_error_t e = roi_opts(opts, tw, th, &p);
    if (e != MARS_OK) return e;
    if (!frames || !boxes || !frame_of_box || !out || n_frames <= 0 || n_boxes <= 0 || n_boxes > 65535) return MARS_ERR_INVALID_FILE;
    return crop_host(frames, n_frames, boxes, sizeof(mars_det_t), NULL, frame_of_box, n_boxes, p, nhwc, out, rois, NULL);
}

mars_error_t mars_yolo_crop_obb(const unsigned char *frames, int n_frames, const mars_obb_t *boxes, const int *frame_of_box, int n_boxes,
                                const mars_hip_roi_opts_t *opts, int tw, int th, int nhwc, signed char *out, mars_roi_t *rois) {
    mhip_roi_t p;
    const mars_error_t e = rot_opts(opts, tw, th, &p);
    if (e != MARS_OK) return e;
    if (!frames || !boxes || !frame_of_box || !out || n_frames <= 0 || n_boxes <= 0 || n_boxes > 65535) return MARS_ERR_INVALID_FILE;
    float *csn = (float *)malloc((size_t)n_boxes * 2 * sizeof(float)); /* the host libm's, as mars_yolo_obb_nms takes them */
    if (!csn) return MARS_ERR_ALLOC_FAILED;
    for (int i = 0; i < n_boxes; i++) {
        csn[2 * i] = cosf(boxes[i].angle);
        csn[2 * i + 1] = sinf(boxes[i].angle);
    }
    const mars_error_t rc = crop_host(frames, n_frames, boxes, sizeof(mars_obb_t), csn, frame_of_box, n_boxes, p, nhwc, out, rois, NULL);
    free(csn);
    return rc;
}

mars_error_t mars_yolo_crop_aligned(const unsigned char *frames, int n_frames, const mars_kpt_t *kpts, const int *frame_of_box, int n_boxes,
                                    const mars_hip_align_opts_t *align, const mars_hip_roi_opts_t *opts, int tw, int th, int nhwc, signed char *out,
                                    mars_roi_t *rois, mars_align_t *fits) {
    mhip_roi_t p;
    const mars_error_t e = align_opts(opts, align, tw, th, &p);
    if (e != MARS_OK) return e;
    if (!frames || !kpts || !frame_of_box || !out || n_frames <= 0 || n_boxes <= 0 || n_boxes > 65535) return MARS_ERR_INVALID_FILE;
    mars_align_t *own = fits ? NULL : (mars_align_t *)malloc((size_t)n_boxes * sizeof(mars_align_t)); /* the sampler reads the table either way */
    if (!fits && !own) return MARS_ERR_ALLOC_FAILED;
    const mars_error_t rc = crop_host(frames, n_frames, kpts, (size_t)p.num_kpt * sizeof(mars_kpt_t), NULL, frame_of_box, n_boxes, p, nhwc, out, rois,
                                      fits ? fits : own);
    free(own);
    return rc;
}

void mars_roi_release(mars_model_ext_t *m) {
    if (m->roi_dev) mhip_free(m->roi_dev);
    if (m->roi_fit_dev) mhip_free(m->roi_fit_dev);
    m->roi_dev = m->roi_fit_dev = NULL;
    m->roi_cap_slots = m->roi_cap_frames = m->roi_slots = m->roi_fit_slots = 0;
    m->roi_from = NULL;
}

/* the table of `slots` crops out of `frames` source frames, on the destination model; only ever grown.  fits: and a fit record per slot
 * beside it ("Aligned crops"), kept from then on */
static int roi_table(mars_model_ext_t *m, int slots, int frames, int fits) {
    if (m->roi_dev && m->roi_cap_slots >= slots && m->roi_cap_frames >= frames && (!fits || m->roi_fit_dev)) return 0;
    if (m->roi_dev && mhip_sync()) return -1; /* kernels queued earlier may still use the old one */
    const int cs = slots > m->roi_cap_slots ? slots : m->roi_cap_slots, cf = frames > m->roi_cap_frames ? frames : m->roi_cap_frames;
    fits = fits || m->roi_fit_dev;
    mars_roi_release(m);
    m->roi_dev = mhip_malloc(16 + (size_t)cs * sizeof(mars_roi_t) + (size_t)cf * sizeof(int));
    if (m->roi_dev && fits) m->roi_fit_dev = mhip_malloc((size_t)cs * sizeof(mars_align_t));
    if (!m->roi_dev || (fits && !m->roi_fit_dev)) {
        mars_roi_release(m);
        return -1;
    }
    m->roi_cap_slots = cs; m->roi_cap_frames = cf;
    return 0;
}

/* the options of a crop mode: upright, oriented (MODE_ROT), aligned (MODE_ALIGN, with its template) */
#define MODE_ROT 1
#define MODE_ALIGN 2
static mars_error_t mode_opts(int mode, const mars_hip_roi_opts_t *o, const mars_hip_align_opts_t *a, int tw, int th, mhip_roi_t *p) {
    return mode == MODE_ALIGN ? align_opts(o, a, tw, th, p) : mode == MODE_ROT ? rot_opts(o, tw, th, p) : roi_opts(o, tw, th, p);
}

/* the device chain; MODE_ROT: over the oriented boxes of det_model's last obb call; MODE_ALIGN: over the keypoints of its last pose call */
static mars_error_t crop_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index, const mars_hip_roi_opts_t *opts,
                                int mode, const mars_hip_align_opts_t *align) {
    const int rot = mode == MODE_ROT;
    if (!det_model || !dst_model || !frames_dev || !opts) return MARS_ERR_INVALID_FILE;
    { /* what can be said without looking at either model */
        mhip_roi_t q;
        const mars_error_t e = mode_opts(mode, opts, align, 1, 1, &q);
        if (e != MARS_OK) return e;
    }
    if (det_model == dst_model) return MARS_ERR_INVALID_TENSOR;
    mars_model_ext_t *det = (mars_model_ext_t *)det_model, *m = (mars_model_ext_t *)dst_model;
    if (!m->act_dev || !det->act_dev || !mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    if (m->pipe || det->pipe) return MARS_ERR_INVALID_TENSOR; /* a pipe's slots own their buffers */
    mars_pixel_input_t in;
    if (mars_pixel_input(m, input_index, 0, &in) != MARS_OK) return MARS_ERR_INVALID_TENSOR;
    if (!mars_has_dets(det)) return MARS_ERR_INVALID_TENSOR;                                                /* no detections in HBM */
    if (rot && (!det->obb.dev || det->obb.frames != det->batch)) return MARS_ERR_INVALID_TENSOR;            /* no obb results in HBM */
    if (mode == MODE_ALIGN && (!det->pose.dev || det->pose.frames != det->batch || det->pose_k != align->num_kpt))
        return MARS_ERR_INVALID_TENSOR;                                                                     /* no pose results in HBM, or of another K */
    mhip_roi_t p;
    const mars_error_t e = mode_opts(mode, opts, align, in.tw, in.th, &p);
    if (e != MARS_OK) return e;
    if (m->batch > 65535) return MARS_ERR_INVALID_TENSOR;
    if (roi_table(m, m->batch, det->batch, mode == MODE_ALIGN)) return MARS_ERR_ALLOC_FAILED;
    p.frames = (const uint8_t *)frames_dev; p.n_frames = det->batch;
    if (rot) { /* the kept records, their counts and their (cos, sin) pairs: index-aligned with the detection list */
        const uint8_t *blk = (const uint8_t *)det->obb.dev;
        p.dets = blk + det->obb_out_off; p.counts = (const int *)(blk + det->obb_cnt_off); p.csn = (const float *)(blk + det->obb_csn_off);
    } else {
        p.dets = det->det_dev; p.counts = det->det_counts_dev;
    }
    if (mode == MODE_ALIGN) { /* the slots of the pose block; their det fields index the detection list above */
        const uint8_t *blk = (const uint8_t *)det->pose.dev;
        p.pose_recs = blk + det->pose_rec_off; p.pose_kpts = blk + det->pose_kpt_off; p.pose_max = det->pose_max;
        p.fits = m->roi_fit_dev;
    }
    p.det_cap = MARS_YOLO_MAX_DET;
    p.n_out = (int *)m->roi_dev;
    p.rois = (uint8_t *)m->roi_dev + 16;
    p.frame_kept = (int *)((uint8_t *)m->roi_dev + 16 + (size_t)m->roi_cap_slots * sizeof(mars_roi_t));
    p.out = in.dev; p.out_stride = in.stride; p.slots = m->batch; p.nhwc = in.nhwc;
    /* The main stream.  It carries every run of dst_model (the parts of a large batch join it again), so the crops come behind an earlier
     * graph that still reads the input and ahead of the next one.  The detections come from the auxiliary stream: wait for the event the
     * tail recorded there -- the one the next run's head-writing layers of det_model wait for */
    mhip_select_stream(0);
    if (det->ev_tail_done && mhip_stream_wait(0, det->ev_tail_done)) return MARS_ERR_LAYER_FAILED;
    if (m->label_pending) { /* a label scatter (mars_hip_label_detections_device, auxiliary stream) still reads the table this call rewrites */
        if (mhip_stream_wait(0, m->ev_label_done)) return MARS_ERR_LAYER_FAILED;
        m->label_pending = 0;
    }
    if (m->shot_pending) { /* ... or a shots call (mars_hip_shots_device, auxiliary stream) still reads the input and the table */
        if (mhip_stream_wait(0, m->ev_shot_done)) return MARS_ERR_LAYER_FAILED;
        m->shot_pending = 0;
    }
    if (mode == MODE_ALIGN ? (mhip_roi_align_select(&p) || mhip_roi_align_crop(&p))
                           : rot ? (mhip_roi_rot_select(&p) || mhip_roi_rot_crop(&p)) : (mhip_roi_select(&p) || mhip_roi_crop(&p)))
        return MARS_ERR_LAYER_FAILED;
    m->roi_slots = m->batch;
    m->roi_fit_slots = mode == MODE_ALIGN ? m->batch : 0;
    m->roi_from = det;
    return MARS_OK;
}

/* the same with the frames in host memory: upload, crop, wait */
static mars_error_t crop_upload(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index, const mars_hip_roi_opts_t *opts,
                                int mode, const mars_hip_align_opts_t *align) {
    if (!det_model || !dst_model || !frames || !opts) return MARS_ERR_INVALID_FILE;
    mhip_roi_t q;
    mars_error_t e = mode_opts(mode, opts, align, 1, 1, &q);
    if (e != MARS_OK) return e;
    if (det_model == dst_model) return MARS_ERR_INVALID_TENSOR;
    if (!mhip_ready()) return MARS_ERR_NNA_INIT_FAILED;
    const int n = mars_hip_get_batch(det_model);
    if (n <= 0) return MARS_ERR_INVALID_TENSOR;
    const size_t in_b = q.frame_stride * (size_t)n;
    uint8_t *d = (uint8_t *)mhip_malloc(in_b);
    if (!d) return MARS_ERR_ALLOC_FAILED;
    mhip_select_stream(0);
    if (mhip_h2d_async(d, frames, in_b)) e = MARS_ERR_LAYER_FAILED;
    if (e == MARS_OK) e = crop_device(det_model, d, dst_model, input_index, opts, mode, align);
    if (mhip_sync() && e == MARS_OK) e = MARS_ERR_LAYER_FAILED;
    mhip_free(d);
    return e;
}

mars_error_t mars_hip_crop_detections_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index,
                                             const mars_hip_roi_opts_t *opts) {
    return crop_device(det_model, frames_dev, dst_model, input_index, opts, 0, NULL);
}

mars_error_t mars_hip_crop_detections(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index,
                                      const mars_hip_roi_opts_t *opts) {
    return crop_upload(det_model, frames, dst_model, input_index, opts, 0, NULL);
}

mars_error_t mars_hip_crop_obb_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index,
                                      const mars_hip_roi_opts_t *opts) {
    return crop_device(det_model, frames_dev, dst_model, input_index, opts, MODE_ROT, NULL);
}

mars_error_t mars_hip_crop_obb(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index,
                               const mars_hip_roi_opts_t *opts) {
    return crop_upload(det_model, frames, dst_model, input_index, opts, MODE_ROT, NULL);
}

mars_error_t mars_hip_crop_pose_device(mars_model_t *det_model, const void *frames_dev, mars_model_t *dst_model, int input_index,
                                       const mars_hip_roi_opts_t *opts, const mars_hip_align_opts_t *align) {
    return crop_device(det_model, frames_dev, dst_model, input_index, opts, MODE_ALIGN, align);
}

mars_error_t mars_hip_crop_pose(mars_model_t *det_model, const unsigned char *frames, mars_model_t *dst_model, int input_index,
                                const mars_hip_roi_opts_t *opts, const mars_hip_align_opts_t *align) {
    return crop_upload(det_model, frames, dst_model, input_index, opts, MODE_ALIGN, align);
}

mars_error_t mars_hip_roi_results(mars_model_t *dst_model, mars_roi_t *rois, int cap, int *n_kept, int *n_dropped) {
    if (!dst_model || cap < 0 || (cap > 0 && !rois)) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)dst_model;
    if (!m->roi_dev || m->roi_slots <= 0) return MARS_ERR_INVALID_TENSOR; /* no crop call yet */
    int n[2] = {0, 0};
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED;
    if (mhip_d2h_async(n, m->roi_dev, sizeof(n)) || mhip_sync()) return MARS_ERR_LAYER_FAILED;
    int k = n[0] < cap ? n[0] : cap;
    if (k > m->roi_slots) k = m->roi_slots;
    if (k > 0 && (mhip_d2h_async(rois, (uint8_t *)m->roi_dev + 16, (size_t)k * sizeof(mars_roi_t)) || mhip_sync())) return MARS_ERR_LAYER_FAILED;
    if (n_kept) *n_kept = n[0];
    if (n_dropped) *n_dropped = n[1];
    return MARS_OK;
}

mars_error_t mars_hip_align_results(mars_model_t *dst_model, mars_align_t *fits, int cap) {
    if (!dst_model || cap < 0 || (cap > 0 && !fits)) return MARS_ERR_INVALID_FILE;
    mars_model_ext_t *m = (mars_model_ext_t *)dst_model;
    if (!m->roi_fit_dev || m->roi_fit_slots <= 0) return MARS_ERR_INVALID_TENSOR; /* the last crop call was no aligned one */
    if (mhip_sync()) return MARS_ERR_LAYER_FAILED;
    const int k = cap < m->roi_fit_slots ? cap : m->roi_fit_slots; /* slots behind the kept ones are zeros on the device already */
    if (k > 0 && (mhip_d2h_async(fits, m->roi_fit_dev, (size_t)k * sizeof(mars_align_t)) || mhip_sync())) return MARS_ERR_LAYER_FAILED;
    return MARS_OK;
}
