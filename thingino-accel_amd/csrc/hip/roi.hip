// roi.hip -- ROI crops on gfx950: detected boxes -> source rectangles -> bilinear crops written straight into a second model's input.
//
// include/mars_hip.h ("ROI crops") states the arithmetic; everything that touches a pixel is integer, so the bytes are defined exactly.  The
// reference has no such step (its demo stops at the boxes, src/mars/mars_yolo_test.c:132-214); the frames, the detections and the second
// model's input all live in HBM here, and these kernels are the link between them:
//   roi_select_kernel<0 / 1>  the selection rules over the detection lists a tail left in HBM: per-frame kept counts by wave ballots in list
//                             order, slot offsets by a sum over the frames in front, the ROI table and the kept / dropped counters;
//   roi_rects_kernel          the rectangle rule alone over a caller's boxes (mars_yolo_crop_boxes), box i -> slot i;
//   roi_crop_kernel<FMT>      the bilinear crop.  The geometry differs per box and only the device knows it: the kernel reads the kept count
//                             and its rectangle from device memory, builds the column table in LDS, stages the source-row segments its
//                             rows touch in LDS (NV12: converted once per pixel while staging) and blends from LDS;
//   roi_area_crop_kernel      the crop under MARS_ROI_AREA / MARS_TILE_AREA: down-scaled axes are box-filtered; a strip streams over its source rows;
//   roi_rot_crop_kernel<FMT>  the crop of an ORIENTED box ("Rotated crops"): samples along the box's axes from a staged bounding rectangle;
//                             the select and rectangle kernels serve it through their SRC_ROT list source.  With FIT the six integers of
//                             its sample frame come from a table instead ("Aligned crops"): align_fit, a least-squares similarity of a
//                             template onto pose keypoints, run by the select and rectangle kernels over their SRC_POSE list source.
// What the three crop kernels share is written once:
//   strip_t      a workgroup owns R output rows of one destination slot.  The strip says where they lie in the destination, fills them grey
//                when there is nothing to sample, keeps their bytes together in an LDS image and stores that image as contiguous runs,
//                16 bytes at a time;
//   slot_geom    an upright slot's rectangle -> live, the resized size (keep_aspect_size, the rotated geometry's rule too) and its place;
//   stage_unit   one unit of a staged source row of the two upright kernels; blend4, the four-tap blend of the two samplers;
//   align_fit    csrc/align_fit.h, the text the host's mars_yolo_align_fit compiles too, with the enclosing rectangle of a rotated box.
// Nothing here uses atomics: a slot number is a function of the lists alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../align_fit.h"
#include "../mhip.h"
#include "nv12.hpp"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

// (roi_rect, the box -> source rectangle rule, lives in tail_core.hpp: redact.hip forms its regions by it too)

// the resized size of a cw x ch source inside a tw x th target under MARS_ROI_KEEP_ASPECT: the longer side fills its axis, the other is rounded, >= 1
__device__ __forceinline__ void keep_aspect_size(const int cw, const int ch, const int tw, const int th, int &nw, int &nh) {
    if ((long long)cw * th >= (long long)ch * tw) nh = max(1, (int)(((long long)ch * tw + cw / 2) / cw));
    else nw = max(1, (int)(((long long)cw * th + ch / 2) / ch));
}

// ---- "Rotated crops": the skip rule, the enclosing rectangle of the ROI table and the Q16 sample frame of an oriented box.  float32, every
// operation rounded on its own; rintf is round-to-nearest-even on both sides; `/` is the correctly rounded division (hipcc's default)

// false = skipped; we, he = the expanded sides.  Behind this rule every conversion below is defined: we, he <= 32768, the centre inside the frame
__device__ __forceinline__ bool rot_sides(const obb_t d, const float expand, const int min_size, const int W, const int H, float &we, float &he) {
    we = he = 0.0f;
    if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.w) && isfinite(d.h) && isfinite(d.conf) && isfinite(d.angle))) return false;
    if (!(d.w > 0.0f) || !(d.h > 0.0f)) return false;
    we = __fmul_rn(d.w, expand);
    he = __fmul_rn(d.h, expand);
    if (we < (float)min_size || he < (float)min_size || we > 32768.0f || he > 32768.0f) return false;
    return !(d.x < 0.0f || d.x > (float)W || d.y < 0.0f || d.y > (float)H);
}

// the rule and, for a kept box, the integer rectangle around the expanded box, clipped to the frame (the ROI table's x0 .. y1: never read back here)
__device__ __forceinline__ bool rot_rect(const obb_t d, const float cs, const float sn, const float expand, const int min_size, const int W, const int H,
                                         int q[4]) {
    q[0] = q[1] = q[2] = q[3] = 0;
    float we, he;
    if (!rot_sides(d, expand, min_size, W, H, we, he)) return false;
    rot_enclose(d.x, d.y, we, he, fabsf(cs), fabsf(sn), W, H, q);
    return true;
}

struct rot_geom_t { int X0, Y0, Ux, Uy, Vx, Vy, nw, nh, px, py; };
__device__ __forceinline__ rot_geom_t rot_geom(const obb_t d, const float we, const float he, const float cs, const float sn, const int tw, const int th,
                                               const int keep_aspect) {
    rot_geom_t g;
    g.nw = tw; g.nh = th;
    if (keep_aspect) keep_aspect_size(max(1, (int)rintf(we)), max(1, (int)rintf(he)), tw, th, g.nw, g.nh);
    g.px = (tw - g.nw) / 2; g.py = (th - g.nh) / 2;
    const float sx = __fdiv_rn(we, (float)(2 * g.nw)), sy = __fdiv_rn(he, (float)(2 * g.nh));
    g.Ux = rot_q16(__fmul_rn(sx, cs)); g.Uy = rot_q16(__fmul_rn(sx, sn));
    g.Vx = rot_q16(-__fmul_rn(sy, sn)); g.Vy = rot_q16(__fmul_rn(sy, cs));
    g.X0 = rot_q16(__fsub_rn(d.x, 0.5f)); g.Y0 = rot_q16(__fsub_rn(d.y, 0.5f));
    return g;
}

// conf >= min_conf and the class window: what the three list sources of the selection ask of a detection before their own rule
__device__ __forceinline__ bool roi_wanted(const mhip_roi_t &p, const float conf, const int cls) {
    return conf >= p.min_conf && (p.cls_count == 0 || ((long long)cls >= p.cls_first && (long long)cls < (long long)p.cls_first + p.cls_count));
}

// One wave per frame.  PHASE 0 counts the frame's kept boxes into frame_kept[f]; PHASE 1 (a second launch: it needs every frame's count) sums
// the counts of the frames in front into the frame's first slot, walks the list again the same way and writes the table.  A box's rank inside
// its frame = kept boxes in front of it in the list: the ballot of the 64 boxes in flight, masked below the lane, plus the chunks before.
// SRC_ROT: the lists are oriented boxes (32-byte records and their (cos, sin) pairs) under the skip rule of "Rotated crops".
// SRC_POSE: the lists are the frame's pose slots up to the first one with det == -1; a slot's detection passes min_conf and the class window,
// its keypoints the fit of "Aligned crops", whose record goes beside the ROI entry (PHASE 0 clears the fit table first).
#define SRC_BOX 0
#define SRC_ROT 1
#define SRC_POSE 2
template <int PHASE, int SRC>
__global__ __launch_bounds__(64) void roi_select_kernel(const mhip_roi_t p) {
    const int f = blockIdx.x, lane = threadIdx.x;
    int base = 0;
    if (PHASE == 1) {
        int before = 0, all = 0;
        for (int i = lane; i < p.n_frames; i += 64) {
            const int k = p.frame_kept[i];
            all += k;
            if (i < f) before += k;
        }
        for (int s = 32; s > 0; s >>= 1) {
            before += __shfl_xor(before, s, 64);
            all += __shfl_xor(all, s, 64);
        }
        base = before;
        if (f == 0 && lane == 0) {
            const int kept = min(all, p.slots);
            p.n_out[0] = kept;
            p.n_out[1] = all - kept;
        }
    }
    const int n_det = min(max(p.counts[f], 0), p.det_cap);
    int n = SRC == SRC_POSE ? p.pose_max : n_det;
    const det_t *dets = (const det_t *)p.dets + (size_t)f * p.det_cap;
    roi_t *rois = (roi_t *)p.rois;
    if (SRC == SRC_POSE && PHASE == 0) { // every slot of the fit table is zero before PHASE 1 (a later launch) writes the kept ones
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (int i = f * 64 + lane; i < 2 * p.slots; i += 64 * (int)gridDim.x) ((uint4 *)p.fits)[i] = z;
    }
    int kept = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        bool ok = false;
        int q[4] = {0, 0, 0, 0};
        int det_i = i;
        align_t fit;
        if (SRC == SRC_POSE) {
            const size_t k = (size_t)f * p.pose_max + min(i, n - 1);
            const int di = ((const pose_t *)p.pose_recs)[k].det;
            const unsigned long long ends = __ballot(i < n && di < 0); // the first such slot ends the list
            if (ends) n = i0 + __ffsll((long long)ends) - 1;
            if (i < n && di < n_det) { // (a det beyond the frame's list cannot come from the pose stage: not taken)
                const det_t d = dets[di];
                ok = roi_wanted(p, d.conf, d.cls) && align_fit((const align_kpt_t *)p.pose_kpts + k * p.num_kpt, &p, &fit, q);
                det_i = di;
            }
        } else if (i < n && SRC == SRC_ROT) {
            const size_t k = (size_t)f * p.det_cap + i;
            const obb_t d = ((const obb_t *)p.dets)[k];
            ok = roi_wanted(p, d.conf, d.cls) && rot_rect(d, p.csn[2 * k], p.csn[2 * k + 1], p.expand, p.min_size, p.w, p.h, q);
        } else if (i < n) {
            const det_t d = dets[i];
            ok = roi_wanted(p, d.conf, d.cls) && roi_rect(d, p.expand, p.min_size, p.w, p.h, q);
        }
        const unsigned long long mask = __ballot(ok);
        const int rank = kept + __popcll(mask & ((1ull << lane) - 1ull));
        if (p.max_per_frame > 0 && rank >= p.max_per_frame) ok = false;
        if (PHASE == 1 && ok && base + rank < p.slots) {
            roi_t r;
            r.frame = f; r.det = SRC == SRC_POSE ? det_i : i; r.x0 = q[0]; r.y0 = q[1]; r.x1 = q[2]; r.y1 = q[3];
            rois[base + rank] = r;
            if (SRC == SRC_POSE) ((align_t *)p.fits)[base + rank] = fit;
        }
        kept += __popcll(mask);
        if (p.max_per_frame > 0 && kept >= p.max_per_frame) {
            kept = p.max_per_frame;
            break;
        }
    }
    if (PHASE == 0 && lane == 0) p.frame_kept[f] = kept;
}

template <int SRC>
__global__ __launch_bounds__(256) void roi_rects_kernel(const mhip_roi_t p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        p.n_out[0] = min(p.n_boxes, p.slots);
        p.n_out[1] = 0;
    }
    if (i >= p.n_boxes || i >= p.slots) return;
    roi_t r;
    r.frame = p.frame_of_box[i];
    r.det = -1;
    const bool ok = r.frame >= 0 && r.frame < p.n_frames;
    int q[4] = {0, 0, 0, 0};
    if (SRC == SRC_POSE) { // box i = the K keypoints at i * K; its fit record beside the ROI entry (zeros: skipped)
        align_t fit = {0, 0, 0, 0, 0, 0, 0u, 0};
        if (ok) align_fit((const align_kpt_t *)p.boxes + (size_t)i * p.num_kpt, &p, &fit, q);
        ((align_t *)p.fits)[i] = fit;
    } else if (SRC == SRC_ROT) {
        const obb_t d = ((const obb_t *)p.boxes)[i];
        if (ok) rot_rect(d, p.csn[2 * i], p.csn[2 * i + 1], p.expand, p.min_size, p.w, p.h, q);
    } else {
        const det_t d = ((const det_t *)p.boxes)[i];
        if (ok) roi_rect(d, p.expand, p.min_size, p.w, p.h, q);
    }
    r.x0 = q[0]; r.y0 = q[1]; r.x1 = q[2]; r.y1 = q[3];
    ((roi_t *)p.rois)[i] = r;
}

#define ROI_R 8 // output rows of a strip

// n bytes of -17 at o, any alignment: bytes up to the first 16-byte boundary, 16-byte stores, bytes behind the last one (fewer than 16 at
// either end: a thread each)
__device__ __forceinline__ void roi_fill_run(int8_t *o, const int n, const int tid) {
    const int head = min(n, (int)((16u - (unsigned)((uintptr_t)o & 15)) & 15u)), body = (n - head) & ~15;
    const unsigned g = 0xefefefefu; // (int8) -17
    if (tid < head) o[tid] = (int8_t)-17;
    for (int i = tid * 16; i < body; i += 256 * 16) *(uint4 *)(o + head + i) = make_uint4(g, g, g, g);
    if (head + body + tid < n) o[head + body + tid] = (int8_t)-17;
}
// n bytes from LDS to o; l and o are congruent mod 16, so the 16-byte runs are aligned on both sides
__device__ __forceinline__ void roi_store_run(int8_t *o, const int8_t *l, const int n, const int tid) {
    const int head = min(n, (int)((16u - (unsigned)((uintptr_t)o & 15)) & 15u)), body = (n - head) & ~15;
    if (tid < head) o[tid] = l[tid];
    for (int i = tid * 16; i < body; i += 256 * 16) *(uint4 *)(o + head + i) = *(const uint4 *)(l + head + i);
    if (head + body + tid < n) o[head + body + tid] = l[head + body + tid];
}

// ---- the strip: the R output rows of one destination slot that a workgroup owns.  In the destination it is one contiguous run of bytes
// (planar: one run per channel, `plane` bytes apart).  Its bytes are put together in LDS and stored in the end: the image of a run starts
// at the same offset inside a 16-byte line as the run does in memory (planar: each channel in a region of its own, a multiple of 16 bytes)
struct strip_t {
    int8_t *run;        // row ys of the slot in the destination (planar: of channel 0)
    int ys, rows;       // the strip's first row in the target and its rows (the last strip may be short)
    int r_lo, r_hi;     // its rows inside the resized crop (strip_cover)
    int n_run;          // runs of rows * pitch bytes: nhwc 1, planar 3
    int pitch, step;    // bytes from row to row and from column to column of one channel: nhwc tw * 3 and 3, planar tw and 1
    unsigned plane, lo; // bytes from run to run (nhwc: 0); the offset of `run` inside a 16-byte line
    int8_t *img;        // the LDS image (strip_image); channel c of a pixel lies strip_base(c) + strip_pix(row, column) into it
    int cs;             // bytes from channel to channel in the image: nhwc 1, planar a channel region
};
__device__ __forceinline__ strip_t strip_open(const mhip_roi_t &p, const int slot, const int ys, const int R) {
    strip_t s;
    s.ys = ys; s.rows = min(R, p.th - ys);
    s.r_lo = s.r_hi = 0;
    s.n_run = p.nhwc ? 1 : 3;
    s.pitch = p.nhwc ? p.tw * 3 : p.tw; s.step = p.nhwc ? 3 : 1;
    s.plane = p.nhwc ? 0u : (unsigned)p.th * (unsigned)p.tw;
    s.run = p.out + (size_t)slot * p.out_stride + (size_t)ys * s.pitch;
    s.lo = (unsigned)((uintptr_t)s.run & 15);
    s.img = nullptr; s.cs = 1;
    return s;
}
// the strip's rows inside a resized crop of nh rows that starts at row py of the target; false: none of them (a pad band)
__device__ __forceinline__ bool strip_cover(strip_t &s, const int py, const int nh) {
    s.r_lo = max(py - s.ys, 0); s.r_hi = min(py + nh - s.ys, s.rows);
    return s.r_hi > s.r_lo;
}
// an empty slot, a skipped box or a pad band: grey, the source is not touched
__device__ __forceinline__ void strip_grey(const strip_t &s, const int tid) {
    for (int c = 0; c < s.n_run; c++) roi_fill_run(s.run + (size_t)c * s.plane, s.rows * s.pitch, tid);
}
// the image in `stage` (3 channel regions of an R-row strip: roi_lds_stage), grey first: the bands left / right of the crop and the rows outside it stay so
__device__ __forceinline__ void strip_image(strip_t &s, int8_t *stage, const int R, const int tw, const int tid) {
    const int chan = ((R * tw + 15) & ~15) + 16; // bytes per channel region: a multiple of 16, so every region starts on a 16-byte line
    s.img = stage; s.cs = s.n_run == 1 ? 1 : chan;
    for (int i = tid * 4; i < 3 * chan; i += 1024) *(unsigned *)(stage + i) = 0xefefefefu;
}
// uniform: with c a constant of an unrolled loop it is scalar work outside the pixel loop
__device__ __forceinline__ int strip_base(const strip_t &s, const int c) { return c * s.cs + (int)((s.lo + (unsigned)c * s.plane) & 15u); }
__device__ __forceinline__ int strip_pix(const strip_t &s, const int row, const int col) { return row * s.pitch + col * s.step; }
__device__ __forceinline__ void strip_put(const strip_t &s, const int pix, const int c, const int8_t v) { s.img[strip_base(s, c) + pix] = v; }
// after a barrier behind the last strip_put
__device__ __forceinline__ void strip_store(const strip_t &s, const int tid) {
    for (int c = 0; c < s.n_run; c++) roi_store_run(s.run + (size_t)c * s.plane, s.img + strip_base(s, c), s.rows * s.pitch, tid);
}

// ---- an upright slot, from device memory: the kept count and the slot's rectangle -> whether there is anything to sample, the source
// rectangle, the resized size inside the target and where it starts
struct slot_geom_t {
    bool live;
    int frame, x0, y0, cw, ch, nw, nh, px, py;
};
__device__ __forceinline__ slot_geom_t slot_geom(const mhip_roi_t &p, const int slot) {
    slot_geom_t g;
    bool live = slot < p.n_out[0];
    roi_t r = {0, 0, 0, 0, 0, 0};
    if (live) r = ((const roi_t *)p.rois)[slot];
    g.frame = r.frame; g.x0 = r.x0; g.y0 = r.y0; g.cw = r.x1 - r.x0; g.ch = r.y1 - r.y0;
    g.live = live && g.cw > 0 && g.ch > 0 && r.frame >= 0 && r.frame < p.n_frames && r.x0 >= 0 && r.y0 >= 0 && r.x1 <= p.w && r.y1 <= p.h;
    g.nw = p.tw; g.nh = p.th;
    if (g.live && p.keep_aspect) keep_aspect_size(g.cw, g.ch, p.tw, p.th, g.nw, g.nh);
    g.px = (p.tw - g.nw) / 2; g.py = (p.th - g.nh) / 2;
    return g;
}

// the four taps of one channel, fx and fy in 1/256 -> the int8 the crops write
__device__ __forceinline__ int8_t blend4(const int t00, const int t01, const int t10, const int t11, const int fx, const int fy) {
    const int top = t00 * (256 - fx) + t01 * fx, bot = t10 * (256 - fx) + t11 * fx;
    return (int8_t)(((top * (256 - fy) + bot * fy + 32768) >> 16) - 128);
}

// position of output sample i of n_out over n_in source samples, half-pixel centres, 8 fractional bits, clamped to the source
__device__ __forceinline__ int roi_pos(const int i, const int n_in, const int n_out) {
    long long pos = ((long long)(2 * i + 1) * n_in * 256) / (2LL * n_out) - 128;
    pos = pos < 0 ? 0 : pos;
    const long long top = (long long)(n_in - 1) * 256;
    return (int)(pos > top ? top : pos);
}

static size_t roi_r16(size_t x) { return (x + 15) & ~(size_t)15; }
// LDS of the crop kernel: [column table][group record][strip bytes][source rows]
static size_t roi_lds_col(int tw) { return roi_r16((size_t)tw * 8); }
#define ROI_META 256
static size_t roi_lds_stage(int tw) { return 3 * (roi_r16((size_t)ROI_R * tw) + 16); } // per channel: a strip's rows + the offset inside a 16-byte line
static size_t roi_pitch_max(int w, int fmt) { return fmt ? roi_r16((((size_t)w + 3) & ~(size_t)3) * 3) : roi_r16((size_t)w * 3); }
static size_t roi_rowbuf(int w, int fmt) {
    const size_t pm = roi_pitch_max(w, fmt), all = 2 * ROI_R * pm;
    return all < 32 * 1024 ? all : (2 * pm > 32 * 1024 ? 2 * pm : 32 * 1024);
}

// ---- staged source rows of the two upright kernels.  A staged row holds the pixels [xe, x0 + cw) of a source row as RGB bytes (xe = x0,
// NV12: x0 & ~1), `units` units in `pitch` bytes: 16-byte pieces of the segment, NV12: quads of pixels converted from an even column
struct stage_rows_t { int xe, units, pitch; };
template <int FMT>
__device__ __forceinline__ stage_rows_t stage_rows(const slot_geom_t &g) {
    stage_rows_t sr;
    sr.xe = FMT ? (g.x0 & ~1) : g.x0;
    sr.units = FMT ? (g.x0 + g.cw - sr.xe + 3) >> 2 : (g.cw * 3 + 15) >> 4;
    sr.pitch = FMT ? (sr.units * 12 + 15) & ~15 : sr.units * 16;
    return sr;
}
// Unit u of the staged image `row` of source row sy.  RGB: 16 bytes of the segment; NV12: four pixels, 12 bytes, each stored on its own
// (packed into dwords inside a helper like this one, the bytes came out wrong: profiles/HISTORY.md, "Area-averaged crops")
template <int FMT>
__device__ __forceinline__ void stage_unit(const mhip_roi_t &p, const nv12_coef_t &kc, const uint8_t *frame, const slot_geom_t &g, const stage_rows_t &sr,
                                          const int sy, const int u, unsigned char *row) {
    if (FMT) { // Y bytes of pixels xe + 4 u .. + 3 and, at the same byte offset of chroma row sy >> 1, their two chroma pairs
        const int x = sr.xe + 4 * u;
        const uint8_t *gy = frame + (size_t)sy * p.w + x, *gc = frame + ((size_t)p.h + (size_t)(sy >> 1)) * p.w + x;
        unsigned yv, cv;
        if (x + 4 <= p.w) {
            __builtin_memcpy(&yv, gy, 4);
            __builtin_memcpy(&cv, gc, 4);
        } else { // w % 4 == 2: the row's last two pixels and their one pair; nothing is read beyond either row
            yv = (unsigned)gy[0] | (unsigned)gy[1] << 8;
            cv = (unsigned)gc[0] | (unsigned)gc[1] << 8;
        }
        int c[4][3];
        nv12_quad(kc, yv, cv, c);
        unsigned char *o = row + u * 12;
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = (unsigned char)c[k / 3][k % 3];
    } else { // 16 bytes of the segment [x0 * 3, x1 * 3) of the row; the last piece byte by byte: nothing is read beyond the segment
        const uint8_t *gp = frame + ((size_t)sy * p.w + g.x0) * 3 + (size_t)u * 16;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        const int left = g.cw * 3 - u * 16;
        if (left >= 16) __builtin_memcpy(v, gp, 16);
        else {
#pragma unroll
            for (int b = 0; b < 15; b++) // (register indices fixed by the unrolling)
                if (b < left) v[b >> 2] |= (unsigned)gp[b] << (8 * (b & 3));
        }
        *(uint4 *)(row + u * 16) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// A workgroup owns ROI_R output rows of one slot: it builds the column table, then takes its rows in groups of as many as the row buffer
// holds source rows for: stage those, blend the group's pixels from them into the strip's image
template <int FMT>
__global__ __launch_bounds__(256) void roi_crop_kernel(const mhip_roi_t p, const int off_meta, const int off_stage, const int off_rows, const int rowbuf_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int tid = threadIdx.x;
    strip_t s = strip_open(p, blockIdx.y, blockIdx.x * ROI_R, ROI_R);
    const slot_geom_t g = slot_geom(p, blockIdx.y);
    if (!g.live || !strip_cover(s, g.py, g.nh)) {
        strip_grey(s, tid);
        return;
    }
    int2 *coltab = (int2 *)sm;          // [nw] {byte offset of the left tap in a staged row, fx | (distance to the right tap) << 8}
    int *meta = (int *)(sm + off_meta); // [0] end of the group of rows, [1] staged source rows; [4 ..) their numbers; [32 ..) per strip row {slot a, slot b, fy, -}
    unsigned char *rowbuf = sm + off_rows;
    const uint8_t *frame = p.frames + (size_t)g.frame * p.frame_stride;
    const stage_rows_t sr = stage_rows<FMT>(g);
    const int cap_rows = rowbuf_bytes / sr.pitch; // >= 2: the launcher sized the buffer for the widest box
    for (int i = tid; i < g.nw; i += 256) {
        const int pos = roi_pos(i, g.cw, g.nw), i0 = pos >> 8, i1 = min(i0 + 1, g.cw - 1);
        coltab[i] = make_int2((i0 + g.x0 - sr.xe) * 3, (pos & 255) | ((i1 - i0) * 3) << 8);
    }
    strip_image(s, (int8_t *)(sm + off_stage), ROI_R, p.tw, tid);
    const nv12_coef_t kc = nv12_coef(p.nv12_flags);
    int r_cur = s.r_lo;
    while (r_cur < s.r_hi) {
        // the next group of rows: as many as the row buffer holds source rows for.  Source rows only grow along the strip, so a row that is
        // already staged is one of the last two
        if (tid == 0) {
            int n_st = 0, rr = r_cur;
            for (; rr < s.r_hi; rr++) {
                const int pos = roi_pos(s.ys + rr - g.py, g.ch, g.nh), j0 = pos >> 8, j1 = min(j0 + 1, g.ch - 1);
                int a = -1, b = -1;
                for (int k = max(n_st - 2, 0); k < n_st; k++) {
                    if (meta[4 + k] == j0) a = k;
                    if (meta[4 + k] == j1) b = k;
                }
                const int need = (a < 0) + (j1 != j0 && b < 0);
                if (n_st + need > cap_rows) break;
                if (a < 0) { a = n_st; meta[4 + n_st++] = j0; }
                if (j1 == j0) b = a;
                else if (b < 0) { b = n_st; meta[4 + n_st++] = j1; }
                meta[32 + 4 * rr] = a; meta[32 + 4 * rr + 1] = b; meta[32 + 4 * rr + 2] = pos & 255;
            }
            meta[0] = rr; meta[1] = n_st;
        }
        __syncthreads(); // (the first time round also: the column table and the grey strip)
        const int r_end = meta[0], n_st = meta[1];
        for (int it = tid; it < n_st * sr.units; it += 256) {
            const int st = it / sr.units, u = it - st * sr.units;
            stage_unit<FMT>(p, kc, frame, g, sr, g.y0 + meta[4 + st], u, rowbuf + st * sr.pitch);
        }
        __syncthreads();
        const int npix = (r_end - r_cur) * g.nw;
        for (int idx = tid; idx < npix; idx += 256) {
            const int rr = idx / g.nw, i = idx - rr * g.nw, row = r_cur + rr;
            const int4 rt = *(const int4 *)(meta + 32 + 4 * row);
            const unsigned char *ra = rowbuf + rt.x * sr.pitch, *rb = rowbuf + rt.y * sr.pitch;
            const int2 ct = coltab[i];
            const int o0 = ct.x, o1 = ct.x + (ct.y >> 8), fx = ct.y & 255, fy = rt.z;
            const int pix = strip_pix(s, row, g.px + i);
#pragma unroll
            for (int c = 0; c < 3; c++) strip_put(s, pix, c, blend4(ra[o0 + c], ra[o1 + c], rb[o0 + c], rb[o1 + c], fx, fy));
        }
        __syncthreads(); // the rows and the group record may be overwritten
        r_cur = r_end;
    }
    strip_store(s, tid);
}

// ---- the area-averaging crop ("Area averaging" in include/mars_hip.h): an axis with more source samples than outputs is box-filtered, the
// other one keeps the bilinear taps.  A strip of output rows covers a contiguous range of source rows, too many to hold at strong
// down-scales, so the kernel streams: it stages a window of the next source rows (as many as the row buffer holds), and for each output row
// walks that row's source rows.  Thread t owns the (column, channel) pairs q = t + 256 k: for a source row it reduces the row's x taps into
// h[q] (<= 255 Dx) once, keeps it in its own LDS entry of a two-row cache indexed by the row's parity -- consecutive output rows share their
// boundary row (averaged) or both rows (interpolated) -- and adds wy * h[q] to the accumulator of the current output row, a register.  Only
// the row window is shared between threads: two barriers per window, none per row.  Accumulators are 32 bits wide where 255.5 Dx Dy fits,
// else 64; the slot's geometry decides, so a workgroup takes one path.  The quotient is the exact unsigned division of that width.
#define AREA_MAX_TW 1280          // 15 pairs per thread
#define AREA_ACC32_MAX 16000000u  // Dx * Dy up to here: 255.5 * Dx * Dy < 2^32
static int area_rows(int tw) { return tw <= 640 ? ROI_R : ROI_R / 2; } // output rows of a strip
// LDS: [column table, 4 bytes a column][h cache: 2 rows x (tw * 3) dwords][strip bytes][source-row window]
static size_t area_lds_col(int tw) { return roi_r16((size_t)tw * 4); }
static size_t area_lds_hs(int tw) { return 2 * roi_r16((size_t)tw * 12); }
static size_t area_lds_stage(int tw) { return 3 * (roi_r16((size_t)area_rows(tw) * tw) + 16); }
static size_t area_rowbuf(int w, int tw, int fmt) { // 0: the widest source row does not fit beside the rest
    const size_t rest = area_lds_col(tw) + area_lds_hs(tw) + area_lds_stage(tw), pm = roi_pitch_max(w, fmt);
    if (rest + pm > 64 * 1024) return 0;
    const size_t want = pm > 16 * 1024 ? pm : 16 * 1024, room = 64 * 1024 - rest;
    return want < room ? want : room;
}

struct area_geom_t {
    const uint8_t *frame;
    stage_rows_t sr;
    int ax, ay; // the axis is averaged
    int cap_rows, np3, hs_pitch;
    const unsigned *coltab; // averaged x: first tap's pixel in a staged row | taps << 16; else: left tap's pixel | (distance to the right tap) << 16 | fx << 24
    unsigned *hs;
    unsigned char *rowbuf;
};

// the source rows [sa, sb] of output row o and, on an interpolated axis, fy
__device__ __forceinline__ void area_row_span(const int o, const int ch, const int nh, const int ay, int &sa, int &sb, int &fy) {
    if (ay) {
        sa = (int)(((long long)o * ch) / nh);
        sb = (int)(((long long)(o + 1) * ch + nh - 1) / nh) - 1;
        fy = 0;
    } else {
        const int pos = roi_pos(o, ch, nh);
        sa = pos >> 8; sb = min(sa + 1, ch - 1); fy = pos & 255;
    }
}

template <int FMT, int NP, typename ACC>
__device__ __forceinline__ void area_strip(const mhip_roi_t &p, const slot_geom_t &g, const area_geom_t &a, const strip_t &s, const int tid) {
    const nv12_coef_t kc = nv12_coef(p.nv12_flags);
    const ACC D = (ACC)(a.ax ? g.cw : 256) * (ACC)(a.ay ? g.ch : 256);
    int s_last, sa, sb, fy;
    area_row_span(s.ys + s.r_hi - 1 - g.py, g.ch, g.nh, a.ay, sa, s_last, fy);
    int tag0 = -1, tag1 = -1, b0 = 0, b1 = -1; // the cached rows, the staged window [b0, b1]
    for (int row = s.r_lo; row < s.r_hi; row++) {
        const int o = s.ys + row - g.py;
        area_row_span(o, g.ch, g.nh, a.ay, sa, sb, fy);
        ACC acc[NP];
#pragma unroll
        for (int k = 0; k < NP; k++) acc[k] = 0;
        for (int sy = sa; sy <= sb; sy++) {
            const int wy = a.ay ? (int)(min((long long)(sy + 1) * g.nh, (long long)(o + 1) * g.ch) - max((long long)sy * g.nh, (long long)o * g.ch))
                                : (sb == sa ? 256 : (sy == sa ? 256 - fy : fy));
            unsigned *hrow = a.hs + (sy & 1) * a.hs_pitch;
            if ((sy & 1 ? tag1 : tag0) != sy) { // (uniform: every thread walks the same rows)
                if (sy < b0 || sy > b1) {
                    __syncthreads(); // the old window is read no more (the first time round: the column table and the grey strip)
                    b0 = sy; b1 = min(sy + a.cap_rows - 1, s_last);
                    for (int it = tid; it < (b1 - b0 + 1) * a.sr.units; it += 256) {
                        const int st = it / a.sr.units, u = it - st * a.sr.units;
                        stage_unit<FMT>(p, kc, a.frame, g, a.sr, g.y0 + b0 + st, u, a.rowbuf + st * a.sr.pitch);
                    }
                    __syncthreads();
                }
                const unsigned char *rp = a.rowbuf + (sy - b0) * a.sr.pitch;
                const int xo = g.x0 - a.sr.xe;
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    const int q = tid + 256 * k;
                    if (q < a.np3) {
                        const int i = q / 3, c = q - 3 * i;
                        const unsigned ct = a.coltab[i];
                        const unsigned char *t = rp + (ct & 0xffffu) * 3 + c;
                        unsigned h;
                        if (a.ax) { // first and last tap by the overlap rule, nw for every one between
                            const int n = (int)(ct >> 16), xa = (int)(ct & 0xffffu) - xo;
                            const unsigned w0 = (unsigned)(min((xa + 1) * g.nw, (i + 1) * g.cw) - i * g.cw), w1 = (unsigned)((i + 1) * g.cw - (xa + n - 1) * g.nw);
                            unsigned mid = 0;
                            for (int x = 1; x < n - 1; x++) mid += t[3 * x];
                            h = w0 * t[0] + (unsigned)g.nw * mid + w1 * t[3 * (n - 1)];
                        } else {
                            const unsigned fx = ct >> 24;
                            h = (unsigned)t[0] * (256u - fx) + (unsigned)t[3 * ((ct >> 16) & 1u)] * fx;
                        }
                        hrow[q] = h;
                    }
                }
                if (sy & 1) tag1 = sy; else tag0 = sy;
            }
#pragma unroll
            for (int k = 0; k < NP; k++) {
                const int q = tid + 256 * k;
                if (q < a.np3) acc[k] += (ACC)(unsigned)wy * (ACC)hrow[q]; // the thread's own entries: no barrier
            }
        }
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int q = tid + 256 * k;
            if (q < a.np3) {
                const int i = q / 3, c = q - 3 * i;
                const int v = (int)((acc[k] + D / 2) / D);
                strip_put(s, strip_pix(s, row, g.px + i), c, (int8_t)(v - 128));
            }
        }
    }
}

template <int FMT, int NP>
__global__ __launch_bounds__(256) void roi_area_crop_kernel(const mhip_roi_t p, const int ar, const int off_hs, const int off_stage, const int off_rows,
                                                            const int rowbuf_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int tid = threadIdx.x;
    strip_t s = strip_open(p, blockIdx.y, blockIdx.x * ar, ar);
    const slot_geom_t g = slot_geom(p, blockIdx.y);
    if (!g.live || !strip_cover(s, g.py, g.nh)) {
        strip_grey(s, tid);
        return;
    }
    area_geom_t a;
    unsigned *coltab = (unsigned *)sm;
    a.frame = p.frames + (size_t)g.frame * p.frame_stride;
    a.sr = stage_rows<FMT>(g);
    a.ax = g.cw > g.nw; a.ay = g.ch > g.nh;
    a.cap_rows = rowbuf_bytes / a.sr.pitch; // >= 1: the launcher sized the window for the widest box
    a.np3 = g.nw * 3;
    a.hs_pitch = (p.tw * 3 + 3) & ~3;
    a.coltab = coltab; a.hs = (unsigned *)(sm + off_hs); a.rowbuf = sm + off_rows;
    const int xo = g.x0 - a.sr.xe;
    for (int i = tid; i < g.nw; i += 256) {
        if (a.ax) {
            const int xa = (int)(((long long)i * g.cw) / g.nw), xb = (int)(((long long)(i + 1) * g.cw + g.nw - 1) / g.nw) - 1;
            coltab[i] = (unsigned)(xa + xo) | (unsigned)(xb - xa + 1) << 16;
        } else {
            const int pos = roi_pos(i, g.cw, g.nw), i0 = pos >> 8, i1 = min(i0 + 1, g.cw - 1);
            coltab[i] = (unsigned)(i0 + xo) | (unsigned)(i1 - i0) << 16 | (unsigned)(pos & 255) << 24;
        }
    }
    strip_image(s, (int8_t *)(sm + off_stage), ar, p.tw, tid);
    const unsigned long long DD = (unsigned long long)(a.ax ? g.cw : 256) * (unsigned long long)(a.ay ? g.ch : 256);
    if (DD <= AREA_ACC32_MAX) area_strip<FMT, NP, unsigned>(p, g, a, s, tid);
    else area_strip<FMT, NP, unsigned long long>(p, g, a, s, tid);
    __syncthreads();
    strip_store(s, tid);
}

// ---- the rotated crop.  A workgroup owns a strip of ROI_R output rows of one slot, as above; it walks them in chunks of cn columns x rn rows.  The taps of a
// chunk lie in a parallelogram of the source; its bounding rectangle is staged in LDS as one dword per pixel (R | G << 8 | B << 16; NV12 is
// converted once per staged pixel pair, pixels outside the frame are 111 in every channel) and the blend reads its four taps from there.
// cn and rn are chosen per strip so that the rectangle fits ROT_PIX pixels: the whole strip for the boxes a second stage sees, a few columns
// at strong down-scales or near 45 degrees, and in the end one pixel (2 x 2 taps always fit).  Positions are the int64 sums of the header;
// the only floats are those of rot_sides / rot_geom, once per workgroup.
#define ROT_PIX 4096 // staged pixels: 16 KB
static size_t rot_lds(int tw) { return roi_lds_stage(tw) + (size_t)ROT_PIX * 4; }

// columns (dx = Ux, Vx) or rows (dy = Uy, Vy) of the bounding rectangle of a cn x rn chunk, at most: the positions span
// D = 2 (cn - 1) |U| + 2 (rn - 1) |V| of Q16, so their integer parts span at most (D >> 16) + 1, + 1 for the tap to the right, + 1 to count
// both ends; NV12 starts at an even column and stages pairs
__device__ __forceinline__ long long rot_extent(const int cn, const int rn, const int u, const int v, const int pad) {
    return ((2LL * (cn - 1) * abs(u) + 2LL * (rn - 1) * abs(v)) >> 16) + 3 + pad;
}

// FIT: the six integers come from the slot's entry of the fit table ("Aligned crops") instead of the obb record and its (cos, sin) pair
template <int FMT, int FIT>
__global__ __launch_bounds__(256) void roi_rot_crop_kernel(const mhip_roi_t p, const int off_buf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int tid = threadIdx.x;
    const int slot = blockIdx.y, ys = blockIdx.x * ROI_R;
    strip_t s = strip_open(p, slot, ys, ROI_R);
    // this slot's box, from device memory: entry (frame, det) of the lists, or the caller's box `slot`
    bool live = slot < p.n_out[0];
    roi_t r = {0, 0, 0, 0, 0, 0};
    if (live) r = ((const roi_t *)p.rois)[slot];
    if (FIT) live = live && r.frame >= 0 && r.frame < p.n_frames;
    else live = live && r.x1 > r.x0 && r.frame >= 0 && r.frame < p.n_frames && (r.det < 0 ? p.boxes != nullptr : (p.dets != nullptr && r.det < p.det_cap));
    rot_geom_t g = {0, 0, 0, 0, 0, 0, p.tw, p.th, 0, 0};
    if (FIT) {
        if (live) {
            const align_t a = ((const align_t *)p.fits)[slot];
            live = a.n_used > 0; // (zeros: a skipped box)
            g.X0 = a.X0; g.Y0 = a.Y0; g.Ux = a.Ux; g.Uy = a.Uy; g.Vx = a.Vx; g.Vy = a.Vy;
        }
    } else if (live) {
        const size_t k = r.det < 0 ? (size_t)slot : (size_t)r.frame * p.det_cap + r.det;
        const obb_t d = ((const obb_t *)(r.det < 0 ? p.boxes : p.dets))[k];
        const float cs = p.csn[2 * k], sn = p.csn[2 * k + 1];
        float we, he;
        live = rot_sides(d, p.expand, p.min_size, p.w, p.h, we, he);
        if (live) g = rot_geom(d, we, he, cs, sn, p.tw, p.th, p.keep_aspect);
    }
    const int nw = g.nw, nh = g.nh, px = g.px, py = g.py;
    if (!live || !strip_cover(s, py, nh)) {
        strip_grey(s, tid);
        return;
    }
    const int r_lo = s.r_lo, r_hi = s.r_hi;
    unsigned *buf = (unsigned *)(sm + off_buf);
    const uint8_t *frame = p.frames + (size_t)r.frame * p.frame_stride;
    strip_image(s, (int8_t *)sm, ROI_R, p.tw, tid);
    // the chunk: columns first, then rows, halved until the bounding rectangle fits
    const int pad = FMT ? 2 : 0;
    int cn = nw, rn = r_hi - r_lo;
    while (cn > 1 && rot_extent(cn, rn, g.Ux, g.Vx, pad) * rot_extent(cn, rn, g.Uy, g.Vy, 0) > ROT_PIX) cn = (cn + 1) >> 1;
    while (rn > 1 && rot_extent(cn, rn, g.Ux, g.Vx, pad) * rot_extent(cn, rn, g.Uy, g.Vy, 0) > ROT_PIX) rn = (rn + 1) >> 1;
    const nv12_coef_t kc = nv12_coef(p.nv12_flags);
    const long long X0 = g.X0, Y0 = g.Y0;
    for (int ra = r_lo; ra < r_hi; ra += rn) {
        const int rb = min(ra + rn, r_hi);
        const long long b0 = 2 * (ys + ra - py) + 1 - nh, b1 = 2 * (ys + rb - 1 - py) + 1 - nh;
        for (int c0 = 0; c0 < nw; c0 += cn) {
            const int c1 = min(c0 + cn, nw);
            const long long a0 = 2 * c0 + 1 - nw, a1 = 2 * (c1 - 1) + 1 - nw;
            // the positions are affine in (a, b): their extremes are at the chunk's corners
            const long long xa = min(a0 * g.Ux, a1 * g.Ux), xb = max(a0 * g.Ux, a1 * g.Ux), xc = min(b0 * g.Vx, b1 * g.Vx), xd = max(b0 * g.Vx, b1 * g.Vx);
            const long long ya = min(a0 * g.Uy, a1 * g.Uy), yb = max(a0 * g.Uy, a1 * g.Uy), yc = min(b0 * g.Vy, b1 * g.Vy), yd = max(b0 * g.Vy, b1 * g.Vy);
            int bx0 = (int)((X0 + xa + xc) >> 16);
            const int bx1 = (int)((X0 + xb + xd) >> 16) + 1, by0 = (int)((Y0 + ya + yc) >> 16), by1 = (int)((Y0 + yb + yd) >> 16) + 1;
            if (FMT) bx0 &= ~1;
            const int bw = FMT ? (bx1 - bx0 + 2) & ~1 : bx1 - bx0 + 1, bh = by1 - by0 + 1; // bw * bh <= ROT_PIX by the choice of cn, rn
            if (FMT) { // pairs of pixels from an even column: two Y bytes and their chroma pair; the frame's sizes are even, so a pair is inside or outside as a whole
                const int hw = bw >> 1;
                for (int it = tid; it < hw * bh; it += 256) {
                    const int s = it / hw, u = it - s * hw, sx = bx0 + 2 * u, sy = by0 + s;
                    unsigned v0 = 0x6f6f6fu, v1 = 0x6f6f6fu;
                    if (sx >= 0 && sx < p.w && sy >= 0 && sy < p.h) {
                        const uint8_t *gy = frame + (size_t)sy * p.w + sx, *gc = frame + ((size_t)p.h + (size_t)(sy >> 1)) * p.w + sx;
                        const unsigned yv = (unsigned)gy[0] | (unsigned)gy[1] << 8, cv = (unsigned)gc[0] | (unsigned)gc[1] << 8;
                        int c[4][3];
                        nv12_quad(kc, yv, cv, c);
                        v0 = (unsigned)c[0][0] | (unsigned)c[0][1] << 8 | (unsigned)c[0][2] << 16;
                        v1 = (unsigned)c[1][0] | (unsigned)c[1][1] << 8 | (unsigned)c[1][2] << 16;
                    }
                    buf[s * bw + 2 * u] = v0;
                    buf[s * bw + 2 * u + 1] = v1;
                }
            } else {
                for (int it = tid; it < bw * bh; it += 256) {
                    const int s = it / bw, u = it - s * bw, sx = bx0 + u, sy = by0 + s;
                    unsigned v = 0x6f6f6fu;
                    if (sx >= 0 && sx < p.w && sy >= 0 && sy < p.h) {
                        const uint8_t *gp = frame + ((size_t)sy * p.w + sx) * 3;
                        v = (unsigned)gp[0] | (unsigned)gp[1] << 8 | (unsigned)gp[2] << 16;
                    }
                    buf[s * bw + u] = v;
                }
            }
            __syncthreads(); // (the first time round also: the grey strip)
            const int wc = c1 - c0;
            for (int idx = tid; idx < (rb - ra) * wc; idx += 256) {
                const int rr = idx / wc, i = c0 + idx - rr * wc, row = ra + rr;
                const long long a = 2 * i + 1 - nw, b = 2 * (ys + row - py) + 1 - nh;
                const long long PX = X0 + a * g.Ux + b * g.Vx, PY = Y0 + a * g.Uy + b * g.Vy;
                const int qx = (int)(PX >> 8), qy = (int)(PY >> 8);
                const int fx = qx & 255, fy = qy & 255;
                const unsigned *t = buf + ((qy >> 8) - by0) * bw + ((qx >> 8) - bx0);
                const unsigned t00 = t[0], t01 = t[1], t10 = t[bw], t11 = t[bw + 1];
                const int pix = strip_pix(s, row, px + i);
#pragma unroll
                for (int c = 0; c < 3; c++)
                    strip_put(s, pix, c, blend4((t00 >> (8 * c)) & 255u, (t01 >> (8 * c)) & 255u, (t10 >> (8 * c)) & 255u, (t11 >> (8 * c)) & 255u, fx, fy));
            }
            __syncthreads(); // the staged rectangle may be overwritten
        }
    }
    strip_store(s, tid);
}

static bool roi_common_ok(const mhip_roi_t *p) {
    return p && p->rois && p->n_out && p->n_frames > 0 && p->slots > 0 && p->expand > 0 && p->min_size >= 1 &&
           mhip_frame_format_ok(p->fmt, p->nv12_flags) && mhip_frame_bytes(p->w, p->h, p->fmt);
}

// what the align calls need on top: the fit table (16-byte aligned: it is cleared 16 bytes at a time), a template size and a mask inside it, a target
static bool roi_align_ok(const mhip_roi_t *p) {
    return p->fits && !((uintptr_t)p->fits & 15) && p->num_kpt >= 1 && p->num_kpt <= MHIP_POSE_MAX_KPT && p->use != 0 &&
           (p->num_kpt == 32 || !(p->use >> p->num_kpt)) && p->tw > 0 && p->th > 0 && !p->csn;
}

// f(the list source as a compile-time constant) for a run-time src: the one place the three sources are spelled out, with their names in the checks
template <typename F>
static void with_src(const int src, F f) {
    if (src == SRC_POSE) f(std::integral_constant<int, SRC_POSE>());
    else if (src == SRC_ROT) f(std::integral_constant<int, SRC_ROT>());
    else f(std::integral_constant<int, SRC_BOX>());
}
static const char *const ROI_SELECT_NAME[3] = {"roi select", "roi select (oriented)", "roi select (aligned)"};
static const char *const ROI_RECTS_NAME[3] = {"roi rects", "roi rects (oriented)", "roi rects (aligned)"};

static int roi_select(const mhip_roi_t *p, const int src) {
    if (!roi_common_ok(p) || !p->dets || !p->counts || !p->frame_kept || p->det_cap <= 0 || p->cls_count < 0 || p->max_per_frame < 0 ||
        (src == SRC_ROT) != (p->csn != nullptr))
        return -1;
    if (src == SRC_POSE && (!roi_align_ok(p) || !p->pose_recs || !p->pose_kpts || p->pose_max <= 0)) return -1;
    const dim3 g((unsigned)p->n_frames);
    with_src(src, [&](auto S) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(roi_select_kernel<0, decltype(S)::value>), g, dim3(64), 0, mhip_stream_native(), *p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(roi_select_kernel<1, decltype(S)::value>), g, dim3(64), 0, mhip_stream_native(), *p);
    });
    return mhip_check(hipGetLastError(), ROI_SELECT_NAME[src]);
}
extern "C" int mhip_roi_select(const mhip_roi_t *p) { return roi_select(p, SRC_BOX); }
extern "C" int mhip_roi_rot_select(const mhip_roi_t *p) { return roi_select(p, SRC_ROT); }
extern "C" int mhip_roi_align_select(const mhip_roi_t *p) { return roi_select(p, SRC_POSE); }

static int roi_rects(const mhip_roi_t *p, const int src) {
    if (!roi_common_ok(p) || !p->boxes || !p->frame_of_box || p->n_boxes <= 0 || p->n_boxes > p->slots || (src == SRC_ROT) != (p->csn != nullptr)) return -1;
    if (src == SRC_POSE && !roi_align_ok(p)) return -1;
    const dim3 g((unsigned)((p->n_boxes + 255) / 256));
    with_src(src, [&](auto S) { hipLaunchKernelGGL(roi_rects_kernel<decltype(S)::value>, g, dim3(256), 0, mhip_stream_native(), *p); });
    return mhip_check(hipGetLastError(), ROI_RECTS_NAME[src]);
}
extern "C" int mhip_roi_rects(const mhip_roi_t *p) { return roi_rects(p, SRC_BOX); }
extern "C" int mhip_roi_rot_rects(const mhip_roi_t *p) { return roi_rects(p, SRC_ROT); }
extern "C" int mhip_roi_align_rects(const mhip_roi_t *p) { return roi_rects(p, SRC_POSE); }

extern "C" int mhip_roi_fits(int w, int tw, int fmt) {
    if (w <= 0 || tw <= 0) return 0;
    return roi_lds_col(tw) + ROI_META + roi_lds_stage(tw) + roi_rowbuf(w, fmt) <= 64 * 1024;
}

extern "C" int mhip_roi_area_fits(int w, int tw, int fmt) {
    if (w <= 0 || tw <= 0) return 0;
    return tw <= AREA_MAX_TW && w <= 65535 && area_rowbuf(w, tw, fmt) != 0;
}

template <int FMT>
static void roi_area_launch(const mhip_roi_t *p) {
    const int ar = area_rows(p->tw), off_hs = (int)area_lds_col(p->tw), off_stage = off_hs + (int)area_lds_hs(p->tw);
    const int off_rows = off_stage + (int)area_lds_stage(p->tw), rowbuf = (int)area_rowbuf(p->w, p->tw, p->fmt);
    const dim3 g((unsigned)((p->th + ar - 1) / ar), (unsigned)p->slots);
    const size_t lds = (size_t)off_rows + rowbuf;
    // pairs per thread: tw * 3 <= 256 NP
    if (p->tw * 3 <= 512) hipLaunchKernelGGL(HIP_KERNEL_NAME(roi_area_crop_kernel<FMT, 2>), g, dim3(256), lds, mhip_stream_native(), *p, ar, off_hs, off_stage, off_rows, rowbuf);
    else if (p->tw * 3 <= 2048) hipLaunchKernelGGL(HIP_KERNEL_NAME(roi_area_crop_kernel<FMT, 8>), g, dim3(256), lds, mhip_stream_native(), *p, ar, off_hs, off_stage, off_rows, rowbuf);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(roi_area_crop_kernel<FMT, 15>), g, dim3(256), lds, mhip_stream_native(), *p, ar, off_hs, off_stage, off_rows, rowbuf);
}

extern "C" int mhip_roi_crop(const mhip_roi_t *p) {
    if (!roi_common_ok(p) || !p->frames || !p->out || p->tw <= 0 || p->th <= 0 || p->slots > 65535 || p->out_stride < (size_t)p->tw * p->th * 3 ||
        !mhip_roi_fits(p->w, p->tw, p->fmt))
        return -1;
    if (p->area) {
        if (!mhip_roi_area_fits(p->w, p->tw, p->fmt)) return -1;
        if (p->fmt) roi_area_launch<1>(p);
        else roi_area_launch<0>(p);
        return mhip_check(hipGetLastError(), p->fmt ? "roi area crop (nv12)" : "roi area crop");
    }
    const int off_meta = (int)roi_lds_col(p->tw), off_stage = off_meta + ROI_META, off_rows = off_stage + (int)roi_lds_stage(p->tw);
    const int rowbuf = (int)roi_rowbuf(p->w, p->fmt);
    const dim3 g((unsigned)((p->th + ROI_R - 1) / ROI_R), (unsigned)p->slots);
    if (p->fmt) hipLaunchKernelGGL(roi_crop_kernel<1>, g, dim3(256), (size_t)off_rows + rowbuf, mhip_stream_native(), *p, off_meta, off_stage, off_rows, rowbuf);
    else hipLaunchKernelGGL(roi_crop_kernel<0>, g, dim3(256), (size_t)off_rows + rowbuf, mhip_stream_native(), *p, off_meta, off_stage, off_rows, rowbuf);
    return mhip_check(hipGetLastError(), p->fmt ? "roi crop (nv12)" : "roi crop");
}

extern "C" int mhip_roi_rot_fits(int w, int h, int tw) {
    if (w <= 0 || h <= 0 || tw <= 0) return 0;
    return w <= 32767 && h <= 32767 && rot_lds(tw) <= 64 * 1024; // (x - 0.5) * 65536 of a centre inside the frame fits an int
}

// the rotated sampler over the obb records (fit 0) or the fit table (fit 1), behind the checks both forms share
static int rot_crop(const mhip_roi_t *p, const int fit) {
    if (!p->frames || !p->out || p->tw <= 0 || p->th <= 0 || p->slots > 65535 || p->out_stride < (size_t)p->tw * p->th * 3 ||
        !mhip_roi_rot_fits(p->w, p->h, p->tw))
        return -1;
    static const char *const name[2][2] = {{"rotated roi crop", "rotated roi crop (nv12)"}, {"aligned roi crop", "aligned roi crop (nv12)"}};
    const auto k = fit ? (p->fmt ? roi_rot_crop_kernel<1, 1> : roi_rot_crop_kernel<0, 1>) : (p->fmt ? roi_rot_crop_kernel<1, 0> : roi_rot_crop_kernel<0, 0>);
    const dim3 g((unsigned)((p->th + ROI_R - 1) / ROI_R), (unsigned)p->slots);
    hipLaunchKernelGGL(k, g, dim3(256), rot_lds(p->tw), mhip_stream_native(), *p, (int)roi_lds_stage(p->tw));
    return mhip_check(hipGetLastError(), name[fit][p->fmt]);
}

extern "C" int mhip_roi_rot_crop(const mhip_roi_t *p) {
    if (!roi_common_ok(p) || !p->csn || (!p->dets && !p->boxes) || (p->dets && p->det_cap <= 0) || (p->boxes && p->n_boxes < p->slots)) return -1;
    return rot_crop(p, 0);
}

extern "C" int mhip_roi_align_crop(const mhip_roi_t *p) {
    if (!roi_common_ok(p) || !roi_align_ok(p)) return -1;
    return rot_crop(p, 1);
}
