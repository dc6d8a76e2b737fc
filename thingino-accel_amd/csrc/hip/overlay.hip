// overlay.hip -- the overlay on gfx950: the detections, track ids, frame-pixel masks and keypoints a batch left in HBM -> the camera frames
// with boxes, labels, mask tints and keypoint markers painted in, before a frame is encoded, stored or streamed.  include/mars_hip.h
// ("Overlay") states the rule; everything that touches a pixel is integer arithmetic, so the bytes are defined exactly.  The reference
// draws on the host only, with PIL in a test script (mgk-decompiler/test_yolo_inference.py, draw_detections).
//   overlay_select_kernel  one workgroup per frame: the selection (confidence, class window, tracked only, or every box of a caller's
//                          list), the rectangle rule of "ROI crops" (roi_rect of tail_core.hpp, min_size 1), the colour of the key, the
//                          label's bytes (mhip_overlay_text of csrc/overlay_rule.h: the host composes with the same code), the mask slot
//                          and the keypoint row of a detection that has one.  The kept detections go in list order (block_rank of
//                          tail_core.hpp) into the frame's element table; their markers go, in no order, into the frame's marker table,
//                          each with the key (element, keypoint) that orders it;
//   overlay_kernel         one workgroup of 256 threads per 64 x 64 pixel tile and frame.  Thread t owns 16 pixels of row t >> 2.  The
//                          workgroup scans the frame's two tables against its tile; every thread folds the hits into two minima per
//                          pixel of its own, in registers: the opaque owner (layer priority, element index[, keypoint]) and the tint
//                          owner (element index).  A minimum does not depend on the order of the hits, and no pixel has two writers, so
//                          there is nothing to synchronise but the hit list.  Then the tile's rows are staged in LDS, every thread paints
//                          its own pixels there, and rows are stored back.  NV12: the luma tile, then its 32 x 32 chroma samples, each
//                          following the pixel (2i, 2j).
// Why the in-place form has no race: as in redact.hip -- tiles are disjoint, a workgroup has read every byte of its tile into LDS (a barrier
// behind the loads) before it stores the first one, and no store reaches over a tile row's ends.  So the result is a function of the
// original frame alone, in place as out of place.  A workgroup whose tile meets no element leaves at once and, in place, touches no byte.
// The row moves are tile_rows_to_lds / tile_rows_from_lds of frame_tile.hpp, shared with redact.hip.  All stores are plain vector stores
// from C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "../overlay_rule.h"
#include "frame_tile.hpp"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

struct trk_t { int id, hits; }; // mars_track_t
static_assert(sizeof(trk_t) == 8 && MHIP_OVERLAY_REC_INTS == 6 + MHIP_OVERLAY_TEXT_MAX / 4, "records of include/mars_hip.h and csrc/mhip.h");

__constant__ unsigned char ov_font[64][7] = MHIP_OVERLAY_FONT_ROWS;

#define OV_NONE 0xffffffffu
#define OV_PX 16 // pixels of a row a thread owns
static_assert(OV_PX * 4 == FT_TILE, "four threads on a row");

__global__ __launch_bounds__(FT_THREADS) void overlay_select_kernel(const mhip_overlay_t p) {
    __shared__ int wave_cnt[FT_THREADS / 64];
    __shared__ int mslot[MAXD], pslot[MAXD]; // the lowest mask / pose slot of this frame that names list index i; MAXD: none
    __shared__ __attribute__((aligned(4))) unsigned char txt[FT_THREADS][MHIP_OVERLAY_TEXT_MAX];
    __shared__ int cnt[4]; // masked, labels, markers, skipped
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, K = p.num_kpt;
    const int n = p.list_off ? max(p.counts[f], 0) : min(max(p.counts[f], 0), p.det_cap);
    const size_t base = p.list_off ? (size_t)p.list_off[f] : (size_t)f * p.det_cap;
    const size_t mbase = p.list_off ? base * (size_t)K : (size_t)f * p.mark_stride;
    for (int i = tid; i < MAXD; i += FT_THREADS) mslot[i] = pslot[i] = MAXD;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    if (p.mask_recs)
        for (int j = tid; j < p.mask_max; j += FT_THREADS) {
            const int d = ((const mask_t *)p.mask_recs)[(size_t)f * p.mask_max + j].det;
            if (d >= 0 && d < min(n, MAXD)) atomicMin(&mslot[d], j);
        }
    if (p.pose_recs)
        for (int j = tid; j < p.pose_max; j += FT_THREADS) {
            const int d = ((const pose_t *)p.pose_recs)[(size_t)f * p.pose_max + j].det;
            if (d >= 0 && d < min(n, MAXD)) atomicMin(&pslot[d], j);
        }
    __syncthreads();
    const det_t *dets = (const det_t *)p.dets + base;
    int kept = 0;
    for (int i0 = 0; i0 < n; i0 += FT_THREADS) {
        const int i = i0 + tid;
        bool ok = false, skip = false;
        int q[4] = {0, 0, 0, 0}, slot = -1, nt = 0;
        long long prow = -1;
        unsigned col = 0;
        if (i < n) {
            const det_t d = dets[i];
            trk_t tr = {-1, 0};
            if (p.tracks) tr = ((const trk_t *)p.tracks)[base + i];
            bool sel = p.select_all || (d.conf >= p.min_conf && (p.cls_count == 0 || ((long long)d.cls >= p.cls_first &&
                                                                                      (long long)d.cls < (long long)p.cls_first + p.cls_count)));
            if (sel && p.tracked_only) sel = tr.id >= 0 && tr.hits >= p.min_hits;
            if (sel) {
                ok = roi_rect(d, 1.0f, 1, p.w, p.h, q);
                skip = !ok;
            }
            if (ok) {
                const int key = p.keys ? p.keys[base + i] : p.color_by == 0 ? d.cls : p.color_by == 1 ? tr.id : 0;
                col = key >= 0 ? p.palette[key % p.n_palette] : p.no_key;
                if (p.layers & MHIP_OVERLAY_MASKS) {
                    if (p.mask_of) slot = max(p.mask_of[base + i], -1);
                    else if (p.mask_recs && i < MAXD && mslot[i] < MAXD) slot = f * p.mask_max + mslot[i];
                }
                if (p.layers & MHIP_OVERLAY_KEYPOINTS) {
                    if (p.kpt_rows) prow = (long long)(base + i);
                    else if (p.pose_recs && i < MAXD && pslot[i] < MAXD) prow = (long long)f * p.pose_max + pslot[i];
                }
                if (p.layers & MHIP_OVERLAY_LABELS) {
                    if (p.texts) {
                        const char *s = p.texts + (base + i) * MHIP_OVERLAY_TEXT_MAX;
                        while (nt < MHIP_OVERLAY_TEXT_MAX && s[nt]) { txt[tid][nt] = (unsigned char)s[nt]; nt++; }
                        for (int k = nt; k < MHIP_OVERLAY_TEXT_MAX; k++) txt[tid][k] = 0;
                    } else {
                        nt = mhip_overlay_text(txt[tid], p.text, p.names, p.n_names, d.cls, tr.id, d.conf);
                    }
                }
            }
        }
        int total;
        const int rank = block_rank<FT_THREADS / 64>(ok, wave_cnt, total);
        if (ok) {
            const int idx = kept + rank;
            int *t = p.table + (base + (size_t)idx) * MHIP_OVERLAY_REC_INTS;
            t[0] = q[0]; t[1] = q[1]; t[2] = q[2]; t[3] = q[3]; t[4] = slot;
            t[5] = (int)((col & 0x01ffffffu) | ((unsigned)nt << 25));
            for (int k = 0; k < MHIP_OVERLAY_TEXT_MAX / 4; k++) t[6 + k] = nt ? ((const int *)txt[tid])[k] : 0;
            if (prow >= 0)
                for (int j = 0; j < K; j++) {
                    const kpt_t kp = ((const kpt_t *)p.kpts)[(size_t)prow * K + j];
                    if (!(isfinite(kp.x) && isfinite(kp.y)) || !(kp.v >= p.kpt_min_v)) continue;
                    const float cx = floorf(kp.x), cy = floorf(kp.y);
                    if (cx < -8.0f || cx > (float)(p.w + 8) || cy < -8.0f || cy > (float)(p.h + 8)) continue; // before any conversion to int
                    int *m = p.marks + (mbase + (size_t)atomicAdd(&cnt[2], 1)) * 4; // a detection has one row: at most K markers each
                    m[0] = (int)cx; m[1] = (int)cy; m[2] = idx * 32 + j; m[3] = 0;
                }
        }
        const unsigned long long ms = __ballot(ok && slot >= 0), lb = __ballot(ok && nt > 0), sk = __ballot(skip);
        if (lane == 0) {
            if (ms) atomicAdd(&cnt[0], __popcll(ms));
            if (lb) atomicAdd(&cnt[1], __popcll(lb));
            if (sk) atomicAdd(&cnt[3], __popcll(sk));
        }
        kept += total;
        __syncthreads(); // behind the readers of wave_cnt, and the counts are in
    }
    if (tid == 0) {
        p.table_n[f] = kept;
        p.marks_n[f] = cnt[2];
        int *s = p.stats + (size_t)f * 6;
        s[0] = kept; s[1] = cnt[0]; s[2] = cnt[1]; s[3] = cnt[2]; s[4] = cnt[3]; s[5] = 0; // pixels: the tiles add to it
    }
}

// bits lo .. hi - 1 of the thread's 16 pixels; 0 <= lo < hi <= 16
__device__ __forceinline__ unsigned ov_span(const int lo, const int hi) { return span_mask(lo, hi - 1); }

// One plane of one tile: stage its rows, let every thread paint its own samples in LDS, store the rows back.  Called by every thread;
// barriers inside; LDS is free again on return.  paint(l): l = the thread's staged row.
template <int C, class Paint>
__device__ __forceinline__ void overlay_plane(const uint8_t *src, uint8_t *dst, const size_t pitch, const int tw, const int th, const unsigned long long *cov,
                                              const bool inplace, uint8_t *pix, const int prow, const Paint paint) {
    const int nb = tw * C;
    const bool wide = !(((uintptr_t)src | (uintptr_t)dst | pitch | (size_t)nb) & 15);
    (void)tile_rows_to_lds(src, pitch, nb, th, pix, wide);
    __syncthreads(); // every byte of the tile has been read: from here on it may be written
    if (prow >= 0 && prow < th) paint(pix + prow * FT_PITCH + (int)((uintptr_t)(src + (size_t)prow * pitch) & 3));
    __syncthreads();
    tile_rows_from_lds<C>(src, dst, pitch, nb, th, pix, wide, cov, inplace);
    __syncthreads();
}

__global__ __launch_bounds__(FT_THREADS) void overlay_kernel(const mhip_overlay_t p) {
    __shared__ __attribute__((aligned(16))) uint8_t pix[FT_TILE * FT_PITCH];
    __shared__ unsigned long long cov[FT_TILE], ccov[FT_TILE / 2];
    __shared__ int hits[FT_THREADS][8];
    __shared__ int nhits;
    const int tid = threadIdx.x, f = blockIdx.z, X0 = blockIdx.x * FT_TILE, Y0 = blockIdx.y * FT_TILE;
    const int W = p.w, H = p.h, tw = min(FT_TILE, W - X0), th = min(FT_TILE, H - Y0);
    const bool inplace = p.dst == p.frames;
    const int n = p.table_n[f], nm = p.marks_n[f];
    const size_t base = p.list_off ? (size_t)p.list_off[f] : (size_t)f * p.det_cap;
    const int *tab = p.table + base * MHIP_OVERLAY_REC_INTS;
    const int *mk = p.marks + (p.list_off ? base * (size_t)p.num_kpt : (size_t)f * p.mark_stride) * 4;
    const size_t mpitch = (size_t)((W + 31) >> 5);
    const int row = tid >> 2, sub = tid & 3, y = Y0 + row, px = X0 + OV_PX * sub; // the thread's pixels: px .. px + 15 of row y
    const int nv = y < H ? min(max(W - px, 0), OV_PX) : 0;
    const unsigned vbits = nv ? ov_span(0, nv) : 0u; // those inside the frame
    const unsigned layers = p.layers;
    const int T = p.thick, S = p.scale, R = p.radius;
    unsigned oo[OV_PX], ot[OV_PX]; // per pixel: the opaque owner (priority << 28 | key), the tint owner (element)
#pragma unroll
    for (int k = 0; k < OV_PX; k++) oo[k] = ot[k] = OV_NONE;
    bool any = false;
    // ---- the frame's elements against this tile: outline, tint and label of each
    for (int i0 = 0; i0 < n; i0 += FT_THREADS) {
        if (tid == 0) nhits = 0;
        __syncthreads();
        if (i0 + tid < n) {
            const int *t = tab + (size_t)(i0 + tid) * MHIP_OVERLAY_REC_INTS;
            const int x0 = t[0], y0 = t[1], x1 = t[2], y1 = t[3], cn = t[5], nt = (cn >> 25) & 31;
            int bx1 = x1, by0 = y0, by1 = y1; // the rectangle and the label's strip
            if ((layers & MHIP_OVERLAY_LABELS) && nt) {
                const int Hl = 9 * S, ly = y0 - Hl >= 0 ? y0 - Hl : y0;
                by0 = min(by0, ly); by1 = max(by1, ly + Hl); bx1 = max(bx1, x0 + S * (6 * nt + 1));
            }
            if (x0 < X0 + FT_TILE && bx1 > X0 && by0 < Y0 + FT_TILE && by1 > Y0) {
                int *h = hits[atomicAdd(&nhits, 1)]; // in any order: a minimum does not depend on it
                h[0] = x0; h[1] = y0; h[2] = x1; h[3] = y1; h[4] = t[4]; h[5] = cn; h[6] = i0 + tid;
            }
        }
        __syncthreads();
        const int nh = nhits;
        any |= nh > 0;
        for (int e = 0; e < nh && vbits; e++) {
            const int *h = hits[e];
            const int x0 = h[0], y0 = h[1], x1 = h[2], y1 = h[3], slot = h[4], nt = (h[5] >> 25) & 31, idx = h[6];
            unsigned obits = 0, tbits = 0, lbits = 0, xbits = 0; // outline, tint, label strip, label text
            if (y >= y0 && y < y1 && x0 < px + OV_PX && x1 > px) {
                const unsigned rb = ov_span(max(x0, px) - px, min(x1, px + OV_PX) - px);
                if (layers & MHIP_OVERLAY_BOXES) {
                    unsigned ib = 0; // the inner rectangle's part of the row
                    const int ix0 = x0 + T, ix1 = x1 - T;
                    if (y >= y0 + T && y < y1 - T && ix0 < ix1) {
                        const int il = max(ix0, px) - px, ih = min(ix1, px + OV_PX) - px;
                        if (ih > il) ib = ov_span(il, ih);
                    }
                    obits = rb & ~ib;
                }
                if ((layers & MHIP_OVERLAY_MASKS) && slot >= 0) // y < y1 <= H; px < x1 <= W; the 16 pixels lie in one word
                    tbits = rb & (p.mask_words[((size_t)slot * H + y) * mpitch + (px >> 5)] >> (px & 31));
            }
            if ((layers & MHIP_OVERLAY_LABELS) && nt) {
                const int Hl = 9 * S, Wl = S * (6 * nt + 1), ly = y0 - Hl >= 0 ? y0 - Hl : y0;
                if (y >= ly && y < ly + Hl && x0 < px + OV_PX && x0 + Wl > px) {
                    const int lo = max(x0, px) - px, hi = min(x0 + Wl, px + OV_PX) - px, v = y - ly - S;
                    lbits = ov_span(lo, hi);
                    if (v >= 0 && v < 7 * S) {
                        const int vr = v / S;
                        const uint8_t *tx = (const uint8_t *)(tab + (size_t)idx * MHIP_OVERLAY_REC_INTS + 6);
                        for (int k = lo; k < hi; k++) {
                            const int u = px + k - x0 - S;
                            if (u < 0) continue;
                            const int kk = u / (6 * S), m = u - kk * 6 * S;
                            if (kk < nt && m < 5 * S && ((ov_font[mhip_overlay_glyph_index(tx[kk])][vr] >> (4 - m / S)) & 1)) xbits |= 1u << k;
                        }
                    }
                }
            }
            lbits &= vbits; obits &= vbits; tbits &= vbits;
            if (!(lbits | obits | tbits)) continue;
            const unsigned kl = (unsigned)idx << 1, ko = (2u << 28) | kl;
#pragma unroll
            for (int k = 0; k < OV_PX; k++) {
                if ((lbits >> k) & 1u) oo[k] = min(oo[k], kl | ((xbits >> k) & 1u));
                else if ((obits >> k) & 1u) oo[k] = min(oo[k], ko);
                if ((tbits >> k) & 1u) ot[k] = min(ot[k], (unsigned)idx);
            }
        }
        __syncthreads(); // the next round rewrites nhits and the hits
    }
    // ---- the frame's markers against this tile
    for (int i0 = 0; i0 < nm; i0 += FT_THREADS) {
        if (tid == 0) nhits = 0;
        __syncthreads();
        if (i0 + tid < nm) {
            const int *t = mk + (size_t)(i0 + tid) * 4;
            const int cx = t[0], cy = t[1];
            if (cx - R < X0 + FT_TILE && cx + R >= X0 && cy - R < Y0 + FT_TILE && cy + R >= Y0) {
                int *h = hits[atomicAdd(&nhits, 1)];
                h[0] = cx; h[1] = cy; h[2] = t[2];
            }
        }
        __syncthreads();
        const int nh = nhits;
        any |= nh > 0;
        for (int e = 0; e < nh && vbits; e++) {
            const int *h = hits[e];
            const int cx = h[0], cy = h[1];
            if (y < cy - R || y > cy + R) continue;
            const int lo = max(cx - R, px) - px, hi = min(cx + R + 1, px + OV_PX) - px;
            if (hi <= lo) continue;
            const unsigned bits = ov_span(lo, hi) & vbits, km = (1u << 28) | (unsigned)h[2];
#pragma unroll
            for (int k = 0; k < OV_PX; k++)
                if ((bits >> k) & 1u) oo[k] = min(oo[k], km);
        }
        __syncthreads();
    }
    if (inplace && !any) return; // nothing of this tile changes: no byte is touched
    // ---- every pixel's colour; the coverage of the rows, for the in-place stores and the statistics
    unsigned col[OV_PX], cb = 0, opq = 0;
#pragma unroll
    for (int k = 0; k < OV_PX; k++) {
        unsigned c = 0;
        if (oo[k] != OV_NONE) {
            const unsigned prio = oo[k] >> 28;
            if (prio == 1u) {
                c = p.palette[(oo[k] & 31u) % (unsigned)p.n_palette];
            } else {
                const unsigned rec = (unsigned)tab[(size_t)((oo[k] & 0x0fffffffu) >> 1) * MHIP_OVERLAY_REC_INTS + 5];
                c = prio == 0u && (oo[k] & 1u) ? p.text_col[(rec >> 24) & 1u] : rec;
            }
            opq |= 1u << k;
            cb |= 1u << k;
        } else if (ot[k] != OV_NONE) {
            c = (unsigned)tab[(size_t)ot[k] * MHIP_OVERLAY_REC_INTS + 5];
            cb |= 1u << k;
        }
        col[k] = c & 0x00ffffffu;
    }
    ((unsigned short *)cov)[tid] = (unsigned short)cb; // bits 16 * sub .. of cov[row]
    if (tid < FT_TILE / 2) ccov[tid] = 0ull;
    {
        int k = __popc(cb);
        for (int s = 32; s > 0; s >>= 1) k += __shfl_xor(k, s, 64);
        if ((tid & 63) == 0 && k) atomicAdd(p.stats + (size_t)f * 6 + 5, k);
    }
    __syncthreads();
    const int A = p.alpha;
    // bytes c0 .. c0 + C - 1 of the colour over sample s of the thread's staged row
    const auto put = [&](uint8_t *l, const int s, const int C, const int c0, const int k) {
        for (int c = 0; c < C; c++) {
            const int v = (int)((col[k] >> (8 * (c0 + c))) & 255u);
            l[s * C + c] = (uint8_t)((opq >> k) & 1u ? v : (l[s * C + c] * (256 - A) + v * A + 128) >> 8);
        }
    };
    const uint8_t *sf = p.frames + (size_t)f * p.frame_stride;
    uint8_t *df = p.dst + (size_t)f * p.frame_stride;
    if (p.fmt == 0) {
        const size_t o = ((size_t)Y0 * W + X0) * 3;
        overlay_plane<3>(sf + o, df + o, (size_t)W * 3, tw, th, cov, inplace, pix, row, [&](uint8_t *l) {
#pragma unroll
            for (int k = 0; k < OV_PX; k++)
                if ((cb >> k) & 1u) put(l, OV_PX * sub + k, 3, 0, k);
        });
        return;
    }
    // NV12: chroma sample (i, j) follows pixel (2i, 2j): the even pixels of the even rows
    unsigned sb = 0;
#pragma unroll
    for (int k = 0; k < OV_PX; k += 2) sb |= ((cb >> k) & 1u) << (k >> 1);
    if (!(row & 1)) ((uint8_t *)ccov)[(row >> 1) * 8 + sub] = (uint8_t)sb; // bits 8 * sub .. of ccov[row / 2]
    const size_t oy = (size_t)Y0 * W + X0, oc = (size_t)W * H + (size_t)(Y0 >> 1) * W + X0; // W and the tile origin are even
    overlay_plane<1>(sf + oy, df + oy, (size_t)W, tw, th, cov, inplace, pix, row, [&](uint8_t *l) {
#pragma unroll
        for (int k = 0; k < OV_PX; k++)
            if ((cb >> k) & 1u) put(l, OV_PX * sub + k, 1, 0, k);
    });
    overlay_plane<2>(sf + oc, df + oc, (size_t)W, tw >> 1, th >> 1, ccov, inplace, pix, row & 1 ? -1 : row >> 1, [&](uint8_t *l) {
#pragma unroll
        for (int k = 0; k < OV_PX; k += 2)
            if ((cb >> k) & 1u) put(l, (OV_PX / 2) * sub + (k >> 1), 2, 1, k);
    });
}

static bool overlay_ok(const mhip_overlay_t *p) {
    const size_t fb = p ? mhip_frame_bytes(p->w, p->h, p->fmt) : 0;
    return fb && p->frames && p->dst && p->table && p->table_n && p->marks && p->marks_n && p->stats && p->dets && p->counts && p->n_frames > 0 &&
           p->n_frames <= 65535 && p->w <= MHIP_OVERLAY_MAX_DIM && p->h <= MHIP_OVERLAY_MAX_DIM && (p->fmt == 0 || p->fmt == 1) && p->frame_stride >= fb &&
           (p->list_off || (p->det_cap > 0 && p->det_cap <= MAXD)) && p->cls_count >= 0 && p->color_by >= 0 && p->color_by <= 2 && p->text && !(p->text & ~7u) &&
           (!p->names || p->n_names > 0) && (!p->mask_recs || (p->mask_max > 0 && p->mask_max <= MAXD)) && ((!p->mask_recs && !p->mask_of) || p->mask_words) &&
           (!p->pose_recs || (p->pose_max > 0 && p->pose_max <= MAXD)) && ((!p->pose_recs && !p->kpt_rows) || p->kpts) && p->num_kpt >= 1 &&
           p->num_kpt <= MHIP_OVERLAY_MAX_KPT && (p->list_off || !p->pose_recs || p->mark_stride >= (size_t)p->pose_max * p->num_kpt) &&
           (p->list_off || !p->kpt_rows) && p->layers && !(p->layers & ~15u) && p->thick >= 1 && p->thick <= 16 && p->radius >= 1 && p->radius <= 8 &&
           p->scale >= 1 && p->scale <= 8 && p->alpha >= 1 && p->alpha <= 256 && p->palette && p->n_palette >= 1 && p->n_palette <= 256 && p->min_hits >= 1;
}

extern "C" int mhip_overlay_select(const mhip_overlay_t *p) {
    if (!overlay_ok(p)) return -1;
    hipLaunchKernelGGL(overlay_select_kernel, dim3((unsigned)p->n_frames), dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "overlay select");
}

extern "C" int mhip_overlay(const mhip_overlay_t *p) {
    if (!overlay_ok(p)) return -1;
    const dim3 g((unsigned)((p->w + FT_TILE - 1) / FT_TILE), (unsigned)((p->h + FT_TILE - 1) / FT_TILE), (unsigned)p->n_frames);
    hipLaunchKernelGGL(overlay_kernel, g, dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "overlay");
}
