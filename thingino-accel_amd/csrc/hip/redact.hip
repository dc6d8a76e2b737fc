// redact.hip -- redaction on gfx950: the detections a tail left in HBM -> the camera frames with what they found mosaicked or filled, before a
// frame is encoded, stored or streamed.  include/mars_hip.h ("Redaction") states the rule; everything that touches a pixel is integer
// arithmetic, so the bytes are defined exactly.  The reference has no such step (its demo stops at the boxes, src/mars/mars_yolo_test.c:132-214).
//   redact_select_kernel   one workgroup per frame: the selection (confidence, class window, identities that spare, or every box of a
//                          caller's list), the rectangle rule of "ROI crops" (roi_rect of tail_core.hpp, min_size 1), the mask slot of a
//                          detection that has one; the kept regions go in list order (block_rank of tail_core.hpp) into the frame's table
//                          {x0, y0, x1, y1, slot or -1}, with their number and the regions / masked / skipped counts;
//   redact_kernel          one workgroup of 256 threads per 64 x 64 pixel tile and frame.  A tile is cell-aligned for every legal cell
//                          (2 .. 64) and two whole mask words wide.  The workgroup scans its frame's table against its tile, ORs the
//                          rectangles and mask words into a 64 x 64 bit coverage map, stages the tile's rows in LDS, forms the cell
//                          sums there (rows first, then cells), replaces the covered pixels in LDS and stores rows back.  NV12: the luma
//                          tile, then its 32 x 32 chroma samples with the any-of-four coverage.
// Why the in-place form has no race: a cell is owned by exactly ONE workgroup (tiles are cell-aligned and disjoint), and that workgroup has
// read every byte of its tile into LDS -- a barrier behind the loads -- before it stores the first one.  No workgroup reads or writes a
// byte of another tile: the wide stores below never reach over a tile row's ends, those are byte stores.  So the result is a function of
// the original frame alone, in place as out of place.  A workgroup whose tile meets no region leaves at once and, in place, touches no pixel.
// Rows of 3 * W bytes have any alignment: a row is moved as 16-byte units where the tile's rows are all 16-byte aligned on both sides,
// else as bytes up to the first 4-byte boundary, 4-byte units and bytes behind the last one; its LDS copy is shifted by the row's address
// & 3, so both sides of every 4-byte move are aligned (tile_rows_to_lds and tile_rows_from_lds of frame_tile.hpp).  All stores are plain vector
// stores from C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "frame_tile.hpp"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define RD_CELLS 32    // cells per tile side at most (cell 2; a chroma tile at cell 2 has 32 cells of one sample)

__global__ __launch_bounds__(FT_THREADS) void redact_select_kernel(const mhip_redact_t p) {
    __shared__ int wave_cnt[FT_THREADS / 64];
    __shared__ int slot_det[64]; // the list index each mask slot of this frame belongs to, -1: none
    __shared__ int cnt[2];       // masked, skipped
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int n = p.list_off ? max(p.counts[f], 0) : min(max(p.counts[f], 0), p.det_cap);
    const size_t base = p.list_off ? (size_t)p.list_off[f] : (size_t)f * p.det_cap;
    if (tid < 64) slot_det[tid] = p.mask_recs && tid < p.mask_max ? ((const mask_t *)p.mask_recs)[(size_t)f * p.mask_max + tid].det : -1;
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const det_t *dets = (const det_t *)p.dets + base;
    int kept = 0;
    for (int i0 = 0; i0 < n; i0 += FT_THREADS) {
        const int i = i0 + tid;
        bool ok = false, skip = false;
        int q[4] = {0, 0, 0, 0}, slot = -1;
        if (i < n) {
            const det_t d = dets[i];
            bool sel = p.select_all || (d.conf >= p.min_conf && (p.cls_count == 0 || ((long long)d.cls >= p.cls_first &&
                                                                                      (long long)d.cls < (long long)p.cls_first + p.cls_count)));
            if (sel && p.idents) { // an identified detection is spared
                const cls_t id = ((const cls_t *)p.idents)[base + i];
                if (id.cls >= 0 && id.score >= p.ident_min) sel = false;
            }
            if (sel) {
                ok = roi_rect(d, p.expand, 1, p.w, p.h, q);
                skip = !ok;
            }
            if (ok && p.mask_of) {
                slot = max(p.mask_of[base + i], -1);
            } else if (ok && p.mask_recs) {
                for (int j = 0; j < p.mask_max; j++)
                    if (slot_det[j] == i) { slot = f * p.mask_max + j; break; }
            }
        }
        int total;
        const int rank = block_rank<FT_THREADS / 64>(ok, wave_cnt, total);
        if (ok) {
            int *t = p.table + (base + (size_t)(kept + rank)) * 5;
            t[0] = q[0]; t[1] = q[1]; t[2] = q[2]; t[3] = q[3]; t[4] = slot;
        }
        const unsigned long long ms = __ballot(ok && slot >= 0), sk = __ballot(skip);
        if (lane == 0) {
            if (ms) atomicAdd(&cnt[0], __popcll(ms));
            if (sk) atomicAdd(&cnt[1], __popcll(sk));
        }
        kept += total;
        __syncthreads(); // behind the readers of wave_cnt, and the counts are in
    }
    if (tid == 0) {
        p.table_n[f] = kept;
        int *s = p.stats + (size_t)f * 4;
        s[0] = kept; s[1] = cnt[0]; s[2] = cnt[1]; s[3] = 0; // pixels: the tiles add to it
    }
}

// One plane of one tile: tw x th samples of C bytes at src, rows `pitch` bytes apart, the same place of the destination at dst; cells of
// 1 << bl samples a side, bit x of cov[r] = sample (x, r) is redacted.  Called by every thread; barriers inside; LDS is free again on return.
template <int C>
__device__ __forceinline__ void redact_plane(const uint8_t *src, uint8_t *dst, const size_t pitch, const int tw, const int th, const int bl, const int mode,
                                             const unsigned fill /* byte c: channel c's fill value */, const unsigned long long *cov, const bool any, const bool inplace, uint8_t *pix,
                                             unsigned short *rowsum, uint8_t *val) {
    const int tid = threadIdx.x;
    const int nb = tw * C;
    const bool wide = !(((uintptr_t)src | (uintptr_t)dst | pitch | (size_t)nb) & 15);
    // ---- the tile's rows -> LDS, row r at pix + r * FT_PITCH + (its address & 3); wide here: the stores below go the same way
    (void)tile_rows_to_lds(src, pitch, nb, th, pix, wide);
    __syncthreads(); // every byte of the tile has been read: from here on it may be written
    if (any) {
        const int B = 1 << bl, ncx = (tw + B - 1) >> bl, ncy = (th + B - 1) >> bl;
        if (mode == 0) {
            // the sums of the ORIGINAL bytes: a row's part of every cell, then the cells
            for (int it = tid; it < th * ncx * C; it += FT_THREADS) {
                const int c = it % C, t2 = it / C, cx = t2 % ncx, r = t2 / ncx;
                const uint8_t *l = pix + r * FT_PITCH + (int)((uintptr_t)(src + (size_t)r * pitch) & 3);
                const int x1 = min(tw, (cx + 1) << bl);
                int s = 0;
                for (int x = cx << bl; x < x1; x++) s += l[x * C + c];
                rowsum[(r * RD_CELLS + cx) * C + c] = (unsigned short)s; // <= 64 * 255
            }
            __syncthreads();
            for (int it = tid; it < ncy * ncx * C; it += FT_THREADS) {
                const int c = it % C, t2 = it / C, cx = t2 % ncx, cy = t2 / ncx;
                const int r1 = min(th, (cy + 1) << bl);
                int s = 0;
                for (int r = cy << bl; r < r1; r++) s += rowsum[(r * RD_CELLS + cx) * C + c];
                const int n = (r1 - (cy << bl)) * (min(tw, (cx + 1) << bl) - (cx << bl));
                val[(cy * RD_CELLS + cx) * C + c] = (uint8_t)((s + n / 2) / n);
            }
            __syncthreads();
        }
        for (int s = tid; s < FT_TILE * FT_TILE; s += FT_THREADS) {
            const int r = s >> 6, x = s & 63;
            if (r < th && x < tw && ((cov[r] >> x) & 1ull)) {
                uint8_t *l = pix + r * FT_PITCH + (int)((uintptr_t)(src + (size_t)r * pitch) & 3) + x * C;
                const uint8_t *v = val + ((r >> bl) * RD_CELLS + (x >> bl)) * C;
#pragma unroll
                for (int c = 0; c < C; c++) l[c] = mode ? (uint8_t)(fill >> (8 * c)) : v[c];
            }
        }
        __syncthreads();
    }
    // ---- LDS -> the destination: everything out of place, in place the units that hold a redacted sample (frame_tile.hpp)
    tile_rows_from_lds<C>(src, dst, pitch, nb, th, pix, wide, cov, inplace);
    __syncthreads();
}

__global__ __launch_bounds__(FT_THREADS) void redact_kernel(const mhip_redact_t p) {
    __shared__ __attribute__((aligned(16))) uint8_t pix[FT_TILE * FT_PITCH];
    __shared__ unsigned short rowsum[FT_TILE * RD_CELLS * 3];
    __shared__ uint8_t val[RD_CELLS * RD_CELLS * 3];
    __shared__ unsigned long long cov[FT_TILE], ccov[FT_TILE / 2];
    __shared__ unsigned covh[2][2 * FT_TILE];
    __shared__ int hits[FT_THREADS][5];
    __shared__ int nhits;
    const int tid = threadIdx.x, f = blockIdx.z, X0 = blockIdx.x * FT_TILE, Y0 = blockIdx.y * FT_TILE;
    const int W = p.w, H = p.h, tw = min(FT_TILE, W - X0), th = min(FT_TILE, H - Y0);
    const bool inplace = p.dst == p.frames;
    const int n = p.table_n[f];
    const int *tab = p.table + (p.list_off ? (size_t)p.list_off[f] : (size_t)f * p.det_cap) * 5;
    const size_t mpitch = (size_t)((W + 31) >> 5);
    // ---- the frame's regions against this tile: thread (half, row, word) ORs every second hit into its 32 pixels of the coverage map
    const int row = (tid >> 1) & (FT_TILE - 1), word = tid & 1, half = tid >> 7;
    unsigned acc = 0;
    bool any = false;
    for (int i0 = 0; i0 < n; i0 += FT_THREADS) {
        if (tid == 0) nhits = 0;
        __syncthreads();
        if (i0 + tid < n) {
            const int *t = tab + (size_t)(i0 + tid) * 5;
            const int x0 = t[0], y0 = t[1], x1 = t[2], y1 = t[3];
            if (x0 < X0 + FT_TILE && x1 > X0 && y0 < Y0 + FT_TILE && y1 > Y0) {
                int *h = hits[atomicAdd(&nhits, 1)]; // in any order: the union does not depend on it
                h[0] = x0; h[1] = y0; h[2] = x1; h[3] = y1; h[4] = t[4];
            }
        }
        __syncthreads();
        const int nh = nhits;
        any |= nh > 0;
        const int y = Y0 + row, px = X0 + 32 * word;
        for (int e = half; e < nh; e += 2) {
            const int *h = hits[e];
            const int lo = max(h[0], px) - px, hi = min(h[2], px + 32) - px;
            if (y < h[1] || y >= h[3] || hi <= lo) continue;
            unsigned bits = span_mask(lo, hi - 1);
            if (h[4] >= 0) bits &= p.mask_words[((size_t)h[4] * H + y) * mpitch + (px >> 5)]; // y < y1 <= H; px < x1 <= W
            acc |= bits;
        }
        __syncthreads(); // the next round rewrites nhits and the hits
    }
    if (inplace && !any) return; // nothing of this tile changes: no pixel is touched
    covh[half][2 * row + word] = acc;
    __syncthreads();
    if (tid < FT_TILE) {
        const unsigned long long c = (unsigned long long)(covh[0][2 * tid] | covh[1][2 * tid]) |
                                     ((unsigned long long)(covh[0][2 * tid + 1] | covh[1][2 * tid + 1]) << 32);
        cov[tid] = c;
        int k = __popcll(c);
        for (int s = 32; s > 0; s >>= 1) k += __shfl_xor(k, s, 64);
        if (tid == 0 && k) atomicAdd(p.stats + (size_t)f * 4 + 3, k); // the rectangles end at the frame's edges: no bit lies outside it
    }
    __syncthreads();
    const unsigned f0 = p.fill[0], f1 = p.fill[1], f2 = p.fill[2];
    const uint8_t *sf = p.frames + (size_t)f * p.frame_stride;
    uint8_t *df = p.dst + (size_t)f * p.frame_stride;
    if (p.fmt == 0) {
        const size_t o = ((size_t)Y0 * W + X0) * 3;
        redact_plane<3>(sf + o, df + o, (size_t)W * 3, tw, th, p.cell_log2, p.mode, f0 | (f1 << 8) | (f2 << 16), cov, any, inplace, pix, rowsum, val);
        return;
    }
    if (tid < FT_TILE / 2) { // a chroma sample is redacted iff any of its four pixels is: the even bits of the two rows' OR, packed
        unsigned long long m = cov[2 * tid] | cov[2 * tid + 1];
        m = (m | (m >> 1)) & 0x5555555555555555ull;
        m = (m | (m >> 1)) & 0x3333333333333333ull;
        m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
        m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
        m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
        m = (m | (m >> 16)) & 0x00000000ffffffffull;
        ccov[tid] = m;
    }
    __syncthreads();
    const size_t oy = (size_t)Y0 * W + X0, oc = (size_t)W * H + (size_t)(Y0 >> 1) * W + X0; // W and the tile origin are even
    const unsigned cfill = p.nv12_flags & 2u ? f2 | (f1 << 8) : f1 | (f2 << 8); // U, V; V, U under MARS_NV12_VU
    redact_plane<1>(sf + oy, df + oy, (size_t)W, tw, th, p.cell_log2, p.mode, f0, cov, any, inplace, pix, rowsum, val);
    redact_plane<2>(sf + oc, df + oc, (size_t)W, tw >> 1, th >> 1, p.cell_log2 - 1, p.mode, cfill, ccov, any, inplace, pix, rowsum, val);
}

static bool redact_ok(const mhip_redact_t *p) {
    const size_t fb = p ? mhip_frame_bytes(p->w, p->h, p->fmt) : 0;
    return fb && p->frames && p->dst && p->table && p->table_n && p->stats && p->dets && p->counts && p->n_frames > 0 && p->n_frames <= 65535 &&
           p->w <= MHIP_REDACT_MAX_DIM && p->h <= MHIP_REDACT_MAX_DIM && mhip_frame_format_ok(p->fmt, p->nv12_flags) && p->frame_stride >= fb &&
           (p->list_off || p->det_cap > 0) && p->expand > 0 && p->cls_count >= 0 &&
           (p->mode == 0 || p->mode == 1) && p->cell_log2 >= 1 && p->cell_log2 <= 6 && (!p->mask_recs || (p->mask_max > 0 && p->mask_max <= 64)) &&
           ((!p->mask_recs && !p->mask_of) || p->mask_words);
}

extern "C" int mhip_redact_select(const mhip_redact_t *p) {
    if (!redact_ok(p)) return -1;
    hipLaunchKernelGGL(redact_select_kernel, dim3((unsigned)p->n_frames), dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "redact select");
}

extern "C" int mhip_redact(const mhip_redact_t *p) {
    if (!redact_ok(p)) return -1;
    const dim3 g((unsigned)((p->w + FT_TILE - 1) / FT_TILE), (unsigned)((p->h + FT_TILE - 1) / FT_TILE), (unsigned)p->n_frames);
    hipLaunchKernelGGL(redact_kernel, g, dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "redact");
}
