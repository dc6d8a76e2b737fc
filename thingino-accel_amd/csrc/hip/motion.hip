// motion.hip -- motion maps on gfx950: camera frames in HBM -> per frame a bit map of the grid cells whose mean luma left the stream's
// background, its statistics, zone counts, and per detection the share of its cells that moved.  include/mars_hip.h ("Motion") states the
// rule; everything is integer arithmetic except the rectangle rule of "ROI crops" (roi_rect of tail_core.hpp), so every result is defined
// exactly.  The reference has no such stage.
//   motion_cells_kernel    one workgroup of 256 threads per 64 x 64 pixel tile and STREAM.  A tile is cell-aligned for every legal cell
//                          (4 .. 64) and holds at most 256 cells: thread t owns cell t of the tile and keeps its background in a register
//                          across the stream's steps of the call -- loaded once, stored once.  Per step the tile's rows (the Y plane of an
//                          NV12 frame) go to LDS (tile_rows_to_lds of frame_tile.hpp), four threads on a row reduce 16 pixels each to luma and to
//                          their cells' parts of the row, the owning thread adds the rows, compares, updates and stores one raw byte.
//   motion_map_kernel      one workgroup per frame, a thread per 32 cells of a grid row (raw rows are padded to whole words, so the 32 bytes
//                          come as two aligned 16-byte loads): the three rows' raw bits in registers, the neighbour count by popcounts,
//                          the packed word (padding bits zero), and into LDS integers the active count, the bounding box, the zone counts.
//   motion_dets_kernel     a thread per list entry: roi_rect, the rectangle's cell range, a popcount over the map words it spans.
// Why no step of a stream overtakes its predecessor: the step loop runs INSIDE the workgroup that owns the tile, so one call over 2T steps
// leaves what two calls over T steps leave.  Why no two workgroups meet: a background cell and a raw byte belong to exactly one tile of one
// stream.  The raw bytes are not packed here -- from cell 16 on a tile owns fewer than 8 bits of a map word and two workgroups would share a
// byte -- the second launch packs them.  The initialised flag is read by the first launch and written by the second alone, and a frame's
// `first` is written by tile (0, 0) of its stream alone.  Every sum in the second launch is an integer: LDS atomics give the same result in
// any order.  All stores are plain vector stores from C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mhip.h"
#include "frame_tile.hpp"
#include "tail_core.hpp"

extern "C" hipStream_t mhip_stream_native(void);
extern "C" int mhip_check(hipError_t e, const char *what);

#define MO_CELLS 16    // cells per tile side at most (cell 4)

// 16 pixels of C bytes from byte `o` of an LDS row (any alignment) -> their luma; pixels from `valid` on give 0.  The word reads end at byte
// 196 of the row at most (o <= 3 + 144, thirteen words from o & ~3): inside FT_PITCH
template <int C>
__device__ __forceinline__ void luma16(const uint8_t *row, const int o, const int valid, int y[16]) {
    const uint32_t *w = (const uint32_t *)(row + (o & ~3));
    const unsigned sh = (unsigned)o & 3u;
    uint32_t v[4 * C];
    uint32_t lo = w[0];
#pragma unroll
    for (int j = 0; j < 4 * C; j++) {
        const uint32_t hi = w[j + 1];
        v[j] = __builtin_amdgcn_alignbyte(hi, lo, sh); // bytes o + 4 j .. o + 4 j + 3
        lo = hi;
    }
#pragma unroll
    for (int x = 0; x < 16; x++) {
        int l;
        if (C == 1) {
            l = (int)((v[x >> 2] >> (8 * (x & 3))) & 255u);
        } else {
            const int k = 3 * x;
            const int r = (int)((v[k >> 2] >> (8 * (k & 3))) & 255u), g = (int)((v[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255u),
                      b = (int)((v[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 255u);
            l = (77 * r + 150 * g + 29 * b + 128) >> 8;
        }
        y[x] = x < valid ? l : 0;
    }
}

template <int C>
__global__ __launch_bounds__(FT_THREADS) void motion_cells_kernel(const mhip_motion_t p) {
    __shared__ __attribute__((aligned(16))) uint8_t pix[FT_TILE * FT_PITCH];
    __shared__ unsigned short part[FT_TILE * MO_CELLS]; // [row][cell column of the tile]: the row's part of the cell's sum, <= 64 * 255
    const int tid = threadIdx.x, row = tid >> 2, sub = tid & 3; // four threads on a row
    const int s = blockIdx.z, X0 = blockIdx.x * FT_TILE, Y0 = blockIdx.y * FT_TILE;
    const int W = p.w, H = p.h, bl = p.cell_log2, B = 1 << bl;
    const int tw = min(FT_TILE, W - X0), th = min(FT_TILE, H - Y0);
    const int ncx = (tw + B - 1) >> bl, ncy = (th + B - 1) >> bl;
    const size_t pitch = (size_t)W * C;
    const int nb = tw * C;
    // the cell this thread owns
    const bool owner = tid < ncx * ncy;
    const int cx = owner ? tid % ncx : 0, cy = owner ? tid / ncx : 0;
    const int r0 = cy << bl, r1 = min(th, r0 + B);
    const int n = (min(tw, (cx + 1) << bl) - (cx << bl)) * (r1 - r0);
    const size_t gy = (size_t)(Y0 >> bl) + cy, gx = (size_t)(X0 >> bl) + cx; // inside the grid: cx < ncx, cy < ncy
    const size_t rp = 32 * (size_t)p.pitch;                                   // bytes of a raw row: whole map words
    uint16_t *bgp = p.bg + ((size_t)s * p.gh + gy) * p.gw + gx;
    const int init0 = p.init[s];
    int bg = owner && init0 ? (int)*bgp : 0;
    int init = init0;
    const int thr = 256 * p.threshold;
    for (int t = 0; t < p.steps; t++) {
        const size_t f = p.stream_major ? (size_t)s * p.steps + t : (size_t)t * p.streams + s;
        const uint8_t *src = p.frames + f * p.frame_stride + ((size_t)Y0 * W + X0) * C;
        const bool wide = !(((uintptr_t)src | pitch | (size_t)nb) & 15);
        // ---- the tile's rows -> LDS, row r at pix + r * FT_PITCH + (its address & 3); nothing is read behind a row's last byte
        const int sh = tile_rows_to_lds(src, pitch, nb, th, pix, wide);
        __syncthreads();
        // ---- pixels 16 sub .. 16 sub + 15 of the row -> luma -> the row's parts of the cells they lie in
        int y[16];
        if (row < th) {
            luma16<C>(pix + row * FT_PITCH, sh + 16 * sub * C, tw - 16 * sub, y);
        } else {
#pragma unroll
            for (int x = 0; x < 16; x++) y[x] = 0;
        }
        int q[4]; // sums of four pixels
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = (y[4 * j] + y[4 * j + 1]) + (y[4 * j + 2] + y[4 * j + 3]);
        unsigned short *pr = part + row * MO_CELLS;
        if (bl == 2) {
#pragma unroll
            for (int j = 0; j < 4; j++) pr[4 * sub + j] = (unsigned short)q[j];
        } else if (bl == 3) {
            pr[2 * sub] = (unsigned short)(q[0] + q[1]);
            pr[2 * sub + 1] = (unsigned short)(q[2] + q[3]);
        } else {
            int v = (q[0] + q[1]) + (q[2] + q[3]);
            if (bl >= 5) v += __shfl_xor(v, 1, 64); // the four threads of a row are neighbouring lanes
            if (bl >= 6) v += __shfl_xor(v, 2, 64);
            if (!(sub & ((1 << (bl - 4)) - 1))) pr[sub >> (bl - 4)] = (unsigned short)v;
        }
        __syncthreads();
        // ---- the cell: rows added, the mean in 8.8, the compare, the update
        if (owner) {
            int S = 0;
            for (int r = r0; r < r1; r++) S += part[r * MO_CELLS + cx];
            const int m = (int)((256u * (unsigned)S + (unsigned)(n >> 1)) / (unsigned)n);
            int raw = 0;
            if (!init) {
                bg = m;
            } else {
                const int delta = m - bg, ad = delta < 0 ? -delta : delta;
                raw = ad > thr;
                if (p.frame_diff) {
                    bg = m;
                } else {
                    const int k = raw ? p.learn_active : p.learn, d = ad >> k; // k <= 16 and ad < 65536: a shift of 16 gives 0
                    bg += delta < 0 ? -d : d;
                }
            }
            p.raw[(f * p.gh + gy) * rp + gx] = (uint8_t)raw;
        }
        if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) p.stats[f * 6 + 5] = !init && t == 0;
        init = 1;
        // (the next step's loads write pix behind the second barrier above, its parts behind its first one: every reader is through)
    }
    if (owner) *bgp = (uint16_t)bg; // 0 .. 65280
}

// cells c0 - 1 .. c0 + 32 of raw row cy as bits 0 .. 33, zero outside the grid.  A raw row is 32 * pitch bytes: c0 is a multiple of 32, so the two
// 16-byte loads are aligned and end inside the row; what they bring from behind cell gw - 1 was never written and is masked away
__device__ __forceinline__ unsigned long long raw_bits(const uint8_t *raw, const int rp, const int gw, const int gh, const int cy, const int c0) {
    if (cy < 0 || cy >= gh) return 0ull;
    const uint8_t *r = raw + (size_t)cy * rp;
    const uint4 a = *(const uint4 *)(r + c0), b = *(const uint4 *)(r + c0 + 16);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) m |= ((w[j] & 1u) | ((w[j] >> 7) & 2u) | ((w[j] >> 14) & 4u) | ((w[j] >> 21) & 8u)) << (4 * j); // a raw byte is 0 or 1
    if (gw - c0 < 32) m &= (1u << (gw - c0)) - 1u;
    unsigned long long out = (unsigned long long)m << 1;
    if (c0 > 0 && r[c0 - 1]) out |= 1ull;
    if (c0 + 32 < gw && r[c0 + 32]) out |= 1ull << 33;
    return out;
}

__global__ __launch_bounds__(FT_THREADS) void motion_map_kernel(const mhip_motion_t p) {
    __shared__ int acc[5];                    // active, min cx, min cy, max cx, max cy
    __shared__ int zc[MHIP_MOTION_MAX_ZONES];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int gw = p.gw, gh = p.gh, rp = 32 * p.pitch;
    if (tid == 0) { acc[0] = 0; acc[1] = gw; acc[2] = gh; acc[3] = -1; acc[4] = -1; }
    if (tid < MHIP_MOTION_MAX_ZONES) zc[tid] = 0;
    __syncthreads();
    const uint8_t *raw = p.raw + (size_t)f * gh * rp;
    uint32_t *map = p.maps + (size_t)f * gh * p.pitch;
    const int words = gh * p.pitch; // <= 2048 * 64
    for (int i = tid; i < words; i += FT_THREADS) {
        const int cy = i / p.pitch, c0 = (i - cy * p.pitch) << 5;
        const unsigned long long mid = raw_bits(raw, rp, gw, gh, cy, c0);
        uint32_t bits = (uint32_t)(mid >> 1);
        if (p.min_neighbors && bits) { // the three rows' bits are in registers: a raw cell's neighbours are a few popcounts
            const unsigned long long up = raw_bits(raw, rp, gw, gh, cy - 1, c0), dn = raw_bits(raw, rp, gw, gh, cy + 1, c0);
            uint32_t cand = bits;
            bits = 0;
            while (cand) {
                const int c = __ffs(cand) - 1; // cell c0 + c is bit c + 1 of the row masks
                cand &= cand - 1;
                const int nbr = __popcll((up >> c) & 7ull) + __popcll((mid >> c) & 5ull) + __popcll((dn >> c) & 7ull);
                if (nbr >= p.min_neighbors) bits |= 1u << c;
            }
        }
        map[i] = bits; // bits at cx >= gw are zero
        if (bits) {
            atomicAdd(&acc[0], __popc(bits));
            atomicMin(&acc[1], c0 + __ffs(bits) - 1);
            atomicMax(&acc[3], c0 + 31 - __clz(bits));
            atomicMin(&acc[2], cy);
            atomicMax(&acc[4], cy);
            for (int z = 0; z < p.n_zones; z++) {
                const int lo = max(p.zones[z][0], c0), hi = min(p.zones[z][2], c0 + 31); // inclusive
                if (cy < p.zones[z][1] || cy > p.zones[z][3] || hi < lo) continue;
                const uint32_t m = span_mask(lo - c0, hi - c0);
                if (bits & m) atomicAdd(&zc[z], __popc(bits & m));
            }
        }
    }
    __syncthreads();
    const int B = 1 << p.cell_log2;
    if (tid == 0) {
        int *st = p.stats + (size_t)f * 6; // [5], `first`, is the first launch's
        const bool any = acc[0] > 0;
        st[0] = acc[0];
        st[1] = any ? acc[1] * B : 0;
        st[2] = any ? acc[2] * B : 0;
        st[3] = any ? min(p.w, (acc[3] + 1) * B) : 0;
        st[4] = any ? min(p.h, (acc[4] + 1) * B) : 0;
        const int step = p.stream_major ? f % p.steps : f / p.streams;
        if (step == 0) p.init[p.stream_major ? f / p.steps : f % p.streams] = 1;
    }
    if (tid < p.n_zones) p.zone_counts[(size_t)f * p.n_zones + tid] = zc[tid];
}

__global__ __launch_bounds__(FT_THREADS) void motion_dets_kernel(const mhip_motion_dets_t p) {
    const int e = blockIdx.x * FT_THREADS + threadIdx.x;
    if (e >= p.n_entries) return;
    int f, act = 0, cells = 0;
    bool listed;
    if (p.counts) {
        f = e / p.det_cap;
        listed = e - f * p.det_cap < min(max(p.counts[f], 0), p.det_cap);
    } else {
        f = p.frame_of[e];
        listed = f >= 0 && f < p.n_frames;
    }
    int q[4];
    if (listed && roi_rect(((const det_t *)p.dets)[e], p.expand, 1, p.w, p.h, q)) {
        // 0 <= x0 < x1 <= W: the cell range lies inside the grid
        const int bl = p.cell_log2, cx0 = q[0] >> bl, cx1 = (q[2] - 1) >> bl, cy0 = q[1] >> bl, cy1 = (q[3] - 1) >> bl;
        cells = (cx1 - cx0 + 1) * (cy1 - cy0 + 1);
        const uint32_t *map = p.maps + (size_t)f * p.gh * p.pitch;
        for (int cy = cy0; cy <= cy1; cy++)
            for (int wi = cx0 >> 5; wi <= cx1 >> 5; wi++) {
                const int c0 = wi << 5, lo = max(cx0, c0), hi = min(cx1, c0 + 31);
                act += __popc(map[(size_t)cy * p.pitch + wi] & span_mask(lo - c0, hi - c0));
            }
    }
    int *o = (int *)p.out + 2 * (size_t)e;
    o[0] = act; o[1] = cells;
}

static bool motion_ok(const mhip_motion_t *p) {
    if (!p || !p->frames || !p->bg || !p->init || !p->raw || !p->maps || !p->stats) return false;
    if (p->w > MHIP_MOTION_MAX_DIM || p->h > MHIP_MOTION_MAX_DIM || p->cell_log2 < 2 || p->cell_log2 > 6) return false;
    const size_t fb = mhip_frame_bytes(p->w, p->h, p->fmt);
    if (!mhip_frame_format_ok(p->fmt, 0) || !fb || p->frame_stride < fb) return false; // (no NV12 flag matters: only the Y plane is read)
    const int B = 1 << p->cell_log2;
    if (p->gw != (p->w + B - 1) / B || p->gh != (p->h + B - 1) / B || p->pitch != (p->gw + 31) / 32) return false;
    if (p->streams <= 0 || p->streams > 65535 || p->steps <= 0 || (long long)p->streams * p->steps != p->n_frames) return false;
    if (p->threshold < 1 || p->threshold > 255 || p->learn < 1 || p->learn > 16 || p->learn_active < 1 || p->learn_active > 16) return false;
    if (p->min_neighbors < 0 || p->min_neighbors > 8 || p->n_zones < 0 || p->n_zones > MHIP_MOTION_MAX_ZONES || (p->n_zones && !p->zone_counts)) return false;
    for (int z = 0; z < p->n_zones; z++)
        if (p->zones[z][0] < 0 || p->zones[z][1] < 0 || p->zones[z][2] < p->zones[z][0] || p->zones[z][3] < p->zones[z][1] || p->zones[z][2] >= p->gw ||
            p->zones[z][3] >= p->gh)
            return false;
    return true;
}

extern "C" int mhip_motion_cells(const mhip_motion_t *p) {
    if (!motion_ok(p)) return -1;
    const dim3 g((unsigned)((p->w + FT_TILE - 1) / FT_TILE), (unsigned)((p->h + FT_TILE - 1) / FT_TILE), (unsigned)p->streams);
    if (p->fmt == 0) hipLaunchKernelGGL(motion_cells_kernel<3>, g, dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    else hipLaunchKernelGGL(motion_cells_kernel<1>, g, dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "motion cells");
}

extern "C" int mhip_motion_map(const mhip_motion_t *p) {
    if (!motion_ok(p)) return -1;
    hipLaunchKernelGGL(motion_map_kernel, dim3((unsigned)p->n_frames), dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "motion map");
}

extern "C" int mhip_motion_dets(const mhip_motion_dets_t *p) {
    if (!p || !p->maps || !p->dets || !p->out || (!p->counts && !p->frame_of) || (p->counts && p->det_cap <= 0) || p->n_frames <= 0 ||
        p->n_entries <= 0 || p->w <= 0 || p->h <= 0 || p->w > MHIP_MOTION_MAX_DIM || p->h > MHIP_MOTION_MAX_DIM || p->cell_log2 < 2 ||
        p->cell_log2 > 6 || p->gw != ((p->w - 1) >> p->cell_log2) + 1 || p->gh != ((p->h - 1) >> p->cell_log2) + 1 || p->pitch != (p->gw + 31) / 32 ||
        !(p->expand > 0) || (p->counts && (long long)p->n_frames * p->det_cap != p->n_entries))
        return -1;
    hipLaunchKernelGGL(motion_dets_kernel, dim3((unsigned)((p->n_entries + FT_THREADS - 1) / FT_THREADS)), dim3(FT_THREADS), 0, mhip_stream_native(), *p);
    return mhip_check(hipGetLastError(), "motion dets");
}
