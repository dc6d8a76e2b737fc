// frame_tile.hpp -- what the kernels that walk camera frames tile by tile share (redact.hip, motion.hip, overlay.hip): the tile's shape, the move of a
// tile's rows into LDS and, for the kernels that write frames, back, and the mask of a span of bits.  What a kernel does with the staged rows, and its barriers, are its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FT_TILE 64     // pixels per tile side: cell-aligned for every cell size that is a power of two up to 64
#define FT_THREADS 256 // four threads on a row
#define FT_PITCH 208   // LDS bytes per staged row
static_assert(FT_THREADS == 4 * FT_TILE && FT_PITCH % 16 == 0 && FT_PITCH >= FT_TILE * 3 + 3,
              "a staged row: 64 x 3 bytes + the shift of at most 3, at a multiple of 16 so that the 16-byte moves are aligned");

// The tile's rows -> LDS.  Called by every thread: thread t is one of the four on row t >> 2.  `rows` rows of nb bytes, `pitch` bytes apart
// from src on; row r lands at pix + r * FT_PITCH + its shift, and the thread gets its row's shift back (0 without a row).  wide is the caller's
// block-uniform decision that src, pitch and nb are multiples of 16 (and whatever else it moves the same way): the row goes as 16-byte units,
// unshifted.  Else it goes as bytes up to the first 4-byte boundary, 4-byte units and bytes behind the last one, its LDS copy shifted by the
// row's address & 3, so both sides of every 4-byte move are aligned.  Nothing is read behind a row's last byte.  No barrier: the caller's.
__device__ __forceinline__ int tile_rows_to_lds(const uint8_t *src, const size_t pitch, const int nb, const int rows, uint8_t *pix, const bool wide) {
    const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
    if (row >= rows) return 0;
    const uint8_t *g = src + (size_t)row * pitch;
    if (wide) {
        uint8_t *l = pix + row * FT_PITCH;
        for (int j = sub; j < (nb >> 4); j += 4) *(uint4 *)(l + 16 * j) = *(const uint4 *)(g + 16 * j);
        return 0;
    }
    const int sh = (int)((uintptr_t)g & 3), head = min(nb, (4 - sh) & 3), nd = (nb - head) >> 2;
    uint8_t *l = pix + row * FT_PITCH + sh;
    if (sub == 0)
        for (int k = 0; k < head; k++) l[k] = g[k];
    for (int j = sub; j < nd; j += 4) *(uint32_t *)(l + head + 4 * j) = *(const uint32_t *)(g + head + 4 * j);
    if (sub == 3)
        for (int k = head + 4 * nd; k < nb; k++) l[k] = g[k];
    return sh;
}

// LDS -> the destination, the way back.  Called by every thread behind the caller's barrier: thread t is one of the four on row t >> 2.  The
// staged rows are those tile_rows_to_lds(src, pitch, nb, rows, pix, wide) left (src gives every row's shift); row r goes to dst + r * pitch.
// C = bytes per sample, bit x of cov[r] = sample (x, r) has changed.  Out of place every unit is stored; in place only the units that hold a
// changed sample.  wide must also cover dst (both sides multiples of 16): 16-byte units; else, where src and dst agree in their low two
// address bits, bytes up to the first 4-byte boundary, 4-byte units and bytes behind the last one; else bytes.  No store reaches over a row's
// ends.  All plain vector stores.  No barrier: the caller's.
template <int C>
__device__ __forceinline__ void tile_rows_from_lds(const uint8_t *src, uint8_t *dst, const size_t pitch, const int nb, const int rows, const uint8_t *pix,
                                                   const bool wide, const unsigned long long *cov, const bool inplace) {
    const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
    if (row >= rows) return;
    const bool same4 = !(((uintptr_t)src ^ (uintptr_t)dst) & 3);
    const unsigned long long cr = cov[row];
    const auto want = [&](const int b0, const int b1) { // bytes b0 .. b1 of the row hold a changed sample
        if (!inplace) return true;
        const int s0 = b0 / C, s1 = b1 / C;
        return ((cr >> s0) & ((2ull << (s1 - s0)) - 1ull)) != 0ull;
    };
    uint8_t *g = dst + (size_t)row * pitch;
    const int sh = (int)((uintptr_t)(src + (size_t)row * pitch) & 3);
    const uint8_t *l = pix + row * FT_PITCH + sh;
    if (inplace && !cr) {
        // nothing of this row changes
    } else if (wide) {
        for (int j = sub; j < (nb >> 4); j += 4)
            if (want(16 * j, 16 * j + 15)) *(uint4 *)(g + 16 * j) = *(const uint4 *)(l + 16 * j);
    } else if (same4) {
        const int head = min(nb, (4 - sh) & 3), nd = (nb - head) >> 2;
        if (sub == 0)
            for (int k = 0; k < head; k++)
                if (want(k, k)) g[k] = l[k];
        for (int j = sub; j < nd; j += 4)
            if (want(head + 4 * j, head + 4 * j + 3)) *(uint32_t *)(g + head + 4 * j) = *(const uint32_t *)(l + head + 4 * j);
        if (sub == 3)
            for (int k = head + 4 * nd; k < nb; k++)
                if (want(k, k)) g[k] = l[k];
    } else { // the two buffers differ in their alignment: bytes
        for (int k = sub; k < nb; k += 4)
            if (want(k, k)) g[k] = l[k];
    }
}

// bits lo .. hi (inclusive, 0 <= lo <= hi <= 31) of a 32-bit word
__device__ __forceinline__ uint32_t span_mask(const int lo, const int hi) { return (hi - lo == 31 ? ~0u : (1u << (hi - lo + 1)) - 1u) << lo; }
