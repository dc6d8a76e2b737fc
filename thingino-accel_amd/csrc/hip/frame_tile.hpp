// frame_tile.hpp -- what the kernels that walk camera frames tile by tile share (redact.hip, motion.hip): the tile's shape, the move of a
// tile's rows into LDS, and the mask of a span of bits.  What a kernel does with the staged rows, and its barriers, are its own.
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

// bits lo .. hi (inclusive, 0 <= lo <= hi <= 31) of a 32-bit word
__device__ __forceinline__ uint32_t span_mask(const int lo, const int hi) { return (hi - lo == 31 ? ~0u : (1u << (hi - lo + 1)) - 1u) << lo; }
