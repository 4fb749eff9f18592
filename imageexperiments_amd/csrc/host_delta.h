// host_delta.h -- product: the host's definition of the delta encoder's device steps (include/mpcodec.h, "delta").  Knows neither HIP
// nor the C ABI and builds on its own (tests/cpp/asan_delta.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mpc {

constexpr int kDeltaPackRows = 64;      // MPC_DELTA_PACK_ROWS

// Tile t = tx * tiles_y + ty of a width x height frame cut into block x block tiles is CHANGED iff any of the three bytes of any pixel
// (x, y) of it with x < width and y < height differs between `prev` and `cur`; pixel (x, y) is the 3 bytes at base + y * stride + 3 * x.
// Only pixel bytes are read: of the last row 3 * width bytes, of the bytes between a row's end and the next row none.  Bytes are
// compared; no tile is computed.  tiles[ceil(width / block) * ceil(height / block)] receives the changed tiles in ascending order,
// the return value is their number.  The caller has checked: non-null pointers, width, height, block >= 1, strides >= 3 * width.
long long changed_tiles(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height, int block,
                        int32_t* tiles);

// The same with a tolerance: sse(t) = the sum of (cur - prev)^2 over the same bytes, exact in 32 bits (at most 64 * 3 * 255^2 =
// 12 484 800); tile t is CHANGED iff sse(t) > tolerance, HELD iff 0 < sse(t) <= tolerance.  tolerance 0 is changed_tiles.  sse: NULL or
// one value per tile, every tile's.  `prev` is not written: the composite the delta encoder keeps is `cur` in the listed tiles and
// `prev` in every other.  Same reads, same caller's checks.
long long changed_tiles_tolerance(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height, int block,
                                  uint32_t tolerance, int32_t* tiles, uint32_t* sse);

// The packed frame of n listed tiles: rows x cols whole 8 x 8 tiles, listed tile j at (tx', ty') = (j / rows, j % rows), so that the
// tile encoder's own order tx' * rows + ty' over the packed frame is j.  rows = min(n, max_rows), cols = ceil(n / rows), stride =
// 24 * cols bytes between pixel rows (a multiple of 8), bytes = stride * 8 * rows.  n = 0: all zero.  The caller has checked n >= 0
// and max_rows >= 1.
struct PackGeometry {
    int rows, cols;
    size_t stride, bytes;
};
PackGeometry pack_geometry(long long n, int max_rows);

}  // namespace mpc
