// host_delta.cpp -- product: what the delta encoder's diff kernel and pack launch compute, on the host (host_delta.h).
#include "host_delta.h"

#include <cstring>

namespace mpc {

long long changed_tiles(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height, int block,
                        int32_t* tiles) {
    const int tiles_x = (width + block - 1) / block, tiles_y = (height + block - 1) / block;
    long long n = 0;
    for (int tx = 0; tx < tiles_x; ++tx)
        for (int ty = 0; ty < tiles_y; ++ty) {
            const int x0 = tx * block, x1 = x0 + block < width ? x0 + block : width;
            const int y0 = ty * block, y1 = y0 + block < height ? y0 + block : height;
            bool changed = false;
            for (int y = y0; y < y1 && !changed; ++y)
                changed = std::memcmp(prev + static_cast<size_t>(y) * prev_stride + 3 * static_cast<size_t>(x0),
                                      cur + static_cast<size_t>(y) * cur_stride + 3 * static_cast<size_t>(x0), 3 * static_cast<size_t>(x1 - x0)) != 0;
            if (changed) tiles[n++] = static_cast<int32_t>(static_cast<long long>(tx) * tiles_y + ty);
        }
    return n;
}

long long changed_tiles_tolerance(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height, int block,
                                  uint32_t tolerance, int32_t* tiles, uint32_t* sse) {
    const int tiles_x = (width + block - 1) / block, tiles_y = (height + block - 1) / block;
    long long n = 0;
    for (int tx = 0; tx < tiles_x; ++tx)
        for (int ty = 0; ty < tiles_y; ++ty) {
            const int x0 = tx * block, x1 = x0 + block < width ? x0 + block : width;
            const int y0 = ty * block, y1 = y0 + block < height ? y0 + block : height;
            uint32_t sum = 0;                                       // at most 64 * 3 * 255^2
            for (int y = y0; y < y1; ++y) {
                const uint8_t* p = prev + static_cast<size_t>(y) * prev_stride + 3 * static_cast<size_t>(x0);
                const uint8_t* q = cur + static_cast<size_t>(y) * cur_stride + 3 * static_cast<size_t>(x0);
                for (int b = 0; b < 3 * (x1 - x0); ++b) {
                    const int diff = static_cast<int>(q[b]) - static_cast<int>(p[b]);
                    sum += static_cast<uint32_t>(diff * diff);
                }
            }
            const long long t = static_cast<long long>(tx) * tiles_y + ty;
            if (sse) sse[t] = sum;
            if (sum > tolerance) tiles[n++] = static_cast<int32_t>(t);
        }
    return n;
}

PackGeometry pack_geometry(long long n, int max_rows) {
    PackGeometry g{0, 0, 0, 0};
    if (n < 1) return g;
    g.rows = static_cast<int>(n < max_rows ? n : max_rows);
    g.cols = static_cast<int>((n + g.rows - 1) / g.rows);
    g.stride = 24 * static_cast<size_t>(g.cols);
    g.bytes = g.stride * 8 * static_cast<size_t>(g.rows);
    return g;
}

}  // namespace mpc
