// asan_delta.cpp -- the delta encoder's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-delta` /
// tests/test_asan_delta.py.  mpc::changed_tiles -- the definition of what the diff kernel computes -- and mpc::pack_geometry on
// exact-size buffers (one byte read past an end, or a padding byte between rows, is a report or a wrong list): the shapes of
// tests/delta_cases.py and the extreme ones -- 1x1, a width that is no multiple of 8 with the minimum stride, n = 0.
#include "../../imageexperiments_amd/csrc/host_delta.cpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

// a frame of exactly (height - 1) * stride + 3 * width bytes on the heap: the last row has no padding to read
struct Frame {
    int width, height;
    size_t stride;
    uint8_t* bytes;
    Frame(int w, int h, size_t s, std::mt19937& rng) : width(w), height(h), stride(s) {
        const size_t n = static_cast<size_t>(h - 1) * s + 3 * static_cast<size_t>(w);
        bytes = static_cast<uint8_t*>(std::malloc(n));
        for (size_t i = 0; i < n; ++i) bytes[i] = static_cast<uint8_t>(rng());
    }
    Frame(const Frame&) = delete;
    ~Frame() { std::free(bytes); }
    uint8_t* pixel(int x, int y) { return bytes + static_cast<size_t>(y) * stride + 3 * static_cast<size_t>(x); }
};

static void copy_pixels(Frame& to, Frame& from) {
    for (int y = 0; y < to.height; ++y)
        for (int x = 0; x < 3 * to.width; ++x) to.pixel(0, y)[x] = from.pixel(0, y)[x];
}

static int g_cases = 0;

static void diff_case(int w, int h, size_t extra_prev, size_t extra_cur, int block, std::mt19937& rng) {
    ++g_cases;
    Frame prev(w, h, 3 * static_cast<size_t>(w) + extra_prev, rng), cur(w, h, 3 * static_cast<size_t>(w) + extra_cur, rng);
    copy_pixels(cur, prev);                                         // the padding still differs
    const int tiles_x = (w + block - 1) / block, tiles_y = (h + block - 1) / block;
    std::vector<int32_t> list(static_cast<size_t>(tiles_x) * tiles_y);
    CHECK(mpc::changed_tiles(prev.bytes, prev.stride, cur.bytes, cur.stride, w, h, block, list.data()) == 0);
    // a few pixels moved: exactly their tiles, ascending
    std::vector<char> want(list.size(), 0);
    const int moves = 1 + static_cast<int>(rng() % 5);
    for (int m = 0; m < moves; ++m) {
        const int x = m == 0 ? w - 1 : static_cast<int>(rng() % w), y = m == 0 ? h - 1 : static_cast<int>(rng() % h);
        cur.pixel(x, y)[rng() % 3] ^= 1 + rng() % 255;
        want[static_cast<size_t>(x / block) * tiles_y + y / block] = 1;
    }
    std::vector<char> truth(list.size(), 0);                        // byte by byte (two moves may undo each other)
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < 3 * w; ++x)
            if (prev.pixel(0, y)[x] != cur.pixel(0, y)[x]) truth[static_cast<size_t>(x / 3 / block) * tiles_y + y / block] = 1;
    const long long n = mpc::changed_tiles(prev.bytes, prev.stride, cur.bytes, cur.stride, w, h, block, list.data());
    long long expect = 0;
    for (size_t t = 0; t < truth.size(); ++t) {
        CHECK(!truth[t] || want[t]);
        if (truth[t]) {
            CHECK(expect < n && list[static_cast<size_t>(expect)] == static_cast<int32_t>(t));
            ++expect;
        }
    }
    CHECK(n == expect);
}

static void geometry_cases() {
    const mpc::PackGeometry none = mpc::pack_geometry(0, mpc::kDeltaPackRows);
    CHECK(none.rows == 0 && none.cols == 0 && none.stride == 0 && none.bytes == 0);
    for (int rows : {1, 3, 64, 1000})
        for (long long n : {1LL, 2LL, 3LL, 4LL, 63LL, 64LL, 65LL, 424LL, 425LL, 251328LL, (1LL << 31) - 1}) {
            ++g_cases;
            const mpc::PackGeometry g = mpc::pack_geometry(n, rows);
            CHECK(g.rows == (n < rows ? n : rows) && g.rows >= 1);
            CHECK(static_cast<long long>(g.rows) * g.cols >= n && static_cast<long long>(g.rows) * (g.cols - 1) < n);
            CHECK(g.stride == 24 * static_cast<size_t>(g.cols) && g.stride % 8 == 0 && g.bytes == g.stride * 8 * static_cast<size_t>(g.rows));
            // listed tile j at (j / rows, j % rows): the tile encoder's own order over the packed frame is j
            for (long long j : {0LL, n / 2, n - 1}) CHECK((j / g.rows) * g.rows + j % g.rows == j && j / g.rows < g.cols);
        }
    const mpc::PackGeometry g = mpc::pack_geometry(424, 64);
    CHECK(g.rows == 64 && g.cols == 7 && g.stride == 168);
}

int main() {
    std::mt19937 rng(20240611);
    const int shapes[][2] = {{83, 45}, {8, 8}, {5, 3}, {16, 16}, {200, 136}, {1, 1}, {1, 9}, {9, 1}, {13, 8}, {7, 7}, {17, 23}};
    for (const auto& s : shapes)
        for (size_t extra_prev : {size_t{0}, size_t{5}})
            for (size_t extra_cur : {size_t{0}, size_t{5}, size_t{13}})     // 0: the minimum stride, rows back to back
                for (int block : {8, 1, 3, 5})
                    for (int round = 0; round < 3; ++round) diff_case(s[0], s[1], extra_prev, extra_cur, block, rng);
    geometry_cases();
    std::printf("asan_delta: %d cases\n", g_cases);
    std::printf("asan_delta: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
