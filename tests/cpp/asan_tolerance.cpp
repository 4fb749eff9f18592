// asan_tolerance.cpp -- the delta encoder's change tolerance on the host under AddressSanitizer + UBSan (g++, no GPU, no HIP):
// `make asan-tolerance` / tests/test_asan_tolerance.py.  mpc::changed_tiles_tolerance -- the definition of what mp_tile_diff_tol_kernel
// computes -- on exact-size heap buffers: widths 1 to 1041, the last row ending with the buffer, odd bases, padded rows whose padding
// differs, the extreme tolerances.  One byte read past an end, or a padding byte counted, is a report or a wrong sum.
#include "../../imageexperiments_amd/csrc/host_delta.cpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

// a frame of exactly lead + (height - 1) * stride + 3 * width bytes on the heap, its first pixel `lead` bytes in: the last row has no
// padding to read, and an odd lead gives an odd base
struct Frame {
    int width, height;
    size_t stride, lead;
    uint8_t* block;
    Frame(int w, int h, size_t s, size_t l, std::mt19937& rng) : width(w), height(h), stride(s), lead(l) {
        const size_t n = l + static_cast<size_t>(h - 1) * s + 3 * static_cast<size_t>(w);
        block = static_cast<uint8_t*>(std::malloc(n));
        for (size_t i = 0; i < n; ++i) block[i] = static_cast<uint8_t>(rng());
    }
    Frame(const Frame&) = delete;
    ~Frame() { std::free(block); }
    uint8_t* base() { return block + lead; }
    uint8_t* row(int y) { return base() + static_cast<size_t>(y) * stride; }
};

static void tolerance_case(int w, int h, size_t extra_prev, size_t extra_cur, size_t lead, int block, int mode, std::mt19937& rng) {
    ++g_cases;
    Frame prev(w, h, 3 * static_cast<size_t>(w) + extra_prev, lead, rng), cur(w, h, 3 * static_cast<size_t>(w) + extra_cur, lead ? lead + 2 : 0, rng);
    // mode 0: random against random; 1: 0 against 255 everywhere; 2: equal pixels but a few bytes moved by a little
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < 3 * w; ++x) {
            if (mode == 1) {
                prev.row(y)[x] = 0;
                cur.row(y)[x] = 255;
            } else if (mode == 2) {
                cur.row(y)[x] = prev.row(y)[x];
            }
        }
    if (mode == 2)
        for (int m = 0; m < 6; ++m) {
            const int x = m == 0 ? 3 * w - 1 : static_cast<int>(rng() % (3 * w)), y = m == 0 ? h - 1 : static_cast<int>(rng() % h);
            cur.row(y)[x] = static_cast<uint8_t>(cur.row(y)[x] + 1 + rng() % 3);
        }
    const int tiles_x = (w + block - 1) / block, tiles_y = (h + block - 1) / block;
    const size_t tiles = static_cast<size_t>(tiles_x) * tiles_y;
    std::vector<uint64_t> truth(tiles, 0);                          // byte by byte, in 64 bits
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < 3 * w; ++x) {
            const long long diff = static_cast<long long>(cur.row(y)[x]) - prev.row(y)[x];
            truth[static_cast<size_t>(x / 3 / block) * tiles_y + y / block] += static_cast<uint64_t>(diff * diff);
        }
    uint64_t largest = 0;
    for (uint64_t v : truth) largest = v > largest ? v : largest;
    CHECK(largest <= 12484800u);
    // exact-size outputs: one list entry per tile, one sum per tile
    int32_t* list = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * tiles));
    uint32_t* sse = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * tiles));
    const uint32_t some = static_cast<uint32_t>(truth[rng() % tiles]);
    for (uint32_t tolerance : {0u, 1u, some, some ? some - 1 : 0u, static_cast<uint32_t>(largest), 12484799u, 12484800u, 0xffffffffu}) {
        for (bool with_sse : {true, false}) {
            const long long n = mpc::changed_tiles_tolerance(prev.base(), prev.stride, cur.base(), cur.stride, w, h, block, tolerance, list,
                                                             with_sse ? sse : nullptr);
            long long expect = 0;
            for (size_t t = 0; t < tiles; ++t) {
                if (with_sse) CHECK(sse[t] == truth[t]);
                if (truth[t] > tolerance) {
                    CHECK(expect < n && list[expect] == static_cast<int32_t>(t));
                    ++expect;
                }
            }
            CHECK(n == expect);
            if (tolerance >= largest) CHECK(n == 0);
        }
        if (tolerance == 0) {                                       // today's rule exactly
            std::vector<int32_t> plain(tiles);
            const long long n0 = mpc::changed_tiles(prev.base(), prev.stride, cur.base(), cur.stride, w, h, block, plain.data());
            const long long n1 = mpc::changed_tiles_tolerance(prev.base(), prev.stride, cur.base(), cur.stride, w, h, block, 0, list, nullptr);
            CHECK(n0 == n1);
            for (long long j = 0; j < n0 && j < n1; ++j) CHECK(plain[static_cast<size_t>(j)] == list[j]);
        }
    }
    std::free(list);
    std::free(sse);
}

int main() {
    std::mt19937 rng(20241021);
    // every width from 1 to 1041 once, at a small height that is no multiple of 8, cycling through the layouts
    for (int w = 1; w <= 1041; ++w) {
        const size_t extras[] = {0, 5, 13, 8};
        tolerance_case(w, 1 + w % 11, extras[w % 4], extras[(w / 4) % 4], w % 3 == 0 ? 1 : w % 3 == 1 ? 0 : 3, 8, w % 3, rng);
    }
    const int shapes[][2] = {{8, 8}, {5, 3}, {531, 29}, {528, 32}, {1040, 72}, {1, 1}, {1, 9}, {9, 1}, {17, 23}};
    for (const auto& s : shapes)
        for (size_t extra : {size_t{0}, size_t{5}, size_t{8}})
            for (size_t lead : {size_t{0}, size_t{1}})
                for (int block : {8, 1, 5})
                    for (int mode = 0; mode < 3; ++mode) tolerance_case(s[0], s[1], extra, extra ? 0 : 5, lead, block, mode, rng);
    std::printf("asan_tolerance: %d cases\n", g_cases);
    std::printf("asan_tolerance: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
