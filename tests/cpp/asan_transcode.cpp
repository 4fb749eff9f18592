// asan_transcode.cpp -- the transcode's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-transcode` /
// tests/test_asan_transcode.py.  mpc::transcode_container -- the definition of what mpc_transcode_views_indexed computes -- and
// mpc::transcode_rect_error on what nobody vouches for: damaged containers, views of every kind.  Beside every sanitizer report the
// rules are checked: the verdict is read_compressed's, then "a length above K"; the whole frame with steps 0 is what coding the
// parsed container again gives; the whole frame with steps m is truncate_container(m); a rectangle of a rectangle is the rectangle
// of the source, and cutting steps commutes with cropping.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <string>

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

static std::vector<uint8_t> random_container(std::mt19937& rng, int W, int H, int K, int bs) {
    const size_t tiles = static_cast<size_t>((W + bs - 1) / bs) * ((H + bs - 1) / bs);
    std::vector<uint16_t> counts(3 * tiles);
    std::vector<uint32_t> choices(3 * tiles * K, 0);
    for (size_t o = 0; o < 3 * tiles; ++o) {
        counts[o] = static_cast<uint16_t>(rng() % (K + 1));
        for (int i = 0; i < counts[o]; ++i)                         // few distinct ids in the chroma channels: run-length packed streams
            choices[o * K + i] = (rng() % (o % 3 == 0 ? 2500 : 3)) | ((rng() % (i == 0 ? 4000 : 60)) << 16);
    }
    std::vector<double> quant(3 * static_cast<size_t>(K), 7.0);
    size_t n = 0;
    uint8_t* b = mpc::encode_records_malloc(W, H, K, bs, quant.data(), counts.data(), choices.data(), &n);
    CHECK(b);
    const std::vector<uint8_t> blob(b, b + (b ? n : 0));
    std::free(b);
    return blob;
}

struct View { int x, y, w, h, steps; };                             // (0, 0, 0, 0): the whole frame

// the C entry's order on an exact-size copy (one byte read past its end is a report): -1 = an argument error, else
// transcode_container's verdict.  The verdict's rules are checked here
static int transcode(const std::vector<uint8_t>& x, View v, std::vector<uint8_t>& out) {
    const std::vector<uint8_t> xc(x.begin(), x.end());
    out.clear();
    if (v.steps < 0) return -1;
    int width, height, K, bs;
    if (!mpc::container_info(xc.data(), xc.size(), &width, &height, &K, &bs)) {
        mpc::Streams s;
        CHECK(!mpc::read_compressed(xc.data(), xc.size(), s));
        return 1;
    }
    if (v.x == 0 && v.y == 0 && v.w == 0 && v.h == 0) v = View{0, 0, width, height, v.steps};
    if (!mpc::transcode_rect_error(width, height, bs, v.x, v.y, v.w, v.h).empty()) return -1;
    const int verdict = mpc::transcode_container(xc.data(), xc.size(), v.x, v.y, v.w, v.h, v.steps, out);
    mpc::Streams s;
    const bool readable = mpc::read_compressed(xc.data(), xc.size(), s);
    CHECK((verdict == 1) == !readable);
    CHECK(verdict != 3);                                            // the rectangle was checked against the same header
    if (readable) {
        bool too_long = false;
        for (uint16_t length : s.lengths) too_long = too_long || length > s.K;
        CHECK((verdict == 2) == too_long);
    }
    if (verdict != 0) {
        CHECK(out.empty());
        return verdict;
    }
    mpc::Streams made;
    CHECK(mpc::read_compressed(out.data(), out.size(), made));
    CHECK(made.width == v.w && made.height == v.h && made.K == s.K && made.block_size == s.block_size);
    CHECK(std::memcmp(made.quant, s.quant, sizeof(s.quant)) == 0);
    const int m = v.steps > 0 && v.steps < s.K ? v.steps : s.K;
    for (uint16_t length : made.lengths) CHECK(length <= m);
    return 0;
}

// the identities of one container; exact: an encoder's container (its step-0 sums survive the difference coder)
static void identities(std::mt19937& rng, const std::vector<uint8_t>& x, bool encoders) {
    int width, height, K, bs;
    std::vector<uint8_t> whole;
    if (transcode(x, View{0, 0, 0, 0, 0}, whole) != 0) return;
    CHECK(mpc::container_info(x.data(), x.size(), &width, &height, &K, &bs));
    std::vector<uint8_t> again, other;
    CHECK(mpc::truncate_container(x.data(), x.size(), K, again) && again == whole);
    if (encoders) CHECK(whole == x);
    CHECK(transcode(x, View{0, 0, width, height, K + 2}, other) == 0 && other == whole);
    for (int m : {1, (K + 1) / 2, K}) {
        std::vector<uint8_t> cut, got;
        CHECK(mpc::truncate_container(x.data(), x.size(), m, cut));
        CHECK(transcode(x, View{0, 0, 0, 0, m}, got) == 0 && got == cut);
    }
    if (!encoders) return;                                          // composition needs sums that survive a second difference coding
    const int tx = (width + bs - 1) / bs, ty = (height + bs - 1) / bs;
    for (int k = 0; k < 6; ++k) {
        // an outer grid, and an inner grid inside it; a grid that ends at the frame's last tile ends at the frame's edge
        const int ox0 = static_cast<int>(rng() % tx), ox1 = ox0 + 1 + static_cast<int>(rng() % (tx - ox0));
        const int oy0 = static_cast<int>(rng() % ty), oy1 = oy0 + 1 + static_cast<int>(rng() % (ty - oy0));
        const int ix0 = ox0 + static_cast<int>(rng() % (ox1 - ox0)), ix1 = ix0 + 1 + static_cast<int>(rng() % (ox1 - ix0));
        const int iy0 = oy0 + static_cast<int>(rng() % (oy1 - oy0)), iy1 = iy0 + 1 + static_cast<int>(rng() % (oy1 - iy0));
        auto rect = [&](int x0, int x1, int y0, int y1, int steps) {
            return View{x0 * bs, y0 * bs, std::min(x1 * bs, width) - x0 * bs, std::min(y1 * bs, height) - y0 * bs, steps};
        };
        const int m = static_cast<int>(rng() % (K + 1));
        std::vector<uint8_t> outer, direct, nested, cut_first, cut_last;
        CHECK(transcode(x, rect(ox0, ox1, oy0, oy1, 0), outer) == 0);
        CHECK(transcode(x, rect(ix0, ix1, iy0, iy1, m), direct) == 0);
        View inner = rect(ix0, ix1, iy0, iy1, m);
        inner.x -= ox0 * bs;
        inner.y -= oy0 * bs;
        CHECK(transcode(outer, inner, nested) == 0 && nested == direct);
        CHECK(transcode(x, rect(ox0, ox1, oy0, oy1, m), cut_first) == 0);
        inner.steps = 0;
        CHECK(transcode(cut_first, inner, cut_last) == 0 && cut_last == direct);
    }
}

static std::vector<View> views_of(std::mt19937& rng, int W, int H, int K, int bs) {
    const int tx = (W + bs - 1) / bs, ty = (H + bs - 1) / bs, lx = (tx - 1) * bs, ly = (ty - 1) * bs;
    std::vector<View> out = {{0, 0, 0, 0, 0}, {0, 0, W, H, 1}, {0, 0, std::min(bs, W), std::min(bs, H), K}, {lx, ly, W - lx, H - ly, K + 3},
                             {lx, 0, W - lx, H, (K + 1) / 2}, {0, ly, W, H - ly, 2},
                             // argument errors: unaligned, a ragged edge that is not the frame's, empty, outside, overflowing, steps < 0
                             {1, 0, bs, bs, 0}, {0, 1, bs, bs, 0}, {0, 0, bs + 1, bs, 0}, {0, 0, bs, bs + 1, 0}, {0, 0, 0, bs, 1}, {0, bs, 0, 0, 1},
                             {-bs, 0, 2 * bs, bs, 1}, {0, 0, W + bs, bs, 1}, {W, H, 1, 1, 0}, {bs, bs, 2147483647, bs, 2}, {2147483640, 0, 16, 8, 2},
                             {0, 0, W, H, -1}};
    for (int k = 0; k < 4; ++k) {
        const int x0 = static_cast<int>(rng() % tx), y0 = static_cast<int>(rng() % ty);
        const int x1 = x0 + 1 + static_cast<int>(rng() % (tx - x0)), y1 = y0 + 1 + static_cast<int>(rng() % (ty - y0));
        out.push_back({x0 * bs, y0 * bs, std::min(x1 * bs, W) - x0 * bs, std::min(y1 * bs, H) - y0 * bs, static_cast<int>(rng() % (K + 2))});
    }
    return out;
}

static void drive(std::mt19937& rng, const std::vector<uint8_t>& blob, int W, int H, int K, int bs, int flips) {
    const std::vector<View> views = views_of(rng, W, H, K, bs);
    for (size_t k = 0; k < views.size(); ++k) {
        std::vector<uint8_t> out;
        CHECK(transcode(blob, views[k], out) == (k >= 6 && k < 18 ? -1 : 0));      // views 6 - 17 are refused as arguments
    }
    identities(rng, blob, true);
    for (int k = 0; k < flips; ++k) {                               // damaged containers
        std::vector<uint8_t> x = blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * (k % 4 == 0 ? std::min<size_t>(x.size(), 14 + 6 * static_cast<size_t>(K)) : x.size()));
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        std::vector<uint8_t> out;
        transcode(x, views[k % views.size()], out);
        transcode(x, View{0, 0, 0, 0, static_cast<int>(rng() % (K + 1))}, out);
        identities(rng, x, false);
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20261019);
    const int shapes[][4] = {{8, 8, 1, 8}, {64, 40, 4, 8}, {203, 117, 8, 8}, {120, 64, 32, 8}, {30, 22, 5, 4}, {13, 9, 3, 2}, {50, 33, 2, 7}};
    for (const auto& s : shapes) drive(rng, random_container(rng, s[0], s[1], s[2], s[3]), s[0], s[1], s[2], s[3], 24);
    if (argc > 1) {                 // written by tests/test_asan_transcode.py: <dir>/<n>.mn, <dir>/<n>.view ("x y w h steps")
        auto slurp = [](const std::string& path, std::vector<uint8_t>& out) {
            std::ifstream f(path, std::ios::binary);
            if (!f) return false;
            out.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            return true;
        };
        int pairs = 0, made = 0;
        for (;; ++pairs) {
            std::vector<uint8_t> x, out;
            const std::string stem = std::string(argv[1]) + "/" + std::to_string(pairs);
            std::ifstream vf(stem + ".view");
            View v{};
            if (!slurp(stem + ".mn", x) || !(vf >> v.x >> v.y >> v.w >> v.h >> v.steps)) break;
            made += transcode(x, v, out) == 0;
            identities(rng, x, false);
        }
        std::printf("asan_transcode: %d pairs from files, %d transcoded\n", pairs, made);
    }
    std::printf("asan_transcode: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
