// asan_region.cpp -- the windowed parse's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-region` /
// tests/test_asan_region.py.  mpc::read_window_by_index -- the definition of what the region decoder's device route computes -- on
// what nobody vouches for: good containers with damaged indexes, damaged containers with a good index, rectangles of every kind.
// Beside every sanitizer report the rules are checked: with "parse all" the result is the serial route's whatever the index holds;
// without, a refused index gives the serial route's result and anything else at least answers.
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

static std::vector<uint8_t> random_container(std::mt19937& rng, int W, int H, int K) {
    const size_t tiles = static_cast<size_t>((W + 7) / 8) * ((H + 7) / 8);
    std::vector<uint16_t> counts(3 * tiles);
    std::vector<uint32_t> choices(3 * tiles * K, 0);
    for (size_t o = 0; o < 3 * tiles; ++o) {
        counts[o] = static_cast<uint16_t>(rng() % (K + 1));
        for (int i = 0; i < counts[o]; ++i)                         // few distinct ids in the chroma channels: run-length packed streams
            choices[o * K + i] = (rng() % (o % 3 == 0 ? 2500 : 3)) | ((rng() % (i == 0 ? 4000 : 60)) << 16);
    }
    std::vector<double> quant(3 * static_cast<size_t>(K), 1.0);
    size_t n = 0;
    uint8_t* b = mpc::encode_records_malloc(W, H, K, 8, quant.data(), counts.data(), choices.data(), &n);
    CHECK(b);
    const std::vector<uint8_t> blob(b, b + (b ? n : 0));
    std::free(b);
    return blob;
}

struct Rect { int x, y, w, h; };

// container x with index `index`, rectangle r, both flags; returns the route without "parse all" (-1: no answer)
static int with_index(const std::vector<uint8_t>& x, const std::vector<uint8_t>& index, const Rect& r) {
    // exact-size copies: one byte read past either end is a report
    const std::vector<uint8_t> xc(x.begin(), x.end()), ic(index.begin(), index.end());
    std::vector<uint16_t> serial, all, cut;
    std::vector<uint64_t> serial_ranges, all_ranges, cut_ranges;
    int serial_route = -1, all_route = -1, cut_route = -1;
    const int want = mpc::read_window_by_index(xc.data(), xc.size(), nullptr, 0, r.x, r.y, r.w, r.h, false, serial, serial_ranges, &serial_route);
    CHECK(want != 0 || serial_route == 1);
    const int got_all = mpc::read_window_by_index(xc.data(), xc.size(), ic.data(), ic.size(), r.x, r.y, r.w, r.h, true, all, all_ranges, &all_route);
    CHECK(got_all == want);
    if (want == 0 && got_all == 0) CHECK(all == serial && all_ranges == serial_ranges && (all_route == 0 || all_route == 1));
    const int got_cut = mpc::read_window_by_index(xc.data(), xc.size(), ic.data(), ic.size(), r.x, r.y, r.w, r.h, false, cut, cut_ranges, &cut_route);
    // Chunks outside the window are not read: damage there goes unseen, so a container the serial route refuses may still answer.
    // What does not answer has the serial route's verdict, and so has every refusal of the index.
    CHECK((got_cut == 2) == (want == 2));
    CHECK(got_cut == 0 || got_cut == want);
    if (got_cut == 0) {
        CHECK(cut_route == 0 || cut_route == 1);
        if (got_all == 0) CHECK(cut_route <= all_route);            // parsing every chunk refuses whatever parsing some of them refuses
        if (cut_route == 1) CHECK(want == 0 && cut == serial && cut_ranges == serial_ranges);
    }
    return want == 0 ? cut_route : -1;
}

static std::vector<Rect> rects_of(std::mt19937& rng, int W, int H) {
    std::vector<Rect> out = {{0, 0, W, H}, {0, 0, 1, 1}, {W - 1, H - 1, 1, 1}, {W / 2, 0, 1, H}, {0, H / 2, W, 1},
                             {-1, 0, 2, 2}, {0, 0, W + 1, 1}, {0, 0, 0, 0}, {W, H, 1, 1}, {2147483647, 0, 2, 2}};
    for (int k = 0; k < 4; ++k) {
        const int x = static_cast<int>(rng() % W), y = static_cast<int>(rng() % H);
        out.push_back({x, y, 1 + static_cast<int>(rng() % (W - x)), 1 + static_cast<int>(rng() % (H - y))});
    }
    return out;
}

static void drive(std::mt19937& rng, const std::vector<uint8_t>& blob, const std::vector<uint8_t>& twin, int W, int H, uint32_t interval,
                  int flips) {
    std::vector<uint8_t> index;
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, index));
    const std::vector<Rect> rects = rects_of(rng, W, H);
    for (size_t k = 0; k < rects.size(); ++k) {
        const int route = with_index(blob, index, rects[k]);
        CHECK(route == (k < 5 || k >= 10 ? 0 : -1));                // the good index is used; rectangles 5 - 9 are refused as arguments
    }
    if (!twin.empty()) {
        std::vector<uint8_t> other;
        CHECK(mpc::build_container_index(twin.data(), twin.size(), interval, other));
        CHECK(with_index(blob, other, rects[10]) == 1);
    }
    int refused = 0;
    for (int k = 0; k < flips; ++k) {                               // damaged indexes
        std::vector<uint8_t> bad = index;
        const size_t bit = rng() % (8 * (k % 4 == 0 ? std::min<size_t>(bad.size(), 56) : bad.size()));
        bad[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        refused += with_index(blob, bad, rects[10 + k % 4]);
    }
    CHECK(refused > 0);
    for (int k = 0; k < 16; ++k)
        CHECK(with_index(blob, std::vector<uint8_t>(index.begin(), index.begin() + index.size() * k / 16), rects[11]) == 1);
    for (int k = 0; k < flips; ++k) {                               // damaged containers with the good index
        std::vector<uint8_t> x = blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * x.size());
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        with_index(x, index, rects[10 + k % 4]);
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250308);
    const int shapes[][3] = {{8, 8, 1}, {64, 40, 4}, {203, 117, 8}, {120, 64, 32}};
    for (const auto& s : shapes) {
        const std::vector<uint8_t> blob = random_container(rng, s[0], s[1], s[2]), twin = random_container(rng, s[0], s[1], s[2]);
        for (uint32_t interval : {32u, 100u, 65536u}) drive(rng, blob, twin, s[0], s[1], interval, 32);
    }
    if (argc > 1) {                 // triples written by tests/test_asan_region.py: <dir>/<n>.mn, <dir>/<n>.idx, <dir>/<n>.rect ("x y w h")
        auto slurp = [](const std::string& path, std::vector<uint8_t>& out) {
            std::ifstream f(path, std::ios::binary);
            if (!f) return false;
            out.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            return true;
        };
        int triples = 0;
        for (;; ++triples) {
            std::vector<uint8_t> x, index;
            const std::string stem = std::string(argv[1]) + "/" + std::to_string(triples);
            std::ifstream rf(stem + ".rect");
            Rect r{};
            if (!slurp(stem + ".mn", x) || !slurp(stem + ".idx", index) || !(rf >> r.x >> r.y >> r.w >> r.h)) break;
            with_index(x, index, r);
        }
        std::printf("asan_region: %d triples from files\n", triples);
    }
    std::printf("asan_region: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
