// asan_view.cpp -- the views' host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-view` /
// tests/test_asan_view.py.  mpc::truncate_container -- the rate-scalable transcode that defines a view's steps -- and
// mpc::read_window_by_index with `steps` -- the definition of what the view decoder's device route parses -- on what nobody vouches
// for: good containers with damaged indexes, damaged containers with a good index, views of every kind.  Beside every sanitizer
// report the rules are checked: the view's parse is the windowed parse of the truncated container; with "parse all" the result is
// the serial route's whatever the index holds; without, a refused index gives the serial route's result and anything else at least
// answers; the truncation refuses exactly what read_compressed refuses and is idempotent.
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

struct View { int x, y, w, h, steps; };

// The truncation of x to `steps` >= 1; returns whether read_compressed takes x.  *exact (optional): every kept stream reads back
// symbol for symbol.  That holds for whatever an encoder writes; it cannot hold for a damaged container whose step-0 coefficient
// sums take steps of 2^15 and more: the difference coder keeps 16 bits of a zig-zag code of 17, in the reference's writer as here
static bool truncation(const std::vector<uint8_t>& x, int steps, std::vector<uint8_t>& cut, bool* exact = nullptr) {
    const std::vector<uint8_t> xc(x.begin(), x.end());              // an exact-size copy: one byte read past its end is a report
    mpc::Streams whole;
    const bool readable = mpc::read_compressed(xc.data(), xc.size(), whole);
    const bool done = mpc::truncate_container(xc.data(), xc.size(), steps, cut);
    CHECK(done == readable);
    if (!done) return false;
    mpc::Streams s;
    CHECK(mpc::read_compressed(cut.data(), cut.size(), s));
    CHECK(s.width == whole.width && s.height == whole.height && s.K == whole.K && s.block_size == whole.block_size);
    CHECK(std::memcmp(s.quant, whole.quant, sizeof(s.quant)) == 0 && s.lengths.size() == whole.lengths.size());
    for (size_t t = 0; t < s.lengths.size() && t < whole.lengths.size(); ++t)
        CHECK(s.lengths[t] == std::min<int>(whole.lengths[t], steps));
    bool same = true;
    for (int i = 0; i < 6 * s.K; ++i) {
        const bool dc = i % (2 * s.K) == 1;
        if ((i % (2 * s.K)) / 2 >= steps) CHECK(s.codes[i].empty());
        else if (!dc) CHECK(s.codes[i] == whole.codes[i]);
        else {
            CHECK(s.codes[i].size() == whole.codes[i].size());
            same = same && s.codes[i] == whole.codes[i];
        }
    }
    if (exact) *exact = same;
    std::vector<uint8_t> again;
    CHECK(mpc::truncate_container(cut.data(), cut.size(), steps, again) && again == cut);
    return true;
}

// container x with index `index`, view v, both flags; returns the route without "parse all" (-1: no answer)
static int with_index(const std::vector<uint8_t>& x, const std::vector<uint8_t>& index, const View& v) {
    const std::vector<uint8_t> xc(x.begin(), x.end()), ic(index.begin(), index.end());
    std::vector<uint16_t> serial, all, cut, defined;
    std::vector<uint64_t> serial_ranges, all_ranges, cut_ranges, defined_ranges;
    int serial_route = -1, all_route = -1, cut_route = -1, defined_route = -1;
    const int want = mpc::read_window_by_index(xc.data(), xc.size(), nullptr, 0, v.x, v.y, v.w, v.h, false, serial, serial_ranges, &serial_route, v.steps);
    CHECK(want != 0 || serial_route == 1);
    // the definition: the windowed parse of the truncated container
    int K = 0, width, height, bs;
    std::vector<uint8_t> truncated;
    bool exact = false;
    if (mpc::container_info(xc.data(), xc.size(), &width, &height, &K, &bs) && v.steps >= 1 && truncation(x, v.steps, truncated, &exact) && exact) {
        const int got = mpc::read_window_by_index(truncated.data(), truncated.size(), nullptr, 0, v.x, v.y, v.w, v.h, false, defined, defined_ranges,
                                                  &defined_route);
        CHECK(got == want);
        if (got == 0 && want == 0) CHECK(defined == serial && defined_ranges == serial_ranges);
    }
    const int got_all = mpc::read_window_by_index(xc.data(), xc.size(), ic.data(), ic.size(), v.x, v.y, v.w, v.h, true, all, all_ranges, &all_route, v.steps);
    CHECK(got_all == want);
    if (want == 0 && got_all == 0) CHECK(all == serial && all_ranges == serial_ranges && (all_route == 0 || all_route == 1));
    const int got_cut = mpc::read_window_by_index(xc.data(), xc.size(), ic.data(), ic.size(), v.x, v.y, v.w, v.h, false, cut, cut_ranges, &cut_route, v.steps);
    // Chunks outside the window and streams of steps at or above the view's are not read: damage there goes unseen, so a container
    // the serial route refuses may still answer.  What does not answer has the serial route's verdict, and so has every refusal
    CHECK((got_cut == 2) == (want == 2));
    CHECK(got_cut == 0 || got_cut == want);
    if (got_cut == 0) {
        CHECK(cut_route == 0 || cut_route == 1);
        // parsing every chunk refuses whatever parsing some of them refuses -- but for the aux entries of a version-2 index, which
        // "parse all" does not use
        mpc::ContainerIndex ix;
        const bool aux_free = !mpc::read_container_index(ic.data(), ic.size(), ix) || ix.version == 1;
        if (got_all == 0 && aux_free) CHECK(cut_route <= all_route);
        if (cut_route == 1) CHECK(want == 0 && cut == serial && cut_ranges == serial_ranges);
        if (v.steps >= 1 && v.steps < K)                            // a stream of a cut step owns nothing
            for (int p = 0; p < 3 * K; ++p)
                if (p % K >= v.steps) CHECK(cut_ranges[2 * static_cast<size_t>(p)] == 0 && cut_ranges[2 * static_cast<size_t>(p) + 1] == 0);
    }
    return want == 0 ? cut_route : -1;
}

static std::vector<View> views_of(std::mt19937& rng, int W, int H, int K) {
    std::vector<View> out = {{0, 0, W, H, 0}, {0, 0, W, H, 1}, {0, 0, 1, 1, K}, {W - 1, H - 1, 1, 1, K + 3}, {W / 2, 0, 1, H, (K + 1) / 2},
                             {-1, 0, 2, 2, 1}, {0, 0, W + 1, 1, 1}, {0, 0, 0, 0, 1}, {W, H, 1, 1, 0}, {2147483647, 0, 2, 2, 2}};
    for (int k = 0; k < 4; ++k) {
        const int x = static_cast<int>(rng() % W), y = static_cast<int>(rng() % H);
        out.push_back({x, y, 1 + static_cast<int>(rng() % (W - x)), 1 + static_cast<int>(rng() % (H - y)), 1 + static_cast<int>(rng() % K)});
    }
    return out;
}

static void drive(std::mt19937& rng, const std::vector<uint8_t>& blob, const std::vector<uint8_t>& twin, int W, int H, int K, uint32_t interval,
                  bool expanded, int flips) {
    std::vector<uint8_t> index;
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, index, expanded));
    const std::vector<View> views = views_of(rng, W, H, K);
    for (size_t k = 0; k < views.size(); ++k) {
        const int route = with_index(blob, index, views[k]);
        CHECK(route == (k < 5 || k >= 10 ? 0 : -1));                // the good index is used; views 5 - 9 are refused as arguments
    }
    if (!twin.empty()) {
        std::vector<uint8_t> other;
        CHECK(mpc::build_container_index(twin.data(), twin.size(), interval, other, expanded));
        CHECK(with_index(blob, other, views[10]) == 1);
    }
    int refused = 0;
    for (int k = 0; k < flips; ++k) {                               // damaged indexes
        std::vector<uint8_t> bad = index;
        const size_t bit = rng() % (8 * (k % 4 == 0 ? std::min<size_t>(bad.size(), 56) : bad.size()));
        bad[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        refused += with_index(blob, bad, views[10 + k % 4]);
    }
    CHECK(refused > 0);
    for (int k = 0; k < 16; ++k)
        CHECK(with_index(blob, std::vector<uint8_t>(index.begin(), index.begin() + index.size() * k / 16), views[11]) == 1);
    for (int k = 0; k < flips; ++k) {                               // damaged containers with the good index
        std::vector<uint8_t> x = blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * x.size());
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        with_index(x, index, views[10 + k % 4]);
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250309);
    const int shapes[][3] = {{8, 8, 1}, {64, 40, 4}, {203, 117, 8}, {120, 64, 32}};
    for (const auto& s : shapes) {
        const std::vector<uint8_t> blob = random_container(rng, s[0], s[1], s[2]), twin = random_container(rng, s[0], s[1], s[2]);
        for (int m = 1; m <= s[2] + 1; ++m) {                       // an encoder's container: K steps and more give it back
            std::vector<uint8_t> cut;
            bool exact = false;
            CHECK(truncation(blob, m, cut, &exact) && exact);
            CHECK((m < s[2]) == (cut != blob));
            CHECK(cut.size() <= blob.size());
        }
        for (uint32_t interval : {32u, 100u})
            for (bool expanded : {false, true}) drive(rng, blob, twin, s[0], s[1], s[2], interval, expanded, 24);
    }
    if (argc > 1) {                 // written by tests/test_asan_view.py: <dir>/<n>.mn, <dir>/<n>.idx, <dir>/<n>.view ("x y w h steps")
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
            std::ifstream vf(stem + ".view");
            View v{};
            if (!slurp(stem + ".mn", x) || !slurp(stem + ".idx", index) || !(vf >> v.x >> v.y >> v.w >> v.h >> v.steps)) break;
            with_index(x, index, v);
            std::vector<uint8_t> cut;
            truncation(x, v.steps < 1 ? 1 : v.steps, cut);
        }
        std::printf("asan_view: %d triples from files\n", triples);
    }
    std::printf("asan_view: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
