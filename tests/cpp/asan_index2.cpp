// asan_index2.cpp -- index version 2's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-index2` /
// tests/test_asan_index2.py.  The aux section's builder and reader, mpc::extend_container_index and the windowed parse that cuts
// packed and step-0 coefficient streams through the aux entries (mpc::read_window_by_index, mpc::window_chunks_by_index), on what
// nobody vouches for: good containers with damaged version-2 indexes (the aux section above all), damaged containers with a good
// one.  Beside every sanitizer report the rules are checked: with "parse all" the result is the serial route's whatever the index
// holds; without, a refused index gives the serial route's result and anything else at least answers; an extended index is the
// built one whatever the version-1 index it starts from holds.
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
            choices[o * K + i] = (rng() % (o % 3 == 0 ? 2500 : 3)) | ((rng() % (i == 0 ? (o % 3 == 2 ? 2 : 4000) : 60)) << 16);
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
    std::vector<uint64_t> serial_ranges, all_ranges, cut_ranges, chunks;
    int serial_route = -1, all_route = -1, cut_route = -1, chunks_route = -1;
    const int want = mpc::read_window_by_index(xc.data(), xc.size(), nullptr, 0, r.x, r.y, r.w, r.h, false, serial, serial_ranges, &serial_route);
    CHECK(want != 0 || serial_route == 1);
    const int got_all = mpc::read_window_by_index(xc.data(), xc.size(), ic.data(), ic.size(), r.x, r.y, r.w, r.h, true, all, all_ranges, &all_route);
    CHECK(got_all == want);
    if (want == 0 && got_all == 0) CHECK(all == serial && all_ranges == serial_ranges && (all_route == 0 || all_route == 1));
    const int got_cut = mpc::read_window_by_index(xc.data(), xc.size(), ic.data(), ic.size(), r.x, r.y, r.w, r.h, false, cut, cut_ranges, &cut_route);
    CHECK((got_cut == 2) == (want == 2));
    CHECK(got_cut == 0 || got_cut == want);
    if (got_cut == 0) {
        CHECK(cut_route == 0 || cut_route == 1);
        if (cut_route == 1) CHECK(want == 0 && cut == serial && cut_ranges == serial_ranges);
    }
    const int got_chunks = mpc::window_chunks_by_index(xc.data(), xc.size(), ic.data(), ic.size(), r.x, r.y, r.w, r.h, false, chunks, &chunks_route);
    CHECK((got_chunks == 2) == (want == 2));
    if (got_chunks == 0) {
        mpc::ContainerIndex ix;
        const bool readable = mpc::read_container_index(ic.data(), ic.size(), ix);
        CHECK(chunks_route == 1 || readable);
        for (size_t i = 0; chunks_route == 0 && 2 * i < chunks.size(); ++i)
            CHECK(chunks[2 * i] <= chunks[2 * i + 1] && chunks[2 * i + 1] <= ix.streams[i + 1].checkpoints.size());
    }
    // the whole-frame parse takes a version-2 index for its version-1 part
    mpc::CodedStreams a, b;
    int route = -1;
    const bool whole = mpc::read_compressed_coded_by_index(xc.data(), xc.size(), ic.data(), ic.size(), a, &route);
    CHECK(whole == mpc::read_compressed_coded(xc.data(), xc.size(), b));
    if (whole) CHECK(a.lengths == b.lengths && a.codes == b.codes && a.expect == b.expect);
    return want == 0 ? cut_route : -1;
}

// the aux reader on a blob of exactly its size, and extend on whatever it is
static void read_back(const std::vector<uint8_t>& x, const std::vector<uint8_t>& index, const std::vector<uint8_t>& built) {
    const std::vector<uint8_t> xc(x.begin(), x.end()), ic(index.begin(), index.end());
    mpc::ContainerIndex ix;
    if (mpc::read_container_index(ic.data(), ic.size(), ix)) {
        uint64_t sum = 0;
        for (const mpc::IndexStream& s : ix.streams) {
            CHECK(s.aux.empty() || s.aux.size() == s.checkpoints.size());
            for (const mpc::IndexAux& a : s.aux) sum += a.out + a.prev + a.state + a.dc;
        }
        CHECK(ix.version == 1 || ix.version == 2 || sum == 0);
    }
    std::vector<uint8_t> extended;
    const bool ok = mpc::extend_container_index(xc.data(), xc.size(), ic.data(), ic.size(), extended);
    if (!built.empty()) {                                           // a good container: the built index, or the version-2 input itself
        CHECK(ok);
        mpc::ContainerIndex in;
        const bool v2 = mpc::read_container_index(ic.data(), ic.size(), in) && in.version == 2;
        bool same_interval = ic.size() >= 12 && built.size() >= 12 && std::memcmp(ic.data() + 8, built.data() + 8, 4) == 0;
        if (ok && v2) CHECK(extended == index);
        else if (ok && same_interval) CHECK(extended == built);
    }
}

static std::vector<Rect> rects_of(std::mt19937& rng, int W, int H) {
    std::vector<Rect> out = {{0, 0, W, H}, {0, 0, 1, 1}, {W - 1, H - 1, 1, 1}, {W / 2, 0, 1, H}, {0, H / 2, W, 1}, {-1, 0, 2, 2}, {0, 0, 0, 0}};
    for (int k = 0; k < 4; ++k) {
        const int x = static_cast<int>(rng() % W), y = static_cast<int>(rng() % H);
        out.push_back({x, y, 1 + static_cast<int>(rng() % (W - x)), 1 + static_cast<int>(rng() % (H - y))});
    }
    return out;
}

static void drive(std::mt19937& rng, const std::vector<uint8_t>& blob, const std::vector<uint8_t>& twin, int W, int H, uint32_t interval,
                  int flips) {
    std::vector<uint8_t> v1, index, again;
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, v1));
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, index, true));
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, again, false) && again == v1);
    CHECK(index.size() >= v1.size() + 8 && std::memcmp(index.data() + 8, v1.data() + 8, v1.size() - 8) == 0);
    read_back(blob, v1, index);
    read_back(blob, index, index);
    {
        std::vector<uint8_t> patched = v1;                          // a version-1 blob that calls itself version 2 is refused
        patched[4] = 2;
        mpc::ContainerIndex ix;
        CHECK(!mpc::read_container_index(patched.data(), patched.size(), ix));
        read_back(blob, patched, index);
    }
    const std::vector<Rect> rects = rects_of(rng, W, H);
    for (size_t k = 0; k < rects.size(); ++k) {
        const int route = with_index(blob, index, rects[k]);
        CHECK(route == (k < 5 || k >= 7 ? 0 : -1));                 // the good index is used; rectangles 5 and 6 are refused as arguments
    }
    if (!twin.empty()) {
        std::vector<uint8_t> other;
        CHECK(mpc::build_container_index(twin.data(), twin.size(), interval, other, true));
        CHECK(with_index(blob, other, rects[7]) == 1);
    }
    const size_t aux_bits = 8 * (index.size() - v1.size());
    int refused = 0;
    for (int k = 0; k < flips; ++k) {                               // damaged indexes: every second flip inside the aux section
        std::vector<uint8_t> bad = index;
        const size_t bit = k % 2 == 0 ? 8 * v1.size() + rng() % aux_bits : rng() % (8 * bad.size());
        bad[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        refused += with_index(blob, bad, rects[7 + k % 4]);
        if (k % 4 == 0) read_back(blob, bad, index);
        std::vector<uint8_t> bad1 = v1;                             // and extend from a damaged version-1 index
        const size_t bit1 = rng() % (8 * bad1.size());
        bad1[bit1 / 8] ^= static_cast<uint8_t>(1u << (bit1 % 8));
        if (k % 4 == 1) read_back(blob, bad1, index);
    }
    CHECK(refused > 0);
    for (int k = 0; k < 16; ++k) {
        const std::vector<uint8_t> shorter(index.begin(), index.begin() + index.size() * k / 16);
        CHECK(with_index(blob, shorter, rects[8]) == 1);
        read_back(blob, shorter, std::vector<uint8_t>());
    }
    for (int k = 0; k < flips; ++k) {                               // damaged containers with the good index
        std::vector<uint8_t> x = blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * x.size());
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        with_index(x, index, rects[7 + k % 4]);
        if (k % 4 == 0) read_back(x, v1, std::vector<uint8_t>());
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250310);
    const int shapes[][3] = {{8, 8, 1}, {64, 40, 4}, {203, 117, 8}, {120, 64, 32}};
    for (const auto& s : shapes) {
        const std::vector<uint8_t> blob = random_container(rng, s[0], s[1], s[2]), twin = random_container(rng, s[0], s[1], s[2]);
        for (uint32_t interval : {32u, 100u, 65536u}) drive(rng, blob, twin, s[0], s[1], interval, 32);
    }
    if (argc > 1) {                 // triples written by tests/test_asan_index2.py: <dir>/<n>.mn, <dir>/<n>.idx, <dir>/<n>.rect ("x y w h")
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
            read_back(x, index, std::vector<uint8_t>());
        }
        std::printf("asan_index2: %d triples from files\n", triples);
    }
    std::printf("asan_index2: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
