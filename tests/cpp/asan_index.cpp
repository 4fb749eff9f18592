// asan_index.cpp -- the seek index's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-index` /
// tests/test_asan_index.py.  The index builder, the validator and the host's chunk decoder on what nobody vouches for: damaged
// containers with a good index, good containers with damaged indexes, both damaged.  Beside every sanitizer report, the rule
// itself is checked: with any index the result is the serial parse's.
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
        for (int i = 0; i < counts[o]; ++i)
            choices[o * K + i] = (rng() % (o % 3 == 0 ? 2500 : 12)) | ((rng() % (i == 0 ? 4000 : 60)) << 16);
    }
    std::vector<double> quant(3 * static_cast<size_t>(K), 1.0);
    size_t n = 0;
    uint8_t* b = mpc::encode_records_malloc(W, H, K, 8, quant.data(), counts.data(), choices.data(), &n);
    CHECK(b);
    const std::vector<uint8_t> blob(b, b + (b ? n : 0));
    std::free(b);
    return blob;
}

static bool same_streams(const mpc::CodedStreams& a, const mpc::CodedStreams& b) {
    return a.width == b.width && a.height == b.height && a.K == b.K && a.block_size == b.block_size && a.lengths == b.lengths &&
           a.codes == b.codes && a.packed == b.packed && a.expect == b.expect && std::memcmp(a.quant, b.quant, sizeof(a.quant)) == 0;
}

// container x with index `index`: the serial parse's verdict and streams, whatever either holds
static int with_index(const std::vector<uint8_t>& x, const std::vector<uint8_t>& index) {
    // exact-size copies: one byte read past either end is a report
    const std::vector<uint8_t> xc(x.begin(), x.end()), ic(index.begin(), index.end());
    mpc::CodedStreams serial, mine;
    const bool ok = mpc::read_compressed_coded(xc.data(), xc.size(), serial);
    int route = -1;
    const bool got = mpc::read_compressed_coded_by_index(xc.data(), xc.size(), ic.data(), ic.size(), mine, &route);
    CHECK(got == ok);
    CHECK(route == 0 || route == 1);
    if (ok && got) CHECK(same_streams(serial, mine));
    mpc::ContainerIndex read;
    (void)mpc::read_container_index(ic.data(), ic.size(), read);
    // the validator as a single-frame decode calls it: the wrappers read on the worker pool; same verdict as on one thread
    mpc::IndexedPlan one, pooled;
    CHECK(mpc::plan_indexed_parse(xc.data(), xc.size(), ic.data(), ic.size(), one, false) ==
          mpc::plan_indexed_parse(xc.data(), xc.size(), ic.data(), ic.size(), pooled, true));
    return route;
}

// twin: another container of the same geometry (may be empty)
static void drive(std::mt19937& rng, const std::vector<uint8_t>& blob, const std::vector<uint8_t>& twin, uint32_t interval, int flips) {
    std::vector<uint8_t> index;
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, index));
    CHECK(with_index(blob, index) == 0);
    if (!twin.empty()) {                                            // another container's index
        std::vector<uint8_t> other;
        CHECK(mpc::build_container_index(twin.data(), twin.size(), interval, other));
        CHECK(with_index(blob, other) == 1);
    }
    int refused = 0;
    for (int k = 0; k < flips; ++k) {                               // damaged indexes
        std::vector<uint8_t> bad = index;
        const size_t bit = rng() % (8 * (k % 4 == 0 ? std::min<size_t>(bad.size(), 56) : bad.size()));
        bad[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        refused += with_index(blob, bad);
    }
    CHECK(refused > 0);
    for (int k = 0; k < 16; ++k) CHECK(with_index(blob, std::vector<uint8_t>(index.begin(), index.begin() + index.size() * k / 16)) == 1);
    for (int k = 0; k < flips; ++k) {                               // damaged containers: the good index, and their own where they have one
        std::vector<uint8_t> x = blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * x.size());
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        with_index(x, index);
        std::vector<uint8_t> own;
        mpc::CodedStreams serial;
        const std::vector<uint8_t> xc(x.begin(), x.end());
        CHECK(mpc::build_container_index(xc.data(), xc.size(), interval, own) == mpc::read_compressed_coded(xc.data(), xc.size(), serial));
        if (!own.empty()) with_index(x, own);
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250307);
    const int shapes[][3] = {{8, 8, 1}, {64, 40, 4}, {200, 120, 8}, {120, 64, 32}};
    for (const auto& s : shapes) {
        const std::vector<uint8_t> blob = random_container(rng, s[0], s[1], s[2]), twin = random_container(rng, s[0], s[1], s[2]);
        for (uint32_t interval : {32u, 100u, 65536u}) drive(rng, blob, twin, interval, 96);
    }
    if (argc > 1 && argv[1][0]) {                                                 // the reference's own container: a few flips of a large index
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> mn((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        CHECK(!mn.empty());
        if (!mn.empty()) drive(rng, mn, {}, 256, 6);
    }
    if (argc > 2) {                                                 // pairs written by tests/test_asan_index.py: <dir>/<n>.mn with <dir>/<n>.idx
        auto slurp = [](const std::string& path, std::vector<uint8_t>& out) {
            std::ifstream f(path, std::ios::binary);
            if (!f) return false;
            out.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            return true;
        };
        int pairs = 0;
        for (;; ++pairs) {
            std::vector<uint8_t> x, index;
            const std::string stem = std::string(argv[2]) + "/" + std::to_string(pairs);
            if (!slurp(stem + ".mn", x) || !slurp(stem + ".idx", index)) break;
            with_index(x, index);
        }
        std::printf("asan_index: %d pairs from files\n", pairs);
    }
    std::printf("asan_index: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
