// asan_index_scan.cpp -- the seek index from a bit scan, on the host, under AddressSanitizer + UBSan (g++, no GPU, no HIP):
// `make asan-index-scan` / tests/test_asan_index_scan.py.  The step table, the segment maps, the chain and the walk that define what
// mp_scan.hip computes, on what nobody vouches for: damaged and truncated containers, at sizes that make codes span segments and
// streams span windows.  Beside every sanitizer report, the contract itself is checked: verdict and blob are the serial builder's,
// and the scan does not give up where the serially built index is one the chunked parse uses.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <string>

static int g_failed = 0, g_scanned = 0;
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

// container x: the scan's verdict, blob and route against the serial builder's, at the given sizes (0 = the defaults)
static int scan(const std::vector<uint8_t>& x, uint32_t interval, bool expanded, uint32_t segment, uint32_t window) {
    const std::vector<uint8_t> xc(x.begin(), x.end());          // an exact-size copy: one byte read past the end is a report
    std::vector<uint8_t> serial, mine;
    const bool ok = mpc::build_container_index(xc.data(), xc.size(), interval, serial, expanded);
    CHECK(mpc::scan_sizes_ok(&segment, &window));
    int route = -1;
    const bool got = mpc::scan_container_index(xc.data(), xc.size(), interval, expanded, segment, window, mine, &route);
    CHECK(got == ok);
    CHECK(route == 0 || route == 1);
    if (ok && got) CHECK(serial == mine);
    if (ok) {                                                   // an index the chunked parse uses: the scan may not have given up
        mpc::CodedStreams s;
        int by_index = -1;
        CHECK(mpc::read_compressed_coded_by_index(xc.data(), xc.size(), serial.data(), serial.size(), s, &by_index));
        if (by_index == 0) CHECK(route == 0);
    } else {
        CHECK(route == 1);
    }
    g_scanned += route == 0;
    return route;
}

static void drive(std::mt19937& rng, const std::vector<uint8_t>& blob, uint32_t interval, int flips) {
    const uint32_t sizes[][2] = {{0, 0}, {32, 64}, {64, 4096}, {256, 1024}, {4096, 4096}};
    for (const auto& sz : sizes)
        for (int expanded = 0; expanded < 2; ++expanded) CHECK(scan(blob, interval, expanded != 0, sz[0], sz[1]) == 0);
    for (int k = 0; k < flips; ++k) {
        std::vector<uint8_t> x = blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * x.size());
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        const auto& sz = sizes[k % 5];
        scan(x, interval, k % 3 == 0, sz[0], sz[1]);
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250911);
    uint32_t bad_segment = 16, bad_window = 64, odd_segment = 64, odd_window = 96;
    CHECK(!mpc::scan_sizes_ok(&bad_segment, &bad_window));
    CHECK(!mpc::scan_sizes_ok(&odd_segment, &odd_window));
    const int shapes[][3] = {{8, 8, 1}, {64, 40, 4}, {200, 120, 8}, {120, 64, 32}};
    for (const auto& s : shapes) {
        if (argc > 2) break;                                    // the second run takes the files alone
        const std::vector<uint8_t> blob = random_container(rng, s[0], s[1], s[2]);
        for (uint32_t interval : {32u, 65536u}) drive(rng, blob, interval, 30);
    }
    if (argc > 1 && argv[1][0]) {                               // the reference's own container, whole and truncated
        std::ifstream f(argv[1], std::ios::binary);
        const std::vector<uint8_t> mn((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        CHECK(!mn.empty());
        if (!mn.empty()) {
            CHECK(scan(mn, 0, false, 0, 0) == 0);
            CHECK(scan(mn, 256, true, 4096, 1u << 16) == 0);
            for (int k = 0; k < 12; ++k) {
                std::vector<uint8_t> cut(mn.begin(), mn.begin() + static_cast<long>(k < 4 ? rng() % 4096 : rng() % mn.size()));
                CHECK(scan(cut, 0, false, 0, 0) == 1);
            }
        }
    }
    if (argc > 2) {                                             // containers written by tests/test_asan_index_scan.py: <dir>/<n>.mn
        int files = 0;
        for (;; ++files) {
            std::ifstream f(std::string(argv[2]) + "/" + std::to_string(files) + ".mn", std::ios::binary);
            if (!f) break;
            const std::vector<uint8_t> x((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            scan(x, 100, files % 2 == 1, files % 3 == 0 ? 0 : 64, files % 3 == 0 ? 0 : 1024);
        }
        std::printf("asan_index_scan: %d containers from files\n", files);
    }
    std::printf("asan_index_scan: %d on route 0\n", g_scanned);
    std::printf("asan_index_scan: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
