// asan_budget.cpp -- the rate control's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-budget` /
// tests/test_asan_budget.py.  mpc::budget_lambda, mpc::budget_weights -- on the seek indexes of a photograph's container and of
// random ones, whole and damaged: cut short, bits flipped, the sizes inside rewritten -- and mpc::budget_allocate, which defines what
// the allocation kernel computes, on exact-size buffers (one word read past a tile's K + 1 is a report), counts above K among them.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"
#include "../../imageexperiments_amd/csrc/host_budget.cpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <string>

static int g_failed = 0, g_cases = 0;
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

// the weights of an index that may hold anything, into exactly the room its own K asks for (or 96 words if it does not read)
static int weigh(const std::vector<uint8_t>& index, std::vector<uint32_t>* out = nullptr) {
    ++g_cases;
    const std::vector<uint8_t> exact(index.begin(), index.end());
    mpc::ContainerIndex x;
    const bool reads = mpc::read_container_index(exact.data(), exact.size(), x);
    std::vector<uint32_t> w(reads ? 3 * static_cast<size_t>(x.K) : 96, 0xDEADBEEFu);
    int K = -1;
    const int verdict = mpc::budget_weights(exact.data(), exact.size(), w.data(), &K);
    CHECK(verdict == 0 || verdict == 1 || verdict == 2);
    CHECK(reads || verdict == 1);
    if (verdict == 0) {
        CHECK(reads && K == x.K && !x.serial_only);
        for (uint32_t v : w) CHECK(v >= mpc::kBudgetWeightMin && v <= mpc::kBudgetWeightMax);
    }
    if (verdict == 2) CHECK(reads && x.serial_only);
    CHECK(mpc::budget_weights(exact.data(), exact.size(), nullptr) == verdict);      // the verdict alone
    if (out) *out = w;
    return verdict;
}

static void weights_cases(std::mt19937& rng, const std::vector<uint8_t>& blob, uint32_t interval, bool expanded) {
    std::vector<uint8_t> index;
    CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, index, expanded));
    std::vector<uint32_t> good;
    CHECK(weigh(index, &good) == 0);
    // the definition, from the index read back
    mpc::ContainerIndex x;
    CHECK(mpc::read_container_index(index.data(), index.size(), x));
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < x.K; ++i) {
            const size_t a = 1 + 2 * static_cast<size_t>(x.K) * ch + 2 * static_cast<size_t>(i);
            const uint64_t bits = x.streams[a + 1].end_bit - x.streams[a].wrapper_bit, n = x.streams[a].expect;
            uint64_t w = n ? (256 * bits + n / 2) / n : 256;
            w = w < 256 ? 256 : w > (1u << 20) ? (1u << 20) : w;
            CHECK(good[static_cast<size_t>(ch) * x.K + i] == w);
        }
    // cut short at every kind of place
    for (size_t cut : {size_t{0}, size_t{1}, size_t{55}, size_t{56}, size_t{57}, index.size() / 2, index.size() - 8, index.size() - 1})
        if (cut < index.size()) CHECK(weigh(std::vector<uint8_t>(index.begin(), index.begin() + static_cast<long>(cut))) == 1);
    // the flag word: serial only
    std::vector<uint8_t> serial = index;
    serial[12] |= 1;
    CHECK(weigh(serial) == 2);
    // bits flipped in the header and the stream records, and the sizes of a stream rewritten: end_bit in front of wrapper_bit, bits and
    // record counts near 2^64
    for (int k = 0; k < 300; ++k) {
        std::vector<uint8_t> bad = index;
        const size_t span = 56 + 64 * x.streams.size();
        bad[rng() % (k < 200 ? span : bad.size())] ^= static_cast<uint8_t>(1u << (rng() % 8));
        (void)weigh(bad);
    }
    for (int k = 0; k < 60; ++k) {
        std::vector<uint8_t> bad = index;
        const size_t j = 1 + rng() % (x.streams.size() - 1), field = rng() % 4;      // wrapper_bit, end_bit, n_coded, expect
        const uint64_t v = k % 3 == 0 ? ~uint64_t{0} : k % 3 == 1 ? (uint64_t{1} << 63) + rng() : rng();
        std::memcpy(bad.data() + 56 + 64 * j + 8 * field, &v, 8);
        (void)weigh(bad);
    }
}

static void allocate_case(std::mt19937& rng, long long tiles, int K, int j, bool above) {
    ++g_cases;
    // exact-size heap buffers
    std::vector<uint32_t> profile(static_cast<size_t>(tiles) * (K + 1)), weights(3 * static_cast<size_t>(K));
    std::vector<uint16_t> counts(3 * static_cast<size_t>(tiles)), cut(counts.size(), 0xFFFF);
    std::vector<uint8_t> depth(static_cast<size_t>(tiles), 0xFF);
    for (uint32_t& w : weights) w = mpc::kBudgetWeightMin + rng() % (rng() % 4 == 0 ? mpc::kBudgetWeightMax - mpc::kBudgetWeightMin + 1 : 5000);
    for (uint16_t& c : counts) c = static_cast<uint16_t>(above && rng() % 7 == 0 ? K + 1 + rng() % 60000 : rng() % (K + 1));
    for (long long t = 0; t < tiles; ++t) {
        int deepest = 0;
        for (int ch = 0; ch < 3; ++ch) deepest = std::max<int>(deepest, std::min<int>(counts[t * 3 + ch], K));
        uint32_t v = 1000 + rng() % 12000000;
        for (int n = 0; n <= K; ++n) {
            if (n >= 1 && n <= deepest) v = rng() % 5 == 0 ? v + rng() % 3000 : v - rng() % (v / 2 + 1);
            profile[t * (K + 1) + n] = v;
        }
    }
    uint64_t totals[3] = {1, 2, 3};
    mpc::budget_allocate(profile.data(), counts.data(), tiles, K, weights.data(), j, depth.data(), cut.data(), totals);
    uint64_t kept = 0, distortion = 0;
    for (long long t = 0; t < tiles; ++t) {
        CHECK(depth[t] <= K);
        if (j == mpc::kBudgetLambdas - 1) CHECK(depth[t] == 0);
        distortion += profile[t * (K + 1) + depth[t]];
        for (int ch = 0; ch < 3; ++ch) {
            CHECK(cut[t * 3 + ch] == std::min<int>(std::min<int>(counts[t * 3 + ch], K), depth[t]));
            kept += cut[t * 3 + ch];
        }
        // no depth does better, and none below it as well
        const uint64_t L = mpc::budget_lambda(j);
        auto J = [&](int n) {
            uint64_t rate = 0;
            for (int ch = 0; ch < 3; ++ch)
                for (int i = 0; i < std::min<int>(n, std::min<int>(counts[t * 3 + ch], K)); ++i) rate += weights[ch * K + i];
            return (static_cast<uint64_t>(profile[t * (K + 1) + n]) << 16) + L * rate;
        };
        for (int n = 0; n <= K; ++n) CHECK(n < depth[t] ? J(n) > J(depth[t]) : J(n) >= J(depth[t]));
    }
    CHECK(totals[0] == distortion && totals[2] == kept);
    if (j == mpc::kBudgetLambdas - 1) CHECK(totals[1] == 0 && kept == 0);
    // the outputs are optional
    uint64_t again[3];
    mpc::budget_allocate(profile.data(), counts.data(), tiles, K, weights.data(), j, nullptr, nullptr, again);
    CHECK(std::memcmp(again, totals, sizeof(again)) == 0);
}

int main(int argc, char** argv) {
    std::mt19937 rng(20240923);
    CHECK(mpc::budget_lambda(0) == 0 && mpc::budget_lambda(1) == 8 && mpc::budget_lambda(9) == 16 && mpc::budget_lambda(255) == (uint64_t{14} << 31));
    for (int j = 1; j < mpc::kBudgetLambdas; ++j) CHECK(mpc::budget_lambda(j) > mpc::budget_lambda(j - 1));
    if (argc > 1) {
        std::ifstream f(argv[1], std::ios::binary);
        const std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        CHECK(!s.empty());
        const std::vector<uint8_t> blob(s.begin(), s.end());
        weights_cases(rng, blob, 0, false);
        weights_cases(rng, blob, 32, true);
    }
    for (int K : {1, 8, 32}) {
        weights_cases(rng, random_container(rng, 40, 24, K), 64, K != 8);
        weights_cases(rng, random_container(rng, 8, 8, K), 32, false);
    }
    for (int K : {1, 8, 32})
        for (long long tiles : {0LL, 1LL, 63LL, 64LL, 65LL, 4097LL})
            for (int j : {0, 1, 77, 130, 190, 255}) {
                if (tiles == 4097 && K == 32 && j % 2) continue;
                allocate_case(rng, tiles, K, j, false);
                allocate_case(rng, tiles, K, j, true);
            }
    std::printf("asan_budget: %d cases\n", g_cases);
    std::printf("asan_budget: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
