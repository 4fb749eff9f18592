// asan_quality.cpp -- the target-quality encode's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-quality` /
// tests/test_asan_quality.py.  mpc::budget_sweep -- which defines what the sweep kernel computes -- on exact-size buffers (one word
// read past a tile's K + 1, or one total written past the 768, is a report) against mpc::budget_allocate at all 256 multipliers,
// mpc::quality_pick against its definition, mpc::sse_for_psnr over mpc::psnr_from_sse against a linear look at its neighbours; and the
// three on hostile arguments: counts above K, profiles and weights at the ends of u32, totals no sweep makes, targets of every kind.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"
#include "../../imageexperiments_amd/csrc/host_budget.cpp"
#include "../../imageexperiments_amd/csrc/host_codec.cpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

constexpr int kWords = 3 * mpc::kBudgetLambdas;

// kind 0: a profile and weights inside their bounds, counts up to K + 1; 1: the bounds themselves (P_MAX, the upper clamp);
// 2: hostile -- any u32 in the profile and the weights, any u16 in the counts (the arithmetic wraps; nothing may be read out of place)
static void sweep_case(std::mt19937& rng, long long tiles, int K, int kind) {
    ++g_cases;
    const uint32_t p_max = 64u * 3u * 255u * 255u;
    std::vector<uint32_t> profile(static_cast<size_t>(tiles) * (K + 1)), weights(3 * static_cast<size_t>(K));
    std::vector<uint16_t> counts(3 * static_cast<size_t>(tiles));
    for (uint32_t& w : weights)
        w = kind == 2 ? static_cast<uint32_t>(rng()) : kind == 1 ? mpc::kBudgetWeightMax : mpc::kBudgetWeightMin + rng() % 20000;
    for (uint16_t& c : counts) c = static_cast<uint16_t>(kind == 2 ? rng() : rng() % (K + 2));
    for (long long t = 0; t < tiles; ++t) {
        int deepest = 0;
        for (int ch = 0; ch < 3; ++ch) deepest = std::max<int>(deepest, std::min<int>(counts[t * 3 + ch], K));
        uint32_t v = kind == 1 ? p_max : 1000 + rng() % 12000000;
        for (int n = 0; n <= K; ++n) {
            if (n >= 1 && n <= deepest) v = rng() % 4 == 0 ? std::min<uint32_t>(p_max, v + rng() % 3000) : v - rng() % (v / 2 + 1);   // not monotone
            profile[t * (K + 1) + n] = kind == 2 ? static_cast<uint32_t>(rng()) : v;
        }
    }
    std::vector<uint64_t> totals(kWords, 0xDEADBEEFDEADBEEFull);              // exact size; the sweep zeroes them itself
    mpc::budget_sweep(profile.data(), counts.data(), tiles, K, weights.data(), totals.data());
    for (int j = 0; j < mpc::kBudgetLambdas; ++j) {
        uint64_t want[3];
        mpc::budget_allocate(profile.data(), counts.data(), tiles, K, weights.data(), j, nullptr, nullptr, want);
        CHECK(std::memcmp(want, totals.data() + 3 * j, sizeof(want)) == 0);
        if (kind != 2 && j > 0) CHECK(totals[3 * j] >= totals[3 * (j - 1)] && totals[3 * j + 1] <= totals[3 * (j - 1) + 1]);
    }
    if (kind != 2) {
        uint64_t least = 0;
        for (long long t = 0; t < tiles; ++t) least += *std::min_element(profile.begin() + t * (K + 1), profile.begin() + (t + 1) * (K + 1));
        CHECK(totals[0] == least);
        CHECK(totals[3 * 255 + 1] == 0 && totals[3 * 255 + 2] == 0);
    }
    // the pick at every distortion of the sweep and beside it
    auto definition = [&](uint64_t s) {
        int at = -1;
        for (int j = 0; j < mpc::kBudgetLambdas; ++j)
            if (totals[3 * j] <= s) at = j;
        return at;
    };
    for (int j = 0; j < mpc::kBudgetLambdas; ++j)
        for (uint64_t s : {totals[3 * j], totals[3 * j] - 1, totals[3 * j] + 1}) CHECK(mpc::quality_pick(totals.data(), s) == definition(s));
    CHECK(mpc::quality_pick(totals.data(), ~uint64_t{0}) == 255);
    CHECK(mpc::quality_pick(totals.data(), 0) == definition(0));
}

static void pick_cases(std::mt19937& rng) {
    for (int k = 0; k < 200; ++k) {
        ++g_cases;
        std::vector<uint64_t> totals(kWords);                                // totals no sweep makes: not monotone, the ends of u64
        for (uint64_t& v : totals) v = k % 4 == 0 ? ~uint64_t{0} - rng() % 3 : k % 4 == 1 ? rng() % 3 : (static_cast<uint64_t>(rng()) << 32) | rng();
        for (int q = 0; q < 40; ++q) {
            const uint64_t s = q == 0 ? 0 : q == 1 ? ~uint64_t{0} : q % 2 ? totals[3 * (rng() % 256)] : (static_cast<uint64_t>(rng()) << 32) | rng();
            const int got = mpc::quality_pick(totals.data(), s);
            CHECK(got >= -1 && got < mpc::kBudgetLambdas);
            if (got >= 0) CHECK(totals[3 * got] <= s);
            for (int j = got + 1; j < mpc::kBudgetLambdas; ++j) CHECK(totals[3 * j] > s);
        }
    }
}

static void psnr_cases(std::mt19937& rng) {
    const double inf = std::numeric_limits<double>::infinity();
    const int geometries[][2] = {{1, 1}, {64, 48}, {197, 117}, {1920, 1080}, {7680, 4320}, {65536, 8190}};
    for (const auto& g : geometries) {
        const int W = g[0], H = g[1];
        const uint64_t tiles = static_cast<uint64_t>((W + 7) / 8) * static_cast<uint64_t>((H + 7) / 8), limit = uint64_t{195075} * 64 * tiles;
        auto psnr = [&](uint64_t s) { return mpc::psnr_from_sse(static_cast<double>(s), W, H); };
        CHECK(psnr(0) == inf);
        auto answer_is_the_largest = [&](double target) {
            ++g_cases;
            const uint64_t s = mpc::sse_for_psnr(target, limit, psnr);
            CHECK(s <= limit && psnr(s) >= target);
            if (s < limit) CHECK(psnr(s + 1) < target);
            return s;
        };
        CHECK(answer_is_the_largest(inf) == 0);
        CHECK(answer_is_the_largest(1e300) == 0);
        CHECK(answer_is_the_largest(-1e300) == limit);
        CHECK(answer_is_the_largest(psnr(limit)) == limit);
        CHECK(answer_is_the_largest(std::nextafter(psnr(limit), inf)) < limit);
        for (double t : {0.0, -0.0, 5e-324, -5e-324, 1.0, 20.0, 30.0, 35.5, 48.13, 60.0, 99.0, 150.0, 1e9}) answer_is_the_largest(t);
        for (int k = 0; k < 300; ++k) {                                      // the PSNR of an s: s itself comes back, or a larger s with the same PSNR
            const uint64_t s = k < 20 ? static_cast<uint64_t>(k) : k < 40 ? limit - (k - 20) : ((static_cast<uint64_t>(rng()) << 32) | rng()) % (limit + 1);
            const uint64_t got = answer_is_the_largest(psnr(s));
            CHECK(got >= s && psnr(got) == psnr(s));
        }
    }
}

int main() {
    std::mt19937 rng(20241020);
    for (int K : {1, 8, 32})
        for (long long tiles : {0LL, 1LL, 3LL, 4LL, 5LL, 65LL, 257LL})
            for (int kind : {0, 1, 2}) sweep_case(rng, tiles, K, kind);
    sweep_case(rng, 4099, 8, 0);
    sweep_case(rng, 400, 1, 1);                                              // a distortion total above 2^32
    pick_cases(rng);
    psnr_cases(rng);
    std::printf("asan_quality: %d cases\n", g_cases);
    std::printf("asan_quality: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
