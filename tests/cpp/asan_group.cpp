// asan_group.cpp -- the group encodes' host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-group` /
// tests/test_asan_group.py.  mpc::budget_allocate_group and mpc::budget_sweep_group -- which define what the two group kernels compute --
// on exact-size heap buffers (one word read past the last frame's profile, weights or map, or one total written past frames * 3 or the
// 768, is a report) against the single-frame functions frame by frame; on hostile values too: counts above K, any u32 in the profile and
// the weights, any byte in the map; and mpc::sse_for_psnr over mpc::psnr_from_sse_pixels against its neighbours and against one frame's.
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

// kind 0: a profile and weights inside their bounds, counts up to K + 1, every frame's weights an octave apart; 1: the bounds themselves;
// 2: hostile -- any u32 in the profile and the weights, any u16 in the counts, any byte in the map
static void group_case(std::mt19937& rng, int frames, long long tiles, int K, int kind, bool with_map) {
    ++g_cases;
    const uint32_t p_max = 64u * 3u * 255u * 255u;
    const size_t all = static_cast<size_t>(frames) * static_cast<size_t>(tiles);
    std::vector<uint32_t> profile(all * (K + 1)), weights(static_cast<size_t>(frames) * 3 * K);
    std::vector<uint16_t> counts(3 * all);
    std::vector<uint8_t> map(with_map ? all : 0);
    for (int f = 0; f < frames; ++f)
        for (int i = 0; i < 3 * K; ++i)
            weights[static_cast<size_t>(f) * 3 * K + i] = kind == 2   ? static_cast<uint32_t>(rng())
                                                          : kind == 1 ? mpc::kBudgetWeightMax
                                                                      : std::min<uint32_t>(mpc::kBudgetWeightMax, (mpc::kBudgetWeightMin + rng() % 20000) << (f % 6));
    for (uint16_t& c : counts) c = static_cast<uint16_t>(kind == 2 ? rng() : rng() % (K + 2));
    for (uint8_t& e : map) e = static_cast<uint8_t>(kind == 0 ? 1 + rng() % 64 : rng());
    for (size_t g = 0; g < all; ++g) {
        int deepest = 0;
        for (int ch = 0; ch < 3; ++ch) deepest = std::max<int>(deepest, std::min<int>(counts[g * 3 + ch], K));
        uint32_t v = kind == 1 ? p_max : 1000 + rng() % 12000000;
        for (int n = 0; n <= K; ++n) {
            if (n >= 1 && n <= deepest) v = rng() % 4 == 0 ? std::min<uint32_t>(p_max, v + rng() % 3000) : v - rng() % (v / 2 + 1);   // not monotone
            profile[g * (K + 1) + n] = kind == 2 ? static_cast<uint32_t>(rng()) : v;
        }
    }
    const uint8_t* e = with_map ? map.data() : nullptr;
    // the sweep: exact size, the function zeroes it itself; against the frames' own sweeps added up
    std::vector<uint64_t> swept(kWords, 0xDEADBEEFDEADBEEFull), sum(kWords, 0), one(kWords);
    mpc::budget_sweep_group(profile.data(), counts.data(), e, frames, tiles, K, weights.data(), swept.data());
    for (int f = 0; f < frames; ++f) {
        const size_t first = static_cast<size_t>(f) * static_cast<size_t>(tiles);
        mpc::budget_sweep_emphasis(profile.data() + first * (K + 1), counts.data() + first * 3, e ? e + first : nullptr, tiles, K,
                                   weights.data() + static_cast<size_t>(f) * 3 * K, one.data());
        for (int w = 0; w < kWords; ++w) sum[w] += one[w];
    }
    CHECK(swept == sum);
    // the allocation at a few multipliers: depth, cut counts and the frames' totals against the single-frame function; null outputs
    for (int j : {0, 1, 77, 130, 200, 255}) {
        std::vector<uint8_t> depth(all, 0xEE);
        std::vector<uint16_t> cut(3 * all, 0xEEEE);
        std::vector<uint64_t> totals(3 * static_cast<size_t>(frames), 0xDEADBEEFDEADBEEFull), bare(3 * static_cast<size_t>(frames), 1);
        mpc::budget_allocate_group(profile.data(), counts.data(), e, frames, tiles, K, weights.data(), j, depth.data(), cut.data(), totals.data());
        mpc::budget_allocate_group(profile.data(), counts.data(), e, frames, tiles, K, weights.data(), j, nullptr, nullptr, bare.data());
        CHECK(bare == totals);
        uint64_t across[3] = {0, 0, 0};
        for (int f = 0; f < frames; ++f) {
            const size_t first = static_cast<size_t>(f) * static_cast<size_t>(tiles);
            std::vector<uint8_t> d1(static_cast<size_t>(tiles));
            std::vector<uint16_t> c1(3 * static_cast<size_t>(tiles));
            uint64_t t1[3];
            mpc::budget_allocate_emphasis(profile.data() + first * (K + 1), counts.data() + first * 3, e ? e + first : nullptr, tiles, K,
                                          weights.data() + static_cast<size_t>(f) * 3 * K, j, d1.data(), c1.data(), t1);
            CHECK(std::equal(d1.begin(), d1.end(), depth.begin() + first));
            CHECK(std::equal(c1.begin(), c1.end(), cut.begin() + 3 * first));
            CHECK(std::memcmp(t1, totals.data() + 3 * f, sizeof(t1)) == 0);
            for (int k = 0; k < 3; ++k) across[k] += t1[k];
        }
        CHECK(std::memcmp(across, swept.data() + 3 * j, sizeof(across)) == 0);
        for (size_t g = 0; g < all; ++g) CHECK(depth[g] <= K && cut[3 * g] <= K && cut[3 * g + 1] <= K && cut[3 * g + 2] <= K);
    }
    if (kind != 2) {
        for (int j = 1; j < mpc::kBudgetLambdas; ++j) CHECK(swept[3 * j] >= swept[3 * (j - 1)] && swept[3 * j + 1] <= swept[3 * (j - 1) + 1]);
        CHECK(swept[3 * 255 + 1] == 0 && swept[3 * 255 + 2] == 0);
    }
}

static void psnr_cases(std::mt19937& rng) {
    const double inf = std::numeric_limits<double>::infinity();
    const int geometries[][2] = {{1, 1}, {64, 48}, {197, 117}, {1920, 1080}, {7680, 4320}};
    for (const auto& g : geometries)
        for (int frames : {1, 2, 9, 64}) {
            const int W = g[0], H = g[1];
            const size_t pixels = static_cast<size_t>(W) * static_cast<size_t>(H) * static_cast<size_t>(frames);
            const uint64_t tiles = static_cast<uint64_t>((W + 7) / 8) * static_cast<uint64_t>((H + 7) / 8), limit = uint64_t{195075} * 64 * tiles * frames;
            auto psnr = [&](uint64_t s) { return mpc::psnr_from_sse_pixels(static_cast<double>(s), pixels); };
            CHECK(psnr(0) == inf);
            auto answer_is_the_largest = [&](double target) {
                ++g_cases;
                const uint64_t s = mpc::sse_for_psnr(target, limit, psnr);
                CHECK(s <= limit && psnr(s) >= target);
                if (s < limit) CHECK(psnr(s + 1) < target);
                if (frames == 1)                                             // one frame: the single-frame function's answer
                    CHECK(s == mpc::sse_for_psnr(target, limit, [&](uint64_t v) { return mpc::psnr_from_sse(static_cast<double>(v), W, H); }));
                return s;
            };
            CHECK(answer_is_the_largest(inf) == 0);
            CHECK(answer_is_the_largest(-1e300) == limit);
            CHECK(answer_is_the_largest(psnr(limit)) == limit);
            for (double t : {0.0, -0.0, 5e-324, 1.0, 20.0, 30.0, 35.5, 48.13, 60.0, 99.0, 150.0, 1e9}) answer_is_the_largest(t);
            for (int k = 0; k < 60; ++k) {
                const uint64_t s = k < 10 ? static_cast<uint64_t>(k) : k < 20 ? limit - (k - 10) : ((static_cast<uint64_t>(rng()) << 32) | rng()) % (limit + 1);
                const uint64_t got = answer_is_the_largest(psnr(s));
                CHECK(got >= s && psnr(got) == psnr(s));
            }
        }
}

int main() {
    std::mt19937 rng(20241021);
    for (int K : {1, 8, 32})
        for (int frames : {1, 2, 3, 9, 64})
            for (long long tiles : {0LL, 1LL, 3LL, 17LL, 33LL})
                for (int kind : {0, 1, 2}) group_case(rng, frames, tiles, K, kind, (frames + tiles + kind) % 2 == 0);
    group_case(rng, 5, 1031, 8, 0, true);
    group_case(rng, 2, 400, 1, 1, false);                                    // a distortion total above 2^32
    psnr_cases(rng);
    std::printf("asan_group: %d cases\n", g_cases);
    std::printf("asan_group: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
