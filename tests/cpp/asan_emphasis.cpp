// asan_emphasis.cpp -- the emphasis maps' host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-emphasis` /
// tests/test_asan_emphasis.py.  The four host definitions on exact-size heap buffers (one byte read past a map, a mask row or a list,
// or one written past an output, is a report): mpc::budget_allocate_emphasis against a loop written out here, mpc::budget_sweep_emphasis
// against it at all 256 multipliers, mpc::budget_allocate_floor_emphasis with lists whose entries lie outside the frame, and
// mpc::emphasis_from_mask on masks whose last row ends with the buffer; and all of them on hostile values: any u8 in the map, any u32 in
// the profile and the weights, any u16 in the counts, any i32 in the list.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"
#include "../../imageexperiments_amd/csrc/host_budget.cpp"
#include "../../imageexperiments_amd/csrc/host_rate.cpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
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

struct Inputs {
    std::vector<uint32_t> profile, weights;
    std::vector<uint16_t> counts;
};

// kind 0: inside the bounds; 1: at them (P_MAX, the upper clamp of the weights); 2: hostile
static Inputs inputs(std::mt19937& rng, long long tiles, int K, int kind) {
    const uint32_t p_max = 64u * 3u * 255u * 255u;
    Inputs in;
    in.profile.resize(static_cast<size_t>(tiles) * (K + 1));
    in.weights.resize(3 * static_cast<size_t>(K));
    in.counts.resize(3 * static_cast<size_t>(tiles));
    for (uint32_t& w : in.weights) w = kind == 2 ? static_cast<uint32_t>(rng()) : kind == 1 ? mpc::kBudgetWeightMax : mpc::kBudgetWeightMin + rng() % 20000;
    for (uint16_t& c : in.counts) c = static_cast<uint16_t>(kind == 2 ? rng() : rng() % (K + 2));
    for (uint32_t& p : in.profile) p = kind == 2 ? static_cast<uint32_t>(rng()) : kind == 1 ? p_max : rng() % (p_max + 1);
    return in;
}

static std::vector<uint8_t> map_of(std::mt19937& rng, long long tiles, int kind) {
    std::vector<uint8_t> e(static_cast<size_t>(tiles));
    for (uint8_t& v : e) v = static_cast<uint8_t>(kind == 0 ? 1 + rng() % 64 : kind == 1 ? 64 : rng());
    return e;
}

static void allocate_case(std::mt19937& rng, long long tiles, int K, int kind) {
    ++g_cases;
    const Inputs in = inputs(rng, tiles, K, kind);
    const std::vector<uint8_t> e = map_of(rng, tiles, kind);
    std::vector<uint64_t> sweep(kWords, 0xDEADBEEFDEADBEEFull);
    mpc::budget_sweep_emphasis(in.profile.data(), in.counts.data(), e.data(), tiles, K, in.weights.data(), sweep.data());
    for (int j = 0; j < mpc::kBudgetLambdas; ++j) {
        std::vector<uint8_t> depth(static_cast<size_t>(tiles));
        std::vector<uint16_t> cut(3 * static_cast<size_t>(tiles));
        uint64_t totals[3];
        mpc::budget_allocate_emphasis(in.profile.data(), in.counts.data(), e.data(), tiles, K, in.weights.data(), j, depth.data(), cut.data(), totals);
        CHECK(std::memcmp(totals, sweep.data() + 3 * j, sizeof(totals)) == 0);
        if (kind != 2 && j > 0) CHECK(sweep[3 * j] >= sweep[3 * (j - 1)] && sweep[3 * j + 1] <= sweep[3 * (j - 1) + 1]);
        if (j % 51 != 0) continue;
        // the definition, written out: the smallest n that minimises P * e * 4096 + L * R
        uint64_t true_sse = 0;
        for (long long t = 0; t < tiles; ++t) {
            const uint64_t factor = static_cast<uint64_t>(e[t] == 0 ? 1 : e[t] > 64 ? 64 : e[t]) * 4096;
            uint64_t best = 0;
            int at = 0;
            for (int n = 0; n <= K; ++n) {
                uint64_t rate = 0;
                for (int ch = 0; ch < 3; ++ch)
                    for (int i = 0; i < std::min<int>({n, in.counts[t * 3 + ch], K}); ++i) rate += in.weights[ch * K + i];
                const uint64_t J = in.profile[t * (K + 1) + n] * factor + mpc::budget_lambda(j) * rate;
                if (n == 0 || J < best) {
                    best = J;
                    at = n;
                }
            }
            if (kind != 2) CHECK(depth[t] == at);
            CHECK(depth[t] <= K);
            for (int ch = 0; ch < 3; ++ch) CHECK(cut[t * 3 + ch] == std::min<int>({depth[t], in.counts[t * 3 + ch], K}));
            true_sse += in.profile[t * (K + 1) + depth[t]];
        }
        CHECK(totals[0] == true_sse);                                          // unweighted
        if (kind != 2 && j == 255) CHECK(totals[1] == 0 && totals[2] == 0);    // the bound: nothing is kept at the last multiplier
    }
    // no map and the neutral map: the plain functions, bit for bit
    std::vector<uint64_t> plain(kWords), neutral(kWords), none(kWords);
    const std::vector<uint8_t> sixteen(static_cast<size_t>(tiles), 16);
    mpc::budget_sweep(in.profile.data(), in.counts.data(), tiles, K, in.weights.data(), plain.data());
    mpc::budget_sweep_emphasis(in.profile.data(), in.counts.data(), sixteen.data(), tiles, K, in.weights.data(), neutral.data());
    mpc::budget_sweep_emphasis(in.profile.data(), in.counts.data(), nullptr, tiles, K, in.weights.data(), none.data());
    CHECK(plain == neutral && plain == none);
}

static void floor_case(std::mt19937& rng, long long n, long long tiles, int K, int kind, bool listed) {
    ++g_cases;
    const Inputs in = inputs(rng, n, K, kind);
    const std::vector<uint8_t> e = map_of(rng, tiles, kind);
    std::vector<uint8_t> floor(static_cast<size_t>(n)), must(static_cast<size_t>(n));
    std::vector<int32_t> list(static_cast<size_t>(n));
    for (long long i = 0; i < n; ++i) {
        floor[i] = static_cast<uint8_t>(kind == 2 ? rng() : rng() % (K + 2));
        must[i] = static_cast<uint8_t>(rng() % 2);
        const int32_t outside[] = {-1, static_cast<int32_t>(tiles), 2147483647, -2147483647 - 1};
        list[i] = kind == 2 ? static_cast<int32_t>(rng()) : rng() % 5 == 0 ? outside[rng() % 4] : static_cast<int32_t>(rng() % tiles);
    }
    for (int j : {0, 1, 113, 200, 255}) {
        std::vector<uint8_t> depth(static_cast<size_t>(n)), send(static_cast<size_t>(n));
        std::vector<uint16_t> cut(3 * static_cast<size_t>(n));
        uint64_t totals[4];
        mpc::budget_allocate_floor_emphasis(in.profile.data(), in.counts.data(), floor.data(), must.data(), e.data(), listed ? list.data() : nullptr,
                                            tiles, n, K, in.weights.data(), j, depth.data(), cut.data(), send.data(), totals);
        uint64_t true_sse = 0, sent = 0;
        for (long long i = 0; i < n; ++i) {
            const int low = std::min<int>(floor[i], K);
            CHECK(depth[i] <= K && (must[i] || depth[i] >= low) && send[i] == (must[i] || depth[i] > low ? 1 : 0));
            true_sse += in.profile[i * (K + 1) + depth[i]];
            sent += send[i];
        }
        CHECK(totals[0] == true_sse && totals[3] == sent);
        // a neutral map, whatever the list: the plain function
        const std::vector<uint8_t> sixteen(static_cast<size_t>(tiles), 16);
        std::vector<uint8_t> d0(depth.size()), s0(send.size()), d1(depth.size()), s1(send.size());
        uint64_t t0[4], t1[4];
        mpc::budget_allocate_floor(in.profile.data(), in.counts.data(), floor.data(), must.data(), n, K, in.weights.data(), j, d0.data(), nullptr, s0.data(), t0);
        mpc::budget_allocate_floor_emphasis(in.profile.data(), in.counts.data(), floor.data(), must.data(), sixteen.data(), listed ? list.data() : nullptr,
                                            tiles, n, K, in.weights.data(), j, d1.data(), nullptr, s1.data(), t1);
        CHECK(d0 == d1 && s0 == s1 && std::memcmp(t0, t1, sizeof(t0)) == 0);
    }
}

static void mask_case(std::mt19937& rng, int width, int height, size_t stride, size_t offset, int lo, int hi) {
    ++g_cases;
    // exact size: the last row ends with its last pixel, not with its stride
    const size_t bytes = offset + static_cast<size_t>(height - 1) * stride + static_cast<size_t>(width);
    std::vector<uint8_t> buffer(bytes, 255);
    const uint8_t* mask = buffer.data() + offset;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) buffer[offset + y * stride + x] = static_cast<uint8_t>(rng() % 3 ? 0 : rng());
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    std::vector<uint8_t> e(static_cast<size_t>(tiles_x) * tiles_y, 0xEE);
    mpc::emphasis_from_mask(mask, width, height, stride, lo, hi, e.data());
    for (int tx = 0; tx < tiles_x; ++tx)
        for (int ty = 0; ty < tiles_y; ++ty) {
            int m = 0;
            for (int y = ty * 8; y < std::min(ty * 8 + 8, height); ++y)
                for (int x = tx * 8; x < std::min(tx * 8 + 8, width); ++x) m = std::max<int>(m, mask[y * stride + x]);
            CHECK(e[static_cast<size_t>(tx) * tiles_y + ty] == lo + ((hi - lo) * m + 127) / 255);
        }
}

int main() {
    std::mt19937 rng(20241021);
    for (int K : {1, 5, 32})
        for (long long tiles : {0LL, 1LL, 3LL, 4LL, 5LL, 17LL, 33LL})
            for (int kind : {0, 1, 2}) allocate_case(rng, tiles, K, kind);
    allocate_case(rng, 1025, 8, 0);
    for (int K : {1, 5, 32})
        for (long long n : {0LL, 1LL, 5LL, 33LL})
            for (int kind : {0, 1, 2}) {
                floor_case(rng, n, n + 7, K, kind, true);
                floor_case(rng, n, n + 1, K, kind, false);
            }
    for (int width : {1, 7, 8, 9, 197})
        for (int height : {1, 8, 117})
            for (size_t pad : {size_t{0}, size_t{13}})
                for (size_t offset : {size_t{0}, size_t{1}, size_t{3}}) mask_case(rng, width, height, width + pad, offset, 1 + (width + height) % 16, 64 - height % 8);
    mask_case(rng, 64, 48, 64, 0, 16, 16);
    mask_case(rng, 4928, 9, 4928, 1, 1, 64);
    std::printf("asan_emphasis: %d cases\n", g_cases);
    std::printf("asan_emphasis: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
