// asan_encode_index2.cpp -- index version 2 as the encoder emits it, on the host under AddressSanitizer + UBSan (g++, no GPU, no
// HIP): `make asan-encode-index2` / tests/test_asan_encode_index2.py.  The by-plan route that computes the aux entries from the
// coded streams it holds, and index_from_plan, which checks them against the plans and writes the version-2 blob: on random
// streams made here and on the stream cases tests/test_asan_encode_index2.py writes to files.  Beside every sanitizer report the
// result itself is checked: the container is the direct route's, the index is build_container_index(..., expanded)'s of that
// container, and aux arrays that contradict the plans are refused.
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

struct Case {
    int W = 0, H = 0, K = 0;
    std::vector<double> quant;                      // [3K]
    std::vector<uint16_t> counts;                   // [3 * tiles]
    std::vector<unsigned long long> off;            // [6K + 1]
    std::vector<uint16_t> symbols;
};

// streams consistent with random counts; contents by kind: small alphabet, wide alphabet, runs (some of them long), wide geometric
static Case random_case(std::mt19937& rng, int W, int H, int K) {
    Case c;
    c.W = W; c.H = H; c.K = K;
    c.quant.assign(3 * static_cast<size_t>(K), 2.0);
    const size_t tiles = static_cast<size_t>((W + 7) / 8) * ((H + 7) / 8);
    c.counts.resize(3 * tiles);
    for (uint16_t& v : c.counts) v = static_cast<uint16_t>(rng() % (K + 1));
    c.off.assign(1, 0);
    for (int i = 0; i < 6 * K; ++i) {
        const int ch = (i / 2) / K, step = (i / 2) % K;
        size_t n = 0;
        for (size_t t = 0; t < tiles; ++t) n += c.counts[3 * t + ch] > step;
        std::geometric_distribution<int> wide(0.004);
        uint16_t run = 0;
        for (size_t k = 0; k < n; ++k) {
            uint16_t v;
            switch (i % 4) {
                case 0: v = static_cast<uint16_t>(rng() % 12); break;
                case 1: v = static_cast<uint16_t>(rng()); break;
                case 2: if (k % (i % 8 == 2 ? 37 : 2) == 0) run = static_cast<uint16_t>(rng() % (i % 8 == 2 ? 5 : 3)); v = run; break;
                default: v = static_cast<uint16_t>(std::min(wide(rng), 4000)); break;
            }
            c.symbols.push_back(v);
        }
        c.off.push_back(c.symbols.size());
    }
    return c;
}

static void drive(const Case& c, uint32_t interval) {
    // exact-size copies: one element read past an end is a report
    const std::vector<uint16_t> counts(c.counts.begin(), c.counts.end()), symbols(c.symbols.begin(), c.symbols.end());
    size_t n_direct = 0, n = 0, n1 = 0;
    uint8_t* direct = mpc::encode_symbol_streams_malloc(c.W, c.H, c.K, 8, c.quant.data(), counts.data(), symbols.data(), c.off.data(), &n_direct);
    std::vector<uint8_t> index, v1;
    uint8_t* mine = mpc::encode_symbol_streams_by_plan_indexed_malloc(c.W, c.H, c.K, 8, c.quant.data(), counts.data(), symbols.data(),
                                                                     c.off.data(), interval, &n, index, true);
    uint8_t* plain = mpc::encode_symbol_streams_by_plan_indexed_malloc(c.W, c.H, c.K, 8, c.quant.data(), counts.data(), symbols.data(),
                                                                      c.off.data(), interval, &n1, v1);
    CHECK(direct && mine && plain);
    if (direct && mine && plain) {
        CHECK(n == n_direct && std::memcmp(direct, mine, n) == 0);
        CHECK(n1 == n_direct && std::memcmp(direct, plain, n1) == 0);
        const std::vector<uint8_t> blob(mine, mine + n);
        std::vector<uint8_t> parsed, parsed1, extended;
        const bool consistent = mpc::streams_match_lengths(counts.data(), counts.size() / 3, c.K, c.off.data());
        if (!consistent) CHECK(index.empty() && v1.empty());
        else {
            CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, parsed, true));
            CHECK(!index.empty() && index == parsed);
            CHECK(mpc::build_container_index(blob.data(), blob.size(), interval, parsed1));
            CHECK(v1 == parsed1);                                   // without the flag: version 1 as before
            CHECK(mpc::extend_container_index(blob.data(), blob.size(), v1.data(), v1.size(), extended) && extended == index);
            mpc::ContainerIndex x;
            CHECK(mpc::read_container_index(index.data(), index.size(), x) && x.version == 2);
            // the emitted index is one the chunked parse accepts
            mpc::CodedStreams out;
            int route = -1;
            CHECK(mpc::read_compressed_coded_by_index(blob.data(), blob.size(), index.data(), index.size(), out, &route) && route == 0);
        }
    }
    std::free(direct);
    std::free(mine);
    std::free(plain);
}

// index_from_plan on aux arrays that contradict the plans: refused, nothing read beyond the arrays
static void contradict(const Case& c, uint32_t interval, std::mt19937& rng) {
    std::vector<mpc::StreamPlan> plans;
    std::vector<mpc::PlannedStream> planned;
    std::vector<uint64_t> cps, auxs;
    bool wide = false;
    size_t n = 0;
    uint8_t* blob = mpc::encode_by_plan(c.W, c.H, c.K, 8, c.quant.data(), c.counts.data(), c.symbols.data(), c.off.data(), interval, &n,
                                        plans, planned, cps, &wide, &auxs);
    CHECK(blob && !wide);
    std::free(blob);
    if (!blob || wide) return;
    const int S = 6 * c.K + 1;
    const size_t head_bits = mpc::container_head(c.W, c.H, c.K, 8, c.quant.data()).bit_size();
    std::vector<uint8_t> index;
    auto take = [&](const std::vector<uint64_t>& aux, size_t entries) {
        const std::vector<uint64_t> exact(aux.begin(), aux.end());  // its own allocation: a read past its end is a report
        const bool took = mpc::index_from_plan(interval, n, c.W, c.H, c.K, 8, head_bits, plans.data(), planned.data(), S, cps.data(), index,
                                               true, exact.data(), entries);
        CHECK(took == !index.empty());
        return took;
    };
    // which stream an entry belongs to, and its place in it
    std::vector<int> stream_of;
    std::vector<size_t> place_of;
    for (int j = 1; j < S; ++j) {
        if (!mpc::index_stream_has_aux(static_cast<size_t>(j), c.K, planned[static_cast<size_t>(j)].shorter)) continue;
        const size_t n_cp = static_cast<size_t>((planned[static_cast<size_t>(j)].eff_n + interval - 1) / interval);
        for (size_t k = 0; k < n_cp; ++k) { stream_of.push_back(j); place_of.push_back(k); }
    }
    const size_t entries = auxs.size() / 2;
    CHECK(stream_of.size() == entries);
    CHECK(take(auxs, entries));
    CHECK(mpc::index_from_plan(interval, n, c.W, c.H, c.K, 8, head_bits, plans.data(), planned.data(), S, cps.data(), index) && !index.empty());
    if (entries == 0) return;
    CHECK(!take(auxs, entries + 1));                                // not exactly the entries the plans imply
    CHECK(!take(std::vector<uint64_t>(auxs.begin(), auxs.end() - 2), entries - 1));
    CHECK(!take(std::vector<uint64_t>(), 0));
    for (int k = 0; k < 64; ++k) {
        std::vector<uint64_t> bad(auxs.begin(), auxs.end());
        const size_t at = rng() % entries;
        const int j = stream_of[at];
        const bool packed = planned[static_cast<size_t>(j)].shorter, first = place_of[at] == 0;
        const bool last = at + 1 == entries || stream_of[at + 1] != j;
        bool must_refuse = true;
        switch (k % 8) {
            case 0: bad[2 * at] += 1; must_refuse = first || !packed || (!last && bad[2 * at] >= bad[2 * at + 2]) ||
                                                    bad[2 * at] > planned[static_cast<size_t>(j)].n; break;
            case 1: bad[2 * at] = ~0ULL; break;                     // beyond the stream
            case 2: bad[2 * at] = first ? 1 : bad[2 * at - 2]; break;      // out[0] != 0; not strictly increasing
            case 3: bad[2 * at + 1] |= 3ULL << 32; break;           // a state that does not exist
            case 4: bad[2 * at + 1] |= 1ULL << (34 + rng() % 30); break;   // the unused bits
            case 5: bad[2 * at + 1] ^= 1ULL << 32; must_refuse = first || !packed || (bad[2 * at + 1] >> 32) > 2; break;
            case 6: bad[2 * at + 1] ^= 1ULL << (rng() % 16); must_refuse = first || !packed; break;      // prev: a hint unless it must be 0
            default: bad[2 * at + 1] ^= 1ULL << (16 + rng() % 16); must_refuse = first || (j - 1) % (2 * c.K) != 1; break;   // dc
        }
        const bool took = take(bad, entries);
        if (must_refuse) CHECK(!took);
    }
}

static bool load(const std::string& path, Case& c) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    uint32_t head[3];
    uint64_t n_counts = 0, n_symbols = 0;
    f.read(reinterpret_cast<char*>(head), sizeof(head));
    c.W = static_cast<int>(head[0]); c.H = static_cast<int>(head[1]); c.K = static_cast<int>(head[2]);
    if (!f || c.K < 1 || c.K > 32) return false;
    c.quant.resize(3 * static_cast<size_t>(c.K));
    f.read(reinterpret_cast<char*>(c.quant.data()), 8 * c.quant.size());
    f.read(reinterpret_cast<char*>(&n_counts), 8);
    if (!f || n_counts != 3 * static_cast<uint64_t>((c.W + 7) / 8) * ((c.H + 7) / 8)) return false;
    c.counts.resize(n_counts);
    f.read(reinterpret_cast<char*>(c.counts.data()), 2 * n_counts);
    c.off.resize(6 * static_cast<size_t>(c.K) + 1);
    f.read(reinterpret_cast<char*>(c.off.data()), 8 * c.off.size());
    f.read(reinterpret_cast<char*>(&n_symbols), 8);
    if (!f || n_symbols != c.off.back() || n_symbols > (1ull << 28)) return false;
    c.symbols.resize(n_symbols);
    f.read(reinterpret_cast<char*>(c.symbols.data()), 2 * n_symbols);
    return static_cast<bool>(f);
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250404);
    const int shapes[][3] = {{8, 8, 1}, {64, 40, 4}, {200, 120, 8}, {520, 264, 2}};
    for (const auto& s : shapes) {
        const Case c = random_case(rng, s[0], s[1], s[2]);
        for (uint32_t interval : {32u, 33u, 100u, 4097u, 65536u}) drive(c, interval);
        contradict(c, 33, rng);
        Case odd = c;                                               // one stream a symbol short of what the counts imply
        if (!odd.symbols.empty()) {
            odd.symbols.pop_back();
            for (size_t i = odd.off.size(); i-- > 0 && odd.off[i] > odd.symbols.size();) odd.off[i] = odd.symbols.size();
            drive(odd, 64);
        }
    }
    if (argc > 1) {                                                 // <dir>/<n>.case written by tests/test_asan_encode_index2.py
        int cases = 0;
        for (;; ++cases) {
            Case c;
            if (!load(std::string(argv[1]) + "/" + std::to_string(cases) + ".case", c)) break;
            for (uint32_t interval : {32u, 33u, 128u, 4097u}) drive(c, interval);
            contradict(c, 32, rng);
        }
        std::printf("asan_encode_index2: %d cases from files\n", cases);
    }
    std::printf("asan_encode_index2: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
