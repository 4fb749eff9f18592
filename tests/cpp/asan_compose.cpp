// asan_compose.cpp -- the compose's host code under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-compose` /
// tests/test_asan_compose.py.  mpc::compose_container -- the definition of what mpc_compose_indexed computes -- on what nobody vouches
// for: damaged containers as the base and as an overlay, part lists of every kind.  Beside every sanitizer report the rules are
// checked: a header that does not parse is "source N", whoever names it; a source that only parts without a tile name is not read; the
// verdict on a body is read_compressed's, then "a length above K", for the lowest owning part; the tile-aligned quadrants that
// transcode_container cut compose to what coding the source again gives.
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

using Blob = std::vector<uint8_t>;

static Blob random_container(std::mt19937& rng, int W, int H, int K, int bs) {
    const size_t tiles = static_cast<size_t>((W + bs - 1) / bs) * ((H + bs - 1) / bs);
    std::vector<uint16_t> counts(3 * tiles);
    std::vector<uint32_t> choices(3 * tiles * K, 0);
    for (size_t o = 0; o < 3 * tiles; ++o) {
        counts[o] = static_cast<uint16_t>(rng() % (K + 1));
        for (int i = 0; i < counts[o]; ++i)                         // few distinct ids in the chroma channels: run-length packed streams
            choices[o * K + i] = (rng() % (o % 3 == 0 ? 2500 : 3)) | ((rng() % (i == 0 ? 4000 : 60)) << 16);
    }
    std::vector<double> quant(3 * static_cast<size_t>(K), 7.0);
    size_t n = 0;
    uint8_t* b = mpc::encode_records_malloc(W, H, K, bs, quant.data(), counts.data(), choices.data(), &n);
    CHECK(b);
    const Blob blob(b, b + (b ? n : 0));
    std::free(b);
    return blob;
}

static mpc::ComposePart part(int source, int x, int y, int w, int h, int dx, int dy) {
    mpc::ComposePart p;
    p.source = source;
    p.x = x;
    p.y = y;
    p.w = w;
    p.h = h;
    p.dx = dx;
    p.dy = dy;
    return p;
}

// compose_container on exact-size copies (one byte read past an end is a report); its verdict, with the rules checked
static int compose(const std::vector<Blob>& sources, const std::vector<mpc::ComposePart>& parts, int width, int height, Blob& out) {
    const std::vector<Blob> copies(sources.begin(), sources.end());
    std::vector<const uint8_t*> bytes;
    std::vector<size_t> nbytes;
    for (const Blob& c : copies) {
        bytes.push_back(c.data());
        nbytes.push_back(c.size());
    }
    bytes.push_back(nullptr);                                       // never a null array, whatever n_sources is
    nbytes.push_back(0);
    const mpc::ComposePart none{};
    out.clear();
    std::string why;
    const int n_sources = static_cast<int>(copies.size()), n_parts = static_cast<int>(parts.size());
    const int verdict = mpc::compose_container(bytes.data(), nbytes.data(), n_sources, parts.empty() ? &none : parts.data(), n_parts, width,
                                               height, out, why);
    CHECK(verdict >= 0 && verdict <= 2 && (verdict == 0) == why.empty());
    if (verdict != 0) CHECK(out.empty());
    // a header that does not parse wins over everything but the arguments that need no container
    int first_bad_header = -1;
    for (int s = 0; s < n_sources && first_bad_header < 0; ++s) {
        int w, h, K, bs;
        if (!mpc::container_info(copies[s].data(), copies[s].size(), &w, &h, &K, &bs)) first_bad_header = s;
    }
    if (verdict == 1 && why.rfind("source ", 0) == 0) CHECK(first_bad_header >= 0 && why == "source " + std::to_string(first_bad_header) + ": Invalid input data");
    if (verdict == 0) CHECK(first_bad_header < 0);
    if (verdict == 1 && why.rfind("part ", 0) == 0) {
        // "part N: ...": N's source is what read_compressed refuses, or holds a length above K
        const int p = std::atoi(why.c_str() + 5);
        CHECK(p >= 0 && p < n_parts && parts[p].source >= 0 && parts[p].source < n_sources);
        if (p >= 0 && p < n_parts && parts[p].source >= 0 && parts[p].source < n_sources) {
            const Blob& x = copies[parts[p].source];
            mpc::Streams s;
            const bool readable = mpc::read_compressed(x.data(), x.size(), s);
            bool too_long = false;
            if (readable)
                for (uint16_t length : s.lengths) too_long = too_long || length > s.K;
            const std::string text = why.substr(why.find(": ") + 2);
            CHECK(readable ? too_long && text == "Invalid bitstream" : text == "Invalid input data");
        }
    }
    if (verdict == 0) {
        mpc::Streams made, first;
        CHECK(mpc::read_compressed(out.data(), out.size(), made));
        mpc::ComposePlan plan;
        std::string again;
        CHECK(mpc::compose_plan(bytes.data(), nbytes.data(), n_sources, parts.data(), n_parts, width, height, nullptr, plan, again) == 0);
        CHECK(made.width == width && made.height == height && made.K == plan.K && made.block_size == plan.block_size);
        CHECK(std::memcmp(made.quant, plan.sources[0].quant, sizeof(made.quant)) == 0);
        for (uint16_t length : made.lengths) CHECK(length <= made.K);
    }
    return verdict;
}

// the quadrant identity of one container: cut at a tile-aligned (cx, cy), composed again
static void quadrants(std::mt19937& rng, const Blob& x, bool encoders) {
    int width, height, K, bs;
    if (!mpc::container_info(x.data(), x.size(), &width, &height, &K, &bs)) return;
    Blob whole;
    if (mpc::transcode_container(x.data(), x.size(), 0, 0, width, height, 0, whole) != 0) return;
    if (encoders) CHECK(whole == x);
    const int tx = (width + bs - 1) / bs, ty = (height + bs - 1) / bs;
    if (tx < 2 || ty < 2) return;
    const int cx = bs * (1 + static_cast<int>(rng() % (tx - 1))), cy = bs * (1 + static_cast<int>(rng() % (ty - 1)));
    const int rects[4][4] = {{0, 0, cx, cy}, {cx, 0, width - cx, cy}, {0, cy, cx, height - cy}, {cx, cy, width - cx, height - cy}};
    std::vector<Blob> pieces(4);
    std::vector<mpc::ComposePart> parts;
    for (int k = 0; k < 4; ++k) {
        CHECK(mpc::transcode_container(x.data(), x.size(), rects[k][0], rects[k][1], rects[k][2], rects[k][3], 0, pieces[k]) == 0);
        parts.push_back(part(k, 0, 0, 0, 0, rects[k][0], rects[k][1]));
    }
    Blob got;
    CHECK(compose(pieces, parts, width, height, got) == 0);
    if (encoders) CHECK(got == whole);                              // sums that survive a second difference coding
    // and straight from the source: four rectangles of one container
    std::vector<mpc::ComposePart> direct;
    for (int k = 0; k < 4; ++k) direct.push_back(part(0, rects[k][0], rects[k][1], rects[k][2], rects[k][3], rects[k][0], rects[k][1]));
    std::shuffle(direct.begin(), direct.end(), rng);
    CHECK(compose({x}, direct, width, height, got) == 0 && got == whole);
}

static void drive(std::mt19937& rng, const Blob& blob, const Blob& other, int W, int H, int K, int bs, int flips) {
    const int tx = (W + bs - 1) / bs, ty = (H + bs - 1) / bs, lx = (tx - 1) * bs, ly = (ty - 1) * bs;
    Blob out;
    CHECK(compose({blob}, {part(0, 0, 0, 0, 0, 0, 0)}, W, H, out) == 0 && out == blob);
    // an overlay: the ragged corner tile stays the corner; the first tile anywhere
    CHECK(compose({blob, other}, {part(0, 0, 0, 0, 0, 0, 0), part(1, lx, ly, W - lx, H - ly, lx, ly)}, W, H, out) == 0);
    CHECK(compose({blob, other}, {part(0, 0, 0, 0, 0, 0, 0), part(1, 0, 0, std::min(bs, W), std::min(bs, H), 0, 0)}, W, H, out) == 0);
    // argument errors
    const std::vector<std::vector<mpc::ComposePart>> refused = {
        {part(0, 0, 0, 0, 0, 0, 0), part(0, 0, 0, std::min(bs, W), std::min(bs, H), 1, 0)},
        {part(0, 0, 0, 0, 0, 0, 0), part(0, 0, 0, std::min(bs, W), std::min(bs, H), 0, -bs)},
        {part(0, 0, 0, 0, 0, 0, 0), part(0, 0, 0, std::min(bs, W), std::min(bs, H), 2147483647 / bs * bs, 0)},
        {part(0, 0, 0, 0, 0, 0, 0), part(0, 0, 0, 2147483647, bs, 0, 0)},
        {part(0, 0, 0, 0, 0, 0, 0), part(1, 0, 0, 0, 0, 0, 0), part(2, 0, 0, 0, 0, 0, 0)},
        {part(0, 0, 0, 0, 0, 0, 0), part(-1, 0, 0, 8, 8, 0, 0)},
        {part(0, 0, 0, 0, 0, bs, 0)},
        {},
    };
    for (const auto& parts : refused) CHECK(compose({blob, other}, parts, W, H, out) == 2);
    CHECK(compose({blob}, {part(0, 0, 0, 0, 0, 0, 0)}, W + bs, H, out) == 2);           // uncovered, or a ragged edge inside
    CHECK(compose({blob}, {part(0, 0, 0, 0, 0, 0, 0)}, 0, H, out) == 2);
    CHECK(compose({}, {part(0, 0, 0, 0, 0, 0, 0)}, W, H, out) == 2);
    quadrants(rng, blob, true);
    for (int k = 0; k < flips; ++k) {                               // damaged containers
        Blob x = k % 2 ? other : blob;
        if (k % 8 == 7) x.resize(rng() % x.size());
        else {
            const size_t bit = rng() % (8 * (k % 4 == 0 ? std::min<size_t>(x.size(), 14 + 6 * static_cast<size_t>(K)) : x.size()));
            x[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        }
        const mpc::ComposePart corner = part(1, lx, ly, W - lx, H - ly, lx, ly);
        compose({x, blob}, {part(0, 0, 0, 0, 0, 0, 0), corner}, W, H, out);            // as the base
        compose({blob, x}, {part(0, 0, 0, 0, 0, 0, 0), corner}, W, H, out);            // as an overlay
        // named only by a part without a tile: its header decides alone
        const int verdict = compose({blob, x}, {part(1, 0, 0, 0, 0, 0, 0), part(0, 0, 0, 0, 0, 0, 0)}, W, H, out);
        mpc::ComposePlan plan;
        std::string why;
        const uint8_t* bytes[2] = {blob.data(), x.data()};
        const size_t nbytes[2] = {blob.size(), x.size()};
        const mpc::ComposePart two[2] = {part(1, 0, 0, 0, 0, 0, 0), part(0, 0, 0, 0, 0, 0, 0)};
        const int planned = mpc::compose_plan(bytes, nbytes, 2, two, 2, W, H, nullptr, plan, why);
        CHECK(verdict == planned);
        if (verdict == 0) CHECK(out == blob);
        quadrants(rng, x, false);
    }
}

int main(int argc, char** argv) {
    std::mt19937 rng(20261019);
    const int shapes[][4] = {{16, 16, 1, 8}, {64, 40, 4, 8}, {203, 117, 8, 8}, {120, 64, 32, 8}, {30, 22, 5, 4}, {13, 9, 3, 2}, {50, 33, 2, 7}};
    for (const auto& s : shapes)
        drive(rng, random_container(rng, s[0], s[1], s[2], s[3]), random_container(rng, s[0], s[1], s[2], s[3]), s[0], s[1], s[2], s[3], 24);
    if (argc > 1) {
        // written by tests/test_asan_compose.py: <dir>/<n>.case = "n_sources n_parts width height expect" and a line
        // "source x y w h dx dy" per part, expect -1 = whatever it is; the sources in <dir>/<n>.<s>.mn
        auto slurp = [](const std::string& path, Blob& out) {
            std::ifstream f(path, std::ios::binary);
            if (!f) return false;
            out.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            return true;
        };
        int cases = 0, made = 0;
        for (;; ++cases) {
            const std::string stem = std::string(argv[1]) + "/" + std::to_string(cases);
            std::ifstream cf(stem + ".case");
            int n_sources, n_parts, width, height, expect;
            if (!(cf >> n_sources >> n_parts >> width >> height >> expect) || n_sources < 0 || n_sources > 16 || n_parts < 0 || n_parts > 64) break;
            std::vector<Blob> sources(static_cast<size_t>(n_sources));
            std::vector<mpc::ComposePart> parts(static_cast<size_t>(n_parts));
            bool complete = true;
            for (int s = 0; s < n_sources; ++s) complete = complete && slurp(stem + "." + std::to_string(s) + ".mn", sources[s]);
            for (mpc::ComposePart& p : parts) complete = complete && static_cast<bool>(cf >> p.source >> p.x >> p.y >> p.w >> p.h >> p.dx >> p.dy);
            if (!complete) break;
            Blob out;
            const int verdict = compose(sources, parts, width, height, out);
            if (expect >= 0 && verdict != expect) {
                std::printf("FAILED case %d: verdict %d, expected %d\n", cases, verdict, expect);
                ++g_failed;
            }
            made += verdict == 0;
            if (n_sources > 0) quadrants(rng, sources[0], false);
        }
        std::printf("asan_compose: %d cases from files, %d composed\n", cases, made);
    }
    std::printf("asan_compose: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
