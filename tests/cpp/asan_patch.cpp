// asan_patch.cpp -- the delta stream's patch format under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-patch` /
// tests/test_asan_patch.py.  mpc::patch_make and mpc::patch_parse (host_patch.cpp, with the container header's reader it calls) on
// exact-size heap buffers (one byte read past an end is a report): valid patches of the three forms, the hostile corpus of
// tests/patch_cases.py -- every prefix, every header field, list_bytes and n off by one, varints too long, too large and with a
// trailing zero group, a tile outside the frame, the forms mixed up, trailing bytes, lengths beyond the blob -- and every single-bit
// flip of two valid patches' headers and lists.  Whatever the parser accepts must be what the writer writes for what it reports.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"
#include "../../imageexperiments_amd/csrc/host_delta.cpp"
#include "../../imageexperiments_amd/csrc/host_patch.cpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

typedef std::vector<uint8_t> Blob;

// a valid container of width x height pixels: every tile-channel of length 0 (K = 1 where the frame has millions of tiles)
static Blob blank_container(int width, int height) {
    const size_t tiles = static_cast<size_t>((width + 7) / 8) * ((height + 7) / 8);
    const int K = tiles > 100000 ? 1 : 8;
    std::vector<double> quant(3 * K, 1.0);
    std::vector<uint16_t> counts(3 * tiles, 0);
    std::vector<uint32_t> choices(3 * tiles * K, 0);
    size_t n = 0;
    uint8_t* made = mpc::encode_records_malloc(width, height, K, 8, quant.data(), counts.data(), choices.data(), &n);
    Blob out(made, made + (made ? n : 0));
    std::free(made);
    return out;
}

static Blob packed_container(long long n) {
    const mpc::PackGeometry g = mpc::pack_geometry(n, mpc::kDeltaPackRows);
    return blank_container(8 * g.cols, 8 * g.rows);
}

// the parser on a heap copy of exactly the blob's size; *info and *list as it leaves them
static std::string parse(const Blob& blob, mpc::PatchInfo* info, std::vector<int32_t>* list) {
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(blob.size() ? blob.size() : 1));
    if (!blob.empty()) std::memcpy(exact, blob.data(), blob.size());
    const std::string why = mpc::patch_parse(exact, blob.size(), info, list);
    if (why.empty()) {
        // what the parser accepts is what the writer writes for what it reports: the format has one spelling for everything
        CHECK(mpc::patch_make_error(info->width, info->height, info->key, list->data(), info->n, exact + info->container_offset, info->container_bytes).empty());
        const Blob again = mpc::patch_make(info->width, info->height, info->sequence, info->key, list->data(), info->n, exact + info->container_offset,
                                           info->container_bytes);
        CHECK(again.size() == blob.size() && std::memcmp(again.data(), exact, blob.size()) == 0);
        CHECK(info->container_offset + info->container_bytes == blob.size() && static_cast<long long>(list->size()) == (info->key ? 0 : info->n));
    } else {
        CHECK(list->empty());
    }
    std::free(exact);
    return why;
}

static void refused(const Blob& blob) {
    ++g_cases;
    mpc::PatchInfo info;
    std::vector<int32_t> list;
    CHECK(!parse(blob, &info, &list).empty());
}

static void put32(Blob& b, size_t at, uint32_t v) {
    for (int i = 0; i < 4; ++i) b[at + i] = static_cast<uint8_t>(v >> (8 * i));
}
static void put64(Blob& b, size_t at, uint64_t v) {
    for (int i = 0; i < 8; ++i) b[at + i] = static_cast<uint8_t>(v >> (8 * i));
}

// header fields of `from` changed, the list and the container replaced
static Blob rebuilt(const Blob& from, const Blob& list, const Blob& container, long long n, int flags, long long list_bytes = -1,
                    long long container_bytes = -1) {
    Blob out(from.begin(), from.begin() + mpc::kPatchHeaderBytes);
    out[6] = static_cast<uint8_t>(flags);
    out[7] = static_cast<uint8_t>(flags >> 8);
    put32(out, 20, static_cast<uint32_t>(n));
    put32(out, 24, static_cast<uint32_t>(list_bytes < 0 ? static_cast<long long>(list.size()) : list_bytes));
    put64(out, 32, container_bytes < 0 ? container.size() : static_cast<uint64_t>(container_bytes));
    out.insert(out.end(), list.begin(), list.end());
    out.insert(out.end(), container.begin(), container.end());
    return out;
}

static void corpus(int width, int height, const std::vector<int32_t>& tiles) {
    const long long all = mpc::patch_frame_tiles(width, height), n = static_cast<long long>(tiles.size());
    const Blob cont = packed_container(n), whole = blank_container(width, height), other = blank_container(8, 24);
    const Blob tile = mpc::patch_make(width, height, 9, false, tiles.data(), n, cont.data(), cont.size());
    const Blob key = mpc::patch_make(width, height, 9, true, nullptr, all, whole.data(), whole.size());
    const Blob empty = mpc::patch_make(width, height, 9, false, nullptr, 0, nullptr, 0);
    mpc::PatchInfo info;
    std::vector<int32_t> list;
    for (const Blob* good : {&tile, &key, &empty}) {
        ++g_cases;
        CHECK(parse(*good, &info, &list).empty());
    }
    CHECK(parse(tile, &info, &list).empty() && list == tiles && info.n == n && info.tiles == all && !info.key && info.sequence == 9);
    CHECK(parse(key, &info, &list).empty() && info.key && info.n == all && info.list_bytes == 0);
    CHECK(empty.size() == mpc::kPatchHeaderBytes);
    CHECK(parse(tile, &info, &list).empty());
    const Blob gaps(tile.begin() + mpc::kPatchHeaderBytes, tile.begin() + static_cast<long>(info.container_offset));
    // every prefix
    for (size_t k = 0; k < tile.size(); ++k) refused(Blob(tile.begin(), tile.begin() + static_cast<long>(k)));
    for (size_t k = 0; k <= mpc::kPatchHeaderBytes; ++k) refused(Blob(key.begin(), key.begin() + static_cast<long>(k)));
    refused(Blob(key.begin(), key.end() - 1));
    for (size_t k = 0; k < mpc::kPatchHeaderBytes; ++k) refused(Blob(empty.begin(), empty.begin() + static_cast<long>(k)));
    // the header's fields
    Blob b = tile;
    b[3] = 'Q';
    refused(b);
    b = tile, b[4] = 2;
    refused(b);
    b = tile, b[4] = 0;
    refused(b);
    refused(rebuilt(tile, gaps, cont, n, 2));
    refused(rebuilt(key, Blob(), whole, all, 0x8001));
    b = tile, b[28] = 1;
    refused(b);
    b = empty, put32(b, 8, 0);
    refused(b);
    b = empty, put32(b, 12, 0);
    refused(b);
    b = empty, put32(b, 8, 0x7fffffffu), put32(b, 12, 0x7fffffffu);
    refused(b);
    b = empty, put32(b, 8, 0xffffffffu);
    refused(b);
    // list_bytes and n one off, the blob's length kept or not
    const long long lb = static_cast<long long>(gaps.size()), cb = static_cast<long long>(cont.size());
    refused(rebuilt(tile, gaps, cont, n, 0, lb - 1));
    refused(rebuilt(tile, gaps, cont, n, 0, lb + 1));
    refused(rebuilt(tile, gaps, cont, n, 0, lb - 1, cb + 1));
    refused(rebuilt(tile, gaps, cont, n, 0, lb + 1, cb - 1));
    refused(rebuilt(tile, gaps, cont, n - 1, 0));
    refused(rebuilt(tile, gaps, cont, n + 1, 0));
    // varints: the first gap (below 128 in every corpus) spelled badly
    const uint8_t first = gaps[0];
    CHECK(first < 0x80);
    const Blob rest(gaps.begin() + 1, gaps.end());
    const auto with_first = [&](std::initializer_list<uint8_t> spelled) {
        Blob l(spelled);
        l.insert(l.end(), rest.begin(), rest.end());
        return rebuilt(tile, l, cont, n, 0);
    };
    refused(with_first({static_cast<uint8_t>(first | 0x80), 0x80, 0x80, 0x80, 0x80, 0x00}));      // six bytes
    refused(with_first({static_cast<uint8_t>(first | 0x80), 0x80, 0x80, 0x80, 0x80}));            // five, and no end
    refused(with_first({static_cast<uint8_t>(first | 0x80), 0x00}));                              // a trailing zero group
    refused(with_first({static_cast<uint8_t>(first | 0x80), 0x80, 0x00}));
    refused(with_first({0x80, 0x80, 0x80, 0x80, 0x08}));                                          // 2^31
    refused(with_first({0xff, 0xff, 0xff, 0xff, 0x7f}));                                          // 2^35 - 1
    refused(with_first({0xff, 0xff, 0xff, 0xff, 0x07}));                                          // 2^31 - 1: outside the frame
    {
        std::vector<int32_t> past = tiles;                                                         // the last tile = tiles
        past.back() = static_cast<int32_t>(all);
        Blob l;
        long long last = -1;
        for (int32_t t : past) {
            mpc::store_gap(l, static_cast<uint32_t>(t - last - 1));
            last = t;
        }
        refused(rebuilt(tile, l, cont, n, 0));
    }
    // the forms mixed up
    refused(rebuilt(key, gaps, whole, all, 1));                                                   // a key patch with a list
    refused(rebuilt(key, Blob(), whole, all - 1, 1));
    refused(rebuilt(empty, Blob(), cont, 0, 0));                                                  // an empty patch with a container
    refused(rebuilt(empty, Blob(1, 0), Blob(), 0, 0));                                            // ... with a list
    refused(rebuilt(tile, gaps, Blob(), n, 0));                                                   // a tile patch without a container
    refused(rebuilt(key, Blob(), whole, all, 0));                                                 // n == tiles without the key flag
    refused(rebuilt(key, Blob(static_cast<size_t>(all), 0), whole, all, 0));                       // ... with every tile listed
    // lengths
    b = tile, b.push_back(0);
    refused(b);
    b = empty, b.push_back(0);
    refused(b);
    refused(rebuilt(tile, gaps, cont, n, 0, -1, cb + 1));
    refused(rebuilt(tile, gaps, cont, n, 0, -1, static_cast<long long>(1ULL << 62)));
    b = tile, put64(b, 32, ~0ULL - mpc::kPatchHeaderBytes - gaps.size() + 1);                     // header + list + container wraps to 0
    refused(b);
    b = tile, put32(b, 24, 0xffffffffu);
    refused(b);
    // the container's own header
    refused(rebuilt(tile, gaps, Blob(cont.size(), 0xff), n, 0));
    refused(rebuilt(tile, gaps, other, n, 0));
    refused(rebuilt(key, Blob(), other, all, 1));
    // every single-bit flip of the header and the list: refused, or accepted and then exactly what the writer writes
    int accepted = 0;
    for (const Blob* valid : {&tile, &key}) {
        const size_t bits = 8 * (mpc::kPatchHeaderBytes + (valid == &tile ? gaps.size() : 0));
        for (size_t bit = 0; bit < bits; ++bit) {
            ++g_cases;
            Blob flipped = *valid;
            flipped[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
            accepted += parse(flipped, &info, &list).empty();
        }
    }
    CHECK(accepted >= 64);                                                                         // the 32 sequence bits of each, at the least
}

int main() {
    corpus(83, 45, {5, 40});
    corpus(200, 136, [] {
        std::vector<int32_t> t;
        for (int32_t i = 1; i < 425; i += 3) t.push_back(i);                                       // 142 tiles: three packed columns
        return t;
    }());
    corpus(16384, 16384, {0, 1, 129, 258, 16642, 33027, 2130180, 4194303});                        // gaps 0, 127, 128, 16383, 16384, 2097152
    std::printf("asan_patch: %d cases\n", g_cases);
    std::printf("asan_patch: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
