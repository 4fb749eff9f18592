// asan_patch_index.cpp -- patch format version 2 under AddressSanitizer + UBSan (g++, no GPU, no HIP): `make asan-patch-index` /
// tests/test_asan_patch_index.py.  mpc::patch_make with an index section, mpc::patch_parse, mpc::patch_add_index and
// mpc::patch_strip_index (host_patch.cpp) on exact-size heap buffers (one byte read past an end is a report): valid patches of both
// versions, the hostile version-2 blobs of tests/patch_index_cases.py -- every prefix, index_bytes 0, off by one and far too large, the
// length one short and one long, version 2 on the empty form, version 1 with index_bytes set -- every single-bit flip of a version-2
// header, and each patch placed in memory so that its index section falls on each of the 8 byte alignments and is read there by the
// host's index reader (mpc::read_compressed_coded_by_index, what mpc_parse_container_by_index calls): the section is unaligned by
// nature, so a reader that loads words from it is an UBSan report here.
#include "../../imageexperiments_amd/csrc/host_bitstream.cpp"
#include "../../imageexperiments_amd/csrc/host_container.cpp"
#include "../../imageexperiments_amd/csrc/host_pool.cpp"
#include "../../imageexperiments_amd/csrc/host_delta.cpp"
#include "../../imageexperiments_amd/csrc/host_patch.cpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

// a container of width x height pixels with random counts and streams that match them: every kind of stream has symbols
static Blob random_container(std::mt19937& rng, int width, int height, int K) {
    const size_t tiles = static_cast<size_t>((width + 7) / 8) * ((height + 7) / 8);
    std::vector<double> quant(3 * static_cast<size_t>(K), 2.0);
    std::vector<uint16_t> counts(3 * tiles), symbols;
    for (uint16_t& v : counts) v = static_cast<uint16_t>(rng() % (K + 1));
    std::vector<unsigned long long> off(1, 0);
    for (int i = 0; i < 6 * K; ++i) {
        const int ch = (i / 2) / K, step = (i / 2) % K;
        uint16_t run = 0;
        size_t k = 0;
        for (size_t t = 0; t < tiles; ++t) {
            if (counts[3 * t + ch] <= step) continue;
            if (k++ % 37 == 0) run = static_cast<uint16_t>(rng() % 5);
            symbols.push_back(i % 3 == 0 ? static_cast<uint16_t>(rng() % 12) : i % 3 == 1 ? static_cast<uint16_t>(rng() % 3000) : run);
        }
        off.push_back(symbols.size());
    }
    size_t n = 0;
    uint8_t* made = mpc::encode_symbol_streams_malloc(width, height, K, 8, quant.data(), counts.data(), symbols.data(), off.data(), &n);
    Blob out(made, made + (made ? n : 0));
    std::free(made);
    return out;
}

// the parser on a heap copy of exactly the blob's size, `lead` bytes into an 8-byte aligned allocation
static std::string parse(const Blob& blob, mpc::PatchInfo* info, std::vector<int32_t>* list, size_t lead = 0, uint8_t** keep = nullptr) {
    uint8_t* base = static_cast<uint8_t*>(std::malloc(lead + (blob.size() ? blob.size() : 1)));
    uint8_t* exact = base + lead;
    if (!blob.empty()) std::memcpy(exact, blob.data(), blob.size());
    const std::string why = mpc::patch_parse(exact, blob.size(), info, list);
    if (why.empty()) {
        // what the parser accepts is what the writer writes for what it reports, index section included
        const uint8_t* index = info->index_bytes ? exact + info->index_offset : nullptr;
        CHECK(mpc::patch_make_error(info->width, info->height, info->key, list->data(), info->n, exact + info->container_offset, info->container_bytes,
                                    index, info->index_bytes)
                  .empty());
        const Blob again = mpc::patch_make(info->width, info->height, info->sequence, info->key, list->data(), info->n, exact + info->container_offset,
                                           info->container_bytes, index, info->index_bytes);
        CHECK(again.size() == blob.size() && std::memcmp(again.data(), exact, blob.size()) == 0);
        CHECK(info->container_offset + info->container_bytes + info->index_bytes == blob.size());
        CHECK(info->index_bytes == 0 ? info->index_offset == 0 : info->index_offset == info->container_offset + info->container_bytes);
        CHECK(static_cast<long long>(list->size()) == (info->key ? 0 : info->n));
        // strip and add on the same exact-size buffer
        const Blob bare = mpc::patch_strip_index(exact, *info);
        mpc::PatchInfo bi;
        std::vector<int32_t> bl;
        CHECK(mpc::patch_parse(bare.data(), bare.size(), &bi, &bl).empty() && bi.index_bytes == 0 && bl == *list && bi.n == info->n &&
              bi.container_bytes == info->container_bytes && bare.size() == blob.size() - info->index_bytes);
        CHECK(bare.size() >= mpc::kPatchHeaderBytes && bare[4] == 1 && std::memcmp(bare.data() + 32, exact + 32, bare.size() - 32) == 0);
    } else {
        CHECK(list->empty());
    }
    if (keep) *keep = base;
    else std::free(base);
    return why;
}

static void refused(const Blob& blob) {
    ++g_cases;
    mpc::PatchInfo info;
    std::vector<int32_t> list;
    CHECK(!parse(blob, &info, &list).empty());
}

static void put16(Blob& b, size_t at, unsigned v) {
    b[at] = static_cast<uint8_t>(v);
    b[at + 1] = static_cast<uint8_t>(v >> 8);
}
static void put32(Blob& b, size_t at, uint32_t v) {
    for (int i = 0; i < 4; ++i) b[at + i] = static_cast<uint8_t>(v >> (8 * i));
}

// one valid version-2 patch: refused under every single change, accepted -- and its index read -- at every alignment
static void drive(const Blob& v1, uint32_t interval, const Blob& empty) {
    mpc::PatchInfo p1, info;
    std::vector<int32_t> list1, list;
    ++g_cases;
    CHECK(parse(v1, &p1, &list1).empty() && p1.index_bytes == 0 && p1.n > 0);
    const Blob good = mpc::patch_add_index(v1.data(), p1, interval, 0);
    ++g_cases;
    CHECK(parse(good, &info, &list).empty() && info.index_bytes > 0 && good[4] == 2 && list == list1);
    if (info.index_bytes == 0) return;
    const Blob index(good.begin() + static_cast<long>(info.index_offset), good.end());
    {
        Blob built;
        CHECK(mpc::build_container_index(v1.data() + p1.container_offset, p1.container_bytes, interval, built) && built == index);
        // add is idempotent, replaces whatever index is there, and honours index_min_bytes on both sides of the boundary
        CHECK(mpc::patch_add_index(good.data(), info, interval, 0) == good);
        CHECK(mpc::patch_add_index(good.data(), info, interval, info.container_bytes) == good);
        CHECK(mpc::patch_add_index(good.data(), info, interval, info.container_bytes + 1) == v1);
        CHECK(mpc::patch_add_index(v1.data(), p1, interval, info.container_bytes + 1) == v1);
        CHECK(mpc::patch_strip_index(good.data(), info) == v1 && mpc::patch_strip_index(v1.data(), p1) == v1);
        const Blob junk = mpc::patch_make(p1.width, p1.height, p1.sequence, p1.key, list1.data(), p1.n, v1.data() + p1.container_offset,
                                          p1.container_bytes, reinterpret_cast<const uint8_t*>("junk"), 4);
        mpc::PatchInfo pj;
        std::vector<int32_t> lj;
        ++g_cases;
        CHECK(parse(junk, &pj, &lj).empty() && pj.index_bytes == 4 && mpc::patch_add_index(junk.data(), pj, interval, 0) == good);
        // a container that does not parse: the version-1 patch
        Blob broken = v1;
        for (size_t k = p1.container_offset + 24 + 6 * static_cast<size_t>(8); k < broken.size(); ++k) broken[k] = 0xff;
        if (mpc::patch_parse(broken.data(), broken.size(), &pj, &lj).empty()) {
            ++g_cases;
            CHECK(mpc::patch_add_index(broken.data(), pj, interval, 0) == broken);
        }
    }
    // every prefix
    for (size_t k = 0; k < good.size(); ++k) refused(Blob(good.begin(), good.begin() + static_cast<long>(k)));
    // index_bytes: 0, off by one, far too large; the length one short and one long; the versions
    Blob b = good;
    put32(b, 28, 0);
    refused(b);
    b.resize(info.index_offset);
    refused(b);                                                     // ... and the section gone: patch_cases's "wrong version"
    b = good, put32(b, 28, static_cast<uint32_t>(index.size() - 1));
    refused(b);
    b = good, put32(b, 28, static_cast<uint32_t>(index.size() + 1));
    refused(b);
    b = good, put32(b, 28, static_cast<uint32_t>(good.size() - mpc::kPatchHeaderBytes));
    refused(b);
    b = good, put32(b, 28, 0xffffffffu);
    refused(b);
    b = good, b.pop_back();
    refused(b);
    b = good, b.push_back(0);
    refused(b);
    b = good, put16(b, 4, 1);                                       // version 1 with index_bytes set
    refused(b);
    b = good, put16(b, 4, 3);
    refused(b);
    b = good, put16(b, 4, 0x0102);
    refused(b);
    // version 2 on the empty form
    b = empty, put16(b, 4, 2);
    refused(b);
    b = empty, put16(b, 4, 2), put32(b, 28, static_cast<uint32_t>(index.size())), b.insert(b.end(), index.begin(), index.end());
    refused(b);
    b = empty, put32(b, 28, static_cast<uint32_t>(index.size())), b.insert(b.end(), index.begin(), index.end());
    refused(b);
    // every single-bit flip of the header: refused, or accepted and then exactly what the writer writes
    int accepted = 0;
    for (size_t bit = 0; bit < 8 * mpc::kPatchHeaderBytes; ++bit) {
        ++g_cases;
        Blob flipped = good;
        flipped[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
        accepted += parse(flipped, &info, &list).empty();
    }
    CHECK(accepted >= 32);                                          // the 32 sequence bits at the least (a tile patch: a larger frame too)
    // the index section at each of the 8 alignments, read where it lies
    mpc::CodedStreams serial;
    CHECK(mpc::read_compressed_coded(v1.data() + p1.container_offset, p1.container_bytes, serial));
    unsigned seen = 0;
    for (size_t lead = 0; lead < 8; ++lead) {
        ++g_cases;
        uint8_t* base = nullptr;
        CHECK(parse(good, &info, &list, lead, &base).empty());
        const uint8_t* at = base + lead;
        seen |= 1u << (reinterpret_cast<uintptr_t>(at + info.index_offset) % 8);
        mpc::CodedStreams got;
        int route = -1;
        CHECK(mpc::read_compressed_coded_by_index(at + info.container_offset, info.container_bytes, at + info.index_offset, info.index_bytes, got,
                                                  &route));
        CHECK(route == 0 && got.lengths == serial.lengths && got.codes == serial.codes);
        mpc::ContainerIndex x;
        CHECK(mpc::read_container_index(at + info.index_offset, info.index_bytes, x) && !x.serial_only && x.nbytes == info.container_bytes);
        // a damaged section is read as safely, and costs the route only
        uint8_t* section = base + lead + info.index_offset;
        section[0] ^= 1;
        CHECK(mpc::read_compressed_coded_by_index(at + info.container_offset, info.container_bytes, section, info.index_bytes, got, &route) &&
              route == 1 && got.codes == serial.codes);
        section[0] ^= 1;
        section[info.index_bytes - 8] ^= 1;                         // the last checkpoint
        CHECK(mpc::read_compressed_coded_by_index(at + info.container_offset, info.container_bytes, section, info.index_bytes, got, &route) &&
              got.lengths == serial.lengths && got.codes == serial.codes);
        CHECK(mpc::read_compressed_coded_by_index(at + info.container_offset, info.container_bytes, section, 56, got, &route) && route == 1);
        std::free(base);
    }
    CHECK(seen == 0xffu);
}

int main() {
    std::mt19937 rng(20250);
    struct Shape {
        int width, height, K;
        std::vector<int32_t> tiles;
    };
    std::vector<Shape> shapes = {{83, 45, 8, {5, 40}}, {83, 45, 8, {0}}, {16, 16, 32, {1, 2, 3}}, {200, 136, 8, {}}};
    for (int32_t t = 0; t < 425; ++t)
        if (t != 212) shapes[3].tiles.push_back(t);                 // 424 of 425 tiles: seven packed columns
    for (int32_t i = 3; i < 425; i += 130) shapes.push_back({200, 136, 8, {i, i + 1, i + 31}});
    for (const Shape& s : shapes) {
        const long long all = mpc::patch_frame_tiles(s.width, s.height), n = static_cast<long long>(s.tiles.size());
        const mpc::PackGeometry g = mpc::pack_geometry(n, mpc::kDeltaPackRows);
        const Blob cont = random_container(rng, 8 * g.cols, 8 * g.rows, s.K), whole = random_container(rng, s.width, s.height, s.K);
        CHECK(!cont.empty() && !whole.empty());
        const Blob tile = mpc::patch_make(s.width, s.height, 9, false, s.tiles.data(), n, cont.data(), cont.size());
        const Blob key = mpc::patch_make(s.width, s.height, 9, true, nullptr, all, whole.data(), whole.size());
        const Blob empty = mpc::patch_make(s.width, s.height, 9, false, nullptr, 0, nullptr, 0);
        for (uint32_t interval : {32u, mpc::kIndexIntervalDefault}) {
            drive(tile, interval, empty);
            drive(key, interval, empty);
        }
        // the empty patch: add and strip leave it alone, and the writer takes no index for it
        mpc::PatchInfo pe;
        std::vector<int32_t> le;
        ++g_cases;
        CHECK(parse(empty, &pe, &le).empty() && mpc::patch_add_index(empty.data(), pe, 32, 0) == empty && mpc::patch_strip_index(empty.data(), pe) == empty);
        CHECK(!mpc::patch_make_error(s.width, s.height, false, nullptr, 0, nullptr, 0, cont.data(), 8).empty());
        CHECK(!mpc::patch_make_error(s.width, s.height, false, s.tiles.data(), n, cont.data(), cont.size(), nullptr, 8).empty());
        CHECK(!mpc::patch_make_error(s.width, s.height, false, s.tiles.data(), n, cont.data(), cont.size(), cont.data(), static_cast<size_t>(1) << 32).empty());
    }
    std::printf("asan_patch_index: %d cases\n", g_cases);
    std::printf("asan_patch_index: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
