// host_patch.cpp -- product: the delta stream's patch format on the host: the one writer and the one parser (host_patch.h).
#include "host_patch.h"

#include <cstring>

#include "host_bitstream.h"
#include "host_delta.h"

namespace mpc {

namespace {

void store16(std::vector<uint8_t>& out, unsigned v) {
    out.push_back(static_cast<uint8_t>(v));
    out.push_back(static_cast<uint8_t>(v >> 8));
}
void store32(std::vector<uint8_t>& out, uint32_t v) {
    store16(out, v & 0xffffu);
    store16(out, v >> 16);
}
uint32_t load16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }
uint32_t load32(const uint8_t* p) { return load16(p) | load16(p + 2) << 16; }
uint64_t load64(const uint8_t* p) { return static_cast<uint64_t>(load32(p)) | static_cast<uint64_t>(load32(p + 4)) << 32; }

void store_gap(std::vector<uint8_t>& out, uint32_t v) {
    while (v >= 0x80u) {
        out.push_back(static_cast<uint8_t>(v | 0x80u));
        v >>= 7;
    }
    out.push_back(static_cast<uint8_t>(v));
}

}  // namespace

long long patch_frame_tiles(long long width, long long height) {
    if (width < 1 || height < 1 || width > 0x7fffffffLL || height > 0x7fffffffLL) return 0;
    const long long tiles = ((width + 7) / 8) * ((height + 7) / 8);
    return tiles < (1LL << 31) ? tiles : 0;
}

std::string patch_make_error(int width, int height, bool key, const int32_t* tiles, long long n, const uint8_t* container,
                             size_t container_bytes, const uint8_t* index, size_t index_bytes) {
    const long long all = patch_frame_tiles(width, height);
    if (all == 0) return "bad geometry";
    if (n < 0 || n > all) return "n outside 0 ... the frame's tiles";
    if (index_bytes != 0) {
        if (!index) return "no index";
        if (static_cast<uint64_t>(index_bytes) >= (1ULL << 32)) return "an index of 2^32 bytes or more";
        if (n == 0) return "an empty patch carries no index";
    }
    if (key) {
        if (n != all) return "a key patch lists every tile";
    } else if (n == all) {
        return "every tile listed: that is a key patch";
    }
    if (n == 0) return container_bytes != 0 ? "an empty patch carries no container" : "";
    if (!container || container_bytes == 0) return "no container";
    if (key) return "";
    if (!tiles) return "no tile list";
    long long last = -1;
    for (long long j = 0; j < n; ++j) {
        if (tiles[j] <= last || tiles[j] >= all) return "the tile list is not ascending inside the frame";
        last = tiles[j];
    }
    return "";
}

std::vector<uint8_t> patch_make(int width, int height, uint32_t sequence, bool key, const int32_t* tiles, long long n,
                                const uint8_t* container, size_t container_bytes, const uint8_t* index, size_t index_bytes) {
    std::vector<uint8_t> list;
    if (!key) {
        long long last = -1;
        for (long long j = 0; j < n; ++j) {
            store_gap(list, static_cast<uint32_t>(tiles[j] - last - 1));
            last = tiles[j];
        }
    }
    std::vector<uint8_t> out;
    out.reserve(kPatchHeaderBytes + list.size() + container_bytes + index_bytes);
    out.insert(out.end(), {'M', 'P', 'C', 'P'});
    store16(out, index_bytes ? kPatchVersionIndexed : kPatchVersion);
    store16(out, key ? 1u : 0u);
    store32(out, static_cast<uint32_t>(width));
    store32(out, static_cast<uint32_t>(height));
    store32(out, sequence);
    store32(out, static_cast<uint32_t>(n));
    store32(out, static_cast<uint32_t>(list.size()));
    store32(out, static_cast<uint32_t>(index_bytes));
    store32(out, static_cast<uint32_t>(static_cast<uint64_t>(container_bytes)));
    store32(out, static_cast<uint32_t>(static_cast<uint64_t>(container_bytes) >> 32));
    out.insert(out.end(), list.begin(), list.end());
    if (container_bytes) out.insert(out.end(), container, container + container_bytes);
    if (index_bytes) out.insert(out.end(), index, index + index_bytes);
    return out;
}

std::string patch_parse(const uint8_t* bytes, size_t nbytes, PatchInfo* info, std::vector<int32_t>* tiles_out) {
    if (tiles_out) tiles_out->clear();
    if (nbytes < kPatchHeaderBytes) return "shorter than a patch header";
    if (std::memcmp(bytes, "MPCP", 4) != 0) return "not a patch";
    const unsigned version = load16(bytes + 4);
    if (version != kPatchVersion && version != kPatchVersionIndexed) return "unknown patch version";
    const unsigned flags = load16(bytes + 6);
    if (flags & ~1u) return "reserved flag bits set";
    PatchInfo p;
    p.key = (flags & 1u) != 0;
    const uint32_t width = load32(bytes + 8), height = load32(bytes + 12), n = load32(bytes + 20), list_bytes = load32(bytes + 24);
    p.sequence = load32(bytes + 16);
    const uint32_t index_bytes = load32(bytes + 28);                // version 1: a reserved word
    if (version == kPatchVersion ? index_bytes != 0 : index_bytes == 0)
        return version == kPatchVersion ? "reserved word not zero" : "a version-2 patch without an index";
    const uint64_t container_bytes = load64(bytes + 32);
    p.tiles = patch_frame_tiles(width, height);
    if (p.tiles == 0) return "bad geometry";
    p.width = static_cast<int>(width);
    p.height = static_cast<int>(height);
    // the length, exactly: nothing below trusts list_bytes, container_bytes or index_bytes beyond it
    if (index_bytes > nbytes - kPatchHeaderBytes) return "the length is not header + list + container + index";
    const size_t body = nbytes - kPatchHeaderBytes - index_bytes;
    if (list_bytes > body || container_bytes != static_cast<uint64_t>(body - list_bytes))
        return index_bytes ? "the length is not header + list + container + index" : "the length is not header + list + container";
    p.n = n;
    p.list_bytes = list_bytes;
    p.container_offset = kPatchHeaderBytes + list_bytes;
    p.container_bytes = static_cast<size_t>(container_bytes);
    if (index_bytes) {
        p.index_offset = p.container_offset + p.container_bytes;
        p.index_bytes = index_bytes;
    }
    if (p.n > p.tiles) return "more tiles listed than the frame has";
    if (p.key) {
        if (p.n != p.tiles) return "a key patch lists every tile";
        if (list_bytes != 0) return "a key patch carries no list";
    } else if (p.n == p.tiles) {
        return "every tile listed without the key flag";
    } else if (p.n == 0) {
        if (index_bytes != 0) return "an empty patch carries no index";
        if (list_bytes != 0 || container_bytes != 0) return "an empty patch carries neither list nor container";
        *info = p;
        return "";
    }
    if (container_bytes == 0) return "no container";
    std::vector<int32_t> list;                                      // handed over only once everything has passed
    if (!p.key) {
        // exactly n values in exactly list_bytes; each at least one byte, so n is no more than the bytes that are there
        if (p.n > static_cast<long long>(list_bytes)) return "the list is shorter than its values";
        list.reserve(static_cast<size_t>(p.n));
        const uint8_t* at = bytes + kPatchHeaderBytes;
        const uint8_t* const end = at + list_bytes;
        long long tile = -1;
        for (long long j = 0; j < p.n; ++j) {
            uint64_t v = 0;
            int used = 0;
            for (;;) {
                if (at == end) return "the list ends inside a value";
                if (used == 5) return "a list value of more than 5 bytes";
                const uint8_t b = *at++;
                v |= static_cast<uint64_t>(b & 0x7fu) << (7 * used);
                ++used;
                if (!(b & 0x80u)) {
                    if (used > 1 && b == 0) return "a list value with a trailing zero group";
                    break;
                }
            }
            if (v >= (1ULL << 31)) return "a list value of 2^31 or more";
            tile += static_cast<long long>(v) + 1;
            if (tile >= p.tiles) return "a listed tile outside the frame";
            list.push_back(static_cast<int32_t>(tile));
        }
        if (at != end) return "the list is longer than its values";
    }
    int cw = 0, ch = 0, cK = 0, cbs = 0;
    const PackGeometry g = pack_geometry(p.n, kDeltaPackRows);
    const long long want_w = p.key ? p.width : 8LL * g.cols, want_h = p.key ? p.height : 8LL * g.rows;
    if (!container_info(bytes + p.container_offset, p.container_bytes, &cw, &ch, &cK, &cbs)) return "the container's header is invalid";
    if (cw != want_w || ch != want_h) return p.key ? "the container is not the frame's size" : "the container is not the packed frame's size";
    if (tiles_out) tiles_out->swap(list);
    *info = p;
    return "";
}

std::vector<uint8_t> patch_strip_index(const uint8_t* bytes, const PatchInfo& p) {
    std::vector<uint8_t> out(bytes, bytes + kPatchHeaderBytes + p.list_bytes + p.container_bytes);
    out[4] = static_cast<uint8_t>(kPatchVersion);                   // version 2 differs in these two words alone
    out[5] = 0;
    out[28] = out[29] = out[30] = out[31] = 0;
    return out;
}

std::vector<uint8_t> patch_add_index(const uint8_t* bytes, const PatchInfo& p, uint32_t interval, size_t index_min_bytes) {
    std::vector<uint8_t> out = patch_strip_index(bytes, p);
    if (p.n == 0 || p.container_bytes < (index_min_bytes ? index_min_bytes : 1)) return out;
    std::vector<uint8_t> index;
    // a container that does not parse has no index, and one whose index says "serial only" has no use for it
    if (!build_container_index(bytes + p.container_offset, p.container_bytes, interval, index) || index.size() < 16 || (index[12] & 1u) ||
        static_cast<uint64_t>(index.size()) >= (1ULL << 32))
        return out;
    out[4] = static_cast<uint8_t>(kPatchVersionIndexed);
    for (int k = 0; k < 4; ++k) out[28 + k] = static_cast<uint8_t>(index.size() >> (8 * k));
    out.insert(out.end(), index.begin(), index.end());
    return out;
}

}  // namespace mpc
