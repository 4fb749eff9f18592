// host_patch.h -- product: the delta stream's patch format, versions 1 and 2 (include/mpcodec.h, "patch"; DESIGN.md 4, "Delta stream").
// Knows neither HIP nor the C ABI and builds on its own (tests/cpp/asan_patch.cpp).  Little endian throughout:
//    0 "MPCP" | 4 u16 version = 1 | 6 u16 flags (bit 0 = key, the rest 0) | 8 u32 width | 12 u32 height | 16 u32 sequence |
//   20 u32 n | 24 u32 list_bytes | 28 u32 0 | 32 u64 container_bytes | 40 the list | the container
// The list: the gaps g0 = t0, gj = tj - t(j-1) - 1 of the ascending tile list, each LEB128 (7 bits a byte, low group first, at most
// 5 bytes, value below 2^31, no multi-byte value that ends in 0x00).  Three forms: key (n = tiles, no list, the whole frame's
// container), empty (n = 0, no list, no container), tile (0 < n < tiles, the container of the packed frame of 8C x 8R pixels with
// (R, C) = pack_geometry(n, kDeltaPackRows)).
// Version 2 is that layout with version = 2, the word at 28 = index_bytes (> 0) and, behind the container, index_bytes of the container's
// seek index (a version-1 "MPIX" blob, host_container.cpp): key and tile forms only, exactly 40 + list_bytes + container_bytes +
// index_bytes long.  Only the section's framing is checked here; what is in it is a hint for the decoder and may be anything.  It
// starts wherever list and container end: readers copy it or read it bytewise.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace mpc {

constexpr size_t kPatchHeaderBytes = 40;
constexpr unsigned kPatchVersion = 1, kPatchVersionIndexed = 2;

struct PatchInfo {
    int width = 0, height = 0;
    uint32_t sequence = 0;
    bool key = false;
    long long n = 0, tiles = 0;                 // tiles listed (a key patch: all of them), tiles of the frame
    size_t list_bytes = 0, container_offset = 0, container_bytes = 0;
    size_t index_offset = 0, index_bytes = 0;   // version 2: the index section; 0, 0 for version 1
};

// tiles of a width x height frame, 0 where the geometry is none a patch can carry (an extent < 1, 2^31 tiles or more)
long long patch_frame_tiles(long long width, long long height);

// The only writer.  The caller has checked: width, height >= 1 with patch_frame_tiles > 0; key: n == tiles of the frame (`tiles` is
// not read) and a container; else n == 0 and no container, or 0 < n < tiles of the frame, tiles[n] ascending, distinct, inside the
// frame, and a container.  The container's bytes are copied as they are.  index_bytes != 0 (only with a container, below 2^32):
// version 2 with those bytes as its index section, copied as they are; else version 1.
std::vector<uint8_t> patch_make(int width, int height, uint32_t sequence, bool key, const int32_t* tiles, long long n,
                                const uint8_t* container, size_t container_bytes, const uint8_t* index = nullptr, size_t index_bytes = 0);
// what patch_make's caller has to check: empty, or what is wrong
std::string patch_make_error(int width, int height, bool key, const int32_t* tiles, long long n, const uint8_t* container,
                             size_t container_bytes, const uint8_t* index = nullptr, size_t index_bytes = 0);

// Validates the patch whole: header, the three forms, the list (exactly n values in exactly list_bytes, the last tile inside the
// frame), the length, and the container's own header through container_info (a key patch: width x height, a tile patch: 8C x 8R).
// tiles_out (optional): the decoded list of a tile patch; empty for the other two forms (a key patch lists every tile by saying so).
// No more is allocated than the patch has list bytes.  Returns an empty string and fills *info, or says what is wrong; nothing is
// read outside [bytes, bytes + nbytes).
std::string patch_parse(const uint8_t* bytes, size_t nbytes, PatchInfo* info, std::vector<int32_t>* tiles_out);

// The version-1 patch of a patch patch_parse has accepted (`p` is its verdict): a version-1 patch's own bytes, a version-2 patch
// without its index section.
std::vector<uint8_t> patch_strip_index(const uint8_t* bytes, const PatchInfo& p);
// What a sender that attaches the index does, defined on the host: the stripped patch, and behind it -- where the patch has a container
// of at least max(index_min_bytes, 1) bytes and build_container_index(container, interval) gives an index that is not "serial only" --
// that index, as version 2.  interval: 0 = the default, else kIndexIntervalMin ... kIndexIntervalMax (the caller has checked).
std::vector<uint8_t> patch_add_index(const uint8_t* bytes, const PatchInfo& p, uint32_t interval, size_t index_min_bytes);

}  // namespace mpc
